"""Whole-file speech gate (janus_vad_probs, csrc/vad_file.hip) against the
streaming kernel (janus_vad_run, csrc/vad.hip) over the same zero-padded chunks: one JSON
document on stdout and in --out (default profiles/vad_file.json).

Shapes: 1 x 30 s, 1 x 600 s and 64 x 30 s of 16 kHz synthetic speech, seeded silero-shaped
weights. Each timing is a host clock around one call that ends in a device synchronise, audio
and outputs already on the device; every shape is warmed, then ROUNDS rounds alternate the two
paths in one process (medians, and the spread of each). The two paths' probabilities are compared
at every shape. For scale, WhisperModel("base.en").transcribe of the same audio (seeded
synthetic weights, T = 0 only; generate_segments for the 64 utterances), timed twice.

Usage (GPU box):  python tools/vad_file_bench.py [--out FILE] [--no-transcribe]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
SHAPES = (("1x30s", 1, 30), ("1x600s", 1, 600), ("64x30s", 64, 30))


def clips(n_streams, seconds):
    """n_streams utterances of `seconds` s at 16 kHz, each a run of different 30 s clips."""
    from janus_amd.workload import synth_speech
    out = []
    for s in range(n_streams):
        parts = [np.ascontiguousarray(synth_speech(1000 + 100 * s + k, 30.0)[::3]) for k in range(seconds // 30)]
        out.append(np.concatenate(parts).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_file.json"))
    ap.add_argument("--no-transcribe", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from janus_amd import _native as nat
    from janus_amd.services import transcriber as tr
    from janus_amd.services.vad import SileroGate, synthetic_weights
    dev = torch.device("cuda", 0)
    gate = SileroGate(synthetic_weights(seed=4))
    doc = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shapes": {}}
    model = None if a.no_transcribe else tr.WhisperModel("base.en")
    for name, S, seconds in SHAPES:
        auds = clips(S, seconds)
        L = len(auds[0])
        n = L // 512 + 1
        offs = np.arange(S + 1, dtype=np.int64) * L
        flat = torch.from_numpy(np.concatenate(auds + [np.zeros(1, np.float32)])).to(dev)
        pad = np.zeros((S, n * 512), np.float32)
        for s, x in enumerate(auds):
            pad[s, :L] = x
        chunks = torch.from_numpy(pad.reshape(S, n, 512)).to(dev)
        prob = torch.empty(S * n, dtype=torch.float32, device=dev)
        state = gate.new_state(S)
        got = {}

        def file_path():
            nat.call("janus_vad_probs", gate._h, flat.data_ptr(), offs.ctypes.data, S, 0, prob.data_ptr(),
                     nat.stream_ptr(dev))
            torch.cuda.synchronize()
            got["file"] = prob

        def stream_path():
            for t in state:
                t.zero_()
            got["stream"] = gate.run(chunks, state, 1)
            torch.cuda.synchronize()

        runs = {"janus_vad_probs": file_path, "janus_vad_run": stream_path}
        for f in runs.values():
            f()
        diff = float((got["file"].reshape(S, n) - got["stream"]).abs().max())
        times = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, f in runs.items():
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e3)
        row = {"streams": S, "seconds": seconds, "chunks_per_stream": n, "max_abs_diff_between_paths": diff,
               "ms": {k: {"calls": [round(t, 3) for t in v], "median": round(float(np.median(v)), 3),
                          "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}}
        row["stream_over_file"] = round(row["ms"]["janus_vad_run"]["median"] / row["ms"]["janus_vad_probs"]["median"], 1)
        row["faster_beyond_spread"] = row["ms"]["janus_vad_probs"]["max"] < row["ms"]["janus_vad_run"]["min"]
        if model is not None:
            tt = []
            for _ in range(3):   # the first call warms
                t0 = time.perf_counter()
                if S == 1:
                    list(model.transcribe(auds[0], temperature=(0.0,))[0])
                else:
                    tr.generate_segments(model.engine, auds, temperatures=(0.0,))
                torch.cuda.synchronize()
                tt.append((time.perf_counter() - t0) * 1e3)
            row["transcribe_base_en_ms"] = [round(t, 1) for t in tt[1:]]
        doc["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
