"""Batched long-form transcription (services/batched.py) against the seek loop on
one long recording: one JSON document on stdout and in --out (default
profiles/longform_batched.json).

base.en with seeded synthetic weights; one seeded 600 s recording of synthetic speech bursts
(4 .. 14 s, over a noise floor) separated by pauses of zeros (0.5 .. 2 s); the speech gate is the
model's own (silero weights when JANUS_VAD_DIR has them, the energy stand-in otherwise). Timed,
alternating in one process after a warm-up of each, REPEATS times, with a host clock around calls
that end in a device synchronise:

* ``BatchedInferencePipeline(model).transcribe(audio)`` (the default: chunks from the gate, no
  timestamps, greedy), and
* ``model.transcribe(audio, vad_filter=True, temperature=0)``, the sequential call this
  change leaves untouched,

both at the same ``max_length``. Seeded weights never emit <|endoftext|>, so BOTH sides decode
every window to max_length: the ratio is that of the two call shapes, not of real speech (where
the seek loop also teacher-forces its previous text). Also 64 x 30 s through
generate_segments_batched (one chunk per file, one round), beside generate_segments over the
same files. Reported with the times: rounds, rows per round, decoder positions stepped
(janus_whisper_decode_info after every decode call of an untimed pass) and the host share
(gate rule, chunking, text) of the batched call.

Usage (GPU box):  python tools/longform_batched_bench.py [--out FILE] [--max-length N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
SECONDS = 600


def recording(seconds=SECONDS, seed=7000):
    """Seeded bursts of synthetic speech over a 0.02 rms noise floor, pauses of zeros between."""
    from janus_amd.workload import synth_speech
    rng = np.random.default_rng(seed)
    n = seconds * 16000
    out = np.zeros(n, np.float32)
    at, k = 0, 0
    while at < n:
        burst = float(rng.uniform(4.0, 14.0))
        b = synth_speech(seed + k, burst, sr=16000)[:n - at]
        out[at:at + len(b)] = b + 0.02 * rng.standard_normal(len(b)).astype(np.float32)
        at += len(b) + int(float(rng.uniform(0.5, 2.0)) * 16000)
        k += 1
    return out


def spread(v):
    return {"calls": [round(t, 1) for t in v], "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longform_batched.json"))
    ap.add_argument("--max-length", type=int, default=448)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from janus_amd.services import batched as bt
    from janus_amd.services import transcriber as tr
    from janus_amd.workload import synth_speech
    ML = a.max_length
    model = tr.WhisperModel("base.en")
    eng = model.engine
    pipe = bt.BatchedInferencePipeline(model)
    audio = recording()
    doc = {"device": torch.cuda.get_device_name(0), "model": "base.en (seeded synthetic weights)",
           "max_length": ML, "repeats": REPEATS, "gate": "silero" if model._vad() is not None else "energy stand-in",
           "note": "seeded weights never emit <|endoftext|>: both sides decode every window to max_length"}

    def positions_of(call):
        """Run ``call`` once with every decode call's positions (decode_info) and rows recorded."""
        seen, orig = [], eng.decode_ex

        def wrapped(*p, **k):
            out = orig(*p, **k)
            torch.cuda.synchronize()
            seen.append({"rows": int(out.n_tokens.shape[0]), "positions": eng.decode_info()[0]})
            return out
        eng.decode_ex = wrapped
        try:
            res = call()
        finally:
            del eng.decode_ex
        return res, seen

    def batched():
        segs, info = pipe.transcribe(audio, max_length=ML)
        segs = list(segs)
        torch.cuda.synchronize()
        return segs, info

    def sequential():
        segs, info = model.transcribe(audio, vad_filter=True, temperature=0, max_length=ML)
        segs = list(segs)
        torch.cuda.synchronize()
        return segs, info

    runs = {"batched": batched, "sequential": sequential}
    shape = {}
    for k, f in runs.items():           # warm-up, and what each call does
        (segs, info), seen = positions_of(f)
        shape[k] = {"decode_calls": len(seen), "rows_per_call": [s["rows"] for s in seen],
                    "positions": sum(s["positions"] for s in seen), "segments": len(segs),
                    "duration_after_vad_s": round(info.duration_after_vad, 2)}
    times = {k: [] for k in runs}
    for _ in range(REPEATS):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    stats = {}
    t0 = time.perf_counter()
    bt.generate_segments_batched(eng, [audio], max_length=ML, vad=model._vad(), stats=stats)
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    host = {k: round(stats[k] * 1e3, 2) for k in ("vad_rule", "chunking", "text")}
    doc["file_600s"] = {
        "audio_s": SECONDS, "ms": {k: spread(v) for k, v in times.items()}, "calls": shape,
        "rounds": stats["rounds"],
        "sequential_over_batched": [round(min(times["sequential"]) / max(times["batched"]), 1),
                                    round(max(times["sequential"]) / min(times["batched"]), 1)],
        "ms_per_audio_second": {k: [round(min(v) / SECONDS, 3), round(max(v) / SECONDS, 3)] for k, v in times.items()},
        "host_ms_of_one_batched_call": dict(host, call=round(total, 1),
                                           share=round(sum(host.values()) / total, 4))}
    print("file_600s", json.dumps(doc["file_600s"]), flush=True)

    # 64 x 30 s: one chunk per file, one round of 64 rows
    files = [np.ascontiguousarray(synth_speech(1000 + i, 30.0, sr=16000)) for i in range(64)]

    def pooled():
        r = bt.generate_segments_batched(eng, files, max_length=ML, vad_filter=False)
        torch.cuda.synchronize()
        return r

    def seek_loop():
        r = tr.generate_segments(eng, files, max_length=ML, temperatures=(0.0,))
        torch.cuda.synchronize()
        return r

    runs = {"generate_segments_batched": pooled, "generate_segments": seek_loop}
    shape = {}
    for k, f in runs.items():
        _, seen = positions_of(f)
        shape[k] = {"decode_calls": len(seen), "rows_per_call": [s["rows"] for s in seen],
                    "positions": sum(s["positions"] for s in seen)}
    times = {k: [] for k in runs}
    for _ in range(REPEATS):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    doc["files_64x30s"] = {"audio_s": 64 * 30, "ms": {k: spread(v) for k, v in times.items()}, "calls": shape,
                           "ms_per_audio_second": {k: [round(min(v) / 1920, 3), round(max(v) / 1920, 3)]
                                                   for k, v in times.items()}}
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
