"""Speed of the 1024-wide, 16-head family (medium.en, distil-medium.en), HIP events, warm-up
then three repeats; one JSON document on stdout (and --out FILE, by default
profiles/medium_family_decode.json).

Seeded synthetic weights (seed 0): medium.en's (24 + 24 layers), and for distil-medium.en the
same tensors without decoder layers 2 .. 23 (the two share the 24-layer encoder, as the
checkpoints do), so the host generates the 0.3 G encoder parameters once. 64 x 30 s windows
(8 clips, seeds 3000 .. 3007, repeated). --models distil-medium.en leaves the 24-layer decoder
out (its 0.4 G parameters are then not generated).
  encoder   ms per 64-window batch (the first model's engine; the encoders are the same),
            achieved TFLOP/s over the algorithmic FLOPs (stem + 24 T d^2 and 4 T^2 d per layer);
  decoder   greedy, 64 rows, max_length 128, no early-exit polling: us per position and
            launches per position (janus_whisper_decode_info);
  sampled   320 rows = 64 windows x best_of 5 at T = 0.6, max_length 64, the rows of a window
            sharing its encoder output through a gathered copy per row (the only form at 16
            heads): us per position.
The decoder figures of the two models alternate in one process (same box), three repeats.
Usage (GPU box):  python tools/medium_family_bench.py [--models a,b] [--parts encoder,decoder,sampled] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights  # noqa: E402
from janus_amd.workload import synth_speech  # noqa: E402

MFMA_F16_PEAK_TFLOPS = 2500.0   # dense fp16 MFMA, MI355X
REPEATS = 3
MODELS = ("medium.en", "distil-medium.en")


def encoder_flops(cfg, B):
    d, T, L = cfg.d_model, cfg.n_audio_ctx, cfg.enc_layers
    stem = 2 * 3 * (2 * T) * cfg.n_mels * d + 2 * 3 * T * d * d
    return B * (stem + L * 24 * T * d * d + L * 4 * T * T * d)


def timed(fn):
    """ms of fn() on the current stream (events around it, synchronised)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"runs": [round(x, 2) for x in xs], "median": round(float(np.median(xs)), 2),
            "min": round(min(xs), 2), "max": round(max(xs), 2)}


def engines(names):
    full, distil = CONFIGS[MODELS[0]], CONFIGS[MODELS[1]]
    W = synthetic_weights(full if MODELS[0] in names else distil, seed=0)
    drop = tuple(f"decoder.layers.{i}." for i in range(distil.dec_layers, full.dec_layers))
    Wd = {k: v for k, v in W.items() if not k.startswith(drop)}
    return {n: WhisperEngine(CONFIGS[n], W if n == MODELS[0] else Wd) for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="encoder,decoder,sampled")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "medium_family_decode.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    names = [n for n in MODELS if n in a.models.split(",")]
    assert names, f"--models: some of {MODELS}"
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    B, windows, best_of = 64, 64, 5
    eng = engines(names)
    clips = [synth_speech(3000 + i, 30.0) for i in range(8)]
    utts = [clips[i % 8] for i in range(B)]
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    first = eng[names[0]]
    mel = first.logmel(pcm, offs, B, 3)
    enc = first.encode(mel)          # warm-up (weights prepared, workspaces allocated)
    torch.cuda.synchronize()
    doc = {"repeats": REPEATS, "device": torch.cuda.get_device_name(0), "windows": B, "seconds": 30.0,
           "models": {n: {"d_model": e.cfg.d_model, "heads": e.cfg.n_heads, "n_mels": e.cfg.n_mels,
                          "enc_layers": e.cfg.enc_layers, "dec_layers": e.cfg.dec_layers}
                      for n, e in eng.items()}}
    if "encoder" in parts:
        ms = [timed(lambda: first.encode(mel)) for _ in range(REPEATS)]
        fl = encoder_flops(first.cfg, B)
        tf = fl / (float(np.median(ms)) * 1e-3) / 1e12
        doc["encoder"] = {"model": names[0], "batch": B, "ms": spread(ms), "flops": float(fl),
                          "achieved_tflops": round(tf, 1),
                          "frac_of_mfma_peak": round(tf / MFMA_F16_PEAK_TFLOPS, 4)}
    ei = [j for j in range(windows) for _ in range(best_of)]
    seeds = [7000 + 13 * i for i in range(len(ei))]
    forms = {}
    if "decoder" in parts:
        forms["greedy_64"] = dict(rows=B, max_length=128, temperature=0.0,
                                  run=lambda e: e.decode_ex(enc, max_length=128, check_every=0))
    if "sampled" in parts:
        forms["sampled_320"] = dict(rows=len(ei), max_length=64, temperature=0.6, windows=windows, best_of=best_of,
                                    run=lambda e: e.decode_ex(enc, max_length=64, temperature=0.6, seeds=seeds,
                                                              enc_index=ei, check_every=0))
    for key, form in forms.items():
        run = form.pop("run")
        info = {}
        for n, e in eng.items():          # warm-up: graphs captured, buffers allocated
            run(e)
            torch.cuda.synchronize()
            pos, lau = e.decode_info()
            info[n] = dict(positions=pos, launches_per_position=round(lau / pos, 2), path=vars(e.decode_path()))
        ms = {n: [] for n in eng}
        for _ in range(REPEATS):          # the models alternating, same process, same box
            for n, e in eng.items():
                ms[n].append(timed(lambda: run(e)))
        doc[key] = dict(form, models={n: dict(info[n], ms=spread(ms[n]),
                                              us_per_position=spread([1e3 * m / info[n]["positions"] for m in ms[n]]))
                                      for n in eng})
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
