"""Speed of the 768-wide, 12-head family (small.en, distil-small.en), HIP events, warm-up
then three repeats of everything; one JSON document on stdout (and --out FILE).

Per model, seeded synthetic weights (seed 0), 64 x 30 s clips (seeds 3000 + i):
  encoder   ms per 64-window batch, achieved TFLOP/s (algorithmic FLOPs: stem + 24 T d^2 and
            4 T^2 d per layer) and its fraction of the dense fp16 MFMA peak;
  decoder   greedy, 64 rows, max_length 128, no early-exit polling: us per position and
            launches per position (janus_whisper_decode_info);
  sampled   320 rows = 64 windows x best_of 5 at T = 0.6, max_length 64, the rows of a window
            sharing its encoder output (enc_index): gathered (one encoder copy per row, this
            family's default) against read in place in blocks of two and of four rows
            (DEC_PATH_XROWS(2) / (4)): us per position, the three alternating in one process
            (same box).
Usage (GPU box):  python tools/small_family_bench.py [--models small.en,distil-small.en]
                  [--parts encoder,decoder,sampled] [--label NAME] [--out FILE]
--label names the run in the document (e.g. an A/B library selected with JANUS_LIB)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from janus_amd.whisper import CONFIGS, WhisperEngine, dec_path_xrows  # noqa: E402
from janus_amd.workload import synth_speech  # noqa: E402

MFMA_F16_PEAK_TFLOPS = 2500.0   # dense fp16 MFMA, MI355X
REPEATS = 3


def encoder_flops(cfg, B):
    d, T, L = cfg.d_model, cfg.n_audio_ctx, cfg.enc_layers
    stem = 2 * 3 * (2 * T) * 80 * d + 2 * 3 * T * d * d
    return B * (stem + L * 24 * T * d * d + L * 4 * T * T * d)


def timed(fn):
    """ms of fn() on the current stream (events around it, synchronised)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(xs):
    return {"runs": [round(x, 2) for x in xs], "median": round(float(np.median(xs)), 2),
            "min": round(min(xs), 2), "max": round(max(xs), 2)}


def run_model(name, parts, B=64, windows=64, best_of=5):
    dev = torch.device("cuda", 0)
    cfg = CONFIGS[name]
    eng = WhisperEngine(cfg, seed=0)
    utts = [synth_speech(3000 + i, 30.0) for i in range(B)]
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    mel = eng.logmel(pcm, offs, B, 3)
    enc = eng.encode(mel)          # warm-up (weights prepared, workspaces allocated)
    torch.cuda.synchronize()
    res = {"model": name, "d_model": cfg.d_model, "heads": cfg.n_heads, "enc_layers": cfg.enc_layers,
           "dec_layers": cfg.dec_layers}
    if "encoder" in parts:
        ms = [timed(lambda: eng.encode(mel))[0] for _ in range(REPEATS)]
        fl = encoder_flops(cfg, B)
        tf = fl / (float(np.median(ms)) * 1e-3) / 1e12
        res["encoder"] = {"batch": B, "seconds": 30.0, "ms": spread(ms), "flops": float(fl),
                          "achieved_tflops": round(tf, 1), "bound": "mfma",
                          "frac_of_mfma_peak": round(tf / MFMA_F16_PEAK_TFLOPS, 4)}
    if "decoder" in parts:
        L = 128
        run = lambda: eng.decode_ex(enc, max_length=L, check_every=0)  # noqa: E731
        run()
        torch.cuda.synchronize()
        ms = [timed(run)[0] for _ in range(REPEATS)]
        pos, lau = eng.decode_info()
        res["decoder"] = {"rows": B, "max_length": L, "positions": pos, "ms": spread(ms),
                          "us_per_position": spread([1e3 * m / pos for m in ms]),
                          "launches_per_position": round(lau / pos, 2), "path": vars(eng.decode_path())}
    if "sampled" in parts:
        L, T = 64, 0.6
        ei = [j for j in range(windows) for _ in range(best_of)]
        seeds = [7000 + 13 * i for i in range(len(ei))]
        out = {}
        runs = {"gather": 0, "rows2": dec_path_xrows(2), "rows4": dec_path_xrows(4)}
        mk = lambda f: (lambda: eng.decode_ex(enc[:windows], max_length=L, temperature=T, seeds=seeds,  # noqa: E731
                                              enc_index=ei, check_every=0, path_flags=f))
        paths = {}
        for k, f in runs.items():   # warm-up: graphs captured, buffers allocated
            mk(f)()
            torch.cuda.synchronize()
            paths[k] = eng.decode_path().enc_rows
        ms = {k: [] for k in runs}
        for _ in range(REPEATS):    # alternating, same process, same box
            for k, f in runs.items():
                ms[k].append(timed(mk(f))[0])
        pos, _ = eng.decode_info()
        for k in runs:
            out[k] = {"enc_rows": paths[k], "ms": spread(ms[k]),
                      "us_per_position": spread([1e3 * m / pos for m in ms[k]])}
        out.update(rows=len(ei), windows=windows, best_of=best_of, temperature=T, max_length=L, positions=pos)
        res["sampled_320"] = out
    del eng
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="small.en,distil-small.en")
    ap.add_argument("--parts", default="encoder,decoder,sampled")
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    doc = {"label": a.label, "lib": os.environ.get("JANUS_LIB", "libjanus_hip.so"),
           "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0),
           "models": [run_model(m, a.parts.split(",")) for m in a.models.split(",")]}
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
