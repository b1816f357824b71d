"""Word alignment (WhisperEngine.align) beside the decode it follows: one JSON
document on stdout and in --out (default profiles/word_align.json).

base.en, seeded synthetic weights, 64 windows of random encoder rows, about 60 random text
tokens per window (55 .. 65), full 30 s windows (F = 1500):
  align          one align call over the 64 windows (host plan, uploads, decoder forward, reduce,
                 DTW, the copies back to the host);
  greedy_64      one greedy decode of the same 64 windows, max_length 64 (63 positions: the
                 tokens the alignment then runs over), check_every 0;
  forward / reduce / dtw   janus_whisper_align's phases 1 / 2 / 4 alone, each over what the
                 whole call left in the workspace.
Each: a host clock around one call that ends in a device synchronise (align returns host
arrays), warmed, ROUNDS alternating rounds in one process, medians.
  accuracy       max |A_gpu - A_ref| and max |p_gpu / p_ref - 1| of tests/test_align_gpu.py's
                 cases against tests/align_ref.py (the figures behind that file's bounds).

Usage (GPU box):  python tools/align_bench.py [--out FILE] [--windows N] [--no-accuracy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = "base.en"
ROUNDS = 5
TEXT = (55, 65)
MAXLEN = 64


def accuracy():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_align_gpu as t
    out = {}
    for model in t.CASES:
        _, _, wins = t.reference(model)
        rows = []
        for w, a in zip(wins, t.aligned(model)):
            rows.append({"N": int(w["A"].shape[0]), "F": int(w["A"].shape[1]),
                         "max_abs_dA": float(np.abs(a.attention - w["A"]).max()),
                         "max_rel_dp": float(np.abs(a.token_probs / w["p"] - 1).max()),
                         "A_ref_std": float(w["A"].std())})
        out[model] = rows
    out["max_abs_dA"] = max(r["max_abs_dA"] for m in t.CASES for r in out[m])
    out["max_rel_dp"] = max(r["max_rel_dp"] for m in t.CASES for r in out[m])
    out["bounds"] = {"ALIGN_E_A": t.ALIGN_E_A, "ALIGN_E_P_REL": t.ALIGN_E_P_REL}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_align.json"))
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--no-accuracy", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights
    cfg = CONFIGS[MODEL]
    dev = torch.device("cuda", 0)
    eng = WhisperEngine(cfg, synthetic_weights(cfg, seed=0))
    g = torch.Generator().manual_seed(1)
    enc = (torch.randn(a.windows, cfg.n_audio_ctx, cfg.d_model, generator=g) * 0.5).half().to(dev)
    rng = np.random.default_rng(2)
    texts = [[int(t) for t in rng.integers(256, 50000, int(rng.integers(TEXT[0], TEXT[1] + 1)))]
             for _ in range(a.windows)]
    sizes = [3000] * a.windows
    runs = {
        "align": lambda: eng.align(enc, texts, sizes),
        "greedy_64": lambda: eng.decode_ex(enc, max_length=MAXLEN, check_every=0),
        "forward": lambda: eng.align(enc, texts, sizes, phases=1),
        "reduce": lambda: eng.align(enc, texts, sizes, phases=2),
        "dtw": lambda: eng.align(enc, texts, sizes, phases=4),
    }
    times = {k: [] for k in runs}
    for f in runs.values():   # warm every shape
        f()
        torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, f in runs.items():
            if k != "align":
                runs["align"]()          # the phases run over a whole call's workspace
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    runs["greedy_64"]()
    torch.cuda.synchronize()
    positions = eng.decode_info()[0]
    doc = {"device": torch.cuda.get_device_name(0), "model": MODEL, "windows": a.windows,
           "text_tokens": [min(map(len, texts)), max(map(len, texts))], "rows": sum(len(t) + 3 for t in texts),
           "frames": 1500, "alignment_heads": len(eng.alignment_heads), "rounds": ROUNDS,
           "greedy_positions": positions, "ms": {}}
    for k in runs:
        doc["ms"][k] = {"calls": [round(t, 2) for t in times[k]], "median": round(float(np.median(times[k])), 2)}
    m = {k: doc["ms"][k]["median"] for k in runs}
    doc["align_over_greedy"] = round(m["align"] / m["greedy_64"], 3)
    parts = m["forward"] + m["reduce"] + m["dtw"]
    doc["split"] = {k: round(m[k] / parts, 3) for k in ("forward", "reduce", "dtw")}
    doc["accuracy"] = None if a.no_accuracy else accuracy()
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
