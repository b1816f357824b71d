"""Cost of the history rules (repetition_penalty, no_repeat_ngram_size): the same
decode with the rules (p = 1.2, n = 3) and without, alternating in one process on one device,
HIP events, warm-up then three repeats; one JSON document on stdout (and --out FILE, by default
profiles/decode_options.json). No target is set: the ratio against the same library's plain
call is what is reported.

base.en, seeded synthetic weights (seed 0), random encoder rows:
  greedy_64    64 rows at T = 0, max_length 128, no early-exit polling: us per position;
  sampled_320  320 rows = 64 windows x best_of 5 at T = 0.6 sharing their encoder rows,
               max_length 64: us per position.
Usage (GPU box):  python tools/decode_options_bench.py [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights  # noqa: E402

REPEATS = 3
RULES = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"runs": [round(x, 2) for x in xs], "min": round(min(xs), 2), "max": round(max(xs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_options.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = CONFIGS["base.en"]
    eng = WhisperEngine(cfg, synthetic_weights(cfg, seed=0))
    windows, best_of = 64, 5
    g = torch.Generator().manual_seed(0)
    enc = (torch.randn(windows, cfg.n_audio_ctx, cfg.d_model, generator=g) * 0.5).half().to(dev)
    ei = [j for j in range(windows) for _ in range(best_of)]
    seeds = [7000 + 13 * i for i in range(len(ei))]
    forms = {
        "greedy_64": dict(rows=windows, max_length=128, temperature=0.0,
                          run=lambda kw: eng.decode_ex(enc, max_length=128, check_every=0, **kw)),
        "sampled_320": dict(rows=len(ei), max_length=64, temperature=0.6, windows=windows, best_of=best_of,
                            run=lambda kw: eng.decode_ex(enc, max_length=64, temperature=0.6, seeds=seeds,
                                                         enc_index=ei, check_every=0, **kw)),
    }
    doc = {"model": "base.en", "repeats": REPEATS, "device": torch.cuda.get_device_name(0), "rules": RULES}
    for key, form in forms.items():
        run = form.pop("run")
        variants = {"plain": {}, "rules": RULES}
        info = {}
        for name, kw in variants.items():     # warm-up: graphs captured, buffers allocated
            run(kw)
            torch.cuda.synchronize()
            pos, lau = eng.decode_info()
            info[name] = dict(positions=pos, launches_per_position=round(lau / pos, 2))
        ms = {name: [] for name in variants}
        for _ in range(REPEATS):              # alternating, same process, same device
            for name, kw in variants.items():
                ms[name].append(timed(lambda: run(kw)))
        us = {name: [1e3 * m / info[name]["positions"] for m in ms[name]] for name in variants}
        doc[key] = dict(form, variants={name: dict(info[name], us_per_position=spread(us[name])) for name in variants},
                        ratio_rules_over_plain={"min": round(min(us["rules"]) / max(us["plain"]), 4),
                                                "max": round(max(us["rules"]) / min(us["plain"]), 4),
                                                "median": round(float(np.median(us["rules"]) / np.median(us["plain"])), 4)})
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
