"""The int8 decoder weights (WhisperEngine(cfg, decoder_compute="int8")) against
the float16 ones, each with the float16 and the int8 cross-attention operand: decoder speed,
launches per position and what the mode costs in tokens. HIP events, warm-up then three
repeats; one JSON document on stdout and in --out (by default profiles/decoder_int8.json,
rewritten after every model).

Seeded synthetic weights (seed 0). The decoder alone: every model's config without its encoder
layers, on a seeded unit-normal encoder output (as a LayerNorm output is). The four combinations
(decoder weights x cross operand) alternate on ONE engine in one process (set_decoder_compute /
set_cross_compute), three repeats, min - max.
  greedy    64 rows, max_length 64 (63 positions), no early-exit polling: us per position;
  sampled   320 rows = 64 windows x best_of 5 at T = 0.6, max_length 32 (31 positions), the rows of
            a window sharing its encoder output: us per position.
Tokens: per leg the share of (row, position) pairs whose token equals the float16 / float16
run's, and the share of rows equal throughout (not asserted anywhere: synthetic weights decide
near ties everywhere).
Below d_model 768 the int8 weights also give up the d <= 512 fusions (LayerNorm prologues, the
embedding's LayerNorm, the fused merge + value projection): the float16 figure beside them is
the default path's, and launches_per_position shows the difference.
Usage (GPU box):  python tools/decoder_int8_bench.py [--models a,b] [--legs greedy,sampled] [--out FILE]"""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights  # noqa: E402

REPEATS = 3
MODELS = ("base.en", "small.en", "distil-medium.en", "medium.en", "large-v3-turbo")
COMBOS = [("float16", "float16"), ("int8", "float16"), ("float16", "int8"), ("int8", "int8")]   # (weights, cross)


def key(c):
    return f"weights_{c[0]}_cross_{c[1]}"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"runs": [round(x, 2) for x in xs], "min": round(min(xs), 2), "max": round(max(xs), 2)}


def weight_bytes(cfg):
    """Derived from the shapes: bytes of weights one position reads per row group (fp16; int8: half)."""
    d, H, V = cfg.d_model, cfg.n_heads, cfg.n_vocab
    return {"layers_fp16_mb": round(cfg.dec_layers * (14 + H) * d * d * 2 / 1e6, 1),
            "vocabulary_fp16_mb": round(V * d * 2 / 1e6, 1)}


def bench(name, legs, dev):
    cfg = dataclasses.replace(CONFIGS[name], enc_layers=0)
    eng = WhisperEngine(cfg, synthetic_weights(cfg, seed=0))
    B, windows, best_of = 64, 64, 5
    g = torch.Generator().manual_seed(17)
    enc = torch.randn(B, cfg.n_audio_ctx, cfg.d_model, generator=g).half().to(dev)
    ei = [j for j in range(windows) for _ in range(best_of)]
    seeds = [7000 + 13 * i for i in range(len(ei))]
    forms = {}
    if "greedy" in legs:
        forms["greedy_64"] = lambda: eng.decode_ex(enc, max_length=64, check_every=0)
    if "sampled" in legs:
        forms["sampled_320"] = lambda: eng.decode_ex(enc, max_length=32, temperature=0.6, seeds=seeds,
                                                     enc_index=ei, check_every=0)

    def mode(c):
        eng.set_decoder_compute(c[0])
        eng.set_cross_compute(c[1])

    out = {"d_model": cfg.d_model, "heads": cfg.n_heads, "dec_layers": cfg.dec_layers, "derived": weight_bytes(cfg)}
    for leg, run in forms.items():
        info, toks = {}, {}
        for c in COMBOS:                      # warm-up: int8 copies made, graphs captured, buffers allocated
            mode(c)
            o = run()
            torch.cuda.synchronize()
            pos, lau = eng.decode_info()
            info[c] = dict(positions=pos, launches_per_position=round(lau / pos, 2),
                           path=dict(vars(eng.decode_path()), weights=eng.decode_weights()))
            toks[c] = o.tokens.cpu().numpy()[:, int(o.prompt_lens[0]):]
        ms = {c: [] for c in COMBOS}
        for _ in range(REPEATS):              # the four combinations alternating, same engine, same box
            for c in COMBOS:
                mode(c)
                ms[c].append(timed(run))
        base = toks[COMBOS[0]]
        res = {}
        for c in COMBOS:
            same = toks[c] == base
            res[key(c)] = dict(info[c], ms=spread(ms[c]),
                               us_per_position=spread([1e3 * v / info[c]["positions"] for v in ms[c]]),
                               positions_equal_to_float16=round(float(same.mean()), 4),
                               rows_equal_to_float16=round(float(same.all(axis=1).mean()), 4))
        for cross in ("float16", "int8"):
            f, q = ms[("float16", cross)], ms[("int8", cross)]
            res[f"float16_over_int8_weights_cross_{cross}"] = [round(min(f) / max(q), 3), round(max(f) / min(q), 3)]
        out[leg] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="greedy,sampled")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_int8.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    doc = {"repeats": REPEATS, "device": torch.cuda.get_device_name(0), "models": {}}
    for n in [n for n in MODELS if n in a.models.split(",")]:
        doc["models"][n] = bench(n, a.legs.split(","), dev)
        print(f"{n}: done", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
