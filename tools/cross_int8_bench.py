"""The int8 cross-attention operand (WhisperEngine(cfg, cross_compute="int8"))
against the float16 one: decoder speed, the one-off quantise, and what it costs in tokens.
HIP events, warm-up then three repeats; one JSON document on stdout and in --out (by default
profiles/cross_int8.json).

Seeded synthetic weights (seed 0). The speed parts run the decoder alone: every model's config
without its encoder layers, on a seeded unit-normal encoder output (as a LayerNorm output is),
int8 and float16 alternating on ONE engine in one process (set_cross_compute), three repeats,
min - max.
  greedy    64 rows, max_length 128 (127 positions), no early-exit polling: us per position;
  sampled   320 rows = 64 windows x best_of 5 at T = 0.6, max_length 64 (63 positions), the rows
            of a window sharing its encoder output (PAIR blocks in place up to 8 heads, gathered
            above): us per position, and ms per call (the gather and the quantise are per call);
  quantise  the row quantiser alone over 64 x 1500 rows of d_model: us;
  tokens    base.en with its encoder, 64 x 30 s synthetic windows, max_length 448: the share of
            windows whose greedy tokens equal the float16 call's (not asserted anywhere).
  share     (--share MODEL MODE, for a kernel-trace run of its own) runs the greedy form only.
Usage (GPU box):  python tools/cross_int8_bench.py [--models a,b] [--parts greedy,sampled,quantise,tokens] [--out FILE]"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from janus_amd import _native as nat  # noqa: E402
from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights  # noqa: E402
from janus_amd.workload import synth_speech  # noqa: E402

REPEATS = 3
MODELS = ("tiny.en", "base.en", "small.en", "distil-medium.en", "large-v3-turbo")
MODES = ("float16", "int8")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"runs": [round(x, 2) for x in xs], "min": round(min(xs), 2), "max": round(max(xs), 2)}


def decoder_engine(name):
    """The model's decoder on synthetic weights: its config without encoder layers."""
    cfg = dataclasses.replace(CONFIGS[name], enc_layers=0)
    return WhisperEngine(cfg, synthetic_weights(cfg, seed=0))


def noise(cfg, n, dev):
    g = torch.Generator().manual_seed(17)
    return torch.randn(n, cfg.n_audio_ctx, cfg.d_model, generator=g).half().to(dev)


def speed(name, parts, dev):
    eng = decoder_engine(name)
    cfg = eng.cfg
    B, windows, best_of = 64, 64, 5
    enc = noise(cfg, B, dev)
    ei = [j for j in range(windows) for _ in range(best_of)]
    seeds = [7000 + 13 * i for i in range(len(ei))]
    forms = {}
    if "greedy" in parts:
        forms["greedy_64"] = lambda: eng.decode_ex(enc, max_length=128, check_every=0)
    if "sampled" in parts:
        forms["sampled_320"] = lambda: eng.decode_ex(enc, max_length=64, temperature=0.6, seeds=seeds,
                                                     enc_index=ei, check_every=0)
    out = {"d_model": cfg.d_model, "heads": cfg.n_heads, "dec_layers": cfg.dec_layers}
    for key, run in forms.items():
        info = {}
        for m in MODES:                      # warm-up: graphs captured, buffers allocated
            eng.set_cross_compute(m)
            run()
            torch.cuda.synchronize()
            pos, lau = eng.decode_info()
            info[m] = dict(positions=pos, launches_per_position=round(lau / pos, 2), path=vars(eng.decode_path()))
        ms = {m: [] for m in MODES}
        for _ in range(REPEATS):             # the two operands alternating, same engine, same box
            for m in MODES:
                eng.set_cross_compute(m)
                ms[m].append(timed(run))
        out[key] = {m: dict(info[m], ms=spread(ms[m]),
                            us_per_position=spread([1e3 * v / info[m]["positions"] for v in ms[m]])) for m in MODES}
        lo = [min(ms["float16"]) / max(ms["int8"]), max(ms["float16"]) / min(ms["int8"])]
        out[key]["float16_over_int8"] = [round(v, 3) for v in lo]
    if "quantise" in parts:
        rows, d = B * cfg.n_audio_ctx, cfg.d_model
        q = torch.empty(rows, d, dtype=torch.int8, device=dev)
        s = torch.empty(rows, dtype=torch.float32, device=dev)
        run = lambda: nat.call("janus_quant_rows_i8", enc.data_ptr(), d, q.data_ptr(), d, s.data_ptr(), rows, d,  # noqa: E731
                               nat.stream_ptr())
        run()
        torch.cuda.synchronize()
        out["quantise_64_windows_us"] = spread([1e3 * timed(run) for _ in range(REPEATS)])
    return out


def tokens(dev):
    """base.en end to end: share of 64 windows whose int8 greedy tokens equal the float16 call's."""
    eng = WhisperEngine(CONFIGS["base.en"], seed=0)
    B = 64
    utts = [synth_speech(3000 + i, 30.0) for i in range(B)]
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(u) for u in utts])]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    enc = eng.encode(eng.logmel(pcm, offs, B, 3))
    got = {}
    for m in MODES:
        eng.set_cross_compute(m)
        o = eng.decode_ex(enc, max_length=448)
        got[m] = (o.tokens.cpu().numpy(), o.n_tokens.cpu().numpy())
    same = [bool(np.array_equal(got["int8"][0][b], got["float16"][0][b])) for b in range(B)]
    first = []
    for b in range(B):
        if not same[b]:
            a, c = got["int8"][0][b], got["float16"][0][b]
            first.append(int(np.argmax(a != c)))
    return {"model": "base.en", "windows": B, "max_length": 448, "identical": int(sum(same)),
            "share_identical": round(sum(same) / B, 4), "first_divergence_positions": sorted(first),
            "mean_sampled_tokens_float16": round(float(got["float16"][1].mean()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="greedy,sampled,quantise,tokens")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--share", nargs=2, metavar=("MODEL", "MODE"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_int8.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    if a.share:
        eng = decoder_engine(a.share[0])
        eng.set_cross_compute(a.share[1])
        enc = noise(eng.cfg, 64, dev)
        for _ in range(REPEATS):
            eng.decode_ex(enc, max_length=128, check_every=0)
        torch.cuda.synchronize()
        return
    parts = a.parts.split(",")
    doc = {"repeats": REPEATS, "device": torch.cuda.get_device_name(0), "models": {}}
    for n in [n for n in MODELS if n in a.models.split(",")]:
        doc["models"][n] = speed(n, parts, dev)
        print(f"{n}: done", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if "tokens" in parts:
        doc["tokens"] = tokens(dev)
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
