"""Beam search (WhisperEngine.decode_beam) against the decodes that exist:
one JSON document on stdout and in --out (default profiles/beam_search.json).

base.en, seeded synthetic weights (seed 0: no <|endoftext|>, every decode runs all 447
positions), 64 windows of random encoder rows, max_length 448, check_every 0:
  greedy_64      decode_ex, 64 rows;
  sampled_320    decode_ex at T = 0.6, 64 windows x 5 hypotheses sharing their encoder rows
                 (enc_index): the same row count as beam 5, the fair yardstick;
  beam5_320      decode_beam(beam_size=5): 64 windows x 5 beams.
Each: HIP events around one call, warmed (graphs captured), ROUNDS alternating rounds in one
process; ms per position = call / positions (decode_info).
  kernel_split   from a separate `rocprofv3 --kernel-trace --stats` run of this script, no
                 counters in it (--trace-child: one warmed beam decode in a fresh process): the
                 shares of the decode's kernel time in the top-2k vocabulary projection, the
                 beam step, the KV reorder and the self-attention kernels.

Usage (GPU box):  python tools/beam_bench.py [--out FILE] [--no-trace] [--windows N]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = "base.en"
ROUNDS = 3
MAXLEN = 448
BEAM = 5


def setup(windows):
    import torch
    from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights
    cfg = CONFIGS[MODEL]
    dev = torch.device("cuda", 0)
    eng = WhisperEngine(cfg, synthetic_weights(cfg, seed=0))
    g = torch.Generator().manual_seed(1)
    enc = (torch.randn(windows, cfg.n_audio_ctx, cfg.d_model, generator=g) * 0.5).half().to(dev)
    return eng, enc


def cases(eng, enc):
    W = enc.shape[0]
    eidx = [w for w in range(W) for _ in range(BEAM)]
    seeds = list(range(1, W * BEAM + 1))
    return {
        "greedy_64": lambda: eng.decode_ex(enc, max_length=MAXLEN, check_every=0),
        "sampled_320": lambda: eng.decode_ex(enc, max_length=MAXLEN, check_every=0, temperature=0.6,
                                             seeds=seeds, enc_index=eidx),
        "beam5_320": lambda: eng.decode_beam(enc, beam_size=BEAM, max_length=MAXLEN, check_every=0),
    }


def trace_child(windows):
    """Run under rocprofv3: one warmed beam decode."""
    import torch
    eng, enc = setup(windows)
    run = cases(eng, enc)["beam5_320"]
    run()
    torch.cuda.synchronize()
    run()
    torch.cuda.synchronize()


def kernel_split(windows):
    out = tempfile.mkdtemp(prefix="beam_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv",
               "--", sys.executable, os.path.abspath(__file__), "--trace-child", "--windows", str(windows)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=500, cwd=out)
        trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        assert trace, "rocprofv3 wrote no kernel trace"
        rows = list(csv.DictReader(open(trace[0])))
    finally:
        shutil.rmtree(out, ignore_errors=True)
    groups = {"logits_top2k": ("logits_partial_kernel",), "beam_step": ("beam_step_kernel",),
              "beam_reorder": ("beam_reorder_kernel",),
              "self_attention": ("decode_split_kernel", "decode_combine",
                                 "decode_head_kernel"),
              "cross_attention": ("xattn",)}
    ns = {k: 0.0 for k in groups}
    total, started = 0.0, 0
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the second decode only: from the second beam_init_kernel on
    for r in rows:
        name = r["Kernel_Name"]
        if "beam_init_kernel" in name:
            started += 1
        if started < 2:
            continue
        t = float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
        total += t
        for k, pats in groups.items():
            if any(p in name for p in pats):
                ns[k] += t
                break
    res = {"decode_kernel_ms": round(total / 1e6, 3)}
    for k in groups:
        res[k + "_ms"] = round(ns[k] / 1e6, 3)
        res[k + "_share"] = round(ns[k] / total, 4) if total else None
    res["reorder_over_self_attention"] = round(ns["beam_reorder"] / ns["self_attention"], 3) if ns["self_attention"] else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_search.json"))
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.windows)
        return
    split = None if a.no_trace else kernel_split(a.windows)   # before this process opens the GPU
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    eng, enc = setup(a.windows)
    runs = cases(eng, enc)
    times = {k: [] for k in runs}
    pos = {}
    for k, f in runs.items():   # warm: graphs captured
        f()
        torch.cuda.synchronize()
        pos[k] = eng.decode_info()[0]
    for _ in range(ROUNDS):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    doc = {"device": torch.cuda.get_device_name(0), "model": MODEL, "windows": a.windows, "beam_size": BEAM,
           "max_length": MAXLEN, "rounds": ROUNDS, "cases": {}}
    for k in runs:
        med = float(np.median(times[k]))
        doc["cases"][k] = {"rows": a.windows * (1 if k == "greedy_64" else BEAM), "positions": pos[k],
                           "call_ms": [round(t, 2) for t in times[k]], "median_ms": round(med, 2),
                           "ms_per_position": round(med / max(pos[k], 1), 4)}
    c = doc["cases"]
    doc["beam5_over_sampled320"] = round(c["beam5_320"]["median_ms"] / c["sampled_320"]["median_ms"], 3)
    doc["beam5_over_greedy64"] = round(c["beam5_320"]["median_ms"] / c["greedy_64"]["median_ms"], 3)
    doc["kernel_split"] = split
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
