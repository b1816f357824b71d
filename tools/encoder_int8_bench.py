"""The int8 encoder (WhisperEngine(encoder_compute="int8")) against the fp16
encoder; one JSON document on stdout and in --out (default profiles/encoder_int8.json).

Per model (base.en, small.en), seeded synthetic weights (seed 0), 64 x 30 s clips (seeds
3000 + i, the bench's 64 windows):
  encoder_ms     fp16 and int8, HIP events around one encode(), both engines warmed, then
                 ROUNDS alternating rounds in one process: median and spread;
  kernels        from a separate `rocprofv3 --kernel-trace --stats` run of this script
                 (--trace-child MODEL: int8 encodes only, a fresh process): time per call of
                 every new kernel; per int8 GEMM shape its integer op/s against the dense i8
                 peak (twice the dense fp16 MFMA peak) and the bound that binds it (the larger
                 of ops / peak and bytes / HBM peak); the share of the int8 encoder's kernel
                 time spent in the two stand-alone quantisation passes (quant_rows_kernel);
  token agreement  int8 against fp16, greedy, the first windows of 32 bench clips at
                 max_length 64, on SYNTHETIC weights (an encoder change of 2e-2 moves the tokens
                 of random weights well past their near-ties: no statement about real ones).
And, as tests/test_int8_gpu.py measures them (tiny.en seed 5, base.en seed 7): e_q = relRMS of
the fp32 oracle with fake-quantised encoder linears against the fp32 oracle, and the GPU int8
encoder's relRMS against the fp32 oracle as a multiple of e_q.

Usage (GPU box):  python tools/encoder_int8_bench.py [--models base.en,small.en] [--out FILE]
                  [--no-trace] [--no-oracle]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F16_PEAK_TFLOPS = 2500.0          # dense fp16 MFMA, MI355X
I8_PEAK_TOPS = 2 * MFMA_F16_PEAK_TFLOPS
HBM_PEAK_TBS = 8.0
ROUNDS = 7
BATCH = 64


def spread(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(float(np.median(xs)), 3),
            "min": round(min(xs), 3), "max": round(max(xs), 3)}


def bench_mel(eng, B, dev):
    import torch
    from janus_amd.workload import synth_speech
    utts = [synth_speech(3000 + i, 30.0) for i in range(B)]
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    return eng.logmel(pcm, offs, B, 3)


def trace_child(model):
    """Run under rocprofv3: int8 encodes only."""
    import torch
    from janus_amd.whisper import CONFIGS, WhisperEngine
    dev = torch.device("cuda", 0)
    eng = WhisperEngine(CONFIGS[model], seed=0, encoder_compute="int8")
    mel = bench_mel(eng, BATCH, dev)
    for _ in range(4):
        eng.encode(mel)
    torch.cuda.synchronize()


def gemm_shapes(cfg, B):
    """(name, M, N, K, output bytes per element, residual read) of a layer's four projections."""
    d, M = cfg.d_model, B * cfg.n_audio_ctx
    return [("qkv", M, 3 * d, d, 2, 0), ("out_proj", M, d, d, 4, 4), ("fc1", M, 4 * d, d, 2, 0),
            ("fc2", M, d, 4 * d, 4, 4)]


def grid_threads(r):
    """Threads of a dispatch from a kernel-trace row (one Grid_Size column, or one per axis)."""
    if "Grid_Size" in r:
        return int(r["Grid_Size"])
    return int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1)


def epi_of(name):
    """Epilogue template argument of a gemm_i8_kernel symbol, demangled or mangled."""
    for e in range(4):
        if f"gemm_i8_kernel<{e}>" in name or f"gemm_i8_kernelILi{e}E" in name:
            return e
    return -1


def kernel_stats(model):
    """Kernel times of 4 int8 encodes from a rocprofv3 run of their own (a fresh process)."""
    from janus_amd.whisper import CONFIGS
    cfg = CONFIGS[model]
    out = tempfile.mkdtemp(prefix="enc_i8_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv",
               "--", sys.executable, os.path.abspath(__file__), "--trace-child", model]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=400,
                       cwd=out)
        trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        assert trace, "rocprofv3 wrote no kernel trace"
        rows = list(csv.DictReader(open(trace[0])))
    finally:
        shutil.rmtree(out, ignore_errors=True)
    n_enc = 4
    per = {}     # (short name, grid) -> [ns]
    resid = []   # the EPI_RESID_F32 GEMMs in launch order: out_proj, fc2, out_proj, ...
    total = 0.0
    started = False
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        ns = float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
        if "conv_kernel" in name or "conv1d" in name:
            started = True            # the encoder begins at its conv stem (the log-mel is before)
        if not started:
            continue
        total += ns
        for key in ("gemm_i8_kernel", "quant_rows_kernel", "layernorm_quant_kernel"):
            if key in name:
                per.setdefault((key, name, grid_threads(r)), []).append(ns)
        if "gemm_i8_kernel" in name and epi_of(name) == 2:
            resid.append(ns)
    res = {"encodes_traced": n_enc, "encoder_kernel_ms_per_encode": round(total / n_enc / 1e6, 3), "kernels": []}
    quant_ns = 0.0
    for (key, name, grid), v in sorted(per.items()):
        res["kernels"].append({"kernel": key, "symbol": name[:120], "grid_threads": grid,
                               "calls_per_encode": len(v) // n_enc,
                               "us_per_call": {"median": round(float(np.median(v)) / 1e3, 1),
                                               "min": round(min(v) / 1e3, 1), "max": round(max(v) / 1e3, 1)}})
        if key == "quant_rows_kernel":
            quant_ns += sum(v)
    res["standalone_quant_share_of_int8_encoder"] = round(quant_ns / total, 4)
    # the GEMMs by shape: QKV and fc1 have an epilogue of their own; out_proj and fc2 share the
    # residual one and alternate in launch order
    gem = []
    for nm, M, N, K, ob, rb in gemm_shapes(cfg, BATCH):
        if nm in ("qkv", "fc1"):
            v = [x for (key, name, g), xs in per.items()
                 if key == "gemm_i8_kernel" and epi_of(name) == (0 if nm == "qkv" else 1) for x in xs]
        else:
            v = resid[(0 if nm == "out_proj" else 1)::2]
        if not v:
            continue
        us = float(np.median(v)) / 1e3
        ops = 2.0 * M * N * K
        byts = M * K + N * K + M * N * (ob + rb) + 4 * (M + 2 * N)
        t_ops, t_bytes = ops / (I8_PEAK_TOPS * 1e12), byts / (HBM_PEAK_TBS * 1e12)
        gem.append({"gemm": nm, "M": M, "N": N, "K": K, "us_median": round(us, 1),
                    "int_tops": round(ops / (us * 1e-6) / 1e12, 1),
                    "frac_of_i8_peak": round(ops / (us * 1e-6) / 1e12 / I8_PEAK_TOPS, 4),
                    "bytes": byts, "tb_per_s": round(byts / (us * 1e-6) / 1e12, 2),
                    "bound": "ops" if t_ops >= t_bytes else "bytes",
                    "least_us": round(max(t_ops, t_bytes) * 1e6, 1),
                    "frac_of_bound": round(max(t_ops, t_bytes) * 1e6 / us, 4)})
    res["gemms"] = gem
    return res


def run_model(model):
    import torch
    from janus_amd.whisper import CONFIGS, WhisperEngine
    dev = torch.device("cuda", 0)
    cfg = CONFIGS[model]
    e16 = WhisperEngine(cfg, seed=0)
    e8 = WhisperEngine(cfg, seed=0, encoder_compute="int8")
    mel = bench_mel(e16, BATCH, dev)
    for _ in range(2):                      # warm every shape of both
        enc16, enc8 = e16.encode(mel), e8.encode(mel)
    torch.cuda.synchronize()

    def timed(eng):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.encode(mel)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    ms = {"float16": [], "int8": []}
    for _ in range(ROUNDS):                 # alternating, same process
        ms["float16"].append(timed(e16))
        ms["int8"].append(timed(e8))
    rel = float((enc8.float() - enc16.float()).norm() / enc16.float().norm())
    res = {"model": model, "d_model": cfg.d_model, "enc_layers": cfg.enc_layers, "windows": BATCH,
           "encoder_ms": {k: spread(v) for k, v in ms.items()},
           "int8_over_fp16": round(float(np.median(ms["int8"]) / np.median(ms["float16"])), 4),
           "relrms_int8_vs_fp16_gpu": round(rel, 5)}
    # token agreement, greedy, 32 first windows, max_length 64
    n, L = 32, 64
    o16 = e16.decode_ex(enc16[:n], max_length=L)
    o8 = e8.decode_ex(enc8[:n], max_length=L)
    torch.cuda.synchronize()
    r16, r8 = [r[0] for r in o16.rows()], [r[0] for r in o8.rows()]
    same_seq = sum(list(a) == list(b) for a, b in zip(r16, r8))
    pos = agree = 0
    for a, b in zip(r16, r8):
        m = min(len(a), len(b))
        first = next((i for i in range(m) if a[i] != b[i]), m)
        agree += first
        pos += max(len(a), len(b))
    res["token_agreement"] = {"weights": "synthetic weights", "clips": n, "max_length": L,
                              "identical_sequences": same_seq,
                              "tokens_before_first_divergence_frac": round(agree / max(pos, 1), 4)}
    del e16, e8
    torch.cuda.empty_cache()
    return res


def oracle_ratio(model, seed, clips):
    """e_q and the GPU ratios as tests/test_int8_gpu.py asserts them."""
    import torch
    from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights
    from janus_amd.workload import synth_speech
    from oracle import whisper as ow
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_int8_gpu import fake_quant_lin, pack, rel_rms
    dev = torch.device("cuda", 0)
    cfg = CONFIGS[model]
    W = synthetic_weights(cfg, seed=seed)
    e8, e16 = WhisperEngine(cfg, W, encoder_compute="int8"), WhisperEngine(cfg, W)
    pcm, offs = pack([synth_speech(s, t) for s, t in clips], dev)
    mel = e16.logmel(pcm, offs, len(clips), 3)
    g8, g16 = e8.encode(mel).float().cpu(), e16.encode(mel).float().cpu()
    m = mel.float().cpu().numpy()
    ref = ow.encoder(m, W, cfg)
    with mock.patch.object(ow, "_lin", fake_quant_lin):
        fq = ow.encoder(m, W, cfg)
    e_q = rel_rms(fq, ref)
    return {"model": model, "seed": seed, "e_q": round(e_q, 5),
            "gpu_int8_vs_ref_over_e_q": round(rel_rms(g8, ref) / e_q, 4),
            "gpu_int8_vs_gpu_fp16_over_e_q": round(rel_rms(g8, g16) / e_q, 4),
            "gpu_fp16_vs_ref": round(rel_rms(g16, ref), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="base.en,small.en")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_int8.json"))
    ap.add_argument("--trace-child", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_child)
        return
    models = a.models.split(",")
    # the traced runs first, each in its own process, before this one opens the GPU
    traces = {}
    for m in ([] if a.no_trace else models):
        print(f"[encoder_int8_bench] kernel trace of {m}", file=sys.stderr, flush=True)
        traces[m] = kernel_stats(m)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
           "peaks": {"i8_dense_tops": I8_PEAK_TOPS, "fp16_dense_tflops": MFMA_F16_PEAK_TFLOPS,
                     "hbm_tb_per_s": HBM_PEAK_TBS},
           "models": []}
    for m in models:
        print(f"[encoder_int8_bench] timing {m}", file=sys.stderr, flush=True)
        r = run_model(m)
        if m in traces:
            r["kernel_trace"] = traces[m]
        doc["models"].append(r)
    if not a.no_oracle:
        doc["oracle"] = [oracle_ratio("tiny.en", 5, [(30, 30.0), (31, 9.0)]),
                         oracle_ratio("base.en", 7, [(31, 9.0)])]
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
