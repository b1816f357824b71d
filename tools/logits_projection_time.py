"""janus_logits_partial_f16 at K = 1024, V = 51 864 on the library JANUS_LIB names (default: this
tree's): us per launch at 64 and 256 rows, greedy and sampled, back to back ("hot": the 106 MB
table stays in the Infinity Cache) and with 512 MB written before each launch ("cold": the table
comes from HBM, as after a 24-layer decoder step). One JSON line on stdout.

The row-group comparison of DESIGN.md §5q (profiles/medium_family_row_group.json): build a
second library with MT = 2 in the K = 1024 row of kLgWidths (csrc/decoder.hip; once kLgMt1024)
  make -C janus_amd/csrc OUT=../libjanus_hip_mt2.so OBJDIR=../../build/obj_mt2
and run this tool in alternating processes, three rounds:
  python tools/logits_projection_time.py; JANUS_LIB=libjanus_hip_mt2.so python tools/logits_projection_time.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from janus_amd import _native as nat
from janus_amd import tokenizer as tok

dev = torch.device("cuda", 0)
TK = tok.WhisperTokenizer()
V, K = TK.n_vocab, 1024
g = torch.Generator().manual_seed(1)
A = torch.randn(256, K, generator=g).half().to(dev)
W = (0.05 * torch.randn(V, K, generator=g)).half().to(dev)
smask = np.zeros((V + 15) // 16 * 16, np.uint8); smask[TK.suppress_tokens()] = 1
sm = torch.from_numpy(smask).to(dev)
rules = np.zeros((256, 8), np.int32); rules[:, 3] = rules[:, 4] = -1
rr = torch.from_numpy(rules).to(dev)
seeds = torch.arange(256, dtype=torch.int32, device=dev)
nblk = nat.lib().janus_beam_partial_blocks(V, K, 256)
parts = torch.zeros(256 * nblk * 56, dtype=torch.uint8, device=dev)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

def launch(B, inv):
    nat.call("janus_logits_partial_f16", A.data_ptr(), W.data_ptr(), K, V, B, TK.eot, 1, TK.blank, TK.timestamp_begin,
             TK.no_timestamps, 50, TK.no_speech, sm.data_ptr(), rr.data_ptr(), 256, float(inv), seeds.data_ptr(), 5,
             parts.data_ptr(), nat.stream_ptr())

def hot(B, inv, n=300):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): launch(B, inv)
    b.record(); b.synchronize()
    return 1e3 * a.elapsed_time(b) / n

def cold(B, inv, n=20):
    tot = 0.0
    for _ in range(n):
        flush.fill_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); launch(B, inv); b.record(); b.synchronize()
        tot += a.elapsed_time(b)
    return 1e3 * tot / n

out = {"lib": os.environ.get("JANUS_LIB", "libjanus_hip.so"), "row_group": nat.lib().janus_history_words(V, K, 1) // ((V + 15) // 16)}
for B in (64, 256):
    for name, inv in (("greedy", 0.0), ("sampled", 1 / 0.6)):
        for _ in range(10): launch(B, inv)
        torch.cuda.synchronize()
        out[f"{name}_{B}_hot_us"] = [round(hot(B, inv), 1) for _ in range(3)]
        out[f"{name}_{B}_cold_us"] = [round(cold(B, inv), 1) for _ in range(3)]
print(json.dumps(out))
