"""Every compiled form of the vocabulary projection (logits_partial_kernel), each launched once.

The launcher chooses among 43 instantiations by (K, SAMPLE, BEAM, HIST, W8); each launches with
more than 64 KB of dynamic LDS, so a form whose opt-in is missing or belongs to another kernel
fails on first use. One case per table entry, through the kernel-level entry points:

    greedy, sample   janus_logits_partial_f16          HIST        janus_logits_partial_hist_f16
    W8               janus_logits_partial_w8_f16       HIST + W8   janus_logits_partial_hist_w8_f16
    BEAM             janus_beam_logits_topk_f16

Shape: V = 1610 (the last tile holds 10 columns, the special ids at the top, as
test_decoder_int8_gpu.py) and logits_row_group(K) + 1 rows — 65, 49 or 33: two row groups, the
second with one row; 13 blocks. Expected values: the float64 product of the same operands (the
int8 table as decoder_int8_ref.quantise gives it), merged by large_family_ref.merge_parts and
filtered by allowed_mask, held to the criteria of check_projection_row
(test_medium_family_gpu.py / test_decoder_int8_gpu.py): 1e-4 relative on the three log-sums, 2e-3
on t_v and m_text, argmax equality where the reference margin exceeds 2e-3 (sampled: 2e-3 / T on
the keys logit / T + the device's own noise, as test_vocabulary_projection_w8_sampling_keys).
The history words hold the bits of tests/history_ref.py's rules for a per-row token history
(p = 1.2, n = 3), laid out as test_decode_options_gpu.py lays them out. BEAM: test_beam_gpu.py's
comparison, the 16 best entries of both sets by index and within 1e-4 of the largest logit.
Every case compares at least as many argmax decisions as it has rows; the seeds below were chosen
on the CPU so that the float64 reference alone has those margins (sampled cases: with
oracle.whisper.sample_noise, which test_whisper_gpu.py::test_sample_noise_matches_oracle pins to the
device's noise).
"""
import functools

import numpy as np
import pytest
import torch

import decoder_int8_ref as d8
import history_ref as hr
import large_family_ref as lf
from janus_amd import _native as nat

pytestmark = pytest.mark.gpu
F32 = np.float32
PV = 16 * 100 + 10          # the last tile holds 10 columns
EOT, NSP, NOTS, TSB, BLANK = 1500, 1501, 1502, 1503, 220      # the special ids at the top
ROW_GROUP = {384: 64, 512: 64, 768: 64, 1024: 48, 1280: 32}   # logits_row_group(K)
SEED = {384: 4392, 512: 4517, 768: 4768, 1024: 5024, 1280: 5280}
PEN, NGRAM = 1.2, 3
T_SAMPLE, POS = 0.6, 5
N2K = 16                    # kBeamTop: the longest list the beam partials carry
NEAR_TIE = 2e-3


def allowed(c, b):
    return lf.allowed_mask(PV, c["smask"], tuple(c["rules"][b, :4]), EOT, BLANK, TSB, NOTS, 50)


@functools.lru_cache(maxsize=None)
def case(K):
    """Operands, rule states and both float64 references of one width, computed once: A fp16
    [rows][K], the fp16 table and its int8 quantisation, L['f16'] / L['w8'] float64 [rows][PV],
    the suppress mask and the row rule states as test_decoder_int8_gpu.proj_case builds them."""
    B = ROW_GROUP[K] + 1
    g = torch.Generator().manual_seed(SEED[K])
    A = torch.randn(B, K, generator=g).half()
    Wt = (0.05 * torch.randn(PV, K, generator=g)).half().numpy()
    Wt *= (2.0 ** np.random.default_rng(K).integers(-2, 3, size=(PV, 1))).astype(np.float16)
    # the last real id wins row 0 by construction: its row along A[0] (logit ~ 40)
    Wt[PV - 1] = (A[0].float() * (40.0 / float((A[0].float() ** 2).sum()))).half().numpy()
    q, s = d8.quantise(Wt)
    A64 = A.double().numpy()
    L = {"f16": A64 @ Wt.astype(np.float64).T, "w8": (A64 @ q.astype(np.float64).T) * s.astype(np.float64)}
    smask = np.zeros((PV + 15) // 16 * 16, np.uint8)
    smask[[1, 2, 7, 300, 301, 1499, NSP]] = 1
    rules = np.zeros((B, 8), np.int32)
    rules[:, 3] = rules[:, 4] = -1
    for b in range(B):
        kind = b % 4
        if kind == 1:      # first sampled token: timestamps up to max_initial only, no blank / eot
            rules[b, 0] = 1
        elif kind == 2:    # after text + timestamp: text banned, timestamps from the floor
            rules[b, 2] = 1
            rules[b, 3] = TSB + 60
        elif kind == 3:    # after two timestamps: every timestamp banned
            rules[b, 1] = 1
            rules[b, 3] = TSB + 7
    return dict(K=K, B=B, A=A, Wt=Wt, q=q, s=s, L=L, smask=smask, rules=rules)


def histories(c, table):
    """Per row the tokens sampled so far: they penalise the row's winner, its runner-up, the eot
    tile and the last tile, and (n = 3: the bigram 17 31 twice before its third occurrence) ban
    the runner-up and a token of the last tile."""
    out = []
    for b in range(c["B"]):
        order = np.argsort(np.where(allowed(c, b), c["L"][table][b], -np.inf))
        out.append([17, 31, PV - 3, EOT, int(order[-1]), 17, 31, int(order[-2]), 17, 31])
    return out


def history_words(c, hist):
    """uint32 [group][tile][row of the group]: bits 0-15 penalised, 16-31 banned columns."""
    rg = ROW_GROUP[c["K"]]
    words = np.zeros(((c["B"] + rg - 1) // rg, (PV + 15) // 16, rg), np.uint32)
    for b, g in enumerate(hist):
        for t in set(g):
            words[b // rg, t >> 4, b % rg] |= np.uint32(1 << (t & 15))
        for t in hr.banned(g, NGRAM):
            words[b // rg, t >> 4, b % rg] |= np.uint32(0x10000 << (t & 15))
    return words


def reference(c, table, hist):
    """Per row (allowed mask, float64 logits the filtered statistics see, raw float64 logits)."""
    out = []
    for b in range(c["B"]):
        ok, raw = allowed(c, b), c["L"][table][b]
        Lp = raw
        if hist is not None:
            ban = hr.banned(hist[b], NGRAM)
            assert len(ban) == 2
            ok[ban] = False
            Lp = hr.penalise(raw, hist[b], PEN).astype(np.float64)
        out.append((ok, Lp, raw))
    return out


def lse(v):
    return float(v.max() + np.log(np.exp(v - v.max()).sum())) if v.size else -np.inf


def check_row(b, g, ok, Lp, raw, keys=None, margin=NEAR_TIE, target=True):
    """check_projection_row's criteria with its numbers; the argmax is taken over ``keys`` (the
    logits unless sampling). Returns the argmax decisions clear enough to be compared."""
    keys = Lp if keys is None else keys
    for name, want in (("lse_all", lse(Lp[ok])), ("lse_ts", lse(Lp[TSB:][ok[TSB:]])), ("lse_raw", lse(raw))):
        if np.isfinite(want):
            assert abs(g[name] - want) <= 1e-4 * abs(want), (b, name, g[name], want)
        else:
            assert g[name] == -np.inf, (b, name, g[name])
    if target:
        assert abs(g["t_v"] - raw[NSP]) <= 2e-3, (b, g["t_v"], raw[NSP])
    checked = 0
    for key, sel in (("best", ok), ("best_ts", ok & (np.arange(PV) >= TSB))):
        if not sel.any():
            continue
        cand = np.where(sel, keys, -np.inf)
        top = np.sort(cand)[-2:]
        assert 0 <= g[key] < PV, (b, key, g[key])             # never a padded column
        if top[-1] - top[-2] > margin:
            assert g[key] == int(np.argmax(cand)), (b, key, g[key], int(np.argmax(cand)))
            checked += 1
    if ok[:TSB].any():
        assert abs(g["m_text"] - Lp[:TSB][ok[:TSB]].max()) <= 2e-3
    return checked


def rule_args(target):
    return [EOT, 1, BLANK, TSB, NOTS, 50] + ([target] if target is not None else [])


def device_operands(gpu, c):
    sm = torch.from_numpy(c["smask"]).to(gpu)
    rr = torch.from_numpy(c["rules"]).to(gpu)
    return c["A"].to(gpu), sm, rr


@pytest.mark.parametrize("table", ["f16", "w8"])
@pytest.mark.parametrize("hist", [False, True], ids=["plain", "hist"])
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sample"])
@pytest.mark.parametrize("K", sorted(ROW_GROUP))
def test_projection_form(gpu, K, sample, hist, table):
    c = case(K)
    B = c["B"]
    Ad, sm, rr = device_operands(gpu, c)
    if table == "w8":
        keep = (torch.from_numpy(c["q"]).to(gpu), torch.from_numpy(c["s"]).to(gpu))
        weights = [keep[0].data_ptr(), keep[1].data_ptr()]
    else:
        keep = (torch.from_numpy(c["Wt"]).to(gpu),)
        weights = [keep[0].data_ptr()]
    nblk = nat.lib().janus_beam_partial_blocks(PV, K, 256)
    # 13 blocks; two row groups of logits_row_group(K) rows, the second holding one row
    assert nblk == 13 and nat.lib().janus_history_words(PV, K, B) == 2 * ((PV + 15) // 16) * (B - 1)
    parts = torch.zeros(B * nblk * 56, dtype=torch.uint8, device=gpu)
    seeds = [7000 + K + b for b in range(B)]
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu)
    args = [Ad.data_ptr()] + weights + [K, PV, B] + rule_args(NSP) + \
        [sm.data_ptr(), rr.data_ptr(), 256, float(1.0 / T_SAMPLE) if sample else 0.0,
         sd.data_ptr() if sample else None, POS, parts.data_ptr()]
    tokens = histories(c, table) if hist else None
    if hist:
        words = torch.from_numpy(history_words(c, tokens).view(np.int32).reshape(-1)).to(gpu)
        assert words.numel() == nat.lib().janus_history_words(PV, K, B)
        args += [words.data_ptr(), float(PEN)]
    entry = "janus_logits_partial" + ("_hist" if hist else "") + ("_w8" if table == "w8" else "") + "_f16"
    nat.call(entry, *args, nat.stream_ptr())
    torch.cuda.synchronize()
    got = lf.merge_parts(parts.cpu().numpy().view(lf.PART_DTYPE).reshape(B, nblk))
    noise = None
    if sample:
        nd = torch.empty(B, PV, dtype=torch.float32, device=gpu)
        nat.call("janus_sample_gumbel_f32", sd.data_ptr(), B, POS, PV, nd.data_ptr(), nat.stream_ptr())
        torch.cuda.synchronize()
        noise = nd.cpu().numpy().astype(np.float64)
    inv = float(F32(1.0) / F32(T_SAMPLE))
    checked = 0
    for b, (ok, Lp, raw) in enumerate(reference(c, table, tokens)):
        if sample:
            checked += check_row(b, got[b], ok, Lp, raw, keys=Lp * inv + noise[b], margin=NEAR_TIE / T_SAMPLE)
        else:
            checked += check_row(b, got[b], ok, Lp, raw)
        if hist:
            assert got[b]["best"] not in hr.banned(tokens[b], NGRAM)
    print(f"{entry} K {K} {'sample' if sample else 'greedy'}: {checked} argmax decisions over {B} rows")
    if not sample and not hist:
        assert got[0]["best"] == PV - 1      # the last real id wins: a padded copy of it would move the sums
    assert checked >= B


def top_of(vals, ok, n):
    idx = np.flatnonzero(ok)
    return idx[np.lexsort((idx, -vals[idx]))][:n + 1]


@pytest.mark.parametrize("K", [384, 512, 768])
def test_projection_beam_form(gpu, K):
    c = case(K)
    B, L = c["B"], c["L"]["f16"]
    Ad, sm, rr = device_operands(gpu, c)
    Wd = torch.from_numpy(c["Wt"]).to(gpu)
    nblk = nat.lib().janus_beam_partial_blocks(PV, K, 256)
    parts = torch.zeros(B * nblk * 56, dtype=torch.uint8, device=gpu)
    tops = torch.zeros(B * nblk * 64, dtype=torch.float32, device=gpu)
    av = torch.empty(B, N2K, dtype=torch.float32, device=gpu)
    tv = torch.empty_like(av)
    ai = torch.empty(B, N2K, dtype=torch.int32, device=gpu)
    ti = torch.empty_like(ai)
    nat.call("janus_beam_logits_topk_f16", Ad.data_ptr(), Wd.data_ptr(), K, PV, B, *rule_args(None), sm.data_ptr(),
             rr.data_ptr(), 256, parts.data_ptr(), tops.data_ptr(), N2K, av.data_ptr(), ai.data_ptr(),
             tv.data_ptr(), ti.data_ptr(), nat.stream_ptr())
    torch.cuda.synchronize()
    av, ai, tv, ti = av.cpu().numpy(), ai.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()
    got = lf.merge_parts(parts.cpu().numpy().view(lf.PART_DTYPE).reshape(B, nblk))
    tol = 1e-4 * float(np.abs(L).max())
    is_ts = np.arange(PV) >= TSB
    checked = 0
    for b in range(B):
        ok = allowed(c, b)
        for gv, gi, sel in ((av[b], ai[b], ok), (tv[b], ti[b], ok & is_ts)):
            o = top_of(L[b], sel, N2K)
            # the reference's own order is clear of rounding (seeds chosen so, on the CPU)
            assert len(o) < 2 or float(np.min(-np.diff(L[b][o]))) > 1e-4, (b, "reference order near a tie")
            o = o[:N2K]
            n = len(o)
            assert list(gi[:n]) == list(o), (b, gi, o)
            assert np.all(gi[n:] == -1) and np.all(np.isneginf(gv[n:]))
            assert np.abs(gv[:n] - L[b][o]).max(initial=0.0) <= tol
        # the statistics the partials carry beside the lists (no target: t_v stays -inf)
        checked += check_row(b, got[b], ok, L[b], L[b], target=False)
        assert got[b]["t_v"] == -np.inf
    assert got[0]["best"] == PV - 1
    assert checked >= B
