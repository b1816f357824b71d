"""The 1280-wide, 20-head family (large-v3, large-v3-turbo, distil-large-v3) on the GPU against
the unchanged oracle (oracle/whisper.py), tests/large_family_ref.py and tests/decoder_ref.py.
Every test runs the cut config — the real width, heads, 128 mel bins and the 51 866-entry
vocabulary over 2 encoder and 2 decoder layers, synthetic weights (seed 11) — a kernel alone, or
the residual-stream model of tests/test_decoder_hidden_gpu.py at 1280 / 20, so each takes
seconds.

Tolerances are the project's: 2e-3 (log-mel), ENC_TOL (encoder, relative RMS), NEAR_TIE (a
free-running decode may leave the oracle's only where the oracle's own top-2 margin is below
it), the sum_logprob / no_speech_prob bounds of tests/test_small_family_gpu.py,
DETECT_BOUND of tests/test_multilingual_gpu.py, the cross-attention bound of
tests/test_kernels_gpu.py (XATTN_TOL = 3e-3, twice that on a single head) and K_BOUND of
tests/decoder_ref.py (three times the fp16 emulation's own distance from float64).

Seeds, chosen on the CPU oracle alone (W = synthetic_weights(CUT, 11)):
* greedy rows: encoder seeds 900 .. 904 with the five prompts of greedy_prompts(); the oracle's
  smallest top-2 margins over 31 steps are 1.6e-2, 5.8e-2, 7.5e-2, 5.3e-2, 1.5e-2;
* sampled rows (T = 0.6, encoder seed 920): noise seeds 3001, 3002, 3003, 3005, 3012, smallest
  key margins 8.5e-2, 7.7e-2, 1.4e-1, 1.0e-1, 9.3e-2 (10 x NEAR_TIE / T is 3.3e-2);
* language windows: encoder seeds 930 .. 932, reference top-2 logit gaps 0.78, 0.62, 0.77;
* seek loop: synth_speech seeds 170 (35 s) and 171 (4 s), first-window language gaps 8.2e-2
  and 9.6e-2;
* residual stream: decoder_ref.config(1280, 20, 141), weights seed 3, inputs seed 5 (the seeds
  of tests/test_decoder_hidden_gpu.py), one draw of 65 rows x 5 positions and one of 17 x 70.

Measured on the MI355X (printed by the tests, pytest -s).

Residual stream of the default (float16) decode call at 1280 / 20, row / tile, with the
emulation's own figure on the same rows after the bar (the bound is three times that one):
  case           x                                        k cache tile        v cache tile
  rows 1, T 5    5.77e-4 / 8.67e-4 | 5.61e-4 / 9.13e-4    9.19e-4 | 9.19e-4   9.81e-4 | 8.48e-4
  rows 17, T 5   6.28e-4 / 8.93e-4 | 6.31e-4 / 9.56e-4    1.06e-3 | 9.98e-4   1.07e-3 | 1.08e-3
  rows 65, T 5   6.28e-4 / 9.95e-4 | 6.31e-4 / 9.91e-4    1.06e-3 | 1.08e-3   1.09e-3 | 1.13e-3
  rows 17, T 70  6.50e-4 / 1.03e-3 | 6.51e-4 / 1.03e-3    1.25e-3 | 1.19e-3   1.21e-3 | 1.22e-3
  shared rows    5.72e-4 / 8.67e-4 | 5.53e-4 / 9.13e-4    9.19e-4 | 9.27e-4   9.94e-4 | 9.60e-4
The path sits at 0.9 - 1.2 times the emulation, as the other widths do. The defect (fc2 bias of
layer 1 zeroed on columns 1264 .. 1279): reference 4.76e-2, engine 4.77e-2, both 17.4x the
bound 2.74e-3 at column 1264; the restored engine's worst tile is 8.93e-4 (0.33x).

Cross-attention alone (xattn_kernel<1280, 32, HG = 10> and the 20-head merge), relative error
overall, then the worst head of group 0 (heads 0 - 9) and of group 1 (10 - 19); the bounds are
3e-3 and 6e-3:
  rows  keys  splits   overall   group 0   group 1
     1  1500       1   2.22e-4   2.73e-4   2.50e-4
     1  1500       8   2.09e-4   2.33e-4   2.25e-4
     2  1500       3   2.13e-4   2.43e-4   2.37e-4
     2   141       1   2.13e-4   2.62e-4   2.66e-4
    17   141       3   2.13e-4   2.84e-4   2.77e-4
    17    77       8   2.14e-4   2.88e-4   2.88e-4
     2    33       1   2.20e-4   2.94e-4   2.69e-4
     2    32       1   2.19e-4   2.79e-4   2.63e-4
     1  1500      17   2.05e-4   2.14e-4   2.15e-4"""
import functools
import math

import numpy as np
import pytest
import torch

import beam_ref
import decoder_ref as dref
import large_family_ref as lf
import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd.whisper import (DEC_PATH_CVP, DEC_PATH_LN_FUSE, DEC_PATH_NO_CVP, DEC_PATH_NO_EMBED_LN,
                               DEC_PATH_RESID_LN, WhisperEngine, dec_path_ln_mask, mel_filters,
                               synthetic_weights)
from janus_amd.workload import synth_speech
from oracle import whisper as ow

pytestmark = pytest.mark.gpu
CUT = lf.CUT
V = lf.V
NEAR_TIE = 2e-3
ENC_TOL = 1e-3
NSP_REL = 5e-3
DETECT_BOUND = 4 * 2.80e-3          # tests/test_multilingual_gpu.py
XATTN_TOL = 3e-3                    # tests/test_kernels_gpu.py::test_cross_attention_absorbed
ML = 32
GREEDY_SEEDS = [900, 901, 902, 903, 904]
SAMPLE_SEEDS = [3001, 3002, 3003, 3005, 3012]


@pytest.fixture(scope="module")
def cut(gpu):
    W = synthetic_weights(CUT, seed=11)
    eng = WhisperEngine(CUT, W)
    tk = eng.tokenizer
    assert tk.n_vocab == V and tk.timestamp_begin == 50365 and tk.n_languages == 100
    return eng, W


def pack(utts, dev):
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    return pcm, offs


# ------------------------------------------------------------------ 1. log-mel at 128 bins
@pytest.mark.parametrize("secs", [1.0, 31.0])
def test_logmel_128(cut, gpu, secs):
    """1 s and 31 s (past the 30 s window) at 48 kHz, decimated by 3: the normalised features
    against oracle.logmel with the 128-bin filters, <= 2e-3 (the 80-bin bound)."""
    eng, _ = cut
    x = synth_speech(40 + int(secs), secs)
    pcm, offs = pack([x], gpu)
    mel, raw = eng.logmel(pcm, offs, 1, 3, want_raw=True)
    torch.cuda.synchronize()
    assert mel.shape == (1, 3000, 128) and raw.shape == (1, 3000, 128)
    ref = ow.logmel(x, 3, mel_filters(n_mels=128))
    assert ref.shape == (3000, 128)
    err = float(np.abs(mel[0].float().cpu().numpy() - ref).max())
    print(f"log-mel 128 bins, {secs} s: max abs error {err:.2e}")
    assert err <= 2e-3, err


# ------------------------------------------------------------------ 2. encoder
def _enc_err(got, ref):
    got = got.float().cpu()
    rel = float((got - ref).norm() / ref.norm())
    per_row = ((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    return rel, per_row


@pytest.mark.parametrize("windows", [1, 2])
def test_encoder_cut(cut, gpu, windows):
    """Conv stem at Cin 128 / Cout 1280, the projections at N = 1280 / 3840 / 5120, 20-head
    attention, LayerNorm at 1280: relative RMS <= ENC_TOL, worst row <= 4 ENC_TOL."""
    eng, W = cut
    pcm, offs = pack([synth_speech(300 + k, [30.0, 9.0][k]) for k in range(windows)], gpu)
    mel = eng.logmel(pcm, offs, windows, 3)
    enc = eng.encode(mel)
    torch.cuda.synchronize()
    assert enc.shape == (windows, 1500, 1280)
    rel, per_row = _enc_err(enc, ow.encoder(mel.float().cpu().numpy(), W, CUT))
    print(f"large-cut, {windows} window(s): encoder rel RMS {rel:.2e}, worst row {per_row:.2e}")
    assert rel <= ENC_TOL and per_row <= 4 * ENC_TOL, (rel, per_row)


# ------------------------------------------------------------------ 3. free-running greedy decode
def greedy_prompts(tk):
    de, ja = tk.sot_sequence_for("de", "transcribe"), tk.sot_sequence_for("ja", "translate")
    return [de, [tk.sot_prev, 400, 1200, 3300] + ja, tk.sot_sequence_for("en", "transcribe"),
            tk.sot_sequence_for("yue", "translate"), [tk.sot_prev, 9000] + de]


@pytest.fixture(scope="module")
def greedy_ref(cut):
    """The oracle's greedy decode of the five base rows to ML tokens and their no-speech
    probability at <|startoftranscript|>, computed once for the module."""
    eng, W = cut
    tk = eng.tokenizer
    enc = beam_ref.rand_enc(CUT, GREEDY_SEEDS)
    prompts = greedy_prompts(tk)
    rows = mr.greedy(enc, W, CUT, tk, prompts, ML)
    nsp = [mr.no_speech_at(p, len(p) - 3, enc[b], W, CUT, tk) for b, p in enumerate(prompts)]
    for r in rows:
        assert min(r["margins"]) >= NEAR_TIE          # the oracle alone: every row decidable
    return enc, prompts, rows, nsp


@pytest.mark.parametrize("nrows", [1, 3, lf.ROW_GROUP + 1])
def test_free_running_greedy_decode(cut, greedy_ref, gpu, nrows):
    """1 row, 3 rows (a partial MFMA row tile) and 33 rows (one past the 32-row group of the
    vocabulary projection at K = 1280); row b is base row b mod 5, so prompts of lengths 3, 7,
    3, 3 and 5 (two with a <|startofprev|> prefix) step together. Tokens identical to the
    oracle's, or first divergence at an oracle margin < NEAR_TIE; at least 0.75 of the rows
    identical; sum_logprob within 1e-3 relative on identical rows, no_speech_prob within 5e-3
    relative."""
    eng, _ = cut
    enc_np, prompts, ref, nsp_ref = greedy_ref
    idx = [b % 5 for b in range(nrows)]
    enc = torch.from_numpy(enc_np[idx]).half().to(gpu)
    pr = [prompts[i] for i in idx]
    out = eng.decode_ex(enc, prompts=pr, max_length=ML)
    torch.cuda.synchronize()
    p = eng.decode_path()
    assert p.enc_rows == "own" and p.persistent == 0
    toks, nt = out.tokens.cpu().numpy(), out.n_tokens.cpu().numpy()
    slp, nsp = out.sum_logprob.cpu().numpy(), out.no_speech_prob.cpu().numpy()
    same = 0
    for b, i in enumerate(idx):
        r, pl = ref[i], len(pr[b])
        assert list(toks[b][:pl]) == pr[b]
        g = [int(t) for t in toks[b][pl:pl + int(nt[b])]]
        assert abs(nsp[b] - nsp_ref[i]) <= NSP_REL * nsp_ref[i] + 1e-12, (b, nsp[b], nsp_ref[i])
        if g == r["tokens"]:
            same += 1
            assert abs(slp[b] - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]), (b, slp[b], r["sum_lp"])
        else:
            first = mr.first_divergence(g, r["tokens"])
            margin = r["margins"][first] if first is not None and first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE, (b, first, margin)
    print(f"{nrows} rows: {same} identical to the oracle")
    assert same >= 0.75 * nrows, (same, nrows)
    # a persistent request at this width takes the launch path and decodes the same bits
    q = eng.decode_ex(enc, prompts=pr, max_length=ML, persistent=2)
    assert eng.decode_path().persistent == 0
    assert torch.equal(q.tokens, out.tokens) and torch.equal(q.sum_logprob, out.sum_logprob)


# ------------------------------------------------------------------ 4. sampled decode
def test_sampled_decode_shares_one_encoder_row(cut, gpu):
    """best_of 5 at T = 0.6 over ONE encoder row (enc_index): the rows take a gathered copy
    each (no in-place blocks at 20 heads — the path report says so) and match the oracle's
    sampler with the same seeds: identical, or first divergence at a key margin < NEAR_TIE / T;
    at most one row diverges."""
    eng, W = cut
    tk = eng.tokenizer
    T, ml = 0.6, 24
    enc_np = beam_ref.rand_enc(CUT, [920])
    prompt = tk.sot_sequence_for("fr", "transcribe")
    enc = torch.from_numpy(enc_np).half().to(gpu)
    out = eng.decode_ex(enc, prompts=[prompt] * 5, max_length=ml, temperature=T, seeds=SAMPLE_SEEDS,
                        enc_index=[0] * 5)
    torch.cuda.synchronize()
    assert eng.decode_path().enc_rows == "gathered"
    ref = ow.greedy_cached(np.repeat(enc_np, 5, 0), W, CUT, tk, ml, prompts=[prompt] * 5, no_speech=None,
                           temperature=T, seeds=SAMPLE_SEEDS)
    toks = out.tokens.cpu().numpy()
    same = 0
    for b, r in enumerate(ref):
        g = [int(t) for t in toks[b][3:3 + int(out.n_tokens[b])]]
        print(f"row {b}: oracle min key margin {min(r['margins']):.2e}, identical {g == r['tokens']}")
        if g == r["tokens"]:
            same += 1
            assert abs(float(out.sum_logprob[b]) - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]) + 1e-3
        else:
            first = mr.first_divergence(g, r["tokens"])
            margin = r["margins"][first] if first is not None and first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE / T, (b, first, margin)
    assert same >= 4, same
    assert len({tuple(t) for t in toks.tolist()}) > 1          # the seeds draw different rows


# ------------------------------------------------------------------ 5. the vocabulary projection
PROJ_SEED = 4100


@pytest.fixture(scope="module")
def proj_case(gpu):
    """A [33][1280], W [51866][1280] in fp16 (one generator), the float64 product, the suppress
    mask and per-row rule states that exercise the first-token rule, the timestamp floor, text
    suppression and timestamp suppression."""
    g = torch.Generator().manual_seed(PROJ_SEED)
    B = lf.ROW_GROUP + 1
    A = torch.randn(B, 1280, generator=g).half()
    Wt = (0.05 * torch.randn(V, 1280, generator=g)).half()
    # the last real id wins row 0 by construction: its row along A[0] (logit ~ 40)
    Wt[V - 1] = (A[0].float() * (40.0 / float((A[0].float() ** 2).sum()))).half()
    L = A.double().numpy() @ Wt.double().numpy().T          # float64 [33][V]
    tk = tok.WhisperTokenizer(n_vocab=V)
    smask = np.zeros((V + 15) // 16 * 16, np.uint8)
    smask[tk.suppress_tokens()] = 1
    rules = np.zeros((B, 8), np.int32)
    rules[:, 3] = rules[:, 4] = -1
    for b in range(B):
        kind = b % 4
        if kind == 1:      # first sampled token: timestamps up to max_initial only, no blank / eot
            rules[b, 0] = 1
        elif kind == 2:    # after text + timestamp: text banned, timestamps from the floor
            rules[b, 2] = 1
            rules[b, 3] = tk.timestamp_begin + 100
        elif kind == 3:    # after two timestamps: every timestamp banned
            rules[b, 1] = 1
            rules[b, 3] = tk.timestamp_begin + 7
    return A, Wt, L, tk, smask, rules


def run_projection(gpu, A, Wt_dev, tk, smask, rules, rows, inv_temp=0.0, seeds=None, pos=5):
    B = len(rows)
    Ad = A[rows].contiguous().to(gpu)
    sm = torch.from_numpy(smask).to(gpu)
    rr = torch.from_numpy(np.ascontiguousarray(rules[rows])).to(gpu)
    nblk = nat.lib().janus_beam_partial_blocks(V, 1280, 256)
    parts = torch.zeros(B * nblk * 56, dtype=torch.uint8, device=gpu)
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu) if seeds is not None else None
    nat.call("janus_logits_partial_f16", Ad.data_ptr(), Wt_dev.data_ptr(), 1280, V, B, tk.eot, 1, tk.blank,
             tk.timestamp_begin, tk.no_timestamps, 50, tk.no_speech, sm.data_ptr(), rr.data_ptr(), 256,
             float(inv_temp), sd.data_ptr() if sd is not None else None, pos, parts.data_ptr(),
             nat.stream_ptr())
    torch.cuda.synchronize()
    return lf.merge_parts(parts.cpu().numpy().view(lf.PART_DTYPE).reshape(B, nblk))


@pytest.mark.parametrize("nrows", [1, 17, lf.ROW_GROUP - 1, lf.ROW_GROUP, lf.ROW_GROUP + 1])
def test_vocabulary_projection_1280(proj_case, gpu, nrows):
    """K = 1280, V = 51 866 (the last tile holds 10 columns) at 1, 17 and 31 / 32 / 33 rows —
    the 32-row group's boundary — against the float64 product of the same fp16 operands: per
    row the filtered log-sum-exps (all, timestamps) and the raw one within 1e-4 relative, the
    largest allowed text logit, the argmax over the allowed tokens and over the allowed
    timestamps wherever the reference margin exceeds 2e-3, and the no-speech logit."""
    A, Wt, L, tk, smask, rules = proj_case
    Wd = Wt.to(gpu)
    rows = list(range(nrows))
    got = run_projection(gpu, A, Wd, tk, smask, rules, rows)
    tb = tk.timestamp_begin
    checked = 0
    for b in rows:
        ok = lf.allowed_mask(V, smask, tuple(rules[b, :4]), tk.eot, tk.blank, tb, tk.no_timestamps, 50)
        ref = L[b]
        g = got[b]

        def lse(v):
            return float(v.max() + np.log(np.exp(v - v.max()).sum())) if v.size else -np.inf
        for name, want in (("lse_all", lse(ref[ok])), ("lse_ts", lse(ref[tb:][ok[tb:]])), ("lse_raw", lse(ref))):
            if np.isfinite(want):
                assert abs(g[name] - want) <= 1e-4 * abs(want), (b, name, g[name], want)
            else:
                assert g[name] == -np.inf, (b, name, g[name])
        assert abs(g["t_v"] - ref[tk.no_speech]) <= 2e-3, (b, g["t_v"], ref[tk.no_speech])
        for key, sel in (("best", ok), ("best_ts", ok & (np.arange(V) >= tb))):
            if not sel.any():
                continue
            cand = np.where(sel, ref, -np.inf)
            top = np.sort(cand)[-2:]
            assert 0 <= g[key] < V, (b, key, g[key])            # never a padded column
            if top[-1] - top[-2] > 2e-3:
                assert g[key] == int(np.argmax(cand)), (b, key, g[key], int(np.argmax(cand)))
                checked += 1
        if ok[:tb].any():
            assert abs(g["m_text"] - ref[:tb][ok[:tb]].max()) <= 2e-3
    assert got[0]["best"] == V - 1                              # the last real id can win
    assert checked >= nrows


def test_vocabulary_projection_padded_columns_never_win(proj_case, gpu):
    """Every logit equal (W is one repeated row, about -30): the first allowed index wins each
    set, no index is a padded column's, and the sums count exactly the V real columns (the
    last tile's 6 padded columns repeat column V - 1; row 0 of the case above, where V - 1
    wins at +40, bounds their leak into the sums far more tightly)."""
    A, _, _, tk, smask, rules = proj_case
    g = torch.Generator().manual_seed(PROJ_SEED + 1)
    row = torch.randn(1280, generator=g).half()
    Wd = row.repeat(V, 1).to(gpu)                               # logits equal over the vocabulary
    A2 = (-row.float() * (30.0 / float((row.float() ** 2).sum()))).half()[None].repeat(3, 1)  # all ~ -30
    free = np.zeros_like(rules[:3])
    free[:, 3] = free[:, 4] = -1
    got = run_projection(gpu, A2, Wd, tk, np.zeros_like(smask), free, [0, 1, 2])
    for r in got:
        assert r["best"] == 0 and r["best_v"] < -20
        assert r["best_ts"] == tk.timestamp_begin
        want = r["best_v"] + np.log(V - 1)                      # (<|notimestamps|> is never allowed)
        assert abs(r["lse_all"] - want) <= 1e-4 * abs(want)
        assert abs(r["lse_raw"] - (r["best_v"] + np.log(V))) <= 1e-4 * abs(want)


def test_vocabulary_projection_sampling_keys(proj_case, gpu):
    """The SAMPLE instantiation at K = 1280: the argmax of logit / T + Gumbel noise (the
    device's own noise, janus_sample_gumbel_f32) over the allowed tokens, 33 rows."""
    A, Wt, L, tk, smask, rules = proj_case
    B = lf.ROW_GROUP + 1
    T, pos = 0.6, 5
    seeds = [7000 + b for b in range(B)]
    got = run_projection(gpu, A, Wt.to(gpu), tk, smask, rules, list(range(B)), inv_temp=1.0 / T, seeds=seeds,
                         pos=pos)
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu)
    noise = torch.empty(B, V, dtype=torch.float32, device=gpu)
    nat.call("janus_sample_gumbel_f32", sd.data_ptr(), B, pos, V, noise.data_ptr(), nat.stream_ptr())
    noise = noise.cpu().numpy().astype(np.float64)
    inv = float(np.float32(1.0) / np.float32(T))
    hit = 0
    for b in range(B):
        ok = lf.allowed_mask(V, smask, tuple(rules[b, :4]), tk.eot, tk.blank, tk.timestamp_begin,
                             tk.no_timestamps, 50)
        keys = np.where(ok, L[b] * inv + noise[b], -np.inf)
        top = np.sort(keys)[-2:]
        if top[-1] - top[-2] > 2e-3 / T:
            assert got[b]["best"] == int(np.argmax(keys)), b
            hit += 1
    assert hit >= B - 2


# ------------------------------------------------------------------ 6. detect_language
def test_detect_language_100(cut, gpu):
    """1 and 3 windows: probabilities over the 100 languages against the rule restated on the
    oracle, DETECT_BOUND relative; the 3-window call's first row is the 1-window call. With
    <|yue|>'s embedding row set to twice the winner's (its logit there is positive), yue — the
    100th language — wins on the reference and on the GPU."""
    eng, W = cut
    tk = eng.tokenizer
    enc_np = beam_ref.rand_enc(CUT, [930, 931, 932])
    p_ref, b_ref, gap = lf.language_probs(enc_np, W, CUT, tk)
    assert (gap >= 2e-2).all(), gap
    enc = torch.from_numpy(enc_np).half().to(gpu)
    p3, b3 = eng.detect_language(enc)
    p1, b1 = eng.detect_language(enc[:1].contiguous())
    torch.cuda.synchronize()
    assert p3.shape == (3, 100) and p1.shape == (1, 100)
    assert torch.equal(p1[0], p3[0]) and torch.equal(b1, b3[:1])
    assert np.array_equal(b3.cpu().numpy(), b_ref)
    p = p3.cpu().numpy().astype(np.float64)
    assert np.abs(p.sum(1) - 1).max() < 1e-5
    err = float((np.abs(p - p_ref) / np.maximum(p_ref, 1e-6)).max())
    print(f"detect_language over 100 languages: rel err {err:.3e}, gaps {np.round(gap, 3)}")
    assert err <= DETECT_BOUND, err
    # yue reachable
    a = tk.language_begin + int(b_ref[0])
    L = mr.language_logits(enc_np[:1], W, CUT, tk)
    assert L[0, int(b_ref[0])] > 1.0
    E = W["decoder.embed_tokens.weight"].copy()
    E[tk.language_token("yue")] = 2 * E[a]
    assert np.array_equal(E.astype(np.float16).astype(np.float32), E)
    W2 = dict(W)
    W2["decoder.embed_tokens.weight"] = E
    _, by, gy = lf.language_probs(enc_np[:1], W2, CUT, tk)
    assert tk.languages[int(by[0])] == "yue" and gy[0] > 1.0
    try:
        eng.set_tensor("decoder.embed_tokens.weight", E)
        py, bg = eng.detect_language(enc[:1].contiguous())
        assert int(bg[0]) == 99 and float(py[0, 99]) > 0.5
    finally:
        eng.set_tensor("decoder.embed_tokens.weight", W["decoder.embed_tokens.weight"])


# ------------------------------------------------------------------ 7. the seek loop
def test_seek_loop_detects_and_translates(cut, gpu):
    """generate_segments on a 35 s and a 4 s utterance, language=None, task="translate",
    max_length 24, temperatures (0.0, 0.4): the detected languages are the reference's; the
    windows, segments and counters equal oracle.transcribe_segments run with the detected
    language's translate prompt. (The oracle reads its no-speech figure from the *.en id at the
    first sampled step; on these weights both readings are ~1e-5, far from the 0.6 gate, which
    the test asserts on the GPU side.) A window whose tokens differ must differ first at an
    oracle top-2 margin < NEAR_TIE."""
    from janus_amd.services.transcriber import generate_segments
    eng, W = cut
    tk = eng.tokenizer
    F = mel_filters(n_mels=128)
    auds = [synth_speech(170, 35.0, sr=16000).astype(np.float32),
            synth_speech(171, 4.0, sr=16000).astype(np.float32)]
    temps = (0.0, 0.4)
    streams = generate_segments(eng, auds, max_length=24, temperatures=temps, language=None, task="translate")
    assert streams[0].windows >= 2
    for i, (a, st) in enumerate(zip(auds, streams)):
        feats = ow.logmel(a, 1, F, n_frames=None)
        enc0 = ow.encoder(ow.window(feats, 0)[None], W, CUT).half().float().numpy()
        p_ref, best, gap = lf.language_probs(enc0, W, CUT, tk)
        code = tk.languages[int(best[0])]
        assert gap[0] >= 2e-2, gap
        assert st.language == code, (st.language, code)
        print(f"utterance {i}: language probability {st.language_probability:.5f}, reference "
              f"{p_ref[0].max():.5f} (its own front end and encoder)")
        tki = tok.WhisperTokenizer(n_vocab=V, language=code, task="translate")
        assert tki.sot_sequence == [tk.sot, tk.language_token(code), tk.translate]
        ref, cnt = ow.transcribe_segments(a, W, CUT, tki, F, max_length=24, temperatures=temps, utt=i)
        got = [(s.start, s.end, s.text, list(s.tokens)) for s in st.segments]
        print(f"utterance {i}: language {code}, {st.windows} windows, {len(got)} segments, "
              f"{st.fallback_decodes} fallback decodes")
        assert st.windows == cnt["windows"] and st.skips == cnt["skips"] == 0
        if [g[3] for g in got] != [r[3] for r in ref]:
            # the near-tie rule: some window of the oracle's own loop has a T = 0 step whose
            # top-2 margin is below NEAR_TIE (a sampled step's near tie does not excuse it)
            mins = []
            for seek, size, prompt in cnt["trace"]:
                enc = ow.encoder(ow.window(feats, seek)[None], W, CUT).half().float().numpy()
                mins.append(min(mr.greedy(enc, W, CUT, tki, [prompt], 24)[0]["margins"]))
            assert min(mins) < NEAR_TIE, (i, mins)
            continue
        assert st.fallbacks == cnt["needs_fallback"] and st.fallback_decodes == cnt["fallback_decodes"]
        assert [g[2] for g in got] == [r[2] for r in ref]
        assert np.allclose([g[:2] for g in got], [r[:2] for r in ref])
    assert eng.decode_path().persistent == 0


# ------------------------------------------------------------------ 8. fusion flags
@pytest.mark.parametrize("flags", [DEC_PATH_NO_CVP, DEC_PATH_CVP, DEC_PATH_NO_EMBED_LN, DEC_PATH_LN_FUSE,
                                   DEC_PATH_RESID_LN, dec_path_ln_mask(15), dec_path_ln_mask(0)],
                         ids=["no_cvp", "cvp", "no_embed_ln", "ln_fuse", "resid_ln", "mask15", "mask0"])
def test_fusion_flags_change_nothing_at_1280(cut, greedy_ref, gpu, flags):
    """Every launch-path fusion is guarded by d <= 512: at 1280 each flag decodes the default's
    bits and none raises."""
    eng, _ = cut
    enc_np, prompts, _, _ = greedy_ref
    enc = torch.from_numpy(enc_np[:3]).half().to(gpu)
    a = eng.decode_ex(enc, prompts=prompts[:3], max_length=16)
    b = eng.decode_ex(enc, prompts=prompts[:3], max_length=16, path_flags=flags)
    torch.cuda.synchronize()
    for f in ("tokens", "n_tokens", "sum_logprob", "no_speech_prob"):
        assert torch.equal(getattr(a, f).cpu(), getattr(b, f).cpu()), f


def test_second_tier_is_refused_before_gpu_work(cut, gpu):
    eng, _ = cut
    enc = torch.zeros(1, 1500, 1280, dtype=torch.float16, device=gpu)
    with pytest.raises(NotImplementedError, match="beam_size"):
        eng.decode_beam(enc, beam_size=4, max_length=16)
    with pytest.raises(NotImplementedError, match="word_timestamps"):
        eng.align(enc, [[300, 400]], [3000])


# ------------------------------------------------------------------ 9. cross-attention alone
XATTN_CASES = [(1, 1500, 1), (1, 1500, 8), (2, 1500, 3), (2, 141, 1), (17, 141, 3), (17, 77, 8), (2, 33, 1),
               (2, 32, 1), (1, 1500, 17)]


@pytest.mark.parametrize("B,Te,nsplit", XATTN_CASES, ids=[f"{b}rows-{t}keys-{n}" for b, t, n in XATTN_CASES])
def test_cross_attention_absorbed_1280(gpu, B, Te, nsplit):
    """xattn_kernel<1280, 32, .., HG = 10> (two head-group blocks per (split, row) in grid.z, each
    on 10 of its 16 MFMA rows) and the 20-head merge through janus_cross_attention_f16:
    softmax_2(qk_h . enc^T) . enc per head against the float64 torch reference of the same fp16
    operands, XATTN_TOL overall and 2 XATTN_TOL on every one of the 20 heads of every row; the
    worst head of group 0 (heads 0 - 9) and of group 1 (10 - 19) is printed on its own. At this
    width one split is the split kernel plus the merge too (no DIRECT form). Key counts 1500 (46
    chunks of 32 + 28), 141 and 77 (ragged last chunks; 77 keys at 8 splits leaves splits without
    keys), 33 (one key past a chunk) and 32 (exactly one); 17 splits is more than 16 through
    xattn_combine_kernel<20>, the only merge at this width. The 17-row cases index two encoder
    rows by gathered copy, and rows over the same encoder row with the same query must come out
    bit-identical. The partials are filled with NaN before the call: a slot the merge reads that
    no block wrote (an empty split, the second group's offset) poisons the output. The entry
    rejected none of the key counts."""
    D, H, HG = 1280, 20, 10
    g = torch.Generator().manual_seed(B * 1000 + Te + D + nsplit)
    n_enc = min(B, 2)
    enc_rows = torch.randn(n_enc, Te, D, generator=g).half()
    idx = [b % n_enc for b in range(B)]
    enc = enc_rows[idx].contiguous()                      # the gather of shared rows
    qk = (torch.randn(B, H, D, generator=g) * 0.15).half()
    if B >= 4:
        qk[2] = qk[0]                                     # same query, same encoder row (0)
    s = torch.einsum("bhd,btd->bht", qk.double(), enc.double())
    p = torch.softmax(s * math.log(2.0), dim=-1)
    ref = torch.einsum("bht,btd->bhd", p, enc.double()).reshape(B, H * D)
    dq, de = qk.to(gpu), enc.to(gpu)
    pc = torch.full((B * nsplit * H * D,), float("nan"), dtype=torch.float32, device=gpu)
    pml = torch.full((B * nsplit * H * 2,), float("nan"), dtype=torch.float32, device=gpu)
    out = torch.full((B, H * D), float("nan"), dtype=torch.float16, device=gpu)
    nat.call("janus_cross_attention_f16", dq.data_ptr(), de.data_ptr(), B, Te, D, H, nsplit,
             pc.data_ptr(), pml.data_ptr(), out.data_ptr(), nat.stream_ptr())
    torch.cuda.synchronize()
    got = out.double().cpu()
    err = float((got - ref).norm() / ref.norm())
    heads = (got - ref).view(B, H, D).norm(dim=-1) / ref.view(B, H, D).norm(dim=-1)      # [B][20]
    g0, g1 = float(heads[:, :HG].max()), float(heads[:, HG:].max())
    b_, h_ = divmod(int(torch.nan_to_num(heads, nan=float("inf")).argmax()), H)
    print(f"xattn 1280 / 20: {B} rows, {Te} keys, {nsplit} splits: rel {err:.2e}, worst head of group 0 "
          f"{g0:.2e}, of group 1 {g1:.2e} (row {b_} head {h_})")
    assert bool(torch.isfinite(got).all()), f"non-finite output, first at row {b_} head {h_}"
    assert err < XATTN_TOL, err
    assert max(g0, g1) < 2 * XATTN_TOL, f"row {b_} head {h_} (group {h_ // HG}): {max(g0, g1):.2e}"
    if B >= 4:
        assert torch.equal(out[2], out[0])


# ------------------------------------------------------------------ 10. decoder residual stream
ENC_INDEX = [0] * 5 + [1] * 5 + [2] * 3
GATHERED = 2                        # call.enc_rows (tests/test_decoder_hidden_gpu.py)
DEFECT_NAME, DEFECT_COL = "decoder.layers.1.fc2.bias", 1264      # the last of the 80 tiles
WIDE_PLAN = dict(persist=0, xabs=1, wide=1, npairs=0, ngroups=0, fused_ln=0, ln_fuse=0, rln=0, ln_pro_mask=0,
                 cvp=0, xsplit=3)


@functools.lru_cache(maxsize=None)
def hidden_case(rows=65, T=5):
    """tests/test_decoder_hidden_gpu.py's model at 1280 / 20: two decoder layers, 64 vocabulary
    entries, 141 encoder keys; rows x T positions of forced tokens and their float64 references
    (exact and emulated), computed once per shape. CPU only."""
    cfg = dref.config(1280, 20, 141)
    W = dref.weights(cfg, 3)
    tokens, enc = dref.inputs(cfg, rows, T, 5)
    exact = dref.hidden(tokens, enc, W, cfg)
    emu = dref.hidden(tokens, enc, W, cfg, emulate=True)
    return cfg, W, tokens, enc, exact, emu


@functools.lru_cache(maxsize=None)
def shared_case():
    """13 rows over the first 3 encoder rows of hidden_case() (5 + 5 + 3), 3 positions. CPU only."""
    cfg, W, tokens, enc, _, _ = hidden_case()
    B, T = len(ENC_INDEX), 3
    exact = dref.hidden(tokens[:B, :T], enc[:3], W, cfg, enc_index=ENC_INDEX)
    emu = dref.hidden(tokens[:B, :T], enc[:3], W, cfg, enc_index=ENC_INDEX, emulate=True)
    return tokens[:B, :T], exact, emu


@functools.lru_cache(maxsize=None)
def defect_case():
    """17 rows x 3 positions of hidden_case() with fc2's bias of layer 1 zeroed on columns
    1264 .. 1279: (tokens, clean x, the tile bound, the defective reference's worst column and
    tile). The reference alone must separate the two by the margin the GPU test asks of the
    engine — asserted here, on the CPU, before any GPU work."""
    cfg, W, tokens, enc, exact, emu = hidden_case()
    B, T = 17, 3
    rx, ex = exact[0][:B, :T], emu[0][:B, :T]
    bound = dref.K_BOUND * dref.metrics(ex, rx)[1]
    bad, _, _ = dref.hidden(tokens[:B, :T], enc[:B], W, cfg, defect="fc2_bias", layer=1, col0=DEFECT_COL)
    _, col, tile = dref.worst(bad, rx)
    print(f"reference defect at 1280: tile {tile:.2e} = {tile / bound:.1f}x the bound {bound:.2e} at columns "
          f"{col}-{col + 15}")
    assert col == DEFECT_COL and tile > 3 * bound, (col, tile, bound)
    return tokens[:B, :T], rx, bound, col, tile


@pytest.fixture(scope="module")
def hidden_engine(gpu):
    """The engine of hidden_case()'s model (one for every shape: the weights depend on the
    config and seed alone) and the cases' encoder rows on the device."""
    cfg, W = hidden_case()[:2]
    eng = WhisperEngine(cfg, W)
    on_dev = {}

    def enc_dev(rows, T, n):
        if (rows, T) not in on_dev:
            on_dev[rows, T] = torch.from_numpy(hidden_case(rows, T)[3]).to(gpu)
        return on_dev[rows, T][:n].contiguous()

    return eng, enc_dev


def hold_hidden(name, out, T, exact, emu):
    """x and the caches of a decode_hidden result against the references, row and tile metric,
    bound K_BOUND x the emulation's own distance; a failure names the worst tile."""
    got = (out.x.transpose(0, 1), out.kc[:, :, :T], out.vc[:, :, :T])
    for what, g, r, e in zip(("x", "k cache", "v cache"), got, exact, emu):
        g = g.double().cpu().numpy()
        e_row, e_tile = dref.metrics(e, r)
        g_row, g_tile = dref.metrics(g, r)
        print(f"hidden 1280 {name} {what}: row {g_row:.2e} tile {g_tile:.2e} | emulation row {e_row:.2e} "
              f"tile {e_tile:.2e}")
        at, col, val = dref.worst(g, r)
        where = f"{name} {what} index {at} (x: row, position; cache: layer, row, slot), columns {col}-{col + 15}"
        assert np.isfinite(g_tile) and g_tile <= dref.K_BOUND * e_tile, \
            f"{where}: tile {val:.2e} is {val / (dref.K_BOUND * e_tile):.1f}x the bound {dref.K_BOUND * e_tile:.2e}"
        assert g_row <= dref.K_BOUND * e_row, \
            f"{where}: row {g_row:.2e} is {g_row / (dref.K_BOUND * e_row):.1f}x the bound {dref.K_BOUND * e_row:.2e}"


HIDDEN_CASES = [(1, 5, 65, 5), (17, 5, 65, 5), (65, 5, 65, 5), (17, 70, 17, 70)]


@pytest.mark.parametrize("B,T,rows,Tc", HIDDEN_CASES, ids=[f"rows{c[0]}-T{c[1]}" for c in HIDDEN_CASES])
def test_decoder_residual_stream_1280(hidden_engine, B, T, rows, Tc):
    """x after every position and the K / V caches of the launch path at 1, 17 and 65 rows over 5
    positions (one row, a ragged m-tile, past 64 rows) and at 17 rows over 70 (the decode
    attention crosses its 64-key round at 20 heads: NR 1 -> 2 inside the call) against
    decoder_ref.hidden(), row and tile metric, bound K_BOUND x the emulation's own distance on
    the case's rows (tests/test_decoder_hidden_gpu.py). The plan that ran must be the wide launch
    path with the absorbed cross-attention, every row on its own encoder row."""
    eng, enc_dev = hidden_engine
    _, _, tokens, _, exact, emu = hidden_case(rows, Tc)
    out = eng.decode_hidden(enc_dev(rows, Tc, B), tokens[:B, :T])
    want = dict(WIDE_PLAN, B=B, **{"call.enc_rows": 0})
    assert {k: out.plan[k] for k in want} == want, out.plan
    cut_ = lambda r: (r[0][:B, :T], r[1][:, :B, :T], r[2][:, :B, :T])
    hold_hidden(f"rows{B} T{T}", out, T, cut_(exact), cut_(emu))


def test_decoder_residual_stream_1280_shared_rows(hidden_engine):
    """13 rows over 3 encoder rows (5 + 5 + 3), 3 positions: no in-place blocks at 20 heads, the
    plan must say the rows took gathered copies; row b against hidden() on enc[enc_index[b]]."""
    eng, enc_dev = hidden_engine
    tokens, exact, emu = shared_case()
    B = len(ENC_INDEX)
    out = eng.decode_hidden(enc_dev(65, 5, 3), tokens, enc_index=ENC_INDEX)
    want = dict(WIDE_PLAN, B=B, **{"call.enc_rows": GATHERED})
    assert {k: out.plan[k] for k in want} == want, out.plan
    hold_hidden("shared rows", out, 3, exact, emu)


def test_engine_defect_is_seen_1280(hidden_engine):
    """The comparison end to end at 1280: an engine whose fc2 bias of layer 1 is zeroed on the
    last tile (columns 1264 .. 1279, one of 80) lies more than 3x over the bound against the
    clean reference, at exactly that tile — as the reference with the same defect does
    (defect_case(), asserted on the CPU first) — and the restored engine is inside the bound."""
    tokens, rx, bound, _, _ = defect_case()
    eng, enc_dev = hidden_engine
    W = hidden_case()[1]
    B = len(tokens)
    bad = W[DEFECT_NAME].copy()
    bad[DEFECT_COL:DEFECT_COL + 16] = 0.0
    eng.set_tensor(DEFECT_NAME, bad)
    try:
        out = eng.decode_hidden(enc_dev(65, 5, B), tokens)
    finally:
        eng.set_tensor(DEFECT_NAME, W[DEFECT_NAME])
    assert {k: out.plan[k] for k in WIDE_PLAN} == WIDE_PLAN, out.plan
    _, col, tile = dref.worst(out.x.transpose(0, 1).double().cpu().numpy(), rx)
    print(f"engine defect at 1280: tile {tile:.2e} = {tile / bound:.1f}x the bound at columns {col}-{col + 15}")
    assert col == DEFECT_COL and tile > 3 * bound, (col, tile, bound)
    clean = eng.decode_hidden(enc_dev(65, 5, B), tokens)
    _, col, tile = dref.worst(clean.x.transpose(0, 1).double().cpu().numpy(), rx)
    print(f"restored engine: worst tile {tile:.2e} = {tile / bound:.2f}x the bound at columns {col}-{col + 15}")
    assert tile <= bound, (col, tile, bound)
