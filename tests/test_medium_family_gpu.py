"""The 1024-wide, 16-head family (medium.en, distil-medium.en) on the GPU against the unchanged
oracle (oracle/whisper.py), tests/decoder_ref.py, tests/align_ref.py, tests/history_ref.py and
tests/medium_family_ref.py. Every test runs the cut config — the real width, heads, 80 mel bins
and the 51 864-entry vocabulary over 2 encoder and 2 decoder layers, synthetic weights (seed 11)
— or a kernel alone, so each takes seconds.

Tolerances are the project's: ENC_TOL (encoder, relative RMS), NEAR_TIE (a free-running decode
may leave the oracle's only where the oracle's own top-2 margin is below it), the sum_logprob /
no_speech_prob bounds of tests/test_small_family_gpu.py, the cross-attention bound of
tests/test_kernels_gpu.py (3e-3), K_BOUND of tests/decoder_ref.py, the projection bounds of
tests/test_large_family_gpu.py and ALIGN_E_A / ALIGN_E_P_REL of tests/test_align_gpu.py.

Seeds, chosen on the CPU oracle alone (W = synthetic_weights(CUT, 11)):
* greedy rows: encoder seeds 900, 901, 902, 908, 904 with the five prompts of
  medium_family_ref.greedy_prompts(); the oracle's smallest top-2 margins over 31 steps are
  5.7e-2, 9.1e-2, 3.9e-2, 4.9e-2, 4.0e-2 (>= 1e-2 = 5 x NEAR_TIE; 903 under the fourth prompt
  has 6.6e-3 and was passed over);
* sampled rows (T = 0.6, encoder seed 920): noise seeds 3001, 3006, 3007, 3010, 3017, smallest
  key margins 4.4e-2, 9.6e-2, 4.4e-2, 1.4e-1, 2.0e-1 (10 x NEAR_TIE / T is 3.3e-2);
* seek loop: synth_speech seeds 170 (35 s, two windows, T = 0 margins 2.2e-1 and 8.6e-2) and
  181 (4 s, 1.2e-1).

Measured on an MI355X (printed by the tests, pytest -s): see DESIGN.md §5q."""
import functools
import math

import numpy as np
import pytest
import torch

import align_ref
import beam_ref
import decoder_ref as dref
import history_ref as hr
import medium_family_ref as mf
import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd.services import transcriber as tr
from janus_amd.whisper import (DEC_PATH_CVP, DEC_PATH_LN_FUSE, DEC_PATH_NO_CVP, DEC_PATH_NO_EMBED_LN,
                               DEC_PATH_RESID_LN, WhisperEngine, dec_path_ln_mask, mel_filters)
from janus_amd.workload import synth_speech
from oracle import whisper as ow

pytestmark = pytest.mark.gpu
CUT = mf.CUT
V = mf.V
RG = mf.ROW_GROUP
NEAR_TIE = 2e-3
ENC_TOL = 1e-3
NSP_REL = 5e-3
XATTN_TOL = 3e-3                    # tests/test_kernels_gpu.py::test_cross_attention_absorbed
ALIGN_E_A = 4 * 7.6e-3              # tests/test_align_gpu.py
ALIGN_E_P_REL = 4 * 3.3e-3
ML = mf.ML
TK = tok.WhisperTokenizer()
SOT = len(TK.sot_sequence)


@pytest.fixture(scope="module")
def cut(gpu):
    W = mf.weights()
    eng = WhisperEngine(CUT, W)
    tk = eng.tokenizer
    assert tk.n_vocab == V and tk.timestamp_begin == 50363 and not tk.multilingual
    return eng, W


def pack(utts, dev):
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    return pcm, offs


# ------------------------------------------------------------------ 1. the vocabulary projection
PROJ_SEED = 4200


@pytest.fixture(scope="module")
def proj_case(gpu):
    """A [49][1024], W [51864][1024] in fp16 (one generator), the float64 product, the suppress
    mask and per-row rule states that exercise the first-token rule, the timestamp floor, text
    suppression and timestamp suppression."""
    g = torch.Generator().manual_seed(PROJ_SEED)
    B = RG + 1
    A = torch.randn(B, 1024, generator=g).half()
    Wt = (0.05 * torch.randn(V, 1024, generator=g)).half()
    # the last real id wins row 0 by construction: its row along A[0] (logit ~ 40)
    Wt[V - 1] = (A[0].float() * (40.0 / float((A[0].float() ** 2).sum()))).half()
    L = A.double().numpy() @ Wt.double().numpy().T          # float64 [49][V]
    smask = np.zeros((V + 15) // 16 * 16, np.uint8)
    smask[TK.suppress_tokens()] = 1
    rules = np.zeros((B, 8), np.int32)
    rules[:, 3] = rules[:, 4] = -1
    for b in range(B):
        kind = b % 4
        if kind == 1:      # first sampled token: timestamps up to max_initial only, no blank / eot
            rules[b, 0] = 1
        elif kind == 2:    # after text + timestamp: text banned, timestamps from the floor
            rules[b, 2] = 1
            rules[b, 3] = TK.timestamp_begin + 100
        elif kind == 3:    # after two timestamps: every timestamp banned
            rules[b, 1] = 1
            rules[b, 3] = TK.timestamp_begin + 7
    return A, Wt.to(gpu), L, smask, rules


def run_projection(gpu, A, Wd, smask, rules, rows, inv_temp=0.0, seeds=None, pos=5, words=None, pen=1.0):
    """The partials of janus_logits_partial_f16 (words None) or the HIST entry, merged per row."""
    B = len(rows)
    Ad = A[rows].contiguous().to(gpu)
    sm = torch.from_numpy(smask).to(gpu)
    rr = torch.from_numpy(np.ascontiguousarray(rules[rows])).to(gpu)
    nblk = nat.lib().janus_beam_partial_blocks(V, 1024, 256)
    parts = torch.zeros(B * nblk * 56, dtype=torch.uint8, device=gpu)
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu) if seeds is not None else None
    args = [Ad.data_ptr(), Wd.data_ptr(), 1024, V, B, TK.eot, 1, TK.blank, TK.timestamp_begin, TK.no_timestamps,
            50, TK.no_speech, sm.data_ptr(), rr.data_ptr(), 256, float(inv_temp),
            sd.data_ptr() if sd is not None else None, pos, parts.data_ptr()]
    if words is None:
        nat.call("janus_logits_partial_f16", *args, nat.stream_ptr())
    else:
        assert words.numel() == nat.lib().janus_history_words(V, 1024, B)
        nat.call("janus_logits_partial_hist_f16", *args, words.data_ptr(), float(pen), nat.stream_ptr())
    torch.cuda.synchronize()
    return mf.merge_parts(parts.cpu().numpy().view(mf.PART_DTYPE).reshape(B, nblk))


def lse(v):
    return float(v.max() + np.log(np.exp(v - v.max()).sum())) if v.size else -np.inf


def check_projection_row(b, g, ref, ok, raw=None):
    """One row of merged partials against float64 logits ``ref`` under the allowed mask ``ok``
    (``raw``: the unpenalised logits the raw statistics are taken on). Returns the number of
    argmax decisions that were clear enough (margin > 2e-3) to be compared."""
    raw = ref if raw is None else raw
    tb = TK.timestamp_begin
    for name, want in (("lse_all", lse(ref[ok])), ("lse_ts", lse(ref[tb:][ok[tb:]])), ("lse_raw", lse(raw))):
        if np.isfinite(want):
            assert abs(g[name] - want) <= 1e-4 * abs(want), (b, name, g[name], want)
        else:
            assert g[name] == -np.inf, (b, name, g[name])
    assert abs(g["t_v"] - raw[TK.no_speech]) <= 2e-3, (b, g["t_v"], raw[TK.no_speech])
    checked = 0
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
    return checked


@pytest.mark.parametrize("nrows", [1, 17, RG - 1, RG, RG + 1])
def test_vocabulary_projection_1024(proj_case, gpu, nrows):
    """K = 1024, V = 51 864 (the last tile holds 8 columns) at 1, 17 and 47 / 48 / 49 rows — the
    48-row group's boundary — against the float64 product of the same fp16 operands: per row the
    filtered log-sum-exps (all, timestamps) and the raw one within 1e-4 relative, the largest
    allowed text logit, the argmax over the allowed tokens and over the allowed timestamps
    wherever the reference margin exceeds 2e-3, and the no-speech logit."""
    A, Wd, L, smask, rules = proj_case
    rows = list(range(nrows))
    got = run_projection(gpu, A, Wd, smask, rules, rows)
    checked = 0
    worst = 0.0
    for b in rows:
        ok = mf.allowed_mask(V, smask, tuple(rules[b, :4]), TK.eot, TK.blank, TK.timestamp_begin,
                             TK.no_timestamps, 50)
        checked += check_projection_row(b, got[b], L[b], ok)
        worst = max(worst, abs(got[b]["lse_all"] - lse(L[b][ok])) / abs(lse(L[b][ok])))
    print(f"projection K 1024, {nrows} rows: worst relative log-sum-exp error {worst:.2e}")
    assert got[0]["best"] == V - 1                              # the last real id can win
    assert checked >= nrows


def test_vocabulary_projection_padded_columns_stay_out(proj_case, gpu):
    """Every logit equal (W is one repeated row, about -30): the first allowed index wins each
    set, no index is a padded column's, and the sums count exactly the V real columns. The last
    tile's 8 padded columns repeat column V - 1; counted, they would add log((V + 8) / V) =
    1.5e-4 to the log-sum-exps. With equal logits every exp(v - m) is exactly 1, the sums are
    integer counts (exact in fp32) and the merge of the partials runs in float64, so the
    log-sum-exp is m + log(count) up to rounding: the bound is 5e-5 absolute, a third of what
    the padded columns would add. (Row 0 of the test above pins the same from the other side:
    column V - 1 wins there at +40, and a repeated copy would move the sum by log 9.)"""
    A, _, _, smask, rules = proj_case
    g = torch.Generator().manual_seed(PROJ_SEED + 1)
    row = torch.randn(1024, generator=g).half()
    Wd = row.repeat(V, 1).to(gpu)                               # logits equal over the vocabulary
    A2 = (-row.float() * (30.0 / float((row.float() ** 2).sum()))).half()[None].repeat(3, 1)  # all ~ -30
    free = np.zeros_like(rules[:3])
    free[:, 3] = free[:, 4] = -1
    got = run_projection(gpu, A2, Wd, np.zeros_like(smask), free, [0, 1, 2])
    assert np.log((V + 8) / V) > 1.5e-4
    for r in got:
        assert r["best"] == 0 and r["best_v"] < -20
        assert r["best_ts"] == TK.timestamp_begin
        e_all = abs(r["lse_all"] - (r["best_v"] + np.log(V - 1)))     # (<|notimestamps|> is never allowed)
        e_raw = abs(r["lse_raw"] - (r["best_v"] + np.log(V)))
        e_ts = abs(r["lse_ts"] - (r["best_ts_v"] + np.log(V - TK.timestamp_begin)))
        print(f"equal logits: |lse - (m + log count)| all {e_all:.1e} raw {e_raw:.1e} timestamps {e_ts:.1e}")
        assert e_all <= 5e-5 and e_raw <= 5e-5 and e_ts <= 5e-5, (e_all, e_raw, e_ts)


@pytest.mark.parametrize("nrows", [1, 17, RG - 1, RG, RG + 1])
def test_vocabulary_projection_sampling_keys(proj_case, gpu, nrows):
    """The SAMPLE instantiation at K = 1024: the argmax of logit / T + oracle.whisper.sample_noise
    (seed, position) over the allowed tokens; a row whose two best keys are closer than
    NEAR_TIE / T is not compared (at most two of 49)."""
    A, Wd, L, smask, rules = proj_case
    T, pos = 0.6, 5
    rows = list(range(nrows))
    seeds = [7000 + b for b in rows]
    got = run_projection(gpu, A, Wd, smask, rules, rows, inv_temp=1.0 / T, seeds=seeds, pos=pos)
    inv = float(np.float32(1.0) / np.float32(T))
    hit = 0
    for b in rows:
        ok = mf.allowed_mask(V, smask, tuple(rules[b, :4]), TK.eot, TK.blank, TK.timestamp_begin,
                             TK.no_timestamps, 50)
        keys = np.where(ok, L[b] * inv + ow.sample_noise(seeds[b], pos, V), -np.inf)
        top = np.sort(keys)[-2:]
        if top[-1] - top[-2] > NEAR_TIE / T:
            assert got[b]["best"] == int(np.argmax(keys)), b
            hit += 1
    assert hit >= nrows - 2 and hit >= 1


def test_vocabulary_projection_history_rules(proj_case, gpu):
    """HIST at K = 1024, p = 1.2, n = 3, 49 rows: the history words come from janus_history_rules
    over token rows whose 3-grams repeat ([group of 48][tile][row] layout), the projection
    against tests/history_ref.py's penalise / banned on the float64 logits. Every row's history
    holds its own unpenalised winner, so the penalty moves or lowers it."""
    A, Wd, L, smask, rules = proj_case
    p, n, B, ld = 1.2, 3, RG + 1, 12
    rows = list(range(B))
    plain = run_projection(gpu, A, Wd, smask, rules, rows)
    rng = np.random.default_rng(61)
    tokens = np.zeros((B, ld), np.int32)
    plens = (1 + np.arange(B) % 3).astype(np.int32)
    for b in rows:
        ok = mf.allowed_mask(V, smask, tuple(rules[b, :4]), TK.eot, TK.blank, TK.timestamp_begin,
                             TK.no_timestamps, 50)
        second = int(np.argsort(np.where(ok, L[b], -np.inf))[-2])
        # x y <second> ... x y: the 3-gram rule bans the runner-up; the winner and V - 1 are penalised
        alphabet = [plain[b]["best"], V - 1, 5, TK.timestamp_begin + 37]
        g = [int(t) for t in rng.choice(alphabet, ld)]
        g[-6:] = [plain[b]["best"], 17, 31, second, 17, 31]
        tokens[b] = g
    nwords = nat.lib().janus_history_words(V, 1024, B)
    words = torch.zeros(nwords, dtype=torch.int32, device=gpu)
    td, pd = torch.from_numpy(tokens).to(gpu), torch.from_numpy(plens).to(gpu)
    nat.call("janus_history_rules", td.data_ptr(), ld, B, pd.data_ptr(), n, V, 1024, 0, ld, words.data_ptr(),
             nat.stream_ptr())
    got = run_projection(gpu, A, Wd, smask, rules, rows, words=words, pen=p)
    checked = moved = 0
    for b in rows:
        g = [int(t) for t in tokens[b][plens[b]:]]
        ban = hr.banned(g, n)
        assert ban, b
        ok = mf.allowed_mask(V, smask, tuple(rules[b, :4]), TK.eot, TK.blank, TK.timestamp_begin,
                             TK.no_timestamps, 50)
        ok[ban] = False
        Lp = hr.penalise(L[b], g, p).astype(np.float64)     # (fp32: 2e-6 on a logit of 40, far inside 2e-3)
        assert got[b]["best"] not in ban
        checked += check_projection_row(b, got[b], Lp, ok, raw=L[b])
        moved += int(got[b]["best"] != plain[b]["best"] or got[b]["best_v"] < plain[b]["best_v"])
    assert checked >= B and moved >= B // 2, (checked, moved)


# ------------------------------------------------------------------ 2. cross-attention alone
@pytest.mark.parametrize("B,Te,nsplit", [(1, 1500, 1), (1, 1500, 8), (2, 1500, 3), (2, 141, 1), (17, 141, 3),
                                         (17, 77, 8), (2, 1500, 8)],
                         ids=["1row-1split", "1row-8", "2rows-3", "2rows-141keys-1", "17rows-3", "17rows-77keys-8",
                              "2rows-8"])
def test_cross_attention_absorbed_1024(gpu, B, Te, nsplit):
    """xattn_kernel<1024, 32> (16 heads in one block's MFMA rows) and the 16-head merge through
    janus_cross_attention_f16: softmax_2(qk_h . enc^T) . enc per head against the float64 torch
    reference of the same fp16 operands, the bound of the 768 cases (tests/test_kernels_gpu.py)
    and of tests/test_large_family_gpu.py::test_cross_attention_absorbed_1280 (3e-3). Key counts
    1500 (46 chunks of 32 + 28), 141 and 77 (ragged last chunks; 77 keys at 8 splits leaves
    splits without keys). Rows that share an encoder row reach this kernel as gathered copies
    (`shared_rows_in_place` is false at 16 heads): the 17-row cases index two encoder rows, and
    rows over the same encoder row with the same query must come out bit-identical. The entry
    takes no sweep direction: the reversed key sweep is the D = 512 row-load form's alone, the
    1024 kernel reads its chunks forwards whatever the plan's xrev says (the decode tests below
    run both plans)."""
    D, H = 1024, 16
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
    pc = torch.empty(B * nsplit * H * D, dtype=torch.float32, device=gpu)
    pml = torch.empty(B * nsplit * H * 2, dtype=torch.float32, device=gpu)
    out = torch.empty(B, H * D, dtype=torch.float16, device=gpu)
    nat.call("janus_cross_attention_f16", dq.data_ptr(), de.data_ptr(), B, Te, D, H, nsplit,
             pc.data_ptr(), pml.data_ptr(), out.data_ptr(), nat.stream_ptr())
    torch.cuda.synchronize()
    got = out.double().cpu()
    err = float((got - ref).norm() / ref.norm())
    per_head = float(((got - ref).view(B, H, D).norm(dim=-1) / ref.view(B, H, D).norm(dim=-1)).max())
    print(f"xattn 1024 / 16: {B} rows, {Te} keys, {nsplit} splits: rel {err:.2e}, worst head {per_head:.2e}")
    assert err < XATTN_TOL, err
    assert per_head < 2 * XATTN_TOL, per_head           # no head (MFMA row) is lost in the average
    if B >= 4:
        assert torch.equal(out[2], out[0])


# ------------------------------------------------------------------ 3. encoder
@pytest.mark.parametrize("windows", [1, 2])
def test_encoder_cut(cut, gpu, windows):
    """Conv stem at Cout 1024, the projections at N = 1024 / 3072 / 4096, 16-head attention,
    LayerNorm at 1024: relative RMS <= ENC_TOL, worst row <= 4 ENC_TOL."""
    eng, W = cut
    pcm, offs = pack([synth_speech(300 + k, [30.0, 9.0][k]) for k in range(windows)], gpu)
    mel = eng.logmel(pcm, offs, windows, 3)
    enc = eng.encode(mel)
    torch.cuda.synchronize()
    assert enc.shape == (windows, 1500, 1024)
    ref = ow.encoder(mel.float().cpu().numpy(), W, CUT)
    got = enc.float().cpu()
    rel = float((got - ref).norm() / ref.norm())
    per_row = ((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    print(f"medium-cut, {windows} window(s): encoder rel RMS {rel:.2e}, worst row {per_row:.2e}")
    assert rel <= ENC_TOL and per_row <= 4 * ENC_TOL, (rel, per_row)


# ------------------------------------------------------------------ 4. decoder residual stream
HID_ROWS, HID_T = 65, 5


@functools.lru_cache(maxsize=None)
def hidden_case():
    """tests/test_decoder_hidden_gpu.py's model at 1024 / 16: two decoder layers, 64 vocabulary
    entries, 141 encoder keys; 65 rows x 5 positions of forced tokens and their float64
    references (exact and emulated), computed once."""
    cfg = dref.config(1024, 16, 141)
    W = dref.weights(cfg, 3)
    tokens, enc = dref.inputs(cfg, HID_ROWS, HID_T, 5)
    exact = dref.hidden(tokens, enc, W, cfg)
    emu = dref.hidden(tokens, enc, W, cfg, emulate=True)
    return cfg, W, tokens, enc, exact, emu


@pytest.fixture(scope="module")
def hidden_engine(gpu):
    cfg, W, _, enc, _, _ = hidden_case()
    return WhisperEngine(cfg, W), torch.from_numpy(enc).to(gpu)


@pytest.mark.parametrize("B", [1, 17, 65])
def test_decoder_residual_stream_1024(hidden_engine, B):
    """x after every position and the K / V caches of the launch path at 1, 17 and 65 rows
    (one row, a ragged m-tile, past 64 rows) against decoder_ref.hidden(), row and tile metric,
    bound K_BOUND x the emulation's own distance (tests/test_decoder_hidden_gpu.py). The plan
    that ran must be the wide launch path with the absorbed cross-attention."""
    eng, enc = hidden_engine
    _, _, tokens, _, exact, emu = hidden_case()
    out = eng.decode_hidden(enc[:B].contiguous(), tokens[:B])
    want = dict(B=B, persist=0, xabs=1, wide=1, npairs=0, ngroups=0, fused_ln=0, ln_fuse=0, rln=0, ln_pro_mask=0,
                cvp=0, xsplit=3)
    assert {k: out.plan[k] for k in want} == want, out.plan
    got = (out.x.transpose(0, 1), out.kc[:, :, :HID_T], out.vc[:, :, :HID_T])
    for what, g, r, e in zip(("x", "k cache", "v cache"), got, exact, emu):
        g = g.double().cpu().numpy()
        r, e = (r[:B], e[:B]) if what == "x" else (r[:, :B], e[:, :B])
        e_row, e_tile = dref.metrics(e, r)
        g_row, g_tile = dref.metrics(g, r)
        print(f"hidden 1024 rows{B} {what}: row {g_row:.2e} tile {g_tile:.2e} | emulation row {e_row:.2e} "
              f"tile {e_tile:.2e}")
        assert np.isfinite(g_tile) and g_tile <= dref.K_BOUND * e_tile, (what, g_tile, e_tile)
        assert g_row <= dref.K_BOUND * e_row, (what, g_row, e_row)


# ------------------------------------------------------------------ 5. free-running greedy decode
@pytest.fixture(scope="module")
def greedy_ref(cut):
    """The oracle's greedy decode of the five base rows to ML tokens and their no-speech
    probability at <|startoftranscript|>, computed once for the module."""
    eng, _ = cut
    enc = beam_ref.rand_enc(CUT, mf.GREEDY_SEEDS)
    prompts = mf.greedy_prompts(eng.tokenizer)
    rows, nsp = mf.greedy_rows(enc, prompts)
    for r in rows:
        assert min(r["margins"]) >= 5 * NEAR_TIE          # the oracle alone: every row decidable
    return enc, prompts, rows, nsp


@pytest.mark.parametrize("nrows", [1, 3, RG + 1])
def test_free_running_greedy_decode(cut, greedy_ref, gpu, nrows):
    """1 row, 3 rows (a partial MFMA row tile) and 49 rows (one past the 48-row group of the
    vocabulary projection at K = 1024); row b is base row b mod 5, so prompts of lengths 1, 5,
    1, 1 and 3 (two with a <|startofprev|> prefix) step together. Tokens identical to the
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
    worst_lp = worst_nsp = 0.0
    for b, i in enumerate(idx):
        r, pl = ref[i], len(pr[b])
        assert list(toks[b][:pl]) == pr[b]
        g = [int(t) for t in toks[b][pl:pl + int(nt[b])]]
        worst_nsp = max(worst_nsp, abs(nsp[b] - nsp_ref[i]) / nsp_ref[i])
        assert abs(nsp[b] - nsp_ref[i]) <= NSP_REL * nsp_ref[i] + 1e-12, (b, nsp[b], nsp_ref[i])
        if g == r["tokens"]:
            same += 1
            worst_lp = max(worst_lp, abs(slp[b] - r["sum_lp"]) / abs(r["sum_lp"]))
            assert abs(slp[b] - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]), (b, slp[b], r["sum_lp"])
        else:
            first = mr.first_divergence(g, r["tokens"])
            margin = r["margins"][first] if first is not None and first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE, (b, first, margin)
    print(f"{nrows} rows: {same} identical to the oracle, sum_logprob rel {worst_lp:.2e}, "
          f"no_speech_prob rel {worst_nsp:.2e}")
    assert same >= 0.75 * nrows, (same, nrows)


# ------------------------------------------------------------------ 6. sampled decode
def test_sampled_decode_shares_one_encoder_row(cut, gpu):
    """best_of 5 at T = 0.6 over ONE encoder row (enc_index): the rows take a gathered copy
    each (no in-place blocks at 16 heads — the path report says so) and match the oracle's
    sampler with the same seeds: identical, or first divergence at a key margin < NEAR_TIE / T;
    at most one row diverges."""
    eng, _ = cut
    T, ml = mf.SAMPLE_T, mf.SAMPLE_ML
    enc_np = beam_ref.rand_enc(CUT, [mf.SAMPLE_ENC_SEED])
    enc = torch.from_numpy(enc_np).half().to(gpu)
    out = eng.decode_ex(enc, max_length=ml, temperature=T, seeds=mf.SAMPLE_SEEDS, enc_index=[0] * 5)
    torch.cuda.synchronize()
    assert eng.decode_path().enc_rows == "gathered"
    ref = mf.sampled_rows(enc_np, mf.SAMPLE_SEEDS)
    toks = out.tokens.cpu().numpy()
    same = 0
    for b, r in enumerate(ref):
        assert min(r["margins"]) >= 10 * NEAR_TIE / T       # the oracle alone
        g = [int(t) for t in toks[b][SOT:SOT + int(out.n_tokens[b])]]
        print(f"row {b}: oracle min key margin {min(r['margins']):.2e}, identical {g == r['tokens']}")
        if g == r["tokens"]:
            same += 1
            assert abs(float(out.sum_logprob[b]) - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"])
        else:
            first = mr.first_divergence(g, r["tokens"])
            margin = r["margins"][first] if first is not None and first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE / T, (b, first, margin)
    assert same >= 4, same
    assert len({tuple(t) for t in toks.tolist()}) > 1          # the seeds draw different rows


# ------------------------------------------------------------------ 7. mixed temperatures
def test_mixed_temperatures_equal_separate_calls(cut, greedy_ref, gpu):
    """One call with per-row temperatures (greedy rows beside sampled rows at two temperatures,
    three encoder rows shared through enc_index) equals the separate calls bit for bit."""
    eng, _ = cut
    enc_np = greedy_ref[0]
    enc = torch.from_numpy(enc_np[:3]).half().to(gpu)
    ei = [0, 0, 0, 1, 1, 2, 2, 2]
    temps = [0.0, 0.2, 1.0, 0.0, 0.6, 0.2, 0.0, 1.0]
    seeds = [500 + 7 * b for b in range(len(ei))]
    mix = eng.decode_ex(enc, max_length=24, temperature=temps, seeds=seeds, enc_index=ei)
    got = [t.cpu() for t in (mix.tokens, mix.n_tokens, mix.sum_logprob, mix.no_speech_prob)]
    for T in sorted(set(temps)):
        rows = [b for b in range(len(ei)) if temps[b] == T]
        kw = dict(temperature=T, seeds=[seeds[b] for b in rows]) if T > 0 else {}
        ref = eng.decode_ex(enc, max_length=24, enc_index=[ei[b] for b in rows], **kw)
        want = [t.cpu() for t in (ref.tokens, ref.n_tokens, ref.sum_logprob, ref.no_speech_prob)]
        for g, w_ in zip(got, want):
            assert torch.equal(g[rows], w_), T


# ------------------------------------------------------------------ 8. flags change nothing
@pytest.mark.parametrize("kw", [dict(path_flags=DEC_PATH_NO_CVP), dict(path_flags=DEC_PATH_CVP),
                                dict(path_flags=DEC_PATH_NO_EMBED_LN), dict(path_flags=DEC_PATH_LN_FUSE),
                                dict(path_flags=DEC_PATH_RESID_LN), dict(path_flags=dec_path_ln_mask(15)),
                                dict(path_flags=dec_path_ln_mask(0)), dict(persistent=2), dict(persistent=3)],
                         ids=["no_cvp", "cvp", "no_embed_ln", "ln_fuse", "resid_ln", "mask15", "mask0",
                              "persistent2", "persistent3"])
def test_flags_change_nothing_at_1024(cut, greedy_ref, gpu, kw):
    """Every launch-path fusion is guarded by d <= 512 and a persistent request takes the launch
    path: at 1024 each decodes the default's bits, none raises, decode_path() reports level 0."""
    eng, _ = cut
    enc_np, prompts, _, _ = greedy_ref
    enc = torch.from_numpy(enc_np[:3]).half().to(gpu)
    a = eng.decode_ex(enc, prompts=prompts[:3], max_length=16)
    b = eng.decode_ex(enc, prompts=prompts[:3], max_length=16, **kw)
    torch.cuda.synchronize()
    assert eng.decode_path().persistent == 0
    for f in ("tokens", "n_tokens", "sum_logprob", "no_speech_prob"):
        assert torch.equal(getattr(a, f).cpu(), getattr(b, f).cpu()), f


# ------------------------------------------------------------------ 9. the seek loop
def cut_model(eng):
    """A WhisperModel over the cut engine (WhisperModel(name) builds the full-depth model)."""
    m = tr.WhisperModel.__new__(tr.WhisperModel)
    m.engine = eng
    m.model_size = CUT.name
    m.stats = {"windows": 0, "needs_fallback": 0, "no_speech_skips": 0, "fallback_decodes": 0}
    m._vad_weights, m._vad_gate = None, None
    return m


@pytest.mark.parametrize("temps", [(0.0,), (0.0, 0.4)], ids=["T0", "fallback"])
def test_seek_loop_matches_oracle(cut, gpu, temps):
    """generate_segments on a 35 s and a 4 s utterance at max_length 24 equals
    oracle.transcribe_segments window by window (windows, segments, texts, times, counters), at
    T = 0 alone and with a fallback temperature (best_of 5 sampled hypotheses over a gathered
    encoder row). A window whose tokens differ must differ first at an oracle top-2 margin <
    NEAR_TIE (a sampled step's near tie does not excuse it). The drop-in call
    transcribe(beam_size=1, language='en') returns the same text."""
    eng, W = cut
    tk = eng.tokenizer
    F = mel_filters()
    auds = [synth_speech(170, 35.0, sr=16000).astype(np.float32),
            synth_speech(181, 4.0, sr=16000).astype(np.float32)]
    streams = tr.generate_segments(eng, auds, max_length=24, temperatures=temps)
    assert streams[0].windows >= 2
    assert eng.decode_path().persistent == 0
    m = cut_model(eng)
    for i, (a, st) in enumerate(zip(auds, streams)):
        ref, cnt = ow.transcribe_segments(a, W, CUT, tk, F, max_length=24, temperatures=temps, utt=i)
        got = [(s.start, s.end, s.text, list(s.tokens)) for s in st.segments]
        print(f"utterance {i}: {st.windows} windows, {len(got)} segments, {st.fallback_decodes} fallback decodes")
        assert st.windows == cnt["windows"] and st.skips == cnt["skips"] == 0
        if [g[3] for g in got] != [r[3] for r in ref]:
            feats = ow.logmel(a, 1, F, n_frames=None)
            mins = []
            for seek, size, prompt in cnt["trace"]:
                enc = ow.encoder(ow.window(feats, seek)[None], W, CUT).half().float().numpy()
                mins.append(min(mr.greedy(enc, W, CUT, tk, [prompt], 24)[0]["margins"]))
            assert min(mins) < NEAR_TIE, (i, mins)
            continue
        assert st.fallbacks == cnt["needs_fallback"] and st.fallback_decodes == cnt["fallback_decodes"]
        assert [g[2] for g in got] == [r[2] for r in ref]
        assert np.allclose([g[:2] for g in got], [r[:2] for r in ref])
        if i == 1:      # the drop-in call (transcriber.py: beam_size=1, language='en') on the short clip
            segs, info = m.transcribe(a, beam_size=1, language="en", temperature=temps, max_length=24)
            if len(temps) > 1:      # alone, the clip is utterance 0: the fallback's noise seeds are keyed on that
                ref, cnt = ow.transcribe_segments(a, W, CUT, tk, F, max_length=24, temperatures=temps, utt=0)
            assert " ".join(s.text.strip() for s in segs).strip() == " ".join(r[2].strip() for r in ref).strip()
            assert info.language == "en" and m.stats["windows"] == cnt["windows"]


# ------------------------------------------------------------------ 10. alignment
@pytest.fixture(scope="module")
def aligned(gpu):
    W, enc, wins = mf.align_case()
    eng = WhisperEngine(CUT, weights=W)
    out = eng.align(enc.to(eng.device), [w["text"] for w in wins], [w["size"] for w in wins],
                    enc_index=[w["enc"] for w in wins], return_attention=True)
    torch.cuda.synchronize()
    return eng, wins, out


def test_align_matches_reference_1024(aligned):
    """The alignment call on the cut (16 alignment heads of layer 1; 61 text tokens over 1500
    frames and 7 over 218) against tests/align_ref.py: A and the token probabilities inside the
    existing bounds, the GPU path monotone from (0, 0) to (N - 1, F - 1) and at most
    2 (N + F) ALIGN_E_A costlier on the reference matrix than the reference optimum."""
    _, wins, out = aligned
    for k, (w, a) in enumerate(zip(wins, out)):
        N, F = w["A"].shape
        assert a.attention.shape == (N, F) and a.token_probs.shape == (len(w["text"]),)
        eA = float(np.abs(a.attention - w["A"]).max())
        eP = float(np.abs(a.token_probs / w["p"] - 1).max())
        print(f"align medium-cut window {k}: N {N} F {F} max|dA| {eA:.3e} max rel dp {eP:.3e}")
        assert eA <= ALIGN_E_A, eA
        assert eP <= ALIGN_E_P_REL, eP
        assert (a.token_probs > 0).all() and (a.token_probs <= 1).all()
        align_ref.check_path_shape(a.text_indices, a.time_indices, N, F)
        x = -w["A"]
        got = align_ref.path_cost(x, a.text_indices, a.time_indices)
        opt = align_ref.path_cost(x, w["ti"], w["fi"])
        assert got <= opt + 2 * (N + F) * ALIGN_E_A, (got, opt)


def test_transcribe_word_timestamps_1024(cut, gpu):
    """transcribe(word_timestamps=True) over two seek windows on the cut: every segment has
    ``words`` with ordered times and probabilities in (0, 1]; the seeks, segments and words
    equal align_ref.seek_loop run over the GPU's window results (the existing end-to-end check
    of tests/test_align_gpu.py)."""
    eng, _ = cut
    m = cut_model(eng)
    audio = np.ascontiguousarray(synth_speech(66, 36.0)[::3])
    segs, info = m.transcribe(audio, word_timestamps=True, temperature=(0.0,), max_length=24)
    segs = list(segs)
    assert len(segs) >= 2 and len({s.seek for s in segs}) >= 2
    last = 0.0
    for s in segs:
        assert s.words is not None
        for w in s.words:
            assert 0.0 <= w.start <= info.duration and 0.0 <= w.end <= info.duration
            assert w.start >= last
            last = w.start
            assert 0.0 < w.probability <= 1.0
    st = tr.generate_segments(eng, [audio], max_length=24, temperatures=(0.0,), word_timestamps=True)[0]
    assert [(g.seek, g.start, g.end, g.text) for g in st.segments] == [(g.seek, g.start, g.end, g.text) for g in segs]
    assert len(st.window_alignments) == st.windows == len(st.window_seeks) >= 2
    wins = [(t, avg, nsp, a) for (t, avg, nsp), a in zip(st.window_rows, st.window_alignments)]
    seeks, ref = align_ref.seek_loop(TK, st.content_frames, wins)
    assert st.window_seeks == seeks
    assert [(g.seek, g.tokens, [(w.word, w.start, w.end, w.probability) for w in g.words])
            for g in st.segments] == [(a, t, ws) for (a, _, _, t, ws) in ref]
    for g, r in zip(st.segments, ref):
        assert abs(g.start - r[1]) < 1e-9 and abs(g.end - r[2]) < 1e-9


# ------------------------------------------------------------------ 11. refusals
def test_second_tier_is_refused_before_gpu_work(cut, gpu):
    eng, _ = cut
    enc = torch.zeros(1, 1500, 1024, dtype=torch.float16, device=gpu)
    with pytest.raises(NotImplementedError, match="beam_size 4 on medium-cut"):
        eng.decode_beam(enc, beam_size=4, max_length=16)
    with pytest.raises(NotImplementedError, match="int8 encoder compute on medium-cut"):
        WhisperEngine(CUT, weights={}, encoder_compute="int8")
    with pytest.raises(NotImplementedError, match="int8"):
        eng.set_encoder_compute("int8")
    # the C entries refuse too
    with pytest.raises(nat.JanusNativeError, match="d_model <= 768"):
        eng.decode_beam(enc, beam_size=1, max_length=16)
