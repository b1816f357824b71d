"""The int8 decoder weights on the MI355X (decoder_compute="int8").

1. the prepare-time quantiser against the numpy float32 rule, exactly;
2. the W8A16 skinny GEMM against the float64 product of the same fp16 A, q and s, under the
   derived bound (every a * q is exact in fp32; K products accumulate in fp32):
   |err| <= (K + 4) 2^-24 s[n] sum_k |a_k| |q_nk| + 2^-24 |bias|, plus 2^-11 |y| where the output
   is fp16 (one rounding; 2^-25 below the fp16 normal range) and, for the residual epilogue,
   2^-24 (|bias + r| + |y|) for the two fp32 additions; GELU by the tolerance of
   tests/test_kernels_gpu.py::test_gemm (Frobenius 2e-3 against float64);
3. the vocabulary projection on an int8 table with the criteria and numbers of
   tests/test_medium_family_gpu.py::test_vocabulary_projection_1024 and
   tests/test_large_family_gpu.py::test_vocabulary_projection_1280;
4. janus_whisper_decode_hidden with INT8 against tests/decoder_int8_ref.py on the matrices read
   back from the engine, bound decoder_ref.K_BOUND x the emulation's own distance;
5. the free-running greedy decode against the teacher-forced reference on the GPU's own prefix;
6. behaviour: shared rows, staggered rows, the persistent request, switching, set_tensor, the
   refusals, align and detect_language;
7. WhisperModel(decoder_compute="int8").transcribe against generate_segments.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cross_int8_ref as cr
import decoder_int8_ref as d8
import decoder_ref as ref
import history_ref as hr
import large_family_ref as lf
from janus_amd import _native as nat
from janus_amd import whisper as jw
from janus_amd._native import JanusNativeError
from oracle import whisper as ow

pytestmark = pytest.mark.gpu
NEAR_TIE = 2e-3
F32 = np.float32


def sp():
    return nat.stream_ptr()


# ------------------------------------------------------------------ 1. the quantiser
def weight_rows(N, K, seed, spread=6):
    """fp16 [N][K]: unit normal / sqrt(K) rows scaled by powers of two over 2^+-spread; row 1
    (where there is one) all zeros."""
    g = np.random.default_rng(seed)
    w = g.standard_normal((N, K)) / np.sqrt(K)
    w *= 2.0 ** g.integers(-spread, spread + 1, size=(N, 1))
    w = w.astype(np.float16)
    if N > 1:
        w[1] = 0
    return w


@pytest.mark.parametrize("K", [384, 1280, 5120])
@pytest.mark.parametrize("N", [1, 17, 100])
def test_quantiser_is_the_rule_exactly(gpu, N, K):
    w = weight_rows(N, K, 100 * N + K)
    if N > 2:
        w[2] *= np.float16(2.0 ** 6)
        w[3] *= np.float16(2.0 ** -6)
    x = torch.from_numpy(w).to(gpu)
    q = torch.full((N, K), 99, dtype=torch.int8, device=gpu)
    s = torch.full((N,), -1.0, dtype=torch.float32, device=gpu)
    nat.call("janus_quant_weight_rows_i8", x.data_ptr(), K, q.data_ptr(), K, s.data_ptr(), N, K, sp())
    torch.cuda.synchronize()
    qr, sr = d8.quantise(w)
    assert np.array_equal(q.cpu().numpy(), qr) and np.array_equal(s.cpu().numpy(), sr)
    if N > 1:
        assert not qr[1].any() and sr[1] == 1.0
    assert np.abs(qr[0]).max() == 127


# ------------------------------------------------------------------ 2. the GEMM
GEMM_M = [1, 17, 64, 65, 130]
GEMM_NK = [(384, 384), (1536, 384), (4096, 512), (3840, 1280), (1280, 5120)]


@functools.lru_cache(maxsize=None)
def gemm_case(N, K, groups=1):
    """A fp16 [130][groups K], q / s of fp16 rows whose scales spread over 2^+-3, bias, R; the
    float64 product and the magnitude sum of the bound, computed once per shape."""
    g = torch.Generator().manual_seed(N * 3 + K + groups)
    A = torch.randn(max(GEMM_M), groups * K, generator=g).half()
    q, s = d8.quantise(weight_rows(N, K, N + K, spread=3))
    if N > 1:
        assert s.max() / s[s != 1.0].min() >= 2.0 ** 4
    bias = torch.randn(N, generator=g).numpy()
    R = torch.randn(max(GEMM_M), N, generator=g).numpy()
    A64, q64 = A.double().numpy(), q.astype(np.float64)
    if groups == 1:
        lin, mag = A64 @ q64.T, np.abs(A64) @ np.abs(q64).T
    else:      # output columns [64 g, 64 g + 64) read A columns [g K, g K + K)
        lin, mag = np.zeros((len(A64), N)), np.zeros((len(A64), N))
        for h in range(groups):
            c, a = slice(64 * h, 64 * h + 64), A64[:, h * K:(h + 1) * K]
            lin[:, c], mag[:, c] = a @ q64[c].T, np.abs(a) @ np.abs(q64[c]).T
    s64 = s.astype(np.float64)
    return A, q, s, bias, R, lin * s64 + bias.astype(np.float64), mag * s64


def run_gemm(gpu, epi, A, q, s, bias, R, M, N, K, groups=1):
    dA, dq, ds, db = A[:M].contiguous().to(gpu), torch.from_numpy(q).to(gpu), torch.from_numpy(s).to(gpu), \
        torch.from_numpy(bias).to(gpu)
    out_dtype = torch.float16 if epi in (0, 1) else torch.float32
    C = torch.from_numpy(R[:M]).to(gpu).clone() if epi == 2 else torch.empty(M, N, dtype=out_dtype, device=gpu)
    nat.call("janus_gemm_w8_f16", epi, dA.data_ptr(), groups * K, dq.data_ptr(), ds.data_ptr(), K, db.data_ptr(),
             C.data_ptr(), N, C.data_ptr() if epi == 2 else None, N, M, N, K, 64 if groups > 1 else 0, sp())
    torch.cuda.synchronize()
    return C.double().cpu().numpy()


def hold_gemm(name, epi, got, y, mag, bias, R, K):
    e_lin = (K + 4) * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(bias)[None]
    if epi == 1:      # tests/test_kernels_gpu.py::test_gemm's fp16 tolerance
        want = F.gelu(torch.from_numpy(y)).numpy()
        err = np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30)
        print(f"{name}: GELU relative error {err:.2e}")
        assert err < 2e-3, (name, err)
        return
    if epi == 2:
        want = y + R.astype(np.float64)
        bound = e_lin + 2.0 ** -24 * (np.abs(bias[None] + R) + np.abs(want))
    else:
        want, bound = y, e_lin
    if epi == 0:
        bound = bound * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(want) + 2.0 ** -25
    ratio = np.abs(got - want) / bound
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{name}: worst error / bound {ratio.max():.3f} at {at}")
    assert np.isfinite(got).all() and ratio.max() <= 1.0, (name, at, got[at], want[at], bound[at])


@pytest.mark.parametrize("epi", [0, 1, 2, 3], ids=["f16", "gelu", "resid", "f32"])
@pytest.mark.parametrize("N,K", GEMM_NK, ids=[f"{n}x{k}" for n, k in GEMM_NK])
def test_gemm_w8(gpu, N, K, epi):
    """Every epilogue the test entry reaches (the QKV cache epilogue runs in the hidden-state
    cases) at 1, 17, 64, 65 and 130 rows: the row-split form (N <= 2048), the all-rows form, its
    one-k-step form (K <= 512) and more than one 64-row block."""
    A, q, s, bias, R, y, mag = gemm_case(N, K)
    for M in GEMM_M:
        got = run_gemm(gpu, epi, A, q, s, bias, R, M, N, K)
        hold_gemm(f"w8 gemm {M}x{N}x{K} epi {epi}", epi, got, y[:M], mag[:M], bias, R[:M], K)


def test_gemm_w8_grouped(gpu):
    """The block-diagonal value projection: 6 heads, output columns [64 h, 64 h + 64) from A
    columns [384 h, 384 h + 384)."""
    N, K, H = 384, 384, 6
    A, q, s, bias, R, y, mag = gemm_case(N, K, groups=H)
    for M in (17, 65):
        got = run_gemm(gpu, 0, A, q, s, bias, R, M, N, K, groups=H)
        hold_gemm(f"w8 grouped gemm {M} rows", 0, got, y[:M], mag[:M], bias, R[:M], K)


def test_gemm_w8_refusals(gpu):
    A, q, s, bias, R, _, _ = gemm_case(384, 384)
    with pytest.raises(JanusNativeError, match="int8 weights are the skinny kernel's"):
        run_gemm(gpu, 0, torch.cat([A] * 4), q, s, bias, np.concatenate([R] * 4), 513, 384, 384)
    with pytest.raises(JanusNativeError, match="epilogues 0 .. 3"):
        run_gemm(gpu, 4, A, q, s, bias, R, 4, 384, 384)


# ------------------------------------------------------------------ 3. the vocabulary projection
PV = 16 * 100 + 10          # the last tile holds 10 columns
EOT, NSP, NOTS, TSB, BLANK = 1500, 1501, 1502, 1503, 220      # the special ids at the top
PROJ_ROWS = {384: (1, 64, 65), 1024: (47, 48, 49), 1280: (31, 32, 33)}


@functools.lru_cache(maxsize=None)
def proj_case(K):
    g = torch.Generator().manual_seed(4300 + K)
    B = max(PROJ_ROWS[K])
    A = torch.randn(B, K, generator=g).half()
    Wt = (0.05 * torch.randn(PV, K, generator=g)).half().numpy()
    Wt *= (2.0 ** np.random.default_rng(K).integers(-2, 3, size=(PV, 1))).astype(np.float16)
    # the last real id wins row 0 by construction: its row along A[0] (logit ~ 40)
    Wt[PV - 1] = (A[0].float() * (40.0 / float((A[0].float() ** 2).sum()))).half().numpy()
    q, s = d8.quantise(Wt)
    L = (A.double().numpy() @ q.astype(np.float64).T) * s.astype(np.float64)      # float64 [B][PV]
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
    return A, q, s, L, smask, rules


def allowed(smask, rules, b):
    return lf.allowed_mask(PV, smask, tuple(rules[b, :4]), EOT, BLANK, TSB, NOTS, 50)


def run_projection(gpu, K, A, q, s, smask, rules, rows, inv_temp=0.0, seeds=None, pos=5, words=None, pen=1.0):
    B = len(rows)
    Ad, qd, sd_ = A[rows].contiguous().to(gpu), torch.from_numpy(q).to(gpu), torch.from_numpy(s).to(gpu)
    sm = torch.from_numpy(smask).to(gpu)
    rr = torch.from_numpy(np.ascontiguousarray(rules[rows])).to(gpu)
    nblk = nat.lib().janus_beam_partial_blocks(PV, K, 256)
    parts = torch.zeros(B * nblk * 56, dtype=torch.uint8, device=gpu)
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu) if seeds is not None else None
    args = [Ad.data_ptr(), qd.data_ptr(), sd_.data_ptr(), K, PV, B, EOT, 1, BLANK, TSB, NOTS, 50, NSP,
            sm.data_ptr(), rr.data_ptr(), 256, float(inv_temp), sd.data_ptr() if sd is not None else None, pos,
            parts.data_ptr()]
    if words is None:
        nat.call("janus_logits_partial_w8_f16", *args, sp())
    else:
        nat.call("janus_logits_partial_hist_w8_f16", *args, words.data_ptr(), float(pen), sp())
    torch.cuda.synchronize()
    return lf.merge_parts(parts.cpu().numpy().view(lf.PART_DTYPE).reshape(B, nblk))


def lse(v):
    return float(v.max() + np.log(np.exp(v - v.max()).sum())) if v.size else -np.inf


def check_projection_row(b, g, L, ok, raw=None):
    """test_vocabulary_projection_1024 / _1280's criteria with their numbers; returns the argmax
    decisions clear enough (margin > 2e-3) to be compared."""
    raw = L if raw is None else raw
    for name, want in (("lse_all", lse(L[ok])), ("lse_ts", lse(L[TSB:][ok[TSB:]])), ("lse_raw", lse(raw))):
        if np.isfinite(want):
            assert abs(g[name] - want) <= 1e-4 * abs(want), (b, name, g[name], want)
        else:
            assert g[name] == -np.inf, (b, name, g[name])
    assert abs(g["t_v"] - raw[NSP]) <= 2e-3, (b, g["t_v"], raw[NSP])
    checked = 0
    for key, sel in (("best", ok), ("best_ts", ok & (np.arange(PV) >= TSB))):
        if not sel.any():
            continue
        cand = np.where(sel, L, -np.inf)
        top = np.sort(cand)[-2:]
        assert 0 <= g[key] < PV, (b, key, g[key])             # never a padded column
        if top[-1] - top[-2] > 2e-3:
            assert g[key] == int(np.argmax(cand)), (b, key, g[key], int(np.argmax(cand)))
            checked += 1
    if ok[:TSB].any():
        assert abs(g["m_text"] - L[:TSB][ok[:TSB]].max()) <= 2e-3
    return checked


@pytest.mark.parametrize("K,nrows", [(K, n) for K in PROJ_ROWS for n in PROJ_ROWS[K]])
def test_vocabulary_projection_w8(gpu, K, nrows):
    A, q, s, L, smask, rules = proj_case(K)
    rows = list(range(nrows))
    got = run_projection(gpu, K, A, q, s, smask, rules, rows)
    checked = sum(check_projection_row(b, got[b], L[b], allowed(smask, rules, b)) for b in rows)
    assert got[0]["best"] == PV - 1          # the last real id wins: a padded copy of it would move the sums
    assert checked >= nrows


@pytest.mark.parametrize("K", sorted(PROJ_ROWS))
def test_vocabulary_projection_w8_padded_columns_stay_out(gpu, K):
    """Every logit equal (one repeated table row, about -30): the sums count exactly the PV real
    columns (the last tile's 6 padded columns repeat column PV - 1: counted, they would add
    log((PV + 6) / PV) = 3.7e-3), the bound of the 1024 test: 5e-5 absolute."""
    A, _, _, _, smask, rules = proj_case(K)
    g = torch.Generator().manual_seed(K + 1)
    row = torch.randn(K, generator=g).half()
    q, s = d8.quantise(row.repeat(PV, 1).numpy())
    w = torch.from_numpy(q[0].astype(np.float32) * s[0])
    A2 = (-w * (30.0 / float((w ** 2).sum()))).half()[None].repeat(3, 1)
    free = np.zeros_like(rules[:3])
    free[:, 3] = free[:, 4] = -1
    for r in run_projection(gpu, K, A2, q, s, np.zeros_like(smask), free, [0, 1, 2]):
        assert r["best"] == 0 and r["best_v"] < -20 and r["best_ts"] == TSB
        e_all = abs(r["lse_all"] - (r["best_v"] + np.log(PV - 1)))      # (<|notimestamps|> is never allowed)
        e_raw = abs(r["lse_raw"] - (r["best_v"] + np.log(PV)))
        assert e_all <= 5e-5 and e_raw <= 5e-5, (e_all, e_raw)


@pytest.mark.parametrize("K", sorted(PROJ_ROWS))
def test_vocabulary_projection_w8_sampling_keys(gpu, K):
    """SAMPLE: the argmax of logit / T + the device's own Gumbel noise over the allowed tokens."""
    A, q, s, L, smask, rules = proj_case(K)
    B = max(PROJ_ROWS[K])
    T, pos = 0.6, 5
    seeds = [7000 + b for b in range(B)]
    got = run_projection(gpu, K, A, q, s, smask, rules, list(range(B)), inv_temp=1.0 / T, seeds=seeds, pos=pos)
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu)
    noise = torch.empty(B, PV, dtype=torch.float32, device=gpu)
    nat.call("janus_sample_gumbel_f32", sd.data_ptr(), B, pos, PV, noise.data_ptr(), sp())
    noise = noise.cpu().numpy().astype(np.float64)
    inv = float(F32(1.0) / F32(T))
    hit = 0
    for b in range(B):
        keys = np.where(allowed(smask, rules, b), L[b] * inv + noise[b], -np.inf)
        top = np.sort(keys)[-2:]
        if top[-1] - top[-2] > NEAR_TIE / T:
            assert got[b]["best"] == int(np.argmax(keys)), b
            hit += 1
    assert hit >= B - 2


def test_vocabulary_projection_w8_history_rules(gpu):
    """HIST at K = 384, p = 1.2, n = 3, 65 rows, as test_vocabulary_projection_history_rules."""
    K = 384
    A, q, s, L, smask, rules = proj_case(K)
    p, n, B, ld = 1.2, 3, 65, 12
    rows = list(range(B))
    plain = run_projection(gpu, K, A, q, s, smask, rules, rows)
    rng = np.random.default_rng(61)
    tokens = np.zeros((B, ld), np.int32)
    plens = (1 + np.arange(B) % 3).astype(np.int32)
    for b in rows:
        second = int(np.argsort(np.where(allowed(smask, rules, b), L[b], -np.inf))[-2])
        g = [int(t) for t in rng.choice([plain[b]["best"], PV - 1, 5, TSB + 37], ld)]
        g[-6:] = [plain[b]["best"], 17, 31, second, 17, 31]
        tokens[b] = g
    words = torch.zeros(nat.lib().janus_history_words(PV, K, B), dtype=torch.int32, device=gpu)
    td, pd = torch.from_numpy(tokens).to(gpu), torch.from_numpy(plens).to(gpu)
    nat.call("janus_history_rules", td.data_ptr(), ld, B, pd.data_ptr(), n, PV, K, 0, ld, words.data_ptr(), sp())
    got = run_projection(gpu, K, A, q, s, smask, rules, rows, words=words, pen=p)
    checked = moved = 0
    for b in rows:
        g = [int(t) for t in tokens[b][plens[b]:]]
        ban = hr.banned(g, n)
        assert ban, b
        ok = allowed(smask, rules, b)
        ok[ban] = False
        Lp = hr.penalise(L[b], g, p).astype(np.float64)
        assert got[b]["best"] not in ban
        checked += check_projection_row(b, got[b], Lp, ok, raw=L[b])
        moved += int(got[b]["best"] != plain[b]["best"] or got[b]["best_v"] < plain[b]["best_v"])
    assert checked >= B and moved >= B // 2, (checked, moved)


# ------------------------------------------------------------------ 4. the hidden state
T_HID, ROWS_HID = 4, 65
SEED_W, SEED_IN = 3, 5
SHAPES = {"tiny.en": (384, 6), "base.en": (512, 8), "768": (768, 12), "1280": (1280, 20)}


class Model:
    """One two-layer cut: weights, inputs, an int8 engine, the matrices read back from it and the
    references on them (65 rows, computed once and sliced: the rows are independent)."""

    def __init__(self, d, H):
        self.cfg = ref.config(d, H)
        self.W = ref.weights(self.cfg, SEED_W)
        self.tokens, self.enc = ref.inputs(self.cfg, ROWS_HID, T_HID, SEED_IN)
        self.engine = jw.WhisperEngine(self.cfg, self.W, decoder_compute="int8")
        self.enc_d = torch.from_numpy(self.enc).cuda()
        self._Q = None

    @property
    def Q(self):
        if self._Q is None:
            self._Q = ([[self.engine.decoder_weight_i8(l, i) for i in range(7)] for l in range(self.cfg.dec_layers)],
                       self.engine.decoder_weight_i8(-1, 0))
        return self._Q

    @functools.lru_cache(maxsize=None)
    def reference(self, emulate, cross=False):
        enc = cr.dequantised(self.enc) if cross else self.enc
        return d8.hidden(self.tokens, enc, d8.dequantised(self.Q[0]), self.W, self.cfg, emulate=emulate)

    def enc_dev(self, n):
        return self.enc_d[:n].contiguous()


@pytest.fixture(scope="module")
def models(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(*SHAPES[name])
        return made[name]
    yield get
    made.clear()


INT8_PLAN = dict(dec_int8=1, persist=0, seg_grid=0, xabs=1, fused_ln=0, ln_fuse=0, ln_pro_mask=0, embed_ln=0, rln=0,
                 cvp=0)


def check_plan(plan, want):
    got = {k: plan.get(k) for k in want}
    assert got == want, f"the plan that ran differs: {got} != {want}"


def hold(name, got, want, emu):
    e_row, e_tile = ref.metrics(emu, want)
    g_row, g_tile = ref.metrics(got, want)
    print(f"{name}: row {g_row:.2e} tile {g_tile:.2e} | emulation row {e_row:.2e} tile {e_tile:.2e}")
    at, col, val = ref.worst(got, want)
    assert np.isfinite(g_tile) and g_tile <= ref.K_BOUND * e_tile, \
        f"{name}: (row, position) {at}, columns {col}-{col + 15}: tile {val:.2e} over the bound {ref.K_BOUND * e_tile:.2e}"
    assert g_row <= ref.K_BOUND * e_row, f"{name}: row {g_row:.2e} over the bound {ref.K_BOUND * e_row:.2e}"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_read_back_weights_are_the_rule(models, name):
    """The plain matrices and the vocabulary table: q and s of the numpy rule on the fp16 copies of
    the (fp16-representable) synthetic parameters, exactly. The absorbed query weight: the rule on
    the fp16 wqk derived as decoder_ref derives it (decoder_int8_ref.wqk_check): only elements
    within one fp16 ulp of a quantiser boundary differ, by 1, and they are under 10 %."""
    M = models(name)
    (Q, table), (want, want_table) = M.Q, d8.quantised(M.W, M.cfg)
    assert np.array_equal(table[0], want_table[0]) and np.array_equal(table[1], want_table[1])
    for l in range(M.cfg.dec_layers):
        for i in range(7):
            if i == d8.XQK:
                r = d8.wqk_check(Q[l][i][0], Q[l][i][1], M.W, M.cfg, l)
                print(f"{name} layer {l} wqk: {r}")
                assert r["share"] < 0.10 and r["bad"] == 0, r
                assert r["s_rows"] <= 0.01 * len(Q[l][i][1]) and r["s_rel"] <= 2.0 ** -10, r
            else:
                assert np.array_equal(Q[l][i][0], want[l][i][0]), (l, d8.WHICH[i])
                assert np.array_equal(Q[l][i][1], want[l][i][1]), (l, d8.WHICH[i])


@pytest.mark.parametrize("B", [1, 17, 65])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hidden_parity(models, name, B):
    M = models(name)
    out = M.engine.decode_hidden(M.enc_dev(B), M.tokens[:B], want_cache=False)
    check_plan(out.plan, dict(INT8_PLAN, B=B))
    assert M.engine.decode_weights() == "int8"
    x = out.x.transpose(0, 1).double().cpu().numpy()
    hold(f"int8 {name} rows {B}", x, M.reference(False)[:B], M.reference(True)[:B])


def test_hidden_parity_with_int8_cross(models):
    M = models("base.en")
    M.engine.set_cross_compute("int8")
    try:
        out = M.engine.decode_hidden(M.enc_dev(17), M.tokens[:17], want_cache=False)
    finally:
        M.engine.set_cross_compute("float16")
    check_plan(out.plan, dict(INT8_PLAN, cross_int8=1))
    x = out.x.transpose(0, 1).double().cpu().numpy()
    hold("int8 weights + int8 cross", x, M.reference(False, True)[:17], M.reference(True, True)[:17])


# ------------------------------------------------------------------ 5. free-running greedy decode
ML = 16


class Cut:
    """A two-layer cut with the full vocabulary (the tokenizer's special ids), for decode calls."""

    def __init__(self, d, H, rows):
        self.cfg = jw.WhisperConfig(f"int8-cut-{d}", d, H, 0, 2, n_audio_ctx=141)
        self.W = jw.synthetic_weights(self.cfg, seed=7)
        self.engine = jw.WhisperEngine(self.cfg, self.W, decoder_compute="int8")
        g = torch.Generator().manual_seed(21 + d)
        self.enc = torch.randn(rows, 141, d, generator=g).half().numpy()
        self.enc_d = torch.from_numpy(self.enc).cuda()
        self.M = d8.dequantised([[self.engine.decoder_weight_i8(l, i) for i in range(7)] for l in range(2)])
        q, s = self.engine.decoder_weight_i8(-1, 0)
        self.table = q.astype(np.float64) * s.astype(np.float64)[:, None]


@pytest.fixture(scope="module")
def cuts(gpu):
    made = {}

    def get(d, H):
        if d not in made:
            made[d] = Cut(d, H, 33)
        return made[d]
    yield get
    made.clear()


def check_free_running(C, out, enc, rows):
    """Every sampled position: the GPU's token is the argmax of the reference's rule-filtered
    logits given the GPU's own prefix, or the row's first difference lies at a top-2 margin below
    NEAR_TIE (the row is left there: its later prefix is no longer the reference's choice)."""
    tk = C.engine.tokenizer
    tokens, ntok = out.tokens.cpu().numpy(), out.n_tokens.cpu().numpy()
    plen = int(out.prompt_lens[0])
    forced = np.where(tokens < 0, tk.eot, tokens)[:, :ML - 1]
    x = d8.hidden(forced[rows], enc[rows], C.M, C.W, C.cfg)
    suppress = tk.suppress_tokens()
    logits = d8.logits(x[:, plen - 1:], C.W, C.cfg, C.table)      # [rows][positions from the first sampled][V]
    clear = ties = 0
    for i, b in enumerate(rows):
        got = [int(t) for t in tokens[b][plen:plen + int(ntok[b])]]
        assert 1 <= len(got) <= logits.shape[1]
        L = logits[i]
        for j, t in enumerate(got):
            Lf, _ = ow.apply_rules(L[j], got[:j], tk, suppress)
            top = np.sort(Lf[np.isfinite(Lf)])[-2:]
            if t == int(np.argmax(Lf)):
                clear += 1
                continue
            assert top[-1] - top[-2] < NEAR_TIE, (b, j, t, int(np.argmax(Lf)), float(top[-1] - top[-2]))
            ties += 1
            break
    print(f"free-running: {clear} positions equal the reference's argmax, {ties} rows left at a near tie")
    assert clear >= 4 * len(rows)


@pytest.mark.parametrize("nrows", [1, 33])
@pytest.mark.parametrize("d,H", [(384, 6), (1280, 20)])
def test_free_running_greedy(cuts, d, H, nrows):
    C = cuts(d, H)
    out = C.engine.decode_ex(C.enc_d[:nrows].contiguous(), max_length=ML)
    assert C.engine.decode_weights() == "int8" and C.engine.decode_path() == jw.DecodePath("own", 0, "float16")
    check_free_running(C, out, C.enc, list(range(nrows)))


def test_free_running_greedy_with_int8_cross(cuts):
    C = cuts(384, 6)
    C.engine.set_cross_compute("int8")
    try:
        out = C.engine.decode_ex(C.enc_d[:9].contiguous(), max_length=ML)
        assert C.engine.decode_path() == jw.DecodePath("own", 0, "int8") and C.engine.decode_weights() == "int8"
    finally:
        C.engine.set_cross_compute("float16")
    check_free_running(C, out, cr.dequantised(C.enc), list(range(9)))


# ------------------------------------------------------------------ 6. behaviour
def same_out(a, b):
    return torch.equal(a.tokens, b.tokens) and torch.equal(a.n_tokens, b.n_tokens) and \
        torch.equal(a.sum_logprob, b.sum_logprob) and torch.equal(a.no_speech_prob, b.no_speech_prob)


def test_sampled_shared_rows_equal_replicated_rows(cuts):
    """2 windows x 5 hypotheses at T = 0.6 on shared encoder rows (read in place through PAIR
    blocks at 384) against the same rows replicated, bit for bit; per-row temperatures and the
    history rules likewise."""
    C = cuts(384, 6)
    idx = [0] * 5 + [1] * 5
    seeds = [900 + i for i in range(10)]
    two = C.enc_d[:2].contiguous()
    rep = C.enc_d[idx].contiguous()
    for kw in (dict(temperature=0.6), dict(temperature=[0.0, 0.2, 0.4, 0.6, 0.8] * 2),
               dict(temperature=0.6, repetition_penalty=1.3, no_repeat_ngram_size=2)):
        a = C.engine.decode_ex(two, enc_index=idx, seeds=seeds, max_length=ML, **kw)
        assert C.engine.decode_path().enc_rows == "in_place" and C.engine.decode_weights() == "int8"
        b = C.engine.decode_ex(rep, seeds=seeds, max_length=ML, **kw)
        assert same_out(a, b), kw
    wide = cuts(1280, 20)
    a = wide.engine.decode_ex(wide.enc_d[:2].contiguous(), enc_index=idx, seeds=seeds, max_length=ML, temperature=0.6)
    assert wide.engine.decode_path().enc_rows == "gathered"
    assert same_out(a, wide.engine.decode_ex(wide.enc_d[idx].contiguous(), seeds=seeds, max_length=ML, temperature=0.6))


def test_staggered_continuation_is_the_one_go_run(models):
    M = models("base.en")
    B, first, more = 6, 3, 1
    eng, enc, tokens = M.engine, M.enc_dev(B), M.tokens[:B]
    whole = eng.decode_hidden(enc, tokens, pos_offset=[0] * B, steps=first + more)
    check_plan(whole.plan, dict(dec_int8=1, stagger=1, persist=0))
    one = eng.decode_hidden(enc, tokens, pos_offset=[0] * B, steps=first)
    assert eng.decode_stand(B) == [first] * B and torch.equal(one.x, whole.x[:first])
    two = eng.decode_hidden(enc, tokens, pos_offset=[first] * 3 + [0] * 3, steps=more)
    check_plan(two.plan, dict(dec_int8=1, stagger=1, max_roff=first))
    assert torch.equal(two.x[:, :3], whole.x[first:, :3]) and torch.equal(two.x[:, 3:], whole.x[:more, 3:])


def test_persistent_request_and_refusals(models, cuts):
    M = models("base.en")
    out = M.engine.decode_hidden(M.enc_dev(4), M.tokens[:4], persistent=2, want_cache=False)
    check_plan(out.plan, INT8_PLAN)
    assert M.engine.decode_path().persistent == 0
    C = cuts(384, 6)
    enc = C.enc_d[:4].contiguous()
    a = C.engine.decode_ex(enc, max_length=ML)
    b = C.engine.decode_ex(enc, max_length=ML, persistent=2)
    assert C.engine.decode_path().persistent == 0 and same_out(a, b)
    before = C.engine.decode_info()
    with pytest.raises(JanusNativeError, match="JANUS_DEC_PATH_NO_XABSORB with decoder_compute int8"):
        C.engine.decode_ex(enc, max_length=ML, path_flags=jw.DEC_PATH_NO_XABSORB)
    with pytest.raises(NotImplementedError, match="decoder_compute='int8'"):
        C.engine.decode_beam(enc, beam_size=2, max_length=ML)
    assert C.engine.decode_info() == before           # nothing ran
    # the C entry refuses too
    opt, keep = C.engine.decode_options(ML, 16, True, 0, 0, 0, 0, 0, 0, 0)
    rows = jw.janus_decode_rows()
    rows.no_speech_token = C.engine.tokenizer.no_speech
    tk, nt = torch.empty(4, ML, dtype=torch.int32, device="cuda"), torch.empty(4, dtype=torch.int32, device="cuda")
    lp = torch.empty(4, dtype=torch.float32, device="cuda")
    with pytest.raises(JanusNativeError, match="beam search with decoder_compute int8"):
        nat.call("janus_whisper_decode_beam_ex", C.engine._h, enc.data_ptr(), 4, ctypes.addressof(opt),
                 ctypes.addressof(rows), 2, ctypes.c_float(1.0), tk.data_ptr(), nt.data_ptr(), lp.data_ptr(), None, sp())
    del keep
    assert C.engine.decode_info() == before


def test_float16_again_is_bit_identical(cuts):
    C = cuts(384, 6)
    enc = C.enc_d[:9].contiguous()
    never = jw.WhisperEngine(C.cfg, C.W)
    assert never.decoder_compute == "float16" and never.decode_weights() == "float16"
    a = never.decode_ex(enc, max_length=ML)
    ah = never.decode_hidden(enc, a.tokens.clamp(min=0).cpu().numpy()[:, :4])
    assert never.decode_weights() == "float16" and "dec_int8" not in ah.plan
    q = C.engine.decode_ex(enc, max_length=ML)
    assert C.engine.decoder_compute == "int8" and not torch.equal(q.sum_logprob, a.sum_logprob)
    C.engine.set_decoder_compute("float16")
    try:
        assert C.engine.decoder_compute == "float16"
        b = C.engine.decode_ex(enc, max_length=ML)
        assert C.engine.decode_weights() == "float16" and same_out(a, b)
        bh = C.engine.decode_hidden(enc, a.tokens.clamp(min=0).cpu().numpy()[:, :4])
        assert bh.plan == ah.plan and torch.equal(ah.x, bh.x) and torch.equal(ah.kc[:, :, :4], bh.kc[:, :, :4])
    finally:
        C.engine.set_decoder_compute("int8")
    assert same_out(C.engine.decode_ex(enc, max_length=ML), q)


def test_set_tensor_requantises(gpu):
    cfg = ref.config(384, 6)
    W = ref.weights(cfg, SEED_W)
    eng = jw.WhisperEngine(cfg, W, decoder_compute="int8")
    q0, s0 = eng.decoder_weight_i8(1, jw.DEC_W_FC1)
    name = "decoder.layers.1.fc1.weight"
    new = W[name].copy()
    new[5] = new[5, ::-1]
    new[9, 3] = 1.0        # a new largest element: row 9's scale moves
    eng.set_tensor(name, new)
    q1, s1 = eng.decoder_weight_i8(1, jw.DEC_W_FC1)
    want = d8.quantise(new.astype(np.float16))
    assert np.array_equal(q1, want[0]) and np.array_equal(s1, want[1])
    assert not np.array_equal(q1[5], q0[5]) and s1[9] == F32(1.0) / F32(127) and s1[9] != s0[9]
    assert np.array_equal(q1[6], q0[6])
    # the next decode call multiplies the new copy
    tokens, enc = ref.inputs(cfg, 2, 3, SEED_IN)
    out = eng.decode_hidden(torch.from_numpy(enc).cuda(), tokens, want_cache=False)
    W2 = dict(W)
    W2[name] = new
    Q, _ = d8.quantised(W2, cfg)
    x = out.x.transpose(0, 1).double().cpu().numpy()
    M = d8.dequantised(Q)
    hold("after set_tensor", x, d8.hidden(tokens, enc, M, W2, cfg), d8.hidden(tokens, enc, M, W2, cfg, emulate=True))


def test_align_and_detect_language_keep_float16(gpu):
    """align (tiny.en) and detect_language (tiny) return bit-identical results in both modes."""
    cfg = jw.CONFIGS["tiny.en"]
    eng = jw.WhisperEngine(cfg, jw.synthetic_weights(cfg, seed=5))
    g = torch.Generator().manual_seed(31)
    enc = torch.randn(2, cfg.n_audio_ctx, cfg.d_model, generator=g).half().cuda()
    texts, sizes = [[400, 1200, 3300, 770, 52], [9000, 17]], [3000, 437]
    a = eng.align(enc, texts, sizes)
    eng.set_decoder_compute("int8")
    eng.decode_ex(enc, max_length=6)                      # the int8 copies exist and were used
    assert eng.decode_weights() == "int8"
    b = eng.align(enc, texts, sizes)
    for x, y in zip(a, b):
        assert np.array_equal(x.text_indices, y.text_indices) and np.array_equal(x.time_indices, y.time_indices)
        assert np.array_equal(x.token_probs, y.token_probs)
    mcfg = jw.CONFIGS["tiny"]
    meng = jw.WhisperEngine(mcfg, jw.synthetic_weights(mcfg, seed=5))
    p0, b0 = meng.detect_language(enc)
    meng.set_decoder_compute("int8")
    meng.decode_ex(enc, max_length=6)
    p1, b1 = meng.detect_language(enc)
    assert torch.equal(p0, p1) and torch.equal(b0, b1)


# ------------------------------------------------------------------ 7. model level
def test_transcribe_is_generate_segments(gpu):
    from janus_amd.services.transcriber import WhisperModel, generate_segments
    model = WhisperModel("tiny.en", decoder_compute="int8")
    assert model.engine.decoder_compute == "int8"
    audio = hr.transcribe_audio()                         # 33 s: two seek windows
    segs, _ = model.transcribe(audio, temperature=(0.0,), max_length=16)
    segs = list(segs)
    assert model.engine.decode_weights() == "int8"
    st = generate_segments(model.engine, [audio], max_length=16, temperatures=(0.0,))[0]
    assert st.windows >= 2 and len(segs) >= 1
    assert [(s.start, s.end, s.tokens) for s in segs] == [(s.start, s.end, s.tokens) for s in st.segments]
    with pytest.raises(NotImplementedError, match="decoder_compute='int8'"):
        model.transcribe(audio, beam_size=2)
