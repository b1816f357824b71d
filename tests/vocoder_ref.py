"""References for the vocoder's kernels (conv.hip, resunit.hip, resunit_wide.hip, vocoder_edge.hip).

Plain torch / numpy in float64 on time-major [B][T][C] activations, independent of janus_amd's
code and of the oracle:

* ``conv1d``: janus_conv1d_f16(_ex): Conv1d / ConvTranspose1d, pre / post activation, residual,
  ``(y + res) * scale + prev`` and the SiLU after the accumulation.
* ``resunit``: one fused ResBlock1 unit (janus_resunit_f16(_ex)).
* ``conv_post``: the generator's tail (janus_conv_post_f32): -> (waveform, pre-tanh).
* ``generator``: the three chained in vocoder.cpp::forward's order, H stored as silu(H).

Every function takes ``emulate``. False: the operation itself on the given inputs, nothing
rounded. True: the same arithmetic rounded where the kernels store or stage fp16 — the
pre-activated operand of a conv, the weights, the intermediate silu(c1 + b1) of a unit and
every output store (one rounding after ``(y + res) * scale + prev`` and its optional SiLU;
bias, post-activation and the epilogue stay unrounded, as the kernels hold them in fp32).
conv_post stores no fp16: its rounding points are the fp32 accumulator, rounded after each
of its 16 x 13 multiply-adds in the kernel's order (channel outer, tap inner, starting from
the bias), fp32 SiLU and fp32 tanh. The distance of ``emulate=True`` from ``emulate=False`` is what
the number formats alone cost; the GPU tests' bound is decoder_ref.K_BOUND times it.

The convolutions are sums over taps of one matrix product per block of ``ROW_BLOCK`` output
rows, blocks aligned to absolute time: a row's value is a function of its own input window
and of nothing else, so a row range computed from a slice (``rows`` / ``origin`` / ``T``)
equals the same rows of the whole utterance bit for bit when the ranges start on a block
(tests/test_vocoder_tiles_host.py).

``metrics`` / ``worst``: the GPU tests' two distances and where the larger one lies.
"""
import functools
import math

import numpy as np
import torch

F64 = torch.float64
ROW_BLOCK = 256
ACT_NONE, ACT_SILU, ACT_GELU, ACT_TANH = 0, 1, 2, 3
TILE_ROWS, TILE_SAMPLES = 16, 64


def f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(F64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))


def r16(x):
    return x.float().half().to(F64)


def _same(x):
    return x


def silu(x):
    return x * torch.sigmoid(x)


def act(x, a):
    if a == ACT_NONE:
        return x
    if a == ACT_SILU:
        return silu(x)
    if a == ACT_GELU:
        return torch.nn.functional.gelu(x)
    if a == ACT_TANH:
        return torch.tanh(x)
    raise ValueError(a)


def _corr(x, w, stride, pad, dil, rows, origin, T):
    """out[b][t] = sum_j x_abs[b][t * stride + j * dil - pad] @ w[:, :, j]^T for t in rows =
    (lo, hi). x [B][n][Cin] holds absolute input rows [origin, origin + n) of an utterance of
    T rows, zero outside [0, T); w [Cout][Cin][k]. -> [B][hi - lo][Cout]."""
    B, n, Cin = x.shape
    Cout, _, k = w.shape
    lo, hi = rows
    wm = w.permute(2, 1, 0).reshape(k * Cin, Cout).contiguous()
    out = torch.empty(B, hi - lo, Cout, dtype=F64)
    taps = torch.arange(k) * dil - pad
    for blk in range(lo // ROW_BLOCK, (hi + ROW_BLOCK - 1) // ROW_BLOCK):
        t = torch.arange(blk * ROW_BLOCK, (blk + 1) * ROW_BLOCK)
        want = (t >= lo) & (t < hi)
        src = t[:, None] * stride + taps[None, :]                    # [R][k] absolute rows
        live = (src >= 0) & (src < T) & want[:, None]
        loc = src - origin
        assert bool(((loc >= 0) & (loc < n))[live].all()), "the slice lacks halo rows"
        loc = loc.clamp(0, n - 1)
        a = x[:, loc.reshape(-1)].reshape(B, ROW_BLOCK, k, Cin) * live[None, :, :, None].to(F64)
        y = a.reshape(B * ROW_BLOCK, k * Cin) @ wm
        y = y.reshape(B, ROW_BLOCK, Cout)
        a0, a1 = max(lo, blk * ROW_BLOCK), min(hi, (blk + 1) * ROW_BLOCK)
        out[:, a0 - lo:a1 - lo] = y[:, a0 - blk * ROW_BLOCK:a1 - blk * ROW_BLOCK]
    return out


def _corr_transposed(x, w, u, pad, T_out):
    """ConvTranspose1d(Cin, Cout, 2u, stride u, padding pad): x [B][T_in][Cin], w
    [Cin][Cout][2u]; output t = q * u + ph - pad reads input rows q (kernel index ph) and
    q - 1 (kernel index ph + u). Whole utterances only."""
    B, T_in, Cin = x.shape
    Cout = w.shape[1]
    t = torch.arange(T_out)
    q, ph = (t + pad) // u, (t + pad) % u
    xp = torch.cat([torch.zeros(B, 1, Cin, dtype=F64), x, torch.zeros(B, 1, Cin, dtype=F64)], 1)

    def rows(i):   # x[i], zero outside [0, T_in)
        return xp[:, (i + 1).clamp(0, T_in + 1)] * ((i >= 0) & (i < T_in))[None, :, None].to(F64)

    a = torch.cat([rows(q), rows(q - 1)], -1)                        # [B][T_out][2 Cin]
    out = torch.empty(B, T_out, Cout, dtype=F64)
    for p in range(u):
        sel = ph == p
        if bool(sel.any()):
            wm = torch.cat([w[:, :, p], w[:, :, p + u]], 0)           # [2 Cin][Cout]
            out[:, sel] = (a[:, sel].reshape(-1, 2 * Cin) @ wm).reshape(B, -1, Cout)
    return out


def conv_out_len(T_in, taps, stride, pad, dil, transposed):
    if transposed:
        return (T_in - 1) * stride - 2 * pad + 2 * stride
    return (T_in + 2 * pad - dil * (taps - 1) - 1) // stride + 1


@torch.no_grad()
def conv1d(x, w, bias, stride=1, padding=0, dilation=1, transposed=False, pre_act=ACT_NONE,
           post_act=ACT_NONE, res=None, scale=1.0, prev=None, post_acc_silu=False, emulate=False,
           rows=None, origin=0, T=None):
    """x [B][n][Cin] (fp16 values) -> [B][T_out][Cout] float64 torch. w: Conv1d [Cout][Cin][k]
    or, transposed, ConvTranspose1d [Cin][Cout][2 stride]. res / prev [B][T_out][Cout] or None
    (prev None: accumulate = 0). rows / origin / T: an output row range from an input slice
    (_corr), plain convs only; res and prev are then the range's rows."""
    rnd = r16 if emulate else _same
    x, w = f64(x), f64(w)
    xa = act(x, pre_act)
    if pre_act != ACT_NONE:
        xa = rnd(xa)
    w = rnd(w)
    if transposed:
        assert rows is None
        y = _corr_transposed(xa, w, stride, padding, conv_out_len(x.shape[1], 0, stride, padding, 1, True))
    else:
        T = x.shape[1] if T is None else T
        T_out = conv_out_len(T, w.shape[2], stride, padding, dilation, False)
        y = _corr(xa, w, stride, padding, dilation, rows or (0, T_out), origin, T)
    if bias is not None:
        y = y + f64(bias)
    y = act(y, post_act)
    return _epilogue(y, res, scale, prev, post_acc_silu, emulate)


def _epilogue(y, res, scale, prev, post_silu, emulate):
    """(y + res) * scale + prev, SiLU of that if asked, one fp16 rounding at the store."""
    if res is not None:
        y = y + f64(res)
    y = y * (float(np.float32(scale)) if emulate else scale)
    if prev is not None:
        y = y + f64(prev)
    if post_silu:
        y = silu(y)
    return r16(y) if emulate else y


@torch.no_grad()
def resunit_core(x, w1, b1, w2, b2, d, emulate=False, rows=None, origin=0, T=None):
    """c2(silu(c1(silu(x)) + b1)) + b2 + x before the epilogue: x [B][n][C], w [C][C][k]."""
    rnd = r16 if emulate else _same
    x, w1, w2 = f64(x), f64(w1), f64(w2)
    k = w1.shape[2]
    p1, p2 = d * (k - 1) // 2, (k - 1) // 2
    T = x.shape[1] if T is None else T
    lo, hi = rows or (0, T)
    # c1 on the rows c2 reads, zero outside [0, T): c2's padding
    m_lo, m_hi = max(0, lo - p2), min(T, hi + p2)
    h = _corr(rnd(silu(x)), rnd(w1), 1, p1, d, (m_lo, m_hi), origin, T) + f64(b1)
    h = rnd(silu(h))
    y = _corr(h, rnd(w2), 1, p2, 1, (lo, hi), m_lo, T) + f64(b2)
    return y + x[:, lo - origin:hi - origin]


@torch.no_grad()
def resunit(x, w1, b1, w2, b2, d, scale=1.0, prev=None, post_silu=False, emulate=False, rows=None,
            origin=0, T=None, core=None):
    """One fused ResBlock1 unit: out = [silu]((x + c2(silu(c1(silu(x)) + b1)) + b2) * scale +
    prev). ``core``: a resunit_core result of the same arguments (shared between epilogues)."""
    if core is None:
        core = resunit_core(x, w1, b1, w2, b2, d, emulate, rows, origin, T)
    return _epilogue(core, None, scale, prev, post_silu, emulate)


def _silu32(x):
    x = x.astype(np.float32)
    one = np.float32(1.0)
    return (x * (one / (one + np.exp(-x)))).astype(np.float32)


@torch.no_grad()
def conv_post(x, w, bias, pre_silu=False, emulate=False, rows=None, origin=0, T=None):
    """x [B][n][16] (fp16 values), w [16][13], bias a number -> (tanh(y), y) float64 numpy
    [B][hi - lo], y[t] = bias + sum_{c, j} w[c][j] s(x[t + j - 6][c])."""
    x = np.asarray(f64(x).numpy())
    w = np.asarray(w, np.float64).reshape(16, 13)
    B, n, C = x.shape
    T = n if T is None else T
    lo, hi = rows or (0, T)
    dt = np.float32 if emulate else np.float64
    if pre_silu:
        xs = _silu32(x) if emulate else x / (1.0 + np.exp(-x))
    else:
        xs = x
    xs = xs.astype(dt)
    # absolute rows lo - 6 .. hi + 6, zero outside [0, T)
    src = np.arange(lo - 6, hi + 6)
    live = (src >= 0) & (src < T)
    loc = src - origin
    assert ((loc >= 0) & (loc < n))[live].all(), "the slice lacks halo rows"
    win = xs[:, np.clip(loc, 0, n - 1)] * live[None, :, None].astype(dt)
    acc = np.full((B, hi - lo), dt(bias), dt)
    wd = w.astype(dt)
    for c in range(C):
        for j in range(13):
            acc = (acc + wd[c, j] * win[:, j:j + hi - lo, c]).astype(dt)
    return np.tanh(acc).astype(np.float64), acc.astype(np.float64)


def pcm16(wav):
    """The kernel's quantisation of an fp32 waveform: clip(rint(wav * 32767))."""
    v = np.rint(np.asarray(wav, np.float32) * np.float32(32767.0))
    return np.clip(v, -32768, 32767).astype(np.int16)


@torch.no_grad()
def generator(lat, W, cfg, emulate=False):
    """lat [B][F][latent] (fp16 values) -> (waveform, pre-tanh) float64 numpy [B][F * hop], in
    vocoder.cpp::forward's order: H, the ParallelBlock mean, is only ever read through a
    SiLU, so its producers (conv_pre, the last unit of each block) store silu(H); the mean
    accumulates into H unit by unit (three stores), the SiLU on the last."""
    inv_k = 1.0 / len(cfg.rb_kernels)
    H = conv1d(lat, W["conv_pre.weight"], W["conv_pre.bias"], padding=(cfg.pre_kernel - 1) // 2,
               post_act=ACT_SILU, emulate=emulate)
    for i, u in enumerate(cfg.up_rates):
        U = conv1d(H, W[f"ups.{i}.weight"], W[f"ups.{i}.bias"], stride=u, padding=u // 2, transposed=True,
                   emulate=emulate)
        H = None
        for j, _ in enumerate(cfg.rb_kernels):
            x = U
            p = f"resblocks.{i}.blocks.{j}"
            for m, d in enumerate(cfg.rb_dilations):
                last = m + 1 == len(cfg.rb_dilations)
                a = (W[f"{p}.convs1.{m}.weight"], W[f"{p}.convs1.{m}.bias"], W[f"{p}.convs2.{m}.weight"],
                     W[f"{p}.convs2.{m}.bias"], d)
                if not last:
                    x = resunit(x, *a, emulate=emulate)
                else:
                    H = resunit(x, *a, scale=inv_k, prev=H, post_silu=j + 1 == len(cfg.rb_kernels),
                                emulate=emulate)
    return conv_post(H, W["conv_post.weight"], float(np.asarray(W["conv_post.bias"]).reshape(-1)[0]),
                     pre_silu=False, emulate=emulate)


# ------------------------------------------------------------------------------ metrics
def _tiles(got, want):
    """-> (tile rms(err) [B][n_tiles], rms(want) of the whole tensor, rows per tile)."""
    got = np.asarray(f64(got).numpy() if isinstance(got, torch.Tensor) else got, np.float64)
    want = np.asarray(f64(want).numpy() if isinstance(want, torch.Tensor) else want, np.float64)
    assert got.shape == want.shape and want.ndim in (2, 3), (got.shape, want.shape)
    step = TILE_ROWS if want.ndim == 3 else TILE_SAMPLES
    e2 = (got - want) ** 2
    if e2.ndim == 3:
        e2 = e2.mean(-1)                                   # all channels of a row
    B, T = e2.shape
    n = (T + step - 1) // step
    pad = np.zeros((B, n * step - T))
    count = np.minimum(step, T - step * np.arange(n))      # the last tile may be short
    tile = np.sqrt(np.concatenate([e2, pad], 1).reshape(B, n, step).sum(-1) / count)
    return tile, float(np.sqrt((want ** 2).mean())), step, float(np.sqrt(e2.mean()))


def metrics(got, want):
    """(tile, global): over tiles of 16 consecutive time rows x all channels of one utterance
    (64 consecutive samples of a 1-D waveform; the last tile of an utterance may be short),
    the worst tile's rms(err) / rms(want of the whole tensor); and rms(err) / rms(want) of the
    whole tensor. A few wrong rows at one seam weigh as much as if every row were that wrong.
    A NaN anywhere makes both NaN."""
    tile, rw, _, re = _tiles(got, want)
    worst_tile = float("nan") if np.isnan(tile).any() else float(tile.max())
    return worst_tile / rw, re / rw


def worst(got, want):
    """Where the tile metric peaks: (utterance, first row of the tile, value)."""
    tile, rw, step, _ = _tiles(got, want)
    t = np.where(np.isnan(tile), np.inf, tile)
    b, i = np.unravel_index(int(np.argmax(t)), t.shape)
    return int(b), int(i) * step, float(t[b, i] / rw)


# ---------------------------------------------------------------- shared test inputs
# (tests/test_vocoder_tiles_host.py and tests/test_vocoder_tiles_gpu.py run the same cases)
UNIT_BM = {16: 240, 32: 240, 64: 176, 128: 112, 256: 112}     # tile heights of the fused units
UNIT_KD = [(3, 1), (7, 3), (11, 5)]                            # compiled (k, d) forms
RUNTIME_KD = [(1, 1), (5, 2), (9, 1), (9, 5), (11, 4)]         # run-time (k, d) forms, C >= 64
T_PERSIST = 7 * 240 + 5                                        # 8 tiles per utterance
T_PERSIST_ODD = 6 * 240 + 5                                    # 7: 14 tiles, no multiple of 8
POST_T = [4, 1020, 1024, 1028, 2048 + 512]
POST_T_UNALIGNED = [1022]                                      # T % 4 != 0: scalar stores
XCD_N = [1, 7, 8, 9, 14, 16, 50, 2757]
B = 2


def unit_Ts(C):
    bm = UNIT_BM[C]
    return [1, bm - 1, bm, bm + 1, 3 * bm + 7]


def runtime_Ts(C):
    return [UNIT_BM[C] + 1, 2 * UNIT_BM[C]]


def conv_bm(Cout):
    return 128 if Cout >= 128 else 256


def _gens(seed):
    """One generator per utterance (independently seeded) and one for the weights."""
    return [torch.Generator().manual_seed(seed * 7919 + 1 + b) for b in range(B)], \
        torch.Generator().manual_seed(seed * 7919)


def _per_utt(gens, *shape, scale=1.0):
    return torch.stack([torch.randn(*shape, generator=g) * scale for g in gens]).half()


@functools.lru_cache(maxsize=None)
def unit_inputs(C, k, d, T):
    """x, prev fp16 [2][T][C]; w1, w2 f32 [C][C][k]; b1, b2 f32 [C] (std 0.1)."""
    gens, gw = _gens(C * 100000 + k * 1000 + d * 100000000 + T)
    w1 = torch.randn(C, C, k, generator=gw) / math.sqrt(C * k)
    w2 = torch.randn(C, C, k, generator=gw) / math.sqrt(C * k)
    b1 = torch.randn(C, generator=gw) * 0.1
    b2 = torch.randn(C, generator=gw) * 0.1
    x = _per_utt(gens, T, C)
    prev = _per_utt(gens, T, C)
    return dict(x=x, prev=prev, w1=w1, b1=b1, w2=w2, b2=b2)


@functools.lru_cache(maxsize=None)
def unit_cores(C, k, d, T):
    """(exact, emulated) resunit_core of unit_inputs: shared by the epilogue variants."""
    i = unit_inputs(C, k, d, T)
    return tuple(resunit_core(i["x"], i["w1"], i["b1"], i["w2"], i["b2"], d, emulate=e) for e in (False, True))


def unit_refs(C, k, d, T, acc, post_silu):
    """(want, emulated) of the unit case: scale 1/3 with accumulate, else 1."""
    i = unit_inputs(C, k, d, T)
    ce, cm = unit_cores(C, k, d, T)
    kw = dict(scale=1 / 3 if acc else 1.0, prev=i["prev"] if acc else None, post_silu=bool(post_silu))
    return (resunit(None, None, None, None, None, d, core=ce, **kw),
            resunit(None, None, None, None, None, d, core=cm, emulate=True, **kw))


def conv_T_ins(case):
    """The T_in of a CONV_CASES geometry that put T_out at 1, BM - 1, BM, BM + 1 (plain convs:
    exactly; transposed: T_out = T_in * stride, the nearest) and, transposed, the row count
    per phase T_in + 1 at BM and BM + 1."""
    Cin, Cout, taps, stride, pad, dil, tr = case[:7]
    bm = conv_bm(Cout)
    if tr:
        return sorted({max(1, round(t / stride)) for t in (1, bm - 1, bm, bm + 1)} | {bm - 1, bm})
    return [max(1, (t - 1) * stride + dil * (taps - 1) + 1 - 2 * pad) for t in (1, bm - 1, bm, bm + 1)]


@functools.lru_cache(maxsize=None)
def conv_inputs(case, T_in):
    Cin, Cout, taps, stride, pad, dil, tr, pre, post, use_res, scale, acc, _ = case
    gens, gw = _gens(Cin * 1000003 + Cout * 1009 + taps * 31 + stride * 7 + T_in * 131071)
    if tr:
        w = torch.randn(Cin, Cout, 2 * stride, generator=gw) / math.sqrt(Cin * 2)
    else:
        w = torch.randn(Cout, Cin, taps, generator=gw) / math.sqrt(Cin * taps)
    bias = torch.randn(Cout, generator=gw) * 0.1
    T_out = conv_out_len(T_in, taps, stride, pad, dil, tr)
    x = _per_utt(gens, T_in, Cin)
    res = _per_utt(gens, T_out, Cout) if use_res else None
    prev = _per_utt(gens, T_out, Cout)
    return dict(x=x, w=w, bias=bias, res=res, prev=prev, T_out=T_out)


@functools.lru_cache(maxsize=None)
def conv_refs(case, T_in, post_acc_silu):
    Cin, Cout, taps, stride, pad, dil, tr, pre, post, use_res, scale, acc, _ = case
    i = conv_inputs(case, T_in)
    return tuple(conv1d(i["x"], i["w"], i["bias"], stride, pad, dil, bool(tr), pre, post, i["res"], scale,
                        i["prev"] if acc else None, bool(post_acc_silu), emulate=e) for e in (False, True))


@functools.lru_cache(maxsize=None)
def post_inputs(T):
    gens, gw = _gens(424243 + T)
    w = torch.randn(16, 13, generator=gw) * (0.35 / math.sqrt(16 * 13))
    return dict(x=_per_utt(gens, T, 16), w=w, bias=0.02)


@functools.lru_cache(maxsize=None)
def post_refs(T, pre_silu):
    """((wav, pre), (wav, pre) emulated)."""
    i = post_inputs(T)
    return tuple(conv_post(i["x"], i["w"], i["bias"], bool(pre_silu), emulate=e) for e in (False, True))


def latents(frames, n, latent_dim=512):
    """Seeded unit-normal latents fp16 [n][frames][latent_dim], each utterance its own seed."""
    return torch.stack([torch.randn(frames, latent_dim, generator=torch.Generator().manual_seed(9100 + 17 * b + frames))
                        for b in range(n)]).half()


_GEN = {}


def generator_refs(key, lat, W, cfg):
    """((wav, pre), (wav, pre) emulated) of generator(), kept per ``key``."""
    if key not in _GEN:
        _GEN[key] = tuple(generator(lat, W, cfg, emulate=e) for e in (False, True))
    return _GEN[key]
