"""The vocoder's kernels against float64 per 16-row tile, at tile edges, in every dispatch form (MI355X).

Each case runs one kernel through the kernel ABI (include/janus_kernels.h) on B = 2 independently
seeded utterances with a nonzero accumulator, into an output that is NaN where the kernel does
not accumulate and over-allocated by 32 guard rows that must come back untouched, and holds
it to tests/vocoder_ref.py's float64 reference on two distances: the worst tile (16 time rows
x all channels of one utterance, 64 samples of a waveform) and the whole tensor, both over the
reference's rms. The bound is no fixed number: decoder_ref.K_BOUND = 3 times the distance of
the reference's own emulation (fp16 where the kernels store or stage it) on the same inputs.
A failure names the worst tile.

  fused units   C 16 .. 256 x (k, d) (3, 1), (7, 3), (11, 5) x accumulate x post_silu at T = 1,
                BM - 1, BM, BM + 1, 3 BM + 7 (BM: 240 narrow, 176 at C = 64, 112 at 128 / 256)
  persistent    C 16 / 32 at T = 7 x 240 + 5 (16 tiles) on 3 and on 8 blocks, and at 6 x 240 + 5
                (14 tiles: C = 32 remaps its tile order on 8 blocks, 14 being no multiple of 8):
                held to the bound and bit-identical to the uncapped grid
  run-time      C 64 / 128 / 256 at (k, d) (1, 1), (5, 2), (9, 1), (9, 5), (11, 4), T = BM + 1, 2 BM
  rejections    narrow k = 5, narrow d = 2, wide (k - 1) d = 60: JanusNativeError, nothing written
  conv          tests/test_kernels_gpu.py's CONV_CASES geometries at T_out = 1, BM - 1, BM, BM + 1
                (BM 128 at Cout >= 128, else 256; transposed: the nearest, and BM / BM + 1 rows
                per phase) x post_acc_silu; tile orders 0 .. 3 bit-identical to the default
  conv_post     T = 4, 1020, 1022, 1024, 1028, 2560 x pre_silu: waveform and pre-tanh on the 64-sample
                tile; PCM equal to the reference quantisation of the GPU's own waveform
  xcd_remap     a permutation of range(n) at n = 1, 7, 8, 9, 14, 16, 50, 2757
  forward       VocoderEngine.forward at 4 and 23 frames, B = 2, pre-tanh and waveform against
                vocoder_ref.generator; dilations (1, 3, 7) (no fused unit takes d = 7: those
                units run as conv pairs) at 4 frames
  defect        C = 64, k = 7, d = 3 with b2 zeroed on channels 16 - 31 stands over 3 x the bound

Measured on the MI355X, tile / global, the maximum over the family's cases, with the
emulation's own figure on the same inputs after the bar (the bound is three times that one):
  family                 tile                    global
  unit C=16              3.59e-4 | 3.59e-4       2.54e-4 | 2.54e-4
  unit C=16 persistent   3.15e-4 | 3.15e-4       2.43e-4 | 2.43e-4
  unit C=32              3.47e-4 | 3.47e-4       2.63e-4 | 2.63e-4
  unit C=32 persistent   2.76e-4 | 2.76e-4       2.46e-4 | 2.46e-4
  unit C=64              3.02e-4 | 3.02e-4       2.52e-4 | 2.52e-4
  unit C=64 run-time     2.58e-4 | 2.58e-4       2.17e-4 | 2.17e-4
  unit C=128             2.89e-4 | 2.89e-4       2.53e-4 | 2.53e-4
  unit C=128 run-time    2.51e-4 | 2.51e-4       2.17e-4 | 2.17e-4
  unit C=256             2.67e-4 | 2.68e-4       2.52e-4 | 2.52e-4
  unit C=256 run-time    2.41e-4 | 2.41e-4       2.16e-4 | 2.15e-4
  conv Cout<=64          5.12e-4 | 5.12e-4       4.15e-4 | 4.15e-4
  conv Cout>=128         4.28e-4 | 4.28e-4       3.66e-4 | 3.66e-4
  conv_post pre-tanh     4.06e-7 | 3.88e-7       2.93e-7 | 2.90e-7
  conv_post waveform     3.43e-7 | 3.46e-7       2.80e-7 | 2.80e-7
  forward pre-tanh       2.91e-3 | 2.42e-3       1.48e-3 | 1.46e-3
  forward waveform       2.41e-3 | 2.27e-3       1.52e-3 | 1.50e-3
  conv pairs pre-tanh    2.11e-3 | 2.08e-3       1.42e-3 | 1.42e-3
  conv pairs waveform    2.08e-3 | 2.03e-3       1.42e-3 | 1.41e-3
A single kernel sits on its emulation to three digits: its one fp16 store decides the error,
and the fp32 accumulation order under it rarely moves a value across a rounding boundary.
Only the chained forward (52 launches) drifts, to 1.2 times the emulation on its worst tile.
No case found a wrong value: the run-time (k, d) forms, the persistent loop, the remapped
tile orders and every conv tile order are right as they stand. The module's teardown prints
these maxima (pytest -s).
"""
import numpy as np
import pytest
import torch

import decoder_ref
import vocoder_ref as vr
from janus_amd import _native as nat
from test_kernels_gpu import CONV_CASES

pytestmark = pytest.mark.gpu

K = decoder_ref.K_BOUND
GUARD_ROWS = 32
MEASURED = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for fam, (g_t, g_g, e_t, e_g) in sorted(MEASURED.items()):
        print(f"MEASURED {fam:18s} gpu tile {g_t:.2e} global {g_g:.2e} | emulation tile {e_t:.2e} global {e_g:.2e}")


def hold(name, family, got, want, emu):
    """got against want on both metrics, bound K_BOUND x (emu against want)."""
    e_tile, e_glob = vr.metrics(emu, want)
    g_tile, g_glob = vr.metrics(got, want)
    print(f"{name}: tile {g_tile:.2e} global {g_glob:.2e} | emulation tile {e_tile:.2e} global {e_glob:.2e}")
    m = MEASURED.setdefault(family, [0.0, 0.0, 0.0, 0.0])
    m[:] = [max(m[0], g_tile), max(m[1], g_glob), max(m[2], e_tile), max(m[3], e_glob)]
    b, row, val = vr.worst(got, want)
    where = f"worst tile: utterance {b}, rows {row}..{row + (vr.TILE_ROWS if want.ndim == 3 else vr.TILE_SAMPLES) - 1}"
    assert e_tile > 0 and e_glob > 0
    assert np.isfinite(g_tile) and g_tile <= K * e_tile, \
        f"{name}: {where}: tile {val:.2e} is {val / (K * e_tile):.1f}x the bound {K * e_tile:.2e}"
    assert np.isfinite(g_glob) and g_glob <= K * e_glob, \
        f"{name}: {where}: global {g_glob:.2e} is {g_glob / (K * e_glob):.1f}x the bound {K * e_glob:.2e}"


class Out:
    """An fp16 [B][T][C] output followed by GUARD_ROWS rows the kernel must not touch: prev
    where the kernel accumulates, else NaN."""

    def __init__(self, gpu, prev, acc, dtype=torch.float16):
        Bn, T = prev.shape[:2]
        self.shape = prev.shape
        n = prev.numel()
        self.buf = torch.empty(n + GUARD_ROWS * (n // (Bn * T)), dtype=dtype, device=gpu)
        self.buf[n:] = 1234.0
        self.buf[:n] = prev.to(gpu).reshape(-1).to(dtype) if acc else float("nan")
        self.n = n

    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        """The [B][T][C] part (a device tensor); the guard rows are checked here."""
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == 1234.0).all()), "rows at index >= T were written"
        return self.buf[:self.n].reshape(self.shape)


def pack_unit(gpu, C, k, w):
    n = nat.lib().janus_resunit_packed_size(C, k)
    p = torch.empty(n, dtype=torch.float16, device=gpu)
    dw = w.float().contiguous().to(gpu)
    nat.call("janus_resunit_pack", dw.data_ptr(), p.data_ptr(), C, k, stream())
    torch.cuda.synchronize()
    return p


class Unit:
    """A unit case's device side: packed weights and inputs, kept for its launches."""

    def __init__(self, gpu, C, k, d, T, b2=None):
        self.C, self.k, self.d, self.T, self.gpu = C, k, d, T, gpu
        self.i = i = vr.unit_inputs(C, k, d, T)
        self.p1, self.p2 = pack_unit(gpu, C, k, i["w1"]), pack_unit(gpu, C, k, i["w2"])
        self.x, self.b1 = i["x"].to(gpu), i["b1"].to(gpu)
        self.b2 = (i["b2"] if b2 is None else b2).to(gpu)

    def run(self, acc, post_silu, max_blocks=0, entry="ex"):
        out = Out(self.gpu, self.i["prev"], acc)
        scale = 1 / 3 if acc else 1.0
        args = [self.x.data_ptr(), out.ptr(), self.p1.data_ptr(), self.b1.data_ptr(), self.p2.data_ptr(),
                self.b2.data_ptr(), vr.B, self.T, self.C, self.k, self.d, scale, acc]
        if entry == "ex":
            nat.call("janus_resunit_f16_ex", *args, post_silu, max_blocks, stream())
        else:
            nat.call("janus_resunit_f16", *args, stream())
        return out.get()


# ------------------------------------------------------------------------------ fused units
@pytest.mark.parametrize("post_silu", [0, 1])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("k,d", vr.UNIT_KD)
@pytest.mark.parametrize("C", sorted(vr.UNIT_BM))
def test_unit_tile_edges(gpu, C, k, d, acc, post_silu):
    for T in vr.unit_Ts(C):
        got = Unit(gpu, C, k, d, T).run(acc, post_silu)
        want, emu = vr.unit_refs(C, k, d, T, acc, post_silu)
        hold(f"unit C={C} k={k} d={d} acc={acc} silu={post_silu} T={T}", f"unit C={C}", got, want, emu)


@pytest.mark.parametrize("C", [16, 32, 64, 128, 256])
def test_unit_ex_entry_matches_plain_entry(gpu, C):
    """janus_resunit_f16_ex(post_silu = 0, max_blocks = 0) is janus_resunit_f16, bit for bit."""
    T = vr.UNIT_BM[C] + 1
    u = Unit(gpu, C, 7, 3, T)
    assert torch.equal(u.run(1, 0), u.run(1, 0, entry="plain"))


@pytest.mark.parametrize("k,d,acc,post_silu", [(3, 1, 0, 0), (7, 3, 1, 1), (11, 5, 1, 0)])
@pytest.mark.parametrize("C", [16, 32])
def test_unit_persistent_loop(gpu, C, k, d, acc, post_silu):
    """Few blocks, many tiles each: the next tile's register prefetch, the LDS reuse between
    iterations and the barriers between them; at C = 32 on 8 blocks the remapped tile order.
    No tile order may change a value."""
    for T, caps in ((vr.T_PERSIST, (3, 8)), (vr.T_PERSIST_ODD, (8,))):
        u = Unit(gpu, C, k, d, T)
        base = u.run(acc, post_silu)
        want, emu = vr.unit_refs(C, k, d, T, acc, post_silu)
        hold(f"persistent C={C} k={k} d={d} T={T} uncapped", f"unit C={C} persistent", base, want, emu)
        for cap in caps:
            got = u.run(acc, post_silu, max_blocks=cap)
            hold(f"persistent C={C} k={k} d={d} T={T} blocks={cap}", f"unit C={C} persistent", got, want, emu)
            assert torch.equal(got, base), f"max_blocks = {cap} changed values"


@pytest.mark.parametrize("k,d", vr.RUNTIME_KD)
@pytest.mark.parametrize("C", [64, 128, 256])
def test_unit_runtime_forms(gpu, C, k, d):
    """(k, d) outside {3, 7, 11} x {1, 3, 5}: resunit_wide_kernel<C, 0, 0> and
    resunit_wide_lds_kernel<64, 0, 0>, k and d at run time, the residual re-read."""
    for T in vr.runtime_Ts(C):
        got = Unit(gpu, C, k, d, T).run(1, 1)
        want, emu = vr.unit_refs(C, k, d, T, 1, 1)
        hold(f"run-time C={C} k={k} d={d} T={T}", f"unit C={C} run-time", got, want, emu)


@pytest.mark.parametrize("C,k,d", [(16, 5, 1), (32, 5, 3), (16, 3, 2), (32, 11, 2), (64, 11, 6), (128, 11, 6),
                                   (256, 11, 6)])
def test_unit_rejections(gpu, C, k, d):
    T = 40
    x = torch.randn(vr.B, T, C, generator=torch.Generator().manual_seed(1)).half().to(gpu)
    w = torch.zeros(nat.lib().janus_resunit_packed_size(C, k), dtype=torch.float16, device=gpu)
    b = torch.zeros(C, device=gpu)
    out = torch.full((vr.B, T, C), float("nan"), dtype=torch.float16, device=gpu)
    for entry, extra in (("janus_resunit_f16", ()), ("janus_resunit_f16_ex", (0, 0))):
        with pytest.raises(nat.JanusNativeError):
            nat.call(entry, x.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(), w.data_ptr(), b.data_ptr(),
                     vr.B, T, C, k, d, 1.0, 0, *extra, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_unit_defect_is_seen(gpu):
    """The counterpart of test_engine_defect_is_seen: a unit that drops b2 on one 16-column
    group (C = 64, k = 7, d = 3) stands over three times the bound on the tile metric."""
    C, k, d, T = 64, 7, 3, vr.UNIT_BM[64] + 1
    i = vr.unit_inputs(C, k, d, T)
    b2 = i["b2"].clone()
    b2[16:32] = 0.0
    got = Unit(gpu, C, k, d, T, b2=b2).run(0, 0)
    want, emu = vr.unit_refs(C, k, d, T, 0, 0)
    e_tile, _ = vr.metrics(emu, want)
    g_tile, _ = vr.metrics(got, want)
    print(f"defect: tile {g_tile:.2e}, bound {K * e_tile:.2e}")
    assert g_tile > 3 * K * e_tile, (g_tile, e_tile)


# ------------------------------------------------------------------------------------- conv
def run_conv(gpu, case, T_in, post_acc_silu, remap, packed=None):
    Cin, Cout, taps, stride, pad, dil, tr, pre, post, use_res, scale, acc, _ = case
    i = vr.conv_inputs(case, T_in)
    T_out = i["T_out"]
    if packed is None:
        packed = torch.empty(nat.lib().janus_conv1d_packed_size(Cin, Cout, taps, tr, stride), dtype=torch.float16,
                             device=gpu)
        dw = i["w"].float().contiguous().to(gpu)
        nat.call("janus_conv1d_pack", dw.data_ptr(), packed.data_ptr(), Cin, Cout, taps, tr, stride, stream())
        torch.cuda.synchronize()
    dx, db = i["x"].to(gpu), i["bias"].to(gpu)
    dres = i["res"].to(gpu) if use_res else None
    out = Out(gpu, i["prev"], acc)
    args = [dx.data_ptr(), vr.B, T_in, Cin, packed.data_ptr(), db.data_ptr(), out.ptr(), T_out, Cout, taps, stride,
            pad, dil, tr, pre, post, dres.data_ptr() if use_res else None, T_out * Cout, scale, acc]
    if remap is None:
        nat.call("janus_conv1d_f16", *args, stream())
    else:
        nat.call("janus_conv1d_f16_ex", *args, post_acc_silu, remap, stream())
    return out.get(), packed


@pytest.mark.parametrize("post_acc_silu", [0, 1])
@pytest.mark.parametrize("ci", range(len(CONV_CASES)))
def test_conv_tile_edges(gpu, ci, post_acc_silu):
    case = CONV_CASES[ci]
    fam = "conv Cout>=128" if case[1] >= 128 else "conv Cout<=64"
    for T_in in vr.conv_T_ins(case):
        got, packed = run_conv(gpu, case, T_in, post_acc_silu, -1)
        want, emu = vr.conv_refs(case, T_in, post_acc_silu)
        assert got.shape == want.shape
        hold(f"conv {case[:7]} T_in={T_in} silu={post_acc_silu}", fam, got, want, emu)
        for remap in (0, 1, 2, 3):
            other, _ = run_conv(gpu, case, T_in, post_acc_silu, remap, packed)
            assert torch.equal(other, got), f"remap = {remap} changed values"
        if not post_acc_silu:
            plain, _ = run_conv(gpu, case, T_in, 0, None, packed)
            assert torch.equal(plain, got), "janus_conv1d_f16_ex(0, -1) differs from janus_conv1d_f16"


# -------------------------------------------------------------------------------- conv_post
@pytest.mark.parametrize("pre_silu", [0, 1])
def test_conv_post(gpu, pre_silu):
    """Block seams at 1024 samples, the +-6-row halo at both ends of an utterance, the PCM
    bytes; T = 1022 takes the scalar stores of a T that is no multiple of 4."""
    for T in vr.POST_T + vr.POST_T_UNALIGNED:
        i = vr.post_inputs(T)
        dx, dw = i["x"].to(gpu), i["w"].float().contiguous().to(gpu)
        blank = torch.zeros(vr.B, T)
        wav, pre = Out(gpu, blank, 0, torch.float32), Out(gpu, blank, 0, torch.float32)
        pcm = Out(gpu, blank, 1, torch.int16)
        nat.call("janus_conv_post_f32", dx.data_ptr(), vr.B, T, dw.data_ptr(), i["bias"], pre_silu, wav.ptr(),
                 pcm.ptr(), pre.ptr(), stream())
        (w_want, p_want), (w_emu, p_emu) = vr.post_refs(T, pre_silu)
        g_wav = wav.get().cpu().numpy()
        hold(f"conv_post T={T} silu={pre_silu} pre-tanh", "conv_post pre", pre.get().cpu().numpy(), p_want, p_emu)
        hold(f"conv_post T={T} silu={pre_silu} waveform", "conv_post wav", g_wav, w_want, w_emu)
        assert np.array_equal(pcm.get().cpu().numpy(), vr.pcm16(g_wav))
        # without the optional outputs: the same waveform
        wav2 = Out(gpu, blank, 0, torch.float32)
        nat.call("janus_conv_post_f32", dx.data_ptr(), vr.B, T, dw.data_ptr(), i["bias"], pre_silu, wav2.ptr(),
                 None, None, stream())
        assert np.array_equal(wav2.get().cpu().numpy(), g_wav)


# -------------------------------------------------------------------------------- xcd_remap
@pytest.mark.parametrize("n", vr.XCD_N)
def test_xcd_remap_is_a_permutation(gpu, n):
    out = torch.full((n + 8,), -7, dtype=torch.int32, device=gpu)
    nat.call("janus_xcd_remap_i32", n, out.data_ptr(), stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == -7).all()
    assert sorted(got[:n].tolist()) == list(range(n))
    if n >= 8:   # the blocks of XCD x (i % 8 == x) hold one contiguous run of tiles
        for x in range(8):
            run = got[:n][x::8]
            assert (np.diff(run) == 1).all()


# ---------------------------------------------------------------------------------- forward
def forward_case(gpu, frames, n, dil):
    from janus_amd.vocoder import FireflyConfig, VocoderEngine, synthetic_weights
    cfg = FireflyConfig(rb_dilations=tuple(dil))
    W = synthetic_weights(cfg, seed=2)
    lat = vr.latents(frames, n)
    eng = VocoderEngine(cfg, W)
    wav, pcm, pre = eng.forward(lat.to(gpu), want_pre_tanh=True)
    torch.cuda.synchronize()
    (w_want, p_want), (w_emu, p_emu) = vr.generator_refs((frames, n, tuple(dil)), lat, W, cfg)
    name = f"forward frames={frames} B={n} dilations={tuple(dil)}"
    fam = "forward" if tuple(dil) == (1, 3, 5) else "forward conv pairs"
    hold(name + " pre-tanh", fam + " pre", pre.cpu().numpy(), p_want, p_emu)
    hold(name + " waveform", fam + " wav", wav.cpu().numpy(), w_want, w_emu)
    assert np.array_equal(pcm.cpu().numpy(), vr.pcm16(wav.cpu().numpy()))


@pytest.mark.parametrize("frames", [4, 23])
def test_forward(gpu, frames):
    forward_case(gpu, frames, 2, (1, 3, 5))


def test_forward_unsupported_dilation_runs_as_conv_pairs(gpu):
    """No fused unit takes d = 7 (narrow: d in {1, 3, 5}; wide: (k - 1) d <= 50 fails at k = 11):
    those units run as the two-conv path, the others stay fused, and the generator matches."""
    forward_case(gpu, 4, 1, (1, 3, 7))
