"""Every decode path's residual stream against float64, per 16-column tile (MI355X).

janus_whisper_decode_hidden runs the decode call's own plan, buffers, uploads and launches on
forced tokens and hands back x after every position, the K / V caches and the plan that ran.
Each case asserts, from the plan text, that the path it names ran (a silent fallback fails
the case), then holds x of every (row, position) and the cache rows to tests/decoder_ref.py's
float64 ``hidden()`` on both metrics (row: |e| / |ref|; tile: the worst 16-column tile scaled
as if all tiles were that bad).

The bound is no fixed number: K_BOUND = 3 times the distance of ``hidden(emulate=True)`` (the
same arithmetic rounded where the engine stores fp16) from ``hidden()`` on the case's own
rows and positions, computed on the CPU — a property of the reference alone. The factor
allows for the fp32 accumulation order and the rounding points the emulation does not model
(fp16 probabilities as MFMA operands, split merges).

Engines: two decoder layers, no encoder layer, 64 vocabulary entries, 141 encoder keys
(two 64-key chunks plus 13) unless stated; the encoder output is seeded noise. T positions:
70 crosses the 64-key chunk of the decode attention; 3 where the row count is large.

Case families (d_model / heads):
  launch 512 / 8   rows 1, 17, 64, 65, 200 at T = 70; at 64 rows every LayerNorm placement
                   (mask 0, mask 15, RESID_LN, FUSED_LN, LN_FUSE), NO_XABSORB, NO_CVP and key
                   splits 1 / 3 / 8; at 65 and 200 rows CVP, cu_count 128 (msplit_n 1024) and
                   msplit_rows_n -1; 3 rows over 1500 keys at 8 splits
  launch 384 / 6   rows 5, 64 at the default and mask 15
  shared rows      13 rows over 3 encoder rows (5 + 5 + 3), T = 3: PAIR, XGROUP, NO_XPAIR at
                   512; gathered, XROWS(2), XROWS(4) at 768 / 12; plain 768 at 1 and 40 rows
  persistent 1-3   rows 1, 17, 40, 64, 128 at T = 3; 8 rows at T = 70; 256 rows on the whole
                   GPU; 256 rows at cu_count 128 plain (the BIG grid) and SEG_2CU; level 3 XFWD
  staggered        2 x 20 rows, launch path and persistent 2: 66 positions fresh, then 20
                   rows continuing at 66 beside 20 fresh rows for 4 positions
At 141 keys the plan clamps xattn_splits 8 to 3 (one 64-key chunk per split at least): the
8-split case runs there as 3 and at 1500 keys as 8. No case was dropped as unreachable.

Measured on the MI355X, row / tile, the maximum over the family's cases, with the emulation's
own figure on the same rows after the bar (the bound is three times that one):
  family         x                                        k cache tile        v cache tile
  launch 512     7.50e-4 / 1.13e-3 | 7.56e-4 / 1.16e-3    1.43e-3 | 1.35e-3   1.51e-3 | 1.38e-3
  launch 384     7.49e-4 / 1.08e-3 | 7.47e-4 / 1.12e-3    1.27e-3 | 1.38e-3   1.33e-3 | 1.41e-3
  launch 768     6.77e-4 / 1.04e-3 | 6.85e-4 / 1.07e-3    1.21e-3 | 1.28e-3   1.28e-3 | 1.32e-3
  shared rows    6.45e-4 / 8.69e-4 | 6.25e-4 / 8.56e-4    9.61e-4 | 9.97e-4   1.15e-3 | 1.18e-3
  persistent 1   7.00e-4 / 1.09e-3 | 7.05e-4 / 1.02e-3    1.28e-3 | 1.26e-3   1.28e-3 | 1.18e-3
  persistent 2   7.05e-4 / 1.09e-3 | 7.05e-4 / 1.02e-3    1.25e-3 | 1.26e-3   1.20e-3 | 1.18e-3
  persistent 3   7.03e-4 / 1.12e-3 | 7.05e-4 / 1.02e-3    1.25e-3 | 1.26e-3   1.20e-3 | 1.18e-3
  staggered      7.50e-4 / 1.13e-3 | 7.12e-4 / 1.04e-3    1.42e-3 | 1.30e-3   1.51e-3 | 1.38e-3
Every path sits at 0.9 - 1.1 times the emulation: the engine's error is its storage formats'.
The module's teardown prints these maxima (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import decoder_ref as ref
from janus_amd import whisper as jw

pytestmark = pytest.mark.gpu

T_LONG, T_SHORT = 70, 3
SEED_W, SEED_IN = 3, 5

# family -> (row, tile) of x on the GPU / of the emulation, cache tile likewise
MEASURED = {}


# ------------------------------------------------------------------ inputs and references
class Model:
    """One engine shape: its weights, master inputs (rows x T_LONG) and the references of
    them, computed once and sliced by the cases (the decoder is causal and its rows are
    independent, tests/test_decoder_hidden_host.py::test_causal_and_row_independent)."""

    def __init__(self, d, H, Te, rows_long, rows_short=0):
        self.cfg = ref.config(d, H, Te)
        self.W = ref.weights(self.cfg, SEED_W)
        self.rows_long = rows_long
        self.tokens, self.enc = ref.inputs(self.cfg, rows_long + rows_short, T_LONG, SEED_IN)
        self._engine = None
        self._enc_dev = None

    @functools.lru_cache(maxsize=None)
    def _ref(self, emulate, xabs):
        """(x, k, v): rows [0, rows_long) over T_LONG positions, the rest over T_SHORT."""
        n = self.rows_long
        a = ref.hidden(self.tokens[:n], self.enc[:n], self.W, self.cfg, emulate=emulate, xabs=xabs)
        if n == len(self.tokens):
            return a, None
        b = ref.hidden(self.tokens[n:, :T_SHORT], self.enc[n:], self.W, self.cfg, emulate=emulate, xabs=xabs)
        return a, b

    def reference(self, B, T, emulate=False, xabs=True):
        """x [B][T][d], k, v [layers][B][T][d] of the first B rows and T positions."""
        a, b = self._ref(emulate, xabs)
        if B <= self.rows_long:
            return a[0][:B, :T], a[1][:, :B, :T], a[2][:, :B, :T]
        assert T <= T_SHORT and b is not None
        m = B - self.rows_long
        return (np.concatenate([a[0][:, :T], b[0][:m, :T]]),
                np.concatenate([a[1][:, :, :T], b[1][:, :m, :T]], 1),
                np.concatenate([a[2][:, :, :T], b[2][:, :m, :T]], 1))

    @property
    def engine(self):
        if self._engine is None:
            self._engine = jw.WhisperEngine(self.cfg, self.W)
            self._enc_dev = torch.from_numpy(self.enc).cuda()
        return self._engine

    def enc_dev(self, n):
        self.engine
        return self._enc_dev[:n].contiguous()


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(d, H, Te=141):
        key = (d, H, Te)
        if key not in made:
            made[key] = {(512, 8, 141): lambda: Model(512, 8, 141, 200, 56),
                         (512, 8, 1500): lambda: Model(512, 8, 1500, 3),
                         (384, 6, 141): lambda: Model(384, 6, 141, 64),
                         (768, 12, 141): lambda: Model(768, 12, 141, 40)}[key]()
        return made[key]

    yield get
    made.clear()
    # the families' maxima (the module docstring's table; shown with -s / -rP)
    for (family, what), (g_row, g_tile, e_row, e_tile) in sorted(MEASURED.items()):
        print(f"MEASURED {family:14s} {what:8s} gpu row {g_row:.2e} tile {g_tile:.2e} | "
              f"emulation row {e_row:.2e} tile {e_tile:.2e}")


# --------------------------------------------------------------------------- the checks
def check_plan(plan, want):
    got = {k: plan[k] for k in want}
    assert got == want, f"the plan that ran differs from the case's path: {got} != {want}"


def hold(name, what, got, want, emu, family):
    """got against want on both metrics, bound K_BOUND x (emu against want)."""
    e_row, e_tile = ref.metrics(emu, want)
    g_row, g_tile = ref.metrics(got, want)
    print(f"{name} {what}: row {g_row:.2e} tile {g_tile:.2e} | emulation row {e_row:.2e} tile {e_tile:.2e}")
    m = MEASURED.setdefault((family, what), [0.0, 0.0, 0.0, 0.0])
    m[:] = [max(m[0], g_row), max(m[1], g_tile), max(m[2], e_row), max(m[3], e_tile)]
    at, col, val = ref.worst(got, want)
    where = f"{what} index {at} (x: row, position; cache: layer, row, slot), columns {col}-{col + 15}"
    assert np.isfinite(g_tile) and g_tile <= ref.K_BOUND * e_tile, \
        f"{name}: {where}: tile {val:.2e} is {val / (ref.K_BOUND * e_tile):.1f}x the bound {ref.K_BOUND * e_tile:.2e}"
    assert g_row <= ref.K_BOUND * e_row, \
        f"{name}: {where}: row {g_row:.2e} is {g_row / (ref.K_BOUND * e_row):.1f}x the bound {ref.K_BOUND * e_row:.2e}"


def run_case(M, name, family, B, T, plan_want, xabs=True, **opts):
    out = M.engine.decode_hidden(M.enc_dev(B), M.tokens[:B, :T], **opts)
    check_plan(out.plan, dict(B=B, **plan_want))
    x = out.x.transpose(0, 1).double().cpu().numpy()                       # [B][T][d]
    kc = out.kc[:, :, :T].double().cpu().numpy()
    vc = out.vc[:, :, :T].double().cpu().numpy()
    rx, rk, rv = M.reference(B, T)
    ex, ek, ev = M.reference(B, T, emulate=True, xabs=xabs)
    hold(name, "x", x, rx, ex, family)
    hold(name, "k cache", kc, rk, ek, family)
    hold(name, "v cache", vc, rv, ev, family)


# ------------------------------------------------------------ launch path, d 512 / 8 heads
LAUNCH = dict(persist=0, seg_grid=0, xabs=1, npairs=0, ngroups=0, grp_rows=0, fused_ln=0, ln_fuse=0, rln=0)
LAUNCH["call.enc_rows"] = 0
SMALL = dict(LAUNCH, ln_pro_mask=9, cvp=1, xsplit=3, msplit_n=0)    # <= 64 rows, the whole GPU
LARGE = dict(LAUNCH, ln_pro_mask=0, cvp=0, xsplit=3, msplit_n=0)    # above 64 rows

CASES_512 = [
    ("rows1", 1, SMALL, {}),
    ("rows17", 17, SMALL, {}),
    ("rows64", 64, SMALL, {}),
    ("rows65", 65, LARGE, {}),
    ("rows200", 200, LARGE, {}),
    ("rows64-lnmask0", 64, dict(SMALL, ln_pro_mask=0), dict(path_flags=jw.dec_path_ln_mask(0))),
    ("rows64-lnmask15", 64, dict(SMALL, ln_pro_mask=15), dict(path_flags=jw.dec_path_ln_mask(15))),
    ("rows64-resid-ln", 64, dict(SMALL, rln=1), dict(path_flags=jw.DEC_PATH_RESID_LN)),
    ("rows64-fused-ln", 64, dict(SMALL, fused_ln=1, ln_pro_mask=0), dict(path_flags=jw.DEC_PATH_FUSED_LN)),
    ("rows64-ln-fuse", 64, dict(SMALL, ln_fuse=1, ln_pro_mask=0), dict(path_flags=jw.DEC_PATH_LN_FUSE)),
    ("rows64-no-xabsorb", 64, dict(SMALL, xabs=0), dict(path_flags=jw.DEC_PATH_NO_XABSORB)),
    ("rows64-no-cvp", 64, dict(SMALL, cvp=0), dict(path_flags=jw.DEC_PATH_NO_CVP)),
    ("rows64-splits1", 64, dict(SMALL, xsplit=1), dict(xattn_splits=1)),
    ("rows64-splits3", 64, dict(SMALL, xsplit=3), dict(xattn_splits=3)),
    ("rows64-splits8", 64, dict(SMALL, xsplit=3), dict(xattn_splits=8)),   # clamped: 3 chunks of keys
]
for _b in (65, 200):
    CASES_512 += [
        (f"rows{_b}-cvp", _b, dict(LARGE, cvp=1), dict(path_flags=jw.DEC_PATH_CVP)),
        (f"rows{_b}-cu128", _b, dict(LARGE, msplit_n=1024), dict(cu_count=128)),
        (f"rows{_b}-no-msplit", _b, dict(LARGE, msplit_n=0), dict(msplit_rows_n=-1)),
    ]


@pytest.mark.parametrize("name,B,plan,opts", CASES_512, ids=[c[0] for c in CASES_512])
def test_launch_path_512(models, name, B, plan, opts):
    run_case(models(512, 8), name, "launch 512", B, T_LONG, plan, xabs=bool(plan["xabs"]), **opts)


def test_launch_path_512_1500_keys(models):
    """The real key count (23 x 64 + 28) at 8 key splits."""
    run_case(models(512, 8, 1500), "keys1500", "launch 512", 3, T_LONG, dict(SMALL, xsplit=8), xattn_splits=8)


# ------------------------------------------------------------ launch path, d 384 / 6 heads
CASES_384 = [
    ("rows5", 5, SMALL, {}),
    ("rows64", 64, SMALL, {}),
    ("rows5-lnmask15", 5, dict(SMALL, ln_pro_mask=15), dict(path_flags=jw.dec_path_ln_mask(15))),
    ("rows64-lnmask15", 64, dict(SMALL, ln_pro_mask=15), dict(path_flags=jw.dec_path_ln_mask(15))),
]


@pytest.mark.parametrize("name,B,plan,opts", CASES_384, ids=[c[0] for c in CASES_384])
def test_launch_path_384(models, name, B, plan, opts):
    run_case(models(384, 6), name, "launch 384", B, T_LONG, plan, **opts)


# ------------------------------------------------------------ d 768 / 12 heads
WIDE = dict(LAUNCH, wide=1, ln_pro_mask=0, cvp=0, xsplit=3)


@pytest.mark.parametrize("B", [1, 40])
def test_launch_path_768(models, B):
    run_case(models(768, 12), f"rows{B}", "launch 768", B, T_LONG, WIDE)


# ------------------------------------------------------------ shared encoder rows
ENC_INDEX = [0] * 5 + [1] * 5 + [2] * 3
IN_PLACE, GATHERED = 1, 2
PAIRS = [0, 1, 0, 2, 3, 0, 4, -1, 0, 5, 6, 1, 7, 8, 1, 9, -1, 1, 10, 11, 2, 12, -1, 2]

SHARED = [
    ("512-pair", (512, 8), {}, dict(npairs=8, ngroups=0, pairs=PAIRS, cvp=1, **{"call.enc_rows": IN_PLACE})),
    ("512-xgroup", (512, 8), dict(path_flags=jw.DEC_PATH_XGROUP),
     dict(npairs=0, ngroups=3, grp_rows=5, cvp=1, **{"call.enc_rows": IN_PLACE})),
    ("512-no-xpair", (512, 8), dict(path_flags=jw.DEC_PATH_NO_XPAIR),
     dict(npairs=0, ngroups=0, **{"call.enc_rows": GATHERED})),
    ("768-gathered", (768, 12), {}, dict(npairs=0, ngroups=0, wide=1, **{"call.enc_rows": GATHERED})),
    ("768-xrows2", (768, 12), dict(path_flags=jw.dec_path_xrows(2)),
     dict(npairs=0, ngroups=8, n_main=5, grp_rows=2, rem_rows=1, wide=1, **{"call.enc_rows": IN_PLACE})),
    ("768-xrows4", (768, 12), dict(path_flags=jw.dec_path_xrows(4)),
     dict(npairs=0, ngroups=5, n_main=2, grp_rows=4, rem_rows=3, wide=1, **{"call.enc_rows": IN_PLACE})),
]


@pytest.mark.parametrize("name,shape,opts,plan", SHARED, ids=[c[0] for c in SHARED])
def test_shared_encoder_rows(models, name, shape, opts, plan):
    """13 rows over 3 encoder rows (5 + 5 + 3): row b against hidden() on enc[enc_index[b]]."""
    M = models(*shape)
    B, T = len(ENC_INDEX), T_SHORT
    out = M.engine.decode_hidden(M.enc_dev(3), M.tokens[:B, :T], enc_index=ENC_INDEX, **opts)
    check_plan(out.plan, dict(B=B, persist=0, xabs=1, **plan))
    exact = ref.hidden(M.tokens[:B, :T], M.enc[:3], M.W, M.cfg, enc_index=ENC_INDEX)
    emu = ref.hidden(M.tokens[:B, :T], M.enc[:3], M.W, M.cfg, enc_index=ENC_INDEX, emulate=True)
    got = (out.x.transpose(0, 1), out.kc[:, :, :T], out.vc[:, :, :T])
    for what, g, r, e in zip(("x", "k cache", "v cache"), got, exact, emu):
        hold(name, what, g.double().cpu().numpy(), r, e, "shared rows")


# ------------------------------------------------------------ persistent levels, d 512
def seg_grid(B, cus):
    """dec_seg_grid's one-block-per-CU answer (dec_persist.hip), restated."""
    mt = 1
    while mt * 16 < B:
        mt *= 2
    for ng in (32, 16):
        if mt * ng <= cus:
            return mt * ng
    return 8 * mt if mt == 16 and 8 * mt <= cus else 0


PERSIST = [(f"level{lv}-rows{B}", lv, B, T_SHORT, {}, dict(seg_grid=seg_grid(B, 256)))
           for lv in (1, 2, 3) for B in (1, 17, 40, 64, 128, 256)]
PERSIST += [(f"level{lv}-rows8-T70", lv, 8, T_LONG, {}, dict(seg_grid=32)) for lv in (1, 2, 3)]
PERSIST += [(f"level{lv}-rows256-cu128-big", lv, 256, T_SHORT, dict(cu_count=128), dict(seg_grid=128))
            for lv in (1, 2, 3)]
PERSIST += [(f"level{lv}-rows256-cu128-2cu", lv, 256, T_SHORT,
             dict(cu_count=128, path_flags=jw.DEC_PATH_SEG_2CU), dict(seg_grid=256)) for lv in (1, 2, 3)]
PERSIST += [("level3-rows64-xfwd", 3, 64, T_SHORT, dict(path_flags=jw.DEC_PATH_XFWD), dict(seg_grid=128, xrev=0))]


@pytest.mark.parametrize("name,level,B,T,opts,plan", PERSIST, ids=[c[0] for c in PERSIST])
def test_persistent(models, name, level, B, T, opts, plan):
    """MT = 1 .. 16 m-tiles (17 and 40 rows leave empty rows inside their tiles), the 256-row
    grid on the whole GPU, the 128-block BIG grid and two blocks per CU on half of it."""
    want = dict(dict(persist=level, xabs=1, xrev=1, fused_ln=0, ln_fuse=0, rln=0, npairs=0, ngroups=0,
                     grp_rows=0), **plan)
    want["call.cus"], want["call.enc_rows"] = opts.get("cu_count", 256), 0
    run_case(models(512, 8), name, f"persistent {level}", B, T, want, persistent=level, **opts)


# ------------------------------------------------------------ staggered rows
@pytest.mark.parametrize("level", [0, 2], ids=["launch", "persistent2"])
def test_staggered(models, level):
    """2 x 20 rows. Call 1: all rows fresh, 66 positions. Call 2: rows 0 .. 19 continue at 66
    beside rows 20 .. 39 starting again, 4 positions: per-row offsets, the cache write at
    pos + roff[r] and key counts on both sides of the 64-key chunk, every (row, position)
    against hidden() of the row's own sequence."""
    M = models(512, 8)
    B, first, more = 40, 66, 4
    eng, enc = M.engine, M.enc_dev(B)
    tokens = M.tokens[:B, :first + more]
    rx, rk, rv = M.reference(B, first + more)
    ex, ek, ev = M.reference(B, first + more, emulate=True)
    want = dict(B=B, persist=level, stagger=1, xabs=1, seg_grid=seg_grid(B, 256) if level else 0)
    name = f"staggered-{level}"

    one = eng.decode_hidden(enc, tokens, pos_offset=[0] * B, steps=first, persistent=level)
    check_plan(one.plan, dict(want, max_roff=0))
    assert eng.decode_stand(B) == [first] * B
    hold(name + " call 1", "x", one.x.transpose(0, 1).double().cpu().numpy(), rx[:, :first], ex[:, :first],
         "staggered")

    off = [first] * 20 + [0] * 20
    two = eng.decode_hidden(enc, tokens, pos_offset=off, steps=more, persistent=level)
    check_plan(two.plan, dict(want, max_roff=first))
    assert eng.decode_stand(B) == [first + more] * 20 + [more] * 20
    x2 = two.x.transpose(0, 1).double().cpu().numpy()
    hold(name + " call 2 continuing", "x", x2[:20], rx[:20, first:], ex[:20, first:], "staggered")
    hold(name + " call 2 fresh", "x", x2[20:], rx[20:, :more], ex[20:, :more], "staggered")
    # the caches after both calls: the continuing rows' 70 slots, the restarted rows' 66
    for what, g, r, e in (("k cache", two.kc, rk, ek), ("v cache", two.vc, rv, ev)):
        g = g[:, :, :first + more].double().cpu().numpy()
        hold(name, what, g[:, :20], r[:, :20], e[:, :20], "staggered")
        hold(name, what, g[:, 20:, :first], r[:, 20:, :first], e[:, 20:, :first], "staggered")


def test_probe_rejections(models):
    """The probe plans as a decode call does: a continuing row past its slot's stand is an error
    before anything runs."""
    from janus_amd._native import JanusNativeError
    M = models(512, 8)
    eng, enc = M.engine, M.enc_dev(2)
    eng.decode_hidden(enc, M.tokens[:2, :8], pos_offset=[0, 0], steps=4)
    with pytest.raises(JanusNativeError, match="stands at 4"):
        eng.decode_hidden(enc, M.tokens[:2, :8], pos_offset=[5, 0], steps=2)


def test_engine_defect_is_seen(models):
    """The comparison end to end: an engine whose fc2 bias of layer 1 is zeroed on columns
    208 .. 223 (the host test's seeded defect, uploaded as a weight) lies more than 3x over
    the bound against the clean reference, at exactly that tile."""
    M = models(512, 8)
    B, T, name = 17, T_SHORT, "decoder.layers.1.fc2.bias"
    bad = M.W[name].copy()
    bad[208:224] = 0.0
    eng = M.engine
    eng.set_tensor(name, bad)
    try:
        out = eng.decode_hidden(M.enc_dev(B), M.tokens[:B, :T])
    finally:
        eng.set_tensor(name, M.W[name])
    x = out.x.transpose(0, 1).double().cpu().numpy()
    rx, _, _ = M.reference(B, T)
    ex, _, _ = M.reference(B, T, emulate=True)
    _, col, tile = ref.worst(x, rx)
    bound = ref.K_BOUND * ref.metrics(ex, rx)[1]
    print(f"engine defect: tile {tile:.2e} = {tile / bound:.1f}x the bound at columns {col}-{col + 15}")
    assert col == 208 and tile > 3 * bound, (col, tile, bound)
