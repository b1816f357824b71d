"""The int8 cross-attention operand on the MI355X (WhisperEngine(cfg, cross_compute="int8"),
include/janus.h janus_whisper_set_cross_compute).

With int8 every decode call quantises its encoder rows E per key (CTranslate2's rule) and the
cross-attention reads E' = fp16(float(q) * s). So the references are the existing ones on
another input: tests/decoder_ref.py's float64 ``hidden(tokens, E')``, E' from
tests/cross_int8_ref.py, with the existing suite's metrics and bound — K_BOUND times the
distance of ``hidden(E', emulate=True)`` from ``hidden(E')``, computed from the reference alone.
Each case asserts from the plan that int8 ran, and on which cross-attention form.

Models: decoder_ref.config — two decoder layers, 64 vocabulary entries, 141 encoder keys (two
64-key chunks plus 13) unless stated; T = 3 positions unless stated.

  1. hidden-state parity   384 / 6 rows 1, 17, and 2 rows at one key split; 512 / 8 rows 1, 17, 64,
                           65 at one key split (at one split the kernel writes the context rows
                           itself, DIRECT) and at 3; 512 / 8 over
                           1500 keys, 3 rows at 8 splits; 768 / 12, 1024 / 16 and 1280 / 20 (two
                           head groups) rows 1, 17
  2. shared rows           13 rows over 3 encoder rows (5 + 5 + 3): PAIR blocks in place at 384
                           and 512, gathered q and s at 768 and 1280
  3. edge rows in E        a zero key row, a row whose amax is negative, 16.0 planted in one
                           seeded column of every other key row
  4. the control           on the outlier input hidden(E) and hidden(E') lie more than 4 bounds
                           apart (asserted on the CPU first): the int8 call meets the bound
                           against hidden(E') and breaks it against hidden(E), the float16 call
                           the opposite. On the CPU (512 / 8, 4 rows, 3 positions, seeds 3 / 5):
                           hidden(E) against hidden(E') 1.44e-2 row / 1.87e-2 tile, the emulation
                           6.5e-4 / 9.0e-4 from hidden(E'): 7.4 / 6.9 bounds. Plain unit-normal E
                           gives only 2.3e-3 / 3.3e-3, too close to the bound to tell them apart.
  5. decode                tiny.en, 4 windows, max_length 20: greedy with int8 against
                           oracle.whisper.greedy_cached on E' (identical, or first divergence at
                           a top-2 margin below NEAR_TIE; the windows chosen on the CPU with every
                           margin >= 2 NEAR_TIE, so at least 3 of 4 identical); beam_size 1 with
                           int8 equals the greedy call bit for bit
  6. staggered             6 rows 4 positions, then 3 continue beside 3 fresh rows for 2
  7. switching back        set_cross_compute("float16") is bit-identical to never having left it
"""
import functools

import numpy as np
import pytest
import torch

import cross_int8_ref as cr
import decoder_ref as ref
from janus_amd import whisper as jw
from janus_amd._native import JanusNativeError

pytestmark = pytest.mark.gpu

T = 3
SEED_W, SEED_IN = 3, 5
NEAR_TIE = 2e-3   # tests/test_whisper_gpu.py's: fp16-operand decoding may only flip a choice this close
OWN, IN_PLACE, GATHERED = 0, 1, 2
ENC_INDEX = [0] * 5 + [1] * 5 + [2] * 3


class Model:
    """One engine shape: weights, inputs (``outliers``: cross_int8_ref.outlier_inputs), E' and the
    float64 references on E and E', computed once over every row and sliced by the cases (the
    decoder's rows are independent)."""

    def __init__(self, d, H, Te, rows, outliers=False):
        self.cfg = ref.config(d, H, Te)
        self.W = ref.weights(self.cfg, SEED_W)
        make = cr.outlier_inputs if outliers else ref.inputs
        self.tokens, self.enc = make(self.cfg, rows, T, SEED_IN)
        self.encq = cr.dequantised(self.enc)
        self._eng = {}

    @functools.lru_cache(maxsize=None)
    def hidden(self, quantised, emulate, enc_index=None):
        e = self.encq if quantised else self.enc
        if enc_index is not None:
            return ref.hidden(self.tokens[:len(enc_index)], e[:max(enc_index) + 1], self.W, self.cfg,
                              enc_index=list(enc_index), emulate=emulate)
        return ref.hidden(self.tokens, e, self.W, self.cfg, emulate=emulate)

    def engine(self, cross):
        if cross not in self._eng:
            self._eng[cross] = jw.WhisperEngine(self.cfg, self.W, cross_compute=cross)
            self._enc_dev = torch.from_numpy(self.enc).cuda()
        return self._eng[cross]

    def enc_dev(self, n):
        return self._enc_dev[:n].contiguous()


SHAPES = {
    (384, 6, 141): 17, (512, 8, 141): 65, (512, 8, 1500): 3, (768, 12, 141): 17, (1024, 16, 141): 17,
    (1280, 20, 141): 17,
}


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(d, H, Te=141, outliers=False):
        key = (d, H, Te, outliers)
        if key not in made:
            made[key] = Model(d, H, Te, 4 if outliers else SHAPES[(d, H, Te)], outliers)
        return made[key]

    yield get
    made.clear()


def check_plan(plan, want):
    got = {k: plan.get(k) for k in want}
    assert got == want, f"the plan that ran differs from the case's path: {got} != {want}"


def distances(got, want, emu):
    """(row, tile) of got against want, and the bound: K_BOUND x (emu against want)."""
    g, e = ref.metrics(got, want), ref.metrics(emu, want)
    return g, (ref.K_BOUND * e[0], ref.K_BOUND * e[1])


def hold(name, what, got, want, emu):
    (g_row, g_tile), (b_row, b_tile) = distances(got, want, emu)
    print(f"{name} {what}: row {g_row:.2e} tile {g_tile:.2e} | bound row {b_row:.2e} tile {b_tile:.2e}")
    at, col, val = ref.worst(got, want)
    where = f"{what} index {at}, columns {col}-{col + 15}"
    assert np.isfinite(g_tile) and g_tile <= b_tile, f"{name}: {where}: tile {val:.2e} over the bound {b_tile:.2e}"
    assert g_row <= b_row, f"{name}: {where}: row {g_row:.2e} over the bound {b_row:.2e}"


def outputs(out):
    return (out.x.transpose(0, 1).double().cpu().numpy(), out.kc[:, :, :T].double().cpu().numpy(),
            out.vc[:, :, :T].double().cpu().numpy())


def sliced(r, B):
    return r[0][:B], r[1][:, :B], r[2][:, :B]


def run_int8(M, name, B, plan_want, **opts):
    eng = M.engine("int8")
    out = eng.decode_hidden(M.enc_dev(B), M.tokens[:B], **opts)
    check_plan(out.plan, dict(B=B, cross_int8=1, persist=0, seg_grid=0, xabs=1, ngroups=0, **plan_want))
    assert eng.decode_path().cross == "int8" and eng.decode_path().persistent == 0
    want, emu = sliced(M.hidden(True, False), B), sliced(M.hidden(True, True), B)
    for what, g, r, e in zip(("x", "k cache", "v cache"), outputs(out), want, emu):
        hold(name, what, g, r, e)


# ------------------------------------------------------------ 1. hidden-state parity
SPLIT = {"call.enc_rows": OWN, "npairs": 0}
CASES = [(f"384-rows{B}", (384, 6), B, dict(SPLIT, xsplit=3, cvp=1), {}) for B in (1, 17)]
# (the one-split form at 384 / 6 has no other test)
CASES.append(("384-rows2-direct", (384, 6), 2, dict(SPLIT, xsplit=1, cvp=0),
              dict(xattn_splits=1, path_flags=jw.DEC_PATH_NO_CVP)))
for _B in (1, 17, 64, 65):
    # one key split and no fused merge: the kernel writes the context rows itself (DIRECT)
    CASES.append((f"512-rows{_B}-direct", (512, 8), _B, dict(SPLIT, xsplit=1, cvp=0),
                  dict(xattn_splits=1, path_flags=jw.DEC_PATH_NO_CVP)))
    CASES.append((f"512-rows{_B}-splits3", (512, 8), _B, dict(SPLIT, xsplit=3, cvp=int(_B <= 64)), dict(xattn_splits=3)))
CASES.append(("512-keys1500-splits8", (512, 8, 1500), 3, dict(SPLIT, xsplit=8, cvp=1), dict(xattn_splits=8)))
for _d, _H in ((768, 12), (1024, 16), (1280, 20)):
    CASES += [(f"{_d}-rows{B}", (_d, _H), B, dict(SPLIT, xsplit=3, cvp=0, wide=1), {}) for B in (1, 17)]


@pytest.mark.parametrize("name,shape,B,plan,opts", CASES, ids=[c[0] for c in CASES])
def test_hidden_parity(models, name, shape, B, plan, opts):
    run_int8(models(*shape), name, B, plan, **opts)


# ------------------------------------------------------------ 2. shared encoder rows
PAIRS = [0, 1, 0, 2, 3, 0, 4, -1, 0, 5, 6, 1, 7, 8, 1, 9, -1, 1, 10, 11, 2, 12, -1, 2]
SHARED = [
    ("384-pair", (384, 6), dict(npairs=8, pairs=PAIRS, cvp=1, **{"call.enc_rows": IN_PLACE, "call.n_enc": 3}), "in_place"),
    ("512-pair", (512, 8), dict(npairs=8, pairs=PAIRS, cvp=1, **{"call.enc_rows": IN_PLACE, "call.n_enc": 3}), "in_place"),
    ("768-gathered", (768, 12), dict(npairs=0, wide=1, **{"call.enc_rows": GATHERED, "call.n_enc": 13}), "gathered"),
    ("1280-gathered", (1280, 20), dict(npairs=0, wide=1, **{"call.enc_rows": GATHERED, "call.n_enc": 13}), "gathered"),
]


@pytest.mark.parametrize("name,shape,plan,rows", SHARED, ids=[c[0] for c in SHARED])
def test_shared_rows(models, name, shape, plan, rows):
    """13 rows over 3 encoder rows (5 + 5 + 3): row b against hidden() on E'[enc_index[b]]."""
    M = models(*shape)
    B = len(ENC_INDEX)
    eng = M.engine("int8")
    out = eng.decode_hidden(M.enc_dev(3), M.tokens[:B], enc_index=ENC_INDEX)
    check_plan(out.plan, dict(B=B, cross_int8=1, persist=0, xabs=1, ngroups=0, **plan))
    assert eng.decode_path() == jw.DecodePath(rows, 0, "int8")
    want, emu = M.hidden(True, False, tuple(ENC_INDEX)), M.hidden(True, True, tuple(ENC_INDEX))
    for what, g, r, e in zip(("x", "k cache", "v cache"), outputs(out), want, emu):
        hold(name, what, g, r, e)


# ------------------------------------------------------------ 3. edge rows, 4. the control
@pytest.mark.parametrize("shape", [(512, 8), (768, 12)], ids=["512", "768"])
def test_edge_rows(models, shape):
    """A zero key row (q = 0, s = 1), a row whose amax is negative (-127 exactly, +127 absent) and
    16.0 in one column of every other key row, through the split form at both chunk sizes."""
    M = models(*shape, outliers=True)
    q, s = cr.quantise(M.enc)
    assert not q[:, 3].any() and (s[:, 3] == 1).all() and (q[:, 5, 7] == -127).all() and q[:, 5].max() < 127
    run_int8(M, f"edge-{shape[0]}", 4, dict(xsplit=3, npairs=0))


def test_control_outliers_tell_the_operands_apart(models):
    M = models(512, 8, outliers=True)
    B = 4
    x_e, x_q = M.hidden(False, False)[0], M.hidden(True, False)[0]
    emu_e, emu_q = M.hidden(False, True)[0], M.hidden(True, True)[0]
    # from the reference alone, before any GPU work: the two operands lie >= 4 bounds apart
    apart = ref.metrics(x_e, x_q)
    bound_q = tuple(ref.K_BOUND * v for v in ref.metrics(emu_q, x_q))
    bound_e = tuple(ref.K_BOUND * v for v in ref.metrics(emu_e, x_e))
    print(f"hidden(E) against hidden(E'): row {apart[0]:.2e} tile {apart[1]:.2e} | bound on E' row "
          f"{bound_q[0]:.2e} tile {bound_q[1]:.2e}, on E row {bound_e[0]:.2e} tile {bound_e[1]:.2e}")
    assert apart[0] >= 4 * bound_q[0] and apart[1] >= 4 * bound_q[1]
    assert ref.metrics(x_q, x_e)[0] >= 4 * bound_e[0] and ref.metrics(x_q, x_e)[1] >= 4 * bound_e[1]

    def run(cross):
        eng = M.engine(cross)
        out = eng.decode_hidden(M.enc_dev(B), M.tokens[:B])
        assert out.plan.get("cross_int8", 0) == int(cross == "int8") and eng.decode_path().cross == cross
        return out.x.transpose(0, 1).double().cpu().numpy()

    for cross, own, own_b, other, other_b in (("int8", x_q, bound_q, x_e, bound_e),
                                              ("float16", x_e, bound_e, x_q, bound_q)):
        x = run(cross)
        g, o = ref.metrics(x, own), ref.metrics(x, other)
        print(f"{cross}: own reference row {g[0]:.2e} tile {g[1]:.2e} | the other's row {o[0]:.2e} tile {o[1]:.2e}")
        assert g[0] <= own_b[0] and g[1] <= own_b[1], (cross, g, own_b)
        assert o[0] > other_b[0] and o[1] > other_b[1], (cross, o, other_b)


# ------------------------------------------------------------ 5. decode
@pytest.fixture(scope="module")
def tiny():
    """tiny.en on synthetic weights; 4 of 12 seeded windows whose oracle decode on E' has every
    top-2 margin >= 2 NEAR_TIE (chosen on the CPU, from the reference alone)."""
    from oracle import whisper as ow
    cfg = jw.CONFIGS["tiny.en"]
    W = jw.synthetic_weights(cfg, seed=5)
    eng = jw.WhisperEngine(cfg, W, cross_compute="int8")
    g = torch.Generator().manual_seed(11)
    enc = torch.randn(12, cfg.n_audio_ctx, cfg.d_model, generator=g).half().numpy()
    rows = ow.greedy_cached(cr.dequantised(enc).astype(np.float32), W, cfg, eng.tokenizer, 20, no_speech=50361)
    clear = [b for b, r in enumerate(rows) if min(r["margins"]) >= 2 * NEAR_TIE][:4]
    assert len(clear) == 4, [min(r["margins"]) for r in rows]
    return eng, torch.from_numpy(enc[clear]).cuda(), [rows[b] for b in clear]


def test_greedy_decode_against_the_oracle_on_the_dequantised_rows(tiny):
    eng, enc, rows = tiny
    out = eng.decode_ex(enc, max_length=20)
    assert eng.decode_path() == jw.DecodePath("own", 0, "int8")
    tokens, ntok = out.tokens.cpu().numpy(), out.n_tokens.cpu().numpy()
    plen = int(out.prompt_lens[0])
    same = 0
    for b, r in enumerate(rows):
        got = [int(t) for t in tokens[b][plen:plen + int(ntok[b])]]
        if got == r["tokens"]:
            same += 1
            continue
        n = min(len(got), len(r["tokens"]))
        first = next((i for i in range(n) if got[i] != r["tokens"][i]), n)
        margin = r["margins"][first] if first < len(r["margins"]) else 0.0
        assert margin < NEAR_TIE, (b, first, margin, got[first:first + 3], r["tokens"][first:first + 3])
    assert same >= 3, same


def test_beam_size_one_is_the_greedy_call(tiny):
    eng, enc, _ = tiny
    a = eng.decode_ex(enc, max_length=20)
    b = eng.decode_beam(enc, beam_size=1, max_length=20)
    assert eng.decode_path().cross == "int8"
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.n_tokens, b.n_tokens)
    assert torch.equal(a.sum_logprob, b.sum_logprob) and torch.equal(a.no_speech_prob, b.no_speech_prob)


def test_persistent_request_runs_the_launch_path_and_refusals(tiny, models):
    eng, enc, _ = tiny
    a = eng.decode_ex(enc, max_length=20)
    b = eng.decode_ex(enc, max_length=20, persistent=2)
    assert eng.decode_path() == jw.DecodePath("own", 0, "int8") and torch.equal(a.tokens, b.tokens)
    M = models(512, 8)
    e8 = M.engine("int8")
    out = e8.decode_hidden(M.enc_dev(4), M.tokens[:4], persistent=2)
    check_plan(out.plan, dict(persist=0, seg_grid=0, cross_int8=1))
    for flags, kw, match in ((jw.DEC_PATH_NO_XABSORB, {}, "JANUS_DEC_PATH_NO_XABSORB with cross_compute int8"),
                             (jw.DEC_PATH_XGROUP, dict(enc_index=[0, 0, 0, 1]), "JANUS_DEC_PATH_XGROUP with cross_compute int8")):
        with pytest.raises(JanusNativeError, match=match):
            e8.decode_hidden(M.enc_dev(2 if kw else 4), M.tokens[:4], path_flags=flags, **kw)
    M7 = models(768, 12)
    with pytest.raises(JanusNativeError, match="JANUS_DEC_PATH_XROWS with cross_compute int8"):
        M7.engine("int8").decode_hidden(M7.enc_dev(2), M7.tokens[:4], enc_index=[0, 0, 0, 1],
                                        path_flags=jw.dec_path_xrows(2))


# ------------------------------------------------------------ 6. staggered
def test_staggered_continuation_is_the_one_go_run(models):
    """6 rows run 4 positions; then rows 0 .. 2 continue at 4 beside rows 3 .. 5 starting again,
    2 positions, handed their encoder rows (quantised) again: bit-identical to the same rows run
    in one go, the continuing rows' positions 4, 5 and the fresh rows' 0, 1."""
    M = models(512, 8)
    B, first, more = 6, 4, 2
    g = torch.Generator().manual_seed(SEED_IN + 1)
    tokens = torch.randint(0, M.cfg.n_vocab, (B, first + more), generator=g).numpy().astype(np.int32)
    eng, enc = M.engine("int8"), M.enc_dev(B)
    whole = eng.decode_hidden(enc, tokens, pos_offset=[0] * B, steps=first + more)
    check_plan(whole.plan, dict(cross_int8=1, stagger=1, persist=0))
    one = eng.decode_hidden(enc, tokens, pos_offset=[0] * B, steps=first)
    assert eng.decode_stand(B) == [first] * B
    assert torch.equal(one.x, whole.x[:first])
    two = eng.decode_hidden(enc, tokens, pos_offset=[first] * 3 + [0] * 3, steps=more)
    check_plan(two.plan, dict(cross_int8=1, stagger=1, max_roff=first))
    assert eng.decode_stand(B) == [first + more] * 3 + [more] * 3
    assert torch.equal(two.x[:, :3], whole.x[first:, :3])
    assert torch.equal(two.x[:, 3:], whole.x[:more, 3:])
    assert torch.equal(two.kc[:, :3, :first + more], whole.kc[:, :3, :first + more])
    assert torch.equal(two.vc[:, 3:, :more], whole.vc[:, 3:, :more])


# ------------------------------------------------------------ 7. switching back
def test_switching_back_is_bit_identical(models):
    M = models(512, 8)
    B = 17
    never = M.engine("float16")
    a = never.decode_hidden(M.enc_dev(B), M.tokens[:B])
    assert "cross_int8" not in a.plan and never.cross_compute == "float16" and never.decode_path().cross == "float16"
    eng = jw.WhisperEngine(M.cfg, M.W, cross_compute="int8")
    assert eng.cross_compute == "int8"
    q = eng.decode_hidden(M.enc_dev(B), M.tokens[:B])
    assert q.plan["cross_int8"] == 1 and not torch.equal(q.x, a.x)
    eng.set_cross_compute("float16")
    assert eng.cross_compute == "float16"
    b = eng.decode_hidden(M.enc_dev(B), M.tokens[:B])
    assert "cross_int8" not in b.plan and eng.decode_path().cross == "float16"
    assert torch.equal(a.x, b.x) and torch.equal(a.kc[:, :, :T], b.kc[:, :, :T]) and torch.equal(a.vc[:, :, :T], b.vc[:, :, :T])
    eng.set_cross_compute("int8")
    assert torch.equal(eng.decode_hidden(M.enc_dev(B), M.tokens[:B]).x, q.x)
