"""The int8 decoder weights on the CPU: the mode names, the planner's view of the context
setting (janus_whisper_set_decoder_compute through janus_decode_plan_describe_modes), its
refusals, the Python argument checks, and the reference (tests/decoder_int8_ref.py): its rule on
hand-computed rows and its sensitivity — every seeded defect lies at least 3x over the bound
the GPU tests (tests/test_decoder_int8_gpu.py) hold the engine's hidden state to."""
import numpy as np
import pytest

import decoder_int8_ref as d8
import decoder_ref as ref
import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import whisper as jw
from janus_amd.services import batched as ba
from janus_amd.services import transcriber as tr

BASE, TINY, SMALL, MEDIUM, TURBO = (jw.CONFIGS[n] for n in ("base.en", "tiny.en", "small.en", "medium.en",
                                                           "large-v3-turbo"))
F32 = np.float32


# ------------------------------------------------------------------ names
def test_mode_names():
    assert jw.decoder_compute_mode("float16") == 0 and jw.decoder_compute_mode("int8") == 1
    assert jw.DECODER_COMPUTE_NAMES == ("float16", "int8")
    assert (jw.DEC_W_QKV, jw.DEC_W_O, jw.DEC_W_XQK, jw.DEC_W_XV, jw.DEC_W_XO, jw.DEC_W_FC1, jw.DEC_W_FC2) == \
        tuple(range(7)) == (d8.QKV, d8.O, d8.XQK, d8.XV, d8.XO, d8.FC1, d8.FC2)
    # compute_type keeps its mapping: decoder_compute is its own argument
    assert tr.resolve_compute_type("int8", True) == ("int8_float16", "int8")
    assert tr.resolve_compute_type("int8", False) == ("float16", "float16")
    assert jw.DecodePath("own", 0) == jw.DecodePath("own", 0, "float16")     # DecodePath keeps its fields


@pytest.mark.parametrize("bad", ["int4", "INT8", "", None, 1, "float32", "int8_float16"])
def test_unknown_names_are_value_errors(bad):
    with pytest.raises(ValueError, match="decoder_compute must be one of"):
        jw.decoder_compute_mode(bad)
    with pytest.raises(ValueError, match="decoder_compute must be one of"):
        jw.WhisperEngine(TINY, decoder_compute=bad)          # before any device work
    with pytest.raises(ValueError, match="decoder_compute must be one of"):
        tr.WhisperModel("tiny.en", decoder_compute=bad)
    with pytest.raises(ValueError, match="decoder_compute must be one of"):
        jw.WhisperEngine.set_decoder_compute(object.__new__(jw.WhisperEngine), bad)


def test_whisper_model_passes_it_through(monkeypatch):
    seen = []

    class Engine:
        def __init__(self, cfg, **kw):
            seen.append((cfg.name, kw))

    monkeypatch.setattr(tr, "WhisperEngine", Engine)
    m = tr.WhisperModel("base.en", decoder_compute="int8")
    assert m.decoder_compute == "int8" and ba.BatchedInferencePipeline(m).model.decoder_compute == "int8"
    tr.WhisperModel("base.en", compute_type="int8", apply_compute_type=True, decoder_compute="int8",
                    cross_compute="int8")
    assert tr.WhisperModel("base.en", compute_type="int8").decoder_compute == "float16"
    assert seen == [("base.en", dict(encoder_compute="float16", decoder_compute="int8")),
                    ("base.en", dict(encoder_compute="int8", cross_compute="int8", decoder_compute="int8")),
                    ("base.en", dict(encoder_compute="float16"))]      # compute_type alone selects nothing here


def test_beam_with_int8_weights_is_refused_before_the_engine(monkeypatch):
    """beam_size 2 with int8 decoder weights: NotImplementedError from the argument checks; the
    engine here is an object that fails on any attribute the decode would touch."""
    class Engine:
        decoder_compute = "int8"

        def __init__(self, cfg=None, **kw):
            pass

        def __getattr__(self, name):
            raise AssertionError(f"the engine was touched: {name}")

    monkeypatch.setattr(tr, "WhisperEngine", Engine)
    m = tr.WhisperModel("tiny.en", decoder_compute="int8")
    audio = np.zeros(16000, np.float32)
    with pytest.raises(NotImplementedError, match="decoder_compute='int8'"):
        m.transcribe(audio, beam_size=2)
    with pytest.raises(NotImplementedError, match="decoder_compute='int8'"):
        ba.BatchedInferencePipeline(m).transcribe(audio, beam_size=2)
    with pytest.raises(NotImplementedError, match="decoder_compute='int8'"):
        tr.generate_segments(Engine(), [audio], beam_size=2)
    with pytest.raises(NotImplementedError, match="decoder_compute='int8'"):
        jw.check_decoder_compute_beam("int8", 5)
    jw.check_decoder_compute_beam("int8", 1)
    jw.check_decoder_compute_beam("float16", 5)


# ------------------------------------------------------------------ the planner
@pytest.mark.parametrize("name", sorted(mr.PLAN_CASES))
def test_float16_plans_are_the_committed_ones(native_lib, name):
    """decoder compute float16: the text and the key of janus_decode_plan_describe for the same
    call, byte for byte."""
    model, B, kw = mr.PLAN_CASES[name]
    kw = {k: v for k, v in kw.items() if k in ("persistent", "max_length", "cus", "temperature", "beam_size",
                                              "enc_index", "prompts")}
    cfg = jw.CONFIGS[model]
    want = d8.describe(native_lib, cfg, B, entry="janus_decode_plan_describe", **kw)
    assert d8.describe(native_lib, cfg, B, 0, 0, **kw) == want
    assert d8.describe(native_lib, cfg, B, entry="janus_decode_plan_describe_cross", **kw) == want
    assert "dec_int8" not in want[0]


@pytest.mark.parametrize("cfg", [TINY, BASE], ids=lambda c: c.name)
@pytest.mark.parametrize("B", [8, 64, 128])
def test_fusions_are_off_at_384_and_512(native_lib, cfg, B):
    ask = jw.DEC_PATH_FUSED_LN | jw.DEC_PATH_RESID_LN | jw.DEC_PATH_CVP
    for flags in (0, ask, jw.DEC_PATH_LN_FUSE, jw.dec_path_ln_mask(15)):
        f = mr.plan_fields(d8.describe(native_lib, cfg, B, 1, flags=flags)[0])
        assert f["dec_int8"] == "1"
        assert {k: f[k] for k in ("fused_ln", "ln_fuse", "ln_pro_mask", "embed_ln", "rln", "cvp", "persist",
                                  "seg_grid")} == dict.fromkeys(
            ("fused_ln", "ln_fuse", "ln_pro_mask", "embed_ln", "rln", "cvp", "persist", "seg_grid"), "0")
        assert f["fuse_se"] == "1" and f["xabs"] == "1"
    off = mr.plan_fields(d8.describe(native_lib, cfg, B, 0)[0])
    assert off["embed_ln"] == "1" and (B > 64 or (off["ln_pro_mask"] == "9" and off["cvp"] == "1"))


@pytest.mark.parametrize("cfg", [SMALL, MEDIUM, TURBO], ids=lambda c: c.name)
def test_wide_models_keep_their_plan(native_lib, cfg):
    """Above d_model 512 the float16 plan is already the unfused one: int8 adds its line and its
    key word and turns off only the fused merge + value projection (where the model has one)."""
    off_text, off_key = d8.describe(native_lib, cfg, 64, 0)
    text, key = d8.describe(native_lib, cfg, 64, 1)
    lines = text.splitlines()
    assert lines.index("dec_int8=1") + 1 == [i for i, ln in enumerate(lines) if ln.startswith("pairs=")][0]
    rest = [ln for ln in lines if ln != "dec_int8=1"]
    assert [ln for ln in rest if not ln.startswith("cvp=")] == [ln for ln in off_text.splitlines()
                                                                if not ln.startswith("cvp=")]
    assert "cvp=0" in rest
    assert key[-1] == 0x776938 << 32 and len(key) == len(off_key) + 1
    both = d8.describe(native_lib, cfg, 64, 1, 1)
    assert both[0].splitlines().index("cross_int8=1") + 1 == both[0].splitlines().index("dec_int8=1")
    assert both[1][-2:] == (0x786938 << 32, 0x776938 << 32)


def test_persistent_request_plans_the_launch_path(native_lib):
    for level in (1, 2, 3):
        f = mr.plan_fields(d8.describe(native_lib, BASE, 8, 0, persistent=level)[0])
        assert f["persist"] == str(level)
        f = mr.plan_fields(d8.describe(native_lib, BASE, 8, 1, persistent=level)[0])
        assert f["persist"] == "0" and f["seg_grid"] == "0" and f["xrev"] == "0" and f["dec_int8"] == "1"


def test_shared_and_sampled_plans_take_it(native_lib):
    f = mr.plan_fields(d8.describe(native_lib, TINY, 10, 1, enc_index=[0] * 5 + [1] * 5)[0])
    assert f["dec_int8"] == "1" and f["npairs"] == "6" and f["call.enc_rows"] == "1" and f["cvp"] == "0"
    f = mr.plan_fields(d8.describe(native_lib, TURBO, 10, 1, enc_index=[0] * 5 + [1] * 5)[0])
    assert f["dec_int8"] == "1" and f["call.enc_rows"] == "2"
    assert "dec_int8=1" in d8.describe(native_lib, BASE, 320, 1, temperature=0.6)[0]


def test_refusals_arrive_by_name(native_lib):
    beam = dict(beam_size=4, prompts=[[50257, 50362]] * 8, enc_index=[0] * 4 + [1] * 4)
    d8.describe(native_lib, BASE, 8, 0, **beam)     # float16: plans
    with pytest.raises(nat.JanusNativeError, match="beam search with decoder_compute int8"):
        d8.describe(native_lib, BASE, 8, 1, **beam)
    d8.describe(native_lib, BASE, 8, 0, flags=jw.DEC_PATH_NO_XABSORB)
    with pytest.raises(nat.JanusNativeError, match="JANUS_DEC_PATH_NO_XABSORB with decoder_compute int8"):
        d8.describe(native_lib, BASE, 8, 1, flags=jw.DEC_PATH_NO_XABSORB)
    with pytest.raises(nat.JanusNativeError, match="JANUS_DEC_PATH_XGROUP with decoder_compute int8"):
        d8.describe(native_lib, BASE, 10, 1, flags=jw.DEC_PATH_XGROUP, enc_index=[0] * 5 + [1] * 5)
    with pytest.raises(nat.JanusNativeError, match="decoder_compute int8 needs the absorbed cross-attention"):
        d8.describe(native_lib, BASE, 513, 1)
    with pytest.raises(nat.JanusNativeError, match="decoder_compute must be"):
        d8.describe(native_lib, BASE, 8, 2)


# ------------------------------------------------------------------ the reference's rule
def test_quantiser_on_hand_computed_rows():
    w = np.zeros((4, 16), np.float16)
    w[1, :4] = [1.0, -3.0, 0.75, 2.9]                        # amax on a negative element
    w[2, :7] = [127.0, -127.0, 0.5, 1.5, 2.5, -0.5, -1.5]    # inv = 1: ties to even
    w[3, :3] = [2.0, 1.0, -0.01]
    q, s = d8.quantise(w)
    assert q.dtype == np.int8 and s.dtype == np.float32
    assert not q[0].any() and s[0] == 1.0                    # a zero row
    assert q[1, :4].tolist() == [42, -127, 32, 123] and s[1] == F32(3) / F32(127)
    assert q[2, :7].tolist() == [127, -127, 0, 2, 2, 0, -2] and s[2] == 1.0
    assert q[3, :3].tolist() == [127, 64, -1] and s[3] == F32(2) / F32(127)
    (m,), = d8.dequantised([[(q, s)]])
    assert m.dtype == np.float64 and m[1, 1] == -127 * float(s[1]) and not m[0].any()


# ------------------------------------------------------------------ the reference's sensitivity
ROWS, T, TE = 6, 5, 40
SHAPES = [(384, 6), (512, 8), (1280, 20)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"d{s[0]}")
def case(request):
    d, H = request.param
    cfg = ref.config(d, H, TE)
    W = ref.weights(cfg, seed=3)
    tokens, enc = ref.inputs(cfg, ROWS, T, seed=5)
    W16, _ = d8.fp16_matrices(W, cfg)
    Q, table = d8.quantised(W, cfg)
    M = d8.dequantised(Q)
    x = d8.hidden(tokens, enc, M, W, cfg)
    xe = d8.hidden(tokens, enc, M, W, cfg, emulate=True)
    row, tile = ref.metrics(xe, x)
    print(f"d {d} int8 emulation: row {row:.2e} tile {tile:.2e}")
    return dict(cfg=cfg, W=W, tokens=tokens, enc=enc, W16=W16, Q=Q, table=table, x=x, bound=ref.K_BOUND * tile)


def test_reference_on_fp16_weights_is_decoder_ref(case):
    """The reference run on the UNquantised fp16 matrices is tests/decoder_ref.py's emulation-free
    hidden() up to the fp16 rounding of the absorbed query weight: it is the same decoder."""
    c = case
    M = [[m.astype(np.float64) for m in layer] for layer in c["W16"]]
    for layer in range(c["cfg"].dec_layers):          # the float64 absorbed weight: decoder_ref's own product
        M[layer][d8.XQK] = d8.wqk_f64(c["W"], c["cfg"], layer)
    x = d8.hidden(c["tokens"], c["enc"], M, c["W"], c["cfg"])
    want, _, _ = ref.hidden(c["tokens"], c["enc"], c["W"], c["cfg"])
    assert ref.metrics(x, want)[1] <= 1e-9


def test_quantisation_moves_the_hidden_state_past_the_bound(case):
    """The int8 and the fp16 weights are told apart by the GPU test's bound: a kernel that
    multiplied the fp16 weights in every layer would fail it."""
    c = case
    M = [[m.astype(np.float64) for m in layer] for layer in c["W16"]]
    x16 = d8.hidden(c["tokens"], c["enc"], M, c["W"], c["cfg"])
    assert ref.metrics(x16, c["x"])[1] >= 3 * c["bound"]


@pytest.mark.parametrize("defect", sorted(d8.DEFECTS))
def test_defect_exceeds_bound(case, defect):
    """Each seeded defect (layer 1, the tile at columns 208 .. 223 where it has one) is at least
    3x over the bound on the tile metric."""
    c = case
    if defect == "w2_first_3072" and 4 * c["cfg"].d_model <= 3072:
        # fc2 has no column past 3072 at this width: the defect is the identity (d 1280 carries it)
        assert c["W16"][1][d8.FC2][:, :3072].shape == c["W16"][1][d8.FC2].shape
        return
    M = d8.with_defect(c["Q"], c["W16"], defect, layer=1, col0=208)
    x = d8.hidden(c["tokens"], c["enc"], M, c["W"], c["cfg"])
    _, tile = ref.metrics(x, c["x"])
    at = ref.worst(x, c["x"])
    print(f"d {c['cfg'].d_model} {defect}: tile {tile:.2e} = {tile / c['bound']:.1f}x the bound {c['bound']:.2e}, "
          f"worst at {at}")
    assert tile >= 3 * c["bound"], (defect, tile, c["bound"])
    if defect == "tile_scales_dropped":
        assert at[1] == 208


def test_logits_use_the_table(case):
    c = case
    got = d8.logits(c["x"], c["W"], c["cfg"], c["table"])
    q, s = c["table"]
    assert got.shape == (ROWS, T, c["cfg"].n_vocab)
    plain = ref.logits(c["x"], c["W"], c["cfg"])
    assert 0 < np.abs(got - plain).max() < 0.05 * np.abs(plain).max()


def test_absorbed_weight_check_on_the_cpu(case):
    """The reference alone: the absorbed query weight derived in float32 (what the engine's
    prepare does) against the float64 derivation, through wqk_check. Only elements within one
    fp16 ulp of a quantiser boundary differ, by 1; they are under 10 % of all elements."""
    import torch
    c, cfg = case, case["cfg"]
    d, H = cfg.d_model, cfg.n_heads
    W = c["W"]
    p = "decoder.layers.1.encoder_attn"
    wq = torch.from_numpy(W[p + ".q_proj.weight"]).view(H, d // H, d)
    wk = torch.from_numpy(W[p + ".k_proj.weight"]).view(H, d // H, d)
    sc = np.float32(np.log2(np.e) / 8.0)
    w32 = (torch.einsum("hci,hcj->hji", wq, wk) * sc).reshape(H * d, d).numpy()
    q, s = d8.quantise(w32.astype(np.float16))
    r = d8.wqk_check(q, s, W, cfg, 1)
    print(f"d {d} wqk: {r}")
    assert r["share"] < 0.10 and r["bad"] == 0
    assert r["s_rows"] <= 0.01 * H * d and r["s_rel"] <= 2.0 ** -10
    # the exact derivation passes trivially, and a shifted scale does not
    q0, s0 = c["Q"][1][d8.XQK]
    r0 = d8.wqk_check(q0, s0, W, cfg, 1)
    assert r0["bad"] == 0 and r0["differ"] == 0 and r0["s_rows"] == 0
    assert d8.wqk_check(np.roll(q0, 1, axis=1), s0, W, cfg, 1)["bad"] > 0
