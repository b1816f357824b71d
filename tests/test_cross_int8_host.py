"""The int8 cross-attention operand on the CPU: the planner's view of the context setting
(janus_whisper_set_cross_compute through janus_decode_plan_describe_cross), its three refusals,
the Python argument checks, and the reference's E' (tests/cross_int8_ref.py) on hand-computed
rows."""
import numpy as np
import pytest

import cross_int8_ref as cr
import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import whisper as jw
from janus_amd.services import transcriber as tr

BASE, TINY, SMALL, MEDIUM, TURBO = (jw.CONFIGS[n] for n in ("base.en", "tiny.en", "small.en", "medium.en",
                                                           "large-v3-turbo"))
F32 = np.float32


# ------------------------------------------------------------------ the planner
@pytest.mark.parametrize("name", sorted(mr.PLAN_CASES))
def test_default_plans_are_the_committed_ones(native_lib, name):
    """cross compute float16: the text and the key of janus_decode_plan_describe, i.e. the
    committed golden plan (the no_speech_back line aside, as test_multilingual_host reads it)."""
    model, B, kw = mr.PLAN_CASES[name]
    want_text, want_key = mr.describe_plan(native_lib, name)
    text, key = cr.describe(native_lib, jw.CONFIGS[model], B, 0, **kw)
    assert text == want_text and key == want_key
    assert [ln for ln in text.splitlines() if ln != "no_speech_back=0"] == mr.golden_plans()[name]["text"].splitlines()
    assert "cross_int8" not in text


@pytest.mark.parametrize("cfg", [TINY, BASE, SMALL, MEDIUM, TURBO], ids=lambda c: c.name)
def test_plan_shows_int8_only_when_set(native_lib, cfg):
    off_text, off_key = cr.describe(native_lib, cfg, 64, 0)
    text, key = cr.describe(native_lib, cfg, 64, 1)
    lines = text.splitlines()
    assert "cross_int8=1" in lines
    # in front of pairs=, and nothing else moved
    assert lines.index("cross_int8=1") + 1 == [i for i, ln in enumerate(lines) if ln.startswith("pairs=")][0]
    assert [ln for ln in lines if ln != "cross_int8=1"] == off_text.splitlines()
    assert key != off_key and len(key) == len(off_key) + 1 and key[:len(off_key)] == off_key


def test_key_differs_from_every_float16_plan(native_lib):
    """One tagged word after the float16 plan's key, above any 32-bit field: no float16 plan,
    whose optional words are the history rules' two 32-bit ones, can end in it."""
    seen = set()
    for kw in ({}, dict(temperature=0.6), dict(persistent=2), dict(enc_index=[0] * 4 + [1] * 4)):
        off, on = (cr.describe(native_lib, BASE, 8, c, **kw)[1] for c in (0, 1))
        assert on[-1] == 0x786938 << 32 and on[:-1] == (off if "persistent" not in kw else on[:-1])
        assert all(abs(w) < 1 << 32 for w in off)
        seen |= {off, on}
    assert len(seen) == 7     # (int8 with a persistent request is the int8 launch plan itself)


def test_shared_and_sampled_and_beam_and_staggered_plans_take_it(native_lib):
    f = mr.plan_fields(cr.describe(native_lib, TINY, 10, 1, enc_index=[0] * 5 + [1] * 5)[0])
    assert f["cross_int8"] == "1" and f["npairs"] == "6" and f["call.enc_rows"] == "1"
    f = mr.plan_fields(cr.describe(native_lib, SMALL, 10, 1, enc_index=[0] * 5 + [1] * 5)[0])
    assert f["cross_int8"] == "1" and f["npairs"] == "0" and f["call.enc_rows"] == "2"
    f = mr.plan_fields(cr.describe(native_lib, TURBO, 10, 1, enc_index=[0] * 5 + [1] * 5)[0])
    assert f["cross_int8"] == "1" and f["call.enc_rows"] == "2"
    assert "cross_int8=1" in cr.describe(native_lib, BASE, 4, 1, temperature=0.6)[0]
    beam = dict(beam_size=4, prompts=[[50257, 50362]] * 8, enc_index=[0] * 4 + [1] * 4)
    assert "cross_int8=1" in cr.describe(native_lib, BASE, 8, 1, **beam)[0]
    stagger = dict(max_length=40, pos_offset=[0, 0, 20, 20], steps=19, stand=[20] * 4, stand_maxlen=40)
    f = mr.plan_fields(cr.describe(native_lib, BASE, 4, 1, **stagger)[0])
    assert f["cross_int8"] == "1" and f["stagger"] == "1"


def test_persistent_request_plans_the_launch_path(native_lib):
    for level in (1, 2, 3):
        f = mr.plan_fields(cr.describe(native_lib, BASE, 8, 0, persistent=level)[0])
        assert f["persist"] == str(level)
        f = mr.plan_fields(cr.describe(native_lib, BASE, 8, 1, persistent=level)[0])
        assert f["persist"] == "0" and f["seg_grid"] == "0" and f["xrev"] == "0" and f["cross_int8"] == "1"


def test_refusals_arrive_by_name(native_lib):
    shared = dict(enc_index=[0] * 5 + [1] * 5)
    cases = [
        ("JANUS_DEC_PATH_NO_XABSORB with cross_compute int8", BASE, 8, jw.DEC_PATH_NO_XABSORB, {}),
        ("JANUS_DEC_PATH_XGROUP with cross_compute int8", BASE, 10, jw.DEC_PATH_XGROUP, shared),
        ("JANUS_DEC_PATH_XROWS with cross_compute int8", SMALL, 10, jw.dec_path_xrows(2), shared),
        ("JANUS_DEC_PATH_XROWS with cross_compute int8", SMALL, 10, jw.dec_path_xrows(4), shared),
    ]
    for match, cfg, B, flags, kw in cases:
        cr.describe(native_lib, cfg, B, 0, flags=flags, **kw)     # float16: all three still plan
        with pytest.raises(nat.JanusNativeError, match=match):
            cr.describe(native_lib, cfg, B, 1, flags=flags, **kw)
    with pytest.raises(nat.JanusNativeError, match="cross_compute int8 needs the absorbed cross-attention"):
        cr.describe(native_lib, BASE, 513, 1)
    with pytest.raises(nat.JanusNativeError, match="cross_compute must be"):
        cr.describe(native_lib, BASE, 8, 2)


# ------------------------------------------------------------------ Python arguments
@pytest.mark.parametrize("bad", ["int4", "INT8", "", None, 1, "float32", "int8_float16"])
def test_unknown_names_are_value_errors(bad):
    with pytest.raises(ValueError, match="cross_compute must be one of"):
        jw.cross_compute_mode(bad)
    with pytest.raises(ValueError, match="cross_compute must be one of"):
        jw.WhisperEngine(TINY, cross_compute=bad)          # before any device work
    with pytest.raises(ValueError, match="cross_compute must be one of"):
        tr.WhisperModel("tiny.en", cross_compute=bad)
    with pytest.raises(ValueError, match="cross_compute must be one of"):
        jw.WhisperEngine.set_cross_compute(object.__new__(jw.WhisperEngine), bad)


def test_whisper_model_passes_it_through(monkeypatch):
    seen = []

    class Engine:
        def __init__(self, cfg, **kw):
            seen.append((cfg.name, kw))

    monkeypatch.setattr(tr, "WhisperEngine", Engine)
    tr.WhisperModel("base.en", cross_compute="int8")
    tr.WhisperModel("base.en", compute_type="int8", apply_compute_type=True, cross_compute="int8")
    tr.WhisperModel("base.en", compute_type="int8")
    assert seen == [("base.en", dict(encoder_compute="float16", cross_compute="int8")),
                    ("base.en", dict(encoder_compute="int8", cross_compute="int8")),
                    ("base.en", dict(encoder_compute="float16"))]      # compute_type alone selects nothing here


def test_names_and_decode_path_field():
    assert jw.cross_compute_mode("float16") == 0 and jw.cross_compute_mode("int8") == 1
    assert jw.CROSS_COMPUTE_NAMES == ("float16", "int8")
    assert jw.DecodePath("own", 0) == jw.DecodePath("own", 0, "float16")     # the default: what ran before
    assert jw.DecodePath("own", 0, "int8").cross == "int8"
    # the faster-whisper front keeps its compute_type mapping: cross_compute is its own argument
    assert tr.resolve_compute_type("int8", True) == ("int8_float16", "int8")
    assert tr.resolve_compute_type("int8", False) == ("float16", "float16")


# ------------------------------------------------------------------ the reference's E'
def test_quantiser_on_hand_computed_rows():
    x = np.zeros((4, 16), np.float16)
    # row 0 stays zero: q = 0, s = 1, E' = 0
    # row 1: amax on a negative element
    x[1, :4] = [1.0, -3.0, 0.75, 2.9]
    # row 2: amax = 127, so inv = 1: ties go to even, +-127 stay
    x[2, :7] = [127.0, -127.0, 0.5, 1.5, 2.5, -0.5, -1.5]
    # row 3: amax = 2, s = 2 / 127
    x[3, :3] = [2.0, 1.0, -0.01]
    q, s = cr.quantise(x)
    assert q.dtype == np.int8 and s.dtype == np.float32
    assert not q[0].any() and s[0] == 1.0
    inv = F32(127) / F32(3)
    assert q[1, :4].tolist() == [int(np.rint(F32(1) * inv)), -127, int(np.rint(F32(0.75) * inv)),
                                 int(np.rint(F32(2.9).astype(np.float16).astype(F32) * inv))]
    assert q[1, :4].tolist() == [42, -127, 32, 123] and q[1].max() < 127 and s[1] == F32(3) / F32(127)
    assert q[2, :7].tolist() == [127, -127, 0, 2, 2, 0, -2] and s[2] == 1.0
    assert q[3, :3].tolist() == [127, 64, -1] and s[3] == F32(2) / F32(127)   # 63.5 -> 64 (even), -0.635 -> -1

    e = cr.dequantised(x)
    assert e.dtype == np.float16 and e.shape == x.shape
    assert not e[0].any()
    # q * s in float32, rounded once to fp16
    assert e[1, :4].tolist() == [float(np.float16(F32(v) * (F32(3) / F32(127)))) for v in (42, -127, 32, 123)]
    assert e[1, 1] == np.float16(-3.0)                       # the extreme comes back exactly
    assert e[2, :7].tolist() == [127.0, -127.0, 0.0, 2.0, 2.0, 0.0, -2.0]
    assert e[3, 0] == np.float16(2.0) and e[3, 1] == np.float16(F32(64) * (F32(2) / F32(127)))
    assert abs(float(e[3, 1]) - 1.0) > 1e-3                  # 1.0 is no level of this row: 1.0079
    # leading axes are rows of their own
    e3 = cr.dequantised(np.stack([x, x[::-1]]))
    assert np.array_equal(e3[0], e) and np.array_equal(e3[1], e[::-1])


def test_outlier_inputs_plant_the_edge_rows():
    cfg = cr.ref.config(512, 8)
    tokens, enc = cr.outlier_inputs(cfg, 2, 3, 5)
    plain = cr.ref.inputs(cfg, 2, 3, 5)[1]
    assert enc.dtype == np.float16 and enc.shape == plain.shape and np.array_equal(tokens, cr.ref.inputs(cfg, 2, 3, 5)[0])
    for e in range(2):
        assert not enc[e, 3].any()
        assert np.abs(enc[e, 5]).max() == 6.0 and enc[e, 5, 7] == -6.0
        for t in range(0, cfg.n_audio_ctx, 2):
            assert np.abs(enc[e, t]).max() == cr.OUTLIER and (enc[e, t] == cr.OUTLIER).sum() == 1
        for t in range(1, cfg.n_audio_ctx, 2):
            if t not in (3, 5):
                assert np.array_equal(enc[e, t], plain[e, t])
    q, s = cr.quantise(enc)
    assert not q[0, 3].any() and s[0, 3] == 1.0 and q[0, 5, 7] == -127 and q[0, 5].max() < 127
    assert s[0, 0] == F32(16) / F32(127)
