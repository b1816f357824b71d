"""The decode planner (csrc/decode_plan.cpp) through janus_decode_plan_describe, on the CPU:
which path a decode call takes, every rejection with its message, and the graph cache key.
Expected values are the rules as plan_decode's comments state them."""
import ctypes
import itertools

import numpy as np
import pytest

from janus_amd import _native as nat
from janus_amd import whisper as jw
from janus_amd.whisper import CONFIGS, dec_path_ln_mask, dec_path_xrows

BASE, TINY, SMALL = CONFIGS["base.en"], CONFIGS["tiny.en"], CONFIGS["small.en"]
BEST_OF = [0] * 5 + [1] * 5      # best_of = 5 rows per window, 2 windows
OWN, IN_PLACE, GATHERED = 0, 1, 2
I32P = ctypes.POINTER(ctypes.c_int32)


def _i32(values):
    a = np.ascontiguousarray(np.asarray(values, np.int32))
    return a, a.ctypes.data_as(I32P)


def describe(native_lib, cfg, B, flags=0, persistent=0, max_length=448, cus=256, resident=True,
             multi_lane=False, temperature=0.0, temperatures=None, beam_size=0, enc_index=None,
             n_enc=None, pos_offset=None, steps=0, stand=None, stand_maxlen=0, prompts=None,
             check_every=16):
    """(fields, key): the plan's name=value lines as a dict (ints; pairs / groups as lists)
    and its graph-key contribution. Raises JanusNativeError where the planner rejects."""
    c = jw.janus_whisper_config(cfg.n_mels, cfg.n_audio_ctx, cfg.d_model, cfg.n_heads,
                                cfg.enc_layers, cfg.dec_layers, cfg.n_vocab, cfg.n_text_ctx)
    keep = []
    opt = jw.janus_decode_options()
    pr, opt.prompt = _i32([50257, 50362])
    keep.append(pr)
    opt.prompt_len, opt.max_length, opt.eot = 2, max_length, 50256
    opt.suppress_blank, opt.blank_token = 1, 220
    opt.timestamp_begin, opt.no_timestamps, opt.max_initial_timestamp_index = 50363, 50362, 50
    opt.check_every, opt.persistent, opt.path_flags = check_every, persistent, flags
    rows = jw.janus_decode_rows()
    rows.no_speech_token = 50361
    if enc_index is not None:
        a, rows.enc_index = _i32(enc_index)
        keep.append(a)
        rows.n_enc = n_enc if n_enc is not None else max(enc_index) + 1
    if pos_offset is not None:
        a, rows.pos_offset = _i32(pos_offset)
        keep.append(a)
        rows.steps = steps
    if prompts is not None:
        stride = max(len(p) for p in prompts)
        flat = np.zeros((B, stride), np.int32)
        for b, p in enumerate(prompts):
            flat[b, :len(p)] = p
        a, rows.prompts = _i32(flat)
        ln, rows.prompt_lens = _i32([len(p) for p in prompts])
        keep += [a, ln]
        rows.stride = stride
    temps = None
    if temperatures is not None:
        temps = np.ascontiguousarray(np.asarray(temperatures, np.float32))
    st = np.ascontiguousarray(np.asarray(stand if stand is not None else [], np.int32))
    text = ctypes.create_string_buffer(1 << 16)
    key = (ctypes.c_int64 * 256)()
    n_key = ctypes.c_int32(0)
    nat.check(native_lib.janus_decode_plan_describe(
        ctypes.addressof(c), ctypes.addressof(opt), ctypes.addressof(rows), B, cus, int(resident),
        int(multi_lane), ctypes.c_float(temperature), temps.ctypes.data if temps is not None else None,
        beam_size, st.ctypes.data if st.size else None, int(st.size), stand_maxlen,
        ctypes.addressof(text), len(text), ctypes.addressof(key), len(key), ctypes.addressof(n_key)))
    del keep
    fields = {}
    for line in text.value.decode().splitlines():
        name, value = line.split("=", 1)
        if name in ("pairs", "groups"):
            fields[name] = [int(v) for v in value.split(",")] if value else []
        else:
            fields[name] = float(value) if name == "R.inv_temp" else int(value)
    return fields, tuple(key[:n_key.value])


def rejected(native_lib, match, *args, **kw):
    with pytest.raises(nat.JanusNativeError, match=match):
        describe(native_lib, *args, **kw)


# ------------------------------------------------------------------ defaults by row count
def test_defaults_by_row_count(native_lib):
    p, _ = describe(native_lib, BASE, 64)
    assert (p["xabs"], p["xsplit"], p["cvp"], p["ln_pro_mask"], p["embed_ln"], p["fuse_se"]) == (1, 8, 1, 9, 1, 1)
    assert p["persist"] == 0 and p["call.enc_rows"] == OWN and p["call.use_graph"] == 1
    assert (p["call.steps"], p["call.f0"], p["call.f1"], p["sample_begin"]) == (447, 0, 64, 2)
    assert (p["lg_cap"], p["msplit_n"], p["chunk"]) == (256, 0, 16)
    p, _ = describe(native_lib, BASE, 128)
    assert (p["ln_pro_mask"], p["cvp"], p["xabs"]) == (0, 0, 1)
    p, _ = describe(native_lib, BASE, 128, jw.DEC_PATH_CVP)
    assert p["cvp"] == 1
    assert describe(native_lib, BASE, 64, jw.DEC_PATH_NO_CVP)[0]["cvp"] == 0
    assert describe(native_lib, BASE, 64, jw.DEC_PATH_NO_XABSORB)[0]["xabs"] == 0
    assert describe(native_lib, BASE, 64, jw.DEC_PATH_NO_GRAPH)[0]["call.use_graph"] == 0
    # a half-GPU partition: one logits block per CU, the skinny projections split rows
    p, _ = describe(native_lib, BASE, 64, cus=128)
    assert (p["lg_cap"], p["msplit_n"]) == (128, 1024)


@pytest.mark.parametrize("B", [64, 128])
def test_ln_mask_is_taken_as_given(native_lib, B):
    for m in range(16):
        assert describe(native_lib, BASE, B, dec_path_ln_mask(m))[0]["ln_pro_mask"] == m


def test_layernorm_placements_exclude_one_another(native_lib):
    F, L, R = jw.DEC_PATH_FUSED_LN, jw.DEC_PATH_LN_FUSE, jw.DEC_PATH_RESID_LN
    names = ("fused_ln", "ln_fuse", "rln", "ln_pro_mask", "embed_ln")

    def got(flags, B=64, cfg=BASE):
        p, _ = describe(native_lib, cfg, B, flags)
        return tuple(p[n] for n in names)
    assert got(F) == (1, 0, 0, 0, 0)
    assert got(L) == (0, 1, 0, 0, 0)
    assert got(R) == (0, 0, 1, 9, 1)
    assert got(F | L | R) == (1, 0, 0, 0, 0)        # FUSED_LN wins over both
    assert got(L | R) == (0, 1, 0, 0, 0)            # LN_FUSE over RESID_LN
    assert got(F | dec_path_ln_mask(15)) == (1, 0, 0, 0, 0)
    assert got(R | dec_path_ln_mask(15)) == (0, 0, 1, 15, 1)
    # all three are for <= 64 rows; LN_FUSE and RESID_LN for d_model <= 512
    assert got(F | L | R, B=128) == (0, 0, 0, 0, 1)
    assert got(F, cfg=SMALL) == (1, 0, 0, 0, 0)
    assert got(L | R, cfg=SMALL) == (0, 0, 0, 0, 0)


# ------------------------------------------------------------------ shared encoder rows
@pytest.mark.parametrize("cfg", [TINY, BASE], ids=["tiny", "base"])
def test_shared_rows_pairs_and_groups(native_lib, cfg):
    p, _ = describe(native_lib, cfg, 10, enc_index=BEST_OF)
    assert p["call.enc_rows"] == IN_PLACE and p["call.n_enc"] == 2 and p["ngroups"] == 0
    assert p["pairs"] == [0, 1, 0, 2, 3, 0, 4, -1, 0, 5, 6, 1, 7, 8, 1, 9, -1, 1]
    assert p["npairs"] == 6
    p, _ = describe(native_lib, cfg, 10, jw.DEC_PATH_XGROUP, enc_index=BEST_OF)
    assert p["call.enc_rows"] == IN_PLACE and p["npairs"] == 0
    assert (p["ngroups"], p["grp_rows"], p["n_main"], p["cvp"]) == (2, 5, -1, 1)
    assert p["groups"] == [0, 0, 1, 2, 3, 4, -1, -1, 1, 5, 6, 7, 8, 9, -1, -1]
    for flag in (jw.DEC_PATH_NO_XPAIR, jw.DEC_PATH_NO_XABSORB):
        p, _ = describe(native_lib, cfg, 10, flag, enc_index=BEST_OF)
        assert p["call.enc_rows"] == GATHERED and p["call.n_enc"] == 10 and p["npairs"] == 0
    rejected(native_lib, "need the fused merge", cfg, 10, jw.DEC_PATH_XGROUP | jw.DEC_PATH_NO_CVP,
             enc_index=BEST_OF)
    rejected(native_lib, "enc_index out of range", cfg, 10, enc_index=BEST_OF, n_enc=1)


def test_shared_rows_small_family(native_lib):
    p, _ = describe(native_lib, SMALL, 10, enc_index=BEST_OF)
    assert p["call.enc_rows"] == GATHERED and p["ngroups"] == 0 and p["npairs"] == 0 and p["wide"] == 1
    p, _ = describe(native_lib, SMALL, 10, dec_path_xrows(4), enc_index=BEST_OF)
    assert p["call.enc_rows"] == IN_PLACE
    assert (p["ngroups"], p["n_main"], p["grp_rows"], p["rem_rows"]) == (4, 2, 4, 1)
    none = [-1] * 6
    assert p["groups"] == ([0, 0, 1, 2, 3, -1, -1, -1] + [1, 5, 6, 7, 8, -1, -1, -1]
                           + [0, 4] + none + [1, 9] + none)
    p, _ = describe(native_lib, SMALL, 10, dec_path_xrows(2), enc_index=BEST_OF)
    assert (p["ngroups"], p["n_main"], p["grp_rows"], p["rem_rows"]) == (6, 4, 2, 1)
    five = [-1] * 5
    assert p["groups"] == ([0, 0, 1] + five + [0, 2, 3] + five + [1, 5, 6] + five + [1, 7, 8] + five
                           + [0, 4] + none + [1, 9] + none)
    rejected(native_lib, r"JANUS_DEC_PATH_XGROUP \(GROUP blocks of 8-head rows\) needs H <= 8, d <= 512",
             SMALL, 10, jw.DEC_PATH_XGROUP, enc_index=BEST_OF)
    rejected(native_lib, r"JANUS_DEC_PATH_XROWS\(n\) is n = 2 or 4 rows per block at 12 heads",
             BASE, 10, dec_path_xrows(4), enc_index=BEST_OF)


# ------------------------------------------------------------------ persistent requests
@pytest.mark.parametrize("B", [8, 64, 128])
@pytest.mark.parametrize("req", [1, 2, 3])
def test_persistent_level(native_lib, req, B):
    p, _ = describe(native_lib, BASE, B, persistent=req)
    assert p["persist"] == req and p["seg_grid"] > 0
    assert p["xrev"] == 1 and describe(native_lib, BASE, B, jw.DEC_PATH_XFWD, persistent=req)[0]["xrev"] == 0
    assert describe(native_lib, BASE, B, persistent=req, resident=False)[0]["persist"] == 0
    assert describe(native_lib, BASE, B, persistent=req, multi_lane=True)[0]["persist"] == 0
    assert describe(native_lib, SMALL, B, persistent=req)[0]["persist"] == 0
    assert describe(native_lib, TINY, B, persistent=req)[0]["persist"] == 0
    assert describe(native_lib, BASE, B, jw.DEC_PATH_RESID_LN, persistent=req)[0]["persist"] == (0 if B <= 64 else req)


@pytest.mark.parametrize("req", [1, 2, 3])
def test_persistent_falls_back(native_lib, req):
    assert describe(native_lib, BASE, 10, persistent=req, enc_index=BEST_OF)[0]["persist"] == 0
    prompts = [[50257, 50362]] * 8
    p, _ = describe(native_lib, BASE, 8, persistent=req, beam_size=4, prompts=prompts,
                    enc_index=[0] * 4 + [1] * 4)
    assert p["persist"] == 0 and p["seg_grid"] == 0
    # too few CUs for the rows: 16 per 16 rows
    assert describe(native_lib, BASE, 64, persistent=req, cus=32)[0]["persist"] == 0
    assert describe(native_lib, BASE, 257, persistent=req)[0]["persist"] == 0


# ------------------------------------------------------------------ staggered rows
def test_stagger_mixed_call(native_lib):
    p, _ = describe(native_lib, BASE, 4, max_length=40, pos_offset=[0, 0, 20, 20], steps=19,
                    stand=[20] * 4, stand_maxlen=40)
    assert (p["call.f0"], p["call.f1"], p["max_roff"], p["call.steps"], p["sample_begin"]) == (0, 2, 20, 19, 0)
    assert p["stagger"] == 1
    p, _ = describe(native_lib, BASE, 4, max_length=40, pos_offset=[7, 0, 0, 3], steps=5,
                    stand=[7, 0, 0, 3], stand_maxlen=40)
    assert (p["call.f0"], p["call.f1"], p["max_roff"], p["call.steps"], p["sample_begin"]) == (1, 3, 7, 5, 0)
    # everything fresh: the rows sample from their prompt's end; steps 0 = max_length - 1
    p, _ = describe(native_lib, BASE, 4, max_length=40, pos_offset=[0] * 4)
    assert (p["call.f0"], p["call.f1"], p["max_roff"], p["call.steps"], p["sample_begin"]) == (0, 4, 0, 39, 2)
    # nothing fresh
    p, _ = describe(native_lib, BASE, 2, max_length=40, pos_offset=[5, 9], steps=3, stand=[9, 9],
                    stand_maxlen=40)
    assert (p["call.f0"], p["call.f1"], p["max_roff"], p["sample_begin"]) == (0, 0, 9, 0)


def test_stagger_rejections(native_lib):
    kw = dict(max_length=40, stand=[20] * 4, stand_maxlen=40)
    rejected(native_lib, "decode: fresh rows must be contiguous", BASE, 4, pos_offset=[0, 5, 0, 5], steps=5, **kw)
    rejected(native_lib, "decode: row 2 continues at pos_offset 21 but its slot stands at 20", BASE, 4,
             pos_offset=[0, 0, 21, 20], steps=5, **kw)
    rejected(native_lib, r"decode: pos_offset \+ steps > max_length", BASE, 4, pos_offset=[0, 0, 20, 20],
             steps=21, **kw)
    rejected(native_lib, "decode: pos_offset out of range", BASE, 4, pos_offset=[0, 0, 40, 20], steps=1, **kw)
    rejected(native_lib, "decode: staggered rows are greedy, unshared", BASE, 4, pos_offset=[0, 0, 20, 20],
             steps=5, temperature=0.5, **kw)
    rejected(native_lib, "decode: staggered rows are greedy, unshared", BASE, 4, pos_offset=[0, 0, 20, 20],
             steps=5, enc_index=[0, 0, 1, 1], **kw)
    rejected(native_lib, "decode: continuing rows need the previous call's batch size and max_length",
             BASE, 4, max_length=40, pos_offset=[0, 0, 20, 20], steps=5, stand=[20] * 3, stand_maxlen=40)
    rejected(native_lib, "decode: continuing rows need the previous call's batch size and max_length",
             BASE, 4, max_length=40, pos_offset=[0, 0, 20, 20], steps=5, stand=[20] * 4, stand_maxlen=48)
    rejected(native_lib, "decode: continuing rows need the previous call's batch size and max_length",
             BASE, 4, max_length=40, pos_offset=[0, 0, 20, 20], steps=5)
    rejected(native_lib, "decode: staggered rows run the default decoder kernels only", BASE, 4,
             jw.DEC_PATH_RESID_LN, pos_offset=[0, 0, 20, 20], steps=5, **kw)
    rejected(native_lib, "decode: staggered rows run the default decoder kernels only", BASE, 4,
             jw.DEC_PATH_NO_XABSORB, pos_offset=[0, 0, 20, 20], steps=5, **kw)


# ------------------------------------------------------------------ beam search, sampling
def test_beam(native_lib):
    prompts = [[50257, 50362]] * 8
    beam = dict(beam_size=4, prompts=prompts, enc_index=[0] * 4 + [1] * 4)
    p, _ = describe(native_lib, BASE, 8, **beam)
    assert (p["fuse_se"], p["nwin"], p["beam_k"], p["call.enc_rows"]) == (0, 2, 4, IN_PLACE)
    assert describe(native_lib, BASE, 8)[0]["nwin"] == 0
    rejected(native_lib, r"decode: beam search does not take staggered rows \(pos_offset\)", BASE, 8,
             beam_size=4, prompts=prompts, pos_offset=[0] * 8)
    rejected(native_lib, "decode: beam search runs at temperature 0", BASE, 8, temperature=0.4, **beam)
    rejected(native_lib, "decode: beam search needs per-row prompts, max_length <= 448", BASE, 8,
             max_length=449, **beam)
    rejected(native_lib, "decode: beam search needs per-row prompts, max_length <= 448", BASE, 8,
             beam_size=4, enc_index=[0] * 4 + [1] * 4)
    rejected(native_lib, "decode: beam_size must be 1 .. 8", BASE, 8, beam_size=3, prompts=prompts)


def test_sampling_and_prompts(native_lib):
    p, _ = describe(native_lib, BASE, 4, temperature=0.5)
    assert (p["sampling"], p["row_temps"], p["R.inv_temp"]) == (1, 0, 2.0)
    p, _ = describe(native_lib, BASE, 4, temperatures=[0.0, 0.5, 1.0, 0.2])
    assert (p["sampling"], p["row_temps"], p["R.inv_temp"]) == (1, 1, 1.0)
    assert describe(native_lib, BASE, 4)[0]["R.inv_temp"] == 0.0
    # per-row prompts: the earliest row's first sampled token
    p, _ = describe(native_lib, BASE, 3, max_length=40, prompts=[[1, 2, 3, 4], [1, 2], [1, 2, 3]])
    assert p["sample_begin"] == 2
    rejected(native_lib, "decode: per-row prompt length out of range", BASE, 2, max_length=4,
             prompts=[[1, 2, 3, 4], [1, 2]])
    rejected(native_lib, "decode: need 1 <= prompt_len < max_length <= n_text_ctx", BASE, 2, max_length=449)


# ------------------------------------------------------------------ the graph cache key
SINGLE_FLAGS = [jw.DEC_PATH_NO_GRAPH, jw.DEC_PATH_NO_XABSORB, jw.DEC_PATH_NO_XPAIR, jw.DEC_PATH_XGROUP,
                jw.DEC_PATH_FUSED_LN, jw.DEC_PATH_LN_FUSE, jw.DEC_PATH_RESID_LN, jw.DEC_PATH_NO_CVP,
                jw.DEC_PATH_CVP, jw.DEC_PATH_NO_SEL_EMBED, jw.DEC_PATH_NO_EMBED_LN,
                jw.DEC_PATH_LN_PROLOGUE, jw.DEC_PATH_SEG_2CU, jw.DEC_PATH_XFWD]
GRID_FLAGS = [0] + SINGLE_FLAGS + [dec_path_ln_mask(m) for m in (0, 9, 15)] + [dec_path_xrows(n) for n in (2, 4)]


def test_key_equals_exactly_when_the_step_fields_do(native_lib):
    """Over the grid of single flags x rows x persistent x model (valid combinations): two
    plans contribute the same graph key exactly when every field a captured position reads
    (the fields not marked call.) is equal."""
    plans = []
    for cfg, flags, B, pers in itertools.product((TINY, BASE, SMALL), GRID_FLAGS, (8, 64, 128), (0, 2)):
        try:
            fields, key = describe(native_lib, cfg, B, flags, persistent=pers)
        except nat.JanusNativeError:
            assert (flags & jw.DEC_PATH_XGROUP and cfg is SMALL) or (flags >> 18 and cfg is not SMALL)
            continue
        step = tuple(sorted((n, v) for n, v in fields.items()
                            if not n.startswith("call.") and n not in ("pairs", "groups")))
        plans.append((step, key, cfg.d_model))
    assert len(plans) > 300
    by_key, by_step = {}, {}
    for step, key, d in plans:
        assert by_key.setdefault(key, step) == step, "one key, two sets of fields"
        assert by_step.setdefault(step, key) == key, "one set of fields, two keys"
        assert len(key) == len(step)
    assert len(by_key) > 20


@pytest.mark.parametrize("level", [1, 2, 3])
def test_key_holds_the_cross_attention_sweep_direction(native_lib, level):
    """JANUS_DEC_PATH_XFWD reaches xattn_launch inside the captured step at the persistent
    levels: two calls that differ in it alone must not share a graph. On the launch path the
    flag decides nothing, and the calls keep sharing."""
    _, rev = describe(native_lib, BASE, 64, persistent=level)
    _, fwd = describe(native_lib, BASE, 64, jw.DEC_PATH_XFWD, persistent=level)
    assert rev != fwd
    assert describe(native_lib, BASE, 64)[1] == describe(native_lib, BASE, 64, jw.DEC_PATH_XFWD)[1]
    # flags that decide nothing at a shape keep sharing: CVP up to 64 rows, SEG_2CU off 256 rows
    assert describe(native_lib, BASE, 64)[1] == describe(native_lib, BASE, 64, jw.DEC_PATH_CVP)[1]
    assert (describe(native_lib, BASE, 64, persistent=level)[1]
            == describe(native_lib, BASE, 64, jw.DEC_PATH_SEG_2CU, persistent=level)[1])
