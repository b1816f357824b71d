"""The 1024-wide, 16-head family (medium.en, distil-medium.en) on the host: the configs and
names, the checkpoint loader's checks, the decode planner at d_model 1024 / 16 heads, the
vocabulary projection's row group, and what the family refuses by name (beam search, the int8
encoder, JanusPipeline, StreamingEncoder) and what it does not (word timestamps)."""
import dataclasses
import types

import numpy as np
import pytest

import medium_family_ref as mf
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd import whisper as jw
from janus_amd.whisper import (CONFIGS, DEC_PATH_CVP, DEC_PATH_LN_FUSE, DEC_PATH_NO_CVP, DEC_PATH_NO_EMBED_LN,
                               DEC_PATH_RESID_LN, DEC_PATH_XGROUP, WhisperConfig, dec_path_ln_mask,
                               dec_path_xrows)

CUT = mf.CUT
NAMES = ("medium.en", "distil-medium.en")


# ------------------------------------------------------------------ configs and names
def test_configs_and_names():
    for name, enc, dec in (("medium.en", 24, 24), ("distil-medium.en", 24, 2)):
        c = CONFIGS[name]
        assert (c.name, c.d_model, c.n_heads, c.enc_layers, c.dec_layers) == (name, 1024, 16, enc, dec)
        assert (c.n_mels, c.n_vocab, c.n_audio_ctx, c.ffn, c.multilingual) == (80, 51864, 1500, 4096, False)
        assert jw.resolve_model(name) == name
        assert jw.large_family(c) and not jw.shared_rows_in_place(c)
    assert (CUT.d_model, CUT.n_heads, CUT.enc_layers, CUT.dec_layers, CUT.n_vocab) == (1024, 16, 2, 2, 51864)
    tk = tok.load_tokenizer(multilingual=False, n_vocab=CONFIGS["medium.en"].n_vocab)
    assert (tk.eot, tk.sot, tk.no_speech, tk.timestamp_begin, tk.n_vocab) == (50256, 50257, 50361, 50363, 51864)
    assert tk.sot_sequence == [50257] and tk.supported_languages() == ["en"]


def test_multilingual_medium_stays_unknown():
    """The 51 865-id `medium` has the same shapes; only its name is not registered."""
    assert "medium" not in CONFIGS
    with pytest.raises(ValueError, match="unknown model"):
        jw.resolve_model("medium")
    from janus_amd.services.transcriber import WhisperModel
    with pytest.raises(ValueError, match="unknown model size"):
        WhisperModel("medium")


def test_alignment_heads_default_against_the_limit():
    """The product's default set (every head of the last half of the decoder layers) against the
    alignment pass's limit: 16 heads on distil-medium.en, 192 on medium.en — more than
    ALIGN_MAX_HEADS, so word timestamps there need a named set. The native default agrees
    (align_default_heads throws past the limit: the host check comes first)."""
    full, distil = CONFIGS["medium.en"], CONFIGS["distil-medium.en"]
    assert jw.ALIGN_MAX_HEADS == 64
    assert jw.default_alignment_heads(distil) == [(1, h) for h in range(16)]
    assert jw.default_alignment_heads(full) == [(l, h) for l in range(12, 24) for h in range(16)]
    assert len(jw.default_alignment_heads(distil)) <= jw.ALIGN_MAX_HEADS < len(jw.default_alignment_heads(full))
    assert jw.check_alignment_heads(distil, [(1, 15), (0, 0)]) is not None
    with pytest.raises(ValueError, match="out of range"):
        jw.check_alignment_heads(distil, [(1, 16)])
    with pytest.raises(ValueError, match="192 heads, the limit is 64"):
        jw.check_alignment_heads(full, jw.default_alignment_heads(full))
    assert len(jw.check_alignment_heads(full, jw.default_alignment_heads(full)[:64])) == 64


def test_word_timestamps_on_medium_en_need_named_heads(monkeypatch):
    """medium.en's default set exceeds the limit: word_timestamps is refused by name on the host
    (generate_segments, WhisperModel.transcribe, WhisperEngine.align), before any GPU work, unless
    the engine was given at most 64 named heads; distil-medium.en's default set passes."""
    from janus_amd.services import transcriber as tr
    audio = [np.zeros(16000, np.float32)]
    full, distil = CONFIGS["medium.en"], CONFIGS["distil-medium.en"]
    with pytest.raises(NotImplementedError, match=r"word_timestamps on medium\.en: its alignment set has 192 heads"):
        jw.check_family_features(full, word_timestamps=True)
    eng = types.SimpleNamespace(cfg=full, alignment_heads=jw.default_alignment_heads(full))
    with pytest.raises(NotImplementedError, match=r"word_timestamps on medium\.en.*at most 64"):
        tr.generate_segments(eng, audio, word_timestamps=True)
    m = tr.WhisperModel.__new__(tr.WhisperModel)
    m.engine = eng
    with pytest.raises(NotImplementedError, match=r"word_timestamps on medium\.en"):
        m.transcribe(audio[0], word_timestamps=True)
    e = jw.WhisperEngine.__new__(jw.WhisperEngine)
    e.cfg, e.alignment_heads = full, eng.alignment_heads
    with pytest.raises(NotImplementedError, match=r"word_timestamps on medium\.en"):
        e.align(None, [[300]], [3000])
    # a named set within the limit, and the distil model's default set, pass the check
    jw.check_family_features(full, word_timestamps=True, alignment_heads=[(23, 0), (20, 7)])
    jw.check_family_features(distil, word_timestamps=True)
    named = types.SimpleNamespace(cfg=full, alignment_heads=[(23, 0), (20, 7)])
    with pytest.raises(AttributeError):          # past the refusals: the stub has no tokenizer
        tr.generate_segments(named, audio, word_timestamps=True)
    # WhisperModel hands a named set to its engine
    seen = {}

    class Engine:
        def __init__(self, cfg, **kw):
            seen.update(kw, cfg=cfg)
    monkeypatch.setattr(tr, "WhisperEngine", Engine)
    tr.WhisperModel("medium.en", alignment_heads=[(23, 0)])
    assert seen["cfg"] is full and seen["alignment_heads"] == [(23, 0)]
    seen.clear()
    tr.WhisperModel("medium.en")
    assert "alignment_heads" not in seen


# ------------------------------------------------------------------ loader
TINY_MEDIUM = WhisperConfig("distil-medium.en", 64, 1, 3, 1, n_audio_ctx=8, n_text_ctx=8)


def _save(path, W, drop=()):
    from safetensors.numpy import save_file
    sd = {"model." + k: np.ascontiguousarray(v) for k, v in W.items() if k not in drop}
    save_file(sd, str(path / "model.safetensors"))


def test_loader_checks_stem_depth_and_vocabulary(tmp_path, monkeypatch):
    """conv1.weight [d][80][3], encoder and decoder depth apart, the 51 864 vocabulary: a
    distil-medium.en file under the medium.en name, and the reverse, is refused by name and
    layer count (shapes cut to d = 64 and depths to 3 / 1 so the file stays small)."""
    pytest.importorskip("safetensors")
    cfg = TINY_MEDIUM
    W = jw.synthetic_weights(cfg, seed=1)
    _save(tmp_path, W)
    monkeypatch.setenv("JANUS_WHISPER_DIR", str(tmp_path))
    got = jw.load_weights(cfg)
    assert got["encoder.conv1.weight"].shape == (64, 80, 3)
    assert got["decoder.embed_tokens.weight"].shape == (51864, 64)
    # the distil file (1 decoder layer) under the teacher's name (as many decoder as encoder layers)
    with pytest.raises(ValueError, match=r"medium\.en: 1 decoder layers, the config has 3"):
        jw.load_weights(dataclasses.replace(cfg, name="medium.en", dec_layers=3))
    # the teacher's file under the distil name
    full = dataclasses.replace(cfg, name="medium.en", dec_layers=3)
    _save(tmp_path, jw.synthetic_weights(full, seed=1))
    with pytest.raises(ValueError, match=r"distil-medium\.en: 3 decoder layers, the config has 1"):
        jw.load_weights(cfg)
    _save(tmp_path, W)
    with pytest.raises(ValueError, match="3 encoder layers, the config has 4"):
        jw.load_weights(dataclasses.replace(cfg, enc_layers=4))
    # a 128-bin stem under an 80-bin name
    bad = dict(W)
    bad["encoder.conv1.weight"] = np.concatenate([W["encoder.conv1.weight"]] * 2, 1)[:, :128].copy()
    _save(tmp_path, bad)
    with pytest.raises(ValueError, match=r"distil-medium\.en.*conv1\.weight.*\(64, 128, 3\)"):
        jw.load_weights(cfg)
    # the multilingual vocabulary (51 865 rows) under a *.en name
    bad = dict(W)
    E = W["decoder.embed_tokens.weight"]
    bad["decoder.embed_tokens.weight"] = np.concatenate([E, E[:1]], 0)
    _save(tmp_path, bad)
    with pytest.raises(ValueError, match=r"distil-medium\.en: decoder\.embed_tokens\.weight \(51865, 64\)"):
        jw.load_weights(cfg)


def test_tokenizer_json_special_ids(tmp_path):
    """The *.en layout's special ids are checked against a tokenizer.json: a multilingual file
    (every special id one higher) is refused."""
    pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, models

    def write(specials):
        vocab = {"a": 0}
        vocab.update(specials)
        Tokenizer(models.WordLevel(vocab, unk_token="a")).save(str(tmp_path / "tokenizer.json"))
    write({"<|endoftext|>": 50256, "<|startoftranscript|>": 50257, "<|startofprev|>": 50360,
           "<|nospeech|>": 50361, "<|notimestamps|>": 50362, "<|0.00|>": 50363})
    tk = tok.WhisperTokenizer(str(tmp_path), n_vocab=CONFIGS["medium.en"].n_vocab)
    assert tk.timestamp_begin == 50363
    write({"<|endoftext|>": 50257, "<|startoftranscript|>": 50258, "<|startofprev|>": 50361,
           "<|nospeech|>": 50362, "<|notimestamps|>": 50363, "<|0.00|>": 50364})
    with pytest.raises(ValueError, match=r"\*\.en layout"):
        tok.WhisperTokenizer(str(tmp_path), n_vocab=CONFIGS["medium.en"].n_vocab)


# ------------------------------------------------------------------ the planner at 1024 / 16
def test_plan_launch_path_and_persistent(native_lib):
    p = mf.describe(native_lib, CUT, 8)
    assert p["wide"] == "1" and p["xabs"] == "1" and p["persist"] == "0" and p["call.enc_rows"] == "0"
    # every fusion guarded by d <= 512 is off
    assert (p["ln_pro_mask"], p["embed_ln"], p["cvp"], p["rln"], p["ln_fuse"]) == ("0", "0", "0", "0", "0")
    q = mf.describe(native_lib, CUT, 8, persistent=2)
    assert q["persist"] == "0" and q["xrev"] == "0"
    for full in NAMES:
        assert mf.describe(native_lib, CONFIGS[full], 64, persistent=3)["persist"] == "0"
        assert mf.describe(native_lib, CONFIGS[full], 64)["wide"] == "1"


def test_plan_shared_rows_are_gathered(native_lib):
    ei = [0] * 5 + [1] * 5
    p = mf.describe(native_lib, CUT, 10, enc_index=ei, temperature=0.6)
    assert p["call.enc_rows"] == "2" and p["pairs"] == "" and p["groups"] == ""   # JANUS_ENC_ROWS_GATHERED
    assert (p["npairs"], p["ngroups"], p["call.n_enc"], p["sampling"]) == ("0", "0", "10", "1")


@pytest.mark.parametrize("flags,match", [(dec_path_xrows(2), "12 heads"), (dec_path_xrows(4), "12 heads"),
                                         (DEC_PATH_XGROUP, "H <= 8")], ids=["xrows2", "xrows4", "xgroup"])
def test_plan_refuses_shared_row_blocks_by_their_messages(native_lib, flags, match):
    with pytest.raises(nat.JanusNativeError, match=match):
        mf.describe(native_lib, CUT, 4, enc_index=[0, 0, 0, 1], path_flags=flags)


@pytest.mark.parametrize("flags", [DEC_PATH_NO_CVP, DEC_PATH_CVP, DEC_PATH_NO_EMBED_LN, DEC_PATH_LN_FUSE,
                                   DEC_PATH_RESID_LN, dec_path_ln_mask(15)])
def test_plan_fusion_flags_change_nothing(native_lib, flags):
    a = mf.describe(native_lib, CUT, 8)
    b = mf.describe(native_lib, CUT, 8, path_flags=flags)
    assert a == b


def test_plan_refuses_beam_at_1024(native_lib):
    with pytest.raises(nat.JanusNativeError, match="d_model <= 768"):
        mf.describe(native_lib, CUT, 8, beam_size=4, enc_index=[0] * 4 + [1] * 4)


def test_projection_row_group_and_history_layout(native_lib):
    """48-row groups at K = 1024 (janus_history_words is [groups of logits_row_group(K)][tiles]
    [rows of the group]): the word count steps at 49 rows; at 33 rows at 1280 and at 65 rows up
    to 768, as before."""
    tiles = (mf.V + 15) // 16
    assert tiles == 3242 and mf.V == 16 * 3241 + 8
    for B, groups in ((1, 1), (47, 1), (48, 1), (49, 2), (96, 2), (97, 3)):
        assert native_lib.janus_history_words(mf.V, 1024, B) == groups * tiles * mf.ROW_GROUP, B
    assert mf.ROW_GROUP == 48
    assert native_lib.janus_history_words(mf.V + 2, 1280, 33) == 2 * ((mf.V + 2 + 15) // 16) * 32
    assert native_lib.janus_history_words(mf.V, 768, 64) == tiles * 64
    assert native_lib.janus_history_words(mf.V, 768, 65) == 2 * tiles * 64
    # the projection's blocks per row: one per 8 tiles, capped
    assert native_lib.janus_beam_partial_blocks(mf.V, 1024, 256) == 256
    assert native_lib.janus_beam_partial_blocks(mf.V, 1024, 1024) == (tiles + 7) // 8


# ------------------------------------------------------------------ what the family refuses
@pytest.mark.parametrize("name", NAMES)
def test_int8_is_refused(name):
    from janus_amd.services.transcriber import WhisperModel
    with pytest.raises(NotImplementedError, match=f"int8 encoder compute on {name}"):
        WhisperModel(name, compute_type="int8", apply_compute_type=True)
    with pytest.raises(NotImplementedError, match="4096"):
        jw.WhisperEngine(CONFIGS[name], weights={}, encoder_compute="int8")
    jw.check_encoder_compute(CONFIGS[name], "float16")
    jw.check_encoder_compute(CONFIGS["small.en"], "int8")        # the 768-wide models keep int8


@pytest.mark.parametrize("name", NAMES)
def test_second_tier_by_name(name):
    """Before any engine is touched: beam search refused naming the model, word timestamps NOT
    refused at 1024 (the stub engine is reached instead; medium.en with a named alignment set,
    its default one exceeds the alignment pass's 64 heads) and still refused at 1280."""
    from janus_amd.services.transcriber import generate_segments
    heads = None if name == "distil-medium.en" else [(23, h) for h in range(16)]
    eng = types.SimpleNamespace(cfg=CONFIGS[name], alignment_heads=heads)
    audio = [np.zeros(16000, np.float32)]
    with pytest.raises(NotImplementedError, match=f"beam_size 4 on {name}: the 1024-wide"):
        generate_segments(eng, audio, beam_size=4)
    jw.check_family_features(CONFIGS[name], beam_size=1, word_timestamps=True, alignment_heads=heads)
    with pytest.raises(AttributeError):          # past the refusals: the stub has no tokenizer
        generate_segments(eng, audio, word_timestamps=True)
    with pytest.raises(NotImplementedError, match="word_timestamps on large-v3-turbo"):
        generate_segments(types.SimpleNamespace(cfg=CONFIGS["large-v3-turbo"]), audio, word_timestamps=True)
    with pytest.raises(NotImplementedError, match="beam_size 2 on large-v3: the 1280-wide"):
        jw.check_family_features(CONFIGS["large-v3"], beam_size=2)
    jw.check_family_features(CONFIGS["small.en"], beam_size=5, word_timestamps=True)   # unchanged below


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_and_streaming_refuse_by_name(name):
    from janus_amd.pipeline import JanusPipeline
    from janus_amd.streaming import StreamingEncoder
    with pytest.raises(NotImplementedError, match=f"JanusPipeline.*1024-wide '{name}'"):
        JanusPipeline(model=name)
    eng = types.SimpleNamespace(cfg=CONFIGS[name], tokenizer=tok.WhisperTokenizer())
    with pytest.raises(NotImplementedError, match=f"StreamingEncoder.*1024-wide '{name}'"):
        StreamingEncoder(2, eng)
