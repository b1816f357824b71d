"""The large-v3 family (large-v3, large-v3-turbo, distil-large-v3) on the host: the 51 866-id
token layout, the configs, the checkpoint loader's checks, the packed 128-bin mel filters,
the decode planner at d_model 1280 / 20 heads and the features the family refuses by name."""
import types

import numpy as np
import pytest

import large_family_ref as lf
import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd import whisper as jw
from janus_amd.whisper import (CONFIGS, DEC_PATH_CVP, DEC_PATH_LN_FUSE, DEC_PATH_NO_CVP, DEC_PATH_NO_EMBED_LN,
                               DEC_PATH_RESID_LN, DEC_PATH_XGROUP, WhisperConfig, dec_path_ln_mask,
                               dec_path_xrows)

CUT = lf.CUT


# ------------------------------------------------------------------ token space
def test_v3_layout_ids():
    tk = tok.WhisperTokenizer(n_vocab=tok.N_VOCAB_V3)
    assert tok.N_VOCAB_V3 == 51866 and tk.n_vocab == 51866 and tk.multilingual
    assert (tk.eot, tk.sot, tk.language_begin) == (50257, 50258, 50259)
    assert (tk.translate, tk.transcribe, tk.sot_lm, tk.sot_prev) == (50359, 50360, 50361, 50362)
    assert (tk.no_speech, tk.no_timestamps, tk.timestamp_begin) == (50363, 50364, 50365)
    assert tk.timestamp_begin + 1501 == tk.n_vocab
    assert tk.n_languages == 100 and tk.languages[:99] == tok.LANGUAGES and tk.languages[-1] == "yue"
    assert tk.supported_languages() == tok.LANGUAGES + ["yue"]
    assert tk.language_token("en") == 50259 and tk.language_token("su") == 50357
    assert tk.language_token("yue") == 50358 and tk.language_code(50358) == "yue"
    assert tk.sot_sequence_for("yue", "translate") == [50258, 50358, 50359]
    assert tk.sot_sequence == [50258, 50259, 50360]
    with pytest.raises(ValueError):
        tk.language_code(50359)
    with pytest.raises(ValueError):
        tk.language_token("xx")
    sup = tk.suppress_tokens()
    assert {50258, 50359, 50360, 50361, 50362} <= set(sup)
    assert not {50257, 50363, 50364, 50358} & set(sup)
    # the text table is the multilingual one (the same 50 257 BPE ids)
    ml = tok.WhisperTokenizer(multilingual=True)
    assert tk.decode([300, 5000, 50256]) == ml.decode([300, 5000, 50256])
    with pytest.raises(ValueError):
        tok.WhisperTokenizer(n_vocab=51867)


def test_older_layouts_unchanged():
    en = tok.WhisperTokenizer()
    assert (en.eot, en.sot, en.translate, en.transcribe, en.sot_lm, en.sot_prev, en.no_speech,
            en.no_timestamps, en.timestamp_begin, en.n_vocab) == \
        (50256, 50257, 50357, 50358, 50359, 50360, 50361, 50362, 50363, 51864)
    assert en.sot_sequence == [50257] and not en.multilingual and en.supported_languages() == ["en"]
    ml = tok.WhisperTokenizer(multilingual=True)
    assert (ml.eot, ml.sot, ml.translate, ml.transcribe, ml.sot_lm, ml.sot_prev, ml.no_speech,
            ml.no_timestamps, ml.timestamp_begin, ml.n_vocab) == \
        (50257, 50258, 50358, 50359, 50360, 50361, 50362, 50363, 50364, 51865)
    assert ml.n_languages == 99 and ml.languages == tok.LANGUAGES and len(tok.LANGUAGES) == 99
    assert "yue" not in tok.LANGUAGES
    with pytest.raises(ValueError):
        ml.language_token("yue")
    assert ml.sot_sequence_for("su", "translate") == [50258, 50357, 50358]
    for nv, ref in ((51864, en), (51865, ml)):
        t = tok.WhisperTokenizer(n_vocab=nv)
        assert (t.sot_sequence, t.suppress_tokens(), t.timestamp_begin) == \
            (ref.sot_sequence, ref.suppress_tokens(), ref.timestamp_begin)
    assert tok.load_tokenizer(multilingual=True).n_vocab == 51865 and tok.load_tokenizer().n_vocab == 51864
    assert tok.load_tokenizer(n_vocab=51866).timestamp_begin == 50365
    # a cut vocabulary (test models) keeps the *.en ids
    assert tok.load_tokenizer(n_vocab=64).timestamp_begin == 50363 and tok.layout_vocab(51865) == 51865


# ------------------------------------------------------------------ configs
def test_configs_and_alias():
    for name, enc, dec in (("large-v3", 32, 32), ("large-v3-turbo", 32, 4), ("distil-large-v3", 32, 2)):
        c = CONFIGS[name]
        assert (c.name, c.d_model, c.n_heads, c.enc_layers, c.dec_layers) == (name, 1280, 20, enc, dec)
        assert (c.n_mels, c.n_vocab, c.n_audio_ctx, c.ffn, c.multilingual) == (128, 51866, 1500, 5120, True)
        assert jw.large_family(c) and not jw.shared_rows_in_place(c)
    assert jw.resolve_model("turbo") == "large-v3-turbo" and jw.resolve_model("base.en") == "base.en"
    with pytest.raises(ValueError, match="unknown model"):
        jw.resolve_model("medium")
    assert not jw.large_family(CONFIGS["small"]) and CONFIGS["small"].n_mels == 80


def test_supported_languages_per_layout():
    from janus_amd.services.transcriber import WhisperModel

    def model(nv):
        m = WhisperModel.__new__(WhisperModel)    # (no engine: the property reads the tokenizer alone)
        m.engine = types.SimpleNamespace(tokenizer=tok.WhisperTokenizer(n_vocab=nv))
        return m
    assert len(model(51866).supported_languages) == 100 and model(51866).supported_languages[-1] == "yue"
    assert model(51865).supported_languages == tok.LANGUAGES
    assert model(51864).supported_languages == ["en"]


def test_vote_language_uses_the_layouts_codes():
    from janus_amd.services.transcriber import _Stream
    tk = tok.WhisperTokenizer(n_vocab=51866)
    st = _Stream(np.zeros(16000, np.float32))
    p = np.full(100, 0.001)
    p[99] = 0.901
    st.language_pending = True
    st.vote_language(tk, p, 1, 0.5, last=True)
    assert st.language == "yue" and len(st.all_language_probs) == 100


# ------------------------------------------------------------------ loader
TINY_V3 = WhisperConfig("large-v3-turbo", 64, 1, 2, 1, n_mels=128, n_vocab=tok.N_VOCAB_V3, n_audio_ctx=8,
                        n_text_ctx=8)


def _save(path, W, drop=()):
    from safetensors.numpy import save_file
    sd = {"model." + k: np.ascontiguousarray(v) for k, v in W.items() if k not in drop}
    save_file(sd, str(path / "model.safetensors"))


def test_loader_checks_stem_and_depth(tmp_path, monkeypatch):
    """conv1.weight [d][128][3], encoder and decoder depth apart: a file of another depth under
    this name is refused by name and count (shapes cut to d = 64 so the file stays small)."""
    cfg = TINY_V3
    W = jw.synthetic_weights(cfg, seed=1)
    _save(tmp_path, W)
    monkeypatch.setenv("JANUS_WHISPER_DIR", str(tmp_path))
    got = jw.load_weights(cfg)
    assert got["encoder.conv1.weight"].shape == (64, 128, 3)
    # 80-bin stem under a 128-bin name
    bad = dict(W)
    bad["encoder.conv1.weight"] = W["encoder.conv1.weight"][:, :80].copy()
    _save(tmp_path, bad)
    with pytest.raises(ValueError, match=r"large-v3-turbo.*conv1\.weight.*\(64, 80, 3\)"):
        jw.load_weights(cfg)
    # a 1-layer decoder file under a name whose config has 2 decoder layers / 3 encoder layers
    _save(tmp_path, W)
    import dataclasses
    with pytest.raises(ValueError, match="large-v3.*1 decoder layers, the config has 2"):
        jw.load_weights(dataclasses.replace(cfg, name="large-v3", dec_layers=2))
    with pytest.raises(ValueError, match="2 encoder layers, the config has 3"):
        jw.load_weights(dataclasses.replace(cfg, enc_layers=3))


def test_tokenizer_json_special_ids(tmp_path):
    """The large-v3 layout's ids are checked against a tokenizer.json: a 99-language file
    (every id past the languages one lower) is refused."""
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, models

    def write(specials):
        t = Tokenizer(models.WordLevel({"a": 0}, unk_token="a"))
        vocab = {"a": 0}
        vocab.update(specials)
        t = Tokenizer(models.WordLevel(vocab, unk_token="a"))
        t.save(str(tmp_path / "tokenizer.json"))
    v3 = {"<|endoftext|>": 50257, "<|startoftranscript|>": 50258, "<|yue|>": 50358, "<|translate|>": 50359,
          "<|transcribe|>": 50360, "<|startofprev|>": 50362, "<|nospeech|>": 50363, "<|notimestamps|>": 50364,
          "<|0.00|>": 50365}
    write(v3)
    tk = tok.WhisperTokenizer(str(tmp_path), n_vocab=51866)
    assert tk.timestamp_begin == 50365
    v2 = {"<|endoftext|>": 50257, "<|startoftranscript|>": 50258, "<|translate|>": 50358,
          "<|transcribe|>": 50359, "<|startofprev|>": 50361, "<|nospeech|>": 50362, "<|notimestamps|>": 50363,
          "<|0.00|>": 50364}
    write(v2)
    with pytest.raises(ValueError, match="large-v3 layout"):
        tok.WhisperTokenizer(str(tmp_path), n_vocab=51866)
    tok.WhisperTokenizer(str(tmp_path), n_vocab=51865)      # the file's own layout loads


# ------------------------------------------------------------------ mel filters
def test_packed_mel_filters():
    basis, f128 = jw.mel_constants(128)
    assert basis.shape == (400, 416) and f128.shape == (208, 128) and f128.dtype == np.float32
    assert np.array_equal(f128[:201], jw.mel_filters(n_mels=128)) and not f128[201:].any()
    assert (f128[:201].sum(0) > 0).all()          # every one of the 128 filters reaches a bin
    b80, f80 = jw.mel_constants()
    assert np.array_equal(b80, basis) and f80.shape == (208, 80)
    assert np.array_equal(f80[:201], jw.mel_filters()) and not f80[201:].any()
    assert np.array_equal(jw.mel_constants(80)[1], f80)
    with pytest.raises(ValueError):
        jw.mel_constants(100)


# ------------------------------------------------------------------ the planner at 1280 / 20
def test_plan_launch_path_and_persistent(native_lib):
    p = lf.describe(native_lib, CUT, 8)
    assert p["wide"] == "1" and p["xabs"] == "1" and p["persist"] == "0" and p["call.enc_rows"] == "0"
    # every fusion guarded by d <= 512 is off
    assert (p["ln_pro_mask"], p["embed_ln"], p["cvp"], p["rln"], p["ln_fuse"]) == ("0", "0", "0", "0", "0")
    q = lf.describe(native_lib, CUT, 8, persistent=2)
    assert q["persist"] == "0" and q["xrev"] == "0"
    for full in ("large-v3", "large-v3-turbo", "distil-large-v3"):
        assert lf.describe(native_lib, CONFIGS[full], 64, persistent=3)["persist"] == "0"


def test_plan_shared_rows_are_gathered(native_lib):
    ei = [0] * 5 + [1] * 5
    p = lf.describe(native_lib, CUT, 10, enc_index=ei, temperature=0.6)
    assert p["call.enc_rows"] == "2" and p["pairs"] == "" and p["groups"] == ""   # JANUS_ENC_ROWS_GATHERED
    assert (p["npairs"], p["ngroups"], p["call.n_enc"], p["sampling"]) == ("0", "0", "10", "1")


@pytest.mark.parametrize("flags,match", [(dec_path_xrows(2), "12 heads"), (dec_path_xrows(4), "12 heads"),
                                         (DEC_PATH_XGROUP, "H <= 8")], ids=["xrows2", "xrows4", "xgroup"])
def test_plan_refuses_shared_row_blocks_by_head_limit(native_lib, flags, match):
    with pytest.raises(nat.JanusNativeError, match=match):
        lf.describe(native_lib, CUT, 4, enc_index=[0, 0, 0, 1], path_flags=flags)


@pytest.mark.parametrize("flags", [DEC_PATH_NO_CVP, DEC_PATH_CVP, DEC_PATH_NO_EMBED_LN, DEC_PATH_LN_FUSE,
                                   DEC_PATH_RESID_LN, dec_path_ln_mask(15)])
def test_plan_fusion_flags_change_nothing(native_lib, flags):
    a = lf.describe(native_lib, CUT, 8)
    b = lf.describe(native_lib, CUT, 8, path_flags=flags)
    assert a == b


def test_plan_refuses_beam_at_1280(native_lib):
    with pytest.raises(nat.JanusNativeError, match="d_model <= 768"):
        lf.describe(native_lib, CUT, 8, beam_size=4, enc_index=[0] * 4 + [1] * 4)


def test_plan_512_description_unchanged(native_lib):
    """The committed descriptions of the 384 / 512 / 768 plans, loaded and compared."""
    gold = mr.golden_plans()
    names = [n for n in mr.PLAN_CASES if n in gold]
    assert "default_base_4" in names and "default_small_8" in names
    for n in names:
        text, key = mr.describe_plan(native_lib, n)
        lines = text.splitlines()
        lines.remove("no_speech_back=0")      # (the field the golden file predates; its own test covers it)
        assert lines == gold[n]["text"].splitlines(), n


# ------------------------------------------------------------------ what the family refuses
@pytest.mark.parametrize("name", ["large-v3", "turbo", "distil-large-v3"])
def test_int8_is_refused(name):
    from janus_amd.services.transcriber import WhisperModel
    with pytest.raises(NotImplementedError, match="int8"):
        WhisperModel(name, compute_type="int8", apply_compute_type=True)
    cfg = CONFIGS[jw.resolve_model(name)]
    with pytest.raises(NotImplementedError, match="5120"):
        jw.WhisperEngine(cfg, weights={}, encoder_compute="int8")
    jw.check_encoder_compute(CONFIGS["small"], "int8")        # the 768-wide models keep int8
    jw.check_encoder_compute(cfg, "float16")


def test_second_tier_is_refused_by_name():
    from janus_amd.services.transcriber import generate_segments
    eng = types.SimpleNamespace(cfg=CONFIGS["large-v3-turbo"])
    audio = [np.zeros(16000, np.float32)]
    with pytest.raises(NotImplementedError, match="beam_size 4 on large-v3-turbo"):
        generate_segments(eng, audio, beam_size=4)
    with pytest.raises(NotImplementedError, match="word_timestamps on large-v3-turbo"):
        generate_segments(eng, audio, word_timestamps=True)
    jw.check_family_features(CONFIGS["small"], beam_size=5, word_timestamps=True)   # unchanged below 1280
    jw.check_family_features(CONFIGS["large-v3"], beam_size=1)
