"""The multilingual models' host side, no GPU: the token space (ids, start sequences, the
synthetic table, the suppress list, the unicode word split), the decode planner with
janus_decode_rows.no_speech_back (through janus_decode_plan_describe), the seek loop's
language handling on a recording stub engine and WhisperModel's argument errors."""
import json
import os
import re

import numpy as np
import pytest
import torch

import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd import whisper as jw
from janus_amd.services import transcriber as tr

LANGS = ("en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur "
         "hr bg lt la mi ml cy sk te fa lv bn sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si "
         "km sn yo so af oc ka be tg sd gu am yi lo uz fo ht ps tk nn mt sa lb my bo tl mg as tt haw ln ha "
         "ba jw su").split()


# --------------------------------------------------------------------------- token space
def test_multilingual_ids():
    t = tok.WhisperTokenizer(multilingual=True)
    assert (t.eot, t.sot, t.language_begin, t.n_languages) == (50257, 50258, 50259, 99)
    assert (t.translate, t.transcribe, t.sot_lm, t.sot_prev) == (50358, 50359, 50360, 50361)
    assert (t.no_speech, t.no_timestamps, t.timestamp_begin) == (50362, 50363, 50364)
    assert (t.n_vocab, t.blank, t.multilingual) == (51865, 220, True)
    assert t.language_begin + t.n_languages - 1 == 50357
    assert list(tok.LANGUAGES) == LANGS and len(set(LANGS)) == 99
    for i, code in enumerate(LANGS):
        assert t.language_token(code) == 50259 + i and t.language_code(50259 + i) == code
    assert t.sot_sequence == [50258, 50259, 50359]
    assert t.sot_sequence_for("de", "transcribe") == [50258, 50261, 50359]
    assert t.sot_sequence_for("ja", "translate") == [50258, 50266, 50358]
    assert t.sot_sequence_for("su", "translate") == [50258, 50357, 50358]
    assert tok.WhisperTokenizer(multilingual=True, language="fr", task="translate").sot_sequence == [50258, 50265, 50358]
    for bad in ("xx", "EN", None, 3):
        with pytest.raises(ValueError, match="language"):
            t.language_token(bad)
    with pytest.raises(ValueError, match="task"):
        t.sot_sequence_for("en", "summarise")
    with pytest.raises(ValueError):
        t.language_code(50258)
    with pytest.raises(ValueError):
        t.language_code(50358)
    assert jw.CONFIGS["tiny"].n_vocab == 51865 and jw.CONFIGS["tiny"].multilingual
    for name in ("tiny", "base", "small"):
        a, b = jw.CONFIGS[name], jw.CONFIGS[name + ".en"]
        assert (a.d_model, a.n_heads, a.enc_layers, a.dec_layers) == (b.d_model, b.n_heads, b.enc_layers, b.dec_layers)
        assert a.multilingual and not b.multilingual and b.n_vocab == 51864
    assert jw.default_alignment_heads(jw.CONFIGS["base"]) == jw.default_alignment_heads(jw.CONFIGS["base.en"])


def test_english_tokenizer_is_unchanged():
    t = tok.WhisperTokenizer()
    assert (t.eot, t.sot, t.translate, t.transcribe, t.sot_lm, t.sot_prev, t.no_speech, t.no_timestamps,
            t.timestamp_begin, t.blank) == (50256, 50257, 50357, 50358, 50359, 50360, 50361, 50362, 50363, 220)
    assert (tok.EOT, tok.SOT, tok.TRANSLATE, tok.TRANSCRIBE, tok.SOT_LM, tok.SOT_PREV, tok.NO_SPEECH,
            tok.NO_TIMESTAMPS, tok.TIMESTAMP_BEGIN, tok.N_VOCAB_EN, tok.BLANK) == (
        50256, 50257, 50357, 50358, 50359, 50360, 50361, 50362, 50363, 51864, 220)
    assert t.sot_sequence == [50257] and t.sot_sequence_for("en", "transcribe") == [50257]
    assert not t.multilingual and t.n_vocab == 51864 and len(t._table) == 50256
    assert (t.language_begin, t.n_languages) == (50258, 99)
    assert tok.load_tokenizer().sot_sequence == [50257]
    # the table is the seeded one of before: its first and last pseudo-words, and a checksum
    import zlib
    assert zlib.crc32(b"\x00".join(t._table)) == zlib.crc32(b"\x00".join(tok.WhisperTokenizer._synthetic_table(1234)))
    assert t.decode([220, 256, 50255, 50256, 50300]) == (b" " + t._table[256] + t._table[50255]).decode()
    assert t.suppress_tokens() == sorted(set(t.non_speech_tokens()) | {50358, 50357, 50257, 50360, 50359})


def test_tables_share_their_first_50256_ids():
    en, ml = tok.WhisperTokenizer(), tok.WhisperTokenizer(multilingual=True)
    assert len(ml._table) == 50257 and ml._table[:50256] == en._table
    assert ml._table[50256] and ml._table[50256].strip().isalpha()
    ids = [0, 220, 255, 256, 1234, 50255]
    assert ml.decode(ids) == en.decode(ids)
    assert ml.decode([50256]) == ml._table[50256].decode()     # a text token there, eot on *.en
    assert en.decode([50256]) == "" and ml.decode([50257, 50258, 50300]) == ""
    assert ml.encode_text("a b") == en.encode_text("a b")


def test_suppress_list_follows_the_ids():
    ml = tok.WhisperTokenizer(multilingual=True)
    s = ml.suppress_tokens()
    assert s == sorted(set(ml.non_speech_tokens()) | {ml.transcribe, ml.translate, ml.sot, ml.sot_prev, ml.sot_lm})
    assert {50359, 50358, 50258, 50361, 50360} <= set(s)
    assert not set(range(50259, 50358)) & set(s)            # no language token
    assert not {ml.eot, ml.no_speech, ml.no_timestamps, ml.timestamp_begin} & set(s)
    assert ml.non_speech_tokens() == tok.WhisperTokenizer().non_speech_tokens()


def test_unicode_only_word_split():
    """zh (and ja th lo my yue): the unicode pieces are the words; a character split over two
    tokens stays one piece; other languages (and None) merge pieces without a leading space."""
    t = tok.WhisperTokenizer(multilingual=True)
    b = "你".encode()                                          # 3 bytes
    inv = {byte: k for k, byte in enumerate(tok.bytes_to_unicode_order())}
    one = [inv[b[0]], inv[b[1]], inv[b[2]]]
    a, c = t.encode_text("a")[0], t.encode_text("c")[0]
    tokens = [a] + one + [c, t.eot]
    words, wt = t.split_to_word_tokens(tokens, language="zh")
    assert words == ["a", "你", "c", ""] and wt == [[a], one, [c], [t.eot]]
    for lang in ("ja", "th", "lo", "my", "yue"):
        assert t.split_to_word_tokens(tokens, language=lang) == (words, wt)
    for lang in (None, "en", "de"):
        w2, wt2 = t.split_to_word_tokens(tokens, language=lang) if lang else t.split_to_word_tokens(tokens)
        assert w2 == ["a你c", ""] and wt2 == [[a] + one + [c], [t.eot]]
    en = tok.WhisperTokenizer()
    assert en.split_to_word_tokens([a] + one + [c, en.eot]) == (["a你c", ""], [[a] + one + [c], [en.eot]])


def test_tokenizer_json_ids_are_checked(tmp_path):
    pytest.importorskip("tokenizers")

    def write(dirname, specials):
        d = tmp_path / dirname
        d.mkdir()
        # a stub file: a word-level model whose vocabulary holds the special tokens at their ids
        js = dict(version="1.0", truncation=None, padding=None, added_tokens=[], normalizer=None,
                  pre_tokenizer=None, post_processor=None, decoder=None,
                  model=dict(type="WordLevel", vocab=dict({"a": 0}, **specials), unk_token="a"))
        (d / "tokenizer.json").write_text(json.dumps(js))
        return str(d)
    ml = {"<|endoftext|>": 50257, "<|startoftranscript|>": 50258, "<|startofprev|>": 50361,
          "<|notimestamps|>": 50363, "<|0.00|>": 50364}
    en = {"<|endoftext|>": 50256, "<|startoftranscript|>": 50257, "<|startofprev|>": 50360,
          "<|notimestamps|>": 50362, "<|0.00|>": 50363}
    assert tok.WhisperTokenizer(write("ml", ml), multilingual=True).sot == 50258
    assert tok.WhisperTokenizer(write("en", en)).sot == 50257
    with pytest.raises(ValueError, match="multilingual layout"):
        tok.WhisperTokenizer(write("en2", en), multilingual=True)
    with pytest.raises(ValueError, match=r"\*\.en layout"):
        tok.WhisperTokenizer(write("ml2", ml))
    with pytest.raises(ValueError, match="0.00"):
        tok.WhisperTokenizer(write("ml3", dict(ml, **{"<|0.00|>": 50365})), multilingual=True)


# --------------------------------------------------------------------------- the planner
@pytest.mark.parametrize("name", sorted(mr.PLAN_CASES))
def test_plan_without_no_speech_back_is_the_parents(native_lib, name):
    """no_speech_back 0: every line of the plan's description and every word of its graph key
    as the commit before the field printed them (tests/golden/plan_descriptions.json), plus
    the field's own line and key word, both 0."""
    want = mr.golden_plans()[name]
    text, key = mr.describe_plan(native_lib, name)
    lines = text.splitlines()
    assert "no_speech_back=0" in lines
    lines.remove("no_speech_back=0")
    assert lines == want["text"].splitlines()
    fields = [ln.split("=")[0] for ln in text.splitlines() if not ln.startswith(("call.", "pairs=", "groups="))]
    at = fields.index("no_speech_back")
    assert key[at] == 0 and list(key[:at] + key[at + 1:]) == want["key"]


def test_plan_with_no_speech_back(native_lib):
    base = jw.CONFIGS["base"]
    prompts = [mr.MULTI_PROMPT, [50361, 1, 2, 3] + mr.MULTI_PROMPT]                 # lengths {3, 7}
    t0, k0 = mr.describe(native_lib, base, 2, max_length=40, prompts=prompts)
    t2, k2 = mr.describe(native_lib, base, 2, max_length=40, prompts=prompts, no_speech_back=2)
    f0, f2 = mr.plan_fields(t0), mr.plan_fields(t2)
    assert (f0["sample_begin"], f0["no_speech_back"]) == ("3", "0")
    assert (f2["sample_begin"], f2["no_speech_back"]) == ("1", "2")
    assert {n for n in f0 if f0[n] != f2[n]} == {"sample_begin", "no_speech_back"}
    assert k0 != k2                                           # the graphs are not shared
    f1 = mr.plan_fields(mr.describe(native_lib, base, 2, max_length=40, prompts=prompts, no_speech_back=1)[0])
    assert f1["sample_begin"] == "2"
    # beam rows, shared rows and sampling plan it the same way
    fb = mr.plan_fields(mr.describe(native_lib, base, 4, max_length=40, prompts=[mr.MULTI_PROMPT] * 4, beam_size=2,
                                    enc_index=[0, 0, 1, 1], no_speech_back=2)[0])
    assert (fb["sample_begin"], fb["beam_k"], fb["no_speech_back"]) == ("1", "2", "2")
    fs = mr.plan_fields(mr.describe(native_lib, base, 2, max_length=40, prompts=prompts, temperature=0.4,
                                    no_speech_back=2)[0])
    assert (fs["sample_begin"], fs["sampling"]) == ("1", "1")
    # staggered: continuing rows sample from the first step on, as before; all fresh: as above
    fg = mr.plan_fields(mr.describe(native_lib, base, 2, max_length=40, prompts=prompts, pos_offset=[0, 0],
                                    no_speech_back=2)[0])
    assert fg["sample_begin"] == "1"
    fc = mr.plan_fields(mr.describe(native_lib, base, 2, max_length=40, prompts=prompts, pos_offset=[0, 9], steps=5,
                                    stand=[9, 9], stand_maxlen=40, no_speech_back=2)[0])
    assert fc["sample_begin"] == "0"
    # out of range: every row needs 0 <= no_speech_back < prompt_len
    for bad in (3, 7, -1):
        with pytest.raises(nat.JanusNativeError, match="no_speech_back"):
            mr.describe(native_lib, base, 2, max_length=40, prompts=prompts, no_speech_back=bad)
    with pytest.raises(nat.JanusNativeError, match="no_speech_back"):
        mr.describe(native_lib, base, 2, no_speech_back=2)    # the options' two-token prompt


def test_entries_declared():
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    api = open(os.path.join(inc, "janus.h")).read()
    kapi = open(os.path.join(inc, "janus_kernels.h")).read()
    assert re.search(r"\bint janus_whisper_detect_language\(", api) and "parity unpinned" in api
    assert re.search(r"int steps;.*?int no_speech_back;\s*\} janus_decode_rows;", api, re.S)
    assert re.search(r"\bint janus_lang_head_f16\(", kapi)
    assert len(nat.SIGNATURES["janus_whisper_detect_language"]) == 9
    assert len(nat.SIGNATURES["janus_lang_head_f16"]) == 11
    assert jw.janus_decode_rows._fields_[-1][0] == "no_speech_back"


def test_engine_checks_the_sot_position():
    e = jw.WhisperEngine.__new__(jw.WhisperEngine)
    e.tokenizer = tok.WhisperTokenizer(multilingual=True)
    assert e._no_speech_back(None, None) == 2
    assert e._no_speech_back(None, [[50258, 50261, 50359], [50361, 7, 50258, 50259, 50358]]) == 2
    assert e._no_speech_back(0, [[1, 50258]]) == 0
    for bad in ([[50258]], [[50258, 50259, 50359], [50258, 50259]], [[50259, 50258, 50359]]):
        with pytest.raises(ValueError, match="startoftranscript"):
            e._no_speech_back(None, bad)
    with pytest.raises(ValueError, match="no_speech_back"):
        e._no_speech_back(-1, None)
    e.tokenizer = tok.WhisperTokenizer()
    assert e._no_speech_back(None, None) == 0 and e._no_speech_back(None, [[50360, 5, 50257]]) == 0
    e.cfg = jw.CONFIGS["tiny.en"]
    with pytest.raises(ValueError, match="English-only"):
        e.detect_language(torch.zeros(1, 1500, 384, dtype=torch.float16))


# --------------------------------------------------------------------------- the seek loop
class _Out:
    def __init__(self, n):
        self.n_tokens = torch.zeros(n, dtype=torch.int32)
        self._n = n

    def rows(self):
        return [([], -0.5, 0.0)] * self._n


class _StubEngine:
    """Enough of WhisperEngine for generate_segments on the CPU, recording its calls: every
    window decodes to nothing and passes its gates (one window per 30 s); detect_language
    answers from ``script``: per call, one row of probabilities per window asked."""

    def __init__(self, multilingual=True, script=None):
        self.tokenizer = tok.load_tokenizer(multilingual=multilingual)
        self.device = torch.device("cpu")
        self.calls, self.detects, self.encodes = [], [], 0
        self.script = list(script or [])

    def logmel_frames(self, pcm, offs, batch, decim, frames):
        return torch.zeros(batch, frames, 80, dtype=torch.float16)

    def encode(self, mel):
        self.encodes += 1
        return torch.zeros(mel.shape[0], 1, 1, dtype=torch.float16)

    def decode_ex(self, enc, prompts=None, max_length=448, **kw):
        self.calls.append([list(p) for p in prompts])
        return _Out(len(prompts))

    def detect_language(self, enc):
        n = int(enc.shape[0])
        self.detects.append(n)
        rows = self.script.pop(0) if self.script else [one_hot("en", 0.9)] * n
        assert len(rows) == n
        p = torch.tensor(np.asarray(rows, np.float32))
        return p, p.argmax(1).to(torch.int32)


def one_hot(code, p, second=None):
    """99 probabilities: ``code`` at p, ``second`` (code, q) if given, the rest spread evenly."""
    out = np.zeros(99)
    rest = 1.0 - p - (second[1] if second else 0.0)
    out[:] = rest / (99 - 1 - (1 if second else 0))
    out[LANGS.index(code)] = p
    if second:
        out[LANGS.index(second[0])] = second[1]
    return out


SEC = 16000


def test_detection_runs_once_in_round_one():
    e = _StubEngine(script=[[one_hot("de", 0.8), one_hot("ja", 0.7), one_hot("en", 0.95)]])
    auds = [np.zeros(70 * SEC, np.float32), np.zeros(10 * SEC, np.float32), np.zeros(40 * SEC, np.float32)]
    st = tr.generate_segments(e, auds, temperatures=(0.0,))
    assert e.detects == [3]                                   # one call, round 1 only
    assert e.encodes == 3                                     # no extra encode: one per round
    assert [s.language for s in st] == ["de", "ja", "en"]
    assert [round(s.language_probability, 3) for s in st] == [0.8, 0.7, 0.95]
    assert e.calls[0] == [[50258, 50261, 50359], [50258, 50266, 50359], [50258, 50259, 50359]]
    assert e.calls[1] == [[50258, 50261, 50359], [50258, 50259, 50359]] and e.calls[2] == [[50258, 50261, 50359]]
    for s in st:
        assert len(s.all_language_probs) == 99 and abs(sum(p for _, p in s.all_language_probs) - 1) < 1e-6
        assert s.all_language_probs[0] == (s.language, pytest.approx(s.language_probability))
        ps = [p for _, p in s.all_language_probs]
        assert ps == sorted(ps, reverse=True)
    # translate: the task token follows each utterance's language
    e = _StubEngine(script=[[one_hot("fr", 0.6)]])
    tr.generate_segments(e, auds[1:2], task="translate", temperatures=(0.0,))
    assert e.calls == [[[50258, 50265, 50358]]]


def test_given_language_makes_no_detect_call():
    e = _StubEngine()
    auds = [np.zeros(10 * SEC, np.float32)] * 3
    st = tr.generate_segments(e, auds, language="es", temperatures=(0.0,))
    assert e.detects == [] and e.calls == [[[50258, 50262, 50359]] * 3]
    assert [(s.language, s.language_probability, s.all_language_probs) for s in st] == [("es", 1.0, None)] * 3
    # per utterance: a list, None entries detected alone
    e = _StubEngine(script=[[one_hot("ko", 0.9)]])
    st = tr.generate_segments(e, auds, language=["zh", None, "pt"], task="translate", temperatures=(0.0,))
    assert e.detects == [1]
    assert e.calls == [[[50258, 50260, 50358], [50258, 50264, 50358], [50258, 50267, 50358]]]
    assert [s.language for s in st] == ["zh", "ko", "pt"] and st[0].all_language_probs is None
    for bad in dict(language="xx"), dict(language=["en"]), dict(task="summarise"), dict(language_detection_segments=0):
        with pytest.raises(ValueError):
            tr.generate_segments(_StubEngine(), auds, **bad)


def test_threshold_segments_and_majority():
    long = [np.zeros(130 * SEC, np.float32)]                  # 5 windows
    # window 1 below the threshold, window 2 above: settled there, no further calls
    e = _StubEngine(script=[[one_hot("de", 0.4)], [one_hot("nl", 0.7)]])
    st = tr.generate_segments(e, long, language_detection_segments=4, temperatures=(0.0,))[0]
    assert e.detects == [1, 1] and (st.language, round(st.language_probability, 3)) == ("nl", 0.7)
    assert [c[0][1] for c in e.calls] == [50261] + [50271] * 4   # window 1 decoded with its own winner
    # never above: the majority of the winners of `segments` windows, its largest probability
    e = _StubEngine(script=[[one_hot("de", 0.3)], [one_hot("nl", 0.45)], [one_hot("nl", 0.35)], [one_hot("de", 0.2)]])
    st = tr.generate_segments(e, long, language_detection_segments=3, temperatures=(0.0,))[0]
    assert e.detects == [1, 1, 1] and (st.language, round(st.language_probability, 3)) == ("nl", 0.45)
    # a tie: the language seen first
    e = _StubEngine(script=[[one_hot("de", 0.3)], [one_hot("nl", 0.45)]])
    st = tr.generate_segments(e, long, language_detection_segments=2, temperatures=(0.0,))[0]
    assert e.detects == [1, 1] and (st.language, round(st.language_probability, 3)) == ("de", 0.3)
    # segments 1: the first window decides whatever its probability; the threshold is strict
    e = _StubEngine(script=[[one_hot("sv", 0.2)]])
    st = tr.generate_segments(e, long, temperatures=(0.0,))[0]
    assert e.detects == [1] and st.language == "sv"
    e = _StubEngine(script=[[one_hot("sv", 0.5)], [one_hot("fi", 0.9)]])
    st = tr.generate_segments(e, long, language_detection_segments=2, temperatures=(0.0,))[0]
    assert e.detects == [1, 1] and st.language == "fi"
    # the utterance ends before the count is reached: settled on what was seen
    e = _StubEngine(script=[[one_hot("it", 0.3)]])
    st = tr.generate_segments(e, [np.zeros(5 * SEC, np.float32)], language_detection_segments=4,
                              temperatures=(0.0,))[0]
    assert e.detects == [1] and st.language == "it" and not st.language_pending
    # two utterances undecided for different numbers of rounds: one call per round for those left
    e = _StubEngine(script=[[one_hot("de", 0.9), one_hot("ru", 0.2)], [one_hot("ru", 0.8)]])
    st = tr.generate_segments(e, long * 2, language_detection_segments=3, temperatures=(0.0,))
    assert e.detects == [2, 1] and [s.language for s in st] == ["de", "ru"]


def test_english_engine_detects_nothing():
    e = _StubEngine(multilingual=False)
    st = tr.generate_segments(e, [np.zeros(40 * SEC, np.float32)], temperatures=(0.0,))[0]
    assert e.detects == [] and e.calls == [[[50257]], [[50257]]]
    assert (st.language, st.language_probability, st.all_language_probs) == ("en", 1.0, None)
    # language / task are not looked at there (WhisperModel rejects them before)
    tr.generate_segments(e, [np.zeros(SEC, np.float32)], language="de", task="translate", temperatures=(0.0,))
    assert e.detects == [] and e.calls[-1] == [[50257]]


# --------------------------------------------------------------------------- WhisperModel
def _model(monkeypatch, name):
    class Engine(_StubEngine):
        def __init__(self, cfg, encoder_compute="float16"):
            super().__init__(multilingual=cfg.multilingual)
            self.cfg = cfg
    monkeypatch.setattr(tr, "WhisperEngine", Engine)
    return tr.WhisperModel(name)


def test_whisper_model_arguments(monkeypatch):
    audio = np.zeros(SEC, np.float32)
    en = _model(monkeypatch, "base.en")
    assert not en.is_multilingual and en.supported_languages == ["en"]
    for kw in ({}, dict(language="en"), dict(language=None)):
        segs, info = en.transcribe(audio, **kw)
        assert (info.language, info.language_probability, info.all_language_probs) == ("en", 1.0, None)
    for kw in (dict(language="de"), dict(task="translate"), dict(language="en", task="translate")):
        with pytest.raises(NotImplementedError, match=r"\*\.en models transcribe English only"):
            en.transcribe(audio, **kw)
    with pytest.raises(ValueError, match="English-only"):
        en.detect_language(audio)
    assert en.engine.detects == []
    for name in ("tiny", "base", "small"):
        assert _model(monkeypatch, name).is_multilingual
    ml = _model(monkeypatch, "base")
    assert ml.supported_languages == LANGS
    for kw in (dict(language="xx"), dict(language="english"), dict(task="summarise"),
               dict(language="de", task="Translate")):
        with pytest.raises(ValueError):
            ml.transcribe(audio, **kw)
    assert ml.engine.calls == [] and ml.engine.detects == []
    _, info = ml.transcribe(audio)                             # language=None: detected
    assert ml.engine.detects == [1] and (info.language, round(info.language_probability, 3)) == ("en", 0.9)
    assert len(info.all_language_probs) == 99 and info.all_language_probs[0][0] == "en"
    _, info = ml.transcribe(audio, language="de", task="translate")
    assert ml.engine.detects == [1] and ml.engine.calls[-1] == [[50258, 50261, 50358]]
    assert (info.language, info.language_probability, info.all_language_probs) == ("de", 1.0, None)
    ml.engine.script = [[one_hot("uk", 0.3, ("ru", 0.25)), one_hot("uk", 0.6)]]
    assert ml.detect_language(np.zeros(40 * SEC, np.float32), language_detection_segments=2)[:2] == (
        "uk", pytest.approx(0.6))
    with pytest.raises(ValueError, match="unknown model size"):
        tr.WhisperModel("medium")


def test_serving_paths_stay_english_only():
    from janus_amd.pipeline import JanusPipeline
    from janus_amd.streaming import StreamingEncoder
    for name in ("tiny", "base", "small"):
        with pytest.raises(NotImplementedError, match="English-only"):
            JanusPipeline(name)
    with pytest.raises(NotImplementedError, match="English-only"):
        StreamingEncoder(1, _StubEngine())
    # Transcriber's fixed language='en' is a given language on a multilingual model too
    import inspect
    assert "language='en'" in inspect.getsource(tr.Transcriber.transcribe_buffer)
