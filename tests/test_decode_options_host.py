"""The decoding options on the CPU: the planner's view of the history rules
(janus_decode_options.repetition_penalty / no_repeat_ngram_size), the three suppress_tokens forms,
argument errors, and the prompt assembly of generate_segments (initial_prompt, hotwords,
condition_on_previous_text, prompt_reset_on_temperature) over a three-window stream against
faster-whisper's get_prompt restated here. The reference of the rules themselves
(tests/history_ref.py) is checked on hand-worked examples."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import history_ref as hr
import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd import whisper as jw
from janus_amd.services import transcriber as tr

BASE, TINY, LARGE = jw.CONFIGS["base.en"], jw.CONFIGS["tiny.en"], jw.CONFIGS["large-v3"]


# ------------------------------------------------------------------ the rule's reference
def test_reference_bans():
    a, b, c, ts = 5, 17, 31, 50400
    assert hr.banned([a, a, a, a], 2) == [a]                     # overlapping matches
    assert hr.banned([a, a, a, a], 3) == [a]
    assert hr.banned([a, b, c, a, b], 3) == [c]
    assert hr.banned([a, b, c, a, b], 2) == [c]                  # ... b -> c seen before
    assert hr.banned([a, ts, b, a, ts], 3) == [b]                # a timestamp inside the n-gram
    assert hr.banned([a, b, c], 1) == [a, b, c]                  # n = 1: every sampled token
    assert hr.banned([a, b], 3) == [] and hr.banned([], 1) == [] and hr.banned([a, b, a], 0) == []
    assert hr.banned([a, b, a], 4) == []                         # m < n
    assert hr.banned([a, b, c, b, a, b], 2) == [a, c]            # every earlier continuation of b


def test_reference_penalty():
    L = np.array([2.0, -2.0, 0.5, -0.5, 1.0], np.float32)
    out = hr.penalise(L, [0, 1, 1, 0, 3], 2.0)                   # once per distinct token
    assert out.tolist() == [1.0, -4.0, 0.5, -1.0, 1.0] and out.dtype == np.float32
    assert hr.penalise(L, [], 2.0).tolist() == L.tolist()
    assert hr.penalise(L, [0, 1], 1.0).tolist() == L.tolist()


# ------------------------------------------------------------------ the planner
def describe(lib, cfg, B, p=None, n=None, persistent=0, max_length=448, temperature=0.0, beam_size=0,
             enc_index=None, pos_offset=None, steps=0, stand=None, stand_maxlen=0, prompts=None):
    """mr.describe with the options' two history fields (None: left untouched)."""
    c = jw.janus_whisper_config(cfg.n_mels, cfg.n_audio_ctx, cfg.d_model, cfg.n_heads,
                                cfg.enc_layers, cfg.dec_layers, cfg.n_vocab, cfg.n_text_ctx)
    keep = []

    def i32(values):
        a = np.ascontiguousarray(np.asarray(values, np.int32))
        keep.append(a)
        return a.ctypes.data_as(mr.I32P)
    opt = jw.janus_decode_options()
    opt.prompt = i32([50257, 50362])
    opt.prompt_len, opt.max_length, opt.eot = 2, max_length, 50256
    opt.suppress_blank, opt.blank_token = 1, 220
    opt.timestamp_begin, opt.no_timestamps, opt.max_initial_timestamp_index = 50363, 50362, 50
    opt.check_every, opt.persistent = 16, persistent
    rows = jw.janus_decode_rows()
    rows.no_speech_token = 50361
    if p is not None:
        opt.repetition_penalty = p
    if n is not None:
        opt.no_repeat_ngram_size = n
    if enc_index is not None:
        rows.enc_index = i32(enc_index)
        rows.n_enc = max(enc_index) + 1
    if pos_offset is not None:
        rows.pos_offset = i32(pos_offset)
        rows.steps = steps
    if prompts is not None:
        stride = max(len(q) for q in prompts)
        flat = np.zeros((B, stride), np.int32)
        for b, q in enumerate(prompts):
            flat[b, :len(q)] = q
        rows.prompts = i32(flat)
        rows.prompt_lens = i32([len(q) for q in prompts])
        rows.stride = stride
    st = np.ascontiguousarray(np.asarray(stand if stand is not None else [], np.int32))
    text = ctypes.create_string_buffer(1 << 16)
    key = (ctypes.c_int64 * 256)()
    n_key = ctypes.c_int32(0)
    nat.check(lib.janus_decode_plan_describe(
        ctypes.addressof(c), ctypes.addressof(opt), ctypes.addressof(rows), B, 256, 1, 0,
        ctypes.c_float(temperature), None, beam_size, st.ctypes.data if st.size else None, int(st.size),
        stand_maxlen, ctypes.addressof(text), len(text), ctypes.addressof(key), len(key),
        ctypes.addressof(n_key)))
    del keep
    return text.value.decode(), tuple(key[:n_key.value])


@pytest.mark.parametrize("name", sorted(mr.PLAN_CASES))
def test_plan_with_the_rules_off_is_the_committed_one(native_lib, name):
    """p = 0 (a zeroed struct), p = 1 and n = 0: the description and the graph key of the call
    without the fields, i.e. the committed golden plan (the no_speech_back line aside, as
    tests/test_multilingual_host.py reads it)."""
    model, B, kw = mr.PLAN_CASES[name]
    want_text, want_key = mr.describe_plan(native_lib, name)
    golden = mr.golden_plans()[name]["text"].splitlines()
    for p, n in ((None, None), (0.0, 0), (1.0, 0)):
        text, key = describe(native_lib, jw.CONFIGS[model], B, p, n, **kw)
        assert text == want_text and key == want_key
        assert [ln for ln in text.splitlines() if ln != "no_speech_back=0"] == golden
        assert "repetition_penalty" not in text and "no_repeat_ngram_size" not in text


def test_plan_shows_the_rules_when_set(native_lib):
    off_text, off_key = describe(native_lib, BASE, 64)
    text, key = describe(native_lib, BASE, 64, 1.2, 3)
    lines = text.splitlines()
    assert "repetition_penalty=1.2" in lines and "no_repeat_ngram_size=3" in lines
    assert lines.index("no_repeat_ngram_size=3") + 1 == [i for i, ln in enumerate(lines) if ln.startswith("pairs=")][0]
    assert [ln for ln in lines if not ln.startswith(("repetition_penalty=", "no_repeat_ngram_size="))] == \
        off_text.splitlines()
    assert len(key) == len(off_key) + 2 and key[:len(off_key)] == off_key and key[-1] == 3
    assert key[-2] == int(np.float32(1.2).view(np.uint32))
    # each of the two alone, and different values, are different graphs
    keys = {describe(native_lib, BASE, 64, p, n)[1] for p, n in ((1.2, 3), (1.2, 0), (1.0, 3), (1.3, 3), (1.2, 2))}
    assert len(keys) == 5 and off_key not in keys
    assert "repetition_penalty=1\n" in describe(native_lib, BASE, 64, 1.0, 2)[0]
    # sampled, per-row prompts and shared encoder rows take them
    t, _ = describe(native_lib, TINY, 10, 1.3, 0, temperature=0.6, enc_index=[0] * 5 + [1] * 5)
    assert "repetition_penalty=1.3" in t and "npairs=6" in t
    t, _ = describe(native_lib, LARGE, 33, 1.0, 2)
    assert "no_repeat_ngram_size=2" in t


def test_persistent_request_with_rules_plans_level_0(native_lib):
    f = mr.plan_fields(describe(native_lib, BASE, 8, persistent=2)[0])
    assert f["persist"] == "2"
    for p, n in ((1.2, 0), (1.0, 3)):
        f = mr.plan_fields(describe(native_lib, BASE, 8, p, n, persistent=2)[0])
        assert f["persist"] == "0" and f["seg_grid"] == "0"


def test_refusals_arrive_by_name(native_lib):
    beam = dict(beam_size=4, prompts=[[50257, 50362]] * 8, enc_index=[0] * 4 + [1] * 4)
    stagger = dict(max_length=40, pos_offset=[0, 0, 20, 20], steps=19, stand=[20] * 4, stand_maxlen=40)
    for p, n in ((1.3, 0), (1.0, 2)):
        with pytest.raises(nat.JanusNativeError, match="beam search takes no repetition_penalty / no_repeat_ngram_size"):
            describe(native_lib, BASE, 8, p, n, **beam)
        with pytest.raises(nat.JanusNativeError, match=r"staggered rows \(pos_offset\) take no repetition_penalty"):
            describe(native_lib, BASE, 4, p, n, **stagger)
    describe(native_lib, BASE, 8, 1.0, 0, **beam)                # off: both still plan
    describe(native_lib, BASE, 4, 0.0, 0, **stagger)
    with pytest.raises(nat.JanusNativeError, match="repetition_penalty must be > 0"):
        describe(native_lib, BASE, 4, -0.5, 0)
    with pytest.raises(nat.JanusNativeError, match="repetition_penalty must be > 0"):
        describe(native_lib, BASE, 4, float("nan"), 0)
    with pytest.raises(nat.JanusNativeError, match="no_repeat_ngram_size must be >= 0"):
        describe(native_lib, BASE, 4, 1.0, -1)


# ------------------------------------------------------------------ engine arguments
def test_suppress_tokens_forms():
    tk = tok.WhisperTokenizer()
    V = tok.N_VOCAB_EN
    default = tk.suppress_tokens()
    five = [tk.transcribe, tk.translate, tk.sot, tk.sot_prev, tk.sot_lm]
    assert jw.resolve_suppress_tokens(tk, None, V) == default
    assert jw.resolve_suppress_tokens(tk, [-1], V) == default
    extra = [t for t in (11, 500, 40000) if t not in default]
    assert extra
    assert jw.resolve_suppress_tokens(tk, [-1] + extra, V) == sorted(set(default) | set(extra))
    assert jw.resolve_suppress_tokens(tk, [500, 11, 500], V) == sorted({11, 500} | set(five))
    assert jw.resolve_suppress_tokens(tk, [], V) == sorted(five)
    assert jw.resolve_suppress_tokens(tk, (-1,), V) == default
    for bad in ([V], [-2], [5, V + 7]):
        with pytest.raises(ValueError, match="outside the vocabulary"):
            jw.resolve_suppress_tokens(tk, bad, V)


def test_engine_options_carry_the_suppress_list():
    e = jw.WhisperEngine.__new__(jw.WhisperEngine)
    e.tokenizer, e.cfg = tok.WhisperTokenizer(), TINY
    opt, keep = e.decode_options()
    assert list(keep[1]) == e.tokenizer.suppress_tokens() and opt.n_suppress == len(keep[1])
    opt, keep = e.decode_options(suppress_tokens=[7, 9])
    assert list(keep[1]) == jw.resolve_suppress_tokens(e.tokenizer, [7, 9], TINY.n_vocab) and opt.n_suppress == 7
    with pytest.raises(ValueError, match="outside the vocabulary"):
        e.decode_options(suppress_tokens=[10 ** 6])


def test_argument_errors_before_any_gpu_work():
    for p in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="repetition_penalty"):
            jw.check_history_args(p, 0)
    for n in (-1, 2.5):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            jw.check_history_args(1.0, n)
    jw.check_history_args(1.0, 0, beam_size=5)
    for p, n in ((1.3, 0), (1, 3)):
        with pytest.raises(NotImplementedError, match="repetition_penalty / no_repeat_ngram_size.*beam"):
            jw.check_history_args(p, n, beam_size=5)
    e = _Engine([])
    aud = [np.zeros(SEC, np.float32)]
    with pytest.raises(NotImplementedError, match="repetition_penalty / no_repeat_ngram_size.*beam"):
        tr.generate_segments(e, aud, beam_size=5, repetition_penalty=1.2, temperatures=(0.0,))
    with pytest.raises(ValueError, match="repetition_penalty"):
        tr.generate_segments(e, aud, repetition_penalty=0, temperatures=(0.0,))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        tr.generate_segments(e, aud, suppress_tokens=[-1, 10 ** 6], temperatures=(0.0,))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        tr.generate_segments(e, aud, initial_prompt=[-3], temperatures=(0.0,))
    assert e.calls == [] and e.encodes == 0
    m = tr.WhisperModel.__new__(tr.WhisperModel)
    m.engine = e
    with pytest.raises(NotImplementedError, match="repetition_penalty / no_repeat_ngram_size.*beam"):
        m.transcribe(aud[0], beam_size=5, no_repeat_ngram_size=3)
    assert e.calls == [] and e.encodes == 0


# ------------------------------------------------------------------ the seek loop's prompts
SEC = 16000
TB = 50363           # <|0.00|> of the *.en layout
WINDOWS = [[TB, 1001, 1002, TB + 100], [TB, 2001, 2002, 2003, TB + 80], [TB, 3001, TB + 40]]


class _Out:
    def __init__(self, rows):
        self._rows = rows
        self.n_tokens = torch.tensor([len(r[0]) + 1 for r in rows], dtype=torch.int32)

    def rows(self):
        return self._rows


class _Engine:
    """Enough of WhisperEngine for generate_segments on the CPU: window k of the stream decodes
    to WINDOWS[k]; a T = 0 decode of a window listed in ``fail`` misses its log-probability
    gate, the sampled re-decode passes. Records every decode call's prompts and keywords."""

    def __init__(self, fail):
        self.tokenizer = tok.WhisperTokenizer()
        self.device = torch.device("cpu")
        self.cfg = TINY
        self.calls, self.kwargs, self.encodes, self.window, self.fail = [], [], 0, -1, set(fail)

    def logmel_frames(self, pcm, offs, batch, decim, frames):
        return torch.zeros(batch, frames, 80, dtype=torch.float16)

    def encode(self, mel):
        self.encodes += 1
        self.window += 1
        return torch.zeros(mel.shape[0], 1, 1, dtype=torch.float16)

    def decode_ex(self, enc, prompts=None, max_length=448, temperature=0.0, seeds=None, enc_index=None, **kw):
        self.calls.append([list(p) for p in prompts])
        self.kwargs.append(dict(kw, temperature=temperature))
        lp = -2.0 if (np.isscalar(temperature) and temperature == 0 and self.window in self.fail) else -0.5
        return _Out([(list(WINDOWS[self.window]), lp, 0.0)] * len(prompts))


def expected_prompts(tk, seed, hot, settled_temps, cond, reset_t, L):
    """faster-whisper's get_prompt / prompt_reset_since over the three windows, restated."""
    all_tokens, since, out = list(seed), 0, []
    for toks, T in zip(WINDOWS, settled_temps):
        prev, p = all_tokens[since:], []
        if prev or hot:
            p = [tk.sot_prev] + list(hot)[:L // 2 - 1] + prev[-(L // 2 - 1):]
        out.append(p + list(tk.sot_sequence))
        all_tokens += toks
        if not cond or T > reset_t:
            since = len(all_tokens)
    return out


PROMPTS = [None, "ba di", [400, 1200, 3300]]
HOTWORDS = [None, "zu ke mo", [9000, 262]]


@pytest.mark.parametrize("initial,hot,cond,reset_t", list(itertools.product(PROMPTS, HOTWORDS, [True, False],
                                                                             [0.5, 0.3])))
def test_prompt_assembly(initial, hot, cond, reset_t):
    """70 s = three windows; window 1's T = 0 decode fails its gate and settles at T = 0.4:
    above a reset temperature of 0.3, below the default 0.5."""
    e = _Engine(fail=[1])
    tk = e.tokenizer
    L = 64
    st = tr.generate_segments(e, [np.zeros(70 * SEC, np.float32)], max_length=L, temperatures=(0.0, 0.4),
                              initial_prompt=initial, hotwords=hot, condition_on_previous_text=cond,
                              prompt_reset_on_temperature=reset_t)[0]
    assert st.windows == 3 and [s.temperature for s in st.segments] == [0.0, 0.4, 0.0]

    def enc(x):
        return [] if x is None else (tk.encode_text(" " + x.strip()) if isinstance(x, str) else list(x))
    want = expected_prompts(tk, enc(initial), enc(hot), [0.0, 0.4, 0.0], cond, reset_t, L)
    t0 = [c[0] for c, k in zip(e.calls, e.kwargs) if np.isscalar(k["temperature"]) and k["temperature"] == 0]
    assert t0 == want
    sampled = [c for c, k in zip(e.calls, e.kwargs) if np.isscalar(k["temperature"]) and k["temperature"] > 0]
    assert sampled == [[want[1]] * tr.BEST_OF]                 # the fallback decodes the same prompt
    if initial is None and hot is None and cond and reset_t == 0.5:
        assert want[0] == list(tk.sot_sequence) and want[1][0] == tk.sot_prev


def test_long_prompts_are_cut_and_overlong_ones_refused():
    e = _Engine([])
    tk = e.tokenizer
    L = 16                                                      # max_length // 2 - 1 = 7
    hot, seed = list(range(300, 320)), list(range(600, 630))
    tr.generate_segments(e, [np.zeros(SEC, np.float32)], max_length=L, temperatures=(0.0,), hotwords=hot)
    assert e.calls[-1] == [[tk.sot_prev] + hot[:7] + list(tk.sot_sequence)]   # hotwords alone emit <|startofprev|>
    # hotwords (7) + previous text (7) + <|startofprev|> + sot = 16 = max_length: nothing left to sample
    with pytest.raises(ValueError, match="no position to sample"):
        tr.generate_segments(e, [np.zeros(SEC, np.float32)], max_length=L, temperatures=(0.0,), hotwords=hot,
                             initial_prompt=seed)
    e2 = _Engine([])
    tr.generate_segments(e2, [np.zeros(SEC, np.float32)], max_length=L, temperatures=(0.0,), initial_prompt=seed)
    assert e2.calls == [[[tk.sot_prev] + seed[-7:] + list(tk.sot_sequence)]]


def test_options_reach_every_decode_and_defaults_reach_none():
    e = _Engine(fail=[0])
    aud = [np.zeros(SEC, np.float32)]
    tr.generate_segments(e, aud, temperatures=(0.0, 0.4))
    assert [set(k) for k in e.kwargs] == [{"temperature"}] * 2    # defaults: the calls as before
    e = _Engine(fail=[0])
    tr.generate_segments(e, aud, temperatures=(0.0, 0.4), repetition_penalty=1, no_repeat_ngram_size=0,
                         suppress_tokens=[-1])
    assert [set(k) for k in e.kwargs] == [{"temperature"}] * 2
    opts = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, suppress_tokens=[-1, 11])
    e = _Engine(fail=[0])
    tr.generate_segments(e, aud, temperatures=(0.0, 0.4), **opts)
    assert len(e.kwargs) == 2 and e.kwargs[1]["temperature"] == 0.4
    for k in e.kwargs:
        assert {n: k[n] for n in opts} == opts
    e = _Engine(fail=[0])
    tr.generate_segments(e, aud, temperatures=(0.0, 0.4), speculative=True, **opts)
    assert len(e.kwargs) == 1 and not np.isscalar(e.kwargs[0]["temperature"])
    assert {n: e.kwargs[0][n] for n in opts} == opts


def test_transcribe_takes_the_names_and_ignores_the_rest():
    import inspect
    sig = inspect.signature(tr.WhisperModel.transcribe).parameters
    want = dict(repetition_penalty=1, no_repeat_ngram_size=0, initial_prompt=None, hotwords=None,
                condition_on_previous_text=True, prompt_reset_on_temperature=0.5)
    for name, default in want.items():
        assert sig[name].default == default, name
    assert list(sig["suppress_tokens"].default) == [-1]
    assert "_ignored" in sig and "prefix" not in sig and "without_timestamps" not in sig
    gs = inspect.signature(tr.generate_segments).parameters
    for name, default in want.items():
        assert gs[name].default == default, name
