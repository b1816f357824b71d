"""Word timestamps on the host: the rules 6 - 8 of include/janus.h as
janus_amd/services/transcriber.py runs them, on hand-built inputs, against exact expected
values and against tests/align_ref.py; the reference DTW against a brute-force minimum."""
import copy
import itertools
import os
import re

import numpy as np
import pytest
import torch

import align_ref
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd.services import transcriber as tr
from janus_amd.whisper import CONFIGS, Alignment, WhisperEngine, check_alignment_heads, default_alignment_heads

TK = tok.WhisperTokenizer()     # the table vocabulary
EOT = TK.eot


def enc(text):
    return TK.encode_text(text)


# ------------------------------------------------------------------ rule 6: the split
def test_split_spaces_and_punctuation():
    toks = enc("hi, yo.")
    words, wt = TK.split_to_word_tokens(toks + [EOT])
    assert words == ["hi", ",", " yo", ".", ""]
    assert wt == [toks[0:2], toks[2:3], toks[3:6], toks[6:7], [EOT]]
    assert (words, wt) == align_ref.split_words(TK, toks + [EOT])


def test_split_table_words_with_leading_space():
    """Pseudo-word tokens of the table: one with a leading space starts a word, one without
    continues the word before it."""
    sp = next(i for i in range(256, 2000) if TK._table[i].startswith(b" "))
    ns = next(i for i in range(256, 2000) if not TK._table[i].startswith(b" "))
    words, wt = TK.split_to_word_tokens([ns, ns, sp, ns, sp, EOT])
    a, b = TK._table[ns].decode(), TK._table[sp].decode()
    assert words == [a + a, b + a, b, ""]
    assert wt == [[ns, ns], [sp, ns], [sp], [EOT]]


def test_split_multibyte_character_across_tokens():
    toks = enc("a é€b")      # é: 2 bytes, €: 3 bytes, one token per byte
    assert len(toks) == 8
    words, wt = TK.split_to_word_tokens(toks + [EOT])
    assert words == ["a", " é€b", ""]
    assert wt == [toks[:1], toks[1:], [EOT]]
    assert (words, wt) == align_ref.split_words(TK, toks + [EOT])
    # a sequence ending inside a character: the whole text carries the U+FFFD too, so the
    # piece closes with it (faster-whisper's test against the full decode)
    words, wt = TK.split_to_word_tokens(toks[:3])
    assert words == ["a", " \ufffd"] and wt == [toks[:1], toks[1:3]]
    assert (words, wt) == align_ref.split_words(TK, toks[:3])
    # bytes that are no UTF-8 at all stay a piece of their own, nothing after them is lost
    bad = [toks[0], toks[2], toks[0], toks[1], toks[0]]          # a, 0xC3, a, " ", a
    words, wt = TK.split_to_word_tokens(bad + [EOT])
    assert words == ["a\ufffda", " a", ""] and wt == [bad[:3], bad[3:], [EOT]]
    assert (words, wt) == align_ref.split_words(TK, bad + [EOT])


def test_split_empty_text():
    assert TK.split_to_word_tokens([EOT]) == ([""], [[EOT]])
    assert tr.find_alignment(TK, [], None) == []
    al = Alignment(np.array([0]), np.array([0]), np.zeros(0, np.float32))
    assert tr.find_alignment(TK, [], al) == []


# ------------------------------------------------------------------ merge_punctuations
def W(word, start=0.0, end=0.0, tokens=None, p=1.0):
    return dict(word=word, tokens=list(tokens if tokens is not None else [1]), start=start, end=end,
                probability=p)


def test_merge_punctuations():
    al = [W(" ("), W("ab", tokens=[2, 3]), W(","), W(" \""), W(" '"), W("cd"), W("."), W(")"), W(" x "), W("!")]
    ref = [[w["word"], list(w["tokens"]), 0.0, 0.0, 1.0] for w in al]
    tr.merge_punctuations(al)
    assert [w["word"] for w in al] == ["", " (ab,", "", "", "", " \" 'cd.)", "", "", " x ", "!"]
    assert [w["tokens"] for w in al] == [[], [1, 2, 3, 1], [], [], [], [1, 1, 1, 1, 1], [], [], [1], [1]]
    align_ref.merge_punct(ref)
    assert [r[0] for r in ref] == [w["word"] for w in al]
    assert [r[1] for r in ref] == [w["tokens"] for w in al]
    # custom sets: nothing merges when both are empty
    al = [W(" ("), W("ab"), W(".")]
    tr.merge_punctuations(al, "", "")
    assert [w["word"] for w in al] == [" (", "ab", "."]


# ------------------------------------------------------------------ jumps and boundaries
def test_find_alignment_jump_arithmetic():
    """A given path: text rows 0 .. 4 (4 text tokens + eot) over 10 frames. The words are
    "hi" (2 tokens), "," and " y": starts / ends are the frames where the path first enters a
    word's first row and the next word's first row, * 0.02 s."""
    text = enc("hi, y")
    assert len(text) == 5
    ti = np.array([0, 0, 1, 2, 2, 2, 3, 4, 4, 5, 5])
    fi = np.array([0, 1, 2, 3, 4, 5, 6, 6, 7, 8, 9])
    probs = np.array([0.5, 0.25, 1.0, 0.125, 0.375], np.float32)
    got = tr.find_alignment(TK, text, Alignment(ti, fi, probs))
    # jumps at path positions 0, 2, 3, 6, 7, 9 -> frames 0, 2, 3, 6, 6, 8; boundaries 0, 2, 3, 5
    assert [w["word"] for w in got] == ["hi", ",", " y"]
    assert [w["tokens"] for w in got] == [text[:2], text[2:3], text[3:]]
    assert [w["start"] for w in got] == [0 * 0.02, 3 * 0.02, 6 * 0.02]
    assert [w["end"] for w in got] == [3 * 0.02, 6 * 0.02, 8 * 0.02]
    assert [w["probability"] for w in got] == [0.375, 1.0, 0.25]
    ref = align_ref.words_of(TK, text, ti, fi, probs)
    assert [(w["word"], w["tokens"], w["start"], w["end"], w["probability"]) for w in got] == \
        [tuple(r) for r in ref]


# ------------------------------------------------------------------ rule 7, branch by branch
def run_both(segs, words, seek=0, last=0.0):
    """add_word_timestamps on copies of the same input through transcriber.py and through
    align_ref.add_words; returns (segments, words per segment, last, branches taken)."""
    s1 = [dict(start=a, end=b, tokens=list(t)) for (a, b, t) in segs]
    a1 = copy.deepcopy(words)
    last1 = tr.add_word_timestamps(TK, s1, a1, seek, last)
    s2 = [[a, b, list(t)] for (a, b, t) in segs]
    a2 = [[w["word"], list(w["tokens"]), w["start"], w["end"], w["probability"]] for w in words]
    taken = []
    s2, w2, last2 = align_ref.add_words(TK, s2, a2, seek, last, taken=taken)
    assert last1 == last2
    assert [(d["start"], d["end"]) for d in s1] == [(s[0], s[1]) for s in s2]
    assert [[(w["word"], w["start"], w["end"], w["probability"]) for w in d["words"]] for d in s1] == w2
    return s1, [d["words"] for d in s1], last1, taken


def even_words(n, step=0.2, t0=0.0, first_tok=300):
    return [W(f" w{k}", t0 + k * step, t0 + (k + 1) * step, [first_tok + k]) for k in range(n)]


def test_rule7_plain_assignment_by_token_count():
    """Two segments of 2 and 3 text tokens: the words go to them by token count, times are
    seek * 0.01 + t rounded to 0.01, the segment bounds become the word bounds."""
    ws = even_words(5)
    segs = [(10.0, 10.4, [tok.TIMESTAMP_BEGIN, 300, 301, tok.TIMESTAMP_BEGIN + 20]),
            (10.4, 11.0, [tok.TIMESTAMP_BEGIN + 20, 302, 303, 304, tok.TIMESTAMP_BEGIN + 50])]
    s, w, last, taken = run_both(segs, ws, seek=1000, last=10.0)
    assert taken == []
    assert [len(x) for x in w] == [2, 3]
    assert [(x["start"], x["end"]) for x in w[0]] == [(10.0, 10.2), (10.2, 10.4)]
    assert (s[0]["start"], s[0]["end"]) == (10.0, 10.4) and (s[1]["start"], s[1]["end"]) == (10.4, 11.0)
    assert last == 11.0


def test_rule7_durations_and_empty_words():
    """median_duration = min(0.7, median of the non-zero durations); a word emptied by the
    punctuation merge is skipped but its tokens count."""
    ws = [W(" a", 0.0, 2.0, [300]), W(",", 2.0, 2.0, [11]), W(" b", 2.0, 4.0, [301])]
    s, w, last, taken = run_both([(0.0, 4.0, [300, 11, 301])], ws)
    assert [x["word"] for x in w[0]] == [" a,", " b"]
    assert taken == []                     # median 0.7 (capped), max 1.4: no sentence mark involved
    # no non-zero duration at all: median 0, nothing moves
    ws = [W(" a", 1.0, 1.0, [300]), W(" b", 1.0, 1.0, [301])]
    s, w, last, taken = run_both([(0.0, 2.0, [300, 301])], ws)
    assert taken == [] and (s[0]["start"], s[0]["end"]) == (1.0, 1.0)


def test_rule7_sentence_end_marks():
    ws = even_words(4) + [W(".", 0.8, 3.0, [13]), W(" z", 3.0, 5.0, [400]), W(" q", 5.0, 5.2, [401])]
    s, w, last, taken = run_both([(0.0, 5.2, [300, 301, 302, 303, 13, 400, 401])], ws)
    assert taken[:2] == ["sentence_end_self", "sentence_end_prev"]
    # median 0.2, max 0.4: "." is cut at its end, the word after it at its start; "." then
    # joins " w3" (appended), keeping " w3"'s own times
    assert [x["word"] for x in w[0]] == [" w0", " w1", " w2", " w3.", " z", " q"]
    z = w[0][4]
    assert (z["start"], z["end"]) == (pytest.approx(4.6, abs=1e-9), 5.0)


def test_rule7_pause_first_word_too_long():
    ws = [W(" a", 0.0, 3.0, [300])] + even_words(4, t0=3.0, first_tok=301)
    s, w, last, taken = run_both([(2.0, 3.8, [300, 301, 302, 303, 304])], ws, last=0.0)
    assert taken[0] == "pause" and "pause_second" not in taken
    assert (w[0][0]["start"], w[0][0]["end"]) == (pytest.approx(2.6, abs=1e-9), 3.0)   # end - max_duration (0.4)
    # no pause before the first word (last_speech close): the rule does not fire
    s, w, last, taken = run_both([(2.0, 3.8, [300, 301, 302, 303, 304])], ws, last=2.5)
    assert "pause" not in taken


def test_rule7_pause_second_word_too_long():
    ws = [W(" a", 5.0, 5.2, [300]), W(" b", 5.2, 8.0, [301])] + even_words(3, t0=8.0, first_tok=302)
    s, w, last, taken = run_both([(5.0, 8.6, [300, 301, 302, 303, 304])], ws, last=0.0)
    assert taken[:2] == ["pause", "pause_second"]
    # median 0.2, max 0.4: boundary = max(8.0 / 2, 8.0 - 0.4) = 7.6
    assert (w[0][0]["start"], w[0][0]["end"]) == (pytest.approx(7.2, abs=1e-9), pytest.approx(7.6, abs=1e-9))
    assert w[0][1]["start"] == w[0][0]["end"] and w[0][1]["end"] == 8.0


def test_rule7_segment_start_and_end_preferred():
    ws = [W(" a", 0.0, 3.0, [300])] + even_words(3, t0=3.0, first_tok=301) + [W(" z", 3.6, 6.0, [304])]
    # close to the last speech (no pause rule); the segment says 2.5 .. 4.0
    s, w, last, taken = run_both([(2.5, 4.0, [300, 301, 302, 303, 304])], ws, last=2.9)
    assert taken == ["segment_start", "segment_end"]
    assert w[0][0]["start"] == 2.5            # min(end - median, seg.start) = min(2.8, 2.5)
    assert w[0][-1]["end"] == 4.0             # max(start + median, seg.end) = max(3.8, 4.0)
    assert (s[0]["start"], s[0]["end"]) == (2.5, 4.0) and last == 4.0
    # otherwise the segment takes the word bounds
    s, w, last, taken = run_both([(0.2, 5.8, [300, 301, 302, 303, 304])], ws, last=2.9)
    assert taken == [] and (s[0]["start"], s[0]["end"]) == (0.0, 6.0) and last == 6.0


def test_rule7_last_speech_carries_over_segments_without_words():
    ws = even_words(2)
    segs = [(0.0, 0.4, [300, 301]), (0.4, 0.9, [tok.TIMESTAMP_BEGIN + 20, tok.TIMESTAMP_BEGIN + 45])]
    s, w, last, taken = run_both(segs, ws, last=0.0)
    assert w[1] == [] and last == 0.4 and (s[1]["start"], s[1]["end"]) == (0.4, 0.9)


# ------------------------------------------------------------------ rule 8
def test_rule8_seek():
    words = [dict(words=[dict(end=12.34)]), dict(words=[])]
    assert tr.word_seek(words, 1000, 4000, False) == 1234
    assert tr.word_seek(words, 1000, 4000, True) == 4000            # single timestamp ending
    assert tr.word_seek(words, 1234, 4000, False) == 4000           # not after the window's start
    assert tr.word_seek([dict(words=[])], 1000, 4000, False) == 4000  # no words at all


def test_rule8_in_the_loop_matches_reference():
    """advance() over two hand-built windows (the second a no-speech skip) against
    align_ref.seek_loop: seeks, segment bounds and words."""
    tb = tok.TIMESTAMP_BEGIN
    text = enc(" ab cd")
    toks = [tb] + text + [tb + 100, tb + 100] + enc(" e")        # no single timestamp ending
    n = len(text) + 2
    ti = np.array(list(range(n + 1)) + [n] * 40)
    fi = np.arange(len(ti)) * 3
    al = Alignment(ti, fi, np.full(n, 0.5, np.float32))
    s = tr._Stream(content_frames=6000)
    c = tr.candidate(TK, toks, -0.3, 0.0, 0.0)
    tr.advance(TK, s, 3000, c, c, 0, 0, True, al)
    skip = tr.candidate(TK, [], -2.0, 0.9, 0.0)
    size2 = s.window_size()
    tr.advance(TK, s, size2, skip, skip, 0, 0, True, None)
    seeks, segs = align_ref.seek_loop(TK, 6000, [(toks, -0.3, 0.0, al), ([], -2.0, 0.9, None)],
                                      complete=False)
    assert s.window_seeks == seeks
    last_end = s.segments[-1].words[-1].end
    assert seeks[0] == (0, 3000, round(last_end * 100)) and seeks[0][2] != 200
    assert [(g.seek, g.tokens, [(w.word, w.start, w.end, w.probability) for w in g.words])
            for g in s.segments] == [(a, t, ws) for (a, _, _, t, ws) in segs]
    for g, r in zip(s.segments, segs):
        assert abs(g.start - r[1]) < 1e-9 and abs(g.end - r[2]) < 1e-9


# ------------------------------------------------------------------ the public interface
class _Out:
    def __init__(self, n):
        self.n_tokens = torch.zeros(n, dtype=torch.int32)
        self._n = n

    def rows(self):
        return [([], -0.5, 0.0)] * self._n


class _StubEngine:
    """Enough of WhisperEngine for generate_segments on the CPU (as tests/test_beam_host.py):
    every window decodes to nothing and passes its gates."""

    def __init__(self):
        self.tokenizer = TK
        self.device = torch.device("cpu")
        self.calls = []

    def logmel_frames(self, pcm, offs, batch, decim, frames):
        return torch.zeros(batch, frames, 80, dtype=torch.float16)

    def encode(self, mel):
        return torch.zeros(mel.shape[0], 1, 1, dtype=torch.float16)

    def decode_ex(self, enc, prompts=None, max_length=448, **kw):
        self.calls.append(("greedy", len(prompts)))
        return _Out(len(prompts))

    def align(self, enc, texts, sizes, enc_index=None):
        self.calls.append(("align", [list(t) for t in texts], list(sizes), list(enc_index)))
        return [None] * len(texts)


def test_transcribe_keywords():
    m = tr.WhisperModel.__new__(tr.WhisperModel)
    m.engine = _StubEngine()
    m.stats = {"windows": 0, "needs_fallback": 0, "no_speech_skips": 0, "fallback_decodes": 0}
    audio = np.zeros(16000, np.float32)
    list(m.transcribe(audio)[0])
    list(m.transcribe(audio, word_timestamps=False)[0])
    assert m.engine.calls == [("greedy", 1), ("greedy", 1)]          # off: no align call
    list(m.transcribe(audio, word_timestamps=True, prepend_punctuations="(", append_punctuations=".",
                      hallucination_silence_threshold=None)[0])
    assert m.engine.calls[-1] == ("align", [[]], [100], [0])
    with pytest.raises(NotImplementedError, match="hallucination_silence_threshold"):
        m.transcribe(audio, word_timestamps=True, hallucination_silence_threshold=2.0)
    assert tr.Segment(0, 0, 0.0, 1.0, "x", [], 0.0, 0.0, 0.0, 0.0).words is None
    assert dataclasses_fields(tr.Segment)[-1] == "words"
    assert dataclasses_fields(tr.Word) == ["start", "end", "word", "probability"]


def dataclasses_fields(cls):
    import dataclasses
    return [f.name for f in dataclasses.fields(cls)]


def test_generate_segments_aligns_a_round_in_one_call():
    e = _StubEngine()
    tr.generate_segments(e, [np.zeros(16000, np.float32), np.zeros(32000, np.float32)], word_timestamps=True)
    assert [c[0] for c in e.calls] == ["greedy", "align"]
    assert e.calls[1][2] == [100, 200] and e.calls[1][3] == [0, 1]


def test_alignment_heads_validation():
    cfg = CONFIGS["tiny.en"]
    assert default_alignment_heads(cfg) == [(l, h) for l in (2, 3) for h in range(6)]
    assert default_alignment_heads(CONFIGS["distil-small.en"]) == [(l, h) for l in (2, 3) for h in range(12)]
    assert check_alignment_heads(cfg, [(3, 5), [0, 0]]) == [(3, 5), (0, 0)]
    for bad in ([], [(4, 0)], [(0, 6)], [(-1, 0)], [(0, 0), (0, 0)], [(0, 0)] * 65, [3], "ab"):
        with pytest.raises(ValueError, match="alignment"):
            check_alignment_heads(cfg, bad)
    with pytest.raises(ValueError, match="alignment"):    # before any GPU call
        WhisperEngine(cfg, weights={}, alignment_heads=[(9, 9)])


def test_align_arguments():
    e = WhisperEngine.__new__(WhisperEngine)
    e.tokenizer, e.cfg = TK, CONFIGS["tiny.en"]
    encd = torch.zeros(2, 1500, 384, dtype=torch.float16)
    assert e.align(encd, [[], []], [3000, 3000]) == [None, None]     # no text: nothing runs
    with pytest.raises(ValueError, match="one text"):
        e.align(encd, [[1]], [3000, 3000])
    with pytest.raises(ValueError, match="n_text_ctx"):
        e.align(encd, [[1] * 446], [3000])
    for bad in (1, 3001):
        with pytest.raises(ValueError, match=r"\[2, 3000\]"):
            e.align(encd, [[1]], [bad])
    with pytest.raises(ValueError, match="enc_index"):
        e.align(encd, [[1]], [3000], enc_index=[2])


def test_align_symbols_declared():
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    api = open(os.path.join(inc, "janus.h")).read()
    kapi = open(os.path.join(inc, "janus_kernels.h")).read()
    for name in ("janus_whisper_align", "janus_whisper_set_alignment_heads"):
        assert re.search(r"\bint %s\(" % name, api) and name in nat.SIGNATURES
    for name in ("janus_align_dtw_f32", "janus_align_reduce_f32", "janus_align_token_prob_f16"):
        assert re.search(r"\bint %s\(" % name, kapi) and name in nat.SIGNATURES


def test_align_plan_host_program():
    """The HIP-free plan and validation of janus_whisper_align (csrc/align_plan.cpp) through
    tools/align_plan_check.cpp, built here with the host compiler: packed rows, tiles, forced
    targets, buffer totals and every rejection."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.join(os.path.dirname(__file__), "..")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "align_plan_check")
        subprocess.run(["g++", "-std=c++17", "-I", os.path.join(root, "janus_amd", "csrc"),
                        os.path.join(root, "tools", "align_plan_check.cpp"),
                        os.path.join(root, "janus_amd", "csrc", "align_plan.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("all ok"), out.stdout


# ------------------------------------------------------------------ the reference DTW itself
def all_paths(N, F):
    """Every monotone path (0, 0) -> (N - 1, F - 1) with steps (1, 1), (1, 0), (0, 1)."""
    def go(i, j):
        if (i, j) == (N - 1, F - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < N and j + dj < F:
                for rest in go(i + di, j + dj):
                    yield [(i, j)] + rest
    return go(0, 0)


@pytest.mark.parametrize("N,F", list(itertools.product(range(1, 6), range(1, 6))))
def test_reference_dtw_is_optimal(N, F):
    """align_ref.dtw against the brute-force minimum over all monotone paths. Random fp32
    matrices (no ties between finite costs): the path's cost is the minimum, up to the fp32
    rounding of at most N + F additions of values below 8. Matrices of multiples of 0.25
    (every sum exact, ties on purpose): cost[N][F] is the minimum exactly; the path is
    well-formed and the same in both forms of the reference, but on a tie c0 == c1 < c2 the
    rule's trace takes c2, so its cost is not asserted."""
    rng = np.random.default_rng(100 * N + F)
    for trial in range(6):
        x = rng.standard_normal((N, F)).astype(np.float32)
        if trial % 2 == 0:
            x = np.round(x * 4) / 4
        ti, fi = align_ref.dtw(x)
        align_ref.check_path_shape(ti, fi, N, F)
        best = min(sum(float(x[i, j]) for i, j in p) for p in all_paths(N, F))
        if trial % 2 == 0:
            assert align_ref.dtw(x, return_cost=True) == best
        else:
            assert align_ref.path_cost(x, ti, fi) <= best + (N + F) * 8 * 2.0 ** -23, (x, ti, fi)
        lt, lf = align_ref.dtw_loop(x)
        assert np.array_equal(ti, lt) and np.array_equal(fi, lf)


def test_reference_dtw_diagonal_form_equals_loop_form():
    rng = np.random.default_rng(7)
    for (N, F, q) in ((17, 40, False), (23, 31, True), (40, 9, True)):
        x = rng.standard_normal((N, F)).astype(np.float32)
        if q:
            x = np.round(x * 4) / 4
        a, b = align_ref.dtw(x), align_ref.dtw_loop(x)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
