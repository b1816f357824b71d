"""Beam search, host side (no GPU): the numpy reference of the rule (tests/beam_ref.py)
against the greedy oracle at beam 1, the walk on hand-made candidates, the argument checks of
WhisperModel.transcribe / generate_segments / WhisperEngine.decode_beam on stub engines, and
the new symbols in the headers and the ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

import beam_ref
from janus_amd import _native
from janus_amd import tokenizer as tok
from janus_amd.services import transcriber as tr
from janus_amd.whisper import CONFIGS, WhisperEngine, check_beam_args, synthetic_weights
from oracle import whisper as ow

CFG = CONFIGS["tiny.en"]
EOT = 50


def test_reference_beam_one_is_greedy():
    """The reference at k = 1 reproduces greedy_cached: tokens and sum_lp, and its nsp."""
    W = synthetic_weights(CFG, seed=5)
    tk = tok.load_tokenizer()
    g = torch.Generator().manual_seed(3)
    enc = (torch.randn(2, CFG.n_audio_ctx, CFG.d_model, generator=g) * 0.5).half().float().numpy()
    ref = ow.greedy_cached(enc, W, CFG, tk, max_length=12, no_speech=tok.NO_SPEECH)
    got = beam_ref.beam_search(enc, W, CFG, tk, 1, max_length=12, no_speech=tok.NO_SPEECH)
    for r, b in zip(ref, got):
        assert b["winner"]["tokens"] == r["tokens"]
        assert abs(b["winner"]["sum_lp"] - r["sum_lp"]) <= 1e-4 * abs(r["sum_lp"])
        assert abs(b["nsp"] - r["nsp"]) <= 1e-4 * r["nsp"] + 1e-12
        assert b["n_finished"] == 0 and b["stop_step"] == 12 - len(tk.sot_sequence)


def lp_row(entries, V=64):
    lp = np.full(V, -np.inf)
    for v, x in entries.items():
        lp[v] = x
    return lp


def test_walk_eot_ahead_of_text():
    """An eot candidate ahead of the text candidates finishes its beam's hypothesis and does
    not take a live slot; the next three candidates become the beams."""
    lps = [lp_row({EOT: -0.1, 7: -0.5, 8: -2.0}), lp_row({9: -0.2, 3: -0.9}), lp_row({4: -3.0})]
    cands = beam_ref.top_candidates([0.0, -0.25, -0.5], lps, 7)
    assert cands[0] == (-0.1, 0, EOT)
    live, fin, used = beam_ref.walk(cands, 3, EOT, 0)
    assert fin == [(0, -0.1)]
    assert [(b, v) for b, v, _ in live] == [(1, 9), (0, 7), (1, 3)] and used == 4
    assert [s for _, _, s in live] == [-0.45, -0.5, -1.15]


def test_walk_finished_list_capped():
    """The finished list holds at most k: with k - 1 already finished, the second eot
    candidate of a step is dropped; the walk still only reads the best 2k."""
    lps = [lp_row({EOT: -0.1, 5: -4.0}), lp_row({EOT: -0.2, 6: -5.0}), lp_row({EOT: -0.3, 7: -6.0})]
    cands = beam_ref.top_candidates([0.0, 0.0, 0.0], lps, 7)
    live, fin, used = beam_ref.walk(cands, 3, EOT, 2)
    assert fin == [(0, -0.1)] and used == 6
    assert [(b, v) for b, v, _ in live] == [(0, 5), (1, 6), (2, 7)]
    live, fin, _ = beam_ref.walk(cands, 3, EOT, 0)
    assert [b for b, _ in fin] == [0, 1, 2]


def test_walk_tie_order():
    """Equal scores order by beam, then by token."""
    lps = [lp_row({9: -1.0, 4: -1.0}), lp_row({2: -0.5, 1: -0.5}), lp_row({0: -1.0})]
    cands = beam_ref.top_candidates([0.0, -0.5, 0.0], lps, 7)
    assert [(b, v) for _, b, v in cands] == [(0, 4), (0, 9), (1, 1), (1, 2), (2, 0)]
    live, _, used = beam_ref.walk(cands, 3, EOT, 0)
    assert [(b, v) for b, v, _ in live] == [(0, 4), (0, 9), (1, 1)] and used == 3


def test_choose_and_close_at_max_length():
    """Rule 6: the best S / n^length_penalty among the finished, the earliest on ties; with
    none finished the live beams close at n + 1."""
    fin = [dict(tokens=[1, 2, EOT], sum_lp=-3.0), dict(tokens=[1, EOT], sum_lp=-2.0),
           dict(tokens=[4, 5, 6, EOT], sum_lp=-3.6)]
    w, margin = beam_ref.choose(fin, [dict(tokens=[1], sum_lp=-0.1)])
    assert w["tokens"] == [4, 5, 6, EOT] and abs(margin - 0.1) < 1e-12
    w, _ = beam_ref.choose(fin[:2], [])
    assert w["tokens"] == [1, 2, EOT]                      # -1.0 twice: the earliest
    w, _ = beam_ref.choose(fin, [], length_penalty=0.5)
    assert w["tokens"] == [1, EOT]                         # -2 / sqrt(2) beats -3 / sqrt(3), -3.6 / 2
    live = [dict(tokens=[1, 2, 3], sum_lp=-4.0), dict(tokens=[7, 8, 9], sum_lp=-3.0)]
    w, margin = beam_ref.choose([], live)
    assert w["tokens"] == [7, 8, 9] and w["score"] == -0.75 and margin == 0.25


# ------------------------------------------------------------------ argument checks
def test_check_beam_args():
    for k in (1, 5, 8):
        check_beam_args(k, 1.0, 1)
    for bad in (9, 16):
        with pytest.raises(NotImplementedError, match="1 .. 8"):
            check_beam_args(bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="beam_size"):
            check_beam_args(bad)
    with pytest.raises(NotImplementedError, match="patience 1"):
        check_beam_args(5, 1.0, 2)
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="length_penalty must be > 0"):
            check_beam_args(5, bad)


class _Out:
    def __init__(self, n):
        self.n_tokens = torch.zeros(n, dtype=torch.int32)
        self._n = n

    def rows(self):
        return [([], -0.5, 0.0)] * self._n


class _StubEngine:
    """Enough of WhisperEngine for generate_segments on the CPU: every window decodes to
    nothing and passes its gates, so each utterance takes one window per 30 s."""

    def __init__(self, cfg=None):
        self.tokenizer = tok.load_tokenizer()
        self.device = torch.device("cpu")
        self.calls = []
        if cfg is not None:
            self.cfg = cfg

    def logmel_frames(self, pcm, offs, batch, decim, frames):
        return torch.zeros(batch, frames, 80, dtype=torch.float16)

    def encode(self, mel):
        return torch.zeros(mel.shape[0], 1, 1, dtype=torch.float16)

    def decode_ex(self, enc, prompts=None, max_length=448, **kw):
        self.calls.append(("greedy", len(prompts), kw))
        return _Out(len(prompts))

    def decode_beam(self, enc, prompts=None, beam_size=5, length_penalty=1.0, max_length=448, **kw):
        self.calls.append(("beam", len(prompts), dict(beam_size=beam_size, length_penalty=length_penalty)))
        return _Out(len(prompts))


def test_generate_segments_routes_and_chunks():
    """beam_size 1 keeps the greedy call; beam_size k sends the T = 0 decode through
    decode_beam in chunks of windows x k <= the model's row cap (320 in place, 60 gathered);
    the speculative form is greedy only."""
    auds = [np.zeros(16000, np.float32)] * 70
    e = _StubEngine()
    tr.generate_segments(e, auds)
    assert [(c[0], c[1]) for c in e.calls] == [("greedy", 64), ("greedy", 6)]
    e = _StubEngine()
    tr.generate_segments(e, auds, beam_size=8, length_penalty=0.8)
    assert [(c[0], c[1]) for c in e.calls] == [("beam", 40), ("beam", 30)]
    assert e.calls[0][2] == dict(beam_size=8, length_penalty=0.8)
    e = _StubEngine(CONFIGS["distil-small.en"])
    tr.generate_segments(e, auds[:30], beam_size=5)
    assert [(c[0], c[1]) for c in e.calls] == [("beam", 12), ("beam", 12), ("beam", 6)]
    with pytest.raises(NotImplementedError, match="speculative"):
        tr.generate_segments(_StubEngine(), auds[:1], beam_size=2, speculative=True)
    with pytest.raises(NotImplementedError, match="1 .. 8"):
        tr.generate_segments(_StubEngine(), auds[:1], beam_size=9)


def test_transcribe_beam_arguments():
    """WhisperModel.transcribe: beam_size 1 .. 8 run (1 on today's greedy path), anything
    else, patience != 1 and length_penalty <= 0 raise with the limit in the message."""
    m = tr.WhisperModel.__new__(tr.WhisperModel)
    m.engine = _StubEngine()
    m.stats = {"windows": 0, "needs_fallback": 0, "no_speech_skips": 0, "fallback_decodes": 0}
    audio = np.zeros(16000, np.float32)
    list(m.transcribe(audio, beam_size=1)[0])
    assert [c[0] for c in m.engine.calls] == ["greedy"]
    list(m.transcribe(audio, beam_size=5, length_penalty=1.0, patience=1)[0])
    assert m.engine.calls[-1] == ("beam", 1, dict(beam_size=5, length_penalty=1.0))
    for bad in (0, 9):
        with pytest.raises((NotImplementedError, ValueError), match="beam_size"):
            m.transcribe(audio, beam_size=bad)
    with pytest.raises(NotImplementedError, match="patience"):
        m.transcribe(audio, beam_size=5, patience=2.0)
    with pytest.raises(ValueError, match="length_penalty"):
        m.transcribe(audio, beam_size=5, length_penalty=0.0)


def test_decode_beam_arguments():
    """WhisperEngine.decode_beam rejects, before any GPU call: a beam outside 1 .. 8, staggered
    rows, a temperature > 0 and more than 512 rows."""
    e = WhisperEngine.__new__(WhisperEngine)
    enc = torch.zeros(4, 1, 1)
    with pytest.raises(NotImplementedError, match="1 .. 8"):
        e.decode_beam(enc, beam_size=12)
    with pytest.raises(ValueError, match="length_penalty"):
        e.decode_beam(enc, beam_size=5, length_penalty=-1.0)
    with pytest.raises(ValueError, match="pos_offset"):
        e.decode_beam(enc, beam_size=5, pos_offset=[0, 0, 0, 0])
    with pytest.raises(ValueError, match="temperature 0"):
        e.decode_beam(enc, beam_size=5, temperature=0.2)
    with pytest.raises(ValueError, match="limit is 512"):
        e.decode_beam(torch.zeros(103, 1, 1), beam_size=5)


def test_beam_symbols_declared():
    """The new entry points are in the headers and in the ctypes table."""
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    api = open(os.path.join(inc, "janus.h")).read()
    kapi = open(os.path.join(inc, "janus_kernels.h")).read()
    assert re.search(r"\bint janus_whisper_decode_beam_ex\(", api)
    assert "beam_size" in api and "length_penalty" in api
    for name in ("janus_beam_partial_blocks", "janus_beam_logits_topk_f16", "janus_beam_step",
                 "janus_beam_reorder_f16"):
        assert re.search(r"\bint %s\(" % name, kapi), name
        assert name in _native.SIGNATURES
    assert len(_native.SIGNATURES["janus_whisper_decode_beam_ex"]) == 12


def test_recorded_references_are_current():
    """tests/golden/beam_refs.json holds every case of beam_ref.CASES and the transcribe case
    as they are defined now, and its first tiny_k2 window is what the reference computes."""
    g = beam_ref._golden()
    for name, case in beam_ref.CASES.items():
        assert g[name]["case"] == case and len(g[name]["windows"]) == len(case["seeds"]), name
    assert g["transcribe"]["case"] == beam_ref.TRANSCRIBE_CASE
    tk = tok.load_tokenizer()
    c = beam_ref.CASES["tiny_k2"]
    cfg, W, enc, _ = beam_ref.case_inputs("tiny_k2", tk)
    r = beam_ref.beam_search(enc[:1], W, cfg, tk, c["k"], max_length=c["max_length"], no_speech=tok.NO_SPEECH)[0]
    want = g["tiny_k2"]["windows"][0]
    assert r["winner"]["tokens"] == want["tokens"]
    # (the oracle's forward is float32: another batch size reorders its sums, ~1e-7 relative)
    assert abs(r["winner"]["sum_lp"] - want["sum_lp"]) <= 1e-5 * abs(want["sum_lp"])
    assert abs(r["min_margin"] - want["min_margin"]) <= 1e-4
