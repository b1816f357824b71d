"""vad_filter host rules (services/vad_filter.py): speech timestamps, the collected speech,
the timestamp map and its restoration, and the wiring through generate_segments — no GPU."""
import numpy as np
import pytest
import torch

from janus_amd import tokenizer as tok
from janus_amd.services import transcriber as tr
from janus_amd.services import vad_filter as vf
from janus_amd.services.transcriber import Segment, Word

H, L, M = 0.9, 0.1, 0.4
B = [L] * 5 + [H] * 10 + [L] * 20 + [H] * 10 + [L] * 5

CASES = {
    "A": ([L] * 10 + [H] * 20 + [L] * 70, 51100, {}, [(0, 21760)]),
    "B": (B, 25600, {}, [(0, 25600)]),
    "B'": (B, 25600, dict(min_silence_duration_ms=500), [(0, 12800), (12800, 25600)]),
    "C": ([L] * 20 + [H] * 10 + [L] * 40 + [H] * 10 + [L] * 20, 51200, dict(min_silence_duration_ms=500),
          [(3840, 21760), (29440, 47360)]),
    "D": ([L] * 4 + [H] * 3 + [M] * 70 + [L] * 70, 75264, dict(speech_pad_ms=0), [(2048, 39424)]),
    "E": ([H] * 30 + [L] * 5 + [H] * 65, 51200, dict(max_speech_duration_s=2, speech_pad_ms=0),
          [(0, 15360), (17920, 49664), (50176, 51200)]),
    "F": ([L] * 3 + [H] * 4 + [L] * 20 + [H] * 30, 29177,
          dict(min_silence_duration_ms=320, min_speech_duration_ms=250, speech_pad_ms=30), [(13344, 29177)]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_speech_timestamps(case):
    """The rule of include/janus.h on hand-made probabilities: padding and merging (A, B), the
    gap split at its middle (B'), two padded speeches (C), hysteresis between the thresholds
    (D), the cut of an over-long speech at its last long-enough silence (E), a too-short
    burst dropped (F). Dict and VadOptions forms agree."""
    probs, n, params, want = CASES[case]
    assert vf.get_speech_timestamps(probs, n, vf.as_vad_options(params)) == want
    assert vf.get_speech_timestamps(np.asarray(probs, np.float32), n, vf.VadOptions(**params)) == want


def test_vad_options():
    o = vf.as_vad_options(None)
    assert (o.threshold, o.neg_threshold, o.min_speech_duration_ms, o.max_speech_duration_s,
            o.min_silence_duration_ms, o.speech_pad_ms) == (0.5, None, 0, float("inf"), 2000, 400)
    assert vf.as_vad_options(o) is o
    assert vf.as_vad_options(dict(threshold=0.3)).threshold == 0.3
    with pytest.raises(TypeError):
        vf.as_vad_options(dict(treshold=0.3))
    with pytest.raises(TypeError):
        vf.as_vad_options(0.5)
    # an explicit neg_threshold replaces threshold - 0.15: 0.4 now closes the speech of case D
    probs, n, _, _ = CASES["D"]
    got = vf.get_speech_timestamps(probs, n, vf.VadOptions(neg_threshold=0.45, speech_pad_ms=0))
    assert got == [(2048, 3584)]


SPEECHES = [(3200, 16000), (48000, 80000), (96000, 112000)]


def test_timestamp_map():
    m = vf.SpeechTimestampsMap(SPEECHES)
    assert m.chunk_end_sample == [12800, 44800, 60800]
    assert m.total_silence_before == [0.2, 2.2, 3.2]
    for t, is_end, want in [(0.5, False, 0.7), (0.8, False, 3.0), (0.8, True, 1.0), (2.8, True, 5.0),
                            (2.8, False, 6.0), (3.8, True, 7.0), (9.0, True, 12.2)]:
        assert m.original_time(t, is_end=is_end) == want, (t, is_end)


def test_collect_chunks():
    audio = np.arange(120000, dtype=np.float32)
    kept = vf.collect_chunks(audio, SPEECHES)
    assert len(kept) == sum(b - a for a, b in SPEECHES)
    assert kept[0] == 3200 and kept[12800] == 48000 and kept[-1] == 111999
    assert len(vf.collect_chunks(audio, [])) == 0


def _seg(start, end, words=None):
    return Segment(0, 0, start, end, "x", [1], 0.0, -0.1, 1.0, 0.0, words=words)


def test_restore_speech_timestamps():
    m = vf.SpeechTimestampsMap(SPEECHES)
    # without words: the start maps as a start, the end as an end (0.8 is the first chunk's end)
    a, b = vf.restore_speech_timestamps([_seg(0.1, 0.8), _seg(0.8, 2.8)], m)
    assert (a.start, a.end) == (0.3, 1.0) and (b.start, b.end) == (3.0, 5.0)
    # with words: each word by its middle. The second straddles the chunk end at 0.8 s with its
    # middle (0.76) before it, the third with its middle (0.84) after it
    words = [Word(0.1, 0.5, " a", 0.9), Word(0.62, 0.9, " b", 0.8), Word(0.7, 0.98, " c", 0.7),
             Word(2.9, 3.1, " d", 0.6)]
    src = _seg(0.1, 3.1, words)
    (s,) = vf.restore_speech_timestamps([src], m)
    assert [(w.start, w.end) for w in s.words] == [(0.3, 0.7), (0.82, 1.1), (2.9, 3.18), (6.1, 6.3)]
    assert [w.word for w in s.words] == [" a", " b", " c", " d"] and s.words[1].probability == 0.8
    assert (s.start, s.end) == (0.3, 6.3)
    assert s.text == src.text and s.tokens == src.tokens
    assert (src.start, src.end, src.words[3].start) == (0.1, 3.1, 2.9)   # the input is not changed


class _Out:
    def __init__(self, n):
        self.n_tokens = torch.zeros(n, dtype=torch.int32)
        self._n = n

    def rows(self):
        return [([], -0.5, 0.0)] * self._n


class _StubEngine:
    """Enough of WhisperEngine for generate_segments on the CPU: every window decodes to
    nothing and passes its gates."""

    def __init__(self):
        self.tokenizer = tok.load_tokenizer()
        self.device = torch.device("cpu")
        self.frames = []

    def logmel_frames(self, pcm, offs, batch, decim, frames):
        self.frames.append(frames)
        return torch.zeros(batch, frames, 80, dtype=torch.float16)

    def encode(self, mel):
        return torch.zeros(mel.shape[0], 1, 1, dtype=torch.float16)

    def decode_ex(self, enc, prompts=None, max_length=448, **kw):
        return _Out(len(prompts))


def test_generate_segments_wiring(monkeypatch):
    """vad_filter=False makes no VAD call; vad_filter=True makes ONE for all utterances, before
    the features, and the seek loop runs on the collected speech."""
    calls = []

    def fake_probs(audios, device, vad=None, max_chunks_per_pass=0):
        calls.append((len(audios), vad))
        # first utterance: windows 10..39 are speech; second: none
        return [np.asarray([L] * 10 + [H] * 30 + [L] * (vf.n_windows(len(audios[0])) - 40), np.float32),
                np.full(vf.n_windows(len(audios[1])), L, np.float32)]

    monkeypatch.setattr(vf, "speech_probabilities", fake_probs)
    auds = [np.zeros(48000, np.float32), np.zeros(16000, np.float32)]
    e = _StubEngine()
    sts = tr.generate_segments(e, auds, temperatures=(0.0,))
    assert calls == [] and e.frames == [300, 100]
    assert [s.speech_chunks for s in sts] == [None, None] and sts[0].duration_after_vad == 3.0
    e = _StubEngine()
    gate = object()
    sts = tr.generate_segments(e, auds, temperatures=(0.0,), vad_filter=True, vad=gate,
                               vad_parameters=dict(min_silence_duration_ms=500, speech_pad_ms=100))
    assert calls == [(2, gate)]
    assert sts[0].speech_chunks == [(5120 - 1600, 20480 + 1600)] and sts[1].speech_chunks == []
    assert sts[0].duration_after_vad == (15360 + 3200) / 16000 and sts[1].duration_after_vad == 0.0
    assert e.frames == [(15360 + 3200) // 160]            # the silent utterance computes no features
    assert sts[1].segments == [] and sts[1].windows == 0
    with pytest.raises(TypeError):
        tr.generate_segments(_StubEngine(), auds, vad_filter=True, vad_parameters=dict(nope=1))


def test_transcription_info_fields():
    """The new fields have defaults: positional construction as before the filter."""
    info = tr.TranscriptionInfo("en", 1.0, 2.5, None)
    assert info.duration_after_vad == 2.5 and info.vad_options is None
    info = tr.TranscriptionInfo("en", 1.0, 2.5, None, 1.25, vf.VadOptions())
    assert info.duration_after_vad == 1.25 and info.vad_options.threshold == 0.5
