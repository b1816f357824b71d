"""The batched long-form call on the CPU: the chunk rule (vad_filter.merge_segments, the clip
forms, the options the gate runs under) on hand-computed cases, and generate_segments_batched /
BatchedInferencePipeline over a stub engine that records every call: the call sequence of a
round, the rows, the prompts, the keywords, the caps, the refusals and the segments."""
import numpy as np
import pytest
import torch

from janus_amd import tokenizer as tok
from janus_amd import whisper as jw
from janus_amd.services import batched as bt
from janus_amd.services import transcriber as tr
from janus_amd.services import vad_filter as vf

SR = 16000
L30 = 30 * SR
TB = 50363           # <|0.00|> of the *.en layout


# ------------------------------------------------------------------ the chunk rule
def test_merge_segments_hand_cases():
    assert vf.merge_segments([]) == []
    assert vf.merge_segments([(1000, 5000)]) == [(1000, 5000, [(1000, 5000)])]
    # three speeches whose last end lies exactly at the limit: one chunk, pauses inside
    sp = [(0, 100000), (150000, 300000), (320000, L30)]
    assert vf.merge_segments(sp) == [(0, L30, sp)]
    # one sample more: the speech whose end crosses the limit opens the next chunk at its start
    sp2 = sp[:2] + [(320000, L30 + 1)]
    assert vf.merge_segments(sp2) == [(0, 300000, sp[:2]), (320000, L30 + 1, [(320000, L30 + 1)])]
    # the limit counts from the open chunk's start, not from zero
    sp3 = [(100000, 200000), (250000, 100000 + L30), (100000 + L30 + 5, 100000 + L30 + 9)]
    assert vf.merge_segments(sp3) == [(100000, 100000 + L30, sp3[:2]), (sp3[2][0], sp3[2][1], sp3[2:])]
    # a first speech alone longer than the limit is a chunk of its own (nothing to close before it)
    long = [(1000, 600000), (610000, 700000)]
    assert vf.merge_segments(long) == [(1000, 600000, long[:1]), (610000, 700000, long[1:])]
    assert vf.merge_segments([(0, 600000)]) == [(0, 600000, [(0, 600000)])]
    # and one in the middle closes the chunk before it and is closed by the speech after it
    mid = [(0, 16000), (20000, 620000), (630000, 640000)]
    assert vf.merge_segments(mid) == [(0, 16000, mid[:1]), (20000, 620000, mid[1:2]), (630000, 640000, mid[2:])]
    assert vf.merge_segments([(0, 16000), (20000, 40000)], chunk_length_s=2) == \
        [(0, 16000, [(0, 16000)]), (20000, 40000, [(20000, 40000)])]


def test_clip_timestamps_both_forms():
    n = 40 * SR
    pairs = vf.clip_chunks([(0.5, 1.0), (2, 33.0)], n)
    dicts = vf.clip_chunks([{"start": 0.5, "end": 1.0}, {"start": 2, "end": 33.0}], n)
    assert pairs == dicts == [(8000, 16000, [(8000, 16000)]), (32000, 528000, [(32000, 528000)])]
    assert vf.clip_chunks([(39.0, 45.0)], n) == [(39 * SR, n, [(39 * SR, n)])]      # cut to the audio
    assert vf.clip_chunks([], n) == []
    for bad in ([(2.0, 1.0)], [(-1.0, 1.0)]):
        with pytest.raises(ValueError, match="clip_timestamps"):
            vf.clip_chunks(bad, n)


def test_gate_options_of_the_batched_call():
    assert vf.batched_vad_options(None) == vf.VadOptions(min_silence_duration_ms=160, max_speech_duration_s=30)
    o = vf.batched_vad_options(dict(min_silence_duration_ms=500, max_speech_duration_s=5, threshold=0.3))
    assert o == vf.VadOptions(threshold=0.3, min_silence_duration_ms=500, max_speech_duration_s=30)
    given = vf.VadOptions(speech_pad_ms=100)
    o = vf.batched_vad_options(given)
    assert o == vf.VadOptions(speech_pad_ms=100, min_silence_duration_ms=2000, max_speech_duration_s=30)
    assert given.max_speech_duration_s == float("inf")                              # the caller's is untouched
    with pytest.raises(TypeError):
        vf.batched_vad_options(dict(no_such_field=1))


# ------------------------------------------------------------------ the stub engine
class _Out:
    def __init__(self, rows):
        self._rows = rows
        self.n_tokens = torch.tensor([len(r[0]) + 1 for r in rows], dtype=torch.int32)

    def rows(self):
        return self._rows


class _Engine:
    """Enough of WhisperEngine for the batched call on the CPU. Every call is recorded in
    ``log`` as (name, details); any other attribute of the engine is an AttributeError, so a
    call outside the five shows. Row r (counted over the whole call) decodes to
    ``script(r)``; ``lang(r)`` is the language index row r of a detect_language call gets."""

    def __init__(self, script=None, multilingual=False, lang=None):
        self.tokenizer = tok.WhisperTokenizer(multilingual=multilingual)
        self.device = torch.device("cpu")
        self.cfg = jw.CONFIGS["tiny" if multilingual else "tiny.en"]
        self.log, self.row = [], 0
        self.script = script or (lambda r: [1000 + r, 2000 + r])
        self.lang = lang or (lambda r: 0)

    def names(self):
        return [n for n, _ in self.log]

    def logmel(self, pcm, offsets, batch, decim):
        self.log.append(("logmel", dict(pcm=pcm.clone(), offsets=offsets.tolist(), batch=batch, decim=decim)))
        return torch.zeros(batch, 3000, 80, dtype=torch.float16)

    def encode(self, mel):
        self.log.append(("encode", dict(rows=mel.shape[0])))
        return torch.zeros(mel.shape[0], 1, 1, dtype=torch.float16) + torch.arange(mel.shape[0])[:, None, None]

    def detect_language(self, enc):
        self.log.append(("detect_language", dict(rows=[int(v) for v in enc[:, 0, 0]])))
        p = np.full((enc.shape[0], self.tokenizer.n_languages), 0.001, np.float32)
        for k, v in enumerate(enc[:, 0, 0]):
            p[k, self.lang(self.row + int(v))] = 0.9
        return torch.from_numpy(p), None

    def _decode(self, name, enc, prompts, max_length, kw):
        self.log.append((name, dict(prompts=[list(p) for p in prompts], max_length=max_length, kw=kw,
                                    rows=enc.shape[0])))
        out = _Out([(list(self.script(self.row + k)), -0.25 - 0.01 * (self.row + k), 0.125) for k in range(len(prompts))])
        self.row += len(prompts)
        return out

    def decode_ex(self, enc, prompts=None, max_length=448, **kw):
        return self._decode("decode_ex", enc, prompts, max_length, kw)

    def decode_beam(self, enc, prompts=None, max_length=448, **kw):
        return self._decode("decode_beam", enc, prompts, max_length, kw)

    def align(self, enc, texts, sizes, enc_index=None, **kw):
        self.log.append(("align", dict(texts=[list(t) for t in texts], sizes=list(sizes), enc_index=list(enc_index), kw=kw)))
        out = []
        for t in texts:
            if not t:
                out.append(None)
                continue
            n = len(t) + 1                                   # text + <|endoftext|>, two frames each
            out.append(jw.Alignment(np.repeat(np.arange(n), 2).astype(np.int32),
                                    (5 * np.arange(2 * n)).astype(np.int32),
                                    np.full(len(t), 0.5, np.float32)))
        return out


class _Gate:
    """A speech gate whose probabilities are given: probs_file as SileroGate's."""

    def __init__(self, speech):
        self.speech, self.calls = speech, []

    def probs_file(self, pcm, offsets, max_chunks_per_pass=0):
        self.calls.append((pcm, [int(o) for o in offsets]))
        out = []
        for a, b in zip(offsets[:-1], offsets[1:]):
            t = (np.arange((b - a) // 512 + 1) * 512 + 256) / SR
            out.append(self.speech(t).astype(np.float32))
        return out


def ramp(seconds, base=0.0):
    return (np.arange(int(seconds * SR), dtype=np.float32) + base)


def bursts(t):
    """12 s of speech, 2 s of pause, from 0 on: five bursts, the last ends at 68 s."""
    return np.where(((t % 14.0) < 12.0) & (t < 68.0), 1.0, 0.0)


def model(engine, gate=None):
    m = tr.WhisperModel.__new__(tr.WhisperModel)
    m.engine, m._vad_gate, m._vad_weights = engine, gate, {}
    m.stats = {"windows": 0, "needs_fallback": 0, "no_speech_skips": 0, "fallback_decodes": 0}
    m._vad = lambda: gate
    return m


def test_exported_beside_whisper_model():
    from janus_amd.services.transcriber import BatchedInferencePipeline, generate_segments_batched
    assert BatchedInferencePipeline is bt.BatchedInferencePipeline
    assert generate_segments_batched is bt.generate_segments_batched
    assert "BatchedInferencePipeline" in tr.__all__ and "WhisperModel" in tr.__all__
    with pytest.raises(AttributeError):
        tr.no_such_name


# ------------------------------------------------------------------ rounds
def test_vad_route_rounds_rows_and_prompts():
    """70 s of 12 s bursts and 2 s pauses: the speeches (padded by 0.4 s) are about
    (0, 12.4) (13.6, 26.4) (27.6, 40.4) (41.6, 54.4) (55.6, 68.4) s, so the third and the fifth
    cross 30 s from their chunk's start: three chunks, in rounds of 2 and 1."""
    audio = ramp(70.0)
    e, g = _Engine(), _Gate(bursts)
    (res,) = bt.generate_segments_batched(e, [audio], batch_size=2, vad=g)
    opts = vf.batched_vad_options(None)
    (probs,) = g.probs_file(None, np.array([0, len(audio)]))
    speeches = vf.get_speech_timestamps(probs, len(audio), opts)
    want = vf.merge_segments(speeches)
    assert len(speeches) == 5 and [len(w[2]) for w in want] == [2, 2, 1]
    assert all(e_ - s_ <= L30 for s_, e_, _ in want)
    assert [(c.start, c.end, c.speeches) for c in res.chunks] == want
    assert len(g.calls) == 2 and g.calls[0][1] == [0, len(audio)]              # (the second is the test's own)
    assert g.calls[0][0].numel() == len(audio) + 1                             # the uploaded buffer itself
    assert e.names() == ["logmel", "encode", "decode_ex"] * 2
    for r, rows in enumerate((want[:2], want[2:])):
        lm, en, de = (d for _, d in e.log[3 * r:3 * r + 3])
        assert lm["batch"] == en["rows"] == de["rows"] == len(de["prompts"]) == len(rows) and lm["decim"] == 1
        lens = [b - a for a, b, _ in rows]
        assert lm["offsets"] == [0] + list(np.cumsum(lens))
        for j, (a, b, _) in enumerate(rows):                                   # the chunk's own samples
            assert torch.equal(lm["pcm"][lm["offsets"][j]:lm["offsets"][j + 1]], torch.from_numpy(audio[a:b]))
        tk = e.tokenizer
        assert de["prompts"] == [[tk.sot, tk.no_timestamps]] * len(rows)
        assert de["kw"] == dict(timestamps=False, no_speech_back=1) and de["max_length"] == 448
    assert res.vad_options == opts and res.duration == 70.0
    assert res.duration_after_vad == sum(b - a for a, b, _ in want) / SR
    assert [(s.id, s.seek, s.start, s.end, s.tokens, s.temperature) for s in res.segments] == \
        [(k, a // 160, a / SR, b / SR, [1000 + k, 2000 + k], 0.0) for k, (a, b, _) in enumerate(want)]
    assert [s.avg_logprob for s in res.segments] == [-0.25, -0.26, -0.27]
    assert all(s.no_speech_prob == 0.125 and s.words is None and not s.needs_fallback for s in res.segments)
    assert all(s.compression_ratio == tr.compression_ratio(s.text.strip()) for s in res.segments)
    # one round or three: the same result
    for bs in (64, 1):
        e2 = _Engine()
        (r2,) = bt.generate_segments_batched(e2, [audio], batch_size=bs, vad=_Gate(bursts))
        assert [len(d["prompts"]) for n, d in e2.log if n == "decode_ex"] == ([3] if bs == 64 else [1, 1, 1])
        assert r2.segments == res.segments


def test_given_vad_parameters_keep_their_fields_but_the_length():
    e, g = _Engine(), _Gate(bursts)
    audio = ramp(70.0)
    given = dict(min_silence_duration_ms=3000, speech_pad_ms=0, max_speech_duration_s=1000.0)
    (res,) = bt.generate_segments_batched(e, [audio], vad=g, vad_parameters=given)
    assert res.vad_options == vf.VadOptions(min_silence_duration_ms=3000, speech_pad_ms=0, max_speech_duration_s=30)
    # 2 s pauses no longer end a speech, so the forced 30 s limit is what cuts: no chunk above it
    assert len(res.chunks) >= 3 and all(c.end - c.start <= L30 for c in res.chunks)


def test_clips_trim_drop_and_two_files():
    """Clips as given: one of 31 s is packed up to the samples its 3000 frames (and the two
    frames after them) read, one shorter than a hop is dropped; two files pool their chunks
    in file-then-time order and share rounds."""
    a0, a1 = ramp(40.0), ramp(3.0, 0.5)
    e = _Engine()
    clips = [[(0.5, 1.0), (2.0, 33.0), (35.0, 35.005)], [{"start": 1.0, "end": 2.5}]]
    r0, r1 = bt.generate_segments_batched(e, [a0, a1], batch_size=2, vad_filter=True, clip_timestamps=clips)
    assert [(c.start, c.end) for c in r0.chunks] == [(8000, 16000), (32000, 528000)]
    assert [(c.start, c.end) for c in r1.chunks] == [(16000, 40000)]
    assert [c.content_frames for c in r0.chunks + r1.chunks] == [50, 3000, 150]
    assert r0.duration_after_vad == (8000 + 496000) / SR and r1.duration_after_vad == 1.5
    assert r0.vad_options is None and r1.vad_options is None                   # no gate ran
    assert e.names() == ["logmel", "encode", "decode_ex"] * 2
    lm0, lm1 = e.log[0][1], e.log[3][1]
    assert lm0["offsets"] == [0, 8000, 8000 + bt.PACK_MAX] and bt.PACK_MAX == L30 + 400
    assert torch.equal(lm0["pcm"][8000:8000 + bt.PACK_MAX], torch.from_numpy(a0[32000:32000 + bt.PACK_MAX]))
    assert lm1["offsets"] == [0, 24000]
    assert torch.equal(lm1["pcm"][:24000], torch.from_numpy(a1[16000:40000]))  # file 1's own samples
    assert [s.id for s in r0.segments] == [0, 1] and [s.id for s in r1.segments] == [0]
    assert [(s.start, s.end, s.seek) for s in r0.segments] == [(0.5, 1.0, 50), (2.0, 33.0, 200)]
    assert r1.segments[0].tokens == [1002, 2002]                               # the call's third row


def test_without_gate_or_clips():
    e = _Engine()
    (res,) = bt.generate_segments_batched(e, [ramp(30.0)], vad_filter=False)
    assert [(c.start, c.end) for c in res.chunks] == [(0, L30)] and res.duration_after_vad == 30.0
    e = _Engine()
    with pytest.raises(RuntimeError) as err:
        bt.generate_segments_batched(e, [ramp(30.0 + 1 / SR)], vad_filter=False)
    assert str(err.value) == "No clip timestamps found. Set 'vad_filter' to True or provide 'clip_timestamps'."
    assert e.log == []
    # no speech: no chunks, no engine call, no segments
    e = _Engine()
    (res,) = bt.generate_segments_batched(e, [ramp(5.0)], vad=_Gate(lambda t: np.zeros_like(t)))
    assert res.chunks == [] and res.segments == [] and res.duration_after_vad == 0.0 and e.log == []
    assert bt.generate_segments_batched(_Engine(), []) == []


def test_beam_cap_and_keywords():
    clips = [[(0.1 * k, 0.1 * k + 0.05) for k in range(45)]]
    e = _Engine()
    bt.generate_segments_batched(e, [ramp(5.0)], clip_timestamps=clips, beam_size=8, length_penalty=0.8)
    assert tr.fallback_rows(e) // 8 == 40
    assert e.names() == ["logmel", "encode", "decode_beam"] * 2
    d0, d1 = e.log[2][1], e.log[5][1]
    assert (d0["rows"], d1["rows"]) == (40, 5)
    assert d0["kw"] == dict(beam_size=8, length_penalty=0.8, timestamps=False, no_speech_back=1)
    e = _Engine()
    bt.generate_segments_batched(e, [ramp(5.0)], clip_timestamps=clips, beam_size=8, batch_size=16)
    assert [d["rows"] for n, d in e.log if n == "decode_beam"] == [16, 16, 13]
    # greedy: the options that differ from the defaults reach the call, the defaults do not
    e = _Engine()
    opts = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, suppress_tokens=[-1, 11])
    bt.generate_segments_batched(e, [ramp(1.0)], vad_filter=False, **opts)
    assert e.log[2][1]["kw"] == dict(opts, timestamps=False, no_speech_back=1)
    e = _Engine()
    bt.generate_segments_batched(e, [ramp(1.0)], vad_filter=False, without_timestamps=False)
    assert e.log[2][1]["kw"] == {} and e.log[2][1]["prompts"] == [[e.tokenizer.sot]]


def test_prompt_and_max_new_tokens():
    e = _Engine()
    tk = e.tokenizer
    hot, seed = list(range(300, 320)), list(range(600, 630))
    bt.generate_segments_batched(e, [ramp(2.0)], clip_timestamps=[[(0, 1), (1, 2)]], max_length=16,
                                 hotwords=hot, max_new_tokens=3)
    want = [tk.sot_prev] + hot[:7] + [tk.sot, tk.no_timestamps]
    assert e.log[2][1]["prompts"] == [want, want] and e.log[2][1]["max_length"] == len(want) + 3
    e = _Engine()
    bt.generate_segments_batched(e, [ramp(1.0)], vad_filter=False, initial_prompt=seed, hotwords=hot[:2],
                                 without_timestamps=False, max_length=64)
    assert e.log[2][1]["prompts"] == [[tk.sot_prev] + hot[:2] + seed[-31:] + [tk.sot]]
    e = _Engine()
    with pytest.raises(ValueError, match="max_new_tokens"):
        bt.generate_segments_batched(e, [ramp(1.0)], vad_filter=False, max_new_tokens=447)
    bt.generate_segments_batched(e, [ramp(1.0)], vad_filter=False, max_new_tokens=446)
    assert e.log[2][1]["max_length"] == 448
    e = _Engine()
    with pytest.raises(ValueError, match="no position to sample"):   # 7 + 7 + <|startofprev|> + sot = 16
        bt.generate_segments_batched(e, [ramp(1.0)], vad_filter=False, max_length=16, hotwords=hot,
                                     initial_prompt=seed, without_timestamps=False)
    with pytest.raises(ValueError, match="no position to sample"):
        bt.generate_segments_batched(e, [ramp(1.0)], vad_filter=False, max_length=2)
    assert e.log == []


def test_refusals_by_name_before_any_engine_call():
    e = _Engine()
    p = bt.BatchedInferencePipeline(model(e))
    a = ramp(1.0)
    for kw, name in ((dict(chunk_length=20), "chunk_length"), (dict(prefix="so"), "prefix"),
                     (dict(patience=2), "patience"), (dict(hallucination_silence_threshold=1.0),
                                                      "hallucination_silence_threshold"),
                     (dict(temperature=0.2), "temperature"), (dict(temperature=(0.4, 0.0)), "temperature"),
                     (dict(beam_size=9), "beam_size"), (dict(beam_size=4, repetition_penalty=1.2), "repetition_penalty"),
                     (dict(beam_size=4, no_repeat_ngram_size=2), "no_repeat_ngram_size"),
                     (dict(beam_size=4, suppress_tokens=[5]), "suppress_tokens"),
                     (dict(language="de"), r"\*\.en"), (dict(task="translate"), r"\*\.en")):
        with pytest.raises(NotImplementedError, match=name):
            p.transcribe(a, **kw)
    with pytest.raises(NotImplementedError, match="chunk_length"):
        bt.generate_segments_batched(e, [a], chunk_length=10)
    for kw, name in ((dict(suppress_tokens=[10 ** 6]), "outside the vocabulary"), (dict(batch_size=0), "batch_size"),
                     (dict(repetition_penalty=0), "repetition_penalty"), (dict(beam_size=0), "beam_size"),
                     (dict(initial_prompt=[-3]), "outside the vocabulary")):
        with pytest.raises(ValueError, match=name):
            p.transcribe(a, **kw)
    assert e.log == []
    # accepted: the defaults' spellings, the unused arguments, later temperatures
    segs, info = p.transcribe(a, chunk_length=30, patience=1, temperature=(0.0, 0.2), log_progress=True,
                              compression_ratio_threshold=1.0, log_prob_threshold=0.0, no_speech_threshold=0.0,
                              vad_filter=False)
    assert len(list(segs)) == 1 and e.names() == ["logmel", "encode", "decode_ex"]


def test_pipeline_info_and_defaults():
    import inspect
    sig = inspect.signature(bt.BatchedInferencePipeline.transcribe).parameters
    want = dict(language=None, task="transcribe", beam_size=1, without_timestamps=True, vad_filter=True,
                vad_parameters=None, clip_timestamps=None, chunk_length=None, batch_size=64, max_new_tokens=None,
                multilingual=False, word_timestamps=False, prefix=None, patience=1)
    for name, default in want.items():
        assert sig[name].default == default, name
    assert "beam_size defaults to 1" in " ".join(bt.BatchedInferencePipeline.transcribe.__doc__.split()).replace("``", "")
    e, g = _Engine(), _Gate(bursts)
    p = bt.BatchedInferencePipeline(model(e, g))
    audio = ramp(70.0)
    segs, info = p.transcribe(audio)
    segs = list(segs)
    (res,) = bt.generate_segments_batched(_Engine(), [audio], vad=_Gate(bursts))
    assert segs == res.segments and len(segs) == 3
    assert info.duration == 70.0 and info.duration_after_vad == res.duration_after_vad
    assert info.vad_options == vf.batched_vad_options(None)
    assert (info.language, info.language_probability, info.all_language_probs) == ("en", 1.0, None)
    # clips win over the gate; without either a short file is one chunk
    segs, info = p.transcribe(audio, clip_timestamps=[(1.0, 2.0), {"start": 3.0, "end": 4.5}])
    assert [(s.start, s.end) for s in segs] == [(1.0, 2.0), (3.0, 4.5)]
    assert info.duration_after_vad == 2.5 and info.vad_options is None and len(g.calls) == 1


# ------------------------------------------------------------------ segments
def test_segments_with_timestamps_from_a_chunk_between_frames():
    """without_timestamps=False: split_window's slices from the chunk's start (8040 samples:
    0.5025 s, no whole frame), no seek carried; a blank chunk gives nothing and ids stay dense."""
    rows = {0: [TB, 1001, 1002, TB + 100, TB + 100, 2001, TB + 150],   # two slices, single ending
            1: [TB + 10, TB + 10],                                      # no text: dropped
            2: [TB, 3001, 3002]}                                        # no closing timestamp: the chunk's length
    e = _Engine(script=lambda r: rows[r])
    clips = [[(8040 / SR, 4.0), (5.0, 6.0), (7.0, 9.3)]]
    (res,) = bt.generate_segments_batched(e, [ramp(10.0)], clip_timestamps=clips, without_timestamps=False)
    off = 8040 / SR
    got = [(s.id, s.seek, s.start, s.end, s.tokens) for s in res.segments]
    assert got == [(0, 50, off + 0.0, off + 2.0, rows[0][:4]), (1, 50, off + 2.0, off + 3.0, rows[0][4:]),
                   (2, 700, 7.0 + 0.0, 7.0 + 3.0, rows[2])]            # ceil(2.3 s) * 100 frames = 3.0 s
    assert e.log[2][1]["kw"] == {} and e.log[2][1]["prompts"] == [[e.tokenizer.sot]] * 3
    assert [s.avg_logprob for s in res.segments] == [-0.25, -0.25, -0.27]
    # without timestamps the blank chunk is dropped the same way
    e = _Engine(script=lambda r: [] if r == 1 else [1000 + r])
    (res,) = bt.generate_segments_batched(e, [ramp(10.0)], clip_timestamps=clips)
    assert [(s.id, s.start, s.end, s.tokens) for s in res.segments] == [(0, off, 4.0, [1000]), (1, 7.0, 9.3, [1002])]
    assert [c.tokens for c in res.chunks] == [[1000], [], [1002]]


def test_default_time_offset_is_todays():
    tk = tok.WhisperTokenizer()
    toks = [TB, 1001, TB + 100, TB + 100, 2001, TB + 150]
    assert tr.split_window(tk, toks, 300, 3000) == tr.split_window(tk, toks, 300, 3000, time_offset=3.0)
    segs, nseek = tr.split_window(tk, toks, 0, 3000, time_offset=0.5025)
    assert [(a, b) for a, b, _ in segs] == [(0.5025, 2.5025), (2.5025, 3.5025)] and nseek == 3000


def test_word_timestamps_one_align_per_round():
    tk = tok.WhisperTokenizer()
    sp = [t for t in range(1000, 1200) if tk.decode([t]).startswith(" ")][:8]     # one word each
    e = _Engine(script=lambda r: [] if r == 1 else sp[2 * r:2 * r + 2])
    clips = [[(8040 / SR, 4.0), (5.0, 6.0), (7.0, 9.3), (9.5, 9.515)]]
    (res,) = bt.generate_segments_batched(e, [ramp(10.0)], clip_timestamps=clips, word_timestamps=True, batch_size=3)
    assert e.names() == ["logmel", "encode", "decode_ex", "align"] * 2
    al = e.log[3][1]
    assert al["sizes"] == [c.content_frames for c in res.chunks[:3]] == [349, 100, 230]
    assert al["texts"] == [sp[0:2], [], sp[4:6]] and al["enc_index"] == [0, 1, 2] and al["kw"] == {}
    assert e.log[7][1]["sizes"] == [1] and e.log[7][1]["texts"] == [[]]        # one frame: nothing to align
    # the stub's path: token k of a chunk spans [0.2 k, 0.2 k + 0.2] s from the chunk's start
    off = 8040 / SR
    s0, s2, s3 = res.segments
    assert [w.word for w in s0.words] == [tk.decode([t]) for t in sp[0:2]]
    assert [(w.start, w.end) for w in s0.words] == [(round(off, 2), round(off + 0.2, 2)), (round(off + 0.2, 2), round(off + 0.4, 2))]
    assert [(w.start, w.end) for w in s2.words] == [(7.0, 7.2), (7.2, 7.4)]
    assert (s0.start, s0.end) == (s0.words[0].start, s0.words[-1].end)         # segments span their words
    assert (s2.start, s2.end) == (7.0, 7.4) and [s.id for s in res.segments] == [0, 1, 2]
    assert s3.words == [] and (s3.start, s3.end) == (9.5, 9.515)
    flat = [w for s in res.segments for w in s.words]
    assert all(a.end <= b.start for a, b in zip(flat, flat[1:])) and all(w.probability == 0.5 for w in flat)


# ------------------------------------------------------------------ languages
def test_language_vote_and_per_chunk_languages():
    clips = [[(k, k + 0.5) for k in range(5)]]
    audio = ramp(6.0)
    e = _Engine(multilingual=True, lang=lambda r: 2)         # every chunk: "de"
    tk = e.tokenizer
    (res,) = bt.generate_segments_batched(e, [audio], clip_timestamps=clips, batch_size=2)
    assert e.names() == ["logmel", "encode", "detect_language", "decode_ex"] + ["logmel", "encode", "decode_ex"] * 2
    assert e.log[2][1]["rows"] == [0, 1]                       # the first round's encoder output, as it is
    de = tk.sot_sequence_for("de", "transcribe")
    for n, d in e.log:
        if n == "decode_ex":
            assert d["prompts"] == [de + [tk.no_timestamps]] * d["rows"]
            assert d["kw"] == dict(timestamps=False, no_speech_back=3)
    assert (res.language, round(res.language_probability, 3)) == ("de", 0.9) and res.all_language_probs[0][0] == "de"
    # multilingual=True: one call per round over every row, each chunk its own start sequence
    langs = [2, 0, 3, 3, 6]
    e = _Engine(multilingual=True, lang=lambda r: langs[r])
    (res,) = bt.generate_segments_batched(e, [audio], clip_timestamps=clips, batch_size=2, multilingual=True,
                                          task="translate", word_timestamps=True)
    assert e.names() == ["logmel", "encode", "detect_language", "decode_ex", "align"] * 3
    codes = [tk.languages[k] for k in langs]
    assert [c.language for c in res.chunks] == codes and res.language == "de"
    got = [p for n, d in e.log if n == "decode_ex" for p in d["prompts"]]
    assert got == [tk.sot_sequence_for(c, "translate") + [tk.no_timestamps] for c in codes]
    sots = [q for n, d in e.log if n == "align" for q in d["kw"]["sot_sequences"]]
    assert sots == [tk.sot_sequence_for(c, "translate") for c in codes]
    # a given language: no detection at all; two files, one code each
    e = _Engine(multilingual=True)
    r0, r1 = bt.generate_segments_batched(e, [audio, audio], clip_timestamps=clips * 2, language=["fr", "ja"],
                                          without_timestamps=False)
    assert "detect_language" not in e.names() and (r0.language, r1.language) == ("fr", "ja")
    assert e.log[2][1]["prompts"] == [tk.sot_sequence_for("fr", "transcribe")] * 5 + [tk.sot_sequence_for("ja", "transcribe")] * 5
    with pytest.raises(ValueError, match="unknown language"):
        bt.generate_segments_batched(_Engine(multilingual=True), [audio], clip_timestamps=clips, language="xx")


def test_language_votes_do_not_depend_on_the_batch_size():
    """language_detection_segments=3 below the threshold: chunk k < 3 decodes with the majority
    of votes 0 .. k (as a window of the seek loop does), the later chunks with the settled
    language — whether the three lie in one round or in three."""
    clips = [[(k, k + 0.5) for k in range(5)]]
    langs = [4, 2, 2, 7, 7]
    results = []
    for bs in (1, 2, 5):
        e = _Engine(multilingual=True, lang=lambda r: langs[r])
        (res,) = bt.generate_segments_batched(e, [ramp(6.0)], clip_timestamps=clips, batch_size=bs,
                                              language_detection_segments=3, language_detection_threshold=0.95)
        results.append(([c.language for c in res.chunks], res.language))
        assert e.names().count("detect_language") == {1: 3, 2: 2, 5: 1}[bs]
    tk = tok.WhisperTokenizer(multilingual=True)
    a, b = tk.languages[4], tk.languages[2]
    assert results == [([a, a, b, b, b], b)] * 3
