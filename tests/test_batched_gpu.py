"""The batched long-form call on the GPU (services/batched.py), tiny.en / tiny
with seeded synthetic weights at max_length <= 24:

1. the packed feature call against a separate log-mel of every slice, bit for bit;
2. the decode of five chunks at batch_size 5, 2 and 1 against each other and against single-row
   engine calls on the same encoder rows, exactly; once with beams;
3. the segments with timestamps against the oracle's greedy decode of every chunk's own window
   (tests/batched_ref.py, tests/golden/batched_refs.json): tokens identical;
4. the speech-gate route on a file of bursts and zeros: the chunks of the host rule, segments
   inside their chunks, duration_after_vad; a single clip against transcribe's first window;
5. a multilingual engine (detected language, per-chunk languages) and word timestamps."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import batched_ref as br
from janus_amd.services import batched as bt
from janus_amd.services import transcriber as tr
from janus_amd.services import vad_filter as vf
from janus_amd.workload import synth_speech

pytestmark = pytest.mark.gpu

SR = 16000
ML = 24


@functools.lru_cache(maxsize=None)
def model_en():
    return tr.WhisperModel("tiny.en")


@functools.lru_cache(maxsize=None)
def model_ml():
    return tr.WhisperModel("tiny")


@contextlib.contextmanager
def spy(engine, name):
    """Record (args, kwargs, result) of every engine.<name> call inside the block."""
    calls, orig = [], getattr(engine, name)

    def wrapped(*a, **k):
        out = orig(*a, **k)
        calls.append((a, k, out))
        return out
    setattr(engine, name, wrapped)
    try:
        yield calls
    finally:
        delattr(engine, name)


def logmel_of(engine, x, dev):
    pcm = torch.from_numpy(np.concatenate([x, np.zeros(1, np.float32)])).to(dev)
    offs = torch.tensor([0, len(x)], dtype=torch.int64, device=dev)
    return engine.logmel(pcm, offs, 1, 1)[0]


# ------------------------------------------------------------------ 1. features
def test_packed_features_equal_each_slice(gpu):
    """Clips of 0.5 s, exactly 30 s and 31 s (trimmed to 3000 frames) inside 70 s: ONE log-mel
    call for the round, row j bit-identical to the log-mel of slice j alone (each normalised
    over itself, zero from its content end on)."""
    m = model_en()
    audio = np.ascontiguousarray(synth_speech(4200, 70.0, sr=SR))
    clips = [(3.0, 3.5), (5.0, 35.0), (36.0, 67.0)]
    with spy(m.engine, "logmel") as calls:
        segs, info = bt.BatchedInferencePipeline(m).transcribe(audio, clip_timestamps=clips, max_length=ML)
    assert len(calls) == 1 and calls[0][0][2] == 3
    mel = calls[0][2]
    assert mel.shape == (3, 3000, 80)
    for j, (a, b) in enumerate(clips):
        one = logmel_of(m.engine, audio[int(a * SR):int(b * SR)], gpu)
        assert torch.equal(mel[j], one), j
    assert float(mel[0, 50:].abs().max()) == 0.0 and float(mel[0, :50].abs().amax(dim=-1).min()) > 0.0
    assert float(mel[1, 2999].abs().max()) > 0.0 and float(mel[2, 2999].abs().max()) > 0.0
    assert info.duration_after_vad == 0.5 + 30.0 + 31.0 and len(list(segs)) == 3
    # the packing alone, on ranges that touch and overlap
    pcm = torch.from_numpy(np.concatenate([audio, np.zeros(1, np.float32)])).to(gpu)
    spans = [(0, 8000), (8000, 8161), (4000, 4000 + 31 * SR)]
    got = bt.chunk_features(m.engine, pcm, spans)
    for j, (a, b) in enumerate(spans):
        assert torch.equal(got[j], logmel_of(m.engine, audio[a:b], gpu)), j


# ------------------------------------------------------------------ 2. decode equivalence
FIVE = [(0.0, 7.3), (8.0, 8.9), (10.0, 40.0), (41.0, 52.52), (53.0, 59.99)]


@functools.lru_cache(maxsize=None)
def five_audio():
    return np.ascontiguousarray(synth_speech(4300, 60.0, sr=SR))


def chunk_rows(res):
    return [(c.tokens, c.avg_logprob, c.no_speech_prob) for c in res.chunks]


def test_decode_does_not_depend_on_the_batch(gpu):
    """Five chunks without timestamps at batch_size 5, 2 and 1: tokens, avg_logprob and
    no_speech_prob identical to each other and to five single-row decode_ex(timestamps=False)
    calls on the same encoder rows (rows are independent of their batch neighbours)."""
    eng = model_en().engine
    tk = eng.tokenizer
    kw = dict(clip_timestamps=[FIVE], max_length=ML)
    with spy(eng, "encode") as encs, spy(eng, "decode_ex") as decs:
        (r5,) = bt.generate_segments_batched(eng, [five_audio()], batch_size=5, **kw)
    assert len(encs) == 1 and len(decs) == 1 and decs[0][1]["timestamps"] is False
    enc = encs[0][2]
    prompt = [tk.sot, tk.no_timestamps]
    assert [c.prompt for c in r5.chunks] == [prompt] * 5
    rows = chunk_rows(r5)
    # (seeded weights decode most chunks to the same few tokens: the statistics tell the rows apart)
    assert all(len(t) == ML - 2 for t, _, _ in rows) and len({lp for _, lp, _ in rows}) == 5
    assert all(t < tk.eot for r in rows for t in r[0])                        # no timestamp is sampled
    for j in range(5):
        one = eng.decode_ex(enc[j:j + 1].contiguous(), prompts=[prompt], max_length=ML, timestamps=False,
                            no_speech_back=1).rows()[0]
        print(f"chunk {j}: batch avg_logprob {rows[j][1]!r} single {one[1]!r}; nsp {rows[j][2]!r} single {one[2]!r}")
        assert one == rows[j], j
    for bs in (2, 1):
        with spy(eng, "decode_ex") as decs:
            (r,) = bt.generate_segments_batched(eng, [five_audio()], batch_size=bs, **kw)
        assert [len(d[1]["prompts"]) for d in decs] == ([2, 2, 1] if bs == 2 else [1] * 5)
        for j, (got, want) in enumerate(zip(chunk_rows(r), rows)):
            print(f"batch_size {bs} chunk {j}: avg_logprob {got[1]!r} against {want[1]!r}")
        assert chunk_rows(r) == rows, bs
        assert r.segments == r5.segments
    assert [(s.start, s.end, s.seek, s.id) for s in r5.segments] == \
        [(a, b, int(round(a * SR)) // 160, k) for k, (a, b) in enumerate(FIVE)]


def test_beam_decode_does_not_depend_on_the_batch(gpu):
    """The same with beam_size=3 against decode_beam on every chunk's encoder row."""
    eng = model_en().engine
    tk = eng.tokenizer
    with spy(eng, "encode") as encs, spy(eng, "decode_beam") as decs:
        (r5,) = bt.generate_segments_batched(eng, [five_audio()], clip_timestamps=[FIVE], max_length=ML, beam_size=3)
    assert len(decs) == 1 and decs[0][1]["beam_size"] == 3 and decs[0][1]["timestamps"] is False
    enc, rows = encs[0][2], chunk_rows(r5)
    for j in range(5):
        one = eng.decode_beam(enc[j:j + 1].contiguous(), prompts=[[tk.sot, tk.no_timestamps]], beam_size=3,
                              max_length=ML, timestamps=False, no_speech_back=1).rows()[0]
        print(f"chunk {j}: beam avg_logprob {rows[j][1]!r} single {one[1]!r}")
        assert one == rows[j], j
    (r2,) = bt.generate_segments_batched(eng, [five_audio()], clip_timestamps=[FIVE], max_length=ML, beam_size=3,
                                         batch_size=2)
    assert chunk_rows(r2) == rows


# ------------------------------------------------------------------ 3. oracle parity
def test_segments_with_timestamps_match_the_oracle(gpu):
    """without_timestamps=False over the four chunks of batched_ref.PARITY_CASE: every chunk's
    tokens are the oracle's greedy decode of that chunk's own window — identical, no chunk
    excused: the generator asserted every reference margin >= 2 NEAR_TIE — and the segments are
    the reference's slices from the chunk's start. The statistics within the project's decode
    tolerances (tests/test_decode_options_gpu.py: sum_logprob 1e-3 relative + 1e-3, nsp 5e-3)."""
    ref = br.parity_reference()
    c = ref["case"]
    assert min(ch["min_margin"] for ch in ref["chunks"]) >= br.MIN_MARGIN
    m = model_en()
    (res,) = bt.generate_segments_batched(m.engine, [br.parity_audio(c)], clip_timestamps=[c["clips"]],
                                          without_timestamps=False, max_length=c["max_length"], batch_size=3)
    assert [(ch.start, ch.end) for ch in res.chunks] == [(w["start"], w["end"]) for w in ref["chunks"]]
    for k, (ch, w) in enumerate(zip(res.chunks, ref["chunks"])):
        print(f"chunk {k}: margin {w['min_margin']:.4f} avg_logprob {ch.avg_logprob:.6f} (ref {w['avg']:.6f}) "
              f"nsp {ch.no_speech_prob:.3e} (ref {w['nsp']:.3e})")
        assert ch.tokens == w["tokens"], k
        n = len(w["tokens"]) + 1
        assert abs(ch.avg_logprob - w["avg"]) <= (1e-3 * abs(w["avg"]) * n + 1e-3) / n
        assert abs(ch.no_speech_prob - w["nsp"]) <= 5e-3 * w["nsp"] + 1e-12
    assert len(res.segments) == len(ref["segments"])
    for s, (st, en, toks) in zip(res.segments, ref["segments"]):
        assert s.tokens == toks and s.start == pytest.approx(st, abs=1e-9) and s.end == pytest.approx(en, abs=1e-9)
    assert [s.id for s in res.segments] == list(range(len(res.segments)))


# ------------------------------------------------------------------ 4. the speech-gate route
def test_vad_route_on_bursts_and_zeros(gpu, monkeypatch):
    """70 s of 12 s speech bursts and 2 s of zeros through the energy stand-in: numpy first
    shows that no window's probability lies near a threshold, then the chunks are
    merge_segments of the host rule on those probabilities, every segment lies within its
    chunk and duration_after_vad is the chunks' sum."""
    audio, inside = br.burst_file()
    p = br.energy_probs(audio)
    n = len(audio) // 512
    full = inside[:n * 512].reshape(n, 512)
    assert (p[:n][full.all(axis=1)] >= 0.9).all() and (p[:n][~full.any(axis=1)] <= 0.1).all()
    assert ((p >= 0.9) | (p <= 0.1)).all()                    # the windows on a burst's edge too
    opts = vf.batched_vad_options(None)
    speeches = vf.get_speech_timestamps(p, len(audio), opts)
    want = vf.merge_segments(speeches)
    assert len(speeches) == 5 and [len(w[2]) for w in want] == [2, 2, 1]
    m = model_en()
    (gp,) = vf.speech_probabilities_device(torch.from_numpy(audio).to(gpu), [0, len(audio)], None)
    assert np.abs(gp - p).max() < 1e-3 and vf.get_speech_timestamps(gp, len(audio), opts) == speeches
    monkeypatch.setattr(m, "_vad", lambda: None)              # the stand-in, whatever weights are around
    with spy(m.engine, "logmel") as mels, spy(m.engine, "decode_ex") as decs:
        segs, info = bt.BatchedInferencePipeline(m).transcribe(audio, max_length=ML, batch_size=2)
    segs = list(segs)
    assert [c[0][2] for c in mels] == [2, 1] and len(decs) == 2
    assert info.vad_options == opts and info.duration == 70.0
    assert info.duration_after_vad == sum(b - a for a, b, _ in want) / SR
    assert [(s.start, s.end) for s in segs] == [(a / SR, b / SR) for a, b, _ in want]
    (res,) = bt.generate_segments_batched(m.engine, [audio], max_length=ML, without_timestamps=False)
    assert [(c.start, c.end, c.speeches) for c in res.chunks] == want
    assert len(res.segments) >= 3
    # with timestamps a segment starts in its chunk and ends within the 30 s its tokens can name
    # (seeded weights name times the audio does not have; the default mode above is the chunk itself)
    starts = {a // 160: a / SR for a, b, _ in want}
    for s in res.segments:
        a = starts[s.seek]
        assert a <= s.start < s.end <= a + 30.0 + 1e-9, (s.start, s.end, a)


def test_single_clip_is_transcribes_first_window(gpu):
    """One clip of at most 30 s with timestamps on: the segments of WhisperModel.transcribe's
    first window at T = 0 (the same features, prompt and decode)."""
    m = model_en()
    audio = np.ascontiguousarray(synth_speech(4400, 21.37, sr=SR))
    want = [s for s in m.transcribe(audio, temperature=0, max_length=ML)[0] if s.seek == 0]
    segs, info = bt.BatchedInferencePipeline(m).transcribe(audio, vad_filter=False, without_timestamps=False,
                                                            max_length=ML)
    segs = list(segs)
    assert len(want) >= 1 and info.duration_after_vad == info.duration == len(audio) / SR

    def key(s):
        return (s.id, s.seek, s.start, s.end, s.text, s.tokens, s.temperature, s.avg_logprob, s.no_speech_prob,
                s.compression_ratio)
    assert [key(s) for s in segs] == [key(s) for s in want]


# ------------------------------------------------------------------ 5. languages and words
THREE = [(0.0, 6.0), (7.0, 18.5), (19.0, 27.25)]


def test_multilingual_engine(gpu):
    """tiny: language=None is the first chunk's detection (from the round's own encoder
    output: one encode, one detect_language call); multilingual=True gives every chunk the
    start sequence of its own detection."""
    m = model_ml()
    eng, tk = m.engine, m.engine.tokenizer
    audio = np.ascontiguousarray(np.concatenate([synth_speech(4500 + k, 10.0, sr=SR, f0=f) for k, f in
                                                 enumerate((110.0, 180.0, 260.0))]))
    pipe = bt.BatchedInferencePipeline(m)
    with spy(eng, "encode") as encs, spy(eng, "detect_language") as dets, spy(eng, "decode_ex") as decs:
        segs, info = pipe.transcribe(audio, clip_timestamps=THREE, max_length=ML)
    assert len(encs) == len(dets) == len(decs) == 1
    probs = eng.detect_language(encs[0][2])[0].cpu().numpy()
    best = [tk.languages[int(np.argmax(q))] for q in probs]
    print("detected per chunk:", best, [float(q.max()) for q in probs])
    assert info.language == best[0] and info.language_probability == float(probs[0].max())
    assert info.all_language_probs[0] == (best[0], float(probs[0].max())) and len(info.all_language_probs) == 99
    want = tk.sot_sequence_for(best[0], "transcribe") + [tk.no_timestamps]
    assert decs[0][1]["prompts"] == [want] * 3 and decs[0][1]["no_speech_back"] == 3
    first = [s.tokens for s in segs]
    with spy(eng, "detect_language") as dets, spy(eng, "decode_ex") as decs:
        (res,) = bt.generate_segments_batched(eng, [audio], clip_timestamps=[THREE], max_length=ML,
                                              multilingual=True, task="translate", batch_size=2)
    assert [d[0][0].shape[0] for d in dets] == [2, 1]
    assert [c.language for c in res.chunks] == best and res.language == best[0]
    assert [p for d in decs for p in d[1]["prompts"]] == \
        [tk.sot_sequence_for(code, "translate") + [tk.no_timestamps] for code in best]
    assert len(first) == len(res.segments) == 3
    # a given language needs no detection
    with spy(eng, "detect_language") as dets:
        segs, info = pipe.transcribe(audio, clip_timestamps=THREE, max_length=ML, language="fr")
    assert dets == [] and (info.language, info.language_probability) == ("fr", 1.0)


def test_word_timestamps_lie_inside_their_chunks(gpu):
    """word_timestamps=True over three chunks in rounds of two: one align call per round, every
    word inside its chunk (times are rounded to 0.01 s) and the words monotone over the file."""
    m = model_en()
    audio = np.ascontiguousarray(synth_speech(4600, 28.0, sr=SR))
    with spy(m.engine, "align") as als:
        segs, info = bt.BatchedInferencePipeline(m).transcribe(audio, clip_timestamps=THREE, max_length=ML,
                                                                word_timestamps=True, batch_size=2)
    segs = list(segs)
    assert [list(a[0][2]) for a in als] == [[600, 1150], [825]]
    assert len(segs) == 3 and all(s.words for s in segs)
    for s, (a, b) in zip(segs, THREE):
        assert s.seek == int(a * 100)
        assert (s.start, s.end) == (s.words[0].start, s.words[-1].end)
        for w in s.words:
            assert a - 0.01 <= w.start <= w.end <= b + 0.01, (w, a, b)
            assert 0.0 <= w.probability <= 1.0
    flat = [w for s in segs for w in s.words]
    assert all(x.start <= y.start and x.end <= y.end for x, y in zip(flat, flat[1:]))
