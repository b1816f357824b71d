"""Batched long-form transcription: faster-whisper's ``BatchedInferencePipeline``.

``WhisperModel.transcribe`` walks one recording through the seek loop, where window n + 1 needs
window n's last timestamp and text: a single file is a batch of one row. The batched call cuts
the file at the pauses the speech gate finds (``vad_filter.merge_segments``), treats every chunk
as a 30 s window of its own and decodes all chunks as the rows of one batch, by default
without timestamps. DESIGN.md §5s states the rule (parity unpinned: faster-whisper is not
reachable offline), the call sequence and the measurement.

Per round of at most ``batch_size`` chunks the engine is called exactly so:

* ONE ``logmel`` over the round's chunks packed on the device (every chunk normalised over
  itself and zero from its content end on, as janus_whisper_logmel does per packed utterance);
* ONE ``encode``;
* at most ONE ``detect_language`` (multilingual engines: the files still undecided, or every
  row with ``multilingual=True``);
* ONE ``decode_ex`` (``beam_size`` 1) or ``decode_beam`` at T = 0 with the same prompt in every
  row — no temperature fallback, no gates and no no-speech skip in this mode;
* with ``word_timestamps``, ONE ``align``.

The files are uploaded once, in one buffer: the gate call and the packing read that buffer.
No kernel is new; the hot path is the project's HIP.
"""
import dataclasses
import math
import time

import numpy as np
import torch

from ..tokenizer import TASKS
from ..whisper import (check_beam_args, check_decoder_compute_beam, check_family_features, check_history_args,
                       resolve_suppress_tokens)
from . import transcriber as tr
from . import vad_filter as vf

SAMPLE_RATE = vf.SAMPLE_RATE
# samples of a chunk that reach its 3000 frames and the two frames after them that the
# normalisation's maximum still covers (frame f reads [160 f - 200, 160 f + 200)): what is
# packed of a chunk longer than 30 s
PACK_MAX = tr.WINDOW_16K + 400


@dataclasses.dataclass
class Chunk:
    """One chunk of a file: the samples [start, end) of that file, the speeches merged into it,
    its place in the file, and — after its round — its decode."""
    file: int
    index: int
    start: int
    end: int
    speeches: list
    tokens: list = None           # sampled tokens without <|endoftext|>
    avg_logprob: float = None
    no_speech_prob: float = None
    language: str = None          # multilingual engines: the language its prompt named
    prompt: list = None

    @property
    def content_frames(self) -> int:
        return min(tr.N_FRAMES, (self.end - self.start) // tr.HOP)


@dataclasses.dataclass
class FileResult:
    """One file of generate_segments_batched."""
    segments: list
    chunks: list
    duration: float
    duration_after_vad: float
    vad_options: object = None
    language: str = "en"
    language_probability: float = 1.0
    all_language_probs: list = None


def file_chunks(spans, file: int):
    """merge_segments' / clip_chunks' spans of one file as Chunks; one shorter than a hop (no
    frame of content) is dropped."""
    kept = [(s, e, inside) for s, e, inside in spans if e - s >= tr.HOP]
    return [Chunk(file, k, int(s), int(e), list(inside)) for k, (s, e, inside) in enumerate(kept)]


def chunk_features(engine, pcm, spans):
    """fp16 [len(spans)][3000][n_mels]: the features of the ranges ``spans`` ([(a, b)], samples)
    of the device buffer ``pcm``, packed on the device and run through ONE engine.logmel
    call. A range longer than 30 s gives its first 3000 frames."""
    parts = [pcm[int(a):min(int(b), int(a) + PACK_MAX)] for a, b in spans]
    offsets = np.zeros(len(parts) + 1, np.int64)
    offsets[1:] = np.cumsum([p.numel() for p in parts])   # (what was copied: never past the packed buffer)
    packed = torch.cat(parts + [pcm.new_zeros(1)])
    return engine.logmel(packed, torch.from_numpy(offsets).to(pcm.device), len(parts), 1)


def batched_prompt(tk, stream, max_length: int, sot_sequence, without_timestamps: bool):
    """_Stream.prompt's prompt with ``sot_sequence`` as its start sequence, then
    <|notimestamps|> when ``without_timestamps``."""
    base = stream.prompt(tk, max_length)
    own = stream.sot_sequence if stream.sot_sequence is not None else tk.sot_sequence
    p = base[:len(base) - len(own)] + list(sot_sequence)
    return p + [tk.no_timestamps] if without_timestamps else p


def generate_segments_batched(engine, audios, batch_size: int = 64, max_length: int = 448,
                              max_new_tokens: int = None, temperatures=(0.0,), beam_size: int = 1,
                              length_penalty: float = 1.0, repetition_penalty: float = 1,
                              no_repeat_ngram_size: int = 0, suppress_tokens=(-1,), initial_prompt=None,
                              hotwords=None, without_timestamps: bool = True, word_timestamps: bool = False,
                              prepend_punctuations: str = tr.PREPEND_PUNCTUATIONS,
                              append_punctuations: str = tr.APPEND_PUNCTUATIONS, language=None,
                              task: str = "transcribe", multilingual: bool = False,
                              language_detection_segments: int = 1,
                              language_detection_threshold: float = 0.5, vad_filter: bool = True,
                              vad_parameters=None, vad=None, clip_timestamps=None, chunk_length=None,
                              stats: dict = None):
    """The batched call for several 16 kHz files at once: their chunks, in file-then-time order,
    are pooled into rounds of ``batch_size`` rows (with ``beam_size`` k > 1 capped so that
    rows x k stays within one decode call's rows, as generate_segments caps its windows); the
    result does not depend on ``batch_size``. Returns one FileResult per file.

    Chunks: ``clip_timestamps`` — None or one entry per file, each None or a list of
    (start_s, end_s) pairs / {"start", "end"} dicts in seconds — are taken as given; a file
    without clips goes through the speech gate when ``vad_filter`` (ONE gate call for the files,
    ``vad``: a SileroGate, None: the energy stand-in; get_speech_timestamps under
    ``vf.batched_vad_options(vad_parameters)``, then ``vf.merge_segments``); without either a
    file of at most 30 s is one chunk and a longer one a RuntimeError. ``chunk_length``: None
    or 30.

    The prompt of every row: <|startofprev|>, ``hotwords``, ``initial_prompt`` (as
    _Stream.prompt cuts them), the start sequence, <|notimestamps|> when
    ``without_timestamps`` — then the call runs with timestamps=False and reads no_speech_prob
    one position further back, at <|startoftranscript|>. ``max_new_tokens``: the decode's
    max_length is len(prompt) + max_new_tokens (ValueError above the model's 448).
    One decode at T = 0 (a first temperature other than 0: NotImplementedError; later ones are
    ignored). ``beam_size``, ``length_penalty``, ``repetition_penalty``, ``no_repeat_ngram_size``
    and ``suppress_tokens`` as in generate_segments, with its refusals.

    Segments: without timestamps one per chunk, [chunk.start, chunk.end] / 16000, dropped when
    its text is blank; with them split_window's slices from the chunk's start (segment_size =
    ceil(seconds) * 100 frames, no seek carried; start == end or blank text dropped). ``id``
    runs over the file, ``seek`` = chunk.start // 160, ``temperature`` 0.0; avg_logprob,
    no_speech_prob and compression_ratio are the chunk's. ``word_timestamps``: the round's
    chunks in one align call (sizes: their content frames), words placed from the chunk's
    start, last_speech_timestamp carried over the file's chunks, segments spanning their words.

    Multilingual engines: ``language`` one code for every file, a list with one entry per file,
    or None to detect — the file's first ``language_detection_segments`` chunks vote
    (_Stream.vote_language) on the encoder output their round computed anyway; a chunk that
    votes decodes with the majority so far, as a window of the seek loop does.
    ``multilingual=True``: every chunk's prompt names its own detected language. On a ``*.en``
    engine none of this runs.

    ``stats`` (a dict, measurement only): filled with ``rounds`` (rows of every round) and the
    host seconds spent in ``vad_rule``, ``chunking`` and ``text``."""
    check_beam_args(beam_size, length_penalty)
    check_decoder_compute_beam(getattr(engine, "decoder_compute", "float16"), beam_size)
    check_family_features(getattr(engine, "cfg", None), beam_size, word_timestamps,
                          getattr(engine, "alignment_heads", None))
    check_history_args(repetition_penalty, no_repeat_ngram_size, beam_size)
    dec_kw = tr.decode_option_kwargs(repetition_penalty, no_repeat_ngram_size, suppress_tokens)
    if "suppress_tokens" in dec_kw:   # (ValueError: an id outside the vocabulary, before any GPU work)
        resolve_suppress_tokens(engine.tokenizer, dec_kw["suppress_tokens"], engine.cfg.n_vocab)
        if beam_size > 1:
            raise NotImplementedError("suppress_tokens other than [-1] is not built for beam search")
    temperatures = (float(temperatures),) if np.isscalar(temperatures) else tuple(float(t) for t in temperatures)
    if not temperatures or temperatures[0] != 0.0:
        raise NotImplementedError("temperature: the batched call decodes once at T = 0; a first "
                                  "temperature other than 0 is not built")
    if chunk_length not in (None, vf.CHUNK_LENGTH_S):
        raise NotImplementedError(f"chunk_length {chunk_length!r}: this build cuts 30 s chunks (None or 30)")
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, not {batch_size!r}")
    tk = engine.tokenizer
    dev = engine.device
    clock = dict(vad_rule=0.0, chunking=0.0, text=0.0)
    audios = [np.ascontiguousarray(a, dtype=np.float32) for a in audios]
    clips = list(clip_timestamps) if clip_timestamps is not None else [None] * len(audios)
    if len(clips) != len(audios):
        raise ValueError("clip_timestamps: None, or one entry (a list of clips or None) per file")
    n_vocab = getattr(getattr(engine, "cfg", None), "n_vocab", None)
    seed_tokens, hot_tokens = tr.encode_prompt(tk, initial_prompt, n_vocab), tr.encode_prompt(tk, hotwords, n_vocab)
    streams = [tr._Stream(content_frames=0) for _ in audios]
    for st in streams:
        st.all_tokens.extend(seed_tokens)
        st.hotwords = list(hot_tokens)
    ml = bool(getattr(tk, "multilingual", False))
    if ml:
        if task not in TASKS:
            raise ValueError(f"unknown task {task!r}: one of {TASKS}")
        if language_detection_segments < 1:
            raise ValueError("language_detection_segments must be >= 1")
        codes = list(language) if isinstance(language, (list, tuple)) else [language] * len(streams)
        if len(codes) != len(streams):
            raise ValueError("language: one code (or None) per file")
        for st, code in zip(streams, codes):
            st.task = task
            if code is None:
                st.language_pending = True
            else:
                st.language = code
                st.sot_sequence = tk.sot_sequence_for(code, task)   # ValueError: unknown code
    # the prompt's length is known before any GPU work (every start sequence has one length)
    proto = tr._Stream(content_frames=0)
    proto.all_tokens, proto.hotwords = list(seed_tokens), list(hot_tokens)
    cut = max_length           # what _Stream.prompt cuts the hotwords / initial_prompt by
    first = batched_prompt(tk, proto, cut, tk.sot_sequence, without_timestamps)
    if max_new_tokens is not None:
        if int(max_new_tokens) != max_new_tokens or max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be an integer >= 1, not {max_new_tokens!r}")
        limit = getattr(getattr(engine, "cfg", None), "n_text_ctx", 448)
        if len(first) + max_new_tokens > limit:
            raise ValueError(f"the prompt ({len(first)} tokens) and max_new_tokens {max_new_tokens} exceed "
                             f"the model's {limit} positions")
        max_length = len(first) + int(max_new_tokens)
    if len(first) >= max_length:
        raise ValueError(f"the prompt (initial_prompt / hotwords and the start sequence) leaves no "
                         f"position to sample within max_length {max_length}")
    # chunks that need no gate first: the RuntimeError comes before anything is uploaded
    t0 = time.perf_counter()
    spans = [None] * len(audios)
    for i, (a, cl) in enumerate(zip(audios, clips)):
        if cl is not None:
            spans[i] = vf.clip_chunks(cl, len(a))
        elif not vad_filter:
            spans[i] = vf.whole_file_chunk(len(a))
    clock["chunking"] += time.perf_counter() - t0
    offs = np.zeros(len(audios) + 1, np.int64)
    offs[1:] = np.cumsum([len(a) for a in audios])
    pcm = torch.from_numpy(np.concatenate(audios + [np.zeros(1, np.float32)])).to(dev)
    opts = None
    if any(s is None for s in spans):
        # ONE gate call over the uploaded buffer (the files with clips ride along unused)
        opts = vf.batched_vad_options(vad_parameters)
        probs = vf.speech_probabilities_device(pcm, offs, vad)
        t0 = time.perf_counter()
        speeches = {i: vf.get_speech_timestamps(probs[i], len(audios[i]), opts)
                    for i in range(len(audios)) if spans[i] is None}
        clock["vad_rule"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        for i, sp in speeches.items():
            spans[i] = vf.merge_segments(sp)
        clock["chunking"] += time.perf_counter() - t0
    chunks = [file_chunks(sp, i) for i, sp in enumerate(spans)]
    results = [FileResult([], ch, len(a) / SAMPLE_RATE, sum(c.end - c.start for c in ch) / SAMPLE_RATE,
                          opts if clips[i] is None and vad_filter else None)
               for i, (a, ch) in enumerate(zip(audios, chunks))]
    per = int(batch_size)
    if beam_size > 1:
        # a chunk's beams are rows of one decode call, capped like generate_segments' windows
        per = max(1, min(per, tr.fallback_rows(engine) // beam_size))
    order = [c for ch in chunks for c in ch]
    rounds = []
    ts_kw = dict(timestamps=False, no_speech_back=len(tk.sot_sequence)) if without_timestamps else {}
    for r0 in range(0, len(order), per):
        grp = order[r0:r0 + per]
        rounds.append(len(grp))
        mel = chunk_features(engine, pcm, [(offs[c.file] + c.start, offs[c.file] + c.end) for c in grp])
        enc = engine.encode(mel)
        if ml:
            need = [j for j, c in enumerate(grp) if multilingual or streams[c.file].language_pending]
            lp = None
            if need:
                lp, _ = engine.detect_language(enc if len(need) == len(grp) else enc[need].contiguous())
                lp = np.asarray(lp.cpu() if hasattr(lp, "cpu") else lp, np.float32)
            row = {j: k for k, j in enumerate(need)}
            for j, c in enumerate(grp):
                st = streams[c.file]
                if st.language_pending:
                    st.vote_language(tk, lp[row[j]], language_detection_segments, language_detection_threshold,
                                     last=c.index + 1 == len(chunks[c.file]))
                c.language = st.language
                if multilingual:
                    c.language = tk.languages[int(np.argmax(lp[row[j]]))]
        sots = [tk.sot_sequence_for(c.language, task) if ml else tk.sot_sequence for c in grp]
        prompts = [batched_prompt(tk, streams[c.file], cut, q, without_timestamps) for c, q in zip(grp, sots)]
        if beam_size > 1:
            out = engine.decode_beam(enc, prompts=prompts, beam_size=beam_size, length_penalty=length_penalty,
                                     max_length=max_length, **ts_kw)
        else:
            out = engine.decode_ex(enc, prompts=prompts, max_length=max_length, **ts_kw, **dec_kw)
        rows = out.rows()          # (waits for the decode)
        t0 = time.perf_counter()
        subs = []
        for c, p, (toks, avg_lp, nsp) in zip(grp, prompts, rows):
            c.tokens, c.avg_logprob, c.no_speech_prob, c.prompt = list(toks), float(avg_lp), float(nsp), p
            t_start, t_end = c.start / SAMPLE_RATE, c.end / SAMPLE_RATE
            if without_timestamps:
                subs.append([dict(start=t_start, end=t_end, tokens=c.tokens)])
            else:
                size = int(math.ceil(t_end - t_start)) * 100
                segs, _ = tr.split_window(tk, c.tokens, 0, size, time_offset=t_start)
                subs.append([dict(start=a, end=b, tokens=part) for a, b, part in segs])
        clock["text"] += time.perf_counter() - t0
        if word_timestamps:
            sizes = [c.content_frames for c in grp]
            texts = [[t for d in cur for t in d["tokens"] if t < tk.eot] if size >= 2 else []
                     for cur, size in zip(subs, sizes)]
            al_kw = dict(sot_sequences=sots) if ml else {}
            al = engine.align(enc, texts, sizes, enc_index=list(range(len(grp))), **al_kw)
            t0 = time.perf_counter()
            for c, cur, text, a in zip(grp, subs, texts, al):
                st = streams[c.file]
                st.last_speech_timestamp = tr.add_word_timestamps(
                    tk, cur, tr.find_alignment(tk, text, a, c.language if ml else None), 0,
                    st.last_speech_timestamp, prepend_punctuations, append_punctuations,
                    time_offset=c.start / SAMPLE_RATE)
            clock["text"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        for c, cur in zip(grp, subs):
            ratio = tr.compression_ratio(tk.decode(c.tokens).strip())
            segments = results[c.file].segments
            for d in cur:
                txt = tk.decode(d["tokens"])
                if d["start"] == d["end"] or not txt.strip():
                    continue
                words = [tr.Word(w["start"], w["end"], w["word"], w["probability"]) for w in d["words"]] \
                    if word_timestamps else None
                segments.append(tr.Segment(len(segments), c.start // tr.HOP, d["start"], d["end"], txt,
                                           list(d["tokens"]), 0.0, c.avg_logprob, ratio, c.no_speech_prob,
                                           False, words))
        clock["text"] += time.perf_counter() - t0
    for res, st in zip(results, streams):
        res.language, res.language_probability = st.language, st.language_probability
        res.all_language_probs = st.all_language_probs
    if stats is not None:
        stats.update(clock, rounds=rounds)
    return results


class BatchedInferencePipeline:
    """faster-whisper's BatchedInferencePipeline over a WhisperModel of this package: one long
    recording decoded as a batch of its speech chunks (generate_segments_batched)."""

    def __init__(self, model):
        self.model = model

    def transcribe(self, audio, language: str = None, task: str = "transcribe", log_progress: bool = False,
                   beam_size: int = 1, best_of: int = tr.BEST_OF, patience: float = 1,
                   length_penalty: float = 1.0, repetition_penalty: float = 1, no_repeat_ngram_size: int = 0,
                   temperature=tr.TEMPERATURES, compression_ratio_threshold=tr.COMPRESSION_RATIO_THRESHOLD,
                   log_prob_threshold=tr.LOG_PROB_THRESHOLD, no_speech_threshold=tr.NO_SPEECH_THRESHOLD,
                   initial_prompt=None, prefix=None, suppress_tokens=(-1,), without_timestamps: bool = True,
                   word_timestamps: bool = False, prepend_punctuations: str = tr.PREPEND_PUNCTUATIONS,
                   append_punctuations: str = tr.APPEND_PUNCTUATIONS, multilingual: bool = False,
                   vad_filter: bool = True, vad_parameters=None, max_new_tokens: int = None,
                   chunk_length: int = None, clip_timestamps=None, hallucination_silence_threshold=None,
                   batch_size: int = 64, hotwords=None, language_detection_threshold: float = 0.5,
                   language_detection_segments: int = 1, max_length: int = 448, **_ignored):
        """faster-whisper's batched transcribe: ``audio`` a WAV path or a 16 kHz array ->
        (iterator of Segment, TranscriptionInfo). The chunks come from ``clip_timestamps``
        ((start_s, end_s) pairs or {"start", "end"} dicts in seconds) when given, else from the
        speech gate (``vad_filter``, the default: the model's silero weights when present, the
        documented energy stand-in otherwise; ``vad_parameters`` None means
        min_silence_duration_ms 160, and max_speech_duration_s is always the chunk length), else
        the audio is one chunk when it is at most 30 s (RuntimeError when longer).
        ``info.duration_after_vad`` is the sum of the chunk lengths, ``info.vad_options`` the
        options the gate ran under (None without it).

        ``beam_size`` defaults to 1 like this package's WhisperModel.transcribe (faster-whisper's
        default is 5); 1 .. 8 run. ``without_timestamps`` (default True), ``word_timestamps``,
        ``max_new_tokens``, ``multilingual``, ``batch_size``, ``initial_prompt``, ``hotwords``,
        the penalties and ``suppress_tokens``: generate_segments_batched. ``max_length``: the
        decoder's token limit per chunk (448), as in WhisperModel.transcribe.

        Not built, refused by name before any GPU work (NotImplementedError): ``chunk_length``
        other than None / 30, ``prefix``, ``patience`` other than 1,
        ``hallucination_silence_threshold``, a first ``temperature`` other than 0.
        ``log_progress``, ``best_of`` and the three thresholds are accepted and unused: this
        mode decodes once at T = 0 and applies no gate."""
        m = self.model
        check_beam_args(beam_size, length_penalty, patience)
        check_decoder_compute_beam(getattr(m, "decoder_compute", "float16"), beam_size)
        check_history_args(repetition_penalty, no_repeat_ngram_size, beam_size)
        check_family_features(getattr(m.engine, "cfg", None), beam_size, word_timestamps,
                              getattr(m.engine, "alignment_heads", None))
        if chunk_length not in (None, vf.CHUNK_LENGTH_S):
            raise NotImplementedError(f"chunk_length {chunk_length!r}: this build cuts 30 s chunks (None or 30)")
        if prefix is not None:
            raise NotImplementedError("prefix is not supported")
        if hallucination_silence_threshold is not None:
            raise NotImplementedError("hallucination_silence_threshold is not supported")
        m._check_language(language, task)
        audio = m._load_audio(audio)
        use_vad = bool(vad_filter) and not clip_timestamps
        res = generate_segments_batched(
            m.engine, [audio], batch_size=batch_size, max_length=max_length, max_new_tokens=max_new_tokens,
            temperatures=temperature, beam_size=beam_size, length_penalty=length_penalty,
            repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
            suppress_tokens=suppress_tokens, initial_prompt=initial_prompt, hotwords=hotwords,
            without_timestamps=bool(without_timestamps), word_timestamps=bool(word_timestamps),
            prepend_punctuations=prepend_punctuations, append_punctuations=append_punctuations,
            language=language, task=task, multilingual=bool(multilingual),
            language_detection_segments=language_detection_segments,
            language_detection_threshold=language_detection_threshold, vad_filter=use_vad,
            vad_parameters=vad_parameters, vad=m._vad() if use_vad else None,
            clip_timestamps=[clip_timestamps] if clip_timestamps else None, chunk_length=chunk_length)[0]
        m.stats["windows"] += len(res.chunks)
        info = tr.TranscriptionInfo(res.language, res.language_probability, res.duration,
                                    res.all_language_probs, res.duration_after_vad, res.vad_options)
        return iter(res.segments), info


__all__ = ["BatchedInferencePipeline", "generate_segments_batched", "chunk_features", "batched_prompt",
           "file_chunks", "Chunk", "FileResult", "PACK_MAX"]
