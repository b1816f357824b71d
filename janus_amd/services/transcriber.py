"""Speech-to-text — drop-in for backend/services/transcriber.py on MI355X.

``Transcriber`` keeps the reference's constructor and methods (transcriber.py:11-91) and
even its body: it builds ``WhisperModel(model_size, device='cpu', compute_type='int8')``
and iterates ``model.transcribe(audio[::3], beam_size=1, language='en')`` segments. Here
``WhisperModel`` is the GPU engine (log-mel, encoder and greedy decoder in
libjanus_hip.so) behind faster-whisper's call shape (``transcribe`` returns
``(segments, info)``; segments carry ``.text`` and the decode statistics), so
module-level patching of ``WhisperModel`` in tests works exactly as in the reference
suite (backend/tests/test_input_processing.py:73-90).

``transcribe`` restates faster-whisper's ``generate_segments`` loop for the reference's
call (beam_size=1, language='en', every other option at its default):

* windows of 3000 log-mel frames at a moving ``seek``; the next seek is the end of the
  window when the tokens end in a single timestamp or hold none, else the last
  consecutive-timestamp pair (the trailing partial segment is re-decoded from there);
* ``condition_on_previous_text``: each window's prompt is ``<|startofprev|>`` + the
  last <= 223 tokens of the segments emitted so far + ``<|startoftranscript|>``;
* the gates, computed per window: ``avg_logprob`` = sum of chosen-token log-probs /
  (tokens + 1), ``compression_ratio`` = len(text) / len(zlib(text)),
  ``no_speech_prob`` = raw P(<|nocaptions|>) at the first step (on the GPU);
  no-speech skip when no_speech_prob > 0.6 and avg_logprob <= -1;
* segments whose start equals their end or whose text is blank are dropped.

* the temperature FALLBACK (``generate_with_fallback``): a window whose gates fail
  (compression ratio > 2.4 or avg_logprob < -1, outside the no-speech case) is re-decoded
  at T = 0.2, 0.4, ... 1.0 with best_of = 5 sampled hypotheses (the best by
  sum-log-prob / length kept, as CTranslate2 orders them) until one passes; when none
  does, the result with the highest avg_logprob among those under the compression
  threshold (else among all) is kept and reported at T = 1.0; a final temperature above
  ``prompt_reset_on_temperature`` (0.5) resets the conditioning prompt. The hypotheses of
  all failing windows of a round are decoded as one GPU batch (``janus_whisper_decode_
  sample_ex``: Gumbel-max over the rule-filtered logits / T). Sampling noise comes from
  a counter-based hash seeded per (utterance, window, temperature, hypothesis)
  (``fallback_seed``), so a run is reproducible and the CPU oracle draws the same noise —
  CTranslate2's own random draws cannot be reproduced offline.

Multilingual models (tiny / base / small): ``language`` is a code, or None to detect it on
the GPU (``WhisperEngine.detect_language`` over the first window's encoder output, which the
first round computes anyway; ``language_detection_segments`` / ``_threshold`` as in
faster-whisper), ``task`` is "transcribe" or "translate"; each utterance's prompt ends in its
own [sot, <|language|>, <|task|>]. On ``*.en`` models none of this runs.

A window that would not advance the seek (a leading <|0.00|><|0.00|>) advances by the
window size, so the loop always terminates.

Features are faster-whisper's: one log-mel of the whole clip (normalised with the maximum
over all its frames), from which each window takes the content frames
[seek, seek + min(3000, content - seek)) and is padded with zeros to 3000 frames
(``features[:, seek:seek + segment_size]`` + ``pad_or_trim``).
"""
import dataclasses
import os
import zlib

import numpy as np
import torch

from .. import _native as nat
from ..audio import decode_audio
from ..common import wavio
from ..tokenizer import LANGUAGES, SOT_PREV, TASKS
from ..whisper import (CONFIGS, WhisperEngine, check_beam_args, check_decoder_compute_beam, check_encoder_compute,
                       check_family_features, check_history_args, cross_compute_mode, decoder_compute_mode,
                       resolve_model,
                       resolve_suppress_tokens, shared_rows_in_place)
from . import vad_filter as vf

WINDOW_16K = 480000
N_FRAMES = 3000          # log-mel frames per window (hop 160 @ 16 kHz)
HOP = 160
TIME_PRECISION = 0.02    # seconds per timestamp step
INPUT_STRIDE = 2         # mel frames per timestamp step
COMPRESSION_RATIO_THRESHOLD = 2.4
LOG_PROB_THRESHOLD = -1.0
NO_SPEECH_THRESHOLD = 0.6
TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)   # faster-whisper transcribe(temperature=...)
BEST_OF = 5
PROMPT_RESET_ON_TEMPERATURE = 0.5
FALLBACK_ROWS = 320      # hypotheses per sampling decode (64 windows x 5: one decode per
                         # temperature for a 64-window round; the windows' encoder outputs are
                         # shared by their hypotheses through enc_index)
FALLBACK_ROWS_GATHER = 60  # the same for models without a shared-row cross-attention kernel
                           # (whisper.shared_rows_in_place): one encoder copy per row


def fallback_rows(engine) -> int:
    """Rows of one sampled decode call on this engine's model: FALLBACK_ROWS where rows
    sharing an encoder row read it in place (tiny.en / base.en PAIR blocks),
    FALLBACK_ROWS_GATHER where every row gets its own encoder copy (the 768-wide 12-head
    family by measurement, DESIGN.md §5i, and any wider model). An engine without a ``cfg``
    (a test stub) counts as in place."""
    return FALLBACK_ROWS if shared_rows_in_place(getattr(engine, "cfg", None)) else FALLBACK_ROWS_GATHER


def _mix32(h: int) -> int:
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def fallback_seed(utt: int, window: int, temp_index: int, hyp: int) -> int:
    """uint32 noise seed of one sampled hypothesis: utterance (index in the call), window
    (counter within the utterance), temperature index (1..5), hypothesis (0..best_of-1)."""
    return _mix32(0x4A414E55 ^ _mix32(utt * 0x01000193 + window * 0x9E3779B1 +
                                      temp_index * 0x85EBCA77 + hyp))


@dataclasses.dataclass
class Word:
    """faster-whisper's Word: times in seconds from the start of the audio."""
    start: float
    end: float
    word: str
    probability: float


@dataclasses.dataclass
class Segment:
    id: int
    seek: int
    start: float
    end: float
    text: str
    tokens: list
    temperature: float
    avg_logprob: float
    compression_ratio: float
    no_speech_prob: float
    needs_fallback: bool = False   # the T = 0 decode failed its gates (fallback entered)
    words: list = None             # [Word] with word_timestamps=True, else None


@dataclasses.dataclass
class Candidate:
    """One decode result of a window (generate_with_fallback's decode_result)."""
    tokens: list
    avg_logprob: float
    no_speech_prob: float
    temperature: float
    text: str
    compression_ratio: float
    needs_fallback: bool


def candidate(tk, toks, avg_lp, nsp, temperature) -> Candidate:
    text = tk.decode(toks).strip()
    return Candidate(list(toks), float(avg_lp), float(nsp), float(temperature), text,
                     compression_ratio(text), gates(text, avg_lp, nsp)[0])


def best_hypothesis(rows):
    """CTranslate2's first hypothesis of a sampled best_of group: the highest score
    sum-log-prob / length (length_penalty 1; sequences without <|endoftext|>), the first on
    ties. rows: [(tokens, avg_logprob, nsp)] as DecodeOut.rows() gives them."""
    def score(r):
        toks, avg, _ = r
        return avg * (len(toks) + 1) / max(len(toks), 1)
    best = 0
    for i in range(1, len(rows)):
        if score(rows[i]) > score(rows[best]):
            best = i
    return rows[best]


def settle(results, temperatures=TEMPERATURES):
    """generate_with_fallback's choice over a window's results in temperature order: the
    first that passes its gates; if none does (every temperature tried), the highest
    avg_logprob among those under the compression-ratio threshold (else among all),
    reported at the last temperature. None while the fallback is still running."""
    for r in results:
        if not r.needs_fallback:
            return r
    if len(results) < len(temperatures):
        return None
    below = [r for r in results if not r.compression_ratio > COMPRESSION_RATIO_THRESHOLD]
    pool = below or results
    best = pool[0]
    for r in pool[1:]:
        if r.avg_logprob > best.avg_logprob:
            best = r
    return dataclasses.replace(best, temperature=float(temperatures[-1]))


@dataclasses.dataclass
class TranscriptionInfo:
    language: str
    language_probability: float
    duration: float
    # [(code, probability)] by descending probability when the language was detected; None
    # for a given language and for *.en models (as faster-whisper)
    all_language_probs: list = None
    # vad_filter: seconds of audio kept (= duration without the filter) and the VadOptions used
    duration_after_vad: float = None
    vad_options: object = None

    def __post_init__(self):
        if self.duration_after_vad is None:
            self.duration_after_vad = self.duration


read_wav_16k = wavio.read_wav_16k  # 16-bit PCM WAV -> f32 @ 16 kHz

# how WhisperModel brings a file to 16 kHz: the reference's rule, or decode_audio's filter
AUDIO_RESAMPLE = ("reference", "bandlimited")


def audio_resample_mode(name: str) -> str:
    if name not in AUDIO_RESAMPLE:
        raise ValueError(f"unsupported audio_resample {name!r}; one of {AUDIO_RESAMPLE}")
    return name

# faster-whisper's device / compute_type vocabulary (WhisperModel(model_size, device=...,
# compute_type=...)); every value names the SAME GPU engine here (see WhisperModel)
DEVICES = ("cpu", "cuda", "auto")
COMPUTE_TYPES = ("default", "auto", "int8", "int8_float32", "int8_float16", "int8_bfloat16",
                 "int16", "float16", "bfloat16", "float32")
# faster-whisper compute types whose linear layers are int8 (CTranslate2 quantisation types)
INT8_COMPUTE_TYPES = ("int8", "int8_float32", "int8_float16", "int8_bfloat16")


def resolve_compute_type(compute_type: str, apply_compute_type: bool = False):
    """(effective_compute_type, encoder_compute) of WhisperModel for a faster-whisper
    compute_type: ("int8_float16", "int8") when apply_compute_type is set and the type is one
    of INT8_COMPUTE_TYPES (int8 encoder linears, fp16 everything else), ("float16",
    "float16") in every other case. ValueError for a type faster-whisper does not know."""
    if compute_type not in COMPUTE_TYPES:
        raise ValueError(f"unsupported compute_type {compute_type!r}")
    if apply_compute_type and compute_type in INT8_COMPUTE_TYPES:
        return "int8_float16", "int8"
    return "float16", "float16"


def compression_ratio(text: str) -> float:
    """faster-whisper get_compression_ratio."""
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b))


def gates(text: str, avg_logprob: float, no_speech_prob: float):
    """(needs_fallback, no_speech_skip) for one T = 0 window, faster-whisper's rules."""
    needs = compression_ratio(text) > COMPRESSION_RATIO_THRESHOLD or avg_logprob < LOG_PROB_THRESHOLD
    if no_speech_prob > NO_SPEECH_THRESHOLD and avg_logprob < LOG_PROB_THRESHOLD:
        needs = False                      # silence: no fallback
    skip = no_speech_prob > NO_SPEECH_THRESHOLD and not avg_logprob > LOG_PROB_THRESHOLD
    return needs, skip


def split_window(tk, tokens, seek, segment_size, time_offset=None):
    """One window's tokens -> ([(start_s, end_s, tokens)], next seek) as faster-whisper's
    generate_segments slices them (timestamps included in the token lists). ``time_offset``:
    the seconds the window's times start at (None: the seek's, seek * 0.01; the batched call's
    chunks start between frames)."""
    tb = tk.timestamp_begin
    if time_offset is None:
        time_offset = seek * HOP / 16000.0
    single_ending = len(tokens) >= 2 and tokens[-2] < tb <= tokens[-1]
    consecutive = [i for i in range(1, len(tokens)) if tokens[i] >= tb and tokens[i - 1] >= tb]
    segs = []
    if consecutive:
        slices = list(consecutive)
        if single_ending:
            slices.append(len(tokens))
        last = 0
        for cur in slices:
            part = tokens[last:cur]
            segs.append((time_offset + (part[0] - tb) * TIME_PRECISION,
                         time_offset + (part[-1] - tb) * TIME_PRECISION, part))
            last = cur
        if single_ending:
            nseek = seek + segment_size
        else:
            nseek = seek + (tokens[last - 1] - tb) * INPUT_STRIDE
    else:
        duration = segment_size * HOP / 16000.0
        stamps = [t for t in tokens if t >= tb]
        if stamps and stamps[-1] != tb:
            duration = (stamps[-1] - tb) * TIME_PRECISION
        segs.append((time_offset, time_offset + duration, tokens))
        nseek = seek + segment_size
    if nseek <= seek:          # no progress (e.g. <|0.00|><|0.00|>): move on a window
        nseek = seek + segment_size
    return segs, nseek


# --------------------------------------------------------------- word timestamps
# faster-whisper 1.x find_alignment / merge_punctuations / add_word_timestamps over the
# path and token probabilities of WhisperEngine.align (include/janus.h rules 1 - 5 on the
# GPU; rules 6 - 8 here).
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
SENTENCE_END_MARKS = ".。!！?？"


def find_alignment(tk, text_tokens, alignment, language=None):
    """One window's words from its alignment (faster-whisper find_alignment after the
    CTranslate2 call): [dict(word, tokens, start, end, probability)], times in seconds from
    the window's start. ``alignment``: WhisperEngine.align's result for ``text_tokens`` (its
    text_indices / time_indices / token_probs); None or no text gives no words. ``language``
    (multilingual models): the utterance's code, which decides the word split."""
    if alignment is None or len(text_tokens) == 0:
        return []
    if language is None:
        words, word_tokens = tk.split_to_word_tokens(list(text_tokens) + [tk.eot])
    else:
        words, word_tokens = tk.split_to_word_tokens(list(text_tokens) + [tk.eot], language)
    if len(word_tokens) <= 1:
        return []
    boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    if len(boundaries) <= 1:
        return []
    text_indices = np.asarray(alignment.text_indices)
    time_indices = np.asarray(alignment.time_indices)
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    jump_times = time_indices[jumps] * TIME_PRECISION
    starts = jump_times[boundaries[:-1]]
    ends = jump_times[boundaries[1:]]
    probs = np.asarray(alignment.token_probs, np.float64)
    return [dict(word=w, tokens=list(t), start=float(st), end=float(en),
                 probability=float(np.mean(probs[i:j])))
            for w, t, st, en, i, j in zip(words, word_tokens, starts, ends, boundaries[:-1], boundaries[1:])]


def merge_punctuations(alignment, prepended=PREPEND_PUNCTUATIONS, appended=APPEND_PUNCTUATIONS):
    """faster-whisper merge_punctuations, in place: a word that is a space plus a prepended
    mark joins the word after it, an appended mark joins the word before it (unless that ends
    in a space); the emptied entry keeps its times with word "" and no tokens."""
    i, j = len(alignment) - 2, len(alignment) - 1
    while i >= 0:
        previous, following = alignment[i], alignment[j]
        if previous["word"].startswith(" ") and previous["word"].strip() in prepended:
            following["word"] = previous["word"] + following["word"]
            following["tokens"] = previous["tokens"] + following["tokens"]
            previous["word"] = ""
            previous["tokens"] = []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):
        previous, following = alignment[i], alignment[j]
        if not previous["word"].endswith(" ") and following["word"] in appended:
            previous["word"] = previous["word"] + following["word"]
            previous["tokens"] = previous["tokens"] + following["tokens"]
            following["word"] = ""
            following["tokens"] = []
        else:
            i = j
        j += 1


def add_word_timestamps(tk, segments, alignment, seek, last_speech_timestamp,
                        prepend_punctuations=PREPEND_PUNCTUATIONS,
                        append_punctuations=APPEND_PUNCTUATIONS, time_offset=None):
    """faster-whisper add_word_timestamps over ONE window: ``segments`` its sub-segments as
    dicts(start, end, tokens) (times absolute), updated in place with "words" ([dict(word,
    start, end, probability)], absolute times rounded to 0.01 s) and the start / end the word
    times move; ``alignment``: find_alignment's words of the window's concatenated text
    tokens. ``time_offset``: the seconds the alignment's times start at (None: seek * 0.01).
    Returns the new last_speech_timestamp."""
    if not segments:
        return last_speech_timestamp
    per_segment = [[t for t in seg["tokens"] if t < tk.eot] for seg in segments]
    durations = np.array([w["end"] - w["start"] for w in alignment])
    durations = durations[durations.nonzero()]
    median_duration = min(0.7, float(np.median(durations))) if len(durations) > 0 else 0.0
    max_duration = median_duration * 2
    if len(durations) > 0:       # truncate long words at sentence boundaries
        for i in range(1, len(alignment)):
            if alignment[i]["end"] - alignment[i]["start"] > max_duration:
                if alignment[i]["word"] in SENTENCE_END_MARKS:
                    alignment[i]["end"] = alignment[i]["start"] + max_duration
                elif alignment[i - 1]["word"] in SENTENCE_END_MARKS:
                    alignment[i]["start"] = alignment[i]["end"] - max_duration
    merge_punctuations(alignment, prepend_punctuations, append_punctuations)
    if time_offset is None:
        time_offset = seek * 0.01
    word_index = 0
    for seg, seg_tokens in zip(segments, per_segment):
        saved, words = 0, []
        while word_index < len(alignment) and saved < len(seg_tokens):
            timing = alignment[word_index]
            if timing["word"]:
                words.append(dict(word=timing["word"], start=round(time_offset + timing["start"], 2),
                                  end=round(time_offset + timing["end"], 2),
                                  probability=timing["probability"]))
            saved += len(timing["tokens"])
            word_index += 1
        if words:
            # the first and second word after a pause: at most twice the median duration
            if words[0]["end"] - last_speech_timestamp > median_duration * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            # prefer the segment-level start / end when the first / last word is too long
            if seg["start"] < words[0]["end"] and seg["start"] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median_duration, seg["start"]))
            else:
                seg["start"] = words[0]["start"]
            if seg["end"] > words[-1]["start"] and seg["end"] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median_duration, seg["end"])
            else:
                seg["end"] = words[-1]["end"]
            last_speech_timestamp = seg["end"]
        seg["words"] = words
    return last_speech_timestamp


def word_seek(segments, seek, nseek, single_timestamp_ending):
    """Rule 8: with word timestamps, a window that does not end in a single timestamp moves
    the next seek to the end of its last word, when that lies after the window's start."""
    if single_timestamp_ending:
        return nseek
    ends = [w["end"] for seg in segments for w in seg.get("words", [])]
    if ends and ends[-1] > seek * 0.01:
        return round(ends[-1] * 100)
    return nseek


def window_text_tokens(tk, tokens, seek, size):
    """The text tokens (< eot) a window's alignment runs over: those of all its sub-segments
    (split_window), concatenated."""
    segs, _ = split_window(tk, list(tokens), seek, size)
    return [t for (_, _, part) in segs for t in part if t < tk.eot]


def encode_prompt(tk, prompt, n_vocab: int = None):
    """faster-whisper's encoding of ``initial_prompt`` / ``hotwords``: a string becomes the
    tokens of " " + s.strip(), an iterable of token ids is taken as given; None: no tokens."""
    if prompt is None:
        return []
    if isinstance(prompt, str):
        return [int(t) for t in tk.encode_text(" " + prompt.strip())]
    ids = [int(t) for t in prompt]
    if any(t < 0 or (n_vocab is not None and t >= n_vocab) for t in ids):
        raise ValueError("prompt token ids outside the vocabulary")
    return ids


def decode_option_kwargs(repetition_penalty=1, no_repeat_ngram_size=0, suppress_tokens=(-1,)):
    """The decode_ex keywords of the options that differ from faster-whisper's defaults (none
    at the defaults: such a call is exactly the call without them)."""
    kw = {}
    if repetition_penalty != 1:
        kw["repetition_penalty"] = float(repetition_penalty)
    if no_repeat_ngram_size:
        kw["no_repeat_ngram_size"] = int(no_repeat_ngram_size)
    if suppress_tokens is not None and list(suppress_tokens) != [-1]:
        kw["suppress_tokens"] = [int(t) for t in suppress_tokens]
    return kw


class _Stream:
    """generate_segments state of one utterance."""

    def __init__(self, audio16k=None, content_frames=None):
        self.audio = audio16k
        self.content_frames = len(audio16k) // HOP if content_frames is None else int(content_frames)
        self.seek = 0
        self.all_tokens = []           # (seeded with initial_prompt's tokens)
        self.prompt_reset_since = 0
        self.hotwords = []             # hotwords' tokens: after <|startofprev|> in every window
        self.segments = []
        self.windows = self.fallbacks = self.skips = 0
        self.fallback_decodes = 0      # sampled decodes (temperature steps) run
        self.window_tokens = []        # the settled tokens of every window, in order
        self.window_rows = []          # every window's T = 0 decode: (tokens, avg_logprob, nsp)
        self.sampled = 0               # tokens sampled at T = 0 over every window (incl. eot)
        self.last_speech_timestamp = 0.0   # word timestamps: the end of the last segment with words
        self.window_seeks = []         # (seek, size, next seek) of every window, in order
        self.window_alignments = []    # word timestamps: every window's Alignment (None: none run)
        # multilingual models: the utterance's language (given or detected), its probability,
        # every language's probability [(code, p)] by descending p (detected only) and its
        # own start sequence [sot, <|language|>, <|task|>] (None: the tokenizer's)
        self.language = "en"
        self.language_probability = 1.0
        self.all_language_probs = None
        self.sot_sequence = None
        self.task = "transcribe"
        self.language_pending = False  # still to be detected (language=None)
        self.language_votes = []       # (code, probability) of every window examined so far
        # vad_filter: the speeches [(start, end)] in samples of the original audio that
        # ``audio`` was collected from (None: unfiltered) and the seconds of audio decoded
        self.speech_chunks = None
        self.duration_after_vad = None if audio16k is None else len(audio16k) / 16000.0

    def transcript(self):
        """transcribe_buffer's join of the segments (transcriber.py:59-64)."""
        return ' '.join(s.text.strip() for s in self.segments).strip()

    @property
    def active(self):
        return self.seek < self.content_frames

    def window_size(self):
        return min(N_FRAMES, self.content_frames - self.seek)

    def prompt(self, tk, max_length=448):
        """faster-whisper's get_prompt (no prefix): <|startofprev|>, the hotwords, the last
        max_length // 2 - 1 previous tokens — when there are hotwords or previous tokens —
        then the start sequence."""
        prev = self.all_tokens[self.prompt_reset_since:]
        hot = self.hotwords[:max_length // 2 - 1]
        p = ([getattr(tk, "sot_prev", SOT_PREV)] + hot + prev[-(max_length // 2 - 1):]) if (prev or hot) else []   # 223 at 448
        return p + list(self.sot_sequence if self.sot_sequence is not None else tk.sot_sequence)

    def vote_language(self, tk, probs, segments: int, threshold: float, last: bool):
        """faster-whisper's language detection over one more window's probabilities (f32
        [n_languages]): the window's winner settles the language at once when its
        probability exceeds ``threshold``; otherwise the next windows of the seek loop are
        examined too, up to ``segments`` (or the utterance's ``last`` window), and the
        majority of the per-window winners is taken, the earliest on ties, with the largest
        probability that language reached. Until then the windows decode with the majority so
        far. all_language_probs are those of the last window examined."""
        probs = np.asarray(probs, np.float64)
        i = int(np.argmax(probs))
        codes = getattr(tk, "languages", LANGUAGES)   # 99, or the large-v3 layout's 100
        self.language_votes.append((codes[i], float(probs[i])))
        order = np.argsort(-probs, kind="stable")
        self.all_language_probs = [(codes[int(k)], float(probs[int(k)])) for k in order]
        if probs[i] > threshold:
            self.language, self.language_probability = self.language_votes[-1]
            self.language_pending = False
        else:
            by = {}
            for code, p in self.language_votes:
                by.setdefault(code, []).append(p)
            self.language = max(by, key=lambda code: len(by[code]))   # first inserted on ties
            self.language_probability = max(by[self.language])
            self.language_pending = len(self.language_votes) < segments and not last
        self.sot_sequence = tk.sot_sequence_for(self.language, self.task)


def _fallback(engine, tk, enc, prompts, first, keys, max_length, temperatures, best_of,
              enc_rows=None, presampled=None, **dec_kw):
    """Run the temperature fallback for the windows of one round: first [Candidate] (T = 0
    results), keys [(utt, window)]; returns each window's settled Candidate. The
    hypotheses of every window still failing at a temperature go out as one sampled batch
    (chunks of FALLBACK_ROWS rows). ``enc_rows``: window j's encoder output is enc[enc_rows[j]]
    (default enc[j]). ``presampled[j][ti - 1]``: window j's best_of hypothesis rows at
    temperatures[ti], already decoded (generate_segments(speculative=True)): the walk keeps
    the same candidates the sequential decodes would give (rows are independent of their
    batch neighbours and every draw is keyed by (utt, window, ti, h))."""
    er = list(range(len(first))) if enc_rows is None else list(enc_rows)
    results = [[c] for c in first]
    final = [settle(r, temperatures) if not r[0].needs_fallback else None for r in results]
    if presampled is not None:
        for j in range(len(first)):
            for ti in range(1, len(temperatures)):
                if final[j] is not None:
                    break
                toks, avg_lp, nsp = best_hypothesis(presampled[j][ti - 1])
                results[j].append(candidate(tk, toks, avg_lp, nsp, float(temperatures[ti])))
                if not results[j][-1].needs_fallback or ti == len(temperatures) - 1:
                    final[j] = settle(results[j], temperatures)
        return final, [len(r) - 1 for r in results]
    # the shared-encoder PAIR path (H <= 8, d <= 512) reads each window's output in place;
    # wider models gather one encoder copy per hypothesis row (0.74 GB per 320 rows at
    # d = 768), so their sampled decodes stay at FALLBACK_ROWS_GATHER rows
    per = max(1, fallback_rows(engine) // best_of)
    for ti in range(1, len(temperatures)):
        T = float(temperatures[ti])
        pend = [j for j in range(len(first)) if final[j] is None]
        if not pend:
            break
        for c0 in range(0, len(pend), per):
            js = pend[c0:c0 + per]
            # the hypotheses of window j share its encoder output: no per-row copy, and the
            # cross-attention reads it once per pair of hypotheses (enc_index)
            rows_prompts = [prompts[j] for j in js for _ in range(best_of)]
            seeds = [fallback_seed(keys[j][0], keys[j][1], ti, h) for j in js for h in range(best_of)]
            out = engine.decode_ex(enc, prompts=rows_prompts, max_length=max_length,
                                   temperature=T, seeds=seeds,
                                   enc_index=[er[j] for j in js for _ in range(best_of)], **dec_kw).rows()
            for k, j in enumerate(js):
                toks, avg_lp, nsp = best_hypothesis(out[k * best_of:(k + 1) * best_of])
                results[j].append(candidate(tk, toks, avg_lp, nsp, T))
        for j in pend:
            if not results[j][-1].needs_fallback or ti == len(temperatures) - 1:
                final[j] = settle(results[j], temperatures)
    return final, [len(r) - 1 for r in results]


def settle_round(engine, tk, rows, prompts, keys, enc, max_length, temperatures=(0.0,),
                 best_of: int = BEST_OF, enc_rows=None, presampled=None, **dec_kw):
    """One round of generate_with_fallback: ``rows`` the T = 0 decode of the round's windows
    ([(tokens, avg_logprob, no_speech_prob)], DecodeOut.rows()), ``prompts`` / ``keys`` [(utt, window)] per window,
    ``enc`` the windows' encoder output (enc[enc_rows[j]] for window j). Returns (first,
    final, sampled decodes) per window: the T = 0 Candidate, the settled one, and the number
    of sampled re-decodes the fallback ran."""
    first = [candidate(tk, toks, avg_lp, nsp, 0.0) for (toks, avg_lp, nsp) in rows]
    if len(temperatures) > 1:
        final, ndec = _fallback(engine, tk, enc, prompts, first, keys, max_length, temperatures,
                                best_of, enc_rows=enc_rows, presampled=presampled, **dec_kw)
    else:
        final, ndec = first, [0] * len(first)
    return first, final, ndec


def advance(tk, s, size, c0, r, nd, sampled: int = 0, word_timestamps: bool = False, alignment=None,
            prepend_punctuations=PREPEND_PUNCTUATIONS, append_punctuations=APPEND_PUNCTUATIONS,
            condition_on_previous_text: bool = True,
            prompt_reset_on_temperature: float = PROMPT_RESET_ON_TEMPERATURE):
    """generate_segments' update of one utterance after its window [seek, seek + size) settled
    (c0: the T = 0 Candidate, r: the settled one, nd: sampled re-decodes, sampled: tokens the
    T = 0 decode emitted): the counters, the no-speech skip, the segments (start == end or
    blank text dropped), the next seek and the prompt reset. ``word_timestamps``: the
    window's sub-segments get their words from ``alignment`` (WhisperEngine.align over
    window_text_tokens) before they are filtered, and the seek follows rule 8."""
    s.windows += 1
    s.fallbacks += int(c0.needs_fallback)
    s.fallback_decodes += nd
    s.sampled += int(sampled)
    s.window_tokens.append(list(r.tokens))
    s.window_rows.append((list(c0.tokens), c0.avg_logprob, c0.no_speech_prob))
    # no-speech skip on the settled result (generate_segments after the fallback)
    if r.no_speech_prob > NO_SPEECH_THRESHOLD and not r.avg_logprob > LOG_PROB_THRESHOLD:
        s.skips += 1
        s.window_seeks.append((s.seek, size, s.seek + size))
        if word_timestamps:
            s.window_alignments.append(None)
        s.seek += size
        return
    segs, nseek = split_window(tk, r.tokens, s.seek, size)
    words = [None] * len(segs)
    if word_timestamps:
        toks = r.tokens
        single = len(toks) >= 2 and toks[-2] < tk.timestamp_begin <= toks[-1]
        cur = [dict(start=st, end=en, tokens=part) for (st, en, part) in segs]
        text = [t for d in cur for t in d["tokens"] if t < tk.eot]
        s.window_alignments.append(alignment)
        s.last_speech_timestamp = add_word_timestamps(
            tk, cur, find_alignment(tk, text, alignment,
                                    s.language if getattr(tk, "multilingual", False) else None),
            s.seek, s.last_speech_timestamp,
            prepend_punctuations, append_punctuations)
        nseek = word_seek(cur, s.seek, nseek, single)
        segs = [(d["start"], d["end"], d["tokens"]) for d in cur]
        words = [[Word(w["start"], w["end"], w["word"], w["probability"]) for w in d["words"]] for d in cur]
    for (st, en, part), ws in zip(segs, words):
        txt = tk.decode(part)
        if st == en or not txt.strip():
            continue
        s.all_tokens.extend(part)
        s.segments.append(Segment(len(s.segments), s.seek, st, en, txt, part,
                                  r.temperature, r.avg_logprob, r.compression_ratio,
                                  r.no_speech_prob, c0.needs_fallback, ws))
    s.window_seeks.append((s.seek, size, nseek))
    s.seek = nseek
    # condition_on_previous_text: a result settled above prompt_reset_on_temperature
    # restarts the prompt after these segments; without it every window does
    if not condition_on_previous_text or r.temperature > prompt_reset_on_temperature:
        s.prompt_reset_since = len(s.all_tokens)


def gather_windows(items, n_frames: int = N_FRAMES, device=None, n_mels: int = 80):
    """fp16 [len(items)][n_frames][n_mels]: item j = (features [B][F][n_mels] fp16 device tensor,
    row, seek, size) -> features[row, seek:seek + size] followed by zeros (faster-whisper's
    ``features[:, seek:seek + segment_size]`` + pad_or_trim). One index gather per distinct
    features tensor (a serving batch's windows come out of one [B][F][n_mels] tensor). The bin
    count is the features' own; ``n_mels`` (the model's cfg.n_mels) only shapes an empty result."""
    if not items:
        return torch.zeros(0, n_frames, n_mels, dtype=torch.float16, device=device)
    dev = items[0][0].device
    out = torch.zeros(len(items), n_frames, items[0][0].shape[-1], dtype=torch.float16, device=dev)
    t = torch.arange(n_frames, device=dev)
    groups = {}
    for j, (f, row, seek, size) in enumerate(items):
        groups.setdefault(id(f), (f, []))[1].append((j, int(row), int(seek), int(size)))
    for f, lst in groups.values():
        F = f.shape[1]
        if len(lst) == 1:
            j, row, seek, size = lst[0]
            n = max(0, min(size, F - seek, n_frames))
            if n > 0:
                out[j, :n] = f[row, seek:seek + n]
            continue
        # the four index vectors in one pinned host tensor, copied without blocking the host
        # (a pageable copy would wait for the stream: the serving step's encoder ahead of it)
        idx = torch.tensor([[r, sk, z, j] for j, r, sk, z in lst], dtype=torch.int64)
        if dev.type == "cuda":
            idx = idx.pin_memory().to(dev, non_blocking=True)
        rows, seeks, sizes, js = idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]
        src = seeks[:, None] + t[None, :]
        valid = (t[None, :] < sizes[:, None]) & (src < F)
        g = f[rows[:, None], torch.where(valid, src, 0)]          # [n][n_frames][n_mels]
        out[js] = torch.where(valid[..., None], g, torch.zeros((), dtype=g.dtype, device=dev))
    return out


def generate_segments(engine: WhisperEngine, audios, max_batch: int = 64, max_length: int = 448,
                      temperatures=TEMPERATURES, best_of: int = BEST_OF, utt_keys=None,
                      speculative: bool = False, beam_size: int = 1, length_penalty: float = 1.0,
                      word_timestamps: bool = False, prepend_punctuations: str = PREPEND_PUNCTUATIONS,
                      append_punctuations: str = APPEND_PUNCTUATIONS, language=None,
                      task: str = "transcribe", language_detection_segments: int = 1,
                      language_detection_threshold: float = 0.5, vad_filter: bool = False,
                      vad_parameters=None, vad=None, repetition_penalty: float = 1,
                      no_repeat_ngram_size: int = 0, suppress_tokens=(-1,), initial_prompt=None,
                      hotwords=None, condition_on_previous_text: bool = True,
                      prompt_reset_on_temperature: float = PROMPT_RESET_ON_TEMPERATURE):
    """faster-whisper's seek loop for several 16 kHz utterances at once: every round
    decodes the current window of each unfinished utterance as one GPU batch (per-row
    prompts), then the temperature fallback of the windows whose gates failed
    (``temperatures`` = (0.0,) disables it). ``utt_keys``: the utterance numbers the
    fallback seeds are keyed on (default: the index in ``audios``; a caller that batches
    the same utterances differently passes stable numbers to draw the same noise).
    ``speculative``: each round decodes every window's T = 0 row AND the best_of hypotheses
    of every fallback temperature in ONE call (per-row temperatures), then walks the
    temperatures exactly as the sequential fallback does — the same results for one decode
    call's latency instead of up to len(temperatures) in a row, at (1 + 5 x 5) rows per
    window (the streaming encoder's setting: a few phrases at a time, latency-bound).
    ``beam_size`` > 1 (up to 8; ``length_penalty`` > 0): the T = 0 decode of every window is
    the beam decode (engine.decode_beam, windows chunked so that windows x beam_size stays
    within one decode call's rows), as in faster-whisper; the fallback temperatures stay the
    sampled best_of decodes and the gates read the winner's sum_logprob / (n + 1). The
    speculative one-call form is greedy only.
    ``word_timestamps``: every settled window of a round that is not skipped as silence is
    aligned in ONE engine.align call (the windows share the round's encoder output through
    enc_index), its segments carry ``words`` and its seek follows rule 8 (include/janus.h,
    DESIGN.md §5l); ``prepend_punctuations`` / ``append_punctuations`` as in faster-whisper.
    Off (the default), no call and no result differs.
    ``language`` / ``task`` (multilingual engines only; on a ``*.en`` engine none of it runs):
    one code for every utterance, a list with one entry per utterance, or None to detect —
    then each round makes ONE engine.detect_language call over the encoder output it computed
    anyway, for the utterances still undecided (_Stream.vote_language: faster-whisper's
    ``language_detection_segments`` / ``language_detection_threshold`` rule); every stream
    carries its language, probability, all_language_probs and its own start sequence.
    ``vad_filter``: ONE whole-file speech-gate call over all utterances before the features
    (``vad``: a services.vad.SileroGate -> SileroGate.probs_file / janus_vad_probs; None: the
    documented energy stand-in janus_vad_energy over 512-sample windows), faster-whisper's
    speech-timestamp rule under ``vad_parameters`` (a dict or VadOptions), then
    each utterance is replaced by its collected speech (_Stream.speech_chunks,
    duration_after_vad), the seek loop runs on that and the segment and word times are
    restored onto the original audio. An utterance without speech yields no segments. Off
    (the default), no VAD call is made and nothing differs.
    ``repetition_penalty`` / ``no_repeat_ngram_size`` (the history rules, include/janus.h
    janus_decode_options) and ``suppress_tokens`` (faster-whisper's list) go to
    every decode of the loop: the T = 0 pass, the sampled fallback and the speculative call;
    with ``beam_size`` > 1 the two history rules raise NotImplementedError. ``initial_prompt``
    (a string or token ids) seeds every utterance's previous tokens, so it is trimmed and reset
    like previous text; ``hotwords`` (the same forms) follow <|startofprev|> in every window's
    prompt; ``condition_on_previous_text=False`` restarts the previous text after every
    window; ``prompt_reset_on_temperature`` is the temperature above which a settled window
    does. A prompt that leaves no position to sample is a ValueError. At the defaults no call
    and no result differs.
    Returns one _Stream (segments + gate counters) per utterance."""
    check_beam_args(beam_size, length_penalty)
    check_decoder_compute_beam(getattr(engine, "decoder_compute", "float16"), beam_size)
    check_family_features(getattr(engine, "cfg", None), beam_size, word_timestamps,
                          getattr(engine, "alignment_heads", None))
    check_history_args(repetition_penalty, no_repeat_ngram_size, beam_size)
    dec_kw = decode_option_kwargs(repetition_penalty, no_repeat_ngram_size, suppress_tokens)
    if "suppress_tokens" in dec_kw:   # (ValueError: an id outside the vocabulary, before any GPU work)
        resolve_suppress_tokens(engine.tokenizer, dec_kw["suppress_tokens"], engine.cfg.n_vocab)
        if beam_size > 1:
            raise NotImplementedError("suppress_tokens other than [-1] is not built for beam search")
    if beam_size > 1 and speculative:
        raise NotImplementedError("speculative=True decodes greedily in one call; beam_size > 1 "
                                  "needs speculative=False")
    temperatures = tuple(float(t) for t in temperatures)
    if not temperatures or temperatures[0] != 0.0:
        raise NotImplementedError("the first temperature must be 0 (faster-whisper's default)")
    tk = engine.tokenizer
    dev = engine.device
    audios = [np.asarray(a, np.float32) for a in audios]
    speeches = None
    if vad_filter:
        opts = vf.as_vad_options(vad_parameters)
        probs = vf.speech_probabilities(audios, dev, vad) if audios else []
        speeches = [vf.get_speech_timestamps(p, len(a), opts) for p, a in zip(probs, audios)]
        audios = [vf.collect_chunks(a, sp) for a, sp in zip(audios, speeches)]
    streams = [_Stream(a) for a in audios]
    n_vocab = getattr(getattr(engine, "cfg", None), "n_vocab", None)
    seed_tokens, hot_tokens = encode_prompt(tk, initial_prompt, n_vocab), encode_prompt(tk, hotwords, n_vocab)
    for st in streams:
        st.all_tokens.extend(seed_tokens)
        st.hotwords = list(hot_tokens)
    if speeches is not None:
        for st, sp in zip(streams, speeches):
            st.speech_chunks = sp
    multilingual = bool(getattr(tk, "multilingual", False))
    if multilingual:
        if task not in TASKS:
            raise ValueError(f"unknown task {task!r}: one of {TASKS}")
        if language_detection_segments < 1:
            raise ValueError("language_detection_segments must be >= 1")
        codes = list(language) if isinstance(language, (list, tuple)) else [language] * len(streams)
        if len(codes) != len(streams):
            raise ValueError("language: one code (or None) per utterance")
        for st, code in zip(streams, codes):
            st.task = task
            if code is None:
                st.language_pending = True
            else:
                st.language = code
                st.sot_sequence = tk.sot_sequence_for(code, task)   # ValueError: unknown code
    # the whole clip's features, once per utterance (faster-whisper's FeatureExtractor call)
    feats = []
    for st in streams:
        if st.content_frames <= 0:
            feats.append(None)
            continue
        pcm = torch.from_numpy(np.concatenate([st.audio, np.zeros(1, np.float32)])).to(dev)
        offs = torch.tensor([0, len(st.audio)], dtype=torch.int64, device=dev)
        feats.append(engine.logmel_frames(pcm, offs, 1, 1, st.content_frames))
    spec = speculative and len(temperatures) > 1
    per_row = 1 + (len(temperatures) - 1) * best_of          # rows per window, speculative
    if spec:
        # the same in-place-or-gather row cap as the sequential fallback (_fallback)
        max_batch = max(1, min(max_batch, fallback_rows(engine) // per_row))
    if beam_size > 1:
        # a window's beams are rows of one decode call, capped like the sampled hypotheses
        max_batch = max(1, min(max_batch, fallback_rows(engine) // beam_size))
    while True:
        act = [i for i, s in enumerate(streams) if s.active]
        if not act:
            break
        for c0 in range(0, len(act), max_batch):
            idx = act[c0:c0 + max_batch]
            grp = [streams[i] for i in idx]
            sizes = [s.window_size() for s in grp]
            mel = gather_windows([(feats[i], 0, s.seek, size) for i, s, size in zip(idx, grp, sizes)])
            enc = engine.encode(mel)
            pend = [j for j, s in enumerate(grp) if s.language_pending]
            if pend:
                lp, _ = engine.detect_language(enc if len(pend) == len(grp) else enc[pend].contiguous())
                lp = np.asarray(lp.cpu() if hasattr(lp, "cpu") else lp, np.float32)
                for k, j in enumerate(pend):
                    grp[j].vote_language(tk, lp[k], language_detection_segments, language_detection_threshold,
                                         last=grp[j].seek + sizes[j] >= grp[j].content_frames)
            prompts = [s.prompt(tk, max_length) for s in grp]
            if any(len(p) >= max_length for p in prompts):
                raise ValueError(f"the prompt (initial_prompt / hotwords / previous text and the start "
                                 f"sequence) leaves no position to sample within max_length {max_length}")
            keys = [(i if utt_keys is None else int(utt_keys[i]), s.windows) for i, s in zip(idx, grp)]
            pres = None
            if spec:
                temps, seeds, eidx, rprom = [], [], [], []
                for j, key in enumerate(keys):
                    temps.append(0.0)
                    seeds.append(0)
                    for ti in range(1, len(temperatures)):
                        temps += [float(temperatures[ti])] * best_of
                        seeds += [fallback_seed(key[0], key[1], ti, h) for h in range(best_of)]
                    eidx += [j] * per_row
                    rprom += [prompts[j]] * per_row
                out = engine.decode_ex(enc, prompts=rprom, max_length=max_length, temperature=temps,
                                       seeds=seeds, enc_index=eidx, **dec_kw)
                allr = out.rows()
                t0 = [allr[j * per_row] for j in range(len(grp))]
                pres = [[allr[j * per_row + 1 + (ti - 1) * best_of: j * per_row + 1 + ti * best_of]
                         for ti in range(1, len(temperatures))] for j in range(len(grp))]
                n_tok = out.n_tokens.cpu().numpy()[0::per_row]
            else:
                if beam_size > 1:
                    out = engine.decode_beam(enc, prompts=prompts, beam_size=beam_size,
                                             length_penalty=length_penalty, max_length=max_length)
                else:
                    out = engine.decode_ex(enc, prompts=prompts, max_length=max_length, **dec_kw)
                t0 = out.rows()
                n_tok = out.n_tokens.cpu().numpy()
            first, final, ndec = settle_round(engine, tk, t0, prompts, keys, enc, max_length,
                                              temperatures, best_of, presampled=pres, **dec_kw)
            reset_kw = {}
            if not condition_on_previous_text or prompt_reset_on_temperature != PROMPT_RESET_ON_TEMPERATURE:
                reset_kw = dict(condition_on_previous_text=bool(condition_on_previous_text),
                                prompt_reset_on_temperature=float(prompt_reset_on_temperature))
            if not word_timestamps:
                for s, size, c0r, r, nd, nt in zip(grp, sizes, first, final, ndec, n_tok):
                    advance(tk, s, size, c0r, r, nd, nt, **reset_kw)
                continue
            texts = [[] if (r.no_speech_prob > NO_SPEECH_THRESHOLD and not r.avg_logprob > LOG_PROB_THRESHOLD)
                     else window_text_tokens(tk, r.tokens, s.seek, size)
                     for s, size, r in zip(grp, sizes, final)]
            if multilingual:   # every window's own start sequence in front of its text
                al = engine.align(enc, texts, sizes, enc_index=list(range(len(grp))),
                                  sot_sequences=[s.sot_sequence for s in grp])
            else:
                al = engine.align(enc, texts, sizes, enc_index=list(range(len(grp))))
            for s, size, c0r, r, nd, nt, a in zip(grp, sizes, first, final, ndec, n_tok, al):
                advance(tk, s, size, c0r, r, nd, nt, True, a, prepend_punctuations, append_punctuations,
                        **reset_kw)
    for st in streams:
        if st.speech_chunks:   # times on the collected speech -> times on the original audio
            st.segments = vf.restore_speech_timestamps(st.segments, vf.SpeechTimestampsMap(st.speech_chunks))
    return streams


class WhisperModel:
    """faster-whisper-shaped front of the GPU Whisper engine.

    Accepts faster-whisper's constructor arguments, including the reference's
    ``device='cpu', compute_type='int8'`` (transcriber.py:23-27), and maps every
    combination onto the engine this build has: the gfx950 HIP kernels on the current
    device. Both arguments are recorded (``requested_device`` / ``requested_compute_type``).
    ``device`` selects nothing: there is no CPU path (the product fails loudly without a
    GPU).

    ``compute_type`` selects the encoder's compute type, and only when the caller passes
    ``apply_compute_type=True``: then ``int8``, ``int8_float16``, ``int8_float32`` and
    ``int8_bfloat16`` run the encoder's linear layers (QKV, out_proj, fc1, fc2) in int8 on
    the i8 MFMA with CTranslate2's row-wise symmetric quantisation, and every other accepted
    value runs them in fp16. The conv stem, attention, LayerNorms and the whole decoder are
    fp16 weights on MFMA with fp32 accumulation whatever ``compute_type`` says (DESIGN.md §5j;
    the decoder's weights have their own keyword, ``decoder_compute``, below). With the
    default ``apply_compute_type=False`` every ``compute_type`` runs fp16 — what
    ``Transcriber`` gets, whose parity tests against the fp32 oracle depend on it.
    ``effective_compute_type`` reports what runs: ``"float16"`` or ``"int8_float16"``.

    ``cross_compute="int8"`` (opt-in, independent of ``compute_type``) is passed to the engine:
    every decode call quantises its encoder rows per key to int8 and the decoder's
    cross-attention streams those (WhisperEngine); the word alignment and the
    language detection keep the fp16 rows. ValueError for any other name but ``"float16"``.

    ``decoder_compute="int8"`` (opt-in, its own keyword: ``compute_type`` keeps meaning what it
    means above) is passed to the engine: every decoder linear layer and the vocabulary
    projection multiply int8 weights (WhisperEngine). ``beam_size`` > 1 is then a
    NotImplementedError before any GPU work. ValueError for any other name but ``"float16"``.

    ``audio_resample`` says how a file (a path, a PathLike, an open binary file or bytes)
    becomes 16 kHz audio: ``"reference"`` (the default) is ``read_wav_16k``, the reference's
    ``[::3]`` at 48 kHz and linear interpolation elsewhere; ``"bandlimited"`` is
    ``janus_amd.audio.decode_audio``. ValueError for any other name. Arrays
    are taken as 16 kHz audio either way."""

    def __init__(self, model_size: str, device: str = "auto", compute_type: str = "default",
                 *, apply_compute_type: bool = False, vad_weights: dict = None, alignment_heads=None,
                 cross_compute: str = "float16", audio_resample: str = "reference",
                 decoder_compute: str = "float16", **_ignored):
        cross_compute_mode(cross_compute)   # ValueError: unknown name
        decoder_compute_mode(decoder_compute)   # ValueError: unknown name
        self.decoder_compute = decoder_compute
        self._audio_resample = audio_resample_mode(audio_resample)   # ValueError: unknown name
        model_size = resolve_model(model_size)   # ValueError: unknown; "turbo" -> "large-v3-turbo"
        if device not in DEVICES:
            raise ValueError(f"unsupported device {device!r}; one of {DEVICES}")
        self.effective_compute_type, enc_compute = resolve_compute_type(compute_type, apply_compute_type)
        self.model_size = model_size
        self.requested_device, self.requested_compute_type = device, compute_type
        check_encoder_compute(CONFIGS[model_size], enc_compute)   # NotImplementedError: int8 at 1280
        # alignment_heads: [(layer, head)] for word_timestamps instead of the default set (needed where
        # that set exceeds the alignment pass's 64 heads: medium.en's has 192)
        kw = {} if alignment_heads is None else {"alignment_heads": alignment_heads}
        if cross_compute != "float16":
            kw["cross_compute"] = cross_compute
        if decoder_compute != "float16":
            kw["decoder_compute"] = decoder_compute
        self.engine = WhisperEngine(CONFIGS[model_size], encoder_compute=enc_compute, **kw)
        self.stats = {"windows": 0, "needs_fallback": 0, "no_speech_skips": 0, "fallback_decodes": 0}
        # vad_filter: silero weights (default: JANUS_VAD_DIR; none: the energy stand-in); the
        # gate is created on the first transcribe(vad_filter=True)
        self._vad_weights = vad_weights
        self._vad_gate = None

    def _vad(self):
        """The SileroGate of vad_filter=True, or None for the energy stand-in."""
        if self._vad_gate is None:
            from .vad import SileroGate, load_weights
            w = self._vad_weights if self._vad_weights is not None else load_weights()
            if w is not None:
                self._vad_gate = SileroGate(w)
        return self._vad_gate

    @property
    def audio_resample(self) -> str:
        return getattr(self, "_audio_resample", "reference")

    def _load_audio(self, audio):
        """What transcribe, detect_language and BatchedInferencePipeline.transcribe make of
        ``audio``: a path, a PathLike, an open binary file or bytes is read and brought to
        16 kHz under ``audio_resample``; anything else is an array of 16 kHz samples."""
        if isinstance(audio, (str, os.PathLike, bytes, bytearray, memoryview)) or hasattr(audio, "read"):
            if self.audio_resample == "bandlimited":
                audio = decode_audio(audio)
            else:
                audio = read_wav_16k(os.fspath(audio) if isinstance(audio, os.PathLike) else audio)
        return np.ascontiguousarray(audio, dtype=np.float32)

    @property
    def is_multilingual(self) -> bool:
        return bool(getattr(getattr(self.engine, "tokenizer", None), "multilingual", False))

    @property
    def supported_languages(self):
        """faster-whisper's supported_languages: the 99 codes (100 on the large-v3 family), or
        ["en"] for a ``*.en`` model."""
        tk = self.engine.tokenizer
        return list(getattr(tk, "languages", LANGUAGES)) if self.is_multilingual else ["en"]

    def _check_language(self, language, task):
        """``*.en``: English transcription only (NotImplementedError, as before the
        multilingual models); multilingual: ValueError for an unknown code or task."""
        if not self.is_multilingual:
            if language not in (None, "en") or task != "transcribe":
                raise NotImplementedError("*.en models transcribe English only (transcriber.py:56)")
            return
        if task not in TASKS:
            raise ValueError(f"unknown task {task!r}: one of {TASKS}")
        if language is not None:
            self.engine.tokenizer.language_token(language)

    def detect_language(self, audio, language_detection_segments: int = 1,
                        language_detection_threshold: float = 0.5):
        """faster-whisper's detect_language: (language, probability, all_language_probs) of
        16 kHz ``audio`` (or a WAV path) from its first ``language_detection_segments``
        30 s windows (one encode and one WhisperEngine.detect_language call over them).
        ValueError on a ``*.en`` model."""
        if not self.is_multilingual:
            raise ValueError(f"detect_language: {self.model_size} is English-only")
        if language_detection_segments < 1:
            raise ValueError("language_detection_segments must be >= 1")
        audio = self._load_audio(audio)
        eng, st = self.engine, _Stream(audio)
        if st.content_frames <= 0:
            raise ValueError("detect_language: empty audio")
        pcm = torch.from_numpy(np.concatenate([audio, np.zeros(1, np.float32)])).to(eng.device)
        offs = torch.tensor([0, len(audio)], dtype=torch.int64, device=eng.device)
        feats = eng.logmel_frames(pcm, offs, 1, 1, st.content_frames)
        seeks = list(range(0, st.content_frames, N_FRAMES))[:language_detection_segments]
        mel = gather_windows([(feats, 0, sk, min(N_FRAMES, st.content_frames - sk)) for sk in seeks])
        probs, _ = eng.detect_language(eng.encode(mel))
        probs = probs.cpu().numpy()
        for k in range(len(seeks)):
            st.vote_language(eng.tokenizer, probs[k], len(seeks), language_detection_threshold,
                             last=k + 1 == len(seeks))
            if not st.language_pending:
                break
        return st.language, st.language_probability, st.all_language_probs

    def transcribe(self, audio, beam_size: int = 1, language: str = None, task: str = "transcribe",
                   temperature=TEMPERATURES, best_of: int = BEST_OF, length_penalty: float = 1.0,
                   patience: float = 1, max_length: int = 448, word_timestamps: bool = False,
                   prepend_punctuations: str = PREPEND_PUNCTUATIONS,
                   append_punctuations: str = APPEND_PUNCTUATIONS,
                   hallucination_silence_threshold=None, language_detection_segments: int = 1,
                   language_detection_threshold: float = 0.5, vad_filter: bool = False,
                   vad_parameters=None, repetition_penalty: float = 1, no_repeat_ngram_size: int = 0,
                   suppress_tokens=(-1,), initial_prompt=None, hotwords=None,
                   condition_on_previous_text: bool = True, prompt_reset_on_temperature: float = 0.5,
                   **_ignored):
        """faster-whisper's transcribe: ``beam_size`` 1 (greedy, the reference's call) .. 8
        (beam search at T = 0), ``length_penalty`` > 0, ``patience`` 1;
        ``max_length``: the decoder's token limit per window (448). ``word_timestamps``: every
        segment carries ``words`` ([Word(start, end, word, probability)]) from the alignment
        pass, with faster-whisper's ``prepend_punctuations`` /
        ``append_punctuations``; ``hallucination_silence_threshold`` is not built (None only).
        ``vad_filter`` / ``vad_parameters`` (a dict or VadOptions): only the speech the gate
        finds is decoded and every time is restored onto ``audio`` (generate_segments);
        ``info.duration_after_vad`` is the audio kept, ``info.vad_options`` the options.
        ``repetition_penalty``, ``no_repeat_ngram_size``, ``suppress_tokens``, ``initial_prompt``,
        ``hotwords``, ``condition_on_previous_text`` and ``prompt_reset_on_temperature`` as in
        faster-whisper (generate_segments): the two history rules need
        ``beam_size`` 1 (NotImplementedError otherwise, before any GPU work)."""
        check_beam_args(beam_size, length_penalty, patience)
        check_decoder_compute_beam(getattr(self, "decoder_compute", "float16"), beam_size)
        check_history_args(repetition_penalty, no_repeat_ngram_size, beam_size)
        check_family_features(getattr(self.engine, "cfg", None), beam_size, word_timestamps,
                              getattr(self.engine, "alignment_heads", None))
        if hallucination_silence_threshold is not None:
            raise NotImplementedError("hallucination_silence_threshold is not supported")
        self._check_language(language, task)
        audio = self._load_audio(audio)
        temps = (float(temperature),) if np.isscalar(temperature) else tuple(temperature)
        vad_options = vf.as_vad_options(vad_parameters) if vad_filter else None
        st = generate_segments(self.engine, [audio], max_length=max_length, temperatures=temps,
                               best_of=best_of, beam_size=beam_size, length_penalty=length_penalty,
                               word_timestamps=bool(word_timestamps),
                               prepend_punctuations=prepend_punctuations,
                               append_punctuations=append_punctuations, language=language, task=task,
                               language_detection_segments=language_detection_segments,
                               language_detection_threshold=language_detection_threshold,
                               vad_filter=bool(vad_filter), vad_parameters=vad_options,
                               vad=self._vad() if vad_filter else None,
                               repetition_penalty=repetition_penalty,
                               no_repeat_ngram_size=no_repeat_ngram_size, suppress_tokens=suppress_tokens,
                               initial_prompt=initial_prompt, hotwords=hotwords,
                               condition_on_previous_text=condition_on_previous_text,
                               prompt_reset_on_temperature=prompt_reset_on_temperature)[0]
        self._count(st)
        info = TranscriptionInfo(st.language, st.language_probability, len(audio) / 16000.0,
                                 st.all_language_probs, st.duration_after_vad, vad_options)
        return iter(st.segments), info

    def _count(self, st):
        self.stats["windows"] += st.windows
        self.stats["needs_fallback"] += st.fallbacks
        self.stats["no_speech_skips"] += st.skips
        self.stats["fallback_decodes"] += st.fallback_decodes


class Transcriber:
    def __init__(self, model_size: str = 'base.en') -> None:
        """transcriber.py:11-27, the same call (WhisperModel maps it onto the GPU engine)."""
        self.model = WhisperModel(
            model_size,
            device='cpu',
            compute_type='int8'
        )

    def transcribe_buffer(self, audio_buffer: np.ndarray) -> str:
        """transcriber.py:29-64."""
        if isinstance(audio_buffer, list):
            audio_buffer = np.concatenate(audio_buffer)
        if not isinstance(audio_buffer, np.ndarray):
            audio_buffer = np.array(audio_buffer, dtype=np.float32)
        if audio_buffer.dtype != np.float32:
            audio_buffer = audio_buffer.astype(np.float32)
        audio_16k = audio_buffer[::3]
        segments, info = self.model.transcribe(audio_16k, beam_size=1, language='en')
        text_parts = []
        for segment in segments:
            text_parts.append(segment.text.strip())
        full_text = ' '.join(text_parts).strip()
        return full_text

    def transcribe_file(self, file_path: str) -> str:
        """transcriber.py:66-91 (16-bit PCM WAV input)."""
        segments, info = self.model.transcribe(file_path, beam_size=1, language='en')
        text_parts = []
        for segment in segments:
            text_parts.append(segment.text.strip())
        full_text = ' '.join(text_parts).strip()
        return full_text

    def transcribe_batch(self, buffers) -> list:
        """Batched extension: 48 kHz buffers (any length) -> transcripts, the seek loops
        of all buffers advanced together (one GPU batch per round)."""
        auds = [np.ascontiguousarray(np.asarray(b, dtype=np.float32)[::3]) for b in buffers]
        streams = generate_segments(self.model.engine, auds)
        for st in streams:
            self.model._count(st)
        return [' '.join(s.text.strip() for s in st.segments).strip() for st in streams]


def __getattr__(name):
    """BatchedInferencePipeline / generate_segments_batched live in services/batched.py (which
    imports this module) and are exported here beside WhisperModel, resolved on first use."""
    if name in ("BatchedInferencePipeline", "generate_segments_batched"):
        from . import batched
        return getattr(batched, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["Transcriber", "WhisperModel", "decode_audio", "BatchedInferencePipeline", "generate_segments_batched", "Segment", "Word", "find_alignment", "merge_punctuations",
           "add_word_timestamps", "word_seek", "window_text_tokens", "TranscriptionInfo", "read_wav_16k",
           "generate_segments", "settle_round", "advance", "gather_windows", "split_window", "compression_ratio", "gates", "nat",
           "Candidate", "candidate", "best_hypothesis", "settle", "fallback_seed", "TEMPERATURES",
           "BEST_OF"]
