"""faster-whisper's ``vad_filter``: speech timestamps from per-window speech probabilities,
the collected speech, and the map that restores times on the original audio.

Pure Python / numpy (no GPU): the probabilities come from ``SileroGate.probs_file`` (one
janus_vad_probs call over whole utterances, csrc/vad_file.hip) or, without silero weights, from
the documented energy stand-in. The rule is stated in include/janus.h (janus_vad_probs) and
DESIGN.md §5n; faster-whisper is not reachable offline, so it is "parity unpinned" against the
package, like beam search and word timestamps.
"""
import bisect
import dataclasses

import numpy as np

SAMPLE_RATE = 16000
WINDOW = 512                  # samples per probability (silero v5 @ 16 kHz)
MIN_SILENCE_AT_MAX = 1568     # 98 ms: a silence long enough to cut an over-long speech at


@dataclasses.dataclass
class VadOptions:
    """faster-whisper's VadOptions with its defaults. ``neg_threshold`` None:
    max(threshold - 0.15, 0.01)."""
    threshold: float = 0.5
    neg_threshold: float = None
    min_speech_duration_ms: int = 0
    max_speech_duration_s: float = float("inf")
    min_silence_duration_ms: int = 2000
    speech_pad_ms: int = 400


def as_vad_options(vad_parameters) -> VadOptions:
    """None -> defaults, a VadOptions as it is, a dict by keyword (unknown key: TypeError)."""
    if vad_parameters is None:
        return VadOptions()
    if isinstance(vad_parameters, VadOptions):
        return vad_parameters
    if isinstance(vad_parameters, dict):
        return VadOptions(**vad_parameters)
    raise TypeError("vad_parameters: a dict or a VadOptions")


def n_windows(n_samples: int) -> int:
    """Probabilities of an utterance: faster-whisper pads with 512 - len % 512 zeros, so a
    length that is a multiple of 512 gets one whole zero window."""
    return n_samples // WINDOW + 1


def get_speech_timestamps(probs, n_samples: int, options: VadOptions = None):
    """[(start, end)] in samples of the speech in an utterance of ``n_samples`` samples whose
    512-sample windows have speech probabilities ``probs`` (rule: include/janus.h)."""
    o = options if options is not None else VadOptions()
    threshold = o.threshold
    neg_threshold = o.neg_threshold if o.neg_threshold is not None else max(threshold - 0.15, 0.01)
    w = WINDOW
    min_speech = SAMPLE_RATE * o.min_speech_duration_ms / 1000
    pad = SAMPLE_RATE * o.speech_pad_ms / 1000
    max_speech = SAMPLE_RATE * o.max_speech_duration_s - w - 2 * pad
    min_sil = SAMPLE_RATE * o.min_silence_duration_ms / 1000
    triggered = False
    temp_end = prev_end = next_start = 0
    start = None
    speeches = []
    for i, p in enumerate(probs):
        at = w * i
        if p >= threshold and temp_end:
            temp_end = 0
            if next_start < prev_end:
                next_start = at
        if p >= threshold and not triggered:
            triggered = True
            start = at
            continue
        if triggered and at - start > max_speech:
            if prev_end:
                speeches.append([start, prev_end])
                if next_start < prev_end:
                    triggered, start = False, None
                else:
                    start = next_start
                prev_end = next_start = temp_end = 0
            else:
                speeches.append([start, at])
                prev_end = next_start = temp_end = 0
                triggered, start = False, None
                continue
        if p < neg_threshold and triggered:
            if not temp_end:
                temp_end = at
            if at - temp_end > MIN_SILENCE_AT_MAX:
                prev_end = temp_end
            if at - temp_end < min_sil:
                continue
            if temp_end - start > min_speech:
                speeches.append([start, temp_end])
            prev_end = next_start = temp_end = 0
            triggered, start = False, None
            continue
    if start is not None and n_samples - start > min_speech:
        speeches.append([start, n_samples])
    for k, sp in enumerate(speeches):
        if k == 0:
            sp[0] = int(max(0, sp[0] - pad))
        if k != len(speeches) - 1:
            nxt = speeches[k + 1]
            sil = nxt[0] - sp[1]
            if sil < 2 * pad:
                sp[1] += int(sil // 2)
                nxt[0] = int(max(0, nxt[0] - sil // 2))
            else:
                sp[1] = int(min(n_samples, sp[1] + pad))
                nxt[0] = int(max(0, nxt[0] - pad))
        else:
            sp[1] = int(min(n_samples, sp[1] + pad))
    return [(int(a), int(b)) for a, b in speeches]


def collect_chunks(audio, speeches):
    """The speech of ``audio``: audio[start:end] of every speech, concatenated."""
    audio = np.asarray(audio)
    if not speeches:
        return np.zeros(0, audio.dtype)
    return np.concatenate([audio[a:b] for a, b in speeches])


class SpeechTimestampsMap:
    """Times on the collected speech -> times on the original audio."""

    def __init__(self, speeches, sampling_rate: int = SAMPLE_RATE):
        self.sampling_rate = sampling_rate
        self.chunk_end_sample = []
        self.total_silence_before = []
        previous_end = silent = 0
        for start, end in speeches:
            silent += start - previous_end
            previous_end = end
            self.chunk_end_sample.append(end - silent)
            self.total_silence_before.append(silent / sampling_rate)

    def chunk_index(self, time: float, is_end: bool = False) -> int:
        sample = int(time * self.sampling_rate)
        if is_end and sample in self.chunk_end_sample:
            return self.chunk_end_sample.index(sample)
        return min(bisect.bisect_right(self.chunk_end_sample, sample), len(self.chunk_end_sample) - 1)

    def original_time(self, time: float, chunk_index: int = None, is_end: bool = False) -> float:
        if chunk_index is None:
            chunk_index = self.chunk_index(time, is_end)
        return round(self.total_silence_before[chunk_index] + time, 2)


def restore_speech_timestamps(segments, ts_map: SpeechTimestampsMap):
    """The segments (dataclasses with start, end, words) with their times on the original
    audio: a word goes by the chunk of its middle; a segment with words spans them, one
    without maps its start and (as an end) its end."""
    out = []
    for seg in segments:
        if seg.words:
            words = []
            for wd in seg.words:
                k = ts_map.chunk_index((wd.start + wd.end) / 2)
                words.append(dataclasses.replace(wd, start=ts_map.original_time(wd.start, k),
                                                 end=ts_map.original_time(wd.end, k)))
            out.append(dataclasses.replace(seg, start=words[0].start, end=words[-1].end, words=words))
        else:
            out.append(dataclasses.replace(seg, start=ts_map.original_time(seg.start),
                                           end=ts_map.original_time(seg.end, is_end=True)))
    return out


def speech_probabilities(audios, device, vad=None, max_chunks_per_pass: int = 0):
    """Per-utterance speech probabilities (f32 [len // 512 + 1]) of 16 kHz ``audios`` from ONE
    GPU call: ``vad`` (a SileroGate) runs janus_vad_probs over the concatenated audio; None runs
    the energy stand-in (janus_vad_energy, decim 1) over the zero-padded 512-sample windows —
    the contract of VoiceActivityDetector without weights."""
    import torch
    offsets = np.zeros(len(audios) + 1, np.int64)
    offsets[1:] = np.cumsum([len(a) for a in audios])
    flat = np.concatenate([np.asarray(a, np.float32) for a in audios] + [np.zeros(1, np.float32)])
    return speech_probabilities_device(torch.from_numpy(flat).to(device), offsets, vad, max_chunks_per_pass)


def speech_probabilities_device(pcm, offsets, vad=None, max_chunks_per_pass: int = 0):
    """speech_probabilities of utterances that already lie on the device: ``pcm`` f32 (device) =
    the 16 kHz audio of S utterances concatenated, ``offsets`` [S + 1] (host) in samples. ONE
    gate call; the stand-in's zero-padded windows are laid out on the device (copies of
    ``pcm``'s ranges), so a caller that keeps the buffer uploads its audio once."""
    import torch

    from .vad import _energy_prob
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if vad is not None:
        return vad.probs_file(pcm, offs, max_chunks_per_pass)
    counts = [n_windows(int(n)) for n in np.diff(offs)]
    padded = torch.zeros(sum(counts) * WINDOW, dtype=torch.float32, device=pcm.device)
    at = 0
    for k, n in enumerate(counts):
        a, b = int(offs[k]), int(offs[k + 1])
        padded[at:at + b - a] = pcm[a:b]
        at += n * WINDOW
    p = _energy_prob(padded.reshape(-1, WINDOW), 1).cpu().numpy()
    return [p[o - n:o] for n, o in zip(counts, np.cumsum(counts))]


# ---------------------------------------------------------------- batched transcription
# BatchedInferencePipeline's chunk rule (services/batched.py; parity unpinned
# like the rule above: faster-whisper is not reachable offline, so this text is the rule).
CHUNK_LENGTH_S = 30
BATCHED_MIN_SILENCE_MS = 160   # min_silence_duration_ms of the batched call without vad_parameters


def merge_segments(speeches, chunk_length_s: float = CHUNK_LENGTH_S):
    """[(start, end, [(s, e), ...])] in samples: consecutive ``speeches`` ([(s, e)], samples,
    in order) merged into chunks of at most ``chunk_length_s`` seconds. A speech whose end
    lies more than the limit after the open chunk's start closes that chunk (when it holds
    anything) and opens the next at its own start, so a single speech longer than the limit
    is a chunk of its own. A chunk is the contiguous span [start, end): the pauses between
    its speeches stay inside. No speeches: no chunks."""
    speeches = [(int(s), int(e)) for s, e in speeches]
    if not speeches:
        return []
    limit = SAMPLE_RATE * chunk_length_s
    out = []
    curr_start, curr_end, inside = speeches[0][0], 0, []
    for s, e in speeches:
        if e - curr_start > limit and curr_end - curr_start > 0:
            out.append((curr_start, curr_end, inside))
            curr_start, inside = s, []
        curr_end = e
        inside.append((s, e))
    out.append((curr_start, curr_end, inside))
    return out


def batched_vad_options(vad_parameters=None, chunk_length_s: float = CHUNK_LENGTH_S) -> VadOptions:
    """The VadOptions of the batched call: None -> the defaults with min_silence_duration_ms
    160; a dict / VadOptions keeps its fields; ``max_speech_duration_s`` is ``chunk_length_s``
    in every case, so no speech outgrows a chunk."""
    if vad_parameters is None:
        return VadOptions(min_silence_duration_ms=BATCHED_MIN_SILENCE_MS, max_speech_duration_s=chunk_length_s)
    return dataclasses.replace(as_vad_options(vad_parameters), max_speech_duration_s=chunk_length_s)


def clip_chunks(clip_timestamps, n_samples: int):
    """merge_segments' form for ``clip_timestamps``: (start_s, end_s) pairs or {"start", "end"}
    dicts in SECONDS, taken as given (sample = round(16000 t), cut to the audio); ValueError
    for a clip that ends before it starts."""
    out = []
    for c in clip_timestamps:
        a, b = (c["start"], c["end"]) if isinstance(c, dict) else c
        s, e = int(round(float(a) * SAMPLE_RATE)), int(round(float(b) * SAMPLE_RATE))
        if s < 0 or e < s:
            raise ValueError(f"clip_timestamps: ({a!r}, {b!r}) is no clip (0 <= start <= end, seconds)")
        s, e = min(s, n_samples), min(e, n_samples)
        out.append((s, e, [(s, e)]))
    return out


NO_CLIPS = "No clip timestamps found. Set 'vad_filter' to True or provide 'clip_timestamps'."


def whole_file_chunk(n_samples: int, chunk_length_s: float = CHUNK_LENGTH_S):
    """Neither the filter nor clips: audio of at most one chunk is the chunk [0, n);
    longer audio is faster-whisper's RuntimeError."""
    if n_samples > SAMPLE_RATE * chunk_length_s:
        raise RuntimeError(NO_CLIPS)
    return [(0, int(n_samples), [(0, int(n_samples))])]


__all__ = ["VadOptions", "as_vad_options", "get_speech_timestamps", "collect_chunks", "SpeechTimestampsMap",
           "restore_speech_timestamps", "speech_probabilities", "speech_probabilities_device", "n_windows",
           "merge_segments", "batched_vad_options", "clip_chunks", "whole_file_chunk", "CHUNK_LENGTH_S",
           "BATCHED_MIN_SILENCE_MS", "WINDOW", "SAMPLE_RATE"]
