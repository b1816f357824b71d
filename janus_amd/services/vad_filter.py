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

    from .vad import _energy_prob
    counts = [n_windows(len(a)) for a in audios]
    if vad is not None:
        offsets = np.zeros(len(audios) + 1, np.int64)
        offsets[1:] = np.cumsum([len(a) for a in audios])
        flat = np.concatenate([np.asarray(a, np.float32) for a in audios] + [np.zeros(1, np.float32)])
        return vad.probs_file(torch.from_numpy(flat).to(device), offsets, max_chunks_per_pass)
    padded = np.zeros(sum(counts) * WINDOW, np.float32)
    at = 0
    for a, n in zip(audios, counts):
        padded[at:at + len(a)] = a
        at += n * WINDOW
    p = _energy_prob(torch.from_numpy(padded).to(device).reshape(-1, WINDOW), 1).cpu().numpy()
    return [p[o - n:o] for n, o in zip(counts, np.cumsum(counts))]


__all__ = ["VadOptions", "as_vad_options", "get_speech_timestamps", "collect_chunks", "SpeechTimestampsMap",
           "restore_speech_timestamps", "speech_probabilities", "n_windows", "WINDOW", "SAMPLE_RATE"]
