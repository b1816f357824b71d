"""References of the batched long-form call (services/batched.py) on the unchanged oracle: the
yardstick of tests/test_batched_gpu.py. A helper module, not a conftest.

What the oracle lacks is restated here in numpy: a chunk is a 30 s window of its own — the
oracle's log-mel of the slice alone (normalised over the slice, zero from its content end),
its encoder (rounded to fp16 as the engine hands it on), its greedy decode with timestamps
under the start sequence — and its tokens are sliced into segments from the chunk's start,
with no seek carried (``chunk_segments``: faster-whisper's rule for one window, written out
independently of services/transcriber.py). ``energy_probs`` is the documented energy stand-in
of the speech gate (include/janus.h janus_vad_energy) over zero-padded 512-sample windows.
"""
import json
import math
import os

import numpy as np

from oracle import whisper as ow

NEAR_TIE = 2e-3
MIN_MARGIN = 2 * NEAR_TIE          # every reference decision is at least this clear
GOLDEN = "batched_refs.json"

# Chunks of one seeded clip: a short one starting between two frames, a middling one, one of
# exactly 30 s and a tail. The audio seed was chosen on the CPU with this reference alone (seeds
# 0 .. 29 tried in turn) so that every chunk's smallest top-2 margin is >= MIN_MARGIN (0.011 here).
PARITY_CASE = dict(model="tiny.en", wseed=0, audio_seed=21, seconds=50.0, max_length=24,
                   clips=[[0.5025, 9.0], [10.0, 16.25], [18.0, 48.0], [48.5, 49.9]])


def parity_audio(case=None):
    from janus_amd.workload import synth_speech
    c = case or PARITY_CASE
    return synth_speech(c["audio_seed"], c["seconds"], sr=16000)


def chunk_segments(tokens, tb, offset_s, seconds):
    """One chunk's sampled tokens (no <|endoftext|>) -> [[start_s, end_s, tokens]]: cut after
    every second of two consecutive timestamps; a tail that ends in a single timestamp is a
    segment too, any other tail is left out (a seek loop would decode it again; here nothing
    is carried); without consecutive timestamps the whole is one segment lasting to its last
    timestamp, or ceil(seconds) when it has none but <|0.00|>. Times count from ``offset_s``."""
    n = len(tokens)
    cuts = [i for i in range(1, n) if tokens[i] >= tb and tokens[i - 1] >= tb]
    if not cuts:
        stamps = [t for t in tokens if t >= tb]
        dur = float(math.ceil(seconds) * 100) * 0.01
        if stamps and stamps[-1] != tb:
            dur = (stamps[-1] - tb) * 0.02
        return [[offset_s, offset_s + dur, list(tokens)]]
    if n >= 2 and tokens[-2] < tb <= tokens[-1]:
        cuts.append(n)
    out, last = [], 0
    for c in cuts:
        part = list(tokens[last:c])
        out.append([offset_s + (part[0] - tb) * 0.02, offset_s + (part[-1] - tb) * 0.02, part])
        last = c
    return out


def compute_parity(case=None):
    """dict(case, chunks=[dict(start, end, tokens, avg, nsp, min_margin)], segments=[[start, end,
    tokens]]): the oracle's greedy decode of every chunk's own window, and the segments kept
    (start != end and some text token)."""
    from janus_amd import tokenizer as tok
    from janus_amd.whisper import CONFIGS, mel_filters, synthetic_weights
    c = case or PARITY_CASE
    cfg = CONFIGS[c["model"]]
    W = synthetic_weights(cfg, seed=c["wseed"])
    tk = tok.WhisperTokenizer()
    audio = parity_audio(c)
    chunks, segments = [], []
    for a_s, b_s in c["clips"]:
        a, b = int(round(a_s * 16000)), int(round(b_s * 16000))
        feats = ow.logmel(audio[a:b], 1, mel_filters())
        enc = ow.encoder(feats[None], W, cfg).half().float().numpy()
        r = ow.greedy_cached(enc, W, cfg, tk, c["max_length"], prompts=[list(tk.sot_sequence)],
                             no_speech=tk.no_speech)[0]
        toks = [t for t in r["tokens"] if t != tk.eot]
        chunks.append(dict(start=a, end=b, tokens=toks, avg=r["sum_lp"] / (len(toks) + 1), nsp=r["nsp"],
                           min_margin=min(r["margins"])))
        for st, en, part in chunk_segments(toks, tk.timestamp_begin, a / 16000.0, (b - a) / 16000.0):
            if st != en and any(t < tk.eot for t in part):
                segments.append([st, en, part])
    return dict(case=c, chunks=chunks, segments=segments)


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def parity_reference():
    """The committed reference when it was made for PARITY_CASE, else computed (a minute)."""
    if os.path.exists(golden_path()):
        with open(golden_path()) as f:
            g = json.load(f)
        if g.get("case") == PARITY_CASE:
            return g
    return compute_parity()


# ------------------------------------------------------------------ the energy stand-in
def energy_probs(audio, center_db=-45.0, width_db=3.0):
    """f64 [len // 512 + 1]: sigmoid((10 log10(mean(x^2)) - center) / width) of the audio's
    512-sample windows, the last padded with zeros (one whole zero window when the length is a
    multiple of 512); an all-zero window is 0."""
    x = np.asarray(audio, np.float64)
    n = len(x) // 512 + 1
    pad = np.zeros(n * 512)
    pad[:len(x)] = x
    ms = (pad.reshape(n, 512) ** 2).mean(axis=1)
    with np.errstate(divide="ignore", over="ignore"):
        db = 10.0 * np.log10(ms)
        return 1.0 / (1.0 + np.exp(-(db - center_db) / width_db))


def burst_file(seconds=70.0, burst_s=12.0, gap_s=2.0, seed=4100):
    """``burst_s`` of seeded synthetic speech over a noise floor of 0.02 rms (-34 dB: the
    speech's own pauses stay well above the gate's -45 dB centre), ``gap_s`` of zeros,
    repeated: f32 @ 16 kHz, and a bool per sample: inside a burst."""
    from janus_amd.workload import synth_speech
    n = int(seconds * 16000)
    period = int((burst_s + gap_s) * 16000)
    out = np.zeros(n, np.float32)
    inside = np.zeros(n, bool)
    rng = np.random.default_rng(seed)
    for k, at in enumerate(range(0, n, period)):
        b = synth_speech(seed + k, burst_s, sr=16000)[:n - at]
        b = (b + 0.02 * rng.standard_normal(len(b))).astype(np.float32)
        out[at:at + len(b)] = b
        inside[at:at + len(b)] = True
    return out, inside
