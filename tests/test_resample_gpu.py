"""The band-limited resampler on the GPU (csrc/resample.hip) against the float64
rule of tests/resample_ref.py:

1. parity at the derived bound for five rate pairs, noise and a constant, lengths around
   every edge of the rule and of the kernel's output tile;
2. clips of one call do not mix and a repeated call gives the same bits;
3. a device tensor in gives a device tensor out;
4. WhisperModel(audio_resample="bandlimited") reads a 44.1 kHz stereo file through
   decode_audio, from a path and from an open file."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

import resample_ref as rr
from janus_amd import audio
from janus_amd.services import transcriber as tr

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (11025, 16000), (44100, 48000)]


@functools.lru_cache(maxsize=None)
def resampler(sr_in, sr_out):
    return audio.Resampler(sr_in, sr_out)


def lengths(r):
    """1, 2, M - 1, M, M + 1, 16 M - 1, 16 M + 1, the lengths whose n_out is the greatest not
    above out_tile - 1, out_tile and out_tile + 1 (out_tile from the library's info entry: what
    one block of the kernel computes; not every n_out exists when L > M), and 3.1 s."""
    L, M = r.L, r.M
    around = [t * M // L for t in (r.out_tile - 1, r.out_tile, r.out_tile + 1)]
    assert r.out_len(around[1]) <= r.out_tile < r.out_len(around[1] + 1)
    assert r.out_len(around[2] + 1) > r.out_tile + 1
    out = [1, 2, M - 1, M, M + 1, 16 * M - 1, 16 * M + 1] + around + [around[2] + 1, int(3.1 * r.sr_in)]
    return sorted({n for n in out if n >= 1})


def signal(kind, n):
    if kind == "const":
        return np.full(n, 0.5, np.float32)
    return (np.random.default_rng(n).normal(size=n) * 0.3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(sr_in, sr_out, kind, n):
    """(y float64, T of the widest phase, max_p ||h_p||_1): computed once, never changed."""
    y, T, norm = rr.resample(signal(kind, n), sr_in, sr_out)
    y.setflags(write=False)
    return y, int(T.max()), float(norm.max())


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("kind", ["noise", "const"])
@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_parity_with_the_rule(gpu, sr_in, sr_out, kind):
    """Every output sample within (T + 4) 2^-24 max_p ||h_p||_1 max|x| of the float64 rule: T
    fused multiply-adds of one chain, one tap rounding of up to 2 ulp, the product rounding.
    No extra margin. The first and last ceil(W L / M) outputs, where the rule's zero extension
    acts, are held to the same bound."""
    r = resampler(sr_in, sr_out)
    assert (r.L, r.M) == rr.reduce_rates(sr_in, sr_out)
    assert r.front_zeros >= math.ceil(rr.half_width(sr_in, sr_out)) + 1
    edge = math.ceil(rr.half_width(sr_in, sr_out) * r.L / r.M)
    for n in lengths(r):
        x = signal(kind, n)
        want, T, norm = reference(sr_in, sr_out, kind, n)
        got = r(x)
        assert got.dtype == np.float32 and got.shape == (rr.out_len(n, sr_in, sr_out),) == want.shape
        bound = (T + 4) * 2.0 ** -24 * norm * float(np.abs(x).max())
        err = np.abs(got.astype(np.float64) - want)
        print(f"{sr_in} -> {sr_out} {kind} n_in {n}: max error {err.max():.3g}, bound {bound:.3g}")
        assert err[:edge].max() <= bound and err[-edge:].max() <= bound, n
        assert err.max() <= bound, n


def test_empty_input_is_empty_output(gpu):
    r = resampler(44100, 16000)
    got = r(np.zeros(0, np.float32))
    assert got.dtype == np.float32 and got.shape == (0,)
    assert [g.shape for g in r([np.zeros(0, np.float32), np.zeros(0, np.float32)])] == [(0,), (0,)]
    assert r([]) == []


def test_equal_rates_copy(gpu):
    x = signal("noise", 1234)
    assert np.array_equal(audio.Resampler(16000, 16000)(x), x)


# ------------------------------------------------------------------ 2. clips do not mix
@pytest.mark.parametrize("sr_in,sr_out", [(44100, 16000), (8000, 16000)])
def test_clips_do_not_mix(gpu, sr_in, sr_out):
    r = resampler(sr_in, sr_out)
    clips = [signal("noise", 7001), signal("noise", 1), np.zeros(0, np.float32), signal("noise", 12345) + 1.0]
    together = r(clips)
    assert [len(t) for t in together] == [r.out_len(len(c)) for c in clips]
    for c, t in zip(clips, together):
        assert np.array_equal(r(c), t)
    for a, b in zip(r(clips), together):
        assert np.array_equal(a, b)
    # a shorter call after a longer one: nothing of the longer one is left in the staging buffer
    assert np.array_equal(r(clips[1]), together[1])


# ------------------------------------------------------------------ 3. device tensors
def test_device_tensor_in_device_tensor_out(gpu):
    r = resampler(44100, 16000)
    x = signal("noise", 30011)
    want = r(x)
    got = r(torch.from_numpy(x).to(gpu))
    assert isinstance(got, torch.Tensor) and got.device == gpu and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)
    two = r([torch.from_numpy(x).to(gpu), torch.from_numpy(x[:500]).to(gpu)])
    assert all(t.device == gpu for t in two)
    assert np.array_equal(two[0].cpu().numpy(), want) and np.array_equal(two[1].cpu().numpy(), r(x[:500]))
    assert np.array_equal(audio.resample(torch.from_numpy(x).to(gpu), 44100, 16000).cpu().numpy(), want)


# ------------------------------------------------------------------ 4. wiring
def test_whisper_model_bandlimited(gpu, tmp_path):
    sr, n = 44100, 2 * 44100
    t = np.arange(n) / sr
    left = 0.3 * np.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * t))
    right = 0.2 * np.sin(2 * np.pi * 330.0 * t) + 0.05 * np.random.default_rng(5).normal(size=n)
    pcm = np.clip(np.round(np.stack([left, right], axis=1) * 32767.0), -32768, 32767).astype("<i2").tobytes()
    path = tmp_path / "stereo44k.wav"
    path.write_bytes(struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(pcm), b"WAVE", b"fmt ", 16, 1, 2, sr,
                                 sr * 4, 4, 16, b"data", len(pcm)) + pcm)
    want = audio.decode_audio(str(path))
    assert want.dtype == np.float32 and len(want) == rr.out_len(n, sr, 16000) == 32000
    l, r = audio.decode_audio(str(path), split_stereo=True)
    assert len(l) == len(r) == 32000 and not np.array_equal(l, r)

    m = tr.WhisperModel("tiny.en", audio_resample="bandlimited")
    assert m.audio_resample == "bandlimited"
    assert np.array_equal(m._load_audio(str(path)), want)
    assert np.array_equal(m._load_audio(path), want)
    # not the reference's interpolation
    assert not np.array_equal(want, tr.read_wav_16k(str(path))[:len(want)])

    def run(a):
        segs, info = m.transcribe(a, temperature=0, max_length=8)
        return [(s.start, s.end, s.text, list(s.tokens)) for s in segs], info
    segs, info = run(str(path))
    assert info.duration == len(want) / 16000
    with open(path, "rb") as f:
        segs_f, info_f = run(f)
    assert segs_f == segs and info_f.duration == info.duration
    assert run(path.read_bytes())[0] == segs
