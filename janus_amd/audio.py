"""Audio front door, named as ``faster_whisper.audio`` is: ``decode_audio`` reads a file at
any rate and resamples it with a band-limited filter on the GPU (csrc/resample.hip; the rule
is stated in include/janus.h and DESIGN.md §5t). faster-whisper takes this step through
PyAV / libswresample, which cannot be pinned offline: parity with it is unpinned."""
import ctypes
import os

import numpy as np
import torch

from . import _native
from .common import wavio


def resample_plan(sr_in: int, sr_out: int):
    """The host plan of a rate pair, no GPU: (L, M, T, first int32 [L], taps float32 [L][T]).
    JanusNativeError, naming both rates, for a pair the resampler refuses."""
    L, M, T = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _native.call("janus_resample_plan", int(sr_in), int(sr_out), ctypes.addressof(L), ctypes.addressof(M),
                 ctypes.addressof(T), None, 0, None, 0)
    first = np.zeros(L.value, np.int32)
    taps = np.zeros((L.value, T.value), np.float32)
    _native.call("janus_resample_plan", int(sr_in), int(sr_out), None, None, None, first.ctypes.data,
                 first.size, taps.ctypes.data, taps.size)
    return L.value, M.value, T.value, first, taps


def resample_out_len(n_in: int, sr_in: int, sr_out: int) -> int:
    """ceil(n_in L / M) from the host plan's L and M (no GPU)."""
    L, M = ctypes.c_int(), ctypes.c_int()
    _native.call("janus_resample_plan", int(sr_in), int(sr_out), ctypes.addressof(L), ctypes.addressof(M),
                 None, None, 0, None, 0)
    return -(-int(n_in) * L.value // M.value)


class Resampler:
    """Band-limited resampling from ``sr_in`` to ``sr_out`` on the GPU. Callable on a 1-D
    array or tensor, or on a list of them (one launch for the whole list; no clip reaches
    another's output). Returns float32 of the kind it was given: numpy in, numpy out; a
    tensor on the resampler's device in, a tensor there out, with no host copy."""

    def __init__(self, sr_in: int, sr_out: int, device=None):
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.L, self.M, self.T, _, _ = resample_plan(self.sr_in, self.sr_out)   # refusals need no GPU
        cur = _native.require_gpu()
        self.device = cur if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"Resampler runs on the GPU only, not on {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _native.call("janus_resampler_create", self.sr_in, self.sr_out, ctypes.addressof(self._h))
        tile, front = ctypes.c_int(), ctypes.c_int()
        _native.call("janus_resampler_info", self._h, None, None, None, ctypes.addressof(tile),
                     ctypes.addressof(front))
        self.out_tile, self.front_zeros = tile.value, front.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _native.lib().janus_resampler_destroy(h)
            except Exception:
                pass

    def out_len(self, n_in: int) -> int:
        return -(-int(n_in) * self.L // self.M)

    def __call__(self, x):
        many = isinstance(x, (list, tuple))
        clips = list(x) if many else [x]
        on_device = bool(clips) and all(isinstance(c, torch.Tensor) for c in clips)
        if not on_device and any(isinstance(c, torch.Tensor) for c in clips):
            raise TypeError("Resampler: a list holds arrays or tensors, not both")
        if on_device:
            for c in clips:
                if c.device != self.device:
                    raise ValueError(f"Resampler on {self.device} was given a tensor on {c.device}")
            dev = [c.detach().to(torch.float32).reshape(-1) if c.dim() <= 1 else None for c in clips]
        else:
            host = [np.asarray(c, dtype=np.float32) for c in clips]
            dev = [h.reshape(-1) if h.ndim <= 1 else None for h in host]
        if any(d is None for d in dev):
            raise ValueError("Resampler takes 1-D audio")
        n_in = [int(d.shape[0]) for d in dev]
        offs = np.zeros(len(dev) + 1, np.int64)
        offs[1:] = np.cumsum(n_in)
        out_offs = np.zeros(len(dev) + 1, np.int64)
        out_offs[1:] = np.cumsum([self.out_len(n) for n in n_in])
        with torch.cuda.device(self.device):
            if on_device:
                pcm = dev[0].contiguous() if len(dev) == 1 else torch.cat(dev)
            else:
                pcm = torch.from_numpy(np.concatenate(dev) if dev else np.zeros(0, np.float32)).to(self.device)
            out = torch.empty(int(out_offs[-1]), dtype=torch.float32, device=self.device)
            _native.call("janus_resample_f32", self._h, pcm.data_ptr(), offs.ctypes.data, len(dev),
                         out.data_ptr(), out_offs.ctypes.data, _native.stream_ptr(self.device))
            if on_device:
                res = [out[out_offs[i]:out_offs[i + 1]] for i in range(len(dev))]
            else:
                flat = out.cpu().numpy()
                res = [flat[out_offs[i]:out_offs[i + 1]].copy() for i in range(len(dev))]
        return res if many else res[0]


_RESAMPLERS = {}


def resample(x, sr_in: int, sr_out: int):
    """``x`` (as Resampler takes it) from ``sr_in`` to ``sr_out``; one Resampler is kept per
    rate pair and device."""
    first = x[0] if isinstance(x, (list, tuple)) and x else x
    if isinstance(first, torch.Tensor) and first.is_cuda:
        device = first.device
    else:
        device = _native.require_gpu()
    key = (int(sr_in), int(sr_out), device.index)
    if key not in _RESAMPLERS:
        _RESAMPLERS[key] = Resampler(sr_in, sr_out, device)
    return _RESAMPLERS[key](x)


def _read_all(input_file) -> bytes:
    if isinstance(input_file, (bytes, bytearray, memoryview)):
        return bytes(input_file)
    if hasattr(input_file, "read"):
        return input_file.read()
    with open(os.fspath(input_file), "rb") as f:
        return f.read()


def decode_audio(input_file, sampling_rate: int = 16000, split_stereo: bool = False):
    """faster-whisper's decode_audio: ``input_file`` (a path, a PathLike, an open binary file
    or bytes) -> mono float32 numpy at ``sampling_rate``, or with ``split_stereo`` the pair
    (left, right), ValueError unless the file has exactly two channels.

    Reads the RIFF encodings ``wavio.wav_to_f32`` reads (compressed formats need FFmpeg:
    ValueError). A file already at ``sampling_rate`` is returned as read, without the GPU; any
    other rate, 48 kHz included, goes through the band-limited Resampler. The float32 samples
    are resampled as they are: they are not re-quantised to int16 as PyAV's s16 path does."""
    data = _read_all(input_file)
    if split_stereo:
        x, sr = wavio.wav_channels_f32(data)
        if x.shape[1] != 2:
            raise ValueError(f"split_stereo needs a file with exactly two channels, this one has {x.shape[1]}")
        left, right = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])
        if sr == sampling_rate:
            return left, right
        left, right = resample([left, right], sr, sampling_rate)
        return left, right
    x, sr = wavio.wav_to_f32(data)
    if sr == sampling_rate:
        return x
    return resample(x, sr, sampling_rate)


__all__ = ["Resampler", "resample", "resample_plan", "resample_out_len", "decode_audio"]
