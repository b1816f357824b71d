"""The band-limited resampling rule of include/janus.h, evaluated in numpy float64 straight
from the formula (never from the library's tap table): the yardstick of test_resample_host.py
and test_resample_gpu.py.

    g = gcd, L = sr_out / g, M = sr_in / g, s = min(1, L / M), Z = 32, beta = 10, W = Z / s
    phi(u) = s sinc(s u) I0(beta sqrt(1 - (u / W)^2)) / I0(beta), |u| < W
    output n: p = n mod L, i = n div L, c = (p M) div L, frac = (p M mod L) / L,
    h_p[k] = phi(frac - k) over |frac - k| < W, normalised to sum 1,
    y[n] = sum_k h_p[k] x[i M + c + k], x = 0 outside [0, n_in), n_out = ceil(n_in L / M).

Which integers k satisfy |frac - k| < W is decided on integers (|r - k L| < Z max(L, M), r =
p M mod L), so that the tap COUNT never hangs on a rounding; the tap values are the formula."""
import math

import numpy as np

Z, BETA = 32, 10.0


def reduce_rates(sr_in: int, sr_out: int):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def half_width(sr_in: int, sr_out: int) -> float:
    L, M = reduce_rates(sr_in, sr_out)
    return Z / min(1.0, L / M)


def phase_taps(sr_in: int, sr_out: int):
    """[(first, h)] per phase: h float64 (normalised), output i L + p = sum_t h[t] x[i M + first + t]."""
    L, M = reduce_rates(sr_in, sr_out)
    s = min(1.0, L / M)
    W = Z / s
    wn = Z * max(L, M)
    out = []
    for p in range(L):
        c, r = divmod(p * M, L)
        frac = r / L
        kmin = (r - wn) // L + 1            # least k with r - k L < wn
        kmax = -((-(r + wn)) // L) - 1      # greatest k with k L - r < wn
        k = np.arange(kmin, kmax + 1, dtype=np.float64)
        u = frac - k
        h = s * np.sinc(s * u) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (u / W) ** 2))) / np.i0(BETA)
        out.append((c + kmin, h / h.sum()))
    return out


def out_len(n_in: int, sr_in: int, sr_out: int) -> int:
    L, M = reduce_rates(sr_in, sr_out)
    return -(-n_in * L // M)


def resample(x, sr_in: int, sr_out: int):
    """x float [n_in] or [rows][n_in] -> (y float64 [.. n_out], T int [L] taps per phase,
    norm float64 [L] = ||h_p||_1)."""
    x = np.asarray(x, dtype=np.float64)
    L, M = reduce_rates(sr_in, sr_out)
    taps = phase_taps(sr_in, sr_out)
    n_in = x.shape[-1]
    n_out = out_len(n_in, sr_in, sr_out)
    front = max(0, -min(f for f, _ in taps))
    periods = -(-n_out // L) if n_out else 0
    back = max(0, (periods - 1) * M + max(f + len(h) for f, h in taps) - n_in) if n_out else 0
    xp = np.concatenate([np.zeros(x.shape[:-1] + (front,)), x, np.zeros(x.shape[:-1] + (back,))], axis=-1)
    y = np.zeros(x.shape[:-1] + (n_out,))
    for p, (first, h) in enumerate(taps):
        i = np.arange(len(range(p, n_out, L)), dtype=np.int64)
        if not len(i):
            continue
        for a in range(0, len(i), 4096):   # bounded gathers
            ii = i[a:a + 4096]
            idx = (ii * M + first + front)[:, None] + np.arange(len(h))[None, :]
            y[..., p + ii * L] = xp[..., idx] @ h
    T = np.array([len(h) for _, h in taps])
    norm = np.array([np.abs(h).sum() for _, h in taps])
    return y, T, norm
