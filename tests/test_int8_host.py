"""Int8 encoder, host side (no GPU): the faster-whisper compute_type -> engine mapping of
WhisperModel, and the numpy restatement of the row-wise symmetric quantiser
 that tests/test_int8_gpu.py compares the kernels against, checked here on
the rows where the rule has something to say (zeros, a negative maximum, ties)."""
import numpy as np
import pytest

from janus_amd.services.transcriber import COMPUTE_TYPES, resolve_compute_type
from janus_amd.whisper import encoder_compute_mode

F127 = np.float32(127.0)


def quant_rows_np(x):
    """Row-wise symmetric int8 quantiser, every operation in float32 with one rounding:
    amax = max |x|; amax == 0: q = 0, scale = 1; else inv = 127 / amax,
    q = clip(rint(x * inv), -127, 127) (rint: ties to even), scale = amax / 127.
    x [..., K] (float16 / float32) -> (q int8 [..., K], scale float32 [...])."""
    x = np.asarray(x).astype(np.float32)
    amax = np.abs(x).max(axis=-1)
    zero = amax == 0
    safe = np.where(zero, np.float32(1.0), amax).astype(np.float32)
    inv = (F127 / safe).astype(np.float32)
    t = (x * inv[..., None]).astype(np.float32)
    q = np.clip(np.rint(t), -127, 127).astype(np.int8)
    scale = np.where(zero, np.float32(1.0), (safe / F127).astype(np.float32)).astype(np.float32)
    q[zero] = 0
    return q, scale


def exact_int_matmul(A, W):
    """(A.astype(int64) @ W.T.astype(int64)) for int8 A [M][K], W [N][K]: computed in float64
    BLAS, where it is exact (every partial sum is an integer below 127 * 127 * K < 2^53)."""
    acc = A.astype(np.float64) @ W.astype(np.float64).T
    return acc.astype(np.int64)


def dequant_np(acc, a_scale, w_scale, bias):
    """The GEMM epilogue in float32, one rounding per operation:
    y = float32(acc) * (a_scale[m] * w_scale[n]) + bias[n]."""
    s = (a_scale.astype(np.float32)[:, None] * w_scale.astype(np.float32)[None, :]).astype(np.float32)
    t = (acc.astype(np.float32) * s).astype(np.float32)
    return (t + bias.astype(np.float32)[None, :]).astype(np.float32)


# ------------------------------------------------------------------ compute-type mapping
INT8_TYPES = {"int8", "int8_float16", "int8_float32", "int8_bfloat16"}


@pytest.mark.parametrize("ct", COMPUTE_TYPES)
def test_compute_type_mapping(ct):
    assert resolve_compute_type(ct) == ("float16", "float16")
    assert resolve_compute_type(ct, apply_compute_type=False) == ("float16", "float16")
    want = ("int8_float16", "int8") if ct in INT8_TYPES else ("float16", "float16")
    assert resolve_compute_type(ct, apply_compute_type=True) == want


def test_compute_type_mapping_covers_the_int8_types():
    assert INT8_TYPES <= set(COMPUTE_TYPES)
    for bad in ("int4", "", "INT8"):
        for flag in (False, True):
            with pytest.raises(ValueError):
                resolve_compute_type(bad, flag)


def test_encoder_compute_names():
    assert encoder_compute_mode("float16") == 0 and encoder_compute_mode("int8") == 1
    for bad in ("int8_float16", "fp16", None, 1):
        with pytest.raises(ValueError):
            encoder_compute_mode(bad)


# ------------------------------------------------------------------ the numpy quantiser
def test_quantiser_zero_row():
    q, s = quant_rows_np(np.zeros((2, 16), np.float16))
    assert q.dtype == np.int8 and s.dtype == np.float32
    assert not q.any() and np.array_equal(s, np.ones(2, np.float32))
    q, s = quant_rows_np(np.array([[0.0, -0.0] * 8], np.float16))
    assert not q.any() and s[0] == 1.0


def test_quantiser_negative_maximum():
    x = np.zeros((1, 16), np.float16)
    x[0, :4] = [0.25, -3.0, 1.5, 2.5]
    q, s = quant_rows_np(x)
    assert q[0, 1] == -127 and q[0].min() == -127 and q[0].max() < 127
    assert s[0] == np.float32(3.0) / F127
    # the positive neighbour of the maximum stays below 127
    assert q[0, 3] == int(np.rint(np.float32(x[0, 3]) * (F127 / np.float32(3.0))))


def test_quantiser_ties_to_even():
    x = np.zeros((1, 16), np.float16)
    x[0, :5] = [127.0, 0.5, 1.5, 2.5, -0.5]
    q, s = quant_rows_np(x)
    assert s[0] == 1.0
    assert q[0, :5].tolist() == [127, 0, 2, 2, 0]
    assert not q[0, 5:].any()


def test_quantiser_subnormal_row_and_clip():
    x = np.zeros((1, 16), np.float16)
    tiny = np.float16(2.0 ** -24)                      # the smallest fp16 subnormal
    x[0, :3] = [tiny, -3 * tiny, 2 * tiny]
    q, s = quant_rows_np(x)
    assert q[0, :3].tolist() == [42, -127, 85]         # rint(127 / 3) = 42, rint(254 / 3) = 85
    assert s[0] == np.float32(3 * 2.0 ** -24) / F127
    assert np.abs(quant_rows_np(np.random.default_rng(0).standard_normal((8, 64)))[0]).max() == 127


def test_epilogue_restatement_rounds_once():
    acc = np.array([[49548288 - 254, 3]], np.int64)    # the first is a tie at 2^25..2^26 (ulp 4)
    y = dequant_np(acc, np.ones(1, np.float32), np.ones(2, np.float32), np.zeros(2, np.float32))
    assert y.dtype == np.float32
    assert int(y[0, 0]) == 49548032 and (49548288 - 254) % 4 == 2   # tie -> the even mantissa
    A = np.full((2, 128), 127, np.int8)
    assert exact_int_matmul(A, A).tolist() == [[127 * 127 * 128] * 2] * 2
