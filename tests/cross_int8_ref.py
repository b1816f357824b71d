"""Reference for the int8 cross-attention operand (include/janus.h janus_whisper_set_cross_compute).

* ``quantise``: CTranslate2's row-wise symmetric rule in numpy float32, one key row at a time:
  amax = max |x|, q = clamp(rint(x * (127 / amax)), -127, 127), s = amax / 127; a zero row
  gives q = 0, s = 1. The same rule tests/test_int8_gpu.py holds the engine's quantiser to.
* ``dequantised``: E' = fp16(float32(q) * s), the product in float32, rounded once — the encoder
  output the decoder's cross-attention sees with cross_compute="int8". The references of the
  GPU tests are tests/decoder_ref.py's ``hidden`` (imported unchanged) on E' instead of E.
* ``outlier_inputs``: decoder_ref.inputs with the edge rows of the GPU tests planted in E: a
  zero key row, a row whose amax sits on a negative element, and the value 16.0 in one seeded
  column of every other key row (a LayerNorm output's rare large coordinate: it sets the row's
  scale, so the other 127 levels are spent on a sixth of their range).
* ``describe``: the planner through janus_decode_plan_describe_cross.
"""
import ctypes

import numpy as np

import decoder_ref as ref   # noqa: F401  (the GPU tests' hidden(), metrics(), K_BOUND)
from janus_amd import _native as nat
from janus_amd import whisper as jw

F32 = np.float32
I32P = ctypes.POINTER(ctypes.c_int32)


def quantise(x):
    """x [..][d] (any float type) -> (q int8 [..][d], s float32 [..]), per last-axis row."""
    x = np.asarray(x).astype(F32)
    amax = np.abs(x).max(axis=-1)
    zero = amax == 0
    safe = np.where(zero, F32(1), amax).astype(F32)
    inv = (F32(127) / safe).astype(F32)
    q = np.clip(np.rint((x * inv[..., None]).astype(F32)), -127, 127).astype(np.int8)
    s = np.where(zero, F32(1), (safe / F32(127)).astype(F32)).astype(F32)
    return q, s


def dequantised(enc):
    """E' fp16 of enc fp16 [..][Te][d]: (q.astype(f32) * s[:, None]).astype(f16) per key row."""
    q, s = quantise(enc)
    return (q.astype(F32) * s[..., None]).astype(np.float16)


OUTLIER = 16.0


def outlier_inputs(cfg, rows, T, seed, n_enc=None):
    """decoder_ref.inputs with the edge rows planted in every encoder row: key 3 all zeros, key 5
    with its largest magnitude on a negative element (-6.0 at column 7), and OUTLIER in one
    seeded column of every other key row (even keys; the zero row stays zero)."""
    tokens, enc = ref.inputs(cfg, rows, T, seed, n_enc)
    enc = enc.copy()
    g = np.random.default_rng(seed + 1000)
    Te, d = cfg.n_audio_ctx, cfg.d_model
    for e in range(enc.shape[0]):
        cols = g.integers(0, d, size=Te)
        for t in range(0, Te, 2):
            enc[e, t, cols[t]] = OUTLIER
        enc[e, 5] = np.clip(enc[e, 5], -4.0, 4.0)
        enc[e, 5, 7] = -6.0
        enc[e, 3] = 0.0
    return tokens, enc


def describe(lib, cfg, B, cross=0, flags=0, persistent=0, max_length=448, cus=256, temperature=0.0,
             beam_size=0, enc_index=None, pos_offset=None, steps=0, stand=None, stand_maxlen=0,
             prompts=None):
    """janus_decode_plan_describe_cross's (text, key) for one planner call with the context's
    cross compute ``cross`` (0 float16, 1 int8); JanusNativeError where the planner rejects."""
    c = jw.janus_whisper_config(cfg.n_mels, cfg.n_audio_ctx, cfg.d_model, cfg.n_heads,
                                cfg.enc_layers, cfg.dec_layers, cfg.n_vocab, cfg.n_text_ctx)
    keep = []

    def i32(values):
        a = np.ascontiguousarray(np.asarray(values, np.int32))
        keep.append(a)
        return a.ctypes.data_as(I32P)
    opt = jw.janus_decode_options()
    opt.prompt = i32([50257, 50362])
    opt.prompt_len, opt.max_length, opt.eot = 2, max_length, 50256
    opt.suppress_blank, opt.blank_token = 1, 220
    opt.timestamp_begin, opt.no_timestamps, opt.max_initial_timestamp_index = 50363, 50362, 50
    opt.check_every, opt.persistent, opt.path_flags = 16, persistent, flags
    rows = jw.janus_decode_rows()
    rows.no_speech_token = 50361
    if enc_index is not None:
        rows.enc_index = i32(enc_index)
        rows.n_enc = max(enc_index) + 1
    if pos_offset is not None:
        rows.pos_offset = i32(pos_offset)
        rows.steps = steps
    if prompts is not None:
        stride = max(len(p) for p in prompts)
        flat = np.zeros((B, stride), np.int32)
        for b, p in enumerate(prompts):
            flat[b, :len(p)] = p
        rows.prompts = i32(flat)
        rows.prompt_lens = i32([len(p) for p in prompts])
        rows.stride = stride
    st = np.ascontiguousarray(np.asarray(stand if stand is not None else [], np.int32))
    text = ctypes.create_string_buffer(1 << 16)
    key = (ctypes.c_int64 * 256)()
    n_key = ctypes.c_int32(0)
    nat.check(lib.janus_decode_plan_describe_cross(
        ctypes.addressof(c), ctypes.addressof(opt), ctypes.addressof(rows), B, cus, 1, 0,
        ctypes.c_float(temperature), None, beam_size, st.ctypes.data if st.size else None, int(st.size),
        stand_maxlen, int(cross), ctypes.addressof(text), len(text), ctypes.addressof(key), len(key),
        ctypes.addressof(n_key)))
    del keep
    return text.value.decode(), tuple(key[:n_key.value])
