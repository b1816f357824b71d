"""Test-side reference for the 1280-wide, 20-head family (large-v3, large-v3-turbo,
distil-large-v3), built on the unchanged oracle (oracle/whisper.py is generic in cfg.n_mels,
cfg.d_model, cfg.n_heads, cfg.n_vocab and every special id of the tokenizer):

* CUT: the real width, heads, mel bins and vocabulary over 2 encoder and 2 decoder layers;
* language probabilities over the layout's 100 language tokens: the rule of
  tests/multilingual_ref.py (which reads tk.n_languages) restated for this layout;
* the planner through janus_decode_plan_describe with path flags and this layout's ids;
* the vocabulary projection's partials (LogitPart, 56 bytes) merged on the host, and the
  float64 reference of the same fp16 operands under the decoding rules.

No GPU is touched here."""
import ctypes

import numpy as np

import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd import whisper as jw

CUT = jw.WhisperConfig("large-cut", 1280, 20, 2, 2, n_mels=128, n_vocab=tok.N_VOCAB_V3)
V = CUT.n_vocab            # 51 866 = 16 * 3241 + 10: the projection's last tile holds 10 columns
ROW_GROUP = 32             # rows of one block of the vocabulary projection at K = 1280


def language_probs(enc, W, cfg, tk):
    """(probs float64 [B][100], best [B], top-2 logit gap [B]) of one <|startoftranscript|>
    position over each window's encoder output: softmax over the 100 language tokens alone."""
    assert tk.n_languages == 100 and tk.languages[-1] == "yue"
    return mr.language_probs(enc, W, cfg, tk)


# --------------------------------------------------------------------------- the planner
def describe(lib, cfg, B, persistent=0, max_length=448, cus=256, temperature=0.0, enc_index=None,
             path_flags=0, beam_size=0):
    """janus_decode_plan_describe's text for one planner call on the large-v3 layout (per-row
    prompts [sot, <|en|>, <|transcribe|>]); JanusNativeError where the planner rejects."""
    tk = tok.WhisperTokenizer(n_vocab=cfg.n_vocab) if cfg.multilingual else tok.WhisperTokenizer()
    c = jw.janus_whisper_config(cfg.n_mels, cfg.n_audio_ctx, cfg.d_model, cfg.n_heads,
                                cfg.enc_layers, cfg.dec_layers, cfg.n_vocab, cfg.n_text_ctx)
    keep = []

    def i32(values):
        a = np.ascontiguousarray(np.asarray(values, np.int32))
        keep.append(a)
        return a.ctypes.data_as(mr.I32P)

    opt = jw.janus_decode_options()
    sot = list(tk.sot_sequence)
    opt.prompt = i32(sot)
    opt.prompt_len, opt.max_length, opt.eot = len(sot), max_length, tk.eot
    opt.suppress_blank, opt.blank_token = 1, tk.blank
    opt.timestamp_begin, opt.no_timestamps = tk.timestamp_begin, tk.no_timestamps
    opt.max_initial_timestamp_index = 50
    opt.check_every, opt.persistent, opt.path_flags = 16, persistent, path_flags
    rows = jw.janus_decode_rows()
    rows.no_speech_token = tk.no_speech
    rows.no_speech_back = len(sot) - 1
    rows.prompts = i32([sot] * B)
    rows.prompt_lens = i32([len(sot)] * B)
    rows.stride = len(sot)
    if enc_index is not None:
        rows.enc_index = i32(enc_index)
        rows.n_enc = max(enc_index) + 1
    text = ctypes.create_string_buffer(1 << 16)
    key = (ctypes.c_int64 * 256)()
    n_key = ctypes.c_int32(0)
    nat.check(lib.janus_decode_plan_describe(
        ctypes.addressof(c), ctypes.addressof(opt), ctypes.addressof(rows), B, cus, 1, 0,
        ctypes.c_float(temperature), None, beam_size, None, 0, 0, ctypes.addressof(text), len(text),
        ctypes.addressof(key), len(key), ctypes.addressof(n_key)))
    del keep
    return mr.plan_fields(text.value.decode())


# --------------------------------------------------------------------------- the projection
PART_FIELDS = [("m_all", "<f4"), ("s_all", "<f4"), ("m_text", "<f4"), ("m_ts", "<f4"), ("s_ts", "<f4"),
               ("b_all_v", "<f4"), ("b_all_i", "<i4"), ("b_ts_v", "<f4"), ("b_ts_i", "<i4"), ("t_v", "<f4"),
               ("m_raw", "<f4"), ("s_raw", "<f4"), ("b_all_r", "<f4"), ("b_ts_r", "<f4")]
PART_DTYPE = np.dtype(PART_FIELDS)
assert PART_DTYPE.itemsize == 56


def merge_parts(parts):
    """parts: structured [B][nblk] (PART_DTYPE) -> per row dict(lse_all, lse_ts, m_text, best,
    best_v, best_ts, best_ts_v, lse_raw, t_v): the selector's reduction in float64, first index
    on ties."""
    out = []
    for row in parts:
        def lse(m, s):
            m = row[m].astype(np.float64)
            s = row[s].astype(np.float64)
            if not np.isfinite(m).any():
                return -np.inf
            M = m[np.isfinite(m)].max()
            return float(M + np.log((s * np.exp(np.where(np.isfinite(m), m - M, -np.inf))).sum()))

        def best(v, i):
            vv, ii = row[v].astype(np.float64), row[i].astype(np.int64)
            k = np.lexsort((ii, -vv))[0]
            return int(ii[k]), float(vv[k])
        b, bv = best("b_all_v", "b_all_i")
        t, tv = best("b_ts_v", "b_ts_i")
        out.append(dict(lse_all=lse("m_all", "s_all"), lse_ts=lse("m_ts", "s_ts"),
                        m_text=float(row["m_text"].max()), best=b, best_v=bv, best_ts=t, best_ts_v=tv,
                        lse_raw=lse("m_raw", "s_raw"), t_v=float(row["t_v"].max())))
    return out


def allowed_mask(V, smask, rr, eot, blank, ts_begin, no_timestamps, max_initial_ts, suppress_blank=1):
    """bool [V]: the decoding rules of one row (decoder.hip allowed_unmasked) before the
    timestamp-mass rule. rr = (sample_begin, suppress_all_ts, suppress_text, ts_floor)."""
    sample_begin, sup_all_ts, sup_text, ts_floor = rr
    t = np.arange(V)
    ok = ~np.asarray(smask[:V], bool)
    if sample_begin and suppress_blank:
        ok &= (t != blank) & (t != eot)
    if ts_begin >= 0:
        is_ts = t >= ts_begin
        ok &= t != no_timestamps
        if sup_all_ts:
            ok &= ~is_ts
        if sup_text:
            ok &= ~(t < eot)
        ok &= ~(is_ts & (t < ts_floor))
        if sample_begin:
            ok &= is_ts
            if max_initial_ts >= 0:
                ok &= ~(t > ts_begin + max_initial_ts)
    return ok
