"""Test-side reference for the multilingual models, built on the unchanged oracle
(oracle/whisper.py is generic in cfg.n_vocab, tk.sot_sequence and every special id):

* language probabilities: decoder_logits([[sot]], enc)[:, 0] restricted to the language
  tokens, softmax in float64 (include/janus.h, the language identification rule);
* no_speech_prob at the <|startoftranscript|> index i of a prompt:
  decoder_logits(prompt[:i + 1])[-1], raw softmax in float64;
* tokens: greedy_cached(prompts=..., no_speech=None);
* the planner through janus_decode_plan_describe with janus_decode_rows.no_speech_back
  (PLAN_CASES: the calls tests/golden/plan_descriptions.json records from the commit before
  that field).

No GPU is touched here."""
import ctypes
import json
import os

import numpy as np

from janus_amd import _native as nat
from janus_amd import whisper as jw
from oracle import whisper as ow

I32P = ctypes.POINTER(ctypes.c_int32)


# --------------------------------------------------------------------------- model side
def language_logits(enc, W, cfg, tk):
    """float64 [B][n_languages]: the language tokens' logits of one decoder position holding
    <|startoftranscript|> at position 0 over each window's encoder output."""
    enc = np.asarray(enc, np.float32)
    B = enc.shape[0]
    logits = ow.decoder_logits(np.full((B, 1), tk.sot, np.int64), enc, W, cfg)[:, 0].numpy()
    return logits[:, tk.language_begin:tk.language_begin + tk.n_languages].astype(np.float64)


def language_probs(enc, W, cfg, tk):
    """(probs float64 [B][n_languages], best [B], top-2 logit gap [B])."""
    L = language_logits(enc, W, cfg, tk)
    p = softmax64(L)
    srt = np.sort(L, axis=1)
    gap = srt[:, -1] - srt[:, -2] if L.shape[1] > 1 else np.full(len(L), np.inf)
    return p, np.argmax(L, axis=1), gap


def softmax64(L):
    L = np.asarray(L, np.float64)
    e = np.exp(L - L.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def no_speech_at(prompt, index, enc_row, W, cfg, tk):
    """Raw softmax probability (float64) of tk.no_speech from the logits at position
    ``index`` of ``prompt`` (the positions before it alone decide them: the decoder is
    causal)."""
    logits = ow.decoder_logits(np.asarray([prompt[:index + 1]], np.int64), np.asarray(enc_row)[None],
                               W, cfg)[0, -1].numpy().astype(np.float64)
    return float(softmax64(logits)[tk.no_speech])


def greedy(enc, W, cfg, tk, prompts, max_length, timestamps=True):
    """oracle greedy_cached over per-row prompts: per row dict(tokens, margins, sum_lp)."""
    return ow.greedy_cached(np.asarray(enc, np.float32), W, cfg, tk, max_length=max_length,
                            timestamps=timestamps, prompts=prompts, no_speech=None)


def first_divergence(got, ref_tokens):
    """Index of the first position where the decoded tokens leave the reference's (None:
    they agree over the reference's length)."""
    for i, t in enumerate(ref_tokens):
        if i >= len(got) or int(got[i]) != int(t):
            return i
    return None


# --------------------------------------------------------------------------- the planner
MULTI_PROMPT = [50258, 50259, 50359]
PLAN_CASES = {
    # name -> (config, rows, keywords of describe_plan)
    "default_base_4": ("base.en", 4, {}),
    "default_tiny_64": ("tiny.en", 64, {}),
    "default_small_8": ("small.en", 8, {}),
    "rows_128": ("base.en", 128, {}),
    "persistent_2": ("base.en", 8, dict(persistent=2)),
    "sampled": ("base.en", 4, dict(temperature=0.6)),
    "shared_pairs": ("tiny.en", 10, dict(enc_index=[0] * 5 + [1] * 5)),
    "beam": ("base.en", 8, dict(beam_size=4, prompts=[[50257, 50362]] * 8, enc_index=[0] * 4 + [1] * 4)),
    "stagger": ("base.en", 4, dict(max_length=40, pos_offset=[0, 0, 20, 20], steps=19, stand=[20] * 4,
                                   stand_maxlen=40)),
    "prompts_3_7": ("base.en", 2, dict(max_length=40, prompts=[MULTI_PROMPT, [50361, 1, 2, 3] + MULTI_PROMPT])),
}


def _i32(values):
    a = np.ascontiguousarray(np.asarray(values, np.int32))
    return a, a.ctypes.data_as(I32P)


def describe(lib, cfg, B, no_speech_back=0, persistent=0, max_length=448, cus=256, temperature=0.0,
             beam_size=0, enc_index=None, pos_offset=None, steps=0, stand=None, stand_maxlen=0,
             prompts=None):
    """janus_decode_plan_describe's (text, key) for one planner call; JanusNativeError where
    the planner rejects. no_speech_back 0 leaves the rows' trailing field untouched (zero)."""
    c = jw.janus_whisper_config(cfg.n_mels, cfg.n_audio_ctx, cfg.d_model, cfg.n_heads,
                                cfg.enc_layers, cfg.dec_layers, cfg.n_vocab, cfg.n_text_ctx)
    keep = []
    opt = jw.janus_decode_options()
    pr, opt.prompt = _i32([50257, 50362])
    keep.append(pr)
    opt.prompt_len, opt.max_length, opt.eot = 2, max_length, 50256
    opt.suppress_blank, opt.blank_token = 1, 220
    opt.timestamp_begin, opt.no_timestamps, opt.max_initial_timestamp_index = 50363, 50362, 50
    opt.check_every, opt.persistent = 16, persistent
    rows = jw.janus_decode_rows()
    rows.no_speech_token = 50361
    if no_speech_back:
        rows.no_speech_back = no_speech_back
    if enc_index is not None:
        a, rows.enc_index = _i32(enc_index)
        keep.append(a)
        rows.n_enc = max(enc_index) + 1
    if pos_offset is not None:
        a, rows.pos_offset = _i32(pos_offset)
        keep.append(a)
        rows.steps = steps
    if prompts is not None:
        stride = max(len(p) for p in prompts)
        flat = np.zeros((B, stride), np.int32)
        for b, p in enumerate(prompts):
            flat[b, :len(p)] = p
        a, rows.prompts = _i32(flat)
        ln, rows.prompt_lens = _i32([len(p) for p in prompts])
        keep += [a, ln]
        rows.stride = stride
    st = np.ascontiguousarray(np.asarray(stand if stand is not None else [], np.int32))
    text = ctypes.create_string_buffer(1 << 16)
    key = (ctypes.c_int64 * 256)()
    n_key = ctypes.c_int32(0)
    nat.check(lib.janus_decode_plan_describe(
        ctypes.addressof(c), ctypes.addressof(opt), ctypes.addressof(rows), B, cus, 1, 0,
        ctypes.c_float(temperature), None, beam_size, st.ctypes.data if st.size else None, int(st.size),
        stand_maxlen, ctypes.addressof(text), len(text), ctypes.addressof(key), len(key),
        ctypes.addressof(n_key)))
    del keep
    return text.value.decode(), tuple(key[:n_key.value])


def describe_plan(lib, name, no_speech_back=0):
    model, B, kw = PLAN_CASES[name]
    return describe(lib, jw.CONFIGS[model], B, no_speech_back=no_speech_back, **kw)


def plan_fields(text):
    out = {}
    for line in text.splitlines():
        name, value = line.split("=", 1)
        out[name] = value
    return out


def golden_plans():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_descriptions.json")
    with open(path) as f:
        return json.load(f)
