"""Whisper model host side: configs, weights, front-end constants and the GPU engine.

The engine owns one ``janus_whisper`` context (include/janus.h) and calls
``janus_whisper_logmel`` -> ``janus_whisper_encode`` -> ``janus_whisper_decode_greedy``
on torch-allocated device buffers and torch's current stream.

Weights: if ``JANUS_WHISPER_DIR`` points at a Hugging Face Whisper checkpoint
(``model.safetensors``), it is loaded (safetensors, no pickle). Otherwise the model has
seeded synthetic weights of the real shapes (no checkpoints are reachable offline).
"""
import ctypes
import dataclasses
import math
import os

import numpy as np
import torch

from . import _native as nat
from . import tokenizer as tok


@dataclasses.dataclass(frozen=True)
class WhisperConfig:
    name: str
    d_model: int
    n_heads: int
    enc_layers: int
    dec_layers: int
    n_mels: int = 80
    n_audio_ctx: int = 1500
    n_vocab: int = tok.N_VOCAB_EN
    n_text_ctx: int = 448

    @property
    def ffn(self):
        return 4 * self.d_model

    @property
    def multilingual(self) -> bool:
        """The 51 865- or 51 866-entry vocabulary: language and task tokens (tokenizer.py picks
        the layout from n_vocab)."""
        return self.n_vocab >= tok.N_VOCAB_MULTILINGUAL


CONFIGS = {
    "tiny.en": WhisperConfig("tiny.en", 384, 6, 4, 4),
    "base.en": WhisperConfig("base.en", 512, 8, 6, 6),
    "small.en": WhisperConfig("small.en", 768, 12, 12, 12),
    # distil-whisper: small.en's encoder over a 4-layer decoder
    "distil-small.en": WhisperConfig("distil-small.en", 768, 12, 12, 4),
    # the multilingual checkpoints: the *.en siblings' shapes over the 51 865-entry vocabulary
    "tiny": WhisperConfig("tiny", 384, 6, 4, 4, n_vocab=tok.N_VOCAB_MULTILINGUAL),
    "base": WhisperConfig("base", 512, 8, 6, 6, n_vocab=tok.N_VOCAB_MULTILINGUAL),
    "small": WhisperConfig("small", 768, 12, 12, 12, n_vocab=tok.N_VOCAB_MULTILINGUAL),
    # the large-v3 family: d_model 1280, 20 heads, 128 mel bins, the 100-language vocabulary;
    # turbo and distil keep large-v3's encoder over a 4- / 2-layer decoder
    "large-v3": WhisperConfig("large-v3", 1280, 20, 32, 32, n_mels=128, n_vocab=tok.N_VOCAB_V3),
    "large-v3-turbo": WhisperConfig("large-v3-turbo", 1280, 20, 32, 4, n_mels=128, n_vocab=tok.N_VOCAB_V3),
    "distil-large-v3": WhisperConfig("distil-large-v3", 1280, 20, 32, 2, n_mels=128, n_vocab=tok.N_VOCAB_V3),
}
# the 1024-wide family: d_model 1024, 16 heads, 80 mel bins, the *.en vocabulary; distil keeps
# medium.en's encoder over a 2-layer decoder. (The multilingual `medium` has the same shapes
# over 51 865 ids; its name is not registered.)
CONFIGS["medium.en"] = WhisperConfig("medium.en", 1024, 16, 24, 24)
CONFIGS["distil-medium.en"] = WhisperConfig("distil-medium.en", 1024, 16, 24, 2)
MODEL_ALIASES = {"turbo": "large-v3-turbo"}   # faster-whisper's short name


def resolve_model(name: str) -> str:
    """A model name or alias -> its CONFIGS key; ValueError for an unknown one."""
    name = MODEL_ALIASES.get(name, name)
    if name not in CONFIGS:
        raise ValueError(f"unknown model size {name!r}; one of {sorted(CONFIGS) + sorted(MODEL_ALIASES)}")
    return name


def large_family(cfg) -> bool:
    """The models past small's width: the 1024-wide, 16-head pair and the
    1280-wide, 20-head family (§5o). They share the launch path, the gathered shared rows, the
    row-grouped vocabulary projection (48 / 32 rows) and the refusals of beam search and the
    int8 encoder."""
    return cfg is not None and getattr(cfg, "d_model", 0) > 768


def wide_name(cfg) -> str:
    """"1024-wide" / "1280-wide": how a refusal names a large_family() model's width."""
    return f"{cfg.d_model}-wide"


def check_family_features(cfg, beam_size: int = 1, word_timestamps: bool = False, alignment_heads=None) -> None:
    """What the models past d_model 768 do not run in this build (second
    tier): beam search (no beam partials of the vocabulary projection at K = 1024 / 1280) and
    word timestamps — above d_model 1024 always, at 1024 when the alignment set holds more than
    ALIGN_MAX_HEADS heads. ``alignment_heads``: the engine's named set (None: the default set,
    every head of the last half of the decoder layers — 192 on medium.en, 16 on
    distil-medium.en). NotImplementedError naming the feature, before any GPU work."""
    if not large_family(cfg):
        return
    if beam_size > 1:
        raise NotImplementedError(f"beam_size {beam_size} on {cfg.name}: the {wide_name(cfg)} models decode "
                                  "greedily or sampled (beam_size 1) in this build")
    if word_timestamps and cfg.d_model > 1024:
        raise NotImplementedError(f"word_timestamps on {cfg.name}: the alignment pass is not built for "
                                  "the 1280-wide, 20-head models")
    if word_timestamps:
        n = len(alignment_heads) if alignment_heads is not None else len(default_alignment_heads(cfg))
        if n > ALIGN_MAX_HEADS:
            raise NotImplementedError(f"word_timestamps on {cfg.name}: its alignment set has {n} heads (the default: "
                                      f"every head of the last half of the decoder layers) and the alignment pass "
                                      f"takes at most {ALIGN_MAX_HEADS}; name up to {ALIGN_MAX_HEADS} with "
                                      "alignment_heads=[(layer, head), ...]")


def check_encoder_compute(cfg, mode) -> None:
    """int8 encoder projections stop at K = 3072 (quant_rows_i8); fc2 of a 1024- / 1280-wide
    model has K = 4096 / 5120: NotImplementedError there."""
    if mode in ("int8", ENCODER_COMPUTE["int8"]) and large_family(cfg):
        raise NotImplementedError(f"int8 encoder compute on {cfg.name}: fc2's K = {cfg.ffn} exceeds the "
                                  "int8 path's 3072; these models run float16")


class janus_whisper_config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("n_mels", "n_audio_ctx", "d_model", "n_heads",
                                            "enc_layers", "dec_layers", "n_vocab", "n_text_ctx")]


class janus_decode_options(ctypes.Structure):
    _fields_ = [("prompt", ctypes.POINTER(ctypes.c_int32)), ("prompt_len", ctypes.c_int),
                ("max_length", ctypes.c_int), ("eot", ctypes.c_int),
                ("suppress", ctypes.POINTER(ctypes.c_int32)), ("n_suppress", ctypes.c_int),
                ("suppress_blank", ctypes.c_int), ("blank_token", ctypes.c_int),
                ("timestamp_begin", ctypes.c_int), ("no_timestamps", ctypes.c_int),
                ("max_initial_timestamp_index", ctypes.c_int), ("check_every", ctypes.c_int),
                ("xattn_splits", ctypes.c_int), ("cu_count", ctypes.c_int),
                ("state_slot", ctypes.c_int), ("logits_blocks", ctypes.c_int),
                ("msplit_rows_n", ctypes.c_int), ("persistent", ctypes.c_int),
                ("path_flags", ctypes.c_uint32), ("lanes", ctypes.c_int),
                ("repetition_penalty", ctypes.c_float), ("no_repeat_ngram_size", ctypes.c_int)]


# janus_decode_options.path_flags (include/janus.h JANUS_DEC_PATH_*): alternative decoder
# paths the parity tests hold bit-identical to the default; 0 = the measured default
DEC_PATH_NO_GRAPH = 0x0001
DEC_PATH_NO_XABSORB = 0x0002
DEC_PATH_NO_XPAIR = 0x0004
DEC_PATH_XGROUP = 0x0008
DEC_PATH_FUSED_LN = 0x0010
DEC_PATH_LN_FUSE = 0x0020
DEC_PATH_RESID_LN = 0x0040
DEC_PATH_NO_CVP = 0x0080
DEC_PATH_CVP = 0x0100
DEC_PATH_NO_SEL_EMBED = 0x0200
DEC_PATH_NO_EMBED_LN = 0x0400
DEC_PATH_LN_PROLOGUE = 0x0800
DEC_PATH_SEG_2CU = 0x10000
DEC_PATH_XFWD = 0x20000


def dec_path_xrows(n: int) -> int:
    """JANUS_DEC_PATH_XROWS(n): 12 heads / d_model 768, rows sharing an encoder row read it
    in place in blocks of up to n = 2 or 4 rows (default there: a gathered copy per row)."""
    return ((n >> 1) & 3) << 18


def dec_path_ln_mask(m: int) -> int:
    """JANUS_DEC_PATH_LN_MASK(m): LayerNorm-into-prologue mask m instead of the default."""
    return DEC_PATH_LN_PROLOGUE | ((m & 15) << 12)


class janus_decode_rows(ctypes.Structure):
    _fields_ = [("prompts", ctypes.POINTER(ctypes.c_int32)),
                ("prompt_lens", ctypes.POINTER(ctypes.c_int32)),
                ("stride", ctypes.c_int), ("no_speech_token", ctypes.c_int),
                ("enc_index", ctypes.POINTER(ctypes.c_int32)), ("n_enc", ctypes.c_int),
                ("pos_offset", ctypes.POINTER(ctypes.c_int32)), ("steps", ctypes.c_int),
                ("no_speech_back", ctypes.c_int)]


# ----------------------------------------------------------------- front end
def sinusoids(length: int, channels: int, max_timescale: float = 10000.0) -> np.ndarray:
    """Whisper's fixed encoder positional embedding (openai whisper model.sinusoids)."""
    inc = np.log(max_timescale) / (channels // 2 - 1)
    inv = np.exp(-inc * np.arange(channels // 2))
    t = np.arange(length)[:, None] * inv[None, :]
    return np.concatenate([np.sin(t), np.cos(t)], axis=1).astype(np.float32)


def hz_to_mel_slaney(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, np.log(6.4) / 27.0
    mel = f / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mel)


def mel_to_hz_slaney(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters(sr=16000, n_fft=400, n_mels=80, fmin=0.0, fmax=8000.0) -> np.ndarray:
    """Slaney-normalised, slaney-scale triangular mel filters, [n_fft//2+1][n_mels]
    (librosa.filters.mel(htk=False, norm='slaney'), as faster-whisper's get_mel_filters)."""
    fft_freqs = np.linspace(0, sr // 2, 1 + n_fft // 2)
    mel_pts = np.linspace(hz_to_mel_slaney(fmin), hz_to_mel_slaney(fmax), n_mels + 2)
    f_pts = mel_to_hz_slaney(mel_pts)
    fdiff = np.diff(f_pts)
    ramps = f_pts[:, None] - fft_freqs[None, :]
    w = np.zeros((n_mels, len(fft_freqs)))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])
    w *= enorm[:, None]
    return w.T.astype(np.float32)  # [201][n_mels]


def mel_constants(n_mels: int = 80):
    """("mel.basis" [400][416], "mel.filters" [208][n_mels]) for janus_whisper_set_tensor;
    n_mels 80 or 128."""
    if n_mels not in (80, 128):
        raise ValueError(f"mel_constants: 80 or 128 bins, not {n_mels}")
    n = np.arange(400)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / 400)  # periodic (torch.hann_window / np.hanning(401)[:-1])
    k = np.arange(201)
    ang = 2 * np.pi * np.outer(n, k) / 400
    basis = np.zeros((400, 416))
    basis[:, :201] = hann[:, None] * np.cos(ang)
    basis[:, 208:208 + 201] = hann[:, None] * np.sin(ang)
    filt = np.zeros((208, n_mels), np.float32)
    filt[:201] = mel_filters(n_mels=n_mels)
    return basis.astype(np.float32), filt


# -------------------------------------------------------------------- weights
def synthetic_weights(cfg: WhisperConfig, seed: int = 0) -> dict:
    """Seeded fp32 weights of the real shapes, HF naming (no 'model.' prefix)."""
    g = torch.Generator().manual_seed(seed)
    d, ff = cfg.d_model, cfg.ffn
    W = {}

    def rn(name, *shape, std=0.02):
        W[name] = (torch.randn(*shape, generator=g) * std).numpy().astype(np.float32)

    def ln(name):
        W[name + ".weight"] = (1.0 + 0.1 * torch.randn(d, generator=g)).numpy().astype(np.float32)
        W[name + ".bias"] = (0.02 * torch.randn(d, generator=g)).numpy().astype(np.float32)

    rn("encoder.conv1.weight", d, cfg.n_mels, 3, std=1.0 / math.sqrt(cfg.n_mels * 3))
    rn("encoder.conv1.bias", d)
    rn("encoder.conv2.weight", d, d, 3, std=1.0 / math.sqrt(d * 3))
    rn("encoder.conv2.bias", d)
    W["encoder.embed_positions.weight"] = sinusoids(cfg.n_audio_ctx, d)

    def attn(p, cross=False):
        for n in ("q", "k", "v", "out"):
            rn(f"{p}.{n}_proj.weight", d, d, std=1.0 / math.sqrt(d))
            if n != "k":
                rn(f"{p}.{n}_proj.bias", d)

    def mlp(p):
        rn(f"{p}.fc1.weight", ff, d, std=1.0 / math.sqrt(d))
        rn(f"{p}.fc1.bias", ff)
        rn(f"{p}.fc2.weight", d, ff, std=1.0 / math.sqrt(ff))
        rn(f"{p}.fc2.bias", d)

    for i in range(cfg.enc_layers):
        p = f"encoder.layers.{i}"
        attn(p + ".self_attn")
        ln(p + ".self_attn_layer_norm")
        mlp(p)
        ln(p + ".final_layer_norm")
    ln("encoder.layer_norm")
    rn("decoder.embed_tokens.weight", cfg.n_vocab, d, std=0.05)
    rn("decoder.embed_positions.weight", cfg.n_text_ctx, d, std=0.02)
    for i in range(cfg.dec_layers):
        p = f"decoder.layers.{i}"
        attn(p + ".self_attn")
        ln(p + ".self_attn_layer_norm")
        attn(p + ".encoder_attn")
        ln(p + ".encoder_attn_layer_norm")
        mlp(p)
        ln(p + ".final_layer_norm")
    ln("decoder.layer_norm")
    return engine_weights(W)


# tensors the engine reads in fp32 (whisper.cpp: the decoder's positional table is added
# to the token embedding in fp32); every other matrix is stored fp16 on the GPU
FP32_MATRICES = frozenset({"decoder.embed_positions.weight"})


def engine_weights(W: dict) -> dict:
    """The numbers the engine multiplies: every matrix the GPU stores in fp16 (conv
    kernels, projections, the token embedding, the encoder's positional table; ndim >= 2)
    rounded to fp16, as a CTranslate2 float16 conversion stores them; biases, LayerNorm
    parameters and the fp32-consumed tables (FP32_MATRICES) stay fp32. The oracle is run on
    these weights, so parity measures arithmetic, not weight rounding."""
    return {k: (v.astype(np.float16).astype(np.float32) if v.ndim >= 2 and k not in FP32_MATRICES
                else v.astype(np.float32))
            for k, v in W.items()}


def load_weights(cfg: WhisperConfig, seed: int = 0) -> dict:
    """``JANUS_WHISPER_DIR/model.safetensors`` (a Hugging Face Whisper checkpoint: names
    ``model.encoder.*`` / ``model.decoder.*``, fp16 or fp32; ``proj_out.weight`` must be
    the tied token embedding) mapped to the engine's names, else seeded synthetic weights
    of the real shapes."""
    path = os.environ.get("JANUS_WHISPER_DIR")
    if path and os.path.exists(os.path.join(path, "model.safetensors")):
        from safetensors.numpy import load_file
        raw = load_file(os.path.join(path, "model.safetensors"))
        W = {k[len("model."):] if k.startswith("model.") else k: v for k, v in raw.items()}
        proj = W.pop("proj_out.weight", None)
        if proj is not None and not np.array_equal(proj, W.get("decoder.embed_tokens.weight")):
            raise ValueError("proj_out.weight differs from decoder.embed_tokens.weight: the "
                             "engine's vocabulary projection is the tied embedding")
        emb = W.get("decoder.embed_tokens.weight")
        if emb is None or emb.shape != (cfg.n_vocab, cfg.d_model):
            raise ValueError(f"checkpoint does not match {cfg.name}: decoder.embed_tokens.weight "
                             f"{None if emb is None else emb.shape}")
        # the stem decides the feature size: 80 or 128 mel bins (large-v3 family)
        conv1 = W.get("encoder.conv1.weight")
        if conv1 is None or tuple(conv1.shape) != (cfg.d_model, cfg.n_mels, 3):
            raise ValueError(f"checkpoint does not match {cfg.name}: encoder.conv1.weight "
                             f"{None if conv1 is None else tuple(conv1.shape)}, the config has "
                             f"{(cfg.d_model, cfg.n_mels, 3)}")
        # depth per side: a distil checkpoint keeps the teacher's encoder (12 layers at
        # small.en's width) over a 4-layer decoder, so the two counts are checked apart
        for side, want in (("encoder", cfg.enc_layers), ("decoder", cfg.dec_layers)):
            have = checkpoint_layers(W, side)
            if have != want:
                raise ValueError(f"checkpoint does not match {cfg.name}: {have} {side} layers, "
                                 f"the config has {want}")
        return engine_weights(W)
    return synthetic_weights(cfg, seed)


def checkpoint_layers(W: dict, side: str) -> int:
    """Layers a checkpoint holds on one side ("encoder" / "decoder"): 1 + the largest index
    among its ``<side>.layers.<i>.`` tensor names (0 when it has none)."""
    pre = side + ".layers."
    idx = [int(k[len(pre):].split(".", 1)[0]) for k in W if k.startswith(pre)]
    return max(idx) + 1 if idx else 0


# --------------------------------------------------------------------- engine
BEAM_MAX = 8           # largest beam_size (csrc/decoder.h kBeamMax)
BEAM_MAX_ROWS = 512    # windows x beam_size of one beam decode (kSkinnyMaxRows)


def resolve_suppress_tokens(tokenizer, suppress_tokens, n_vocab: int):
    """faster-whisper's get_suppressed_tokens: None or [-1] is the tokenizer's default set
    (the non-speech tokens and the five always-suppressed specials); a list holding -1 is that
    set plus the list's other ids; a list without -1 (or []) is the list plus the five
    specials. Sorted ids; ValueError for an id outside the vocabulary."""
    if suppress_tokens is None:
        return list(tokenizer.suppress_tokens())
    ids = [int(t) for t in suppress_tokens]
    bad = [t for t in ids if t != -1 and not 0 <= t < n_vocab]
    if bad:
        raise ValueError(f"suppress_tokens: ids {bad} outside the vocabulary (0 .. {n_vocab - 1})")
    s = set(t for t in ids if t >= 0)
    if -1 in ids:
        s.update(tokenizer.suppress_tokens())
    t = tokenizer
    s.update([t.transcribe, t.translate, t.sot, t.sot_prev, t.sot_lm])
    return sorted(s)


def check_history_args(repetition_penalty, no_repeat_ngram_size, beam_size: int = 1):
    """The history rules' arguments (include/janus.h janus_decode_options): a penalty > 0
    (1 = off), an n-gram size >= 0 (0 = off); with beam search neither is built."""
    if not repetition_penalty > 0:
        raise ValueError("repetition_penalty must be > 0 (1 = off)")
    if int(no_repeat_ngram_size) != no_repeat_ngram_size or no_repeat_ngram_size < 0:
        raise ValueError("no_repeat_ngram_size must be an integer >= 0 (0 = off)")
    if beam_size > 1 and (repetition_penalty != 1 or no_repeat_ngram_size > 0):
        raise NotImplementedError("repetition_penalty / no_repeat_ngram_size are not built for beam "
                                  "search (beam_size > 1): use beam_size=1")


def check_beam_args(beam_size, length_penalty=1.0, patience=1):
    """faster-whisper's beam options as this build runs them: beam_size 1 .. 8, patience 1,
    length_penalty > 0. NotImplementedError for a value faster-whisper accepts and this build
    does not run, ValueError for one that is no beam search at all."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, (int, np.integer)) or beam_size < 1:
        raise ValueError(f"beam_size must be an integer >= 1, not {beam_size!r}")
    if beam_size > BEAM_MAX:
        raise NotImplementedError(f"beam_size {beam_size}: this build runs beam_size 1 .. {BEAM_MAX}")
    if patience is not None and float(patience) != 1.0:
        raise NotImplementedError(f"patience {patience!r}: this build runs patience 1 only")
    if not float(length_penalty) > 0:
        raise ValueError(f"length_penalty must be > 0, not {length_penalty!r}")


# compute types of the encoder's linear layers (janus.h JANUS_ENC_COMPUTE_*)
ENCODER_COMPUTE = {"float16": 0, "int8": 1}


def encoder_compute_mode(name) -> int:
    """"float16" / "int8" -> JANUS_ENC_COMPUTE_*; ValueError for anything else."""
    if not isinstance(name, str) or name not in ENCODER_COMPUTE:
        raise ValueError(f"encoder_compute must be one of {sorted(ENCODER_COMPUTE)}, not {name!r}")
    return ENCODER_COMPUTE[name]


# compute types of the decoder's cross-attention operand (janus.h JANUS_CROSS_COMPUTE_*)
CROSS_COMPUTE = {"float16": 0, "int8": 1}
CROSS_COMPUTE_NAMES = ("float16", "int8")


def cross_compute_mode(name) -> int:
    """"float16" / "int8" -> JANUS_CROSS_COMPUTE_*; ValueError for anything else."""
    if not isinstance(name, str) or name not in CROSS_COMPUTE:
        raise ValueError(f"cross_compute must be one of {sorted(CROSS_COMPUTE)}, not {name!r}")
    return CROSS_COMPUTE[name]


# compute types of the decoder's weights (janus.h JANUS_DEC_COMPUTE_*)
DECODER_COMPUTE = {"float16": 0, "int8": 1}
DECODER_COMPUTE_NAMES = ("float16", "int8")


def decoder_compute_mode(name) -> int:
    """"float16" / "int8" -> JANUS_DEC_COMPUTE_*; ValueError for anything else."""
    if not isinstance(name, str) or name not in DECODER_COMPUTE:
        raise ValueError(f"decoder_compute must be one of {sorted(DECODER_COMPUTE)}, not {name!r}")
    return DECODER_COMPUTE[name]


def check_decoder_compute_beam(decoder_compute: str, beam_size: int) -> None:
    """Beam search has no int8-weight form (the vocabulary projection's beam partials read the
    fp16 table): NotImplementedError for beam_size > 1 with decoder_compute "int8"."""
    if decoder_compute_mode(decoder_compute) != DECODER_COMPUTE["float16"] and beam_size > 1:
        raise NotImplementedError(f"beam_size {beam_size} with decoder_compute='int8': beam search multiplies the "
                                  "float16 decoder weights only; use beam_size=1 or decoder_compute='float16'")


ALIGN_MAX_HEADS = 64   # alignment heads of one engine (csrc/align_plan.h kAlignMaxHeads)


def default_alignment_heads(cfg):
    """Every head of the last half of the decoder layers (CTranslate2's default for a
    checkpoint that names no alignment heads)."""
    return [(l, h) for l in range(cfg.dec_layers // 2, cfg.dec_layers) for h in range(cfg.n_heads)]


def check_alignment_heads(cfg, heads):
    """[(layer, head)] validated against the model: non-empty, at most ALIGN_MAX_HEADS,
    indices in range, no pair twice. ValueError otherwise."""
    try:
        out = [(int(l), int(h)) for (l, h) in heads]
    except (TypeError, ValueError):
        raise ValueError(f"alignment_heads must be (layer, head) pairs, not {heads!r}") from None
    if not out:
        raise ValueError("alignment_heads must not be empty")
    if len(out) > ALIGN_MAX_HEADS:
        raise ValueError(f"alignment_heads: {len(out)} heads, the limit is {ALIGN_MAX_HEADS}")
    for l, h in out:
        if not (0 <= l < cfg.dec_layers and 0 <= h < cfg.n_heads):
            raise ValueError(f"alignment head ({l}, {h}) out of range for {cfg.name} "
                             f"({cfg.dec_layers} decoder layers, {cfg.n_heads} heads)")
    if len(set(out)) != len(out):
        raise ValueError("alignment_heads: a pair is listed twice")
    return out


@dataclasses.dataclass
class Alignment:
    """One window's alignment (janus_whisper_align): the DTW path over (row of text + [eot],
    encoder frame) and the forced-token probabilities of the text tokens."""
    text_indices: np.ndarray   # int32 [L]
    time_indices: np.ndarray   # int32 [L]
    token_probs: np.ndarray    # float32 [len(text)]
    attention: np.ndarray = None   # float32 [len(text) + 1][size // 2] (return_attention)


class WhisperEngine:
    """One janus_whisper context on the current GPU (thread-safe per call in C++).

    encoder_compute: "float16" (default: fp16 weights and activations on the fp16 MFMA) or
    "int8" (the encoder's QKV / out_proj / fc1 / fc2 on the i8 MFMA with row-wise symmetric
    quantisation, CTranslate2's int8 compute type). It leaves the decoder alone.

    cross_compute: "float16" (default: the decoder's cross-attention streams the encoder
    output it is handed) or "int8" (every decode call quantises its encoder rows per key to
    int8 first, CTranslate2's rule for the input of the cross-attention K / V projections, and
    the cross-attention streams those: half the bytes; include/janus.h
    janus_whisper_set_cross_compute). align() and detect_language() read the
    fp16 rows in both.

    decoder_compute: "float16" (default) or "int8": every decoder linear layer and the
    vocabulary projection multiply int8 weights (per-row scales, fp16 activations, W8A16;
    include/janus.h janus_whisper_set_decoder_compute) on the unfused launch
    path. Greedy and sampled calls; decode_beam() is refused. The fp16 weights stay resident."""

    def __init__(self, cfg: WhisperConfig, weights: dict = None, seed: int = 0,
                 encoder_compute: str = "float16", alignment_heads=None, cross_compute: str = "float16",
                 decoder_compute: str = "float16"):
        mode = encoder_compute_mode(encoder_compute)
        cross = cross_compute_mode(cross_compute)
        dmode = decoder_compute_mode(decoder_compute)
        check_encoder_compute(cfg, mode)
        if alignment_heads is not None:
            alignment_heads = check_alignment_heads(cfg, alignment_heads)
        self.device = nat.require_gpu()
        self.cfg = cfg
        self.tokenizer = tok.load_tokenizer(multilingual=cfg.multilingual, n_vocab=cfg.n_vocab)
        c = janus_whisper_config(cfg.n_mels, cfg.n_audio_ctx, cfg.d_model, cfg.n_heads,
                                 cfg.enc_layers, cfg.dec_layers, cfg.n_vocab, cfg.n_text_ctx)
        h = ctypes.c_void_p()
        nat.call("janus_whisper_create", ctypes.addressof(c), ctypes.addressof(h))
        self._h = h
        weights = weights if weights is not None else load_weights(cfg, seed)
        basis, filt = mel_constants(cfg.n_mels)
        weights = dict(weights)
        weights["mel.basis"] = basis
        weights["mel.filters"] = filt
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            nat.call("janus_whisper_set_tensor", self._h, name.encode(), a.ctypes.data, a.size)
        if mode != ENCODER_COMPUTE["float16"]:
            nat.call("janus_whisper_set_encoder_compute", self._h, mode)
        if cross != CROSS_COMPUTE["float16"]:
            nat.call("janus_whisper_set_cross_compute", self._h, cross)
        if dmode != DECODER_COMPUTE["float16"]:
            nat.call("janus_whisper_set_decoder_compute", self._h, dmode)
        self.alignment_heads = alignment_heads or default_alignment_heads(cfg)
        if alignment_heads is not None:
            pairs = np.ascontiguousarray(np.asarray(alignment_heads, np.int32).reshape(-1, 2))
            nat.call("janus_whisper_set_alignment_heads", self._h, pairs.ctypes.data, len(pairs))

    @property
    def encoder_compute(self) -> str:
        """The compute type the next encode() runs its linear layers in."""
        m = ctypes.c_int32(-1)
        nat.call("janus_whisper_encoder_compute", self._h, ctypes.addressof(m))
        return {v: k for k, v in ENCODER_COMPUTE.items()}[m.value]

    def set_encoder_compute(self, mode: str) -> None:
        """Switch the encoder's linear layers between "float16" and "int8" (either direction,
        between calls); the int8 weights are quantised on the first int8 encode()."""
        check_encoder_compute(self.cfg, mode)
        nat.call("janus_whisper_set_encoder_compute", self._h, encoder_compute_mode(mode))

    @property
    def cross_compute(self) -> str:
        """The operand the next decode call's cross-attention reads: "float16" | "int8"."""
        m = ctypes.c_int32(-1)
        nat.call("janus_whisper_cross_compute", self._h, ctypes.addressof(m))
        return CROSS_COMPUTE_NAMES[m.value]

    def set_cross_compute(self, mode: str) -> None:
        """Switch the cross-attention's encoder output between "float16" and "int8" (either
        direction, between calls); "float16" again is bit-identical to never having left it."""
        m = cross_compute_mode(mode)   # ValueError: unknown name
        nat.call("janus_whisper_set_cross_compute", self._h, m)

    @property
    def decoder_compute(self) -> str:
        """The weights the next decode call multiplies: "float16" | "int8"."""
        m = ctypes.c_int32(-1)
        nat.call("janus_whisper_decoder_compute", self._h, ctypes.addressof(m))
        return DECODER_COMPUTE_NAMES[m.value]

    def set_decoder_compute(self, mode: str) -> None:
        """Switch the decoder's weights between "float16" and "int8" (either direction, between
        calls); the int8 copies are quantised on the first int8 decode call, "float16" again is
        bit-identical to never having left it."""
        m = decoder_compute_mode(mode)   # ValueError: unknown name
        nat.call("janus_whisper_set_decoder_compute", self._h, m)

    def decode_weights(self) -> str:
        """The weights the last decode call multiplied (janus_whisper_decode_weights):
        "float16" | "int8"."""
        m = ctypes.c_int32(0)
        nat.call("janus_whisper_decode_weights", self._h, ctypes.addressof(m))
        return DECODER_COMPUTE_NAMES[int(m.value)]

    def decoder_weight_i8(self, layer: int, which: int):
        """(q int8 [N][K], s float32 [N]) of one quantised decoder matrix as the int8 mode
        multiplies it (janus_whisper_decoder_weight_i8, test entry): ``which`` a
        DEC_W_* index of layer ``layer``, or layer -1: the vocabulary table."""
        d, c = self.cfg.d_model, self.cfg
        n, k = ((c.n_vocab, d) if layer < 0 else
                {0: (3 * d, d), 1: (d, d), 2: (c.n_heads * d, d), 3: (d, d), 4: (d, d), 5: (4 * d, d),
                 6: (d, 4 * d)}[int(which)])
        q = np.empty((n, k), np.int8)
        s = np.empty(n, np.float32)
        nat.call("janus_whisper_decoder_weight_i8", self._h, int(layer), int(which), q.ctypes.data, s.ctypes.data)
        return q, s

    def set_tensor(self, name: str, arr) -> None:
        """Re-upload one parameter (janus_whisper_set_tensor); the next call re-prepares
        the derived fp16 weights and re-captures the decode graphs."""
        a = np.ascontiguousarray(arr, dtype=np.float32)
        nat.call("janus_whisper_set_tensor", self._h, name.encode(), a.ctypes.data, a.size)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                nat.lib().janus_whisper_destroy(h)
            except Exception:
                pass

    # ---- stages (device tensors in/out, current stream)
    def logmel(self, pcm: torch.Tensor, offsets: torch.Tensor, batch: int, decim: int,
               want_raw: bool = False):
        frames = 2 * self.cfg.n_audio_ctx
        nm = self.cfg.n_mels
        mel = torch.empty(batch, frames, nm, dtype=torch.float16, device=self.device)
        raw = torch.empty(batch, frames, nm, dtype=torch.float32, device=self.device) if want_raw else None
        nat.call("janus_whisper_logmel", self._h, pcm.data_ptr(), offsets.data_ptr(), batch, decim,
                 raw.data_ptr() if raw is not None else None, mel.data_ptr(), nat.stream_ptr())
        return (mel, raw) if want_raw else mel

    def logmel_frames(self, pcm: torch.Tensor, offsets: torch.Tensor, batch: int, decim: int,
                      frames: int) -> torch.Tensor:
        """Whole-clip features (janus_whisper_logmel_frames): fp16 [batch][frames][n_mels],
        normalised over every frame of each clip, 0.0 from each clip's content end on."""
        mel = torch.empty(batch, frames, self.cfg.n_mels, dtype=torch.float16, device=self.device)
        nat.call("janus_whisper_logmel_frames", self._h, pcm.data_ptr(), offsets.data_ptr(), batch,
                 decim, frames, mel.data_ptr(), nat.stream_ptr())
        return mel

    def encode(self, mel: torch.Tensor) -> torch.Tensor:
        B = mel.shape[0]
        assert mel.dtype == torch.float16 and mel.is_contiguous()
        enc = torch.empty(B, self.cfg.n_audio_ctx, self.cfg.d_model, dtype=torch.float16,
                          device=self.device)
        nat.call("janus_whisper_encode", self._h, mel.data_ptr(), B, enc.data_ptr(), nat.stream_ptr())
        return enc

    def decode_options(self, max_length: int = 448, check_every: int = 16,
                       timestamps: bool = True, xattn_splits: int = 0, cu_count: int = 0,
                       state_slot: int = 0, logits_blocks: int = 0, msplit_rows_n: int = 0,
                       persistent: int = 0, path_flags: int = 0, lanes: int = 0, suppress_tokens=None):
        t = self.tokenizer
        prompt = np.array(t.sot_sequence, np.int32)
        supp = np.array(t.suppress_tokens() if suppress_tokens is None else
                        resolve_suppress_tokens(t, suppress_tokens, self.cfg.n_vocab), np.int32)
        opt = janus_decode_options()
        opt.prompt = prompt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        opt.prompt_len = len(prompt)
        opt.max_length = max_length
        opt.eot = t.eot
        opt.suppress = supp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        opt.n_suppress = len(supp)
        opt.suppress_blank = 1
        opt.blank_token = t.blank
        opt.timestamp_begin = t.timestamp_begin if timestamps else -1
        opt.no_timestamps = t.no_timestamps
        opt.max_initial_timestamp_index = 50
        opt.check_every = check_every
        opt.xattn_splits = xattn_splits
        opt.cu_count = cu_count
        opt.state_slot = state_slot
        opt.logits_blocks = logits_blocks
        opt.msplit_rows_n = msplit_rows_n
        opt.persistent = persistent
        opt.path_flags = path_flags
        opt.lanes = lanes
        return opt, (prompt, supp)

    def decode(self, enc: torch.Tensor, max_length: int = 448, check_every: int = 16,
               timestamps: bool = True, xattn_splits: int = 0, cu_count: int = 0,
               path_flags: int = 0, lanes: int = 0):
        B = enc.shape[0]
        opt, keep = self.decode_options(max_length, check_every, timestamps, xattn_splits,
                                        cu_count, path_flags=path_flags, lanes=lanes)
        tokens = torch.empty(B, max_length, dtype=torch.int32, device=self.device)
        ntok = torch.empty(B, dtype=torch.int32, device=self.device)
        slp = torch.empty(B, dtype=torch.float32, device=self.device)
        nat.call("janus_whisper_decode_greedy", self._h, enc.data_ptr(), B, ctypes.addressof(opt),
                 tokens.data_ptr(), ntok.data_ptr(), slp.data_ptr(), nat.stream_ptr())
        del keep
        return tokens, ntok, slp

    def decode_ex(self, enc: torch.Tensor, prompts=None, max_length: int = 448,
                  check_every: int = 16, timestamps: bool = True, xattn_splits: int = 0,
                  cu_count: int = 0, temperature: float = 0.0, seeds=None, enc_index=None,
                  pos_offset=None, steps: int = 0, state_slot: int = 0, logits_blocks: int = 0,
                  msplit_rows_n: int = 0, persistent: int = 0, path_flags: int = 0,
                  no_speech_back: int = None, repetition_penalty: float = 1.0,
                  no_repeat_ngram_size: int = 0, suppress_tokens=None):
        """janus_whisper_decode_greedy_ex: per-row prompts (lists of token ids; None = the
        SOT sequence for every row) and the no-speech probability. Returns a DecodeOut.
        temperature > 0 samples instead (janus_whisper_decode_sample_ex: Gumbel-max over the
        rule-filtered logits / T with per-row uint32 ``seeds``); a sequence of temperatures
        (one per row, each >= 0; 0 = a greedy row) samples row b at temperature[b] in the
        same call (janus_whisper_decode_sample_rows_ex). ``enc_index`` (one int per
        decoder row): row b attends to enc[enc_index[b]] — the best_of hypotheses of a
        window share its encoder output, read once per pair of rows. ``pos_offset`` /
        ``steps`` (greedy): a staggered call — row b runs ``steps`` positions from
        pos_offset[b]; rows with an offset > 0 continue this context's previous call in the
        same row (pass the same batch size and their encoder output again), rows with 0
        start fresh (one contiguous range). ``state_slot``: the context's decoder state slot
        the call runs in (a sampled re-decode between two staggered calls takes another
        slot); ``logits_blocks`` / ``msplit_rows_n``: launch geometry (0 = measured
        defaults, janus_decode_options); ``persistent``: the persistent decoder segments
        (dec_persist.hip) where the shape allows; ``path_flags``: an alternative decoder path
        (DEC_PATH_*, parity tests). ``no_speech_back``: no_speech_prob is read that many
        positions before each prompt's last one (janus_decode_rows.no_speech_back), where the
        prompt must hold <|startoftranscript|>; None = len(tokenizer.sot_sequence) - 1 (0 on
        ``*.en``, 2 on a multilingual model). ``repetition_penalty`` (> 0, 1 = off) /
        ``no_repeat_ngram_size`` (>= 0, 0 = off): the history rules over each row's sampled
        tokens (include/janus.h janus_decode_options), greedy and sampled calls,
        not staggered ones. ``suppress_tokens``: faster-whisper's list (None or [-1] = the
        tokenizer's set; with -1: that set plus the ids; without: the ids plus the five
        always-suppressed specials)."""
        B = enc.shape[0] if enc_index is None else len(enc_index)
        check_history_args(repetition_penalty, no_repeat_ngram_size)
        if steps < 0:
            raise ValueError("steps must be >= 0")
        if steps and pos_offset is None:
            raise ValueError("steps applies to a staggered call (pos_offset) only")
        row_t = None
        if not np.isscalar(temperature):
            row_t = np.ascontiguousarray(np.asarray(temperature, np.float32))
            if row_t.shape != (B,) or not (row_t >= 0).all():
                raise ValueError("per-row temperatures: one value >= 0 per row")
            temperature = 1.0
        if temperature > 0:
            if seeds is None or len(seeds) != B:
                raise ValueError("sampling needs one uint32 seed per row")
            sd = np.ascontiguousarray(np.asarray(seeds, np.uint64) & 0xFFFFFFFF, dtype=np.uint32)
        opt, keep = self.decode_options(max_length, check_every, timestamps, xattn_splits, cu_count,
                                        state_slot, logits_blocks, msplit_rows_n, persistent,
                                        path_flags, suppress_tokens=suppress_tokens)
        rows = janus_decode_rows()
        rows.no_speech_token = self.tokenizer.no_speech
        opt.repetition_penalty = float(repetition_penalty)
        opt.no_repeat_ngram_size = int(no_repeat_ngram_size)
        po = None
        if pos_offset is not None:
            po = np.ascontiguousarray(np.asarray(pos_offset, np.int32))
            if po.shape != (B,):
                raise ValueError("pos_offset needs one offset per row")
            rows.pos_offset = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.steps = int(steps)
        ei = None
        if enc_index is not None:
            ei = np.ascontiguousarray(np.asarray(enc_index, np.int32))
            if ei.size and (ei.min() < 0 or ei.max() >= enc.shape[0]):
                raise ValueError("enc_index out of range")
            rows.enc_index = ei.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.n_enc = int(enc.shape[0])
        plens = np.full(B, len(self.tokenizer.sot_sequence), np.int32)
        pr = None
        if prompts is not None:
            assert len(prompts) == B
            plens = np.array([len(p) for p in prompts], np.int32)
            stride = int(max(plens.max(), 1))
            pr = np.zeros((B, stride), np.int32)
            for b, p in enumerate(prompts):
                pr[b, :len(p)] = p
            rows.prompts = pr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.prompt_lens = plens.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.stride = stride
        rows.no_speech_back = self._no_speech_back(no_speech_back, prompts)
        tokens = torch.empty(B, max_length, dtype=torch.int32, device=self.device)
        ntok = torch.empty(B, dtype=torch.int32, device=self.device)
        slp = torch.empty(B, dtype=torch.float32, device=self.device)
        nsp = torch.empty(B, dtype=torch.float32, device=self.device)
        if row_t is not None:
            nat.call("janus_whisper_decode_sample_rows_ex", self._h, enc.data_ptr(), B,
                     ctypes.addressof(opt), ctypes.addressof(rows), row_t.ctypes.data,
                     sd.ctypes.data, tokens.data_ptr(), ntok.data_ptr(), slp.data_ptr(),
                     nsp.data_ptr(), nat.stream_ptr())
        elif temperature > 0:
            nat.call("janus_whisper_decode_sample_ex", self._h, enc.data_ptr(), B,
                     ctypes.addressof(opt), ctypes.addressof(rows), ctypes.c_float(temperature),
                     sd.ctypes.data, tokens.data_ptr(), ntok.data_ptr(), slp.data_ptr(),
                     nsp.data_ptr(), nat.stream_ptr())
        else:
            nat.call("janus_whisper_decode_greedy_ex", self._h, enc.data_ptr(), B, ctypes.addressof(opt),
                     ctypes.addressof(rows), tokens.data_ptr(), ntok.data_ptr(), slp.data_ptr(),
                     nsp.data_ptr(), nat.stream_ptr())
        del keep, pr, ei, po, row_t
        return DecodeOut(tokens, ntok, slp, nsp, plens, self.tokenizer.eot)

    def decode_beam(self, enc: torch.Tensor, prompts=None, beam_size: int = 5,
                    length_penalty: float = 1.0, max_length: int = 448, check_every: int = 16,
                    timestamps: bool = True, xattn_splits: int = 0, cu_count: int = 0,
                    temperature: float = 0.0, pos_offset=None, state_slot: int = 0,
                    logits_blocks: int = 0, msplit_rows_n: int = 0, persistent: int = 0,
                    path_flags: int = 0, no_speech_back: int = None):
        """janus_whisper_decode_beam_ex: beam search at temperature 0 over ``enc``
        [windows][1500][d] (``prompts``: one token list per window; None = the SOT sequence).
        Returns a DecodeOut with one row per window: the winning hypothesis' tokens,
        ``n_tokens``, ``sum_logprob`` (its cumulative score S) and the window's
        no_speech_prob. The rule (include/janus.h): per window up to
        ``beam_size`` (1 .. 8) live beams, the best 2k candidates S + log-prob per step walked
        in order (an <|endoftext|> candidate finishes a hypothesis, the others become the next
        beams), the window stops at beam_size finished hypotheses or at ``max_length``, the
        best S / n^length_penalty wins; patience 1. beam_size 1 is the greedy decode.
        windows x beam_size <= 512; staggered rows (``pos_offset``) and ``temperature`` > 0
        are rejected, a ``persistent`` request runs the launch path (decode_path())."""
        check_beam_args(beam_size, length_penalty)
        if getattr(self, "_h", None) is not None and self.decoder_compute != "float16":
            raise NotImplementedError("decode_beam with decoder_compute='int8': beam search multiplies the float16 "
                                      "decoder weights only")
        check_family_features(getattr(self, "cfg", None), beam_size)   # (beam_size 1 there: the C entry refuses)
        if pos_offset is not None:
            raise ValueError("decode_beam: staggered rows (pos_offset) are not supported")
        if not np.isscalar(temperature) or temperature > 0:
            raise ValueError("decode_beam: beam search runs at temperature 0 (the fallback "
                             "temperatures are sampled best_of decodes)")
        W = int(enc.shape[0])
        if W * beam_size > BEAM_MAX_ROWS:
            raise ValueError(f"decode_beam: windows x beam_size = {W * beam_size} rows, the limit "
                             f"is {BEAM_MAX_ROWS}")
        opt, keep = self.decode_options(max_length, check_every, timestamps, xattn_splits, cu_count,
                                        state_slot, logits_blocks, msplit_rows_n, persistent,
                                        path_flags)
        rows = janus_decode_rows()
        rows.no_speech_token = self.tokenizer.no_speech
        plens = np.full(W, len(self.tokenizer.sot_sequence), np.int32)
        pr = None
        if prompts is not None:
            if len(prompts) != W:
                raise ValueError("decode_beam: one prompt per window")
            plens = np.array([len(p) for p in prompts], np.int32)
            stride = int(max(plens.max(), 1))
            pr = np.zeros((W, stride), np.int32)
            for b, p in enumerate(prompts):
                pr[b, :len(p)] = p
            rows.prompts = pr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.prompt_lens = plens.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.stride = stride
        rows.no_speech_back = self._no_speech_back(no_speech_back, prompts)
        tokens = torch.empty(W, max_length, dtype=torch.int32, device=self.device)
        ntok = torch.empty(W, dtype=torch.int32, device=self.device)
        slp = torch.empty(W, dtype=torch.float32, device=self.device)
        nsp = torch.empty(W, dtype=torch.float32, device=self.device)
        nat.call("janus_whisper_decode_beam_ex", self._h, enc.data_ptr(), W, ctypes.addressof(opt),
                 ctypes.addressof(rows), int(beam_size), ctypes.c_float(length_penalty),
                 tokens.data_ptr(), ntok.data_ptr(), slp.data_ptr(), nsp.data_ptr(), nat.stream_ptr())
        del keep, pr
        return DecodeOut(tokens, ntok, slp, nsp, plens, self.tokenizer.eot)

    def _no_speech_back(self, no_speech_back, prompts) -> int:
        """janus_decode_rows.no_speech_back of a call: the given value, or where the
        tokenizer's start sequence puts <|startoftranscript|>; every prompt must hold it
        there (ValueError otherwise)."""
        t = self.tokenizer
        back = len(t.sot_sequence) - 1 if no_speech_back is None else int(no_speech_back)
        if back < 0:
            raise ValueError(f"no_speech_back must be >= 0, not {back}")
        for b, p in enumerate(prompts if prompts is not None else [t.sot_sequence]):
            if len(p) <= back or int(p[len(p) - 1 - back]) != t.sot:
                raise ValueError(f"prompt {b}: <|startoftranscript|> ({t.sot}) expected {back} "
                                 f"tokens before its end (no_speech_back)")
        return back

    def decode_hidden(self, enc: torch.Tensor, tokens, enc_index=None, pos_offset=None,
                      steps: int = 0, want_cache: bool = True, xattn_splits: int = 0,
                      cu_count: int = 0, state_slot: int = 0, msplit_rows_n: int = 0,
                      persistent: int = 0, path_flags: int = 0):
        """janus_whisper_decode_hidden (test entry): the decoder's residual rows of the forced
        ``tokens`` int [B][n], through the decode call's own plan and launches (no final
        LayerNorm, no selection). ``enc_index`` / ``pos_offset`` / ``steps`` / the options as
        decode_ex. Returns a HiddenOut: ``x`` f32 [positions][B][d] (row b of step i is
        position pos_offset[b] + i), the self-attention caches ``kc`` / ``vc`` fp16
        [layers][B][n_text_ctx][d] (``want_cache``) and ``plan``, the plan that ran as a dict
        of its name=value lines (ints; pairs / groups as lists)."""
        tk = np.ascontiguousarray(np.asarray(tokens, np.int32))
        if tk.ndim != 2 or tk.shape[1] < 1:
            raise ValueError("tokens must be [B][n], n >= 1")
        B, n = tk.shape
        if B != (enc.shape[0] if enc_index is None else len(enc_index)):
            raise ValueError("one token row per decoder row")
        if steps and pos_offset is None:
            raise ValueError("steps applies to a staggered call (pos_offset) only")
        assert enc.dtype == torch.float16 and enc.is_contiguous()
        c = self.cfg
        opt = janus_decode_options()
        opt.max_length = n + 1
        opt.eot = opt.blank_token = opt.timestamp_begin = opt.no_timestamps = -1
        opt.max_initial_timestamp_index = -1
        opt.xattn_splits, opt.cu_count, opt.state_slot = xattn_splits, cu_count, state_slot
        opt.msplit_rows_n, opt.persistent, opt.path_flags = msplit_rows_n, persistent, path_flags
        rows = janus_decode_rows()
        rows.no_speech_token = -1
        plens = np.full(B, n, np.int32)
        rows.prompts = tk.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        rows.prompt_lens = plens.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        rows.stride = n
        po = ei = None
        if pos_offset is not None:
            po = np.ascontiguousarray(np.asarray(pos_offset, np.int32))
            if po.shape != (B,):
                raise ValueError("pos_offset needs one offset per row")
            rows.pos_offset = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.steps = int(steps)
        if enc_index is not None:
            ei = np.ascontiguousarray(np.asarray(enc_index, np.int32))
            if ei.min() < 0 or ei.max() >= enc.shape[0]:
                raise ValueError("enc_index out of range")
            rows.enc_index = ei.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            rows.n_enc = int(enc.shape[0])
        T = int(steps) if (pos_offset is not None and steps > 0) else n
        x = torch.empty(T, B, c.d_model, dtype=torch.float32, device=self.device)
        kc = vc = None
        if want_cache:
            kc = torch.empty(c.dec_layers, B, c.n_text_ctx, c.d_model, dtype=torch.float16, device=self.device)
            vc = torch.empty_like(kc)
        text = ctypes.create_string_buffer(1 << 16)
        nat.call("janus_whisper_decode_hidden", self._h, enc.data_ptr(), B, ctypes.addressof(opt),
                 ctypes.addressof(rows), x.data_ptr(), T, kc.data_ptr() if want_cache else None,
                 vc.data_ptr() if want_cache else None, text, len(text), nat.stream_ptr())
        del po, ei, plens
        plan = {}
        for line in text.value.decode().splitlines():
            k, v = line.split("=", 1)
            plan[k] = [int(t) for t in v.split(",") if t] if k in ("pairs", "groups") else int(float(v))
        return HiddenOut(x, kc, vc, plan)

    def detect_language(self, enc: torch.Tensor):
        """janus_whisper_detect_language over ``enc`` [B][1500][d]: (probs f32 [B][n_languages]
        — the softmax over the language tokens alone of one <|startoftranscript|> position —,
        best int32 [B], indices into the tokenizer's ``languages``: 99, or 100 on the large-v3
        family), device tensors (include/janus.h,
        DESIGN.md §5m). ValueError on an English-only engine."""
        t = self.tokenizer
        if not self.cfg.multilingual:
            raise ValueError(f"detect_language: {self.cfg.name} is English-only")
        assert enc.dtype == torch.float16 and enc.is_contiguous()
        B = int(enc.shape[0])
        probs = torch.empty(B, t.n_languages, dtype=torch.float32, device=self.device)
        best = torch.empty(B, dtype=torch.int32, device=self.device)
        nat.call("janus_whisper_detect_language", self._h, enc.data_ptr(), B, int(t.sot),
                 int(t.language_begin), int(t.n_languages), probs.data_ptr(), best.data_ptr(),
                 nat.stream_ptr())
        return probs, best

    def align(self, enc: torch.Tensor, texts, sizes, enc_index=None, return_attention: bool = False,
              phases: int = 0, sot_sequences=None):
        """janus_whisper_align: word alignment of several windows in one call. ``texts``: one
        list of text token ids (< eot, the window's segments concatenated) per window;
        ``sizes``: each window's content size in mel frames (2 .. 3000); ``enc_index``: window
        j attends to enc[enc_index[j]] (default enc[j]). Returns one Alignment per window (None
        for a window without text, which runs nothing): the DTW path over the rows of
        text + [eot] and the frames < size // 2, and the text tokens' forced probabilities
        (include/janus.h rules 1 - 5). ``return_attention`` also returns the
        matrix A the path was solved on; ``phases``: janus_whisper_align's measurement mask;
        ``sot_sequences``: one start sequence per window instead of the tokenizer's (a
        multilingual model's per-utterance language and task)."""
        check_family_features(getattr(self, "cfg", None), word_timestamps=True,
                              alignment_heads=getattr(self, "alignment_heads", None))
        t = self.tokenizer
        if len(texts) != len(sizes) or (enc_index is not None and len(enc_index) != len(texts)):
            raise ValueError("align: one text, one size (and one enc_index) per window")
        sot = list(t.sot_sequence)
        # multilingual models: every window's own [sot, <|language|>, <|task|>] (one length)
        sots = [sot] * len(texts) if sot_sequences is None else [list(q) for q in sot_sequences]
        if len(sots) != len(texts) or any(len(q) != len(sot) for q in sots):
            raise ValueError("align: one start sequence of the tokenizer's length per window")
        live = [j for j, x in enumerate(texts) if len(x) > 0]
        out = [None] * len(texts)
        if not live:
            return out
        seqs = [sots[j] + [t.no_timestamps] + [int(v) for v in texts[j]] + [t.eot] for j in live]
        lens = np.array([len(q) for q in seqs], np.int32)
        if lens.max() > self.cfg.n_text_ctx:
            raise ValueError(f"align: a sequence of {int(lens.max())} tokens exceeds n_text_ctx "
                             f"{self.cfg.n_text_ctx}")
        szs = np.array([int(sizes[j]) for j in live], np.int32)
        if szs.min() < 2 or szs.max() > 2 * self.cfg.n_audio_ctx:
            raise ValueError("align: sizes must lie in [2, 3000] mel frames")
        stride = int(lens.max())
        toks = np.zeros((len(live), stride), np.int32)
        for k, q in enumerate(seqs):
            toks[k, :len(q)] = q
        ei = np.array([int(enc_index[j]) if enc_index is not None else j for j in live], np.int32)
        if ei.min() < 0 or ei.max() >= enc.shape[0]:
            raise ValueError("align: enc_index out of range")
        assert enc.dtype == torch.float16 and enc.is_contiguous()
        N = lens - len(sot) - 2 + 1
        F = szs // 2
        ps = int((N + F).max())
        ti = torch.empty(len(live), ps, dtype=torch.int32, device=self.device)
        fi = torch.empty(len(live), ps, dtype=torch.int32, device=self.device)
        pl = torch.empty(len(live), dtype=torch.int32, device=self.device)
        pr = torch.empty(len(live), stride, dtype=torch.float32, device=self.device)
        aoff = np.concatenate([[0], np.cumsum(N.astype(np.int64) * F)])
        att = torch.empty(int(aoff[-1]), dtype=torch.float32, device=self.device) if return_attention else None
        nat.call("janus_whisper_align", self._h, enc.data_ptr(), int(enc.shape[0]), len(live),
                 toks.ctypes.data, lens.ctypes.data, stride, szs.ctypes.data, ei.ctypes.data, len(sot),
                 int(t.eot), ti.data_ptr(), fi.data_ptr(), pl.data_ptr(), ps, pr.data_ptr(),
                 att.data_ptr() if att is not None else None, int(phases), nat.stream_ptr())
        ti, fi, pl, pr = ti.cpu().numpy(), fi.cpu().numpy(), pl.cpu().numpy(), pr.cpu().numpy()
        att = att.cpu().numpy() if att is not None else None
        for k, j in enumerate(live):
            L = int(pl[k])
            out[j] = Alignment(ti[k, :L].copy(), fi[k, :L].copy(), pr[k, :int(N[k]) - 1].copy(),
                               att[aoff[k]:aoff[k + 1]].reshape(int(N[k]), int(F[k])).copy()
                               if att is not None else None)
        return out

    def decode_stand(self, batch: int, state_slot: int = 0):
        """Where each of the last decode call's ``batch`` row slots stands in decoder state
        slot ``state_slot`` (the largest pos_offset a staggered call may continue it from;
        janus_whisper_decode_stand_slot)."""
        out = np.zeros(batch, np.int32)
        nat.call("janus_whisper_decode_stand_slot", self._h, int(state_slot), out.ctypes.data,
                 int(batch))
        return [int(v) for v in out]

    def decode_check(self, state_slot: int = 0):
        """janus_whisper_decode_check: raise if the last non-polling call (check_every 0) of
        decoder state slot ``state_slot`` hit a persistent-segment barrier timeout (waits for
        that call's flag; nothing pending: returns at once). Call before using its outputs."""
        nat.call("janus_whisper_decode_check", self._h, int(state_slot))

    def decode_info(self):
        """(positions stepped, kernel launches issued) by the last decode call
        (janus_whisper_decode_info: captured graph nodes; measurement only)."""
        pos, lau = ctypes.c_int32(0), ctypes.c_int64(0)
        nat.call("janus_whisper_decode_info", self._h, ctypes.addressof(pos), ctypes.addressof(lau))
        return int(pos.value), int(lau.value)

    def decode_path(self):
        """Which path the last decode call took (janus_whisper_decode_path): a DecodePath
        of ``enc_rows`` ("own": no enc_index; "in_place": shared encoder rows read where
        they lie; "gathered": one encoder copy per decoder row) and ``persistent`` (the
        persistent level actually run; 0 = the launch path) and ``cross`` (the encoder output
        its cross-attention read: "float16" | "int8", janus_whisper_decode_cross)."""
        er, ps, cr = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        nat.call("janus_whisper_decode_path", self._h, ctypes.addressof(er), ctypes.addressof(ps))
        nat.call("janus_whisper_decode_cross", self._h, ctypes.addressof(cr))
        return DecodePath(ENC_ROWS_NAMES[int(er.value)], int(ps.value), CROSS_COMPUTE_NAMES[int(cr.value)])

    def texts(self, tokens: torch.Tensor, prompt_lens=None):
        """Host-side detokenisation of decoded rows (after each row's prompt)."""
        t = tokens.cpu().numpy()
        plen = len(self.tokenizer.sot_sequence)
        pl = prompt_lens if prompt_lens is not None else [plen] * len(t)
        return [self.tokenizer.transcript(row[int(p):]) for row, p in zip(t, pl)]


# janus_whisper_decoder_weight_i8 `which` (include/janus.h JANUS_DEC_W_*)
DEC_W_QKV, DEC_W_O, DEC_W_XQK, DEC_W_XV, DEC_W_XO, DEC_W_FC1, DEC_W_FC2 = range(7)

# janus_whisper_decode_path enc_rows (include/janus.h JANUS_ENC_ROWS_*)
ENC_ROWS_NAMES = ("own", "in_place", "gathered")


@dataclasses.dataclass(frozen=True)
class DecodePath:
    enc_rows: str      # "own" | "in_place" | "gathered"
    persistent: int    # persistent level the call ran (0: the launch path)
    cross: str = "float16"   # "float16" | "int8": the encoder output the cross-attention read


def shared_rows_in_place(cfg) -> bool:
    """True when decoder rows sharing an encoder row (enc_index) read it in place by default
    on this model: PAIR blocks up to 8 heads / d_model 512 (decode_plan.cpp pair_ok). Otherwise a
    call gathers one encoder copy per row — the 768-wide 12-head family too, whose in-place
    blocks (DEC_PATH_XROWS) measured slower than the copies — and callers keep their
    sampled batches small (services/transcriber.py FALLBACK_ROWS_GATHER)."""
    if cfg is None:
        return True
    return cfg.n_heads <= 8 and cfg.d_model <= 512   # (16 heads / 1024, 20 heads / 1280: gathered too)


@dataclasses.dataclass
class HiddenOut:
    """Device tensors of one decode_hidden call plus the plan that ran."""
    x: torch.Tensor     # f32 [positions][B][d]: the residual rows before the final LayerNorm
    kc: torch.Tensor    # fp16 [layers][B][n_text_ctx][d] self-attention keys (None: not asked)
    vc: torch.Tensor    # ... values
    plan: dict          # DecodePlan::describe() as name -> int (pairs / groups: lists)


@dataclasses.dataclass
class DecodeOut:
    """Device tensors of one batched decode plus the host prompt lengths."""
    tokens: torch.Tensor          # int32 [B][max_length]: prompt, sampled tokens, -1
    n_tokens: torch.Tensor        # int32 [B]: sampled tokens incl. <|endoftext|>
    sum_logprob: torch.Tensor     # f32 [B]: sum of the chosen tokens' (filtered) log-probs
    no_speech_prob: torch.Tensor  # f32 [B]: raw P(<|nocaptions|>) at the first sampled step
    prompt_lens: np.ndarray       # int32 [B]
    eot: int = tok.EOT            # the decoding tokenizer's <|endoftext|>

    def rows(self):
        """Per row: (sampled tokens without <|endoftext|>, avg_logprob, no_speech_prob),
        avg_logprob as faster-whisper derives it (sum / (len + 1), the +1 for eot)."""
        t, n = self.tokens.cpu().numpy(), self.n_tokens.cpu().numpy()
        lp, ns = self.sum_logprob.cpu().numpy(), self.no_speech_prob.cpu().numpy()
        out = []
        for b in range(len(n)):
            s = t[b][int(self.prompt_lens[b]):int(self.prompt_lens[b]) + int(n[b])]
            s = [int(x) for x in s if x != self.eot]
            out.append((s, float(lp[b]) / (len(s) + 1), float(ns[b])))
        return out
