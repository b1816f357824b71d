"""Reference for the int8 decoder weights (include/janus.h janus_whisper_set_decoder_compute).

numpy / torch float64, independent of janus_amd's code (``describe`` alone calls the planner):

* ``quantise``: the rule in numpy float32, per output row: amax = max |w|,
  q = clamp(rint(w * (127 / amax)), -127, 127), s = amax / 127; a zero row gives q = 0, s = 1.
* ``fp16_matrices``: the seven fp16 matrices per decoder layer the engine prepares from the fp32
  parameters (WHICH order: fused QKV, self out, absorbed cross query, cross value, cross out,
  fc1, fc2) and the vocabulary table; the absorbed query weight as tests/decoder_ref.py derives
  it, in float64, rounded once to fp16 (``wqk_f64`` keeps the float64 value).
* ``quantised`` / ``dequantised``: (q, s) of every matrix, and q * s in float64: the numbers the
  int8 mode multiplies (no rounding: q is exact in fp16 and s is applied in fp32).
* ``hidden``: tests/decoder_ref.py's teacher-forced decoder taking the dequantised matrices,
  the absorbed query weight given directly (the cross-attention in its absorbed form in the
  plain reference too: a quantised Wqk has no q / k factors). ``emulate=True`` rounds where the
  engine stores fp16 / fp32, as decoder_ref does.
* ``logits``: the final LayerNorm and the projection on the table's q * s.
* ``DEFECTS`` / ``with_defect``: seeded wrong weight sets, each a plausible kernel or prepare
  bug; tests/test_decoder_int8_host.py holds every one of them far over the bound.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
F64 = torch.float64
QKV, O, XQK, XV, XO, FC1, FC2 = range(7)
WHICH = ("wqkv", "wo", "wqk", "wv_c", "wo_c", "w1", "w2")
ROW_CHUNK = 32

DEFECTS = {
    "unquantised_layer": "one layer multiplies its fp16 weights, not q * s",
    "tile_scales_dropped": "the scales of one 16-column tile of one layer's fc2 dropped (taken as 1)",
    "scales_shifted": "one layer's fc1 scales shifted by one column",
    "w2_first_3072": "fc2 quantised over its first 3072 input columns only (amax and q; the rest 0)",
}


def quantise(w):
    """w [N][K] (any float type) -> (q int8 [N][K], s float32 [N]), per row, float32 arithmetic."""
    w = np.asarray(w).astype(F32)
    amax = np.abs(w).max(axis=-1)
    zero = amax == 0
    safe = np.where(zero, F32(1), amax).astype(F32)
    inv = (F32(127) / safe).astype(F32)
    q = np.clip(np.rint((w * inv[..., None]).astype(F32)), -127, 127).astype(np.int8)
    s = np.where(zero, F32(1), (safe / F32(127)).astype(F32)).astype(F32)
    return q, s


def wqk_f64(W, cfg, layer):
    """The absorbed cross-attention query weight [H d][d] in float64 (decoder_ref's derivation):
    row h d + j, column i = sum_c Wq[h c][i] Wk[h c][j] log2(e) / 8."""
    d, H = cfg.d_model, cfg.n_heads
    hd = d // H
    c = f"decoder.layers.{layer}.encoder_attn"
    sc = math.log2(math.e) / math.sqrt(hd)
    wq = torch.from_numpy(np.asarray(W[c + ".q_proj.weight"])).to(F64).view(H, hd, d)
    wk = torch.from_numpy(np.asarray(W[c + ".k_proj.weight"])).to(F64).view(H, hd, d)
    return (torch.einsum("hci,hcj->hji", wq, wk) * sc).reshape(H * d, d).numpy()


def fp16_matrices(W, cfg):
    """([layer][which] fp16 [N][K], table fp16 [V][d]): the engine's prepared fp16 weights."""
    out = []
    for i in range(cfg.dec_layers):
        p = f"decoder.layers.{i}."
        g = lambda n: np.asarray(W[p + n + ".weight"], F32)
        out.append([
            np.concatenate([g("self_attn.q_proj"), g("self_attn.k_proj"), g("self_attn.v_proj")]).astype(np.float16),
            g("self_attn.out_proj").astype(np.float16),
            wqk_f64(W, cfg, i).astype(np.float16),
            g("encoder_attn.v_proj").astype(np.float16),
            g("encoder_attn.out_proj").astype(np.float16),
            g("fc1").astype(np.float16),
            g("fc2").astype(np.float16),
        ])
    return out, np.asarray(W["decoder.embed_tokens.weight"], F32).astype(np.float16)


def quantised(W, cfg):
    """([layer][which] (q, s), (q, s) of the table) by the rule, from fp16_matrices."""
    mats, table = fp16_matrices(W, cfg)
    return [[quantise(m) for m in layer] for layer in mats], quantise(table)


def dequantised(Q):
    """[layer][which] (q, s) -> [layer][which] float64 q * s."""
    return [[q.astype(np.float64) * s.astype(np.float64)[:, None] for (q, s) in layer] for layer in Q]


def with_defect(Q, W16, defect, layer=1, col0=208):
    """The dequantised matrices of Q with one DEFECTS entry applied at ``layer`` (W16: the fp16
    matrices, fp16_matrices()[0])."""
    assert defect in DEFECTS
    M = dequantised(Q)
    if defect == "unquantised_layer":
        M[layer] = [m.astype(np.float64) for m in W16[layer]]
    elif defect == "tile_scales_dropped":
        q, s = Q[layer][FC2]
        s = s.astype(np.float64).copy()
        s[col0:col0 + 16] = 1.0
        M[layer][FC2] = q.astype(np.float64) * s[:, None]
    elif defect == "scales_shifted":
        q, s = Q[layer][FC1]
        M[layer][FC1] = q.astype(np.float64) * np.roll(s.astype(np.float64), 1)[:, None]
    elif defect == "w2_first_3072":
        w = W16[layer][FC2]
        assert w.shape[1] > 3072, "fc2 must be wider than 3072 input columns for this defect"
        q, s = quantise(w[:, :3072])
        full = np.zeros(w.shape, np.float64)
        full[:, :3072] = q.astype(np.float64) * s.astype(np.float64)[:, None]
        M[layer][FC2] = full
    return M


def wqk_check(q_got, s_got, W, cfg, layer):
    """(q_got, s_got) of a layer's absorbed query weight against the rule applied to the fp16
    wqk derived in float64. A derivation in other arithmetic (the engine's fp32) lands on the
    neighbouring fp16 value where the float64 value sits at an fp16 rounding boundary; that moves
    t = w * 127 / amax by one fp16 ulp of w times 127 / amax, and q by 1 where t lies that close
    to a half-integer. Returns dict: ``share`` of such elements, ``bad`` elements that differ
    otherwise (or by more than 1) in rows with equal scales, ``differ`` those that differ at
    all there, ``s_rows`` rows whose scale differs (their largest element is such a neighbour)
    and ``s_rel`` the largest relative scale difference."""
    w64 = wqk_f64(W, cfg, layer)
    w16 = w64.astype(np.float16)
    q_ref, s_ref = quantise(w16)
    same_s = np.asarray(s_got) == s_ref
    a = np.abs(w64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -14))) - 10)
    amax = np.abs(w16.astype(np.float64)).max(axis=1)
    inv = 127.0 / np.where(amax == 0, 1.0, amax)
    t = a * inv[:, None]
    near = np.abs(t - (np.floor(t) + 0.5)) <= ulp * inv[:, None]
    diff = np.asarray(q_got).astype(np.int64) - q_ref.astype(np.int64)
    bad = (diff != 0) & ~(near & (np.abs(diff) == 1))
    return dict(share=float(near.mean()), bad=int(bad[same_s].sum()), differ=int((diff != 0)[same_s].sum()),
                s_rows=int((~same_s).sum()),
                s_rel=float(np.max(np.abs(np.asarray(s_got, np.float64) - s_ref) / s_ref)))


def _t(W, name):
    return torch.from_numpy(np.asarray(W[name])).to(F64)


def _r16(x):
    return x.float().half().to(F64)


def _r32(x):
    return x.float().to(F64)


def _same(x):
    return x


@torch.no_grad()
def hidden(tokens, enc, M, W, cfg, enc_index=None, emulate=False):
    """tokens int [B][T], enc [n_enc][Te][d] (row b attends to enc[enc_index[b]], default enc[b]),
    M [layer][which] float64 matrices (dequantised()), W the fp32 parameters (biases, LayerNorms,
    embeddings) -> x [B][T][d] float64 numpy, the residual rows before the final LayerNorm."""
    tokens = np.asarray(tokens, np.int64)
    B = tokens.shape[0]
    idx = np.arange(B) if enc_index is None else np.asarray(enc_index, np.int64)
    Mt = [[torch.from_numpy(np.asarray(m, np.float64)) for m in layer] for layer in M]
    xs = []
    for b0 in range(0, B, ROW_CHUNK):
        sl = slice(b0, min(B, b0 + ROW_CHUNK))
        e = torch.as_tensor(np.asarray(enc)[idx[sl]].astype(np.float64))
        xs.append(_hidden_rows(tokens[sl], e, Mt, W, cfg, emulate))
    return torch.cat(xs, 0).numpy()


def _hidden_rows(tokens, enc, M, W, cfg, emulate):
    r16, r32 = (_r16, _r32) if emulate else (_same, _same)
    tok = torch.as_tensor(tokens)
    B, T = tok.shape
    d, H = cfg.d_model, cfg.n_heads
    hd = d // H
    sc = math.log2(math.e) / math.sqrt(hd)

    def ln(x, p):
        return F.layer_norm(x, (d,), _t(W, p + ".weight"), _t(W, p + ".bias"), 1e-5)

    def bias(name):
        return _t(W, name) if name in W else 0.0

    def heads(t):
        return t.view(t.shape[0], t.shape[1], H, hd).transpose(1, 2)    # [B][H][T][hd]

    x = r32(_t(W, "decoder.embed_tokens.weight")[tok] + _t(W, "decoder.embed_positions.weight")[:T])
    mask = torch.full((T, T), float("-inf"), dtype=F64).triu(1)
    for i in range(cfg.dec_layers):
        p = f"decoder.layers.{i}"
        m = M[i]
        # self-attention
        h = r16(ln(x, p + ".self_attn_layer_norm"))
        q = r16(h @ m[QKV][:d].T + bias(p + ".self_attn.q_proj.bias"))
        k = r16(h @ m[QKV][d:2 * d].T)
        v = r16(h @ m[QKV][2 * d:].T + bias(p + ".self_attn.v_proj.bias"))
        s = heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(hd) + mask
        o = r16((s.softmax(-1) @ heads(v)).transpose(1, 2).reshape(B, T, d))
        x = r32(x + o @ m[O].T + bias(p + ".self_attn.out_proj.bias"))
        # cross-attention, absorbed: scores in the log2 domain straight from enc
        h = r16(ln(x, p + ".encoder_attn_layer_norm"))
        c = p + ".encoder_attn"
        wk = _t(W, c + ".k_proj.weight").view(H, hd, d)
        bq = _t(W, c + ".q_proj.bias").view(H, hd) if (c + ".q_proj.bias") in W else torch.zeros(H, hd, dtype=F64)
        bqk = torch.einsum("hc,hcj->hj", bq, wk) * sc
        xqk = r16(torch.einsum("bti,hji->bthj", h, m[XQK].view(H, d, d)) + bqk)      # [B][T][H][d]
        s = torch.einsum("bthj,bkj->bthk", xqk, enc) * math.log(2.0)
        ctx = r16(torch.einsum("bthk,bkj->bthj", s.softmax(-1), enc))                # [B][T][H][d]
        bv = _t(W, c + ".v_proj.bias").view(H, hd) if (c + ".v_proj.bias") in W else 0.0
        o = r16(torch.einsum("bthj,hcj->bthc", ctx, m[XV].view(H, hd, d)) + bv).reshape(B, T, d)
        x = r32(x + o @ m[XO].T + bias(c + ".out_proj.bias"))
        # MLP
        h = r16(ln(x, p + ".final_layer_norm"))
        f = r16(F.gelu(h @ m[FC1].T + bias(p + ".fc1.bias")))
        x = r32(x + f @ m[FC2].T + bias(p + ".fc2.bias"))
    return x


@torch.no_grad()
def logits(x, W, cfg, table):
    """final LayerNorm(x) . (q * s)^T in float64: x [..][d], table (q, s) of the vocabulary (or
    their float64 product [V][d], made once by the caller) -> [..][V]."""
    x = torch.as_tensor(np.asarray(x, np.float64))
    h = F.layer_norm(x, (cfg.d_model,), _t(W, "decoder.layer_norm.weight"), _t(W, "decoder.layer_norm.bias"), 1e-5)
    if isinstance(table, tuple):
        table = table[0].astype(np.float64) * table[1].astype(np.float64)[:, None]
    return (h @ torch.from_numpy(table).T).numpy()


# ---------------------------------------------------------------- the planner (host tests)
I32P = ctypes.POINTER(ctypes.c_int32)


def describe(lib, cfg, B, dec=0, cross=0, flags=0, persistent=0, max_length=448, cus=256, temperature=0.0,
             beam_size=0, enc_index=None, prompts=None, entry="janus_decode_plan_describe_modes"):
    """(text, key) of one planner call with the context's decoder compute ``dec`` and cross compute
    ``cross`` (0 float16, 1 int8); ``entry``: the describe entry asked (the older ones take fewer
    modes). JanusNativeError where the planner rejects."""
    from janus_amd import _native as nat
    from janus_amd import whisper as jw
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
    if prompts is not None:
        stride = max(len(p) for p in prompts)
        flat = np.zeros((B, stride), np.int32)
        for b, p in enumerate(prompts):
            flat[b, :len(p)] = p
        rows.prompts = i32(flat)
        rows.prompt_lens = i32([len(p) for p in prompts])
        rows.stride = stride
    text = ctypes.create_string_buffer(1 << 16)
    key = (ctypes.c_int64 * 256)()
    n_key = ctypes.c_int32(0)
    head = (ctypes.addressof(c), ctypes.addressof(opt), ctypes.addressof(rows), B, cus, 1, 0,
            ctypes.c_float(temperature), None, beam_size, None, 0, 0)
    modes = {"janus_decode_plan_describe": (), "janus_decode_plan_describe_cross": (int(cross),),
             "janus_decode_plan_describe_modes": (int(cross), int(dec))}[entry]
    nat.check(getattr(lib, entry)(*head, *modes, ctypes.addressof(text), len(text), ctypes.addressof(key),
                                  len(key), ctypes.addressof(n_key)))
    del keep
    return text.value.decode(), tuple(key[:n_key.value])
