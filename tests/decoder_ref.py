"""Reference for the decoder's residual stream (janus_whisper_decode_hidden, include/janus_kernels.h).

Plain torch in float64, independent of janus_amd's code:

* ``hidden``: the teacher-forced decoder of oracle.whisper.decoder_logits (full sequence,
  causal mask) on the engine's weights, stopped before the final LayerNorm: x [B][T][d], and
  every layer's self-attention k / v projections [layers][B][T][d] — what the engine's K / V
  cache must hold.
* ``hidden(emulate=True)``: the same arithmetic rounded to fp16 where the engine stores
  fp16 — the LayerNorm outputs, q / k / v (the cache), the attention outputs, the GELU
  output, and for the absorbed cross-attention the products the engine keeps instead of
  q / k / v: the absorbed weight Wqk_h = (Wq_h^T Wk_h) log2(e) / 8, the query row
  LN2(x) Wqk_h^T + bqk_h, the context row sum_t p_t enc_t and the per-head value projection
  of it. The residual stream is rounded to fp32. Its distance from ``hidden()`` is what the
  storage formats alone cost: the GPU tests' bound is a small multiple of it.
* ``metrics``: the two distances of the GPU tests, ``worst``: where the larger one lies.
* ``DEFECTS``: seeded wrong references (``hidden(defect=...)``), each a plausible kernel bug;
  tests/test_decoder_hidden_host.py holds every one of them far over the bound.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
ROW_CHUNK = 32   # rows per pass (bounds the absorbed query rows [rows][T][H][d] in memory)

# name -> what it does to the reference (layer / row / columns: hidden()'s defect arguments)
DEFECTS = {
    "fc2_bias": "fc2's bias zeroed on 16 columns of one layer",
    "self_out_bias": "the self-attention out_proj's bias zeroed on 16 columns of one layer",
    "cross_out_bias": "the cross-attention out_proj's bias zeroed on 16 columns of one layer",
    "drop_last_key": "the last encoder key left out of every cross-attention",
    "pos_off_by_one": "one row's positional embedding one position ahead",
    "cache_late": "one row's K / V cache rows of one layer written one slot late",
}


def _t(W, name):
    return torch.from_numpy(np.asarray(W[name])).to(F64)


def _r16(x):
    return x.float().half().to(F64)


def _r32(x):
    return x.float().to(F64)


def _same(x):
    return x


@torch.no_grad()
def hidden(tokens, enc, W, cfg, enc_index=None, emulate=False, xabs=True, defect=None,
           layer=0, row=0, col0=0):
    """tokens int [B][T], enc [n_enc][Te][d] (row b attends to enc[enc_index[b]], default
    enc[b]) -> (x [B][T][d], k [layers][B][T][d], v [layers][B][T][d]), float64 numpy.
    ``emulate``: round where the engine stores fp16 / fp32 (``xabs``: the absorbed
    cross-attention's stores, else the projected q / K / V's). ``defect``: a DEFECTS name,
    applied at ``layer`` / ``row`` / columns [col0, col0 + 16)."""
    assert defect is None or defect in DEFECTS
    tokens = np.asarray(tokens, np.int64)
    B = tokens.shape[0]
    idx = np.arange(B) if enc_index is None else np.asarray(enc_index, np.int64)
    xs, ks, vs = [], [], []
    for b0 in range(0, B, ROW_CHUNK):
        sl = slice(b0, min(B, b0 + ROW_CHUNK))
        e = torch.as_tensor(np.asarray(enc)[idx[sl]].astype(np.float64))
        hit = row - b0 if b0 <= row < sl.stop else None   # the defect's row inside this chunk
        x, k, v = _hidden_rows(tokens[sl], e, W, cfg, emulate, xabs, defect, layer, hit, col0)
        xs.append(x); ks.append(k); vs.append(v)
    return (torch.cat(xs, 0).numpy(), torch.cat(ks, 1).numpy(), torch.cat(vs, 1).numpy())


def _hidden_rows(tokens, enc, W, cfg, emulate, xabs, defect, layer, row, col0):
    r16, r32 = (_r16, _r32) if emulate else (_same, _same)
    tok = torch.as_tensor(tokens)
    B, T = tok.shape
    d, H = cfg.d_model, cfg.n_heads
    hd = d // H
    cols = slice(col0, col0 + 16)

    def ln(x, p):
        return F.layer_norm(x, (d,), _t(W, p + ".weight"), _t(W, p + ".bias"), 1e-5)

    def lin(x, p, bias=True, zero_cols=False):
        b = _t(W, p + ".bias").clone() if bias and (p + ".bias") in W else None
        if zero_cols:
            b[cols] = 0.0
        return F.linear(x, _t(W, p + ".weight"), b)

    def heads(t):
        return t.view(t.shape[0], t.shape[1], H, hd).transpose(1, 2)    # [B][H][T][hd]

    pos = _t(W, "decoder.embed_positions.weight")
    P = pos[:T].expand(B, T, d).clone()
    if defect == "pos_off_by_one" and row is not None:
        P[row] = pos[1:T + 1]
    x = r32(_t(W, "decoder.embed_tokens.weight")[tok] + P)
    mask = torch.full((T, T), float("-inf"), dtype=F64).triu(1)
    if defect == "drop_last_key":
        enc = enc[:, :-1]
    kc, vc = [], []
    for i in range(cfg.dec_layers):
        p = f"decoder.layers.{i}"
        here = defect is not None and i == layer
        # self-attention
        h = r16(ln(x, p + ".self_attn_layer_norm"))
        q = r16(lin(h, p + ".self_attn.q_proj"))
        k = r16(lin(h, p + ".self_attn.k_proj", bias=False))
        v = r16(lin(h, p + ".self_attn.v_proj"))
        kc.append(k); vc.append(v)
        if defect == "cache_late" and here and row is not None:
            # slot t holds the row of position t - 1, slot 0 nothing yet (zeros)
            k, v = k.clone(), v.clone()
            k[row] = torch.cat([torch.zeros(1, d, dtype=F64), k[row, :-1]])
            v[row] = torch.cat([torch.zeros(1, d, dtype=F64), v[row, :-1]])
        s = heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(hd) + mask
        o = r16((s.softmax(-1) @ heads(v)).transpose(1, 2).reshape(B, T, d))
        x = r32(x + lin(o, p + ".self_attn.out_proj", zero_cols=here and defect == "self_out_bias"))
        # cross-attention
        h = r16(ln(x, p + ".encoder_attn_layer_norm"))
        c = p + ".encoder_attn"
        if emulate and xabs:
            # the engine's absorbed form: scores in the log2 domain straight from enc
            sc = math.log2(math.e) / math.sqrt(hd)
            wq = _t(W, c + ".q_proj.weight").view(H, hd, d)
            wk = _t(W, c + ".k_proj.weight").view(H, hd, d)
            wqk = r16(torch.einsum("hci,hcj->hji", wq, wk) * sc)             # [H][j][i]
            bqk = torch.einsum("hc,hcj->hj", _t(W, c + ".q_proj.bias").view(H, hd), wk) * sc
            xqk = r16(torch.einsum("bti,hji->bthj", h, wqk) + bqk)           # [B][T][H][d]
            s = torch.einsum("bthj,bkj->bthk", xqk, enc) * math.log(2.0)
            ctx = r16(torch.einsum("bthk,bkj->bthj", s.softmax(-1), enc))    # [B][T][H][d]
            wv = _t(W, c + ".v_proj.weight").view(H, hd, d)
            o = r16(torch.einsum("bthj,hcj->bthc", ctx, wv) + _t(W, c + ".v_proj.bias").view(H, hd))
            o = o.reshape(B, T, d)
        else:
            q = r16(lin(h, c + ".q_proj"))
            k = r16(lin(enc, c + ".k_proj", bias=False))
            v = r16(lin(enc, c + ".v_proj"))
            s = heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(hd)
            o = r16((s.softmax(-1) @ heads(v)).transpose(1, 2).reshape(B, T, d))
        x = r32(x + lin(o, c + ".out_proj", zero_cols=here and defect == "cross_out_bias"))
        # MLP
        h = r16(ln(x, p + ".final_layer_norm"))
        f = r16(F.gelu(lin(h, p + ".fc1")))
        x = r32(x + lin(f, p + ".fc2", zero_cols=here and defect == "fc2_bias"))
    return x, torch.stack(kc), torch.stack(vc)


@torch.no_grad()
def logits(x, W, cfg):
    """final LayerNorm(x) . E^T in float64: x [..][d] -> [..][V]."""
    x = torch.as_tensor(np.asarray(x, np.float64))
    h = F.layer_norm(x, (cfg.d_model,), _t(W, "decoder.layer_norm.weight"), _t(W, "decoder.layer_norm.bias"), 1e-5)
    return (h @ _t(W, "decoder.embed_tokens.weight").T).numpy()


def _errors(got, ref):
    """Per leading index: (|e| / |ref|, per 16-column tile |e_tile| sqrt(d / 16) / |ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and ref.shape[-1] % 16 == 0, (got.shape, ref.shape)
    d = ref.shape[-1]
    e = got - ref
    n = np.linalg.norm(ref, axis=-1)
    row = np.linalg.norm(e, axis=-1) / n
    tile = np.linalg.norm(e.reshape(e.shape[:-1] + (d // 16, 16)), axis=-1) * math.sqrt(d / 16) / n[..., None]
    return row, tile


def metrics(got, ref):
    """(row, tile) of e = got - ref over rows of d columns (any leading shape), both maxima
    over the leading indices: row = |e| / |ref|; tile = max_j |e[16j : 16j + 16]| sqrt(d / 16)
    / |ref| — one bad 16-column tile counts as if every tile were that bad, so the other
    d / 16 - 1 do not dilute it."""
    row, tile = _errors(got, ref)
    return float(row.max()), float(tile.max())


def worst(got, ref):
    """Where the tile metric peaks: (leading index tuple, first column of the tile, value)."""
    _, tile = _errors(got, ref)
    at = np.unravel_index(int(np.argmax(tile)), tile.shape)
    return tuple(int(i) for i in at[:-1]), 16 * int(at[-1]), float(tile[at])


# ---------------------------------------------------------------- shared test inputs
K_BOUND = 3.0   # the GPU tests' bound: K_BOUND x the emulation's own distance from hidden()


def config(d, H, Te=141, n_vocab=64):
    """The decoder tests' model: two decoder layers (the layer kernel's l -> l + 1 chain, the
    head kernel and the last segment's final LayerNorm all need a second layer), no encoder
    layer and a 64-entry vocabulary (the engine takes any count; the rows' tokens stay
    distinct), Te encoder keys (141: two 64-key chunks plus 13)."""
    from janus_amd.whisper import WhisperConfig
    return WhisperConfig(f"hidden-{d}-{Te}", d, H, 0, 2, n_audio_ctx=Te, n_vocab=n_vocab)


def inputs(cfg, rows, T, seed, n_enc=None):
    """Seeded forced tokens int32 [rows][T] and an encoder output fp16 [n_enc][Te][d] (unit
    normal, as a LayerNorm output is; not an encoder run)."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, cfg.n_vocab, (rows, T), generator=g).numpy().astype(np.int32)
    enc = torch.randn(n_enc or rows, cfg.n_audio_ctx, cfg.d_model, generator=g).half().numpy()
    return tokens, enc


def weights(cfg, seed):
    """janus_amd.whisper.synthetic_weights with the decoder's three residual-side biases (self
    out_proj, cross out_proj, fc2) three times as large (std 0.06): a kernel that drops one on
    a 16-column tile then stands clear of the bound at every width (at std 0.02 a tile of small
    draws at d_model 768 reached only 2.5x)."""
    from janus_amd.whisper import synthetic_weights
    W = synthetic_weights(cfg, seed)
    for i in range(cfg.dec_layers):
        for n in ("self_attn.out_proj", "encoder_attn.out_proj", "fc2"):
            W[f"decoder.layers.{i}.{n}.bias"] = W[f"decoder.layers.{i}.{n}.bias"] * np.float32(3.0)
    return W
