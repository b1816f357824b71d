"""The decoder residual-stream reference (tests/decoder_ref.py) against the oracle, and its
sensitivity: every seeded defect lies at least 3x over the bound the GPU tests
(tests/test_decoder_hidden_gpu.py) hold the engine to on the same inputs. CPU only."""
import numpy as np
import pytest

import decoder_ref as ref
from oracle import whisper as ow

ROWS, T = 8, 12
SHAPES = [(512, 8), (384, 6), (768, 12)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"d{s[0]}")
def case(request):
    d, H = request.param
    cfg = ref.config(d, H)
    W = ref.weights(cfg, seed=3)
    tokens, enc = ref.inputs(cfg, ROWS, T, seed=5)
    x, k, v = ref.hidden(tokens, enc, W, cfg)
    return dict(cfg=cfg, W=W, tokens=tokens, enc=enc, x=x, k=k, v=v)


def test_hidden_matches_oracle_logits(case):
    """final LayerNorm(hidden) . E^T is oracle.whisper.decoder_logits (fp32) to fp32 rounding:
    the logits are O(1) sums of d products, held to 1e-5 of their largest magnitude."""
    c = case
    got = ref.logits(c["x"], c["W"], c["cfg"])
    want = ow.decoder_logits(c["tokens"], c["enc"].astype(np.float32), c["W"], c["cfg"]).numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"logits vs oracle: {err:.2e}")
    assert err <= 1e-5, err


def test_cache_rows_are_the_projections(case):
    """The reference's cache rows are its own k / v projections of LN1(x) per layer: checked
    on layer 0, whose input is the embedding alone."""
    import torch
    import torch.nn.functional as F
    c = case
    W, cfg = c["W"], c["cfg"]
    t = lambda n: torch.from_numpy(W[n]).double()
    x0 = t("decoder.embed_tokens.weight")[torch.as_tensor(c["tokens"].astype(np.int64))] + \
        t("decoder.embed_positions.weight")[:T]
    p = "decoder.layers.0.self_attn"
    h = F.layer_norm(x0, (cfg.d_model,), t(p + "_layer_norm.weight"), t(p + "_layer_norm.bias"), 1e-5)
    np.testing.assert_allclose(c["k"][0], F.linear(h, t(p + ".k_proj.weight")).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(c["v"][0], F.linear(h, t(p + ".v_proj.weight"), t(p + ".v_proj.bias")).numpy(),
                               rtol=0, atol=1e-12)
    assert c["k"].shape == (cfg.dec_layers, ROWS, T, cfg.d_model)


def test_causal_and_row_independent(case):
    """What lets the GPU tests share one reference: a prefix of the positions and a subset of
    the rows give the same rows."""
    c = case
    x, k, _ = ref.hidden(c["tokens"][2:5, :7], c["enc"][2:5], c["W"], c["cfg"])
    np.testing.assert_allclose(x, c["x"][2:5, :7], rtol=0, atol=1e-11)
    np.testing.assert_allclose(k, c["k"][:, 2:5, :7], rtol=0, atol=1e-11)
    xs, _, _ = ref.hidden(c["tokens"][[0, 1, 2]], c["enc"][[4]], c["W"], c["cfg"], enc_index=[0, 0, 0])
    xo, _, _ = ref.hidden(c["tokens"][[0, 1, 2]], c["enc"][[4, 4, 4]], c["W"], c["cfg"])
    np.testing.assert_array_equal(xs, xo)


def test_metrics():
    """row / tile on a constructed error: one tile off by a known amount."""
    r = np.ones((2, 3, 64))
    g = r.copy()
    g[1, 2, 16:32] += 0.5
    row, tile = ref.metrics(g, r)
    assert row == pytest.approx(0.5 * 4 / 8) and tile == pytest.approx(0.5 * 4 * 2 / 8)
    assert ref.worst(g, r) == ((1, 2), 16, pytest.approx(tile))
    assert ref.metrics(r, r) == (0.0, 0.0)


@pytest.fixture(scope="module")
def bound(case):
    """The GPU tests' bound on these inputs: K_BOUND x the emulation's distance."""
    c = case
    out = {}
    for xabs in (True, False):
        x, k, v = ref.hidden(c["tokens"], c["enc"], c["W"], c["cfg"], emulate=True, xabs=xabs)
        row, tile = ref.metrics(x, c["x"])
        print(f"d {c['cfg'].d_model} emulation xabs={xabs}: row {row:.2e} tile {tile:.2e} "
              f"cache k {ref.metrics(k, c['k'])[1]:.2e} v {ref.metrics(v, c['v'])[1]:.2e} "
              f"row norm {np.linalg.norm(c['x'], axis=-1).mean():.1f}")
        out[xabs] = ref.K_BOUND * tile
    return out


@pytest.mark.parametrize("defect", sorted(ref.DEFECTS))
def test_defect_exceeds_bound(case, bound, defect):
    """Each seeded defect (layer 1, row 5, columns 208 .. 223 where it has any) is at least 3x
    over the larger of the two bounds (absorbed / projected cross-attention) on the tile
    metric."""
    c = case
    x, _, _ = ref.hidden(c["tokens"], c["enc"], c["W"], c["cfg"], defect=defect, layer=1, row=5, col0=208)
    _, tile = ref.metrics(x, c["x"])
    at = ref.worst(x, c["x"])
    b = max(bound.values())
    print(f"d {c['cfg'].d_model} {defect}: tile {tile:.2e} = {tile / b:.1f}x the bound {b:.2e}, worst at {at}")
    assert tile >= 3 * b, (defect, tile, b)
    if defect.endswith("_bias"):
        assert at[1] == 208
    if defect in ("pos_off_by_one", "cache_late"):
        assert at[0][0] == 5     # the row
