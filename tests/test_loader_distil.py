"""JANUS_WHISPER_DIR loader with decoder depth != encoder depth (a distil checkpoint: the
teacher's 12 encoder layers over 4 decoder layers), on CPU. The file is written here with
the Hugging Face names at a cut-down width (d_model 64, one head) so it stays small; the
depths and the model name are distil-small.en's."""
import dataclasses

import numpy as np
import pytest

from janus_amd.whisper import CONFIGS, checkpoint_layers, load_weights, synthetic_weights

DISTIL = dataclasses.replace(CONFIGS["distil-small.en"], d_model=64, n_heads=1)
FULL = dataclasses.replace(CONFIGS["small.en"], d_model=64, n_heads=1)


def _write(path, W):
    from safetensors.numpy import save_file
    sd = {"model." + k: v.astype(np.float16) for k, v in W.items()}
    sd["proj_out.weight"] = W["decoder.embed_tokens.weight"].astype(np.float16)
    save_file(sd, str(path / "model.safetensors"))


def test_distil_checkpoint_loads(tmp_path, monkeypatch):
    assert (DISTIL.enc_layers, DISTIL.dec_layers) == (12, 4)
    W = synthetic_weights(DISTIL, seed=4)
    _write(tmp_path, W)
    monkeypatch.setenv("JANUS_WHISPER_DIR", str(tmp_path))
    got = load_weights(DISTIL)
    assert set(got) == set(W)
    assert checkpoint_layers(got, "encoder") == 12 and checkpoint_layers(got, "decoder") == 4
    assert "encoder.layers.11.fc2.weight" in got and "decoder.layers.3.encoder_attn.q_proj.weight" in got
    assert "decoder.layers.4.fc1.weight" not in got
    d = DISTIL.d_model
    shapes = {"encoder.conv1.weight": (d, 80, 3), "encoder.conv2.weight": (d, d, 3),
              "encoder.embed_positions.weight": (1500, d), "encoder.layers.11.fc1.weight": (4 * d, d),
              "decoder.embed_tokens.weight": (DISTIL.n_vocab, d), "decoder.embed_positions.weight": (448, d),
              "decoder.layers.3.encoder_attn.k_proj.weight": (d, d), "decoder.layers.3.fc2.weight": (d, 4 * d),
              "decoder.layer_norm.bias": (d,)}
    for k, shp in shapes.items():
        assert got[k].shape == shp and got[k].dtype == np.float32, k
    for k, v in got.items():
        assert np.array_equal(v, W[k].astype(np.float16).astype(np.float32)) or k == "decoder.embed_positions.weight", k


def test_full_depth_file_under_distil_name_rejected(tmp_path, monkeypatch):
    """small.en's 12 decoder layers under the distil name: a clear error, not a model that
    silently drops eight layers."""
    _write(tmp_path, synthetic_weights(FULL, seed=4))
    monkeypatch.setenv("JANUS_WHISPER_DIR", str(tmp_path))
    with pytest.raises(ValueError, match=r"distil-small\.en: 12 decoder layers, the config has 4"):
        load_weights(DISTIL)
    # and the other way round: a distil file under small.en's name
    _write(tmp_path, synthetic_weights(DISTIL, seed=4))
    with pytest.raises(ValueError, match=r"small\.en: 4 decoder layers, the config has 12"):
        load_weights(FULL)
    assert load_weights(DISTIL)["decoder.layer_norm.weight"].shape == (64,)
