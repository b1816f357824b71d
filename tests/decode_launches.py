"""The decode calls whose launch structure tests/golden/decode_launches.json records
(tests/golden/make_decode_launches.py writes it, test_whisper_gpu.py::test_decode_launch_counts
checks it): per call (positions, launches, enc_rows, persistent) as decode_info() and
decode_path() report them. Every call runs without early-exit polling (check_every 0) to
max_length 24, so every position runs and the counts depend on the call's plan alone, not on
what the rows decode (the encoder output is zeros)."""
import json
import os

import torch

from janus_amd.whisper import (CONFIGS, DEC_PATH_FUSED_LN, DEC_PATH_LN_FUSE, DEC_PATH_NO_CVP,
                               DEC_PATH_NO_EMBED_LN, DEC_PATH_NO_SEL_EMBED, DEC_PATH_NO_XABSORB,
                               DEC_PATH_RESID_LN, DEC_PATH_XGROUP, WhisperConfig, WhisperEngine,
                               dec_path_ln_mask, dec_path_xrows, synthetic_weights)

ML = 24
SHARED = [0] * 5 + [1] * 5          # best_of = 5 rows per window, 2 windows
MODELS = {"tiny": (CONFIGS["tiny.en"], 5), "base": (CONFIGS["base.en"], 7),
          "cut": (WhisperConfig("small-cut", 768, 12, 2, 4), 11)}     # (config, weight seed)

# name -> (model, rows, decode_ex keywords)
FLAG_CASES = {
    "default": 0, "no_cvp": DEC_PATH_NO_CVP, "no_sel_embed": DEC_PATH_NO_SEL_EMBED,
    "no_embed_ln": DEC_PATH_NO_EMBED_LN, "no_xabsorb": DEC_PATH_NO_XABSORB,
    "ln_mask_0": dec_path_ln_mask(0), "ln_mask_15": dec_path_ln_mask(15),
    "resid_ln": DEC_PATH_RESID_LN, "fused_ln": DEC_PATH_FUSED_LN, "ln_fuse": DEC_PATH_LN_FUSE,
}
CASES = {name: ("base", 4, dict(path_flags=f)) for name, f in FLAG_CASES.items()}
CASES.update({f"persistent_{m}": ("base", 8, dict(persistent=m)) for m in (1, 2, 3)})
CASES.update({
    "shared_pairs": ("tiny", 2, dict(enc_index=SHARED)),
    "shared_groups": ("tiny", 2, dict(enc_index=SHARED, path_flags=DEC_PATH_XGROUP)),
    "shared_xrows4": ("cut", 2, dict(enc_index=SHARED, path_flags=dec_path_xrows(4))),
    "sampled": ("base", 4, dict(temperature=0.6, seeds=[11, 12, 13, 14])),
    "beam": ("base", 2, dict(beam_size=4)),
    # a fresh call of 12 positions, then rows 0-1 fresh beside rows 2-3 continuing for 11
    "stagger_fresh": ("base", 4, dict(pos_offset=[0, 0, 0, 0], steps=12)),
    "stagger_continued": ("base", 4, dict(pos_offset=[0, 0, 12, 12], steps=11)),
})


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launches.json")


def golden():
    with open(golden_path()) as f:
        return json.load(f)


def make_engine(model):
    cfg, seed = MODELS[model]
    return WhisperEngine(cfg, synthetic_weights(cfg, seed=seed))


def run_case(eng, name):
    """Runs CASES[name] on ``eng`` (the engine of its model): [positions, launches, enc_rows,
    persistent]. "stagger_continued" continues the slots "stagger_fresh" left: run it next."""
    _, rows, kw = CASES[name]
    kw = dict(kw)
    enc = torch.zeros(rows, eng.cfg.n_audio_ctx, eng.cfg.d_model, dtype=torch.float16, device=eng.device)
    if "beam_size" in kw:
        eng.decode_beam(enc, max_length=ML, check_every=0, **kw)
    else:
        eng.decode_ex(enc, max_length=ML, check_every=0, **kw)
    torch.cuda.synchronize()
    positions, launches = eng.decode_info()
    path = eng.decode_path()
    return [positions, launches, path.enc_rows, path.persistent]
