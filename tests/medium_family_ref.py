"""Test-side reference for the 1024-wide, 16-head family (medium.en, distil-medium.en), built on
the unchanged oracle (oracle/whisper.py is generic in cfg.d_model, cfg.n_heads and cfg.n_vocab)
and the helpers of tests/large_family_ref.py (the planner's description, the vocabulary
projection's partials merged on the host, the decoding rules' allowed mask):

* CUT: the real width, heads, 80 mel bins and the 51 864-entry vocabulary over 2 encoder and 2
  decoder layers;
* the greedy prompts of the free-running decode and the oracle's rows for them;
* the alignment case of tests/test_align_gpu.py's generator on CUT.

No GPU is touched here."""
import functools

import numpy as np

import align_ref
import large_family_ref as lf
import multilingual_ref as mr
from janus_amd import tokenizer as tok
from janus_amd import whisper as jw
from oracle import whisper as ow

CUT = jw.WhisperConfig("medium-cut", 1024, 16, 2, 2)
V = CUT.n_vocab            # 51 864 = 16 * 3241 + 8: the projection's last tile holds 8 columns
ROW_GROUP = 48             # rows of one block of the vocabulary projection at K = 1024
WEIGHT_SEED = 11
NEAR_TIE = 2e-3
ML = 32

describe = lf.describe
merge_parts = lf.merge_parts
allowed_mask = lf.allowed_mask
PART_DTYPE = lf.PART_DTYPE

# seeds chosen on the CPU oracle alone (tests/test_medium_family_gpu.py's docstring has the margins)
GREEDY_SEEDS = [900, 901, 902, 908, 904]
SAMPLE_ENC_SEED = 920
SAMPLE_SEEDS = [3001, 3006, 3007, 3010, 3017]
SAMPLE_T = 0.6
SAMPLE_ML = 24


@functools.lru_cache(maxsize=None)
def weights():
    return jw.synthetic_weights(CUT, seed=WEIGHT_SEED)


def greedy_prompts(tk):
    """Five prompts of lengths 1, 5, 1, 1 and 3, two with a <|startofprev|> prefix (each ends
    with <|startoftranscript|>: the *.en start sequence)."""
    sot = list(tk.sot_sequence)
    return [sot, [tk.sot_prev, 400, 1200, 3300] + sot, sot, sot, [tk.sot_prev, 9000] + sot]


def sot_index(tk, prompt):
    """Position of <|startoftranscript|> in a prompt: where no_speech_prob is read."""
    return len(prompt) - 1 - prompt[::-1].index(tk.sot)


def greedy_rows(enc, prompts, max_length=ML):
    """The oracle's greedy decode (per row dict(tokens, margins, sum_lp)) and the no-speech
    probability at each prompt's <|startoftranscript|>."""
    tk = tok.WhisperTokenizer()
    W = weights()
    rows = mr.greedy(enc, W, CUT, tk, prompts, max_length)
    nsp = [mr.no_speech_at(p, sot_index(tk, p), enc[b], W, CUT, tk) for b, p in enumerate(prompts)]
    return rows, nsp


def sampled_rows(enc_row, seeds, T=SAMPLE_T, max_length=SAMPLE_ML):
    """The oracle's sampler over one encoder row [1][1500][d], one hypothesis per noise seed."""
    tk = tok.WhisperTokenizer()
    n = len(seeds)
    return ow.greedy_cached(np.repeat(enc_row, n, 0), weights(), CUT, tk, max_length,
                            prompts=[list(tk.sot_sequence)] * n, no_speech=None, temperature=T, seeds=list(seeds))


# --------------------------------------------------------------------------- alignment
Q_SCALE = 4.0
ALIGN_WINDOWS = [(61, 3000, 0), (7, 437, 1)]       # (text tokens, size in mel frames, encoder row)


@functools.lru_cache(maxsize=None)
def align_case():
    """tests/test_align_gpu.py's generator on CUT: q_proj of the alignment layers (the last half
    of the decoder layers: layer 1, 16 heads) scaled by Q_SCALE, a time-smooth unit-variance
    encoder output, random text tokens, and the fp32 reference of each window (A, its DTW path,
    the token probabilities)."""
    import torch
    tk = tok.WhisperTokenizer()
    sot = len(tk.sot_sequence)
    W = dict(weights())
    heads = align_ref.default_heads(CUT)
    assert len(heads) == 16 and {l for l, _ in heads} == {1}
    for l in sorted({l for l, _ in heads}):
        for k in ("weight", "bias"):
            name = f"decoder.layers.{l}.encoder_attn.q_proj.{k}"
            W[name] = W[name] * np.float32(Q_SCALE)
    W = jw.engine_weights(W)
    g = torch.Generator().manual_seed(5)
    raw = torch.randn(2, 1500 + 24, CUT.d_model, generator=g)
    sm = torch.nn.functional.avg_pool1d(raw.transpose(1, 2), 25, 1).transpose(1, 2)
    enc = (sm / sm.std()).half()
    rng = np.random.default_rng(3)
    wins = []
    for (L, size, e) in ALIGN_WINDOWS:
        text = [int(t) for t in rng.integers(256, 50000, L)]
        seq = align_ref.sequence(tk, text)
        probs, logits = align_ref.forward(enc[e].float().numpy(), seq, W, CUT)
        A = align_ref.attention_matrix(probs, heads, size, sot)
        ti, fi = align_ref.dtw(-A)
        N, F = A.shape
        assert A.std() >= 0.5 / np.sqrt(len(heads)), (L, A.std())
        assert ((ti > 0) & (ti < N - 1) & (fi > 0) & (fi < F - 1)).any(), L
        wins.append(dict(text=text, size=size, enc=e, A=A, ti=ti, fi=fi,
                         p=align_ref.token_probs(logits, seq, sot, tk.eot)))
    return W, enc, wins
