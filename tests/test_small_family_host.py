"""Host side of the 768-wide, 12-head family (small.en, distil-small.en), no GPU: the
configs and the drop-in constructor, and the row cap of the sampled decodes — sequential
and speculative — following the model: rows sharing an encoder row read it in place by
default on the 8-head models only (PAIR blocks); this family's in-place blocks measured
slower than gathered copies, so it gathers a copy per row like any wider
model and keeps its calls at FALLBACK_ROWS_GATHER rows."""
import numpy as np
import torch

from janus_amd import whisper as jw
from janus_amd.services import transcriber as tr
from janus_amd.tokenizer import load_tokenizer

WIDER = jw.WhisperConfig("wide", 1024, 16, 2, 2)   # no shared-row kernel at this width


def test_distil_small_config():
    c = jw.CONFIGS["distil-small.en"]
    assert (c.d_model, c.n_heads, c.enc_layers, c.dec_layers) == (768, 12, 12, 4)
    s = jw.CONFIGS["small.en"]
    assert (s.d_model, s.n_heads, s.enc_layers, s.dec_layers) == (768, 12, 12, 12)


def test_whisper_model_resolves_distil_small(monkeypatch):
    """The reference's docstring example: WhisperModel('distil-small.en') (transcriber.py:11-27
    through Transcriber) resolves a config instead of raising ``unknown model size``."""
    built = []

    class Stub:
        def __init__(self, cfg, *a, **k):
            built.append(cfg)

    monkeypatch.setattr(tr, "WhisperEngine", Stub)
    t = tr.Transcriber("distil-small.en")
    assert t.model.model_size == "distil-small.en" and built == [jw.CONFIGS["distil-small.en"]]
    tr.WhisperModel("small.en")
    assert built[-1] is jw.CONFIGS["small.en"]


def test_shared_rows_in_place_by_model():
    for name in ("tiny.en", "base.en"):
        assert jw.shared_rows_in_place(jw.CONFIGS[name]), name
    for cfg in (jw.CONFIGS["small.en"], jw.CONFIGS["distil-small.en"], WIDER):
        assert not jw.shared_rows_in_place(cfg), cfg.name
    assert jw.shared_rows_in_place(None)
    assert jw.dec_path_xrows(2) == 0x40000 and jw.dec_path_xrows(4) == 0x80000 and jw.dec_path_xrows(0) == 0


def test_xrows_flag_matches_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "janus.h")).read()
    m = re.search(r"#define JANUS_DEC_PATH_XROWS\(n\)\s+\(\(\(\(uint32_t\)\(n\) >> 1\) & 3u\) << 18\)", src)
    assert m, "JANUS_DEC_PATH_XROWS(n) changed: keep whisper.dec_path_xrows in step"
    used = [int(v, 16) for v in re.findall(r"#define JANUS_DEC_PATH_[A-Z0-9_]+\s+(0x[0-9a-fA-F]+)u", src)]
    assert all(not (v & (3 << 18)) for v in used)     # bits 18-19 are XROWS' alone


class _Eng:
    """generate_segments / _fallback stand-in: every T = 0 row fails the log-prob gate and no
    sampled hypothesis passes, so each window walks all five temperatures; records the rows
    of every decode call."""

    class _Out:
        def __init__(self, n):
            self._n = n
            self.n_tokens = torch.full((n,), 3, dtype=torch.int32)

        def rows(self):
            return [([11, 12], -3.0, 0.0)] * self._n

    def __init__(self, cfg):
        self.cfg = cfg
        self.tokenizer = load_tokenizer()
        self.device = torch.device("cpu")
        self.calls = []

    def logmel_frames(self, pcm, offs, batch, decim, frames):
        return torch.zeros(batch, frames, 80, dtype=torch.float16)

    def encode(self, mel):
        return torch.zeros(mel.shape[0], 2, 4, dtype=torch.float16)

    def decode_ex(self, enc, prompts=None, enc_index=None, **kw):
        n = len(enc_index) if enc_index is not None else enc.shape[0]
        self.calls.append(n)
        return self._Out(n)


def test_sequential_fallback_cap_follows_model():
    tk = load_tokenizer()
    n = 70
    first = [tr.candidate(tk, [21, 22], -3.0, 0.0, 0.0) for _ in range(n)]
    keys = [(u, 0) for u in range(n)]
    for cfg, cap in ((jw.CONFIGS["small.en"], tr.FALLBACK_ROWS_GATHER), (jw.CONFIGS["base.en"], tr.FALLBACK_ROWS),
                     (WIDER, tr.FALLBACK_ROWS_GATHER)):
        eng = _Eng(cfg)
        assert tr.fallback_rows(eng) == cap
        tr._fallback(eng, tk, None, [[1]] * n, first, keys, 64, tr.TEMPERATURES, tr.BEST_OF)
        per = cap // tr.BEST_OF
        assert max(eng.calls) == per * tr.BEST_OF and sum(eng.calls) == 5 * n * tr.BEST_OF
        assert len(eng.calls) == 5 * -(-n // per)


def test_speculative_cap_follows_model():
    """generate_segments(speculative=True) sends 1 + 5 x 5 rows per window: its windows per
    call follow the same in-place-or-gather row cap as the sequential fallback — 12 windows
    (312 rows) on tiny.en / base.en, 2 (52 rows) on a model that gathers copies (the 768-wide
    family included), where it ran 12 whatever the model."""
    auds = [np.zeros(16000, np.float32) for _ in range(30)]
    per_row = 1 + 5 * tr.BEST_OF
    for cfg, cap in ((jw.CONFIGS["distil-small.en"], tr.FALLBACK_ROWS_GATHER), (jw.CONFIGS["tiny.en"], tr.FALLBACK_ROWS),
                     (WIDER, tr.FALLBACK_ROWS_GATHER)):
        eng = _Eng(cfg)
        st = tr.generate_segments(eng, auds, max_length=64, speculative=True)
        assert all(s.windows == 1 and s.fallback_decodes == 5 for s in st)
        wins = cap // per_row
        assert max(eng.calls) == wins * per_row <= cap
        assert len(eng.calls) == -(-len(auds) // wins) and sum(eng.calls) == len(auds) * per_row
