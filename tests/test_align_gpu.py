"""Word-level timestamps on the GPU (janus_whisper_align): the DTW, reduce and
token-probability kernels through their test entries against tests/align_ref.py / numpy, the
whole alignment call against the fp32 reference on synthetic weights, the words, the
end-to-end transcribe(word_timestamps=True), and the unchanged default.

Bounds of the alignment call (ALIGN_E_A, ALIGN_E_P): 4 x the largest error measured on the
MI355X over every case of this file (the margin the beam tests took), each
beside the estimate the number formats give; the figures are printed by the tests and kept in
profiles/word_align.json."""
import functools

import numpy as np
import pytest
import torch

import align_ref
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd.services import transcriber as tr
from janus_amd.whisper import CONFIGS, WhisperEngine, engine_weights, synthetic_weights
from janus_amd.workload import synth_speech

pytestmark = pytest.mark.gpu
TK = tok.WhisperTokenizer()
SOT = len(TK.sot_sequence)

# E_A = max |A_gpu - A_ref| over the cases below, measured on the MI355X: 7.60e-3 (tiny.en, the
# 222-token window over 1500 frames; the other tiny.en windows 1.8e-3 .. 3.6e-3, base.en
# 2.16e-3, distil-small.en 1.86e-3), x 4. The formats' own estimate: the alignment layers'
# scaled scores (std 4 at Q_SCALE 4) reach |s| of order 20 and carry the fp16 rounding of q
# and k (2^-11 relative each), so a probability is off by up to ~ 20 x 2^-10 = 2 % of itself,
# and so is its z-score of order 1 .. 10 before the 12 .. 24 heads are averaged: ~ 1e-2 at the
# largest of 335 000 entries.
# The measured figure lies under it.
ALIGN_E_A = 4 * 7.6e-3
# E_P = max |p_gpu / p_ref - 1| of the forced-token probabilities, measured 3.22e-3 (tiny.en,
# N = 34; probabilities ~ 2e-5: synthetic weights give a near-uniform vocabulary
# distribution), x 4. Estimate: a logit is a 384 .. 768-term product of the final LayerNorm
# row, which carries the fp16 roundings of four layers of activations (~ 1e-3 on values of
# order 1); a probability moves by the logit's absolute error, relatively.
ALIGN_E_P_REL = 4 * 3.3e-3
SEEN = {}   # the figures behind the two constants, printed by test_align_figures


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ DTW kernel
def gpu_dtw(gpu, x):
    N, F = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(gpu)
    trace = torch.zeros((N + 1) * (F + 1), dtype=torch.uint8, device=gpu)
    ti = torch.zeros(N + F, dtype=torch.int32, device=gpu)
    fi = torch.zeros(N + F, dtype=torch.int32, device=gpu)
    ln = torch.zeros(1, dtype=torch.int32, device=gpu)
    nat.call("janus_align_dtw_f32", dx.data_ptr(), N, F, trace.data_ptr(), ti.data_ptr(), fi.data_ptr(),
             ln.data_ptr(), stream())
    L = int(ln.cpu()[0])
    ti, fi = ti.cpu().numpy(), fi.cpu().numpy()
    assert (ti[L:] == -1).all() and (fi[L:] == -1).all()
    return ti[:L], fi[:L]


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("N,F", [(1, 1), (3, 2), (2, 3), (17, 218), (225, 1500)])
def test_dtw_kernel_exact(gpu, N, F, quantised):
    """The DTW kernel's path equals align_ref.dtw's, element for element: random fp32
    matrices, and matrices of multiples of 0.25, whose sums are exact so that ties occur on
    every diagonal and the comparison order decides."""
    rng = np.random.default_rng(1000 * N + F + int(quantised))
    x = rng.standard_normal((N, F)).astype(np.float32)
    if quantised:
        x = (np.round(x * 4) / 4).astype(np.float32)
    rt, rf = align_ref.dtw(x)
    ti, fi = gpu_dtw(gpu, x)
    assert np.array_equal(ti, rt) and np.array_equal(fi, rf)
    align_ref.check_path_shape(ti, fi, N, F)


# ------------------------------------------------------------------ reduce kernel
@pytest.mark.parametrize("n", [3, 35])
@pytest.mark.parametrize("heads", [1, 12, 24])
@pytest.mark.parametrize("F", [3, 4, 7, 218, 1500])
def test_reduce_kernel(gpu, F, heads, n):
    """Normalise over rows, median of 7 along frames (none at F = 3, every reflected index at
    F = 4), mean over heads, against numpy in float64 on the same fp32 input. The values are
    z-scores of order 1 and the kernel's mean / variance / median arithmetic is fp64, so the
    error is the final fp32 rounding plus one fp32 mean / variance's worth: 1e-5 relative to
    max(1, |ref|). The median picks one of its 7 inputs: no further error."""
    rng = np.random.default_rng(F * 100 + heads * 3 + n)
    P = (rng.random((heads, n, F)) ** 4).astype(np.float32)
    want = align_ref.reduce_heads(P, SOT)
    dP = torch.from_numpy(P).to(gpu)
    out = torch.zeros(n - SOT - 1, F, dtype=torch.float32, device=gpu)
    nat.call("janus_align_reduce_f32", dP.data_ptr(), heads, n, F, SOT, out.data_ptr(), stream())
    got = out.cpu().numpy().astype(np.float64)
    assert want.shape == got.shape
    assert (np.abs(got - want) <= 1e-5 * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()


# ------------------------------------------------------------------ token probability
@pytest.mark.parametrize("rows,d,V", [(1, 384, 50256), (70, 512, 50256), (5, 768, 1001)])
def test_token_prob_kernel(gpu, rows, d, V):
    """LayerNorm -> logits over V ids -> softmax at the target, against float64 on the fp16
    LayerNorm rows the kernel multiplies; 70 rows cross the 64-row chunk, V = 1001 is no
    multiple of 8. Bound: fp32 accumulation of exact fp16 products, logits within 1e-4 of the
    float64 ones (the GEMM tests' fp32-output bound), so 2e-4 relative on a probability."""
    g = torch.Generator().manual_seed(rows * 7 + d)
    x = torch.randn(rows, d, generator=g)
    gam = 1 + 0.1 * torch.randn(d, generator=g)
    bet = 0.02 * torch.randn(d, generator=g)
    Wt = (torch.randn(V, d, generator=g) / np.sqrt(d)).half()
    target = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    a = torch.nn.functional.layer_norm(x, (d,), gam, bet, 1e-5).half().double()
    lg = a @ Wt.double().T
    want = torch.softmax(lg, -1)[torch.arange(rows), target.long()].numpy()
    out = torch.zeros(rows, dtype=torch.float32, device=gpu)
    dx, dg, db, dW, dt = x.to(gpu), gam.to(gpu), bet.to(gpu), Wt.to(gpu), target.to(gpu)
    nat.call("janus_align_token_prob_f16", dx.data_ptr(), dg.data_ptr(), db.data_ptr(), dW.data_ptr(),
             rows, d, V, dt.data_ptr(), out.data_ptr(), stream())
    got = out.cpu().numpy().astype(np.float64)
    # the kernel's own LayerNorm may round a row's fp16 value the other way: 2^-11 relative
    # on an operand of a d-term sum of random signs, ~ 2^-11 on a logit of order 1
    assert np.allclose(got, want, rtol=2e-4 + 2.0 ** -10, atol=0), np.abs(got / want - 1).max()


# ------------------------------------------------------------------ the alignment call
Q_SCALE = 4.0   # encoder_attn.q_proj of the alignment layers, so that the rows peak

# (model, [(text length, size in mel frames, encoder row)]): tiny.en in one batched call over a
# shared pair of encoder rows — 1 / 5 / 33 / 222 text tokens (one tile, one tile, three, 15
# with a ragged last one), sizes 3000 / 437 / 6 (F = 1500, 218 and 3: unfiltered, N > F)
CASES = {
    "tiny.en": [(1, 3000, 0), (5, 437, 1), (33, 6, 0), (222, 3000, 1), (33, 3000, 1)],
    "base.en": [(19, 3000, 0)],
    "distil-small.en": [(26, 700, 0)],
}


@functools.lru_cache(maxsize=None)
def reference(model):
    """Synthetic weights whose alignment layers' cross-attention queries are scaled (plain
    synthetic weights give near-uniform attention), a time-smooth unit-variance encoder
    output (a peak spans several frames and survives the median filter), random text tokens,
    and the fp32 reference of every window: A, its DTW path, the token probabilities. CPU only."""
    cfg = CONFIGS[model]
    W = dict(synthetic_weights(cfg, seed=11))
    heads = align_ref.default_heads(cfg)
    for l in sorted({l for l, _ in heads}):
        for k in ("weight", "bias"):
            name = f"decoder.layers.{l}.encoder_attn.q_proj.{k}"
            W[name] = W[name] * np.float32(Q_SCALE)
    W = engine_weights(W)
    g = torch.Generator().manual_seed(5)
    n_enc = 1 + max(e for _, _, e in CASES[model])
    raw = torch.randn(n_enc, 1500 + 24, cfg.d_model, generator=g)
    sm = torch.nn.functional.avg_pool1d(raw.transpose(1, 2), 25, 1).transpose(1, 2)
    enc = (sm / sm.std()).half()
    rng = np.random.default_rng(3)
    wins = []
    for (L, size, e) in CASES[model]:
        text = [int(t) for t in rng.integers(256, 50000, L)]
        seq = align_ref.sequence(TK, text)
        probs, logits = align_ref.forward(enc[e].float().numpy(), seq, W, cfg)
        A = align_ref.attention_matrix(probs, heads, size, SOT)
        ti, fi = align_ref.dtw(-A)
        N, F = A.shape
        # the z-scores have unit variance per head and frame; the mean over h independent
        # heads has 1 / sqrt(h): the case must keep at least half of that (it is no flat matrix)
        if N >= 6 and F >= 6:
            assert A.std() >= 0.5 / np.sqrt(len(heads)), (model, L, A.std())
            # and its optimal path leaves the border: some cell strictly inside the matrix
            assert ((ti > 0) & (ti < N - 1) & (fi > 0) & (fi < F - 1)).any(), (model, L)
        wins.append(dict(text=text, size=size, enc=e, A=A, ti=ti, fi=fi,
                         p=align_ref.token_probs(logits, seq, SOT, TK.eot)))
    return W, enc, wins


@functools.lru_cache(maxsize=None)
def aligned(model):
    W, enc, wins = reference(model)
    eng = WhisperEngine(CONFIGS[model], weights=W)
    out = eng.align(enc.to(eng.device), [w["text"] for w in wins], [w["size"] for w in wins],
                    enc_index=[w["enc"] for w in wins], return_attention=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("model", list(CASES))
def test_align_matches_reference(gpu, model):
    """A, the token probabilities and the path of every window against the fp32 reference.
    The path is not compared for identity: the GPU path is optimal on the GPU matrix, whose
    entries lie within E of the reference's, so on the reference matrix it costs at most
    2 (N + F) E more than the reference's optimum (a path has at most N + F cells)."""
    _, _, wins = reference(model)
    for k, (w, a) in enumerate(zip(wins, aligned(model))):
        N, F = w["A"].shape
        assert a.attention.shape == (N, F) and a.token_probs.shape == (len(w["text"]),)
        eA = float(np.abs(a.attention - w["A"]).max())
        eP = float(np.abs(a.token_probs / w["p"] - 1).max())
        SEEN[(model, k)] = (eA, eP, float(np.abs(a.token_probs - w["p"]).max()), float(w["p"].mean()))
        print(f"align {model} window {k}: N {N} F {F} max|dA| {eA:.3e} max rel dp {eP:.3e}")
        assert eA <= ALIGN_E_A
        assert eP <= ALIGN_E_P_REL
        assert (a.token_probs > 0).all() and (a.token_probs <= 1).all()
        align_ref.check_path_shape(a.text_indices, a.time_indices, N, F)
        x = -w["A"]
        got = align_ref.path_cost(x, a.text_indices, a.time_indices)
        opt = align_ref.path_cost(x, w["ti"], w["fi"])
        assert got <= opt + 2 * (N + F) * ALIGN_E_A, (got, opt)


def test_align_figures(gpu):
    """Prints the figures behind ALIGN_E_A / ALIGN_E_P_REL (run after the cases above)."""
    for model in CASES:
        aligned(model)
    if not SEEN:
        for model in CASES:
            test_align_matches_reference(gpu, model)
    print("max |dA|", max(v[0] for v in SEEN.values()), "max rel dp", max(v[1] for v in SEEN.values()))


@pytest.mark.parametrize("model", list(CASES))
def test_words_from_gpu_path(gpu, model):
    """The words the GPU path gives through transcriber.py's host rules equal align_ref's host
    rules run on that same path, exactly."""
    _, _, wins = reference(model)
    for w, a in zip(wins, aligned(model)):
        got = tr.find_alignment(TK, w["text"], a)
        want = align_ref.words_of(TK, w["text"], a.text_indices, a.time_indices, a.token_probs)
        assert [(g["word"], g["tokens"], g["start"], g["end"], g["probability"]) for g in got] == \
            [tuple(r) for r in want]
        assert len(got) >= 1 and sum(len(g["tokens"]) for g in got) == len(w["text"])


def test_align_rejects_bad_calls(gpu):
    """janus_whisper_align validates before it runs anything: a sequence past n_text_ctx, a size
    outside [2, 3000], a window without text, a text token >= eot, an enc_index out of range."""
    W, enc, _ = reference("tiny.en")
    eng = WhisperEngine(CONFIGS["tiny.en"], weights=W)
    denc = enc.to(eng.device)

    def call(seq, size, ei=0, stride=None):
        seq = np.array(seq, np.int32)
        n = len(seq)
        ln, sz, e = np.array([n], np.int32), np.array([size], np.int32), np.array([ei], np.int32)
        ps = 2000
        bufs = [torch.zeros(ps, dtype=torch.int32, device=eng.device) for _ in range(3)]
        pr = torch.zeros(max(n, 1), dtype=torch.float32, device=eng.device)
        nat.call("janus_whisper_align", eng._h, denc.data_ptr(), int(denc.shape[0]), 1, seq.ctypes.data,
                 ln.ctypes.data, stride or n, sz.ctypes.data, e.ctypes.data, SOT, TK.eot,
                 bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ps, pr.data_ptr(), None, 0,
                 stream())

    good = align_ref.sequence(TK, [300, 301])
    call(good, 3000)
    for seq, size, ei, msg in ((align_ref.sequence(TK, [300] * 446), 3000, 0, "n_text_ctx"),
                               (good, 1, 0, "size"), (good, 3001, 0, "size"),
                               (align_ref.sequence(TK, []), 3000, 0, "text token"),
                               (align_ref.sequence(TK, [TK.eot + 5]), 3000, 0, "< eot"),
                               (good, 3000, 2, "enc_index")):
        with pytest.raises(nat.JanusNativeError, match=msg):
            call(seq, size, ei)
    heads = np.array([[0, 0], [9, 0]], np.int32)
    with pytest.raises(nat.JanusNativeError, match="out of range"):
        nat.call("janus_whisper_set_alignment_heads", eng._h, heads.ctypes.data, 2)


def test_alignment_heads_override(gpu):
    """WhisperEngine(alignment_heads=...): the named heads replace the default set."""
    W, enc, wins = reference("tiny.en")
    cfg = CONFIGS["tiny.en"]
    heads = [(1, 2), (3, 0), (2, 5)]
    eng = WhisperEngine(cfg, weights=W, alignment_heads=heads)
    w = wins[1]
    a = eng.align(enc.to(eng.device), [w["text"]], [w["size"]], enc_index=[w["enc"]], return_attention=True)[0]
    seq = align_ref.sequence(TK, w["text"])
    probs, _ = align_ref.forward(enc[w["enc"]].float().numpy(), seq, W, cfg)
    A = align_ref.attention_matrix(probs, heads, w["size"], SOT)
    # three heads average less than twelve: the same per-head error, up to sqrt(12 / 3) as much
    assert np.abs(a.attention - A).max() <= 2 * ALIGN_E_A
    assert np.abs(a.attention - w["A"]).max() > 4 * ALIGN_E_A        # not the default set's matrix


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def model_tiny():
    return tr.WhisperModel("tiny.en")


def clip():
    return np.ascontiguousarray(synth_speech(66, 36.0)[::3])        # 36 s: more than one seek window


def begins_word(text_tokens):
    """The tokens' first word starts with a space and none of their words is a bare
    punctuation mark that merge_punctuations would move into a neighbouring segment."""
    words = TK.split_to_word_tokens(text_tokens)[0]
    marks = tr.PREPEND_PUNCTUATIONS + tr.APPEND_PUNCTUATIONS
    return bool(words) and words[0].startswith(" ") and not any(w.strip() in marks for w in words)


def test_transcribe_word_timestamps(gpu):
    """transcribe(word_timestamps=True) on a clip of several seek windows: every segment has
    ``words``, with ordered times inside the clip and probabilities in (0, 1]; the seeks
    (rule 8), the segments and their words equal align_ref's loop run over the GPU's window
    results.

    Each segment's words concatenate to its text — where rule 7 lets them: it hands out whole
    words by token count, so a word that spans a segment boundary goes to the segment it
    starts in and shifts every later segment of that window (faster-whisper does the same;
    with a real vocabulary a segment's first text token begins with a space and the case does
    not arise, the synthetic table has ~ 30 % tokens without one). The check therefore runs on
    the windows all of whose sub-segments begin a word, computed from the tokens alone, and at
    least one such window with two or more segments must exist."""
    m = model_tiny()
    audio = clip()
    segs, info = m.transcribe(audio, word_timestamps=True, temperature=(0.0,), max_length=24)
    segs = list(segs)
    assert len(segs) >= 2 and len({s.seek for s in segs}) >= 2
    last = 0.0
    for s in segs:
        assert s.words is not None
        for w in s.words:
            assert 0.0 <= w.start <= info.duration and 0.0 <= w.end <= info.duration
            assert w.start >= last
            last = w.start
            assert 0.0 < w.probability <= 1.0
    st = tr.generate_segments(m.engine, [audio], max_length=24, temperatures=(0.0,), word_timestamps=True)[0]
    assert [(g.seek, g.start, g.end, g.text) for g in st.segments] == [(g.seek, g.start, g.end, g.text) for g in segs]
    assert len(st.window_alignments) == st.windows == len(st.window_seeks) >= 2
    # windows whose every sub-segment (dropped ones too) begins a word
    clean = set()
    for toks, (seek, size, _) in zip(st.window_tokens, st.window_seeks):
        parts = [[t for t in part if t < TK.eot] for (_, _, part) in tr.split_window(TK, list(toks), seek, size)[0]]
        if parts and all(begins_word(p) for p in parts):
            clean.add(seek)
    checked = 0
    for s in segs:
        if s.seek in clean:
            assert len(s.words) >= 1 and "".join(w.word for w in s.words) == s.text
            checked += 1
    assert checked >= 2 and any(sum(1 for s in segs if s.seek == k) >= 2 for k in clean)
    wins = [(t, avg, nsp, a) for (t, avg, nsp), a in zip(st.window_rows, st.window_alignments)]
    seeks, ref = align_ref.seek_loop(TK, st.content_frames, wins)
    assert st.window_seeks == seeks
    assert [(g.seek, g.tokens, [(w.word, w.start, w.end, w.probability) for w in g.words])
            for g in st.segments] == [(a, t, ws) for (a, _, _, t, ws) in ref]
    for g, r in zip(st.segments, ref):
        assert abs(g.start - r[1]) < 1e-9 and abs(g.end - r[2]) < 1e-9


def test_default_is_unchanged(gpu):
    """word_timestamps=False is the call without the keyword: same segments, no words."""
    m = model_tiny()
    audio = clip()
    a = list(m.transcribe(audio, temperature=(0.0,), max_length=24)[0])
    b = list(m.transcribe(audio, word_timestamps=False, temperature=(0.0,), max_length=24)[0])
    assert a == b and len(a) >= 1 and all(s.words is None for s in a)


def test_align_between_staggered_decodes(gpu):
    """An align call between two staggered decode calls leaves the second call's output
    bit-identical to a run without it: the alignment uses no decoder state slot."""
    W, enc, wins = reference("tiny.en")
    eng = WhisperEngine(CONFIGS["tiny.en"], weights=W)
    denc = enc.to(eng.device)
    L, S = 40, 20

    def run(with_align):
        eng.decode_ex(denc, max_length=L, pos_offset=[0, 0], steps=S)
        if with_align:
            w = wins[2]
            al = eng.align(denc, [w["text"]], [w["size"]], enc_index=[w["enc"]])
            assert al[0] is not None
        out = eng.decode_ex(denc, max_length=L, pos_offset=[S, S], steps=L - 1 - S)
        torch.cuda.synchronize()
        return [t.cpu() for t in (out.tokens, out.n_tokens, out.sum_logprob, out.no_speech_prob)]

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(a[1].min()) >= 1
