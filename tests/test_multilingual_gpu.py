"""The multilingual models on the GPU against tests/multilingual_ref.py (the unchanged oracle):
the language head kernel, janus_whisper_detect_language, the greedy decode with the
no-speech probability read at the <|startoftranscript|> position on every decode form, the
last vocabulary column of the 51 865-entry projection, beam search, and transcribe end to
end (language=None, task="translate", word_timestamps).

Probability bounds are 4 x the largest relative error measured on the MI355X over the cases
of the test (the convention of tests/test_align_gpu.py; profiles/multilingual.json keeps the
measured figures), written beside what the number formats alone predict."""
import ctypes

import numpy as np
import pytest
import torch

import beam_ref
import multilingual_ref as mr
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd.services import transcriber as tr
from janus_amd.whisper import CONFIGS, WhisperEngine, mel_filters, synthetic_weights
from janus_amd.workload import synth_speech
from oracle import whisper as ow

pytestmark = pytest.mark.gpu
TINY = CONFIGS["tiny"]
V = TINY.n_vocab                      # 51 865 = 16 * 3241 + 9
NEAR_TIE = 2e-3                       # tests/test_whisper_gpu.py: logit units
NSP_REL = 5e-3                        # tests/test_whisper_gpu.py: no_speech_prob, relative
P_FLOOR = 1e-6                        # probabilities below it are compared absolutely
# Language head (fp32 LayerNorm, fp16 weights exact in the fp32 products, fp32 sums): only the
# summation order differs from float64, so a logit errs by about sqrt(d) * 2^-24 * its terms
# ~ 1e-6 and a probability by the same relative amount; __expf adds ~2 ulp (2e-7). Measured
# on the MI355X over the 36 cases below and the dominant-logit case: 1.143e-6 largest
# relative error (rows 64, d 768, 128 languages; 4.1e-7 .. 1.1e-6 over the others).
HEAD_BOUND = 4 * 1.143e-6
# detect_language (the decoder's fp16 activations and fp16 MFMA operands in front of the
# head): the language logits err like the decode's logits, ~1e-3 absolute (NEAR_TIE is 2e-3),
# a probability by that relative amount. Measured: 1.58e-3 (tiny), 2.80e-3 (small) largest
# relative error over the three windows.
DETECT_BOUND = 4 * 2.80e-3


def rel_err(got, ref):
    """Largest relative error of probabilities: |got - ref| / max(ref, P_FLOOR)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(ref, P_FLOOR)).max())


# ------------------------------------------------------------------ 1. the language head
def head_inputs(rows, d, n_lang, seed, kind="random"):
    """x f32 [rows][d] (mean 2, std 3), gamma, beta, the n_lang embedding rows fp16, and the
    float64 reference (probs, best, top-2 logit gap per row)."""
    g = torch.Generator().manual_seed(seed)
    x = 2.0 + 3.0 * torch.randn(rows, d, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(d, generator=g)
    beta = 0.2 * torch.randn(d, generator=g)
    E = (0.05 * torch.randn(n_lang, d, generator=g)).half()
    if kind == "equal":
        E[:] = E[0]
    x64, g64, b64 = x.double().numpy(), gamma.double().numpy(), beta.double().numpy()
    mu = x64.mean(1, keepdims=True)
    y = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(1, keepdims=True) + 1e-5) * g64 + b64
    if kind == "dominant":       # language 5's row along row 0's normalised row: its logit there is ~130
        E[5] = torch.from_numpy(y[0] * (130.0 / (y[0] ** 2).sum())).half()
    L = y @ E.double().numpy().T
    srt = np.sort(L, axis=1)
    gap = srt[:, -1] - srt[:, -2] if n_lang > 1 else np.full(rows, np.inf)
    return x, gamma, beta, E, mr.softmax64(L), np.argmax(L, axis=1), gap, L


def run_head(gpu, x, gamma, beta, E, lang_begin):
    rows, d = x.shape
    n_lang = E.shape[0]
    emb = torch.zeros(V, d, dtype=torch.float16, device=gpu)
    emb[lang_begin:lang_begin + n_lang] = E.to(gpu)
    xd, gd, bd = x.to(gpu), gamma.to(gpu), beta.to(gpu)
    probs = torch.full((rows, n_lang), -1.0, dtype=torch.float32, device=gpu)
    best = torch.full((rows,), -1, dtype=torch.int32, device=gpu)
    nat.call("janus_lang_head_f16", xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), emb.data_ptr(), d,
             lang_begin, n_lang, rows, probs.data_ptr(), best.data_ptr(), nat.stream_ptr())
    torch.cuda.synchronize()
    return probs.cpu().numpy(), best.cpu().numpy()


HEAD_LANGS = [(50259, 99), (50259, 1), (7, 128), (V - 100, 100)]


@pytest.mark.parametrize("d", [384, 512, 768])
@pytest.mark.parametrize("rows", [1, 3, 64])
def test_lang_head_kernel(gpu, rows, d):
    worst = 0.0
    for k, (lb, n) in enumerate(HEAD_LANGS):
        # (seed base picked on the CPU: every case's smallest reference gap is >= 2.6e-3)
        x, gamma, beta, E, p_ref, b_ref, gap, _ = head_inputs(rows, d, n, 12000 + 10 * d + rows + k)
        assert (gap >= 1e-3).all(), (lb, n, gap.min())         # the precondition of an exact best
        p, b = run_head(gpu, x, gamma, beta, E, lb)
        assert np.isfinite(p).all() and (p >= 0).all()
        assert np.array_equal(b, b_ref), (lb, n)
        assert np.abs(p.sum(1) - 1).max() < 1e-5
        e = rel_err(p, p_ref)
        worst = max(worst, e)
        print(f"lang head rows {rows} d {d} ({lb}, {n}): rel err {e:.3e}")
        assert e <= HEAD_BOUND, (lb, n, e)
    print(f"lang head rows {rows} d {d}: worst {worst:.3e}")


def test_lang_head_extremes(gpu):
    """One logit dominating by more than 100: the others underflow, nothing is NaN, the sum
    is 1. All language rows equal: uniform 1 / n and best 0 (the lowest index of a tie)."""
    x, gamma, beta, E, p_ref, b_ref, gap, L = head_inputs(3, 512, 99, 77, kind="dominant")
    assert gap[0] > 100 and b_ref[0] == 5
    p, b = run_head(gpu, x, gamma, beta, E, 50259)
    assert np.isfinite(p).all() and np.array_equal(b, b_ref)
    assert p[0, 5] == 1.0 and np.delete(p[0], 5).max() == 0.0
    assert np.abs(p.sum(1) - 1).max() < 1e-5
    e = rel_err(p, p_ref)
    print(f"lang head dominant: rel err {e:.3e}")
    assert e <= HEAD_BOUND
    for n in (99, 128, 2):
        x, gamma, beta, E, p_ref, _, _, _ = head_inputs(3, 384, n, 78, kind="equal")
        p, b = run_head(gpu, x, gamma, beta, E, 50259 if n == 99 else 7)
        assert (b == 0).all()
        assert np.abs(p - 1.0 / n).max() <= 1e-7 and (p == p[:, :1]).all()


def test_lang_head_rejects(gpu):
    x = torch.zeros(1, 384, device=gpu)
    emb = torch.zeros(200, 384, dtype=torch.float16, device=gpu)
    out = torch.zeros(129, device=gpu)
    best = torch.zeros(1, dtype=torch.int32, device=gpu)
    for d, lb, n in ((384, 0, 129), (384, 0, 0), (380, 0, 4), (384, -1, 4)):
        with pytest.raises(nat.JanusNativeError, match="lang_head"):
            nat.call("janus_lang_head_f16", x.data_ptr(), x.data_ptr(), x.data_ptr(), emb.data_ptr(), d, lb, n,
                     1, out.data_ptr(), best.data_ptr(), nat.stream_ptr())


# ------------------------------------------------------------------ 2. detect_language
@pytest.fixture(scope="module")
def tiny(gpu):
    W = synthetic_weights(TINY, seed=5)
    return WhisperEngine(TINY, W), W


def lang_enc(cfg, seeds):
    """Random encoder rows at std 4 (beam_ref.rand_enc x 8, exact in fp16): at that scale the
    synthetic models' language winner differs from row to row."""
    return beam_ref.rand_enc(cfg, seeds) * 8.0


@pytest.mark.parametrize("name,wseed", [("tiny", 5), ("small", 3)])
def test_detect_language(gpu, tiny, name, wseed):
    cfg = CONFIGS[name]
    eng, W = tiny if name == "tiny" else (None, synthetic_weights(cfg, seed=wseed))
    eng = eng if eng is not None else WhisperEngine(cfg, W)
    tk = eng.tokenizer
    assert tk.multilingual and tk.sot_sequence == [50258, 50259, 50359]
    enc = beam_ref.rand_enc(cfg, [700, 701, 702])    # std 0.5, the decode tests' encoder rows
    p_ref, b_ref, gap = mr.language_probs(enc, W, cfg, tk)
    assert (gap >= 2e-2).all(), gap                  # seeds picked on the CPU for this
    probs, best = eng.detect_language(torch.from_numpy(enc).half().to(gpu))
    torch.cuda.synchronize()
    assert probs.shape == (3, 99) and best.dtype == torch.int32
    assert np.array_equal(best.cpu().numpy(), b_ref)
    p = probs.cpu().numpy()
    assert np.abs(p.sum(1) - 1).max() < 1e-5
    e = rel_err(p, p_ref)
    print(f"detect_language {name}: rel err {e:.3e}, gaps {np.round(gap, 3)}")
    assert e <= DETECT_BOUND, e
    # three more windows at std 4, where the synthetic models' winner differs from row to row
    # (and the fp16 cross-attention's error grows with the scores: measured 6.9e-3 / 1.0e-1
    # relative on the probabilities there): the winners, whose reference gaps are >= 0.14
    loud = lang_enc(cfg, [700, 701, 702])
    _, b_loud, gap_loud = mr.language_probs(loud, W, cfg, tk)
    assert (gap_loud >= 0.1).all() and len(set(b_loud.tolist())) == 3
    _, best = eng.detect_language(torch.from_numpy(loud).half().to(gpu))
    assert np.array_equal(best.cpu().numpy(), b_loud)


def test_detect_language_chunks_and_leaves_the_slots(gpu, tiny):
    """65 windows (two chunks) equal the per-window calls bit for bit; a call between two
    staggered decode calls leaves state slot 0 as it stood."""
    eng, _ = tiny
    g = torch.Generator().manual_seed(9)
    enc = (torch.randn(65, TINY.n_audio_ctx, TINY.d_model, generator=g) * 4.0).half().to(gpu)
    probs, best = eng.detect_language(enc)
    one = [eng.detect_language(enc[i:i + 1].contiguous()) for i in range(65)]
    assert torch.equal(probs, torch.cat([p for p, _ in one])) and torch.equal(best, torch.cat([b for _, b in one]))
    assert len(set(best.cpu().tolist())) > 3
    ref = eng.decode_ex(enc[:2].contiguous(), max_length=24)
    eng.decode_ex(enc[:2].contiguous(), max_length=24, pos_offset=[0, 0], steps=10)
    eng.detect_language(enc[2:5].contiguous())
    assert eng.decode_stand(2) == [10, 10]
    out = eng.decode_ex(enc[:2].contiguous(), max_length=24, pos_offset=[10, 10], steps=13)
    assert torch.equal(out.tokens, ref.tokens) and torch.equal(out.no_speech_prob, ref.no_speech_prob)
    with pytest.raises(nat.JanusNativeError, match="detect_language"):
        nat.call("janus_whisper_detect_language", eng._h, enc.data_ptr(), 1, 50258, V - 50, 99,
                 probs.data_ptr(), best.data_ptr(), nat.stream_ptr())


# ------------------------------------------------------------------ 3. greedy decode
ML = 24
GREEDY_SEEDS = [724, 725, 722, 723]     # reference margins >= 0.014 in every row (CPU-picked)


def greedy_case(tk):
    de, ja = tk.sot_sequence_for("de", "transcribe"), tk.sot_sequence_for("ja", "translate")
    prompts = [de, [tk.sot_prev, 400, 1200, 3300] + ja, tk.sot_sequence_for("en", "transcribe"),
               [tk.sot_prev, 9000, 262, 770] + de]
    return beam_ref.rand_enc(TINY, GREEDY_SEEDS), prompts


@pytest.fixture(scope="module")
def greedy_ref(tiny):
    eng, W = tiny
    tk = eng.tokenizer
    enc, prompts = greedy_case(tk)
    rows = mr.greedy(enc, W, TINY, tk, prompts, ML)
    at_sot = [mr.no_speech_at(p, len(p) - 3, enc[b], W, TINY, tk) for b, p in enumerate(prompts)]
    at_end = [mr.no_speech_at(p, len(p) - 1, enc[b], W, TINY, tk) for b, p in enumerate(prompts)]
    return rows, at_sot, at_end


def check_tokens(out, ref_rows, prompts, label, max_near_ties=1):
    t, n = out.tokens.cpu().numpy(), out.n_tokens.cpu().numpy()
    near = 0
    for b, r in enumerate(ref_rows):
        pl = len(prompts[b])
        assert list(t[b][:pl]) == list(prompts[b])
        got = t[b][pl:pl + int(n[b])]
        first = mr.first_divergence(got, r["tokens"])
        if first is not None:
            assert r["margins"][first] < NEAR_TIE, (label, b, first, r["margins"][first])
            near += 1
    assert near <= max_near_ties, (label, near)


def test_greedy_decode_and_no_speech_position(gpu, tiny, greedy_ref):
    eng, W = tiny
    tk = eng.tokenizer
    enc_np, prompts = greedy_case(tk)
    rows, at_sot, at_end = greedy_ref
    # the two candidate positions differ by far more than the bound: the test tells them apart
    for a, z in zip(at_sot, at_end):
        assert abs(a - z) > 10 * NSP_REL * a, (a, z)
    enc = torch.from_numpy(enc_np).half().to(gpu)
    out = eng.decode_ex(enc, prompts=prompts, max_length=ML)
    torch.cuda.synchronize()
    check_tokens(out, rows, prompts, "greedy")
    nsp = out.no_speech_prob.cpu().numpy()
    for b, a in enumerate(at_sot):
        print(f"row {b}: no_speech_prob {nsp[b]:.6e}, reference at sot {a:.6e}, at the prompt's end {at_end[b]:.6e}")
        assert abs(nsp[b] - a) <= NSP_REL * a + 1e-12, (b, nsp[b], a)
    # an explicit no_speech_back 0 reads the prompt's last position (the *.en place)
    with pytest.raises(ValueError, match="startoftranscript"):
        eng.decode_ex(enc, prompts=prompts, max_length=ML, no_speech_back=0)
    with pytest.raises(ValueError, match="startoftranscript"):
        eng.decode_ex(enc, prompts=[p[1:] if len(p) == 3 else p for p in prompts], max_length=ML)


def test_decode_forms_agree_bit_for_bit(gpu, tiny):
    """The same rows through a persistent request, a sampled call's T = 0 rows, a staggered
    call and decode_beam(beam_size=1): tokens and no_speech_prob bit-identical."""
    eng, _ = tiny
    enc_np, prompts = greedy_case(eng.tokenizer)
    enc = torch.from_numpy(enc_np).half().to(gpu)
    a = eng.decode_ex(enc, prompts=prompts, max_length=ML)
    assert (a.no_speech_prob > 0).all()

    def same(b, label, rows=slice(None)):
        assert torch.equal(a.tokens, b.tokens[rows]), label
        assert torch.equal(a.no_speech_prob, b.no_speech_prob[rows]), label
    same(eng.decode_ex(enc, prompts=prompts, max_length=ML, persistent=2), "persistent")
    enc5 = torch.cat([enc, enc[:1]])
    same(eng.decode_ex(enc5, prompts=prompts + prompts[:1], max_length=ML, temperature=[0.0] * 4 + [0.7],
                       seeds=[1, 2, 3, 4, 5]), "sampled rows", slice(0, 4))
    eng.decode_ex(enc, prompts=prompts, max_length=ML, pos_offset=[0] * 4, steps=3)
    same(eng.decode_ex(enc, prompts=prompts, max_length=ML, pos_offset=[3] * 4, steps=ML - 1 - 3), "staggered")
    same(eng.decode_beam(enc, prompts=prompts, beam_size=1, max_length=ML), "beam 1")
    # shared encoder rows: two hypotheses per window at T = 0 are the window's greedy row
    b = eng.decode_ex(enc, prompts=[p for p in prompts for _ in range(2)], max_length=ML,
                      temperature=[0.0] * 8, seeds=list(range(8)), enc_index=[0, 0, 1, 1, 2, 2, 3, 3])
    assert torch.equal(a.tokens, b.tokens[0::2]) and torch.equal(a.no_speech_prob, b.no_speech_prob[1::2])


def test_english_default_is_no_speech_back_zero(gpu):
    cfg = CONFIGS["tiny.en"]
    eng = WhisperEngine(cfg, synthetic_weights(cfg, seed=5))
    enc = torch.from_numpy(beam_ref.rand_enc(cfg, [724, 725])).half().to(gpu)
    a = eng.decode_ex(enc, max_length=ML)
    b = eng.decode_ex(enc, max_length=ML, no_speech_back=0)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.no_speech_prob, b.no_speech_prob)
    assert torch.equal(a.sum_logprob, b.sum_logprob) and (a.no_speech_prob > 0).all()
    with pytest.raises(ValueError, match="English-only"):
        eng.detect_language(enc)
    with pytest.raises(ValueError, match="startoftranscript"):
        eng.decode_ex(enc, max_length=ML, no_speech_back=1)


# ------------------------------------------------------------------ 4. the last column
def test_last_vocabulary_column(gpu, tiny):
    """V = 51 865 = 16 * 3241 + 9: the projection's last tile holds 9 columns. With embedding
    row V - 1 set to 8 x the row of the reference's first-step argmax (whose logit is
    positive), reference and GPU both pick V - 1 first and agree afterwards."""
    _, W = tiny
    tk = tok.WhisperTokenizer(multilingual=True)
    enc = beam_ref.rand_enc(TINY, [740])
    prompt = tk.sot_sequence_for("en", "transcribe")
    logits = ow.decoder_logits(np.array([prompt]), enc, W, TINY)[0, -1].numpy()
    L, _ = ow.apply_rules(logits, [], tk, tk.suppress_tokens(), timestamps=False)
    a = int(np.argmax(L))
    assert L[a] > 1.0 and a < V - 1
    W2 = dict(W)
    E = W["decoder.embed_tokens.weight"].copy()
    E[V - 1] = 8 * E[a]
    assert np.array_equal(E.astype(np.float16).astype(np.float32), E)
    W2["decoder.embed_tokens.weight"] = E
    ref = mr.greedy(enc, W2, TINY, tk, [prompt], 16, timestamps=False)
    assert ref[0]["tokens"][0] == V - 1 and ref[0]["margins"][0] > 1.0
    eng = WhisperEngine(TINY, W2)
    out = eng.decode_ex(torch.from_numpy(enc).half().to(gpu), prompts=[prompt], max_length=16, timestamps=False)
    assert int(out.tokens[0, len(prompt)]) == V - 1
    check_tokens(out, ref, [prompt], "last column")


# ------------------------------------------------------------------ 5. beam search
def test_beam_search(gpu, tiny):
    """beam 2 on two multilingual windows against tests/beam_ref.py (generic in the
    tokenizer), seeds picked on the CPU for reference margins >= 2 NEAR_TIE; no_speech_prob
    is the greedy call's, bit for bit."""
    eng, W = tiny
    tk = eng.tokenizer
    enc_np = beam_ref.rand_enc(TINY, [760, 761])
    prompts = [tk.sot_sequence_for("de", "transcribe"),
               [tk.sot_prev, 400, 1200] + tk.sot_sequence_for("fr", "translate")]
    ref = beam_ref.beam_search(enc_np, W, TINY, tk, 2, max_length=14, prompts=prompts)
    assert min(r["min_margin"] for r in ref) >= 2 * NEAR_TIE
    enc = torch.from_numpy(enc_np).half().to(gpu)
    out = eng.decode_beam(enc, prompts=prompts, beam_size=2, max_length=14)
    t, n = out.tokens.cpu().numpy(), out.n_tokens.cpu().numpy()
    for w, r in enumerate(ref):
        pl = len(prompts[w])
        want = [x for x in r["winner"]["tokens"] if x != tk.eot]
        got = [int(x) for x in t[w][pl:pl + int(n[w])] if x != tk.eot]
        assert got == want, (w, got, want)
    g = eng.decode_ex(enc, prompts=prompts, max_length=14)
    assert torch.equal(out.no_speech_prob, g.no_speech_prob) and (g.no_speech_prob > 0).all()


# ------------------------------------------------------------------ 6. end to end
E2E_ML = 32


@pytest.fixture(scope="module")
def model(gpu):
    return tr.WhisperModel("tiny")


def e2e_reference(tk, audio):
    W = synthetic_weights(TINY, seed=0)                      # WhisperModel's weights
    mel = ow.logmel(audio, 1, mel_filters())[None]
    enc = ow.encoder(mel, W, TINY).half().float().numpy()
    p, best, gap = mr.language_probs(enc, W, TINY, tk)
    return W, enc, p[0], tok.LANGUAGES[int(best[0])], float(gap[0])


def test_transcribe_detects_and_translates(gpu, model):
    audio = synth_speech(300, 3.0, sr=16000).astype(np.float32)
    tk = model.engine.tokenizer
    W, enc, p_ref, code, gap = e2e_reference(tk, audio)
    assert gap >= 2e-2 and model.is_multilingual and len(model.supported_languages) == 99
    segs, info = model.transcribe(audio, max_length=E2E_ML, temperature=0.0)
    segs = list(segs)
    assert info.language == code and segs
    print(f"language {code}: probability {info.language_probability:.5f}, reference {p_ref.max():.5f} "
          "(the reference's own front end and encoder)")
    assert len(info.all_language_probs) == 99 and abs(sum(p for _, p in info.all_language_probs) - 1) < 1e-5
    assert info.all_language_probs[0] == (code, info.language_probability)
    assert model.detect_language(audio)[:2] == (code, info.language_probability)
    given, ginfo = model.transcribe(audio, language=code, max_length=E2E_ML, temperature=0.0)
    assert list(given) == segs
    assert (ginfo.language, ginfo.language_probability, ginfo.all_language_probs) == (code, 1.0, None)
    # translate: the reference's tokens for the translate prompt
    for task in ("transcribe", "translate"):
        prompt = tk.sot_sequence_for(code, task)
        ref = mr.greedy(enc, W, TINY, tk, [prompt], E2E_ML)[0]
        st = tr.generate_segments(model.engine, [audio], max_length=E2E_ML, temperatures=(0.0,), language=code,
                                  task=task)[0]
        got, want = st.window_tokens[0], [t for t in ref["tokens"] if t != tk.eot]
        first = mr.first_divergence(got, want)
        print(f"{task}: {len(want)} tokens, first divergence {first}")
        if first is not None:
            assert ref["margins"][first] < NEAR_TIE, (task, first, ref["margins"][first])
    tsegs, _ = model.transcribe(audio, language=code, task="translate", max_length=E2E_ML, temperature=0.0)
    assert [s.tokens for s in tsegs] != [s.tokens for s in segs]
    with pytest.raises(ValueError):
        model.transcribe(audio, language="xx")
    # word timestamps: words for every segment, from the three-token start sequence
    wsegs, _ = model.transcribe(audio, language=code, max_length=E2E_ML, temperature=0.0, word_timestamps=True)
    wsegs = list(wsegs)
    assert wsegs and all(s.words for s in wsegs)
    assert all(w.end >= w.start >= 0.0 and 0.0 <= w.probability <= 1.0 for s in wsegs for w in s.words)


def test_english_model_default_language(gpu):
    audio = synth_speech(300, 3.0, sr=16000).astype(np.float32)
    m = tr.WhisperModel("tiny.en")
    a, ia = m.transcribe(audio, max_length=E2E_ML, temperature=0.0)
    b, ib = m.transcribe(audio, language="en", max_length=E2E_ML, temperature=0.0)
    a, b = list(a), list(b)
    assert a == b and a and ia == ib
    assert (ia.language, ia.language_probability, ia.all_language_probs) == ("en", 1.0, None)
    with pytest.raises(NotImplementedError, match="English only"):
        m.transcribe(audio, task="translate")
