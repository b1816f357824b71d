"""The 768-wide, 12-head family (small.en, distil-small.en) on the GPU, against the oracle
(oracle/whisper.py) and against itself. Shapes: ``small-cut`` — the real width and heads,
distil's 4 decoder layers, 2 encoder layers — except where depth is the point. Tolerances
are the project's: ENC_TOL (encoder, relative RMS) and NEAR_TIE (a free-running decode may
leave the oracle's only where the oracle's own top-2 margin is below it).

Oracle margins on the free-running rows (CPU, its own encoder output rounded to fp16, 127
steps): rows k in ROWS8 >= 1.8e-2; row k = 1 (the 9 s clip) 6.3e-4 with two sub-NEAR_TIE
steps — it rides along as a witness of the near-tie rule only."""
import numpy as np
import pytest
import torch

from janus_amd.whisper import (CONFIGS, DEC_PATH_NO_CVP, DEC_PATH_NO_EMBED_LN, DEC_PATH_NO_XPAIR,
                               DEC_PATH_XGROUP, WhisperConfig, WhisperEngine, dec_path_ln_mask,
                               dec_path_xrows, mel_filters, synthetic_weights)
from janus_amd.workload import synth_speech
from oracle import packet as opk
from oracle import whisper as ow
from oracle.prosody import OracleProsody

pytestmark = pytest.mark.gpu
CUT = WhisperConfig("small-cut", 768, 12, 2, 4)
NEAR_TIE = 2e-3
ENC_TOL = 1e-3
SECS = [30.0, 9.0, 3.0, 0.3, 17.0, 24.0, 12.0, 1.0, 6.0, 21.0, 4.5, 15.0]
ROWS8 = [0, 2, 3, 4, 6, 7, 9, 11]
WITNESS = 1
ML = 128


def pack(utts, dev):
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    return pcm, offs


def encode_clips(eng, utts, dev):
    pcm, offs = pack(utts, dev)
    return eng.encode(eng.logmel(pcm, offs, len(utts), 3))


@pytest.fixture(scope="module")
def cut(gpu):
    W = synthetic_weights(CUT, seed=11)
    return WhisperEngine(CUT, W), W


@pytest.fixture(scope="module")
def enc9(cut, gpu):
    """Engine encoder output of the eight free-running rows and the witness row (last)."""
    eng, _ = cut
    enc = encode_clips(eng, [synth_speech(300 + k, SECS[k]) for k in ROWS8 + [WITNESS]], gpu)
    torch.cuda.synchronize()
    return enc


@pytest.fixture(scope="module")
def oracle9(cut, enc9):
    """The oracle's greedy decode of enc9 to ML tokens, computed once for the module."""
    eng, W = cut
    return ow.greedy_cached(enc9.float().cpu(), W, CUT, eng.tokenizer, ML, no_speech=50361)


@pytest.fixture(scope="module")
def small_tr(gpu):
    from janus_amd.services.transcriber import Transcriber
    return Transcriber("small.en")


# ------------------------------------------------------------------ 2. encoder
def _enc_err(got, ref):
    got = got.float().cpu()
    rel = float((got - ref).norm() / ref.norm())
    per_row = ((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    return rel, per_row


def test_encoder_small_cut(cut, gpu):
    eng, W = cut
    pcm, offs = pack([synth_speech(300, 30.0), synth_speech(301, 9.0)], gpu)
    mel = eng.logmel(pcm, offs, 2, 3)
    enc = eng.encode(mel)
    torch.cuda.synchronize()
    rel, per_row = _enc_err(enc, ow.encoder(mel.float().cpu().numpy(), W, CUT))
    print(f"small-cut: encoder rel RMS {rel:.2e}, worst row {per_row:.2e}")
    assert rel < ENC_TOL and per_row < 4 * ENC_TOL, (rel, per_row)


def test_encoder_small_en_full_depth(small_tr, gpu):
    """12 encoder layers at d = 768 against the fp32 oracle, one 30 s clip, the bound of the
    4- and 6-layer models (ENC_TOL 1e-3 relative RMS, worst row 4e-3; tiny.en measured
    3.9e-4, base.en 4.2e-4). Measured on an MI355X: 3.6e-4, worst row 4.0e-4 (the 2-layer
    small-cut case above: 3.7e-4 / 4.4e-4) — the error does not grow with depth."""
    eng = small_tr.model.engine
    cfg = CONFIGS["small.en"]
    W = synthetic_weights(cfg, seed=0)
    pcm, offs = pack([synth_speech(300, 30.0)], gpu)
    mel = eng.logmel(pcm, offs, 1, 3)
    enc = eng.encode(mel)
    torch.cuda.synchronize()
    rel, per_row = _enc_err(enc, ow.encoder(mel.float().cpu().numpy(), W, cfg))
    print(f"small.en: encoder rel RMS {rel:.2e}, worst row {per_row:.2e}")
    assert rel < ENC_TOL and per_row < 4 * ENC_TOL, (rel, per_row)


# ------------------------------------------------------------------ 3. free-running decode
def _first_diff(g, rt):
    return next((i for i in range(min(len(g), len(rt))) if g[i] != rt[i]), min(len(g), len(rt)))


def test_free_running_decode_small_cut(cut, enc9, oracle9, gpu):
    """Eight rows (and the witness) free-running to 128 tokens against the oracle on the same
    encoder output: per row identical, or first divergence at an oracle margin < NEAR_TIE;
    at least 7 of the 8 identical; the gate inputs as test_free_running_decode_base. Then 65
    rows (the eight repeated): past the 64-row group of the vocabulary projection and the
    skinny GEMMs' row split, its first eight rows equal the 8-row call exactly."""
    eng, _ = cut
    tk = eng.tokenizer
    plen = len(tk.sot_sequence)
    dec = eng.decode_ex(enc9, max_length=ML)
    torch.cuda.synchronize()
    assert eng.decode_path().enc_rows == "own" and eng.decode_path().persistent == 0
    toks, nt = dec.tokens.cpu().numpy(), dec.n_tokens.cpu().numpy()
    slp, nsp = dec.sum_logprob.cpu().numpy(), dec.no_speech_prob.cpu().numpy()
    same = 0
    for b, r in enumerate(oracle9):
        g = [int(t) for t in toks[b][plen:plen + int(nt[b])]]
        print(f"row {b}: {len(g)} tokens, oracle min margin {min(r['margins']):.2e}, "
              f"identical {g == r['tokens']}")
        assert abs(nsp[b] - r["nsp"]) <= 5e-3 * r["nsp"] + 1e-12, (b, nsp[b], r["nsp"])
        if g == r["tokens"]:
            same += b < 8
            assert abs(slp[b] - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]), (b, slp[b], r["sum_lp"])
        else:
            first = _first_diff(g, r["tokens"])
            margin = r["margins"][first] if first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE, (b, first, margin)
    assert same >= 7, same
    enc8 = enc9[:8]
    d8 = eng.decode_ex(enc8, max_length=ML)
    big = torch.cat([enc8] * 8 + [enc8[:1]])
    assert big.shape[0] == 65
    d65 = eng.decode_ex(big, max_length=ML)
    torch.cuda.synchronize()
    for f in ("tokens", "n_tokens", "sum_logprob", "no_speech_prob"):
        a, b65 = getattr(d8, f).cpu(), getattr(d65, f).cpu()
        assert torch.equal(a, getattr(dec, f).cpu()[:8]), f
        assert torch.equal(b65[:8], a) and torch.equal(b65[56:64], a) and torch.equal(b65[64:], a[:1]), f


# ------------------------------------------------------------------ 4. sampled decode
SAMPLE_SEEDS = [2026, 2169, 2273, 2299, 3092, 2390, 2403, 2416, 2520, 2546]


def test_sampled_decode_matches_oracle_small_cut(cut, gpu):
    """Two windows (the 30 s and the 3 s clip) x best_of 5 at T = 0.6, max_length 40, rows
    sharing their window's encoder output in place (four-row blocks: 4 + 1), against the
    oracle's sampler with the same seeds:
    identical, or first divergence at a key margin < NEAR_TIE / T; at most one of ten rows
    diverges. Seeds chosen on the CPU oracle alone so that no row has a key margin under
    10 x NEAR_TIE / T = 3.3e-2: window 0 seeds 2026, 2169, 2273, 2299, 3092 (smallest
    margins 4.5e-2, 5.2e-2, 5.6e-2, 8.7e-2, 6.7e-2), window 1 seeds 2390, 2403, 2416, 2520,
    2546 (1.5e-1, 5.5e-2, 5.1e-2, 2.2e-1, 7.3e-2)."""
    eng, W = cut
    T, ml = 0.6, 40
    enc = encode_clips(eng, [synth_speech(300, 30.0), synth_speech(302, 3.0)], gpu)
    ei = [0] * 5 + [1] * 5
    out = eng.decode_ex(enc, max_length=ml, temperature=T, seeds=SAMPLE_SEEDS, enc_index=ei,
                        path_flags=dec_path_xrows(4))
    torch.cuda.synchronize()
    assert eng.decode_path().enc_rows == "in_place"
    rows, toks = out.rows(), out.tokens.cpu().numpy()
    rep = enc.index_select(0, torch.tensor(ei, device=gpu)).float().cpu()
    ref = ow.greedy_cached(rep, W, CUT, eng.tokenizer, ml, no_speech=50361, temperature=T,
                           seeds=SAMPLE_SEEDS)
    plen = len(eng.tokenizer.sot_sequence)
    same = 0
    for b, r in enumerate(ref):
        g = [int(t) for t in toks[b][plen:plen + int(out.n_tokens[b])]]
        print(f"row {b}: oracle min key margin {min(r['margins']):.2e}, identical {g == r['tokens']}")
        if g == r["tokens"]:
            same += 1
            assert abs(float(out.sum_logprob[b]) - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]) + 1e-3
        else:
            first = _first_diff(g, r["tokens"])
            margin = r["margins"][first] if first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE / T, (b, first, margin)
        assert abs(rows[b][2] - r["nsp"]) <= 5e-3 * max(r["nsp"], 1e-6) + 1e-7
    assert same >= len(ref) - 1, same


# ------------------------------------------------------------------ 5. shared = replicated
@pytest.fixture(scope="module")
def enc3(cut, gpu):
    eng, _ = cut
    enc = encode_clips(eng, [synth_speech(70 + k, 2.0 + k) for k in range(3)], gpu)
    torch.cuda.synchronize()
    return enc


def _same_out(a, b):
    for f in ("tokens", "n_tokens", "sum_logprob", "no_speech_prob"):
        assert torch.equal(getattr(a, f).cpu(), getattr(b, f).cpu()), f


@pytest.mark.parametrize("T", [0.0, 0.6])
@pytest.mark.parametrize("idx", [[0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2], [0, 1, 1, 2, 2, 2, 2]],
                         ids=["five", "odd"])
@pytest.mark.parametrize("block", [4, 2])
def test_shared_encoder_rows_match_replicated_768(cut, enc3, gpu, T, idx, block):
    """Rows sharing an encoder row (enc_index) at 12 heads, read in place with
    DEC_PATH_XROWS(n) — blocks of up to n = 4 or 2 rows per (encoder row, key split),
    xattn_rows_kernel: 4 + 1 or 2 + 2 + 1 for best_of 5, odd groups, a lone row — decode
    bit-identically to a private copy per row, also above 64 rows. The path report must say
    "in place": a silent gather copy would pass the comparison. Without the flag (this
    family's measured default) and with DEC_PATH_NO_XPAIR the same call gathers, and still
    decodes the same bits."""
    eng, _ = cut
    for reps in (1, 10):
        ei = idx * reps
        seeds = [1000 + i for i in range(len(ei))] if T > 0 else None
        rep = enc3.index_select(0, torch.tensor(ei, device=gpu)).contiguous()
        a = eng.decode_ex(rep, max_length=40, temperature=T, seeds=seeds)
        assert eng.decode_path().enc_rows == "own"
        b = eng.decode_ex(enc3, max_length=40, temperature=T, seeds=seeds, enc_index=ei,
                          path_flags=dec_path_xrows(block))
        assert eng.decode_path().enc_rows == "in_place"
        torch.cuda.synchronize()
        _same_out(a, b)
        if reps == 1:
            first = b.tokens.cpu()
            for flags in (0, DEC_PATH_NO_XPAIR, DEC_PATH_NO_XPAIR | dec_path_xrows(block)):
                c = eng.decode_ex(enc3, max_length=40, temperature=T, seeds=seeds, enc_index=ei,
                                  path_flags=flags)
                assert eng.decode_path().enc_rows == "gathered"
                _same_out(a, c)
        else:
            assert torch.equal(b.tokens.cpu()[:len(idx)], first)


@pytest.mark.parametrize("idx", [[0, 1, 2], [0, 0, 1, 2, 2], [1, 1, 1, 0]], ids=["lone", "two", "three"])
def test_shared_rows_small_groups_768(cut, enc3, gpu, idx):
    """The one-, two- and three-m-tile instantiations on their own: calls whose largest group
    has one row, two rows, three rows (in blocks of up to four)."""
    eng, _ = cut
    rep = enc3.index_select(0, torch.tensor(idx, device=gpu)).contiguous()
    a = eng.decode_ex(rep, max_length=40)
    b = eng.decode_ex(enc3, max_length=40, enc_index=idx, path_flags=dec_path_xrows(4))
    assert eng.decode_path().enc_rows == "in_place"
    torch.cuda.synchronize()
    _same_out(a, b)


def test_xrows_flag_names_its_limit(gpu):
    """DEC_PATH_XROWS is the 12-head family's: on tiny.en the call is refused by name."""
    from janus_amd import _native as nat
    cfg = WhisperConfig("tiny-cut", 384, 6, 1, 1)
    eng = WhisperEngine(cfg, synthetic_weights(cfg, seed=2))
    enc = torch.zeros(1, cfg.n_audio_ctx, cfg.d_model, dtype=torch.float16, device=gpu)
    with pytest.raises(nat.JanusNativeError, match="XROWS"):
        eng.decode_ex(enc, max_length=8, enc_index=[0, 0], path_flags=dec_path_xrows(2))


def test_xgroup_flag_names_its_limit_768(cut, enc3, gpu):
    from janus_amd import _native as nat
    eng, _ = cut
    with pytest.raises(nat.JanusNativeError, match="H <= 8"):
        eng.decode_ex(enc3, max_length=16, enc_index=[0, 0, 0, 1], path_flags=DEC_PATH_XGROUP)


# ------------------------------------------------------------------ 6. staggered rows
def test_staggered_decode_matches_full_768(cut, gpu):
    """test_staggered_decode_matches_full at L = 40 on small-cut, with the persistent
    segments requested (ServingTuning's default): they are 512-only, so the calls take the
    launch path silently (path report: no persistent segments) and every set equals its own
    full decode bit for bit."""
    eng, _ = cut
    L = 40
    N, S = 3, L // 2
    batches = [encode_clips(eng, [synth_speech(300 + 10 * k + j, 1.5 + j) for j in range(N)], gpu)
               for k in range(3)]
    ref = [eng.decode_ex(e, max_length=L, persistent=2) for e in batches]
    assert eng.decode_path().persistent == 0
    sets = [None, None]
    got = {}
    for call in range(4):
        fresh = call % 2
        cont = 1 - fresh
        sets[fresh] = call if call < 3 else None
        rows_enc, offs = [], []
        for st in (0, 1):
            bi = sets[st]
            if bi is None:
                rows_enc.append(torch.zeros_like(batches[0]))
                offs += [L - S] * N if st == cont or call == 3 else [0] * N
            else:
                rows_enc.append(batches[bi])
                offs += [0 if st == fresh else S] * N
        if call == 0:
            offs = [0] * (2 * N)
        out = eng.decode_ex(torch.cat(rows_enc), max_length=L, pos_offset=offs, steps=S, persistent=2)
        p = eng.decode_path()
        assert p.persistent == 0 and p.enc_rows == "own"
        if call > 0 and sets[cont] is not None:
            bi = sets[cont]
            sl = slice(cont * N, cont * N + N)
            got[bi] = (out.tokens[sl].cpu(), out.n_tokens[sl].cpu(), out.sum_logprob[sl].cpu(),
                       out.no_speech_prob[sl].cpu())
            sets[cont] = None
    torch.cuda.synchronize()
    assert sorted(got) == [0, 1, 2]
    plen = len(eng.tokenizer.sot_sequence)
    for bi, r in enumerate(ref):
        t, n, lp, ns = got[bi]
        assert torch.equal(n, r.n_tokens.cpu()) and torch.equal(lp, r.sum_logprob.cpu())
        assert torch.equal(ns, r.no_speech_prob.cpu())
        rt = r.tokens.cpu()
        for j in range(N):
            k = plen + int(n[j])
            assert torch.equal(t[j, :k], rt[j, :k]), (bi, j)
        assert int(n.min()) >= min(16, L - plen - 1)


# ------------------------------------------------------------------ 7. seek loop + fallback
def test_seek_loop_matches_oracle_768(cut, gpu):
    """generate_segments on small-cut at max_length 64 with the temperature fallback against
    the oracle's restatement (a 35 s clip, so a second window runs, and a 3 s one): windows,
    segments, texts, counters; sequential and speculative=True identical to each other."""
    from janus_amd.services.transcriber import TEMPERATURES, generate_segments
    eng, W = cut
    auds = [synth_speech(160, 35.0, sr=16000), synth_speech(161, 3.0, sr=16000)]
    streams = generate_segments(eng, auds, max_length=64, temperatures=TEMPERATURES)
    assert eng.decode_path().enc_rows == "gathered"      # the last call: a sampled re-decode
    spec = generate_segments(eng, auds, max_length=64, temperatures=TEMPERATURES, speculative=True)
    assert eng.decode_path().enc_rows == "gathered"
    tk = eng.tokenizer
    assert streams[0].windows >= 2
    for i, (a, st, sp) in enumerate(zip(auds, streams, spec)):
        ref, cnt = ow.transcribe_segments(a, W, CUT, tk, mel_filters(), max_length=64,
                                          temperatures=TEMPERATURES, utt=i)
        got = [(s.start, s.end, s.text, list(s.tokens)) for s in st.segments]
        assert st.windows == cnt["windows"] and st.fallbacks == cnt["needs_fallback"] and st.skips == cnt["skips"]
        assert st.fallback_decodes == cnt["fallback_decodes"]
        assert [g[3] for g in got] == [r[3] for r in ref]
        assert [g[2] for g in got] == [r[2] for r in ref]
        assert np.allclose([g[:2] for g in got], [r[:2] for r in ref])
        assert [(s.start, s.end, s.text, list(s.tokens), s.temperature) for s in st.segments] == \
            [(s.start, s.end, s.text, list(s.tokens), s.temperature) for s in sp.segments]
        assert (st.windows, st.fallbacks, st.skips, st.fallback_decodes, st.sampled) == \
            (sp.windows, sp.fallbacks, sp.skips, sp.fallback_decodes, sp.sampled)
        assert st.window_tokens == sp.window_tokens and st.window_rows == sp.window_rows


# ------------------------------------------------------------------ 8. pipeline, drop-in
def test_pipeline_distil_small(gpu):
    """JanusPipeline(model='distil-small.en') on three 5 s clips: the packets of the
    back-to-back step are generate_segments' transcripts through the oracle packer with the
    oracle's prosody tags, and step_staggered() gives the same packets, seek loops, tokens
    and waveforms bit for bit (its persistent decoder request falls back to launches)."""
    from janus_amd.pipeline import JanusPipeline
    from janus_amd.services.transcriber import generate_segments
    pipe = JanusPipeline(model="distil-small.en", max_length=24, temperatures=(0.0,))
    utts = [synth_speech(810 + k, 5.0) for k in range(3)]
    lengths = [len(u) for u in utts]
    pcm, offs = pack(utts, gpu)
    frames = 16
    ref = pipe.encode(pcm, offs, lengths, timestamp=5.0)
    wav0, pcm0, _ = pipe.decode(ref.packets, frames)
    segs = generate_segments(pipe.whisper, [np.ascontiguousarray(u[::3]) for u in utts],
                             max_length=24, temperatures=(0.0,))
    for b, (u, st) in enumerate(zip(utts, segs)):
        text = st.transcript()
        tags = OracleProsody(48000).analyze_buffer(u)[0]
        assert ref.texts[b] == text and ref.tags[b] == tags
        assert ref.packets[b] == (opk.serialize(text, 0, tags, "auto", 5.0) if text.strip() else None)
    assert any(p is not None for p in ref.packets)
    res, wav, pcm16 = pipe.step(pcm, offs, lengths, frames)
    assert res.texts == ref.texts
    outs = [pipe.step_staggered(pcm, offs, lengths, frames, 16, timestamp=5.0) for _ in range(2)]
    done = [o for o in outs if o[0] is not None] + pipe.flush_staggered(frames)
    assert pipe.whisper.decode_path().persistent == 0
    assert len(done) == 2
    for res, wav, pcm16 in done:
        assert res.packets == ref.packets
        assert torch.equal(res.n_tokens, ref.n_tokens)
        for j in range(len(res.n_tokens)):
            k = 1 + int(res.n_tokens[j])
            assert torch.equal(res.tokens[j, :k], ref.tokens[j, :k])
        if wav0 is None:
            assert wav is None
        else:
            assert torch.equal(wav, wav0) and torch.equal(pcm16, pcm0)


def test_transcriber_small_en_full_depth(small_tr, gpu):
    """Transcriber('small.en') (12 decoder layers) transcribes a 2 s buffer: the drop-in call
    with its default temperature fallback; transcribe_batch agrees with it."""
    x = synth_speech(5, 2.0)
    t = small_tr.transcribe_buffer(x)
    assert isinstance(t, str)
    assert small_tr.model.stats["windows"] >= 1
    assert small_tr.transcribe_batch([x]) == [t]
    p = small_tr.model.engine.decode_path()
    assert p.persistent == 0


# ------------------------------------------------------------------ 9. fusions off at 768
@pytest.mark.parametrize("flags", [DEC_PATH_NO_CVP, DEC_PATH_NO_EMBED_LN, dec_path_ln_mask(15),
                                   dec_path_ln_mask(0)], ids=["no_cvp", "no_embed_ln", "mask15", "mask0"])
def test_launch_path_fusions_fall_back_silently_768(cut, enc9, gpu, flags):
    """The launch-path fusions that have no 768 form are off at this width
    whatever the flags ask for: every flag decodes the default's bits on the free-running
    rows, none raises."""
    eng, _ = cut
    a = eng.decode_ex(enc9[:8], max_length=40)
    b = eng.decode_ex(enc9[:8], max_length=40, path_flags=flags)
    torch.cuda.synchronize()
    _same_out(a, b)
