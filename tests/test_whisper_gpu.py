"""GPU parity of the STT path (janus_whisper_*) against the oracle (oracle/whisper.py,
pinned to transformers), on tiny.en and base.en (the bench model, config 3):

* log-mel within 2e-3 (fp16 output);
* encoder within 1e-3 relative RMS of the fp32 oracle (measured 3.9e-4 tiny / 4.2e-4
  base: fp16 MFMA operands, fp32 accumulation, weights fp16-exact for both sides);
* FREE-RUNNING greedy decode to the full 448-token context against the KV-cached fp32
  oracle decoder on the same encoder output, and end to end from the same PCM through
  the oracle's own front end and encoder: token sequences (and the MessagePack packets
  built from them) must be identical, except where the oracle itself is at a near-tie —
  a first divergence is allowed only at a step whose rule-filtered top-2 logit margin is
  below NEAR_TIE. Measured (tools/decode_parity.py, profiles/r02_decode_parity.json):
  base.en 8/8 sequences identical at 447 tokens (decoder-only and end to end), tiny.en
  15/16 (the 16th diverges at step 7, oracle margin 1.2e-4; r02 v44 build), 16/16 end to end.
"""
import numpy as np
import pytest
import torch

from janus_amd.whisper import (CONFIGS, DEC_PATH_NO_CVP, DEC_PATH_NO_SEL_EMBED, DEC_PATH_RESID_LN,
                               DEC_PATH_XGROUP, WhisperEngine, dec_path_ln_mask, engine_weights,
                               mel_filters, synthetic_weights)
from janus_amd.workload import synth_speech
from oracle import packet as opk
from oracle import whisper as ow

pytestmark = pytest.mark.gpu
CFG = CONFIGS["tiny.en"]
BASE = CONFIGS["base.en"]
NEAR_TIE = 2e-3   # logit units: fp16-operand decoding may only flip a choice this close
ENC_TOL = 1e-3    # relative RMS of the encoder output vs fp32


@pytest.fixture(scope="module")
def engine(gpu):
    W = synthetic_weights(CFG, seed=5)
    return WhisperEngine(CFG, W), W


@pytest.fixture(scope="module")
def base_engine(gpu):
    W = synthetic_weights(BASE, seed=7)
    return WhisperEngine(BASE, W), W


def pack(utts, dev):
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    return pcm, offs


def test_logmel(engine, gpu):
    eng, _ = engine
    utts = [synth_speech(20, 30.0), synth_speech(21, 7.3), synth_speech(22, 0.05), synth_speech(23, 12.0)]
    pcm, offs = pack(utts, gpu)
    mel = eng.logmel(pcm, offs, len(utts), 3)
    torch.cuda.synchronize()
    filt = mel_filters()
    for b, u in enumerate(utts):
        ref = ow.logmel(u, 3, filt)
        got = mel[b].float().cpu().numpy()
        err = np.abs(got - ref).max()
        assert err < 2e-3, (b, err)


def test_whole_clip_features(engine, gpu):
    """faster-whisper's features for the seek loop (janus_whisper_logmel_frames): one
    log-mel of the whole clip normalised over all of its frames (here a 47 s clip whose loud
    part lies beyond the first 30 s, so the first window's clamp differs from a per-window
    log-mel), 0.0 from the content end on; and the single-window call pads with zeros."""
    eng, _ = engine
    x = np.concatenate([0.05 * synth_speech(40, 30.0, sr=16000), synth_speech(41, 17.0, sr=16000)])
    x = x.astype(np.float32)
    c = len(x) // 160
    pcm, offs = pack([x], gpu)
    full = eng.logmel_frames(pcm, offs, 1, 1, c + 7)
    torch.cuda.synchronize()
    ref = ow.logmel(x, 1, mel_filters(), n_frames=None)
    got = full[0].float().cpu().numpy()
    assert np.abs(got[:c] - ref).max() < 2e-3
    assert not got[c:].any()
    win0 = ow.logmel(x[:480000], 1, mel_filters())           # per-window scope: different
    assert np.abs(ow.window(ref, 0) - win0).max() > 0.05
    short = synth_speech(42, 3.3, sr=16000)
    pcm2, offs2 = pack([short], gpu)
    m = eng.logmel(pcm2, offs2, 1, 1)[0].float().cpu().numpy()
    cs = len(short) // 160
    assert not m[cs:].any() and np.abs(m[:cs] - ow.logmel(short, 1, mel_filters())[:cs]).max() < 2e-3


@pytest.mark.parametrize("which", ["tiny.en", "base.en"])
def test_encoder(engine, base_engine, gpu, which):
    eng, W = engine if which == "tiny.en" else base_engine
    cfg = CFG if which == "tiny.en" else BASE
    utts = [synth_speech(30, 30.0), synth_speech(31, 9.0)]
    pcm, offs = pack(utts, gpu)
    mel = eng.logmel(pcm, offs, 2, 3)
    enc = eng.encode(mel)
    torch.cuda.synchronize()
    ref = ow.encoder(mel.float().cpu().numpy(), W, cfg)
    got = enc.float().cpu()
    rel = float((got - ref).norm() / ref.norm())
    per_row = ((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()  # no bad head/tile
    print(f"{which}: encoder rel RMS {rel:.2e}, worst row {per_row:.2e}")
    assert rel < ENC_TOL, rel
    assert per_row < 4 * ENC_TOL, per_row


def _check_free_running(gpu_rows, ref_rows, tk, plen, ntok):
    """-> (sequence identity rate, packet identity rate); asserts the near-tie bound."""
    tags = {"energy": "Normal", "pitch": "High"}
    seq = pk = 0
    for b, r in enumerate(ref_rows):
        g = [int(t) for t in gpu_rows[b][plen:plen + int(ntok[b])]]
        rt = r["tokens"]
        if g == rt:
            seq += 1
        else:
            first = next((i for i in range(min(len(g), len(rt))) if g[i] != rt[i]), min(len(g), len(rt)))
            margin = r["margins"][first] if first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE, (b, first, margin, g[first:first + 3], rt[first:first + 3])
        pk += opk.serialize(tk.transcript(g), 0, tags, "auto", 1.0) == \
            opk.serialize(tk.transcript(rt), 0, tags, "auto", 1.0)
    return seq / len(ref_rows), pk / len(ref_rows)


def test_free_running_decode_base(base_engine, gpu):
    """base.en, 8 utterances (30 s .. 0.3 s), free-running to the 448-token context
    (synthetic weights never emit eot: 447 sampled tokens each), vs the oracle decoder on
    the same encoder output (transcriber.py:53-64 -> greedy, beam_size=1)."""
    eng, W = base_engine
    secs = [30.0, 17.0, 8.0, 3.0, 1.0, 0.3, 24.0, 12.0]
    utts = [synth_speech(140 + k, s) for k, s in enumerate(secs)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    dec = eng.decode_ex(enc, max_length=448)
    torch.cuda.synchronize()
    tk = eng.tokenizer
    nt = dec.n_tokens.cpu().numpy()
    assert (nt >= 128).all()
    ref = ow.greedy_cached(enc.float().cpu(), W, BASE, tk, 448, no_speech=50361)
    seq, pk = _check_free_running(dec.tokens.cpu().numpy(), ref, tk, len(tk.sot_sequence), nt)
    print(f"base.en free-running: sequences identical {seq:.3f}, packets identical {pk:.3f}")
    assert seq >= 0.75 and pk >= 0.75
    # the gate inputs: sum of chosen log-probs and the no-speech probability
    slp, nsp = dec.sum_logprob.cpu().numpy(), dec.no_speech_prob.cpu().numpy()
    for b, r in enumerate(ref):
        assert abs(nsp[b] - r["nsp"]) <= 5e-3 * r["nsp"] + 1e-12, (b, nsp[b], r["nsp"])
        if dec.tokens[b].tolist()[1:1 + len(r["tokens"])] == r["tokens"]:
            assert abs(slp[b] - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]), (b, slp[b], r["sum_lp"])


def test_free_running_end_to_end_tiny(engine, gpu):
    """PCM -> tokens: the GPU path vs the oracle's own log-mel + fp32 encoder (output
    stored fp16, as the engine hands it to the decoder) + oracle greedy decoder."""
    eng, W = engine
    utts = [synth_speech(150 + k, s) for k, s in enumerate([30.0, 11.0, 4.0, 1.5])]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    tokens, ntok, _ = eng.decode(enc, max_length=448)
    torch.cuda.synchronize()
    mels = np.stack([ow.logmel(u, 3, mel_filters()) for u in utts])
    enc_ref = ow.encoder(mels, W, CFG)
    tk = eng.tokenizer
    ref = ow.greedy_cached(enc_ref.half().float(), W, CFG, tk, 448)
    seq, pk = _check_free_running(tokens.cpu().numpy(), ref, tk, len(tk.sot_sequence), ntok.cpu().numpy())
    print(f"tiny.en end to end: sequences identical {seq:.3f}, packets identical {pk:.3f}")
    assert seq >= 0.75 and pk >= 0.75


def test_weight_reupload_after_decode(gpu):
    """A parameter re-uploaded after a decode (janus_whisper_set_tensor) is what the next
    decode uses: no captured graph may keep pointing at the freed weight memory. The
    re-uploaded context must decode exactly as a fresh one built with the new weights."""
    W = synthetic_weights(CFG, seed=11)
    eng = WhisperEngine(CFG, W)
    g = torch.Generator().manual_seed(3)
    enc = (torch.randn(3, CFG.n_audio_ctx, CFG.d_model, generator=g) * 0.5).half().to(gpu)
    t1, n1, _ = eng.decode(enc, max_length=40)
    name = "decoder.layers.0.fc1.weight"
    W2 = dict(W)
    W2[name] = engine_weights({name: -1.5 * W[name]})[name]
    eng.set_tensor(name, W2[name])
    t2, n2, _ = eng.decode(enc, max_length=40)
    fresh = WhisperEngine(CFG, W2)
    t3, n3, _ = fresh.decode(enc, max_length=40)
    torch.cuda.synchronize()
    assert torch.equal(n2, n3) and all(torch.equal(t2[b, :n2[b]], t3[b, :n3[b]]) for b in range(3))
    assert not (torch.equal(n1, n2) and all(torch.equal(t1[b, :n1[b]], t2[b, :n2[b]]) for b in range(3)))


@pytest.mark.parametrize("T", [0.0, 0.6])
@pytest.mark.parametrize("idx", [[0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, 1, 0], [0, 0, 1, 2, 2, 1, 0]],
                         ids=["five", "two"])
@pytest.mark.parametrize("xgroup", [0, DEC_PATH_XGROUP], ids=["pairs", "groups"])
def test_shared_encoder_rows_match_replicated(engine, gpu, T, idx, xgroup):
    """Decoder rows sharing an encoder output (enc_index: faster-whisper's best_of
    hypotheses of one window) decode exactly as with a private copy per row: the
    cross-attention reads it once per PAIR of rows (default), or with DEC_PATH_XGROUP and
    more than two rows per window once per GROUP of up to 6 (xattn_group_kernel);
    including a batch above 64 rows (the skinny GEMMs split the rows over blocks). Tokens,
    summed log-probabilities and no-speech probabilities bit-identical."""
    eng, _ = engine
    utts = [synth_speech(70 + k, 2.0 + k) for k in range(3)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    for reps in (1, 10):                                       # then > 64 rows
        ei = idx * reps
        seeds = [1000 + i for i in range(len(ei))] if T > 0 else None
        rep = enc.index_select(0, torch.tensor(ei, device=gpu)).contiguous()
        a = eng.decode_ex(rep, max_length=40, temperature=T, seeds=seeds)
        b = eng.decode_ex(enc, max_length=40, temperature=T, seeds=seeds, enc_index=ei,
                          path_flags=xgroup)
        torch.cuda.synchronize()
        assert torch.equal(a.tokens.cpu(), b.tokens.cpu())
        assert torch.equal(a.n_tokens.cpu(), b.n_tokens.cpu())
        assert torch.equal(a.sum_logprob.cpu(), b.sum_logprob.cpu())
        assert torch.equal(a.no_speech_prob.cpu(), b.no_speech_prob.cpu())
        # rows are independent of the batch they ride in: the 84-row decode repeats the
        # 14-row one
        if reps == 1:
            first = b.tokens.cpu()
        else:
            assert torch.equal(b.tokens.cpu()[:len(idx)], first)


@pytest.mark.parametrize("L", [40, 448])
def test_staggered_decode_matches_full(engine, gpu, L):
    """Continuous batching across decode calls (janus_decode_rows.pos_offset): two row sets
    share one context, each call runs S = L / 2 positions; a set starts fresh in one call
    and continues (offset S, its KV cache / tokens / rule state kept in its slots) in the
    next, while the other set does the opposite. Every batch's tokens, summed
    log-probabilities and no-speech probabilities equal a single full decode of that batch
    alone: rows are independent of their neighbours' positions."""
    eng, _ = engine
    N, S = 3, L // 2
    batches = []
    for k in range(3):
        utts = [synth_speech(300 + 10 * k + j, 1.5 + j) for j in range(N)]
        pcm, offs = pack(utts, gpu)
        batches.append(eng.encode(eng.logmel(pcm, offs, N, 3)))
    ref = [eng.decode_ex(e, max_length=L) for e in batches]
    sets = [None, None]          # slot set -> batch index in it
    got = {}
    for call in range(4):
        fresh = call % 2         # slot set taking a new batch this call
        cont = 1 - fresh
        if call < 3:
            sets[fresh] = call
        else:
            sets[fresh] = None   # nothing new: zero rows at the end of their positions
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
            offs = [0] * (2 * N)                      # the first call: everything fresh
        out = eng.decode_ex(torch.cat(rows_enc), max_length=L, pos_offset=offs, steps=S)
        if call > 0 and sets[cont] is not None:       # the continuing set just finished
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
        for j in range(N):   # up to the row's end (past an eot the two pad differently)
            k = plen + int(n[j])
            assert torch.equal(t[j, :k], rt[j, :k]), (bi, j)
        assert int(n.min()) >= min(16, L - plen - 1)


def test_staggered_offset_past_stand_is_rejected(engine, gpu):
    """The context records where every row slot stands after each call
    (janus_whisper_decode_stand) and rejects a continuing row whose pos_offset lies past it
    — it would read tokens and KV rows never written — with a non-zero status and
    janus_last_error, as it rejects continuing after a call of another batch size. The
    valid plan right after the rejected one is still bit-identical to the full decode (a
    call rejected by the checks runs nothing and keeps the slots' state)."""
    from janus_amd import _native as nat
    eng, _ = engine
    N, L, S = 2, 40, 20
    utts = [synth_speech(400 + j, 2.0) for j in range(N)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, N, 3))
    ref = eng.decode_ex(enc, max_length=L)
    two = torch.cat([enc, enc])
    eng.decode_ex(two, max_length=L, pos_offset=[0] * (2 * N), steps=S)
    assert eng.decode_stand(2 * N) == [S] * (2 * N)
    # continuing one position past the stand: rejected before anything runs (the slots
    # keep their state)
    with pytest.raises(nat.JanusNativeError, match="stands at"):
        eng.decode_ex(two, max_length=L, pos_offset=[0] * N + [S + 1] * N, steps=S - 1)
    assert eng.decode_stand(2 * N) == [S] * (2 * N)
    # negative steps are refused on the Python side, a stray steps without offsets too
    with pytest.raises(ValueError):
        eng.decode_ex(two, max_length=L, pos_offset=[0] * (2 * N), steps=-1)
    with pytest.raises(ValueError):
        eng.decode_ex(two, max_length=L, steps=S)
    # the good plan: continue at S, bit-identical to the one-call decode
    out = eng.decode_ex(two, max_length=L, pos_offset=[0] * N + [S] * N, steps=L - 1 - S)
    assert eng.decode_stand(2 * N) == [L - 1 - S] * N + [L - 1] * N
    sl = slice(N, 2 * N)
    assert torch.equal(out.n_tokens[sl].cpu(), ref.n_tokens.cpu())
    assert torch.equal(out.sum_logprob[sl].cpu(), ref.sum_logprob.cpu())
    plen = len(eng.tokenizer.sot_sequence)
    for j in range(N):
        k = plen + int(ref.n_tokens[j])
        assert torch.equal(out.tokens[N + j, :k].cpu(), ref.tokens[j, :k].cpu())
    # another batch size cannot continue these slots
    with pytest.raises(nat.JanusNativeError, match="batch size"):
        eng.decode_ex(enc[:1].repeat(3, 1, 1), max_length=L, pos_offset=[0, 5, 5], steps=5)


def test_decode_lanes_match_single_lane(engine, gpu):
    """Opt-in decoder lanes (janus_decode_options.lanes: the batch split over concurrent streams and
    host threads) decode every utterance exactly as the single-lane decoder does: rows
    are independent through every decoder kernel."""
    eng, _ = engine
    utts = [synth_speech(60 + k, 3.0 + k) for k in range(5)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    t1, n1, _ = eng.decode(enc, 24, lanes=1)
    t1, n1 = t1.cpu(), n1.cpu()
    t2, n2, _ = eng.decode(enc, 24, lanes=2)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2.cpu()) and torch.equal(n1, n2.cpu())


@pytest.mark.parametrize("temps", [(0.0,), (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)], ids=["t0", "fallback"])
def test_seek_loop_matches_oracle(engine, gpu, temps):
    """faster-whisper's generate_segments loop (seek by the last timestamp pair, previous
    text as the <|startofprev|> prompt, gates, no-speech skip, blank-segment drop) on the
    GPU (per-row prompts, batched over utterances) vs the oracle's restatement of the same
    loop, for a 40 s (several windows) and a 7 s utterance — at temperature 0 alone and with
    generate_with_fallback (every window of the seeded synthetic model fails the log-prob
    gate, so each runs all five sampled temperatures x best_of 5 and settles on the best
    avg_logprob at T = 1.0, resetting the prompt). max_length 64 bounds the oracle's time;
    the prompt keeps max_length // 2 - 1 previous tokens as at 448."""
    from janus_amd.services.transcriber import generate_segments
    eng, W = engine
    auds = [synth_speech(160, 40.0, sr=16000), synth_speech(161, 7.0, sr=16000)]
    streams = generate_segments(eng, auds, max_length=64, temperatures=temps)
    tk = eng.tokenizer
    for i, (a, st) in enumerate(zip(auds, streams)):
        ref, cnt = ow.transcribe_segments(a, W, CFG, tk, mel_filters(), max_length=64,
                                          temperatures=temps, utt=i)
        got = [(s.start, s.end, s.text, list(s.tokens)) for s in st.segments]
        assert st.windows == cnt["windows"] and st.fallbacks == cnt["needs_fallback"] and st.skips == cnt["skips"]
        assert st.fallback_decodes == cnt["fallback_decodes"]
        assert [g[3] for g in got] == [r[3] for r in ref]
        assert [g[2] for g in got] == [r[2] for r in ref]
        assert np.allclose([g[:2] for g in got], [r[:2] for r in ref])
        if len(temps) > 1:
            assert st.fallbacks == st.windows and st.fallback_decodes == 5 * st.windows
            assert all(s.temperature == 1.0 for s in st.segments)
        print(f"seek loop {temps}: {st.windows} windows, {len(got)} segments, "
              f"{st.fallbacks} failed at T=0, {st.fallback_decodes} sampled decodes")


def test_seek_loop_speculative_matches_sequential(engine, gpu):
    """generate_segments(speculative=True) — each round's T = 0 rows and every fallback
    temperature's best_of hypotheses in ONE decode call (per-row temperatures) — gives
    exactly the sequential temperature walk's result: segments, tokens, windows, gate and
    fallback counters (the streaming encoder's setting)."""
    from janus_amd.services.transcriber import TEMPERATURES, generate_segments
    eng, _ = engine
    auds = [synth_speech(160, 40.0, sr=16000), synth_speech(161, 7.0, sr=16000),
            synth_speech(162, 3.0, sr=16000)]
    res = {}
    for spec in (False, True):
        res[spec] = generate_segments(eng, auds, max_length=64, temperatures=TEMPERATURES,
                                      speculative=spec, utt_keys=[11, 12, 13])
    for a, b in zip(res[False], res[True]):
        assert [(s.start, s.end, s.text, list(s.tokens), s.temperature) for s in a.segments] == \
            [(s.start, s.end, s.text, list(s.tokens), s.temperature) for s in b.segments]
        assert (a.windows, a.fallbacks, a.skips, a.fallback_decodes, a.sampled) == \
            (b.windows, b.fallbacks, b.skips, b.fallback_decodes, b.sampled)
        assert a.window_tokens == b.window_tokens and a.window_rows == b.window_rows
    assert sum(s.fallback_decodes for s in res[True]) > 0


def test_per_row_temperatures_match_scalar(engine, gpu):
    """janus_whisper_decode_sample_rows_ex: rows at different temperatures (0 = greedy) in
    one call decode bit-identically to the greedy call and to one scalar-temperature call
    per temperature with the same seeds and shared encoder rows."""
    eng, _ = engine
    utts = [synth_speech(330 + k, 3.0 + 2 * k) for k in range(3)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    ei = [0, 0, 0, 1, 1, 2, 2, 2]
    temps = [0.0, 0.2, 1.0, 0.0, 0.6, 0.2, 0.0, 1.0]
    seeds = [500 + 7 * b for b in range(len(ei))]
    mix = eng.decode_ex(enc, max_length=40, temperature=temps, seeds=seeds, enc_index=ei)
    got = [t.cpu() for t in (mix.tokens, mix.n_tokens, mix.sum_logprob, mix.no_speech_prob)]
    for T in sorted(set(temps)):
        rows = [b for b in range(len(ei)) if temps[b] == T]
        kw = dict(temperature=T, seeds=[seeds[b] for b in rows]) if T > 0 else {}
        ref = eng.decode_ex(enc, max_length=40, enc_index=[ei[b] for b in rows], **kw)
        want = [t.cpu() for t in (ref.tokens, ref.n_tokens, ref.sum_logprob, ref.no_speech_prob)]
        for g, w_ in zip(got, want):
            assert torch.equal(g[rows], w_), T


def test_non_polling_call_matches_polling(base_engine, gpu):
    """A decode call without early-exit polling (check_every 0: the staggered serving
    step's calls, which return without waiting for their stream) gives the polling call's
    rows — tokens up to each row's end, counts, log-prob sums — on the persistent segments,
    and janus_whisper_decode_check then reports no barrier timeout."""
    eng, _ = base_engine
    utts = [synth_speech(340 + k, 2.0 + k) for k in range(4)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    a = eng.decode_ex(enc, max_length=48, persistent=2, check_every=16)
    b = eng.decode_ex(enc, max_length=48, persistent=2, check_every=0)
    eng.decode_check()
    torch.cuda.synchronize()
    plen = len(eng.tokenizer.sot_sequence)
    assert torch.equal(a.n_tokens.cpu(), b.n_tokens.cpu())
    assert torch.equal(a.sum_logprob.cpu(), b.sum_logprob.cpu())
    for r in range(len(utts)):
        n = plen + int(a.n_tokens[r])
        assert torch.equal(a.tokens[r, :n].cpu(), b.tokens[r, :n].cpu())


def test_sample_noise_matches_oracle(gpu):
    """The decoder's Gumbel noise (janus_sample_gumbel_f32: the hash and -log(-log u) the
    sampling logits kernel adds) equals the oracle's restatement (float64 logs) to f32
    rounding, over a whole vocabulary for several seeds and positions."""
    from janus_amd import _native as nat
    V = 51864
    seeds = np.array([0, 1, 0xDEADBEEF, 123456789], np.uint32)
    sd = torch.from_numpy(seeds.view(np.int32).copy()).to(gpu)
    out = torch.empty(len(seeds), V, dtype=torch.float32, device=gpu)
    for pos in (0, 3, 447):
        nat.call("janus_sample_gumbel_f32", sd.data_ptr(), len(seeds), pos, V, out.data_ptr(),
                 nat.stream_ptr())
        got = out.cpu().numpy().astype(np.float64)
        for b, sdv in enumerate(seeds):
            ref = ow.sample_noise(int(sdv), pos, V)
            err = np.abs(got[b] - ref) / np.maximum(1.0, np.abs(ref))
            assert err.max() < 4e-7, (pos, b, err.max())
    # the noise is a Gumbel(0, 1) sample: mean 0.5772, variance pi^2 / 6
    assert abs(got.mean() - 0.5772) < 0.01 and abs(got.var() - np.pi ** 2 / 6) < 0.03


@pytest.mark.parametrize("which,T", [("tiny", 0.2), ("tiny", 1.0), ("base", 0.6)])
def test_sampled_decode_matches_oracle(engine, base_engine, gpu, which, T):
    """Decode at temperature T (faster-whisper's fallback re-decode,
    janus_whisper_decode_sample_ex: Gumbel-max over the rule-filtered logits / T with
    per-row counter-based noise) vs the oracle's sampler with the same seeds on the same
    encoder output: each row identical, or its first divergence at a step where the
    oracle's top-2 keys (logit / T + noise) are closer than NEAR_TIE / T (the fp16 path's
    logit error scaled by 1 / T); sum of log-probs within 0.1 % for identical rows.
    Rows of one window share the encoder output (best_of replication) and differ only in
    their seeds."""
    eng, W = engine if which == "tiny" else base_engine
    cfg = CFG if which == "tiny" else BASE
    utts = [synth_speech(300 + k, 6.0 + 7 * k) for k in range(3)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    enc = enc.repeat_interleave(2, 0).contiguous()          # two hypotheses per utterance
    seeds = [1000 + 17 * b for b in range(enc.shape[0])]
    ml = 48
    out = eng.decode_ex(enc, max_length=ml, temperature=T, seeds=seeds)
    rows = out.rows()
    toks = out.tokens.cpu().numpy()
    ref = ow.greedy_cached(enc.float().cpu(), W, cfg, eng.tokenizer, ml, no_speech=50361,
                           temperature=T, seeds=seeds)
    plen = len(eng.tokenizer.sot_sequence)
    same = 0
    for b, r in enumerate(ref):
        g = [int(t) for t in toks[b][plen:plen + int(out.n_tokens[b])]]
        if g == r["tokens"]:
            same += 1
            assert abs(float(out.sum_logprob[b]) - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]) + 1e-3
        else:
            first = next((i for i in range(min(len(g), len(r["tokens"]))) if g[i] != r["tokens"][i]),
                         min(len(g), len(r["tokens"])))
            margin = r["margins"][first] if first < len(r["margins"]) else 0.0
            assert margin < NEAR_TIE / T, (b, first, margin)
        assert abs(rows[b][2] - r["nsp"]) <= 5e-3 * max(r["nsp"], 1e-6) + 1e-7
    # the two hypotheses of one window share logits but not draws: they differ
    assert any(rows[2 * k][0] != rows[2 * k + 1][0] for k in range(len(utts)))
    assert same >= len(ref) - 1, same
    print(f"{which} T={T}: {same}/{len(ref)} sampled rows identical")


def test_sampling_leaves_greedy_unchanged(engine, gpu):
    """A sampled decode between two greedy decodes on the same context (the sampling
    logits kernel is a separate instantiation, its graphs keyed on the temperature) leaves
    the greedy result bit-identical."""
    eng, _ = engine
    utts = [synth_speech(320 + k, 5.0 + 3 * k) for k in range(4)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    t1, n1, s1 = eng.decode(enc, 40)
    t1, n1, s1 = t1.cpu(), n1.cpu(), s1.cpu()
    eng.decode_ex(enc, max_length=40, temperature=0.4, seeds=[7, 8, 9, 10])
    t2, n2, s2 = eng.decode(enc, 40)
    assert torch.equal(t1, t2.cpu()) and torch.equal(n1, n2.cpu()) and torch.equal(s1, s2.cpu())


@pytest.mark.parametrize("which", ["tiny", "base"])
def test_fused_xattn_merge_vproj_bit_identical(engine, base_engine, gpu, which):
    """The cross-attention split merge fused with the per-head value projection
    (xattn_combine_vproj_kernel, default) decodes bit-identically to the two launches it
    replaces (DEC_PATH_NO_CVP): same tokens, same summed log-probabilities."""
    eng, _ = engine if which == "tiny" else base_engine
    utts = [synth_speech(80 + k, 4.0 + 2 * k) for k in range(6)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    t1, n1, s1 = eng.decode(enc, 48, path_flags=DEC_PATH_NO_CVP)
    t1, n1, s1 = t1.cpu(), n1.cpu(), s1.cpu()
    t2, n2, s2 = eng.decode(enc, 48)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2.cpu()) and torch.equal(n1, n2.cpu())
    assert torch.equal(s1, s2.cpu())


def test_fused_select_embed_bit_identical(base_engine, gpu):
    """The token selection at position p fused with the embedding of the chosen token at
    p + 1 (select_embed_kernel, default) decodes bit-identically to the two launches
    (DEC_PATH_NO_SEL_EMBED), including rows that finish early and the last position."""
    eng, _ = base_engine
    utts = [synth_speech(90 + k, 3.0 + 3 * k) for k in range(5)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    t1, n1, s1 = eng.decode(enc, 37, check_every=8, path_flags=DEC_PATH_NO_SEL_EMBED)
    t1, n1, s1 = t1.cpu(), n1.cpu(), s1.cpu()
    t2, n2, s2 = eng.decode(enc, 37, check_every=8)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2.cpu()) and torch.equal(n1, n2.cpu()) and torch.equal(s1, s2.cpu())


@pytest.mark.parametrize("flags", [DEC_PATH_RESID_LN, dec_path_ln_mask(15), dec_path_ln_mask(0)],
                         ids=["resid_ln", "mask15", "mask0"])
def test_layernorm_placements_bit_identical(base_engine, gpu, flags):
    """Every LayerNorm placement rounds alike (mfma.h ln_sum4 / ln_sq4 / ln_norm4): the
    separate launch (mask 0), the GEMM prologues (mask 15: LN1 -> QKV, LN2 -> absorbed query
    projection, LN3 -> fc1, final -> vocabulary projection), the whole-row residual
    projection + LayerNorm kernel (DEC_PATH_RESID_LN) and the default (mask 9) decode the same
    tokens with the same summed log-probabilities."""
    eng, _ = base_engine
    utts = [synth_speech(120 + k, 3.0 + 2 * k) for k in range(4)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    t1, n1, s1 = eng.decode(enc, 40)
    t1, n1, s1 = t1.cpu(), n1.cpu(), s1.cpu()
    t2, n2, s2 = eng.decode(enc, 40, path_flags=flags)
    torch.cuda.synchronize()
    assert torch.equal(t1, t2.cpu()) and torch.equal(n1, n2.cpu()) and torch.equal(s1, s2.cpu())


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_persistent_segments_vs_oracle(base_engine, gpu, mode):
    """The persistent decoder segments (janus_decode_options.persistent: per layer two
    resident-grid launches with in-launch barriers instead of ten launches) decode base.en
    free-running to 448 tokens like the oracle — identical, or first divergence at an
    oracle near-tie — and agree with the launch path on the gate inputs (sum of chosen
    log-probs within 1e-3 where the sequences match, no-speech probability within 0.5 %).
    mode 2: the layer kernel (segment B, the next layer's self-attention and its segment A in
    one launch per layer step)."""
    eng, W = base_engine
    secs = [30.0, 17.0, 8.0, 3.0, 1.0, 0.3, 24.0, 12.0]
    utts = [synth_speech(140 + k, s) for k, s in enumerate(secs)]
    pcm, offs = pack(utts, gpu)
    enc = eng.encode(eng.logmel(pcm, offs, len(utts), 3))
    per = eng.decode_ex(enc, max_length=448, persistent=mode)
    lau = eng.decode_ex(enc, max_length=448, persistent=0)
    torch.cuda.synchronize()
    tk = eng.tokenizer
    plen = len(tk.sot_sequence)
    nt = per.n_tokens.cpu().numpy()
    assert (nt >= 128).all()
    ref = ow.greedy_cached(enc.float().cpu(), W, BASE, tk, 448, no_speech=50361)
    seq, pk = _check_free_running(per.tokens.cpu().numpy(), ref, tk, plen, nt)
    print(f"persistent mode {mode}, base.en free-running: sequences identical {seq:.3f}, packets {pk:.3f}")
    assert seq >= 0.75 and pk >= 0.75
    pt, lt = per.tokens.cpu(), lau.tokens.cpu()
    for b in range(len(utts)):
        if torch.equal(pt[b], lt[b]):
            a, c = float(per.sum_logprob[b]), float(lau.sum_logprob[b])
            assert abs(a - c) <= 1e-3 * abs(c), (b, a, c)
        a, c = float(per.no_speech_prob[b]), float(lau.no_speech_prob[b])
        assert abs(a - c) <= 5e-3 * c + 1e-12, (b, a, c)


@pytest.mark.parametrize("rows,mode,flags", [(40, 1, 0), (64, 1, 0), (40, 2, 0), (64, 2, 0), (64, 3, 0),
                                             (128, 1, 0), (128, 2, 0), (128, 3, 0), (128, 2, 0x10000)])
def test_persistent_staggered_bit_identical(base_engine, gpu, rows, mode, flags):
    """Continuous batching through the persistent segments: two slot sets of `rows` rows
    (2 x 128 = the bench's decoder call: each set a batch's first windows and an earlier
    batch's continuation windows; 256 rows run a 128-block grid with two split-K pairs and
    attention blocks per block, or with DEC_PATH_SEG_2CU two blocks per CU), each batch
    started fresh in one call and continued in the next, equal a full persistent decode of
    that batch alone bit for bit — a row's arithmetic in the segments does not depend on the
    rows beside it or on the grid."""
    eng, _ = base_engine
    L, S = 40, 20
    batches = []
    for k in range(3):
        utts = [synth_speech(600 + 10 * k + j, 1.0 + (j % 5)) for j in range(rows)]
        pcm, offs = pack(utts, gpu)
        batches.append(eng.encode(eng.logmel(pcm, offs, rows, 3)))
    # the same launch geometry on both sides (cu_count sets the vocabulary projection's
    # block count, whose partial merge order reaches the log-prob sums' last bits)
    ref = [eng.decode_ex(e, max_length=L, persistent=mode, cu_count=128) for e in batches]
    sets = [None, None]
    got = {}
    for call in range(4):
        fresh, cont = call % 2, 1 - call % 2
        sets[fresh] = call if call < 3 else None
        rows_enc, offs = [], []
        for st in (0, 1):
            bi = sets[st]
            if bi is None:
                rows_enc.append(torch.zeros_like(batches[0]))
                offs += [L - S] * rows if st == cont or call == 3 else [0] * rows
            else:
                rows_enc.append(batches[bi])
                offs += [0 if st == fresh else S] * rows
        if call == 0:
            offs = [0] * (2 * rows)
        out = eng.decode_ex(torch.cat(rows_enc), max_length=L, pos_offset=offs, steps=S, persistent=mode,
                            cu_count=128, path_flags=flags)
        if call > 0 and sets[cont] is not None:
            bi = sets[cont]
            sl = slice(cont * rows, cont * rows + rows)
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
        for j in range(rows):
            k = plen + int(n[j])
            assert torch.equal(t[j, :k], rt[j, :k]), (bi, j)


@pytest.fixture(scope="module")
def launch_engines(engine, base_engine, gpu):
    """The engines of tests/decode_launches.py's models: the module's tiny.en and base.en
    ones, the small-cut one (768 wide, 12 heads) made on first use."""
    import decode_launches as dl
    made = {"tiny": engine[0], "base": base_engine[0]}

    def get(model):
        if model not in made:
            made[model] = dl.make_engine(model)
        return made[model]
    return get


def _launch_case_ids():
    import decode_launches as dl
    return [n for n in dl.CASES if n != "stagger_continued"]


@pytest.mark.parametrize("name", _launch_case_ids())
def test_decode_launch_counts(launch_engines, name):
    """The launch structure of a decode call is the plan's alone: positions stepped, kernel
    launches issued (captured graph nodes), how the rows reached their encoder output and the
    persistent level run equal tests/golden/decode_launches.json, recorded by
    tests/golden/make_decode_launches.py before the decode call's host side was split up
    (the staggered pair: a fresh call, then the call that continues two of its rows)."""
    import decode_launches as dl
    golden = dl.golden()
    for case in ([name, "stagger_continued"] if name == "stagger_fresh" else [name]):
        got = dl.run_case(launch_engines(dl.CASES[case][0]), case)
        print(case, got, golden[case])
        assert got == golden[case], case
