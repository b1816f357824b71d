"""The history rules (repetition_penalty, no_repeat_ngram_size; include/janus.h
janus_decode_options) and the prompt options on the GPU, against tests/history_ref.py:

1. janus_history_rules (the bit-set kernel) exact against numpy;
2. janus_logits_partial_hist_f16 (the HIST vocabulary projection) against the float64 product of
   the same fp16 operands, bounds as tests/test_large_family_gpu.py's K = 1280 test: the argmax
   wherever the float64 margin exceeds 2e-3, log-sum-exps within 1e-4 relative; raw statistics
   equal to the plain kernel's bits; all-zero bit sets bit-identical to janus_logits_partial_f16;
3. decode parity with tests/golden/history_refs.json: every reference margin is >= 2 NEAR_TIE
   (asserted by the generator on the CPU), so the GPU tokens must be IDENTICAL, no position
   exempt;
4. WhisperModel("tiny.en").transcribe with the options against the reference seek loop."""
import numpy as np
import pytest
import torch

import beam_ref
import history_ref as hr
import large_family_ref as lf
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd.whisper import WhisperEngine

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the bit-set kernel
def expected_words(tokens, plens, pos, n, V, rg):
    """uint32 [groups][tiles][rg] after positions 0 .. pos: bits 0-15 every token sampled so far,
    16-31 the bans of position pos (history_ref.banned)."""
    B = len(tokens)
    words = np.zeros(((B + rg - 1) // rg, (V + 15) // 16, rg), np.uint32)
    for b in range(B):
        g = [int(t) for t in tokens[b][plens[b]:pos + 1]]
        for t in set(g):
            words[b // rg, t >> 4, b % rg] |= np.uint32(1 << (t & 15))
        for t in hr.banned(g, n):
            words[b // rg, t >> 4, b % rg] |= np.uint32(0x10000 << (t & 15))
    return words


def history_tokens(B, ld, V, ts_begin, seed):
    """Token rows from a six-token alphabet (so n-grams repeat) that holds a timestamp and V - 1
    (the last partial tile); row 0 is `a a a a ...` (overlapping matches), row 1 repeats
    `x <ts> y` (a timestamp inside an n-gram); prompt lengths 1 .. 4 differ by row."""
    rng = np.random.default_rng(seed)
    alphabet = np.array([5, 17, 16, 31, ts_begin + 37, V - 1], np.int32)
    tokens = alphabet[rng.integers(0, len(alphabet), size=(B, ld))].astype(np.int32)
    tokens[0, :] = 17
    if B > 1:
        tokens[1, :] = np.resize(np.array([31, ts_begin + 37, 5], np.int32), ld)
    plens = (1 + np.arange(B) % 4).astype(np.int32)
    return tokens, plens


@pytest.mark.parametrize("K,V", [(384, tok.N_VOCAB_EN), (1280, tok.N_VOCAB_V3)])
@pytest.mark.parametrize("B", [1, 33, 65])
def test_history_rules_kernel_is_exact(gpu, K, V, B):
    """n = 0 .. 4 (positions with m < n included), every position of a 14-token row in turn on
    the same words, so each step must clear exactly the bans of the step before it."""
    rg = 32 if K == 1280 else 64
    ld = 14
    tk = tok.WhisperTokenizer(n_vocab=V) if V != tok.N_VOCAB_EN else tok.WhisperTokenizer()
    tokens, plens = history_tokens(B, ld, V, tk.timestamp_begin, 77 + B)
    nwords = nat.lib().janus_history_words(V, K, B)
    assert nwords == ((B + rg - 1) // rg) * ((V + 15) // 16) * rg
    td, pd = torch.from_numpy(tokens).to(gpu), torch.from_numpy(plens).to(gpu)
    for n in range(5):
        hist = torch.zeros(nwords, dtype=torch.int32, device=gpu)
        for pos in range(ld):
            nat.call("janus_history_rules", td.data_ptr(), ld, B, pd.data_ptr(), n, V, K, pos, 1,
                     hist.data_ptr(), nat.stream_ptr())
            got = hist.cpu().numpy().view(np.uint32).reshape(-1, (V + 15) // 16, rg)
            want = expected_words(tokens, plens, pos, n, V, rg)
            assert np.array_equal(got, want), (n, pos, np.argwhere(got != want)[:4])
        if n >= 1:
            assert (want >> 16).any()          # the case does ban something
    # several positions in one call equal the same positions one by one
    hist = torch.zeros(nwords, dtype=torch.int32, device=gpu)
    nat.call("janus_history_rules", td.data_ptr(), ld, B, pd.data_ptr(), 2, V, K, 0, ld, hist.data_ptr(),
             nat.stream_ptr())
    got = hist.cpu().numpy().view(np.uint32).reshape(-1, (V + 15) // 16, rg)
    assert np.array_equal(got, expected_words(tokens, plens, ld - 1, 2, V, rg))


# ------------------------------------------------------------------ 2. the HIST projection
PEN = 1.3


_HIST_CASES = {}


def hist_case(K, gpu):
    """(Built once per K.) A [65][K], W [V][K] in fp16 (one generator; 33 rows at K = 1280), the float64 product,
    the suppress mask, per-row rule states (as the K = 1280 projection test) and per row the
    penalised / banned tokens: penalised — the row's unpenalised winner, a negative-logit
    token of a plain tile, <|endoftext|> (the eot tile), the no-speech target and V - 1 (the
    last tile); banned — the runner-up and a token of the last tile."""
    if K in _HIST_CASES:
        return _HIST_CASES[K]
    V = tok.N_VOCAB_V3 if K == 1280 else tok.N_VOCAB_EN
    B = 33 if K == 1280 else 65
    g = torch.Generator().manual_seed(5200 + K)
    A = torch.randn(B, K, generator=g).half()
    Wt = (0.05 * torch.randn(V, K, generator=g)).half()
    L = A.double().numpy() @ Wt.double().numpy().T
    tk = tok.WhisperTokenizer(n_vocab=V) if K == 1280 else tok.WhisperTokenizer()
    smask = np.zeros((V + 15) // 16 * 16, np.uint8)
    smask[tk.suppress_tokens()] = 1
    rules = np.zeros((B, 8), np.int32)
    rules[:, 3] = rules[:, 4] = -1
    for b in range(B):
        kind = b % 4
        if kind == 1:
            rules[b, 0] = 1
        elif kind == 2:
            rules[b, 2] = 1
            rules[b, 3] = tk.timestamp_begin + 100
        elif kind == 3:
            rules[b, 1] = 1
            rules[b, 3] = tk.timestamp_begin + 7
    pen, ban = [], []
    for b in range(B):
        ok = lf.allowed_mask(V, smask, tuple(rules[b, :4]), tk.eot, tk.blank, tk.timestamp_begin,
                             tk.no_timestamps, 50)
        order = np.argsort(np.where(ok, L[b], -np.inf))
        neg = 992 + int(np.argmax(L[b, 992:1056] < -0.2))       # tiles 62 .. 65: text, none special
        assert L[b, neg] < 0
        pen.append([int(order[-1]), neg, tk.eot, tk.no_speech, V - 1])
        ban.append([int(order[-2]), V - 3])
    _HIST_CASES[K] = dict(K=K, V=V, B=B, A=A, Wd=Wt.to(gpu), L=L, tk=tk, smask=smask, rules=rules, pen=pen,
                          ban=ban)
    return _HIST_CASES[K]


def words_of(rows, V, rg, pen, ban):
    words = np.zeros(((len(rows) + rg - 1) // rg, (V + 15) // 16, rg), np.uint32)
    for i, b in enumerate(rows):
        for t in pen[b]:
            words[i // rg, t >> 4, i % rg] |= np.uint32(1 << (t & 15))
        for t in ban[b]:
            words[i // rg, t >> 4, i % rg] |= np.uint32(0x10000 << (t & 15))
    return words


def run_projection(gpu, c, rows, words=None, inv_temp=0.0, seeds=None, pos=5):
    """The raw partials [B][nblk] (lf.PART_DTYPE) of the plain entry (words None) or the HIST one."""
    K, V, tk, B = c["K"], c["V"], c["tk"], len(rows)
    Ad = c["A"][rows].contiguous().to(gpu)
    sm = torch.from_numpy(c["smask"]).to(gpu)
    rr = torch.from_numpy(np.ascontiguousarray(c["rules"][rows])).to(gpu)
    nblk = nat.lib().janus_beam_partial_blocks(V, K, 256)
    parts = torch.zeros(B * nblk * 56, dtype=torch.uint8, device=gpu)
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu) if seeds is not None else None
    args = [Ad.data_ptr(), c["Wd"].data_ptr(), K, V, B, tk.eot, 1, tk.blank, tk.timestamp_begin,
            tk.no_timestamps, 50, tk.no_speech, sm.data_ptr(), rr.data_ptr(), 256, float(inv_temp),
            sd.data_ptr() if sd is not None else None, pos, parts.data_ptr()]
    if words is None:
        nat.call("janus_logits_partial_f16", *args, nat.stream_ptr())
    else:
        hd = torch.from_numpy(words.view(np.int32).reshape(-1)).to(gpu)
        assert hd.numel() == nat.lib().janus_history_words(V, K, B)
        nat.call("janus_logits_partial_hist_f16", *args, hd.data_ptr(), float(PEN), nat.stream_ptr())
    torch.cuda.synchronize()
    return parts.cpu().numpy().view(lf.PART_DTYPE).reshape(B, nblk)


def penalised_rows(c, rows):
    """(allowed mask incl. the bans, penalised float64 logits) per row."""
    V, tk = c["V"], c["tk"]
    out = []
    for b in rows:
        ok = lf.allowed_mask(V, c["smask"], tuple(c["rules"][b, :4]), tk.eot, tk.blank, tk.timestamp_begin,
                             tk.no_timestamps, 50)
        ok[c["ban"][b]] = False
        Lp = c["L"][b].copy()
        idx = sorted(set(c["pen"][b]))
        Lp[idx] = np.where(Lp[idx] < 0, Lp[idx] * PEN, Lp[idx] / PEN)
        out.append((ok, Lp))
    return out


@pytest.mark.parametrize("K,nrows", [(384, 1), (384, 17), (384, 64), (384, 65), (1280, 31), (1280, 32),
                                     (1280, 33)])
def test_hist_projection_greedy(gpu, K, nrows):
    c = hist_case(K, gpu)
    V, tk, tb = c["V"], c["tk"], c["tk"].timestamp_begin
    rg = 32 if c["K"] == 1280 else 64
    rows = list(range(nrows))
    plain = run_projection(gpu, c, rows)
    zero = run_projection(gpu, c, rows, np.zeros(((nrows + rg - 1) // rg, (V + 15) // 16, rg), np.uint32))
    assert plain.tobytes() == zero.tobytes()                    # all-zero bit sets: the sibling's bits
    raw = run_projection(gpu, c, rows, words_of(rows, V, rg, c["pen"], c["ban"]))
    for f in ("t_v", "m_raw", "s_raw"):                          # the raw statistics stay unpenalised
        assert raw[f].tobytes() == plain[f].tobytes(), f
    got, base = lf.merge_parts(raw), lf.merge_parts(plain)
    checked = changed = 0
    for b, (ok, Lp) in zip(rows, penalised_rows(c, rows)):
        g = got[b]

        def lse(v):
            return float(v.max() + np.log(np.exp(v - v.max()).sum())) if v.size else -np.inf
        for name, want in (("lse_all", lse(Lp[ok])), ("lse_ts", lse(Lp[tb:][ok[tb:]])), ("lse_raw", lse(c["L"][b]))):
            if np.isfinite(want):
                assert abs(g[name] - want) <= 1e-4 * abs(want), (b, name, g[name], want)
            else:
                assert g[name] == -np.inf, (b, name, g[name])
        assert abs(g["t_v"] - c["L"][b][tk.no_speech]) <= 2e-3      # raw, though the target is penalised
        for key, sel in (("best", ok), ("best_ts", ok & (np.arange(V) >= tb))):
            if not sel.any():
                continue
            cand = np.where(sel, Lp, -np.inf)
            top = np.sort(cand)[-2:]
            assert 0 <= g[key] < V and g[key] not in c["ban"][b], (b, key, g[key])
            if top[-1] - top[-2] > 2e-3:
                assert g[key] == int(np.argmax(cand)), (b, key, g[key], int(np.argmax(cand)))
                checked += 1
        if ok[:tb].any():
            assert abs(g["m_text"] - Lp[:tb][ok[:tb]].max()) <= 2e-3
        changed += int(g["best"] != base[b]["best"])
    assert checked >= nrows
    assert changed >= max(1, nrows // 2), (changed, nrows)       # penalising the winner moves it


@pytest.mark.parametrize("K", [384, 1280])
def test_hist_projection_sampling_keys(gpu, K):
    """SAMPLE at T = 0.6, every row of the case: the argmax of penalised logit / T + the device's
    own Gumbel noise over the allowed, unbanned tokens."""
    c = hist_case(K, gpu)
    V, B = c["V"], c["B"]
    rg = 32 if c["K"] == 1280 else 64
    T, pos = 0.6, 5
    rows = list(range(B))
    seeds = [7000 + b for b in rows]
    words = words_of(rows, V, rg, c["pen"], c["ban"])
    got = lf.merge_parts(run_projection(gpu, c, rows, words, inv_temp=1.0 / T, seeds=seeds, pos=pos))
    plain = run_projection(gpu, c, rows, inv_temp=1.0 / T, seeds=seeds, pos=pos)
    zero = run_projection(gpu, c, rows, np.zeros_like(words), inv_temp=1.0 / T, seeds=seeds, pos=pos)
    assert plain.tobytes() == zero.tobytes()
    sd = torch.tensor(seeds, dtype=torch.int64).to(torch.int32).to(gpu)
    noise = torch.empty(B, V, dtype=torch.float32, device=gpu)
    nat.call("janus_sample_gumbel_f32", sd.data_ptr(), B, pos, V, noise.data_ptr(), nat.stream_ptr())
    noise = noise.cpu().numpy().astype(np.float64)
    inv = float(np.float32(1.0) / np.float32(T))
    hit = 0
    for b, (ok, Lp) in zip(rows, penalised_rows(c, rows)):
        keys = np.where(ok, Lp * inv + noise[b], -np.inf)
        top = np.sort(keys)[-2:]
        if top[-1] - top[-2] > 2e-3 / T:
            assert got[b]["best"] == int(np.argmax(keys)), b
            hit += 1
    assert hit >= B - 3


# ------------------------------------------------------------------ 3. decode parity
@pytest.fixture(scope="module", params=["tiny", "cut"])
def model(request, gpu):
    name = request.param
    cfg, W = hr.model_cfg(name), hr.weights(name)
    return name, cfg, WhisperEngine(cfg, W)


def sampled_tokens(out, b):
    pl = int(out.prompt_lens[b])
    return [int(t) for t in out.tokens[b][pl:pl + int(out.n_tokens[b])].tolist()]


def check_rows(out, want, label, nsp=True):
    for b, r in enumerate(want):
        got = sampled_tokens(out, b)
        assert got == r["tokens"], (label, b, hr.first_difference(got, r["tokens"]), r["min_margin"])
        assert abs(float(out.sum_logprob[b]) - r["sum_lp"]) <= 1e-3 * abs(r["sum_lp"]) + 1e-3, (label, b)
        if nsp:   # (*.en: the reference reads it at the first sampled step, where the engine does)
            assert abs(float(out.no_speech_prob[b]) - r["nsp"]) <= 5e-3 * r["nsp"] + 1e-12, (label, b)


@pytest.mark.parametrize("p,n", hr.OPTION_SETS, ids=[hr.opt_key(p, n) for p, n in hr.OPTION_SETS])
def test_decode_parity(model, gpu, p, n):
    """Greedy rows, 70 rows (two row groups; three at K = 1280), per-row prompts of different
    lengths (one holding a token its row samples: prompt tokens are not penalised), five T = 0.6
    rows on each of two shared encoder rows, and per-row temperatures mixing both kinds."""
    name, cfg, eng = model
    tk = eng.tokenizer
    ref = hr.reference(name, p, n)
    sd = ref["seeds"]
    kw = dict(max_length=hr.ML, repetition_penalty=p, no_repeat_ngram_size=n)
    sot = list(tk.sot_sequence)
    nsp = not cfg.multilingual
    enc_g = torch.from_numpy(beam_ref.rand_enc(cfg, sd["greedy"])).half().to(gpu)
    out = eng.decode_ex(enc_g, prompts=[sot] * len(enc_g), **kw)
    check_rows(out, ref["greedy"], "greedy", nsp)
    assert eng.decode_path().persistent == 0
    again = eng.decode_ex(enc_g, prompts=[sot] * len(enc_g), **kw)       # the replayed graph: clean bits
    assert torch.equal(again.tokens, out.tokens) and torch.equal(again.sum_logprob, out.sum_logprob)
    idx = [b % len(enc_g) for b in range(70)]
    out = eng.decode_ex(enc_g[idx].contiguous(), prompts=[sot] * 70, **kw)
    check_rows(out, [ref["greedy"][i] for i in idx], "70 rows", nsp)
    enc_p = torch.from_numpy(beam_ref.rand_enc(cfg, sd["prompt_enc"])).half().to(gpu)
    out = eng.decode_ex(enc_p, prompts=ref["prompts"], **kw)
    check_rows(out, ref["prompt"], "prompts", nsp)
    enc_s = torch.from_numpy(beam_ref.rand_enc(cfg, sd["sample_enc"])).half().to(gpu)
    eidx = [e for e in range(len(enc_s)) for _ in range(hr.BEST_OF)]
    noise = [s for e in sd["sample_noise"] for s in e]
    out = eng.decode_ex(enc_s, prompts=[sot] * len(eidx), temperature=hr.T_SAMPLE, seeds=noise, enc_index=eidx, **kw)
    check_rows(out, ref["sampled"], "sampled", nsp)
    # per-row temperatures: greedy rows 0 and 1 (sample_enc = their encoder rows) among the sampled
    temps = [0.0] + [hr.T_SAMPLE] * hr.BEST_OF + [0.0] + [hr.T_SAMPLE] * hr.BEST_OF
    rows = [ref["greedy"][0]] + ref["sampled"][:hr.BEST_OF] + [ref["greedy"][1]] + ref["sampled"][hr.BEST_OF:]
    out = eng.decode_ex(enc_s, prompts=[sot] * len(temps), temperature=temps,
                        seeds=[0] + noise[:hr.BEST_OF] + [0] + noise[hr.BEST_OF:],
                        enc_index=[0] * (1 + hr.BEST_OF) + [1] * (1 + hr.BEST_OF), **kw)
    check_rows(out, rows, "row temperatures", nsp)


def test_options_off_change_nothing(model, gpu):
    """p = 1 and n = 0 given explicitly: the call without the fields, bit for bit; a persistent
    request with rules runs the launch path; the refusals arrive by name."""
    name, cfg, eng = model
    sd = hr.reference(name, *hr.OPTION_SETS[0])["seeds"]
    enc = torch.from_numpy(beam_ref.rand_enc(cfg, sd["greedy"])).half().to(gpu)
    a = eng.decode_ex(enc, max_length=hr.ML)
    b = eng.decode_ex(enc, max_length=hr.ML, repetition_penalty=1.0, no_repeat_ngram_size=0)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.sum_logprob, b.sum_logprob)
    c = eng.decode_ex(enc, max_length=hr.ML, repetition_penalty=1.3)
    d = eng.decode_ex(enc, max_length=hr.ML, repetition_penalty=1.3, persistent=2)
    assert eng.decode_path().persistent == 0
    assert torch.equal(c.tokens, d.tokens) and not torch.equal(a.tokens, c.tokens)
    a2 = eng.decode_ex(enc, max_length=hr.ML)                   # and back: nothing of the rules lingers
    assert torch.equal(a.tokens, a2.tokens) and torch.equal(a.sum_logprob, a2.sum_logprob)
    with pytest.raises(nat.JanusNativeError, match="staggered rows .* repetition_penalty"):
        eng.decode_ex(enc, max_length=hr.ML, pos_offset=[0] * len(enc), steps=4, no_repeat_ngram_size=2)


# ------------------------------------------------------------------ 4. transcribe
def test_transcribe_with_options(gpu):
    """The 33 s clip through WhisperModel("tiny.en").transcribe with a penalty, n-grams, an
    initial prompt, hotwords and no conditioning at a small max_length: the reference seek
    loop's segments, and not those of the call without options."""
    from janus_amd.services.transcriber import WhisperModel
    m = WhisperModel("tiny.en")
    tk = m.engine.tokenizer
    ref = hr.transcribe_reference(tk)
    c = hr.TRANSCRIBE_CASE
    audio = hr.transcribe_audio()
    with pytest.raises(NotImplementedError, match="repetition_penalty.*beam"):
        m.transcribe(audio, beam_size=5, repetition_penalty=1.3)
    opts = {k: c[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "initial_prompt", "hotwords",
                              "condition_on_previous_text")}
    segs = list(m.transcribe(audio, temperature=(0.0,), max_length=c["max_length"], **opts)[0])
    assert len(ref["windows"]) >= 2
    assert min(w["min_margin"] for w in ref["windows"]) >= hr.MIN_MARGIN
    assert [list(s.tokens) for s in segs] == [g[2] for g in ref["segments"]]
    assert np.allclose([(s.start, s.end) for s in segs], [g[:2] for g in ref["segments"]])
    plain = list(m.transcribe(audio, temperature=(0.0,), max_length=c["max_length"])[0])
    assert [list(s.tokens) for s in plain] != [list(s.tokens) for s in segs]
