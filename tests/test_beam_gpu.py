"""Beam search on the GPU (janus_whisper_decode_beam_ex): the three kernels
through their test entries against numpy, and the decode against tests/beam_ref.py.

Pass rule of the decode tests: a window passes if its winner's tokens equal the reference's,
and then |S_gpu - S_ref| <= 1e-3 |S_ref| + 1e-3 (the greedy tests' bound). A differing window
is excused only if the reference's own smallest margin for it (over every step's decision
margin and the final-choice margin) is below BEAM_TIE; at least 3 of every 4 windows of each
test must be identical outright."""
import ctypes

import numpy as np
import pytest
import torch

import beam_ref
from janus_amd import _native as nat
from janus_amd import tokenizer as tok
from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights

pytestmark = pytest.mark.gpu
CFG = CONFIGS["tiny.en"]
NEAR_TIE = 2e-3
# max(NEAR_TIE, 4 E): E = the largest |S_gpu - S_ref| over the identical windows of these
# tests on the MI355X (two competing scores each off by up to E, doubled for headroom).
# Measured E = 3.79e-3 (base.en, 70 rows, S about -52; the largest of 34 identical windows,
# DESIGN.md §5k), so BEAM_TIE = 1.52e-2.
BEAM_E = 3.8e-3
BEAM_TIE = max(NEAR_TIE, 4 * BEAM_E)
E_SEEN = []   # |S_gpu - S_ref| of every identical window (printed: the source of BEAM_E)


def stream():
    return torch.cuda.current_stream().cuda_stream


def tk_rules():
    t = tok.load_tokenizer()
    return t, dict(eot=t.eot, suppress_blank=1, blank=t.blank, ts_begin=t.timestamp_begin,
                   no_timestamps=t.no_timestamps, max_initial_ts=50)


# ------------------------------------------------------------------ top-2k epilogue
def allowed_rows(V, rules, R, smask):
    """numpy restatement of decoder.hip allowed(): bool [rows][V]."""
    ar = np.arange(V)
    is_ts = ar >= R["ts_begin"]
    out = []
    for (sb, sat, st, floor, _last) in rules:
        ok = ~smask.copy()
        if sb and R["suppress_blank"]:
            ok[[R["blank"], R["eot"]]] = False
        ok[R["no_timestamps"]] = False
        if sat:
            ok[is_ts] = False
        if st:
            ok[:R["eot"]] = False
        ok[is_ts & (ar < floor)] = False
        if sb:
            ok[~is_ts] = False
            ok[ar > R["ts_begin"] + R["max_initial_ts"]] = False
        out.append(ok)
    return np.array(out), is_ts


def top_of(vals, ok, n):
    idx = np.flatnonzero(ok)
    order = idx[np.lexsort((idx, -vals[idx]))][:n + 1]
    return order


@pytest.mark.parametrize("n2k", [2, 10, 16])
@pytest.mark.parametrize("rows", [1, 5, 70])
@pytest.mark.parametrize("K", [384, 512, 768])
def test_topk_epilogue(gpu, K, rows, n2k):
    """The beam instantiation of the vocabulary projection: per row the best 2k allowed
    entries (every token / timestamps only), no logits in memory, against numpy on the same
    fp16 operands. Rule states put the blank tile, the eot / timestamp tiles and a ts_floor
    into play; 70 rows cross the 64-row group. Indices identical; values within 1e-4 of the
    largest logit (fp32 accumulation of exact fp16 products against float64, the fp32-output
    bound of the GEMM tests)."""
    t, R = tk_rules()
    V = tok.N_VOCAB_EN
    smask = np.zeros(V, bool)
    smask[list(t.suppress_tokens())] = True
    tb = R["ts_begin"]
    states = [(1, 0, 0, -1, -1), (0, 0, 0, -1, -1), (0, 1, 0, tb + 38, tb + 37),
              (0, 0, 1, tb + 12, tb + 12), (0, 0, 0, tb + 700, tb + 699)]
    rules = [states[i % len(states)] for i in range(rows)]
    ok, is_ts = allowed_rows(V, rules, R, smask)
    g = torch.Generator().manual_seed(1000 * K + 10 * rows + n2k)
    Wt = (torch.randn(V, K, generator=g) / np.sqrt(K)).half()
    Wd = Wt.double().T.contiguous()
    A, L, want = [], [], []
    for b in range(rows):
        seed = 100000 + 1000 * b + K + n2k
        while True:   # a row whose reference order is not within rounding of a tie (CPU only)
            a = torch.randn(K, generator=torch.Generator().manual_seed(seed)).half()
            Lb = (a.double() @ Wd).numpy()
            per, gap = [], np.inf
            for sel in (ok[b], ok[b] & is_ts):
                o = top_of(Lb, sel, n2k)
                if len(o) > 1:
                    gap = min(gap, float(np.min(-np.diff(Lb[o]))))
                per.append(o[:n2k])
            if gap > 1e-4:
                break
            seed += 7919
        A.append(a)
        L.append(Lb)
        want.append(per)
    A, L = torch.stack(A), np.array(L)
    nblk = nat.lib().janus_beam_partial_blocks(V, K, 256)
    dA, dW = A.to(gpu), Wt.to(gpu)
    sm = np.zeros((V + 15) // 16 * 16, np.uint8)
    sm[:V] = smask
    dsm = torch.from_numpy(sm).to(gpu)
    rr = np.zeros((rows, 8), np.int32)
    rr[:, :5] = rules
    drr = torch.from_numpy(rr).to(gpu)
    parts = torch.zeros(rows * nblk * 14, dtype=torch.float32, device=gpu)
    tops = torch.zeros(rows * nblk * 64, dtype=torch.float32, device=gpu)
    av = torch.empty(rows, n2k, dtype=torch.float32, device=gpu)
    tv = torch.empty_like(av)
    ai = torch.empty(rows, n2k, dtype=torch.int32, device=gpu)
    ti = torch.empty_like(ai)
    nat.call("janus_beam_logits_topk_f16", dA.data_ptr(), dW.data_ptr(), K, V, rows, R["eot"],
             R["suppress_blank"], R["blank"], R["ts_begin"], R["no_timestamps"], R["max_initial_ts"],
             dsm.data_ptr(), drr.data_ptr(), 256, parts.data_ptr(), tops.data_ptr(), n2k,
             av.data_ptr(), ai.data_ptr(), tv.data_ptr(), ti.data_ptr(), stream())
    torch.cuda.synchronize()
    av, ai, tv, ti = av.cpu().numpy(), ai.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()
    tol = 1e-4 * float(np.abs(L).max())
    for b in range(rows):
        for (gv, gi, o) in ((av[b], ai[b], want[b][0]), (tv[b], ti[b], want[b][1])):
            n = len(o)
            assert list(gi[:n]) == list(o), (b, gi, o)
            assert np.all(gi[n:] == -1) and np.all(np.isneginf(gv[n:]))
            assert np.abs(gv[:n] - L[b][o]).max(initial=0.0) <= tol
    # the filtered maximum the partials carry beside the lists (LogitPart.m_all)
    p = parts.cpu().numpy().reshape(rows, nblk, 14)
    for b in range(rows):
        assert abs(p[b, :, 0].max() - L[b][ok[b]].max()) <= tol


# ------------------------------------------------------------------------ beam step
V_TOY, EOT, TS0, NOTS, BLANK = 64, 50, 56, 55, 1
R_TOY = dict(eot=EOT, suppress_blank=1, blank=BLANK, ts_begin=TS0, no_timestamps=NOTS, max_initial_ts=4)


def next_rules(r, prev_tok, nxt):
    """decoder_dev.h next_row_rules."""
    sb, _sat, _st, _floor, last = r
    last_ts = nxt >= TS0
    pen_ts = bool(sb) or prev_tok >= TS0
    if last_ts:
        last = nxt
    floor = (last if (last_ts and not pen_ts) else last + 1) if last >= 0 else -1
    return (0, int(last_ts and pen_ts), int(last_ts and not pen_ts), floor, last)


def ref_step(k, win, pos, ld):
    """The numpy walk of one window at position pos. win: dict(plen, nlive, nfin, wdone, S,
    ntok, rules, tokens [k][ld], lists [k] of (set_all [(v, i)], set_ts [(v, i)], m_all,
    m_text, m_ts)). Returns the expected state after the step."""
    out = dict(tokens=win["tokens"].copy(), S=list(win["S"]), ntok=list(win["ntok"]),
               rules=list(win["rules"]), done=list(win["done"]), nlive=win["nlive"], nfin=win["nfin"],
               wdone=win["wdone"], moved=0, parent=list(range(k)), fin=[], n_new=0)
    if pos + 1 < win["plen"]:
        return out
    if win["wdone"]:
        out["tokens"][:, pos + 1] = EOT
        return out
    cands = []
    for b in range(win["nlive"]):
        sa, st, m_all, m_text, m_ts = win["lists"][b]
        use_ts = m_ts > -np.inf and m_ts > m_text     # s_all = s_ts = 1: lse = the maxima
        lse = m_ts if use_ts else m_all
        ent = sorted(st if use_ts else sa, key=lambda e: (-e[0], e[1]))[:2 * k]
        cands += [(win["S"][b] + (v - lse), b, i) for (v, i) in ent]
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    live, fin, _ = beam_ref.walk(cands, k, EOT, win["nfin"])
    for (b, sc) in fin:
        row = win["tokens"][b].copy()
        row[pos + 1] = EOT
        row[pos + 2:] = -1
        out["fin"].append((row, sc, win["ntok"][b] + 1))
    out["nfin"] = win["nfin"] + len(fin)
    out["n_new"] = len(live)
    for i in range(k):
        if i < len(live):
            b, v, sc = live[i]
            out["tokens"][i, :pos + 1] = win["tokens"][b, :pos + 1]
            out["tokens"][i, pos + 1] = v
            out["S"][i], out["ntok"][i] = sc, win["ntok"][b] + 1
            out["rules"][i] = next_rules(win["rules"][b], win["tokens"][b, pos], v)
            out["parent"][i] = b
        else:
            out["tokens"][i, pos + 1] = EOT
    out["moved"] = int(any(out["parent"][i] != i for i in range(len(live))))
    if out["nfin"] >= k or not live:
        out["wdone"] = 1
        out["done"] = [1] * k
    else:
        out["nlive"] = len(live)
    return out


def toy_window(rng, k, kind, pos, ld, nblk):
    """One window's state and hand-built partials. Every value is a small multiple of 1/8
    and every softmax sum is 1 (one block carries s = 1, the others nothing), so scores are
    exact in fp32."""
    plen = {"first": pos + 1, "prompt": pos + 3}.get(kind, 3)
    nlive = 1 if kind == "first" else k
    tokens = np.full((k, ld), -1, np.int32)
    tokens[:, :plen] = rng.integers(2, 40, plen)
    for b in range(k):
        if kind not in ("first", "prompt"):
            tokens[b, plen:pos + 1] = rng.integers(2, 40, pos + 1 - plen)
            if b % 2:
                tokens[b, pos] = TS0 + 2          # a beam whose last token is a timestamp
    ntok = [0 if kind in ("first", "prompt") else pos + 1 - plen] * k
    S = [0.0] * k if kind in ("first", "prompt") else [float(-rng.integers(0, 64)) / 8 for _ in range(k)]
    if kind in ("eot", "fill"):
        S[0] = 0.0                                 # beam 0 leads: its eot is the best candidate
    rules = [(1, 0, 0, -1, -1) if kind in ("first", "prompt") else
             ((0, 0, 1, TS0 + 2, TS0 + 2) if b % 2 else (0, 0, 0, -1, -1)) for b in range(k)]
    lists = []
    for b in range(k):
        # distinct logits: a permutation of multiples of 1/8 over the vocabulary
        vals = rng.permutation(V_TOY).astype(np.float64) / 8
        if kind in ("eot", "fill") and b < 2:
            vals[EOT] = 20.0 + b / 8               # eot ahead of the text candidates
        ts_mode = kind == "first" or (b % 2 == 1 and kind != "prompt")
        sa = [(float(vals[i]), i) for i in range(V_TOY) if not (ts_mode and i < TS0)]
        st = [(float(vals[i]), i) for i in range(TS0, V_TOY)]
        m_all = max(v for v, _ in sa)
        m_ts = max(v for v, _ in st)
        m_text = -np.inf if ts_mode else max(v for v, i in sa if i < TS0)
        if not ts_mode:
            m_ts = min(m_ts, m_text - 1)           # timestamp mass below the best text token
            st = [(min(v, m_ts), i) for v, i in st]
        lists.append((sa, st, m_all, m_text, m_ts))
    nfin = {"fill": k - 1, "eot": 0}.get(kind, 0)
    return dict(plen=plen, nlive=nlive, nfin=nfin, wdone=int(kind == "done"), S=S, ntok=ntok,
                rules=rules, tokens=tokens, lists=lists, done=[int(kind == "done")] * k)


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_beam_step_kernel(gpu, k):
    """beam_step_kernel on hand-built partials against the numpy walk, exactly: parents,
    tokens, S, n_tok, RowRules, the finished list and the done flags. Windows: the first
    sampled step (only beam 0 live), eot among the candidates, a window that fills its
    finished list, a row inside its prompt, a mid-decode window with timestamp beams, a
    stopped window."""
    rng = np.random.default_rng(100 + k)
    kinds = ["first", "eot", "fill", "prompt", "mid", "done"]
    nw, pos, ld, nblk = len(kinds), 6, 12, 3
    wins = [toy_window(rng, k, kind, pos, ld, nblk) for kind in kinds]
    B = nw * k
    parts = np.zeros((B, nblk, 14), np.float32)
    parts[:, :, [0, 2, 3, 5, 7, 9, 10, 12, 13]] = -np.inf
    pi = parts.view(np.int32)
    pi[:, :, 6] = pi[:, :, 8] = 0x7FFFFFFF
    tops = np.zeros((B, nblk, 64), np.float32)
    tops[:, :, :16] = tops[:, :, 32:48] = -np.inf
    ti = tops.view(np.int32)
    ti[:, :, 16:32] = ti[:, :, 48:64] = 0x7FFFFFFF
    for w, win in enumerate(wins):
        for b in range(k):
            sa, st, m_all, m_text, m_ts = win["lists"][b]
            blk = (w + b) % nblk                   # the block that carries the statistics
            parts[w * k + b, blk, [0, 1, 2, 3, 4]] = [m_all, 1.0, m_text, m_ts, 1.0]
            parts[w * k + b, blk, [10, 11]] = [m_all, 1.0]
            for (ents, o) in ((sa, 0), (st, 32)):
                for c in range(nblk):              # entries dealt to blocks by index, sorted lists of <= 16
                    mine = sorted([e for e in ents if e[1] % nblk == c], key=lambda e: (-e[0], e[1]))[:16]
                    for q, (v, i) in enumerate(mine):
                        tops[w * k + b, c, o + q] = v
                        ti[w * k + b, c, o + 16 + q] = i
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    d = dict(parts=dev(parts), tops=dev(tops),
             rules=dev(np.array([[*r, 0, 0, 0] for win in wins for r in win["rules"]], np.int32)),
             tokens=dev(np.concatenate([win["tokens"] for win in wins])),
             done=dev(np.array([x for win in wins for x in win["done"]], np.int32)),
             S=dev(np.array([x for win in wins for x in win["S"]], np.float32)),
             ntok=dev(np.array([x for win in wins for x in win["ntok"]], np.int32)),
             plen=dev(np.array([win["plen"] for win in wins for _ in range(k)], np.int32)),
             nlive=dev(np.array([win["nlive"] for win in wins], np.int32)),
             nfin=dev(np.array([win["nfin"] for win in wins], np.int32)),
             wdone=dev(np.array([win["wdone"] for win in wins], np.int32)),
             moved=dev(np.full(nw, 7, np.int32)), parent=dev(np.full(B, -5, np.int32)),
             fin_tok=dev(np.full((nw, k, ld), -9, np.int32)), fin_s=dev(np.full((nw, k), -77.0, np.float32)),
             fin_n=dev(np.full((nw, k), -9, np.int32)))
    nat.call("janus_beam_step", d["parts"].data_ptr(), d["tops"].data_ptr(), nblk, EOT, 1, BLANK, TS0, NOTS, 4,
             d["rules"].data_ptr(), d["tokens"].data_ptr(), ld, pos, d["done"].data_ptr(), d["S"].data_ptr(),
             d["ntok"].data_ptr(), d["plen"].data_ptr(), k, nw, d["nlive"].data_ptr(), d["nfin"].data_ptr(),
             d["wdone"].data_ptr(), d["moved"].data_ptr(), d["parent"].data_ptr(), d["fin_tok"].data_ptr(),
             d["fin_s"].data_ptr(), d["fin_n"].data_ptr(), stream())
    torch.cuda.synchronize()
    g = {n: v.cpu().numpy() for n, v in d.items()}
    seen = set()
    for w, (kind, win) in enumerate(zip(kinds, wins)):
        want = ref_step(k, win, pos, ld)
        rows = slice(w * k, (w + 1) * k)
        assert g["moved"][w] == want["moved"], kind
        if kind == "prompt":
            assert np.array_equal(g["tokens"][rows], win["tokens"]) and g["nlive"][w] == win["nlive"]
            continue
        assert np.array_equal(g["tokens"][rows][:, :pos + 2], want["tokens"][:, :pos + 2]), kind
        assert list(g["S"][rows]) == [np.float32(x) for x in want["S"]], kind
        assert list(g["ntok"][rows]) == want["ntok"], kind
        assert list(g["done"][rows]) == want["done"] and g["wdone"][w] == want["wdone"], kind
        assert g["nfin"][w] == want["nfin"], kind
        if kind == "done":
            continue
        assert list(g["parent"][rows]) == want["parent"], kind
        if not want["wdone"]:
            assert g["nlive"][w] == want["nlive"], kind
        for i in range(want["n_new"]):   # the children's rule states
            assert tuple(g["rules"][w * k + i][:5]) == want["rules"][i], (kind, i)
        for f, (row, sc, n) in enumerate(want["fin"]):
            slot = win["nfin"] + f
            assert np.array_equal(g["fin_tok"][w, slot][:pos + 2], row[:pos + 2]), kind
            assert g["fin_s"][w, slot] == np.float32(sc) and g["fin_n"][w, slot] == n, kind
        if want["fin"]:
            seen.add("eot")
        if want["wdone"] and kind == "fill":
            seen.add("filled")
        if len(set(want["parent"])) < k and want["moved"]:
            seen.add("dup")
    assert {"eot", "filled", "dup"} <= seen, seen


# --------------------------------------------------------------------- KV reorder
@pytest.mark.parametrize("d", [384, 768])
@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_beam_reorder_kernel(gpu, k, d):
    """beam_reorder_kernel, bit-exact against numpy indexing: non-permutation parents with
    duplicates in one window, identity parents (moved = 0: cache untouched) in the other;
    positions 0, 1, the 8-position chunk boundary +- 1 and 446; positions past pos and the
    other layers' rows stay as they were."""
    layers, nw, nctx = 2, 2, 448
    rng = np.random.default_rng(k * 1000 + d)
    par0 = [0] * k if k == 2 else [0, 0, 1, 0, 2, 2, 7, 3][:k]
    if k == 8:
        par0[6] = 7
    parent = np.array(par0 + list(range(k)), np.int32)
    moved = np.array([1, 0], np.int32)
    kc0 = rng.integers(0, 1 << 16, (layers, nw * k, nctx, d), dtype=np.uint16)
    vc0 = rng.integers(0, 1 << 16, (layers, nw * k, nctx, d), dtype=np.uint16)
    dp, dm = torch.from_numpy(parent).to(gpu), torch.from_numpy(moved).to(gpu)
    for pos in (0, 1, 7, 8, 9, 446):
        kc = torch.from_numpy(kc0.view(np.int16)).to(gpu)
        vc = torch.from_numpy(vc0.view(np.int16)).to(gpu)
        nat.call("janus_beam_reorder_f16", kc.data_ptr(), vc.data_ptr(), layers, nw, k, nctx, d, pos,
                 dp.data_ptr(), dm.data_ptr(), stream())
        torch.cuda.synchronize()
        for (got, src) in ((kc, kc0), (vc, vc0)):
            want = src.copy()
            want[:, :k, :pos + 1] = src[:, parent[:k], :pos + 1]
            assert np.array_equal(got.cpu().numpy().view(np.uint16), want), (pos, k, d)


# ------------------------------------------------------------------------- decode
@pytest.fixture(scope="module")
def engine(gpu):
    W = synthetic_weights(CFG, seed=5)
    return WhisperEngine(CFG, W), W


def rand_enc(cfg, n, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, cfg.n_audio_ctx, cfg.d_model, generator=g) * 0.5).half().to(gpu)


def check_decode(out, ref, label):
    """The pass rule of the module docstring over one decode's windows; ref: per window
    dict(tokens, sum_lp, min_margin, nsp, ...) of beam_ref.reference()."""
    t, n = out.tokens.cpu().numpy(), out.n_tokens.cpu().numpy()
    S, nsp = out.sum_logprob.cpu().numpy(), out.no_speech_prob.cpu().numpy()
    same = 0
    for w, r in enumerate(ref):
        pl = int(out.prompt_lens[w])
        got = [int(x) for x in t[w][pl:pl + int(n[w])]]
        err = abs(float(S[w]) - r["sum_lp"])
        print(f"{label} window {w}: identical={got == r['tokens']} n={len(got)} S_gpu={float(S[w]):.6f} "
              f"S_ref={r['sum_lp']:.6f} |dS|={err:.3e} min_margin={r['min_margin']:.3e} "
              f"finished={r['n_finished']} steps={r['stop_step']}")
        if got == r["tokens"]:
            same += 1
            E_SEEN.append(err)
            assert err <= 1e-3 * abs(r["sum_lp"]) + 1e-3, (label, w, float(S[w]), r["sum_lp"])
            assert abs(float(nsp[w]) - r["nsp"]) <= 5e-3 * r["nsp"] + 1e-7, (label, w, float(nsp[w]), r["nsp"])
            assert np.all(t[w][pl + int(n[w]):] == -1)
        else:
            assert r["min_margin"] < BEAM_TIE, (label, w, r["min_margin"], got, r["tokens"])
    assert same >= -(-3 * len(ref) // 4), (label, same, len(ref))
    print(f"{label}: E so far {max(E_SEEN, default=0.0):.3e}")


def run_case(name, gpu, eng=None):
    """Decode one case of beam_ref.CASES on the GPU and check it against its reference."""
    c = beam_ref.CASES[name]
    tk = tok.load_tokenizer()
    cfg, W, enc_np, prompts = beam_ref.case_inputs(name, tk)
    ref = beam_ref.reference(name, tk)
    eng = eng if eng is not None else WhisperEngine(cfg, W)
    enc = torch.from_numpy(enc_np).half().to(gpu)
    out = eng.decode_beam(enc, prompts=prompts, beam_size=c["k"], max_length=c["max_length"])
    check_decode(out, ref, name)
    return eng, out, ref, prompts


def test_decode_tiny_k5(engine, gpu):
    """tiny.en, 4 windows, beam 5, max_length 20."""
    eng, _, _, _ = run_case("tiny_k5", gpu, engine[0])
    assert eng.decode_path().enc_rows == "in_place"


@pytest.mark.parametrize("k", [2, 3, 8])
def test_decode_other_beams(engine, gpu, k):
    """2 windows at beam 2, 3 and 8 (an odd beam leaves the PAIR blocks a lone row)."""
    run_case(f"tiny_k{k}", gpu, engine[0])


def test_decode_base_70_rows(gpu):
    """base.en, 14 windows x 5 = 70 rows (the row-split projections), max_length 12."""
    run_case("base_k5", gpu)


def test_decode_distil_small(gpu):
    """distil-small.en (12 heads, d_model 768), 2 windows, beam 5: gathered encoder rows."""
    eng, _, _, _ = run_case("distil_k5", gpu)
    assert eng.decode_path().enc_rows == "gathered"


def test_decode_per_window_prompts(engine, gpu):
    """Windows with prompts of different lengths (<|startofprev|> + previous tokens): each
    starts sampling at its own position, rows inside their prompt keep the forced tokens."""
    _, out, _, prompts = run_case("tiny_prompts", gpu, engine[0])
    assert list(out.prompt_lens) == [len(p) for p in prompts] and len({len(p) for p in prompts}) == 3
    t = out.tokens.cpu().numpy()
    for w, p in enumerate(prompts):
        assert list(t[w][:len(p)]) == p


def test_decode_reachable_eot(gpu):
    """Weights whose <|endoftext|> is reachable (synthetic weights never emit it; E[eot] += 9 x
    decoder.layer_norm.bias): the finished list, the stop at k finished and the choice by
    normalised score. Amount and windows were chosen on the CPU with the reference alone so
    that at beam 5, max_length 20, at least one window fills its finished list before
    max_length, at least one reaches max_length with 1 .. 4 finished, and two windows stop
    at different steps; the test asserts that of the reference it reads."""
    _, _, ref, _ = run_case("tiny_eot", gpu)
    steps = beam_ref.CASES["tiny_eot"]["max_length"] - len(tok.load_tokenizer().sot_sequence)
    assert any(r["n_finished"] == 5 and r["stop_step"] < steps for r in ref)
    assert any(1 <= r["n_finished"] <= 4 and r["stop_step"] == steps for r in ref)
    assert len({r["stop_step"] for r in ref}) >= 2
    assert any(r["tokens"][-1] == tok.EOT for r in ref)


def test_beam_one_is_greedy(engine, gpu):
    """decode_beam(beam_size=1) runs the beam kernels with one beam: bit-identical to
    decode_ex in tokens, n_tokens, sum_logprob and no_speech_prob."""
    eng, _ = engine
    enc = rand_enc(CFG, 3, 81, gpu)
    a = eng.decode_ex(enc, max_length=24)
    b = eng.decode_beam(enc, beam_size=1, max_length=24)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.n_tokens, b.n_tokens)
    assert torch.equal(a.sum_logprob, b.sum_logprob) and torch.equal(a.no_speech_prob, b.no_speech_prob)


def test_beam_checks(engine, gpu):
    """pos_offset, a temperature > 0 and windows x k > 512 are rejected by name; a
    persistent request runs the launch path and decode_path() says so."""
    eng, _ = engine
    enc = rand_enc(CFG, 2, 91, gpu)
    with pytest.raises(ValueError, match="pos_offset"):
        eng.decode_beam(enc, beam_size=2, pos_offset=[0, 0])
    with pytest.raises(ValueError, match="temperature"):
        eng.decode_beam(enc, beam_size=2, temperature=0.4)
    with pytest.raises(ValueError, match="512"):
        eng.decode_beam(enc[:1].expand(65, -1, -1), beam_size=8)
    # the library's own checks behind the Python ones
    from janus_amd.whisper import janus_decode_rows
    opt, keep = eng.decode_options(16)
    rows = janus_decode_rows()
    po = np.zeros(4, np.int32)
    rows.pos_offset = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    buf = torch.zeros(2 * 16 + 8, dtype=torch.int32, device=gpu)
    with pytest.raises(nat.JanusNativeError, match="pos_offset"):
        nat.call("janus_whisper_decode_beam_ex", eng._h, enc.data_ptr(), 2, ctypes.addressof(opt),
                 ctypes.addressof(rows), 2, ctypes.c_float(1.0), buf.data_ptr(), buf.data_ptr(),
                 buf.data_ptr(), None, stream())
    with pytest.raises(nat.JanusNativeError, match="512"):
        nat.call("janus_whisper_decode_beam_ex", eng._h, enc.data_ptr(), 65, ctypes.addressof(opt), None, 8,
                 ctypes.c_float(1.0), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, stream())
    a = eng.decode_beam(enc, beam_size=3, max_length=12)
    b = eng.decode_beam(enc, beam_size=3, max_length=12, persistent=2)
    assert eng.decode_path().persistent == 0
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.sum_logprob, b.sum_logprob)


def test_transcribe_beam5(gpu):
    """WhisperModel('tiny.en').transcribe(audio, beam_size=5) over a clip of two seek
    windows at max_length 16 against the reference seek loop driven by beam_ref
    (beam_ref.compute_transcribe): every window's T = 0 decode by the pass rule above, and,
    when every window is identical, the same segments. With the default temperatures the
    sampled fallback still runs for the windows that fail their gates."""
    from janus_amd.services.transcriber import WhisperModel, generate_segments
    model = WhisperModel("tiny.en")
    tk = model.engine.tokenizer
    ref = beam_ref.transcribe_reference(tk)
    c = beam_ref.TRANSCRIBE_CASE
    audio = beam_ref.transcribe_audio()
    segs, info = model.transcribe(audio, beam_size=c["k"], temperature=(0.0,), max_length=c["max_length"])
    segs = list(segs)
    st = generate_segments(model.engine, [audio], max_length=c["max_length"], temperatures=(0.0,),
                           beam_size=c["k"])[0]
    assert [(s.start, s.end, s.tokens) for s in segs] == [(s.start, s.end, s.tokens) for s in st.segments]
    assert len(ref["windows"]) >= 2
    same = 0
    for i, (r, (got, avg, _nsp)) in enumerate(zip(ref["windows"], st.window_rows)):
        print(f"transcribe window {i}: identical={got == r['tokens']} min_margin={r['min_margin']:.3e}")
        if got != r["tokens"]:
            assert r["min_margin"] < BEAM_TIE, (i, r["min_margin"], got, r["tokens"])
            break    # the later windows' prompts differ from here on
        same += 1
        assert abs(avg - r["avg"]) <= 1e-3 * abs(r["avg"]) + 1e-3, (i, avg, r["avg"])
    assert same >= -(-3 * len(ref["windows"]) // 4)
    if same == len(ref["windows"]):
        assert st.windows == same
        assert [list(s.tokens) for s in st.segments] == [g[2] for g in ref["segments"]]
        assert np.allclose([(s.start, s.end) for s in st.segments], [g[:2] for g in ref["segments"]])
    # the fallback temperatures still run when the gates fail
    before = dict(model.stats)
    list(model.transcribe(audio, beam_size=c["k"], max_length=c["max_length"])[0])
    ran = {k: model.stats[k] - before[k] for k in before}
    assert ran["windows"] >= 2 and ran["needs_fallback"] >= 1
    assert ran["fallback_decodes"] >= ran["needs_fallback"]
