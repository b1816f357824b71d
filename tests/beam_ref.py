"""Numpy restatement of the beam-search rule (include/janus.h janus_whisper_decode_beam_ex,
DESIGN.md §5k) over oracle.whisper.decoder_logits + apply_rules: the yardstick of the beam
tests. A helper module, not a conftest.

Per window, k = beam_size, patience 1:
  1. up to k live beams (tokens, cumulative score S, rule state = the sampled tokens), at
     most k finished hypotheses; only beam 0 is live at the first sampled position;
  2. lp_b = apply_rules(logits_b, sampled_b)[1];
  3. candidates (S_b + lp_b[v], b, v): the best 2k by (score descending, b, v);
  4. walked in order: eot -> finished (while fewer than k), else the next live beam until k
     are filled, then the walk stops;
  5. stop at k finished or at max_length (live beams closed at S / (n + 1)^length_penalty);
  6. the finished hypothesis with the best S / n^length_penalty wins (earliest on ties), the
     best closed live beam if none finished.
"""
import numpy as np

from oracle import whisper as ow


def top_candidates(scores, lps, n):
    """The best n candidates (score, b, v) of live beams with cumulative scores ``scores``
    and log-prob rows ``lps`` (-inf = not allowed), ordered by score descending, then b, then
    v. At most n per beam can be among them, so n per beam are gathered first."""
    cand = []
    for b, (S, lp) in enumerate(zip(scores, lps)):
        lp = np.asarray(lp, np.float64)
        ok = np.flatnonzero(np.isfinite(lp))
        if len(ok) > n:
            # n best of this beam by (lp descending, v): a stable sort on -lp keeps v ascending
            ok = ok[np.argsort(-lp[ok], kind="stable")[:n]]
        cand += [(float(S) + float(lp[v]), b, int(v)) for v in ok]
    cand.sort(key=lambda c: (-c[0], c[1], c[2]))
    return cand[:n]


def walk(cands, k, eot, n_finished):
    """Rule 4 over ordered candidates (the best 2k or more; only the first 2k are walked):
    returns (live [(b, v, score)], finished [(b, score)], consumed)."""
    live, fin, used = [], [], 0
    for (sc, b, v) in cands[:2 * k]:
        if len(live) >= k:
            break
        used += 1
        if v == eot:
            if n_finished + len(fin) < k:
                fin.append((b, sc))
        else:
            live.append((b, v, sc))
    return live, fin, used


def _norm(S, n, length_penalty):
    return S / float(n) ** length_penalty


def choose(finished, live, length_penalty=1.0):
    """Rule 6: (winner dict, final-choice margin). finished / live: dicts(tokens, sum_lp)."""
    pool = [dict(h, score=_norm(h["sum_lp"], len(h["tokens"]), length_penalty)) for h in finished]
    if not pool:
        pool = [dict(h, score=_norm(h["sum_lp"], len(h["tokens"]) + 1, length_penalty)) for h in live]
    best = 0
    for i in range(1, len(pool)):
        if pool[i]["score"] > pool[best]["score"]:
            best = i
    others = [p["score"] for i, p in enumerate(pool) if i != best]
    margin = pool[best]["score"] - max(others) if others else float("inf")
    return pool[best], margin


def beam_search(enc, W, cfg, tk, beam_size, max_length=448, prompts=None, length_penalty=1.0,
                no_speech=None, timestamps=True):
    """enc [windows][1500][d] -> per window a dict: winner (tokens incl. eot if it finished,
    sum_lp, score), finished [dict(tokens, sum_lp)], live (the beams standing at the end),
    margins [per-step decision margin: the last candidate the walk consumed minus the best it
    did not], final_margin, min_margin, nsp, stop_step (sampled steps run), n_finished."""
    enc = np.asarray(enc, np.float32)
    nw, k = len(enc), int(beam_size)
    suppress = tk.suppress_tokens()
    prompts = [list(tk.sot_sequence)] * nw if prompts is None else [list(p) for p in prompts]
    st = [dict(live=[dict(tokens=[], sum_lp=0.0)], finished=[], margins=[], nsp=0.0, done=False,
               steps=0) for _ in range(nw)]
    while True:
        # one forward over every live beam of every running window that still has room
        rows, owner = [], []
        for w in range(nw):
            if st[w]["done"]:
                continue
            if len(prompts[w]) + len(st[w]["live"][0]["tokens"]) >= max_length:
                st[w]["done"] = True
                continue
            for b, h in enumerate(st[w]["live"]):
                rows.append(prompts[w] + h["tokens"])
                owner.append((w, b))
        if not rows:
            break
        logits = {}
        for T in sorted({len(r) for r in rows}):
            idx = [i for i, r in enumerate(rows) if len(r) == T]
            out = ow.decoder_logits(np.array([rows[i] for i in idx]),
                                    enc[[owner[i][0] for i in idx]], W, cfg)[:, -1].numpy()
            for i, o in zip(idx, out):
                logits[owner[i]] = o
        for w in range(nw):
            s = st[w]
            if s["done"] or (w, 0) not in logits:
                continue
            if not s["live"][0]["tokens"] and no_speech is not None:
                raw = logits[(w, 0)].astype(np.float64)
                s["nsp"] = float(np.exp(raw[no_speech] - raw.max()) / np.exp(raw - raw.max()).sum())
            lps = [ow.apply_rules(logits[(w, b)], h["tokens"], tk, suppress, timestamps=timestamps)[1]
                   for b, h in enumerate(s["live"])]
            cands = top_candidates([h["sum_lp"] for h in s["live"]], lps, 2 * k + 1)
            live, fin, used = walk(cands, k, tk.eot, len(s["finished"]))
            if used < len(cands):
                s["margins"].append(cands[used - 1][0] - cands[used][0] if used else float("inf"))
            else:
                s["margins"].append(float("inf"))
            for (b, sc) in fin:
                s["finished"].append(dict(tokens=s["live"][b]["tokens"] + [tk.eot], sum_lp=sc))
            s["steps"] += 1
            if len(s["finished"]) >= k or not live:
                s["done"] = True        # the live beams stay as they stood
            else:
                s["live"] = [dict(tokens=s["live"][b]["tokens"] + [v], sum_lp=sc) for (b, v, sc) in live]
    out = []
    for s in st:
        winner, fm = choose(s["finished"], s["live"], length_penalty)
        out.append(dict(winner=winner, finished=s["finished"], live=s["live"], margins=s["margins"],
                        final_margin=fm, min_margin=min(s["margins"] + [fm]), nsp=s["nsp"],
                        stop_step=s["steps"], n_finished=len(s["finished"])))
    return out


def reachable_eot_weights(W, amount=9.0):
    """Synthetic weights never emit <|endoftext|>: a copy whose eot embedding row is raised
    along decoder.layer_norm.bias (logit[eot] grows by about amount * |bias|^2), rounded to
    fp16 as every engine matrix is."""
    from janus_amd import tokenizer as tok
    W = dict(W)
    E = W["decoder.embed_tokens.weight"].copy()
    E[tok.EOT] = (E[tok.EOT] + amount * W["decoder.layer_norm.bias"]).astype(np.float16).astype(np.float32)
    W["decoder.embed_tokens.weight"] = E
    return W


def rand_enc(cfg, seeds):
    """Random encoder rows, one seeded generator per window (so windows can be chosen one by
    one): fp16-rounded float32 [len(seeds)][n_audio_ctx][d_model]."""
    import torch
    rows = []
    for sd in seeds:
        g = torch.Generator().manual_seed(int(sd))
        rows.append((torch.randn(cfg.n_audio_ctx, cfg.d_model, generator=g) * 0.5).half())
    return torch.stack(rows).float().numpy()


# ------------------------------------------------------------------ the decode cases
# The decode tests' windows: random encoder rows by per-window seed, chosen on the CPU with
# this reference alone so that every window's smallest margin is >= 2 NEAR_TIE (4e-3), and
# for "tiny_eot" so that the finished list, the stop at k finished and a window reaching
# max_length with a partly filled list all occur. Their reference results are recorded in
# tests/golden/beam_refs.json by tests/golden/make_beam_refs.py (a CPU minute per case);
# reference(name) reads them, or computes them when the file has no such case.
SOT_PREV_PROMPTS = ([400, 1200, 3300, 770], [9000, 262])
CASES = {
    "tiny_k5": dict(model="tiny.en", wseed=5, k=5, max_length=20, seeds=[102, 104, 107, 110]),
    "tiny_k2": dict(model="tiny.en", wseed=5, k=2, max_length=16, seeds=[200, 202]),
    "tiny_k3": dict(model="tiny.en", wseed=5, k=3, max_length=16, seeds=[202, 203]),
    "tiny_k8": dict(model="tiny.en", wseed=5, k=8, max_length=10, seeds=[206, 209]),
    "base_k5": dict(model="base.en", wseed=7, k=5, max_length=12,
                    seeds=[400, 402, 403, 405, 406, 412, 414, 417, 418, 419, 422, 428, 430, 432]),
    "distil_k5": dict(model="distil-small.en", wseed=3, k=5, max_length=12, seeds=[501, 503]),
    "tiny_prompts": dict(model="tiny.en", wseed=5, k=5, max_length=20, seeds=[112, 300, 300, 115],
                         prev=[None, 0, 1, None]),
    "tiny_eot": dict(model="tiny.en", wseed=5, k=5, max_length=20, seeds=[100, 102, 104, 110],
                     eot_amount=9.0),
}
# (clip and max_length chosen the same way: both windows' margins >= 2 NEAR_TIE)
TRANSCRIBE_CASE = dict(model="tiny.en", wseed=0, k=5, max_length=16, audio_seed=176, seconds=33.0)
GOLDEN = "beam_refs.json"


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def case_inputs(name, tk):
    """(cfg, weights, enc [windows][1500][d] float32, prompts or None) of a decode case."""
    from janus_amd import tokenizer as tok
    from janus_amd.whisper import CONFIGS, synthetic_weights
    c = CASES[name]
    cfg = CONFIGS[c["model"]]
    W = synthetic_weights(cfg, seed=c["wseed"])
    if "eot_amount" in c:
        W = reachable_eot_weights(W, c["eot_amount"])
    prompts = None
    if "prev" in c:
        sot = list(tk.sot_sequence)
        prompts = [sot if p is None else [tok.SOT_PREV] + SOT_PREV_PROMPTS[p] + sot for p in c["prev"]]
    return cfg, W, rand_enc(cfg, c["seeds"]), prompts


def compute_case(name, tk):
    from janus_amd import tokenizer as tok
    c = CASES[name]
    cfg, W, enc, prompts = case_inputs(name, tk)
    ref = beam_search(enc, W, cfg, tk, c["k"], max_length=c["max_length"], prompts=prompts,
                      no_speech=tok.NO_SPEECH)
    return [dict(tokens=r["winner"]["tokens"], sum_lp=r["winner"]["sum_lp"], min_margin=r["min_margin"],
                 nsp=r["nsp"], n_finished=r["n_finished"], stop_step=r["stop_step"]) for r in ref]


def _golden():
    import json
    import os
    if not os.path.exists(golden_path()):
        return {}
    with open(golden_path()) as f:
        return json.load(f)


def reference(name, tk):
    """Per window of the case: dict(tokens, sum_lp, min_margin, nsp, n_finished, stop_step)."""
    g = _golden().get(name)
    if g is not None and g["case"] == CASES[name]:
        return g["windows"]
    return compute_case(name, tk)


def transcribe_audio():
    from janus_amd.workload import synth_speech
    c = TRANSCRIBE_CASE
    return synth_speech(c["audio_seed"], c["seconds"], sr=16000)


def compute_transcribe(tk):
    """The reference seek loop over beam decodes: faster-whisper's bookkeeping (the
    transcriber's _Stream / advance, themselves pinned to the oracle's loop by the greedy
    tests) driven by beam_search on the oracle's log-mel and encoder. Returns dict(windows =
    [dict(seek, size, prompt, tokens, avg, nsp, min_margin)], segments = [[start, end, tokens]])."""
    from janus_amd import tokenizer as tok
    from janus_amd.services import transcriber as tr
    from janus_amd.whisper import CONFIGS, mel_filters, synthetic_weights
    c = TRANSCRIBE_CASE
    cfg = CONFIGS[c["model"]]
    W = synthetic_weights(cfg, seed=c["wseed"])
    audio = transcribe_audio()
    feats = ow.logmel(audio, 1, mel_filters(), n_frames=None)
    s = tr._Stream(np.asarray(audio, np.float32))
    windows = []
    while s.active:
        seek, size, prompt = s.seek, s.window_size(), s.prompt(tk, c["max_length"])
        enc = ow.encoder(ow.window(feats, seek)[None], W, cfg).half().float().numpy()
        r = beam_search(enc, W, cfg, tk, c["k"], max_length=c["max_length"], prompts=[prompt],
                        no_speech=tok.NO_SPEECH)[0]
        toks = [t for t in r["winner"]["tokens"] if t != tk.eot]
        avg = r["winner"]["sum_lp"] / (len(toks) + 1)
        cand = tr.candidate(tk, toks, avg, r["nsp"], 0.0)
        tr.advance(tk, s, size, cand, cand, 0, len(r["winner"]["tokens"]))
        windows.append(dict(seek=seek, size=size, prompt=prompt, tokens=toks, avg=avg, nsp=r["nsp"],
                            min_margin=r["min_margin"]))
    return dict(windows=windows, segments=[[g.start, g.end, list(g.tokens)] for g in s.segments])


def transcribe_reference(tk):
    g = _golden().get("transcribe")
    if g is not None and g["case"] == TRANSCRIBE_CASE:
        return g
    return compute_transcribe(tk)
