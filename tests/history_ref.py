"""Numpy restatement of the history rules (include/janus.h janus_decode_options: repetition
penalty and no-repeat n-grams) on top of the unchanged oracle: the yardstick of
the decoding-option tests. A helper module, not a conftest.

oracle.whisper.greedy_cached looks apply_rules up at module level, so ``history_rules`` wraps
it for the length of a ``with`` block: penalise the logits of the tokens sampled so far (fp32),
extend the suppress list by the banned tokens, call the original. The raw statistics
(no_speech_prob) are taken by greedy_cached before apply_rules, so they stay unpenalised, and
its margins are the top-2 gaps of the penalised, filtered keys.

For one row, g = the tokens sampled in this call (timestamps included, the prompt not), m = len(g):
  1. penalty p: every distinct t of g gets logit[t] * p if logit[t] < 0 else logit[t] / p;
  2. n-grams: { g[i+n-1] : 0 <= i <= m-n, g[i .. i+n-2] == g[m-n+1 .. m-1] } are banned.
"""
import contextlib
import json
import os

import numpy as np

from oracle import whisper as ow

NEAR_TIE = 2e-3
MIN_MARGIN = 2 * NEAR_TIE          # every reference decision is at least this clear
OPTION_SETS = [(1.3, 0), (1.0, 3), (1.2, 2)]      # (repetition_penalty, no_repeat_ngram_size)
T_SAMPLE = 0.6
BEST_OF = 5
ML = 20                         # max_length of every decode case
GOLDEN = "history_refs.json"


def penalise(logits, sampled, p):
    """Rule 1 in fp32 (a copy)."""
    L = np.array(logits, np.float32)
    idx = sorted(set(int(t) for t in sampled))
    if idx and p != 1.0:
        v = L[idx]
        L[idx] = np.where(v < 0, v * np.float32(p), v / np.float32(p))
    return L


def banned(sampled, n):
    """Rule 2: the sorted banned tokens."""
    g = [int(t) for t in sampled]
    m = len(g)
    if n <= 0 or m < n:
        return []
    suffix = g[m - n + 1:]
    return sorted({g[i + n - 1] for i in range(m - n + 1) if g[i:i + n - 1] == suffix})


@contextlib.contextmanager
def history_rules(p=1.0, n=0, prefix=()):
    """oracle.whisper.apply_rules with the history rules in front, inside the block.
    ``prefix``: tokens counted as sampled before the row's own (only to show that a result
    depends on the prompt NOT being part of g: the generator's check)."""
    orig = ow.apply_rules

    def wrapped(logits, sampled, tk, suppress, **kw):
        g = list(prefix) + list(sampled)
        return orig(penalise(logits, g, p), sampled, tk, list(suppress) + banned(g, n), **kw)
    ow.apply_rules = wrapped
    try:
        yield
    finally:
        ow.apply_rules = orig


def first_difference(a, b):
    """Index of the first differing element of two lists (None: equal)."""
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i
    return None if len(a) == len(b) else min(len(a), len(b))


def decode(enc, W, cfg, tk, p, n, max_length=ML, prompts=None, temperature=0.0, seeds=None, prefix=()):
    """greedy_cached under the rules: per row dict(tokens, margins, sum_lp, nsp)."""
    with history_rules(p, n, prefix):
        return ow.greedy_cached(enc, W, cfg, tk, max_length, prompts=prompts, no_speech=tk.no_speech,
                                temperature=temperature, seeds=seeds)


# ------------------------------------------------------------------ the decode cases
# Per model and option set: greedy base rows (random encoder rows by seed, the start sequence
# as prompt), prompt rows (encoder rows of their own under <|startofprev|> prompts of different
# lengths; the last one's prompt holds ``winner``, tokens of which its row goes on to sample) and
# sampled rows (T = 0.6, BEST_OF noise seeds on each of two encoder rows). Every seed was chosen
# on the CPU with this reference alone so that each row's smallest top-2 margin of the
# penalised keys is >= MIN_MARGIN; tests/golden/make_history_refs.py asserts that again, and
# that the case differs from the same decode without options (check_case: every form under a
# penalty, the greedy rows under n-grams alone).
MODELS = {
    "tiny": dict(model="tiny.en", wseed=5),
    "cut": dict(model="large-cut", wseed=11),
}


def model_cfg(name):
    from janus_amd.whisper import CONFIGS
    if MODELS[name]["model"] == "large-cut":
        import large_family_ref as lf
        return lf.CUT
    return CONFIGS[MODELS[name]["model"]]


def tokenizer_for(cfg):
    from janus_amd import tokenizer as tok
    return tok.WhisperTokenizer(n_vocab=cfg.n_vocab) if cfg.multilingual else tok.WhisperTokenizer()


def weights(name):
    from janus_amd.whisper import synthetic_weights
    return synthetic_weights(model_cfg(name), seed=MODELS[name]["wseed"])


def opt_key(p, n):
    return f"p{p:g}_n{n}"


# case name -> greedy / prompt rows' encoder seeds, the third prompt's tokens, the sampled rows'
# encoder seeds and BEST_OF noise seeds on each
SEEDS = {
    "tiny_p1.3_n0": dict(greedy=[100, 101, 103, 104], prompt_enc=[301, 401, 500],
                         winner=[49247, 27365, 14543, 5096, 28398], sample_enc=[100, 101],
                         sample_noise=[[3000, 3001, 3002, 3003, 3005], [3000, 3001, 3002, 3003, 3004]]),
    "tiny_p1_n3": dict(greedy=[100, 103, 104, 105], prompt_enc=[301, 400, 510],
                       winner=[27865, 43425, 31167, 23718, 10199, 15833], sample_enc=[100, 103],
                       sample_noise=[[3000, 3001, 3002, 3003, 3005], [3000, 3001, 3002, 3003, 3004]]),
    "tiny_p1.2_n2": dict(greedy=[100, 101, 103, 104], prompt_enc=[301, 401, 500],
                         winner=[23271, 13765, 35797, 43615, 19720, 35399], sample_enc=[100, 101],
                         sample_noise=[[3000, 3001, 3002, 3003, 3005], [3000, 3001, 3002, 3003, 3004]]),
    "cut_p1.3_n0": dict(greedy=[100, 101, 102, 103], prompt_enc=[300, 400, 500], winner=[16511, 262],
                        sample_enc=[100, 101],
                        sample_noise=[[3000, 3001, 3002, 3003, 3004], [3001, 3002, 3004, 3006, 3007]]),
    "cut_p1_n3": dict(greedy=[100, 101, 103, 104], prompt_enc=[300, 400, 500], winner=[16511, 262],
                      sample_enc=[100, 101],
                      sample_noise=[[3016, 3001, 3002, 3003, 3004], [3001, 3002, 3004, 3005, 3006]]),
    "cut_p1.2_n2": dict(greedy=[100, 101, 102, 103], prompt_enc=[300, 400, 503], winner=[16511, 262],
                        sample_enc=[100, 101],
                        sample_noise=[[3000, 3001, 3002, 3003, 3004], [3001, 3002, 3004, 3005, 3006]]),
}


def prompt_rows(tk, winner):
    """The prompt rows' prompts: lengths differ; the last holds the tokens ``winner``."""
    sot = list(tk.sot_sequence)
    return [[tk.sot_prev, 400, 1200, 3300, 770] + sot, [tk.sot_prev, 9000] + sot,
            [tk.sot_prev] + [int(t) for t in winner] + sot]


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def _golden():
    if not os.path.exists(golden_path()):
        return {}
    with open(golden_path()) as f:
        return json.load(f)


def case_name(model, p, n):
    return f"{model}_{opt_key(p, n)}"


def compute_case(model, p, n):
    """dict(seeds, greedy=[row], prompts=[[ids]], prompt=[row], sampled=[row], plain_*): rows are
    dict(tokens, sum_lp, nsp, min_margin); plain_* the same decodes without options (tokens only)."""
    import beam_ref
    cfg, W = model_cfg(model), weights(model)
    tk = tokenizer_for(cfg)
    sd = SEEDS[case_name(model, p, n)]

    def rows(out):
        return [dict(tokens=r["tokens"], sum_lp=r["sum_lp"], nsp=r["nsp"], min_margin=min(r["margins"]))
                for r in out]
    enc_g = beam_ref.rand_enc(cfg, sd["greedy"])
    sot = [list(tk.sot_sequence)] * len(sd["greedy"])
    greedy = decode(enc_g, W, cfg, tk, p, n, prompts=sot)
    plain_g = decode(enc_g, W, cfg, tk, 1.0, 0, prompts=sot)
    prompts = prompt_rows(tk, sd["winner"])
    enc_p = beam_ref.rand_enc(cfg, sd["prompt_enc"])
    prow = decode(enc_p, W, cfg, tk, p, n, prompts=prompts)
    plain_p = decode(enc_p, W, cfg, tk, 1.0, 0, prompts=prompts)
    # the prompt is not part of g: counting the winner's prompt as sampled changes its row
    wrong = decode(enc_p[2:3], W, cfg, tk, p, n, prompts=prompts[2:3], prefix=prompts[2][1:1 + len(sd["winner"])])
    enc_s = beam_ref.rand_enc(cfg, sd["sample_enc"])
    eidx = [e for e in range(len(sd["sample_enc"])) for _ in range(BEST_OF)]
    noise = [s for e in sd["sample_noise"] for s in e]
    sp = [list(tk.sot_sequence)] * len(eidx)
    sampled = decode(enc_s[eidx], W, cfg, tk, p, n, prompts=sp, temperature=T_SAMPLE, seeds=noise)
    plain_s = decode(enc_s[eidx], W, cfg, tk, 1.0, 0, prompts=sp, temperature=T_SAMPLE, seeds=noise)
    return dict(seeds=sd, greedy=rows(greedy), prompts=prompts, prompt=rows(prow), sampled=rows(sampled),
                plain_greedy=[r["tokens"] for r in plain_g], plain_prompt=[r["tokens"] for r in plain_p],
                plain_sampled=[r["tokens"] for r in plain_s], prompt_in_history=wrong[0]["tokens"])


def check_case(c, p):
    """The generator's assertions on one computed case (CPU only)."""
    for form in ("greedy", "prompt", "sampled"):
        for b, r in enumerate(c[form]):
            assert r["min_margin"] >= MIN_MARGIN, (form, b, r["min_margin"])
        # the greedy rows always differ from the decode without options, and every form under a
        # penalty; n-grams alone need a row that repeats an n-gram inside ML tokens, which the
        # sampled tiny.en rows never do (220 noise seeds tried): those rows are recorded as they are
        if form == "greedy" or p != 1.0:
            assert [r["tokens"] for r in c[form]] != c["plain_" + form], form
    w = c["prompt"][2]["tokens"]
    assert set(c["seeds"]["winner"]) & set(w), "the winner's row samples none of its prompt's tokens"
    if p != 1.0:   # (n-grams alone: a prompt this short seldom completes a ban)
        assert c["prompt_in_history"] != w, "the winner's row does not depend on the prompt staying out of g"


def reference(model, p, n):
    g = _golden().get(case_name(model, p, n))
    if g is not None and g["seeds"] == SEEDS.get(case_name(model, p, n)):
        return g
    return compute_case(model, p, n)


# ------------------------------------------------------------------ the seek loop
# (clip, options and max_length chosen the same way: every window's margins >= MIN_MARGIN)
TRANSCRIBE_CASE = dict(model="tiny.en", wseed=0, audio_seed=179, seconds=33.0, max_length=24,
                       repetition_penalty=1.3, no_repeat_ngram_size=3, initial_prompt="ba di",
                       hotwords=[700, 1500, 2600], condition_on_previous_text=False)


def transcribe_audio():
    from janus_amd.workload import synth_speech
    c = TRANSCRIBE_CASE
    return synth_speech(c["audio_seed"], c["seconds"], sr=16000)


def compute_transcribe(tk, options=True):
    """The reference seek loop at T = 0: the transcriber's own bookkeeping (_Stream / advance,
    pinned to the oracle's loop by the greedy tests) driven by ``decode`` on the oracle's
    log-mel and encoder. ``options=False``: the same clip without any option. Returns
    dict(windows=[dict(seek, size, prompt, tokens, avg, nsp, min_margin)], segments=[[start,
    end, tokens]])."""
    from janus_amd.services import transcriber as tr
    from janus_amd.whisper import CONFIGS, mel_filters, synthetic_weights
    c = TRANSCRIBE_CASE
    cfg = CONFIGS[c["model"]]
    W = synthetic_weights(cfg, seed=c["wseed"])
    audio = transcribe_audio()
    feats = ow.logmel(audio, 1, mel_filters(), n_frames=None)
    s = tr._Stream(np.asarray(audio, np.float32))
    p, n, cond = 1.0, 0, True
    if options:
        p, n, cond = c["repetition_penalty"], c["no_repeat_ngram_size"], c["condition_on_previous_text"]
        s.all_tokens.extend(tr.encode_prompt(tk, c["initial_prompt"]))
        s.hotwords = tr.encode_prompt(tk, c["hotwords"])
    windows = []
    while s.active:
        seek, size, prompt = s.seek, s.window_size(), s.prompt(tk, c["max_length"])
        enc = ow.encoder(ow.window(feats, seek)[None], W, cfg).half().float().numpy()
        r = decode(enc, W, cfg, tk, p, n, max_length=c["max_length"], prompts=[prompt])[0]
        toks = [t for t in r["tokens"] if t != tk.eot]
        avg = r["sum_lp"] / (len(toks) + 1)
        cand = tr.candidate(tk, toks, avg, r["nsp"], 0.0)
        tr.advance(tk, s, size, cand, cand, 0, len(r["tokens"]), condition_on_previous_text=cond)
        windows.append(dict(seek=seek, size=size, prompt=prompt, tokens=toks, avg=avg, nsp=r["nsp"],
                            min_margin=min(r["margins"])))
    return dict(windows=windows, segments=[[g.start, g.end, list(g.tokens)] for g in s.segments])


def transcribe_reference(tk):
    g = _golden().get("transcribe")
    if g is not None and g["case"] == TRANSCRIBE_CASE:
        return g
    r = compute_transcribe(tk)
    r["plain_segments"] = compute_transcribe(tk, options=False)["segments"]
    return r
