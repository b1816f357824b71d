"""Reference for word-level timestamps (include/janus.h, janus_whisper_align).

CTranslate2's Whisper.align and faster-whisper are not available offline, so the rule the
build implements is restated here in numpy / python, independently of janus_amd's code:

* ``forward``: the teacher-forced decoder in fp32 torch (oracle.whisper's helpers), keeping
  every layer's cross-attention probabilities and the logits;
* ``attention_matrix``: rule 3 in float64 (normalise over rows, median of 7 along the frames
  with reflect padding, mean over heads, keep the text rows);
* ``dtw``: rule 4 in fp32, anti-diagonal by anti-diagonal; ``dtw_loop`` is the same rule as
  OpenAI's plain double loop; tests/test_align_host.py pins both to a brute-force minimum;
* ``token_probs``: rule 5 in float64;
* ``words_of`` / ``merge_punct`` / ``add_words`` / ``seek_loop``: rules 6 - 8 on the host.
"""
import string

import numpy as np
import torch

from oracle.whisper import _lin, _ln, _t

MEDIAN_WIDTH = 7
PREPEND = "\"'“¿([{-"
APPEND = "\"'.。,，!！?？:：”)]}、"
SENTENCE_END = ".。!！?？"


def default_heads(cfg):
    return [(l, h) for l in range(cfg.dec_layers // 2, cfg.dec_layers) for h in range(cfg.n_heads)]


def sequence(tk, text):
    return list(tk.sot_sequence) + [tk.no_timestamps] + [int(t) for t in text] + [tk.eot]


@torch.no_grad()
def forward(enc, seq, W, cfg):
    """enc [1500][d], seq [n] -> (cross-attention probabilities [layers][heads][n][1500]
    float32, logits [n][V] float32): oracle.whisper.decoder_logits with the attention kept."""
    enc = torch.as_tensor(np.asarray(enc, np.float32))[None]
    tokens = torch.as_tensor(np.asarray(seq, np.int64))[None]
    T = tokens.shape[1]
    H = cfg.n_heads
    hd = cfg.d_model // H
    x = _t(W, "decoder.embed_tokens.weight")[tokens] + _t(W, "decoder.embed_positions.weight")[:T]
    mask = torch.full((T, T), float("-inf")).triu(1)

    def mha(xq, xkv, p, m):
        q = _lin(xq, W, p + ".q_proj").view(1, -1, H, hd).transpose(1, 2)
        k = _lin(xkv, W, p + ".k_proj", bias=False).view(1, -1, H, hd).transpose(1, 2)
        v = _lin(xkv, W, p + ".v_proj").view(1, -1, H, hd).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)) / float(np.sqrt(hd))
        if m is not None:
            s = s + m
        pr = s.softmax(-1)
        o = (pr @ v).transpose(1, 2).reshape(1, -1, H * hd)
        return _lin(o, W, p + ".out_proj"), pr[0]

    probs = []
    for i in range(cfg.dec_layers):
        p = f"decoder.layers.{i}"
        h = _ln(x, W, p + ".self_attn_layer_norm")
        x = x + mha(h, h, p + ".self_attn", mask)[0]
        h = _ln(x, W, p + ".encoder_attn_layer_norm")
        o, pr = mha(h, enc, p + ".encoder_attn", None)
        probs.append(pr.numpy())
        x = x + o
        h = _ln(x, W, p + ".final_layer_norm")
        x = x + _lin(torch.nn.functional.gelu(_lin(h, W, p + ".fc1")), W, p + ".fc2")
    x = _ln(x, W, "decoder.layer_norm")
    logits = (x @ _t(W, "decoder.embed_tokens.weight").T)[0].numpy()
    return np.stack(probs), logits


def reduce_heads(P, sot_len):
    """Rule 3 on P [heads][n][F] (already cut to the frames kept): float64 A [n - sot_len - 1][F]."""
    P = np.asarray(P, np.float64)
    n, F = P.shape[1], P.shape[2]
    Z = (P - P.mean(axis=1, keepdims=True)) / P.std(axis=1, keepdims=True)
    if F > MEDIAN_WIDTH // 2:
        pad = MEDIAN_WIDTH // 2
        Zp = np.pad(Z, ((0, 0), (0, 0), (pad, pad)), mode="reflect")
        Z = np.median(np.lib.stride_tricks.sliding_window_view(Zp, MEDIAN_WIDTH, axis=2), axis=-1)
    return Z.mean(axis=0)[sot_len:n - 1]


def attention_matrix(probs, heads, size, sot_len):
    """probs [layers][heads][n][1500], heads [(layer, head)], size in mel frames -> A."""
    F = size // 2
    return reduce_heads(np.stack([probs[l][h][:, :F] for (l, h) in heads]), sot_len)


def token_probs(logits, seq, sot_len, eot):
    """Rule 5: p[r] for r < len(text), float64."""
    n = len(seq)
    out = []
    for r in range(n - sot_len - 2):
        row = np.asarray(logits[sot_len + r][:eot], np.float64)
        e = np.exp(row - row.max())
        out.append(e[seq[sot_len + 1 + r]] / e.sum())
    return np.array(out)


# ------------------------------------------------------------------ rule 4
def dtw_loop(x):
    """The rule as OpenAI's dtw_cpu writes it, a plain double loop, on x [N][F] in fp32:
    (text_indices, time_indices)."""
    x = np.asarray(x, np.float32)
    N, F = x.shape
    cost = np.full((N + 1, F + 1), np.inf, np.float32)
    trace = -np.ones((N + 1, F + 1), np.int8)
    cost[0, 0] = 0
    for j in range(1, F + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                t = 0
            elif c1 < c0 and c1 < c2:
                t = 1
            else:
                t = 2
            cost[i, j] = x[i - 1, j - 1] + min(c0, c1, c2)
            trace[i, j] = t
    return backtrace(trace)


def dtw(x, return_cost=False):
    """The same rule, one anti-diagonal at a time (every cell of a diagonal depends on the two
    before it only), so the large cases run in numpy vectors. The cost takes the true
    minimum of the three predecessors while the trace follows the strict comparisons, so on a
    tie c0 == c1 < c2 the trace says 2: cost[N][F] is always the optimum, the path is the
    optimum when no such tie occurs (any matrix of computed attention weights).
    ``return_cost``: cost[N][F] instead of the path."""
    x = np.asarray(x, np.float32)
    N, F = x.shape
    cost = np.full((N + 1, F + 1), np.inf, np.float32)
    trace = -np.ones((N + 1, F + 1), np.int8)
    cost[0, 0] = 0
    for k in range(2, N + F + 1):
        i = np.arange(max(1, k - F), min(N, k - 1) + 1)
        j = k - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        cost[i, j] = x[i - 1, j - 1] + np.minimum(np.minimum(c0, c1), c2)
        trace[i, j] = t
    if return_cost:
        return float(cost[N, F])
    return backtrace(trace)


def backtrace(trace):
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    trace = trace.copy()
    trace[0, :] = 2
    trace[:, 0] = 1
    out = []
    while i > 0 or j > 0:
        out.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        elif t == 2:
            j -= 1
        else:
            raise ValueError("unexpected trace")
    out = np.array(out[::-1], np.int64).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def path_cost(x, ti, fi):
    """Sum of x over the path's cells, float64."""
    return float(np.asarray(x, np.float64)[np.asarray(ti), np.asarray(fi)].sum())


def check_path_shape(ti, fi, N, F):
    ti, fi = np.asarray(ti), np.asarray(fi)
    assert len(ti) == len(fi) and len(ti) >= max(N, F) and len(ti) <= N + F
    assert (ti[0], fi[0]) == (0, 0) and (ti[-1], fi[-1]) == (N - 1, F - 1)
    dt, df = np.diff(ti), np.diff(fi)
    assert ((dt == 0) | (dt == 1)).all() and ((df == 0) | (df == 1)).all()
    assert ((dt + df) >= 1).all()


# ------------------------------------------------------------------ rules 6 - 8
def split_words(tk, tokens):
    """Rule 6's split: (words, word_tokens) of text + [eot]."""
    whole = tk.decode(tokens)
    pieces, cur, done = [], [], 0
    for t in tokens:
        cur = cur + [int(t)]
        s = tk.decode(cur)
        k = s.find("\ufffd")
        # no U+FFFD, or one the whole text carries at the same place (faster-whisper's test)
        if k == -1 or whole[done + k:done + k + 1] == "\ufffd":
            pieces.append((s, cur))
            done += len(s)
            cur = []
    words = []
    for s, toks in pieces:
        new = toks[0] >= tk.eot or s.startswith(" ") or s.strip() in string.punctuation or not words
        if new:
            words.append([s, list(toks)])
        else:
            words[-1][0] += s
            words[-1][1] += toks
    return [w for w, _ in words], [t for _, t in words]


def words_of(tk, text, ti, fi, probs):
    """Rule 6: [[word, tokens, start, end, probability]] of one window (window-relative s)."""
    if len(text) == 0:
        return []
    words, wtoks = split_words(tk, list(text) + [tk.eot])
    words, wtoks = words[:-1], wtoks[:-1]
    if not words:
        return []
    bounds = np.concatenate([[0], np.cumsum([len(t) for t in wtoks])]).astype(int)
    ti, fi = np.asarray(ti), np.asarray(fi)
    jumps = np.concatenate([[True], np.diff(ti) != 0])
    jump_times = fi[jumps] * 0.02
    probs = np.asarray(probs, np.float64)
    return [[w, list(t), float(jump_times[bounds[k]]), float(jump_times[bounds[k + 1]]),
             float(probs[bounds[k]:bounds[k + 1]].mean())]
            for k, (w, t) in enumerate(zip(words, wtoks))]


def merge_punct(al, prepend=PREPEND, append=APPEND):
    """merge_punctuations on [[word, tokens, ...]] rows, in place."""
    j = len(al) - 1
    for i in range(len(al) - 2, -1, -1):
        if al[i][0].startswith(" ") and al[i][0].strip() in prepend:
            al[j][0] = al[i][0] + al[j][0]
            al[j][1] = al[i][1] + al[j][1]
            al[i][0], al[i][1] = "", []
        else:
            j = i
    i = 0
    for j in range(1, len(al)):
        if not al[i][0].endswith(" ") and al[j][0] in append:
            al[i][0] = al[i][0] + al[j][0]
            al[i][1] = al[i][1] + al[j][1]
            al[j][0], al[j][1] = "", []
        else:
            i = j


def add_words(tk, segs, al, seek, last_speech, prepend=PREPEND, append=APPEND, taken=None):
    """Rule 7 over one window: segs [[start, end, tokens]] (absolute s) -> (segs with start /
    end moved, words per segment [(word, start, end, probability)], new last_speech).
    ``taken`` (a list, optional) collects the names of the branches that fired."""
    taken = [] if taken is None else taken
    dur = np.array([w[3] - w[2] for w in al])
    dur = dur[dur != 0]
    median = min(0.7, float(np.median(dur))) if len(dur) else 0.0
    mx = 2 * median
    for i in range(1, len(al)):
        if al[i][3] - al[i][2] > mx:
            if al[i][0] in SENTENCE_END:
                al[i][3] = al[i][2] + mx
                taken.append("sentence_end_self")
            elif al[i - 1][0] in SENTENCE_END:
                al[i][2] = al[i][3] - mx
                taken.append("sentence_end_prev")
    merge_punct(al, prepend, append)
    t0 = seek * 0.01
    k = 0
    out_words = []
    for seg in segs:
        ntext = len([t for t in seg[2] if t < tk.eot])
        saved, ws = 0, []
        while k < len(al) and saved < ntext:
            w = al[k]
            if w[0]:
                ws.append([w[0], round(t0 + w[2], 2), round(t0 + w[3], 2), w[4]])
            saved += len(w[1])
            k += 1
        if ws:
            if ws[0][2] - last_speech > 4 * median and (
                    ws[0][2] - ws[0][1] > mx or (len(ws) >= 2 and ws[1][2] - ws[0][1] > 2 * mx)):
                taken.append("pause")
                if len(ws) >= 2 and ws[1][2] - ws[1][1] > mx:
                    b = max(ws[1][2] / 2, ws[1][2] - mx)
                    ws[0][2] = ws[1][1] = b
                    taken.append("pause_second")
                ws[0][1] = max(0, ws[0][2] - mx)
            if seg[0] < ws[0][2] and seg[0] - 0.5 > ws[0][1]:
                ws[0][1] = max(0, min(ws[0][2] - median, seg[0]))
                taken.append("segment_start")
            else:
                seg[0] = ws[0][1]
            if seg[1] > ws[-1][1] and seg[1] + 0.5 < ws[-1][2]:
                ws[-1][2] = max(ws[-1][1] + median, seg[1])
                taken.append("segment_end")
            else:
                seg[1] = ws[-1][2]
            last_speech = seg[1]
        out_words.append([tuple(w) for w in ws])
    return segs, out_words, last_speech


def split_tokens(tk, toks, seek, size):
    """generate_segments' slicing of one window's tokens: ([[start, end, tokens]], next seek,
    single_timestamp_ending)."""
    tb = tk.timestamp_begin
    t0 = seek * 0.01
    single = len(toks) >= 2 and toks[-2] < tb <= toks[-1]
    cons = [i for i in range(1, len(toks)) if toks[i] >= tb and toks[i - 1] >= tb]
    segs = []
    if cons:
        last = 0
        for c in cons + ([len(toks)] if single else []):
            part = toks[last:c]
            segs.append([t0 + (part[0] - tb) * 0.02, t0 + (part[-1] - tb) * 0.02, part])
            last = c
        nseek = seek + size if single else seek + (toks[last - 1] - tb) * 2
    else:
        st = [t for t in toks if t >= tb]
        d = (st[-1] - tb) * 0.02 if st and st[-1] != tb else size * 0.01
        segs.append([t0, t0 + d, toks])
        nseek = seek + size
    if nseek <= seek:
        nseek = seek + size
    return segs, nseek, single


def seek_loop(tk, content_frames, windows, prepend=PREPEND, append=APPEND, complete=True):
    """The seek loop with word timestamps over given window results: windows [(tokens without
    eot, avg_logprob, no_speech_prob, alignment or None)] in order, alignment with
    text_indices / time_indices / token_probs. Returns (seeks [(seek, size, next seek)],
    segments [(seek, start, end, tokens, words)]). ``complete``: the windows must take the seek
    to the end of the content."""
    seek, last_speech, seeks, out = 0, 0.0, [], []
    for toks, avg, nsp, al in windows:
        assert seek < content_frames
        size = min(3000, content_frames - seek)
        if nsp > 0.6 and not avg > -1.0:
            seeks.append((seek, size, seek + size))
            seek += size
            continue
        segs, nseek, single = split_tokens(tk, list(toks), seek, size)
        text = [t for s in segs for t in s[2] if t < tk.eot]
        rows = words_of(tk, text, al.text_indices, al.time_indices, al.token_probs) if al is not None else []
        segs, words, last_speech = add_words(tk, segs, rows, seek, last_speech, prepend, append)
        if not single:                                     # rule 8
            ends = [w[2] for ws in words for w in ws]
            if ends and ends[-1] > seek * 0.01:
                nseek = round(ends[-1] * 100)
        for s, ws in zip(segs, words):
            if s[0] == s[1] or not tk.decode(s[2]).strip():
                continue
            out.append((seek, s[0], s[1], s[2], ws))
        seeks.append((seek, size, nseek))
        seek = nseek
    assert seek >= content_frames or not complete
    return seeks, out
