"""Whisper token spaces (English-only and multilingual) and detokenisation (host side).

Special-token layout of the ``*.en`` Whisper vocabulary (51 864 ids; GPT-2 byte-level
BPE in 0..50255): <|endoftext|> 50256, <|startoftranscript|> 50257, 99 language tokens,
<|translate|> 50357, <|transcribe|> 50358, <|startoflm|> 50359, <|startofprev|> 50360,
<|nocaptions|> 50361, <|notimestamps|> 50362, timestamps <|0.00|>..<|30.00|> from 50363.

The multilingual vocabulary (tiny / base / small; 51 865 ids) has one more BPE token, so
every special id sits one higher: <|endoftext|> 50257, <|startoftranscript|> 50258, the 99
language tokens 50259..50357, <|translate|> 50358, <|transcribe|> 50359, <|startoflm|> 50360,
<|startofprev|> 50361, <|nospeech|> 50362, <|notimestamps|> 50363, timestamps from 50364; its
start sequence is [sot, <|language|>, <|task|>].

The large-v3 vocabulary (large-v3 / large-v3-turbo / distil-large-v3; 51 866 ids) has one more
language, <|yue|>, appended to the 99: <|startoftranscript|> 50258, the 100 language tokens
50259..50358, <|translate|> 50359, <|transcribe|> 50360, <|startoflm|> 50361, <|startofprev|>
50362, <|nospeech|> 50363, <|notimestamps|> 50364, timestamps from 50365.

No tokenizer files exist offline. If ``JANUS_WHISPER_DIR`` holds a Hugging Face
``tokenizer.json``, it is used through the ``tokenizers`` package; otherwise a
deterministic synthetic vocabulary of the same size is used: ids 0..255 are the 256
GPT-2 byte symbols (so id 220 is " " exactly as in GPT-2) and ids 256..50255 are seeded
pseudo-words, ~70 % with a leading space like BPE "Ġ" tokens.

Segment assembly follows faster-whisper's greedy path for one window
(``_split_segments_by_timestamps`` + ``' '.join(seg.text.strip())``,
transcriber.py:59-64).
"""
import os

import numpy as np

EOT = 50256
SOT = 50257
TRANSLATE = 50357
TRANSCRIBE = 50358
SOT_LM = 50359
SOT_PREV = 50360
NO_SPEECH = 50361
NO_TIMESTAMPS = 50362
TIMESTAMP_BEGIN = 50363
N_VOCAB_EN = 51864
N_VOCAB_MULTILINGUAL = 51865
N_VOCAB_V3 = 51866
BLANK = 220

# the 99 language tokens in openai/whisper's order (tokenizer.LANGUAGES)
LANGUAGES = ("en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu "
             "ta no th ur hr bg lt la mi ml cy sk te fa lv bn sr az sl kn et mk br eu is hy ne mn bs "
             "kk sq sw gl mr pa si km sn yo so af oc ka be tg sd gu am yi lo uz fo ht ps tk nn mt sa "
             "lb my bo tl mg as tt haw ln ha ba jw su").split()
# the large-v3 family's 100: the same order with Cantonese appended
LANGUAGES_V3 = LANGUAGES + ["yue"]
TASKS = ("transcribe", "translate")
# languages written without spaces: words are the unicode pieces (faster-whisper's
# Tokenizer.split_to_word_tokens)
UNSPACED_LANGUAGES = frozenset({"zh", "ja", "th", "lo", "my", "yue"})

# openai/whisper tokenizer.non_speech_tokens symbol set
_SYMBOLS = list("\"#()*+/:;<=>@[\\]^_`{|}~「」『』") + \
    "<< >> <<< >>> -- --- -( -[ (' (\" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪".split()
_MISC = set("♩♪♫♬♭♮♯")


def bytes_to_unicode_order():
    """GPT-2's byte order: id k < 256 is byte order[k]."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + \
        list(range(ord("®"), ord("ÿ") + 1))
    rest = [b for b in range(256) if b not in bs]
    return bs + rest


class WhisperTokenizer:
    """One token space: ``multilingual=False`` the ``*.en`` ids (the module constants),
    ``multilingual=True`` the 51 865-entry vocabulary with every special id one higher and
    the start sequence [sot, <|language|>, <|task|>]. ``n_vocab`` (None: from
    ``multilingual``) names the layout outright: 51 864, 51 865 or 51 866 — the large-v3
    layout, multilingual with 100 languages, so every id past them one higher again."""

    def __init__(self, path: str = None, seed: int = 1234, multilingual: bool = False,
                 language: str = "en", task: str = "transcribe", n_vocab: int = None):
        if n_vocab is None:
            n_vocab = N_VOCAB_MULTILINGUAL if multilingual else N_VOCAB_EN
        if n_vocab not in (N_VOCAB_EN, N_VOCAB_MULTILINGUAL, N_VOCAB_V3):
            raise ValueError(f"no token layout for a vocabulary of {n_vocab}")
        self.multilingual = n_vocab != N_VOCAB_EN
        self.languages = LANGUAGES_V3 if n_vocab == N_VOCAB_V3 else LANGUAGES
        up = 1 if self.multilingual else 0
        up2 = up + (1 if n_vocab == N_VOCAB_V3 else 0)   # ids past the language tokens
        self.eot, self.sot = EOT + up, SOT + up
        self.translate, self.transcribe = TRANSLATE + up2, TRANSCRIBE + up2
        self.sot_lm, self.sot_prev = SOT_LM + up2, SOT_PREV + up2
        self.no_speech = NO_SPEECH + up2
        self.no_timestamps = NO_TIMESTAMPS + up2
        self.timestamp_begin = TIMESTAMP_BEGIN + up2
        self.language_begin = self.sot + 1
        self.n_languages = len(self.languages)
        self.n_vocab = n_vocab
        self.blank = BLANK
        self.language, self.task = language, task
        # *.en: no language / task tokens
        self.sot_sequence = self.sot_sequence_for(language, task)
        self._hf = None
        if path and os.path.exists(os.path.join(path, "tokenizer.json")):
            from tokenizers import Tokenizer
            self._hf = Tokenizer.from_file(os.path.join(path, "tokenizer.json"))
            # the decoder's prompt and rules use this layout's special-token ids: the file must agree
            layout = ("large-v3" if n_vocab == N_VOCAB_V3 else "multilingual") if self.multilingual else "*.en"
            names = [("<|endoftext|>", self.eot), ("<|startoftranscript|>", self.sot),
                     ("<|startofprev|>", self.sot_prev), ("<|notimestamps|>", self.no_timestamps)]
            if n_vocab == N_VOCAB_V3:   # the ids the 100th language moved
                names += [("<|yue|>", self.language_begin + 99), ("<|translate|>", self.translate),
                          ("<|transcribe|>", self.transcribe), ("<|nospeech|>", self.no_speech)]
            for name, want in names:
                got = self._hf.token_to_id(name)
                if got != want:
                    raise ValueError(f"tokenizer.json: {name} is {got}, expected {want} ({layout} layout)")
            ts0 = self._hf.token_to_id("<|0.00|>")
            if ts0 is not None and ts0 != self.timestamp_begin:
                raise ValueError(f"tokenizer.json: <|0.00|> is {ts0}, expected {self.timestamp_begin}")
        else:
            self._table = self._synthetic_table(seed, self.eot)

    # ---- language / task tokens
    def language_token(self, code: str) -> int:
        """<|code|>'s id; ValueError for a code that is none of this layout's languages."""
        if not isinstance(code, str) or code not in self.languages:
            raise ValueError(f"unknown language code {code!r}")
        return self.language_begin + self.languages.index(code)

    def supported_languages(self):
        """The codes this layout has tokens for: 99, 100 (large-v3), or ["en"] for ``*.en``."""
        return list(self.languages) if self.multilingual else ["en"]

    def language_code(self, token: int) -> str:
        i = int(token) - self.language_begin
        if not 0 <= i < self.n_languages:
            raise ValueError(f"token {token} is no language token")
        return self.languages[i]

    def task_token(self, task: str) -> int:
        if task not in TASKS:
            raise ValueError(f"unknown task {task!r}: one of {TASKS}")
        return self.transcribe if task == "transcribe" else self.translate

    def sot_sequence_for(self, language: str = "en", task: str = "transcribe"):
        """The start sequence of one utterance: [sot] for ``*.en``, else
        [sot, <|language|>, <|task|>]. ValueError for an unknown code or task."""
        lang, tk = self.language_token(language), self.task_token(task)
        return [self.sot, lang, tk] if self.multilingual else [self.sot]

    @staticmethod
    def _synthetic_table(seed, n=EOT):
        """ids 0 .. n - 1: the multilingual table (n = 50257) draws the *.en table's words
        from the same stream and then one more."""
        order = bytes_to_unicode_order()
        table = [bytes([order[k]]) for k in range(256)]
        rng = np.random.default_rng(seed)
        cons = list("bcdfghjklmnprstvwz")
        vows = list("aeiou")
        for _ in range(256, n):
            n = int(rng.integers(1, 4))
            word = "".join(cons[rng.integers(len(cons))] + vows[rng.integers(len(vows))]
                           for _ in range(n))
            if rng.random() < 0.7:
                word = " " + word
            table.append(word.encode())
        return table

    def encode_text(self, text: str):
        if self._hf is not None:
            return self._hf.encode(text, add_special_tokens=False).ids
        order = bytes_to_unicode_order()
        inv = {b: k for k, b in enumerate(order)}
        return [inv[b] for b in text.encode("utf-8")]

    def decode(self, tokens) -> str:
        a = np.asarray(tokens, dtype=np.int64).reshape(-1)
        toks = a[(a >= 0) & (a < self.eot)].tolist()   # text tokens only (vectorised filter)
        if self._hf is not None:
            return self._hf.decode(toks)
        return b"".join(map(self._table.__getitem__, toks)).decode("utf-8", errors="replace")

    def non_speech_tokens(self):
        if self._hf is None:
            order = bytes_to_unicode_order()
            inv = {b: k for k, b in enumerate(order)}
            out = set()
            for sym in _SYMBOLS:
                b = sym.encode("utf-8")
                out.add(inv[b[0]])
            return sorted(out)
        out = {self.encode_text(" -")[0], self.encode_text(" '")[0]}
        for sym in _SYMBOLS + sorted(_MISC):
            for tokens in (self.encode_text(sym), self.encode_text(" " + sym)):
                if len(tokens) == 1 or sym in _MISC:
                    out.add(tokens[0])
        return sorted(out)

    def suppress_tokens(self):
        """faster-whisper get_suppressed_tokens(tokenizer, [-1])."""
        s = set(self.non_speech_tokens())
        s.update([self.transcribe, self.translate, self.sot, self.sot_prev, self.sot_lm])
        return sorted(s)

    def split_to_word_tokens(self, tokens, language=None):
        """faster-whisper's Tokenizer.split_to_word_tokens (split_tokens_on_spaces over
        split_tokens_on_unicode; for ``language`` in zh ja th lo my yue, written without
        spaces, the unicode split alone): (words, word_tokens). First the tokens are cut where
        the incremental decode of the tokens gathered so far holds no U+FFFD (a multi-byte
        character split over tokens stays in one piece) — or holds one that the decode of the
        whole sequence has at the same place, i.e. the text itself carries it (bytes that
        are no UTF-8 at all); then a piece starts a new word when its first token is >= eot,
        or it starts with a space, or its stripped text is in string.punctuation, or it is
        the first piece — otherwise it is appended to the previous word. Works on the table
        vocabulary and on a tokenizer.json alike (both decode ids >= eot to nothing)."""
        import string
        full = self.decode(tokens)
        pieces, piece_tokens, cur, offset = [], [], [], 0
        for t in tokens:
            cur.append(int(t))
            text = self.decode(cur)
            at = text.find("\ufffd")
            if at < 0 or (offset + at < len(full) and full[offset + at] == "\ufffd"):
                pieces.append(text)
                piece_tokens.append(cur)
                cur = []
                offset += len(text)
        if language in UNSPACED_LANGUAGES:
            return pieces, [list(t) for t in piece_tokens]
        words, word_tokens = [], []
        for text, toks in zip(pieces, piece_tokens):
            special = toks[0] >= self.eot
            with_space = text.startswith(" ")
            punctuation = text.strip() in string.punctuation
            if special or with_space or punctuation or not words:
                words.append(text)
                word_tokens.append(list(toks))
            else:
                words[-1] = words[-1] + text
                word_tokens[-1].extend(toks)
        return words, word_tokens

    def segments(self, sampled):
        """Split sampled tokens (up to, excluding, <|endoftext|>) the way faster-whisper's
        single-window greedy path does; returns list of (start_ts, end_ts, text)."""
        toks = []
        for t in sampled:
            t = int(t)
            if t == self.eot or t < 0:
                break
            toks.append(t)
        tb = self.timestamp_begin
        single_ending = len(toks) >= 2 and toks[-2] < tb <= toks[-1]
        consecutive = [i for i in range(1, len(toks)) if toks[i] >= tb and toks[i - 1] >= tb]
        segs = []
        if consecutive:
            slices = list(consecutive)
            if single_ending:
                slices.append(len(toks))
            last = 0
            for cur in slices:
                part = toks[last:cur]
                segs.append(self._seg(part))
                last = cur
            if last < len(toks):  # single window: keep the trailing partial segment
                segs.append(self._seg(toks[last:]))
        else:
            segs.append(self._seg(toks))
        return segs

    def _seg(self, part):
        ts = [t for t in part if t >= self.timestamp_begin]
        start = (ts[0] - self.timestamp_begin) * 0.02 if ts else 0.0
        end = (ts[-1] - self.timestamp_begin) * 0.02 if ts else 0.0
        return (start, end, self.decode(part))

    def transcript(self, sampled) -> str:
        if self._hf is None:
            return self._transcript_table(sampled)
        parts = [text.strip() for (_, _, text) in self.segments(sampled)]
        return " ".join(parts).strip()

    def _transcript_table(self, sampled) -> str:
        """transcript() for the table vocabulary with numpy index work (same segments,
        same text): the per-token Python loop cost ~0.4 ms per 447-token row."""
        if getattr(self, "_table_np", None) is None:
            self._table_np = np.empty(len(self._table), dtype=object)
            self._table_np[:] = self._table
        a = np.asarray(sampled, dtype=np.int64).ravel()
        stop = np.nonzero((a == self.eot) | (a < 0))[0]
        toks = a[: stop[0]] if stop.size else a
        n = toks.size
        tb = self.timestamp_begin
        ts = toks >= tb
        consecutive = (np.nonzero(ts[1:] & ts[:-1])[0] + 1).tolist() if n > 1 else []
        if consecutive:
            single_ending = n >= 2 and toks[-2] < tb <= toks[-1]
            bounds = [0] + consecutive + ([n] if single_ending else [])
            if bounds[-1] < n:
                bounds.append(n)
        else:
            bounds = [0, n]
        # text tokens per part from a prefix count: parts without any decode to ""
        is_text = (toks >= 0) & (toks < self.eot)
        csum = np.concatenate([[0], np.cumsum(is_text)])
        texts = []
        for i in range(len(bounds) - 1):
            lo, hi = bounds[i], bounds[i + 1]
            if csum[hi] == csum[lo]:
                texts.append("")
                continue
            part = toks[lo:hi]
            sel = part[is_text[lo:hi]]
            texts.append(b"".join(self._table_np[sel]).decode("utf-8", errors="replace").strip())
        return " ".join(texts).strip()


def layout_vocab(n_vocab: int) -> int:
    """The token layout a model of ``n_vocab`` entries decodes with: the large-v3 layout for
    exactly 51 866, the multilingual one from 51 865 on, else ``*.en`` (test models with a
    cut vocabulary keep the ``*.en`` ids, as WhisperConfig.multilingual says)."""
    if n_vocab == N_VOCAB_V3:
        return N_VOCAB_V3
    return N_VOCAB_MULTILINGUAL if n_vocab >= N_VOCAB_MULTILINGUAL else N_VOCAB_EN


def load_tokenizer(multilingual: bool = False, n_vocab: int = None):
    """The tokenizer of a model: ``n_vocab`` (WhisperConfig.n_vocab) picks the layout."""
    if n_vocab is not None:
        n_vocab = layout_vocab(n_vocab)
    return WhisperTokenizer(os.environ.get("JANUS_WHISPER_DIR"), multilingual=multilingual, n_vocab=n_vocab)

