"""Vietnamese word segmentation by lexicon, on the GPU: raw text (syllables between spaces) -> the word-segmented text the tokenizer
takes ("sinh viên công nghệ" -> "sinh_viên công_nghệ").

    lex = Lexicon.from_tokenizer()                               # the underscore words of the bundled vocab.txt, equal costs: fewest words
    lex = Lexicon.from_corpus(segmented_documents)               # words and counts of a segmented corpus: the most probable segmentation
    lex = Lexicon.from_words(words, counts=counts)
    segment_batch(["Sinh viên đại học (Hà Nội)."], lex)          # ['Sinh_viên đại_học ( Hà_Nội ) .']
    tok.encode_batch(segment_batch(texts, lex), max_len=128)

The reference forwards this step to an external VnCoreNLP server (preprocess.py:83-89); its learnt rules cannot be reproduced, so the
rule is this library's own -- minimum-cost segmentation against a lexicon, stated at "segment" in include/genz_tokenize.h and in
DESIGN.md section 8: tokens are `str.split()` pieces with leading and trailing ASCII punctuation split off; a word is 1..max_syllables
tokens whose '_'-joined, case-folded bytes are a lexicon entry (or any single token, at `unk_cost`); the segmentation with the smallest
total cost wins, the longest last word among equals.  There is no CPU fallback."""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from ._packing import pack as _pack

__all__ = ["Lexicon", "segment_batch", "segment_packed", "segment_to_device", "fold_case", "cost_of_count"]

COST_LIMIT = _native.GZ_SEG_COST_LIMIT
_FOLD_PLUS_ONE = (0x0102, 0x0110, 0x0128, 0x0168, 0x01A0, 0x01AF)
FOLD_MAP = {c: c + 32 for c in range(0x41, 0x5B)}
FOLD_MAP.update({c: c + 32 for c in range(0xC0, 0xDF) if c != 0xD7})
FOLD_MAP.update({c: c + 1 for c in _FOLD_PLUS_ONE})
FOLD_MAP.update({c: c + 1 for c in range(0x1EA0, 0x1EF9, 2)})


def fold_case(s: str) -> str:
    """Lower-case by the Vietnamese alphabet's map only (FOLD_MAP): what the lexicon and the candidates are compared under."""
    return s.translate(FOLD_MAP)


_fold = fold_case


def cost_of_count(count: int, total: int, n_words: int) -> int:
    """clip(rint(2^16 * (log2(total + V) - log2(count + 1))), 1, 2^24 - 1) in float64: the cost of a word seen `count` times among
    `total` words of a lexicon of V entries (add-one smoothing); count 0 is the cost of an unknown word."""
    v = np.rint(65536.0 * (math.log2(float(total + n_words)) - math.log2(float(count + 1))))
    return int(min(max(v, 1.0), float(COST_LIMIT - 1)))


def _context(ctx):
    if ctx is not None:
        return ctx
    from .ranking import _context as shared
    return shared()


class Lexicon:
    """A gz_lexicon of a context: `words` (folded and merged), `costs`, `max_syllables`, `fold_case`, `unk_cost` (the cost of count 0
    where the costs come from counts, else the largest cost: 1 at equal costs).  Freed when the object goes."""

    def __init__(self, words: List[str], costs: List[int], max_syllables: int, fold: bool, unk_cost: int, ctx=None):
        self.words, self.costs, self.max_syllables, self.fold_case, self.unk_cost = words, costs, int(max_syllables), bool(fold), int(unk_cost)
        self.ctx = _context(ctx)
        buf, off = _pack(words)
        self.handle = self.ctx.lexicon_create(buf, off, np.asarray(costs, dtype=np.int32), self.max_syllables, _native.GZ_LEX_FOLD_CASE if fold else 0)

    def close(self):
        if getattr(self, "handle", 0):
            self.ctx.lexicon_destroy(self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __len__(self):
        return len(self.words)

    def info(self) -> dict:
        return self.ctx.lexicon_info(self.handle)

    @classmethod
    def from_words(cls, words: Sequence[str], counts=None, costs=None, max_syllables: int = 8, fold_case: bool = True, ctx=None) -> "Lexicon":
        """Entries from `words` with `counts` (cost = `cost_of_count`), with `costs` (integers in [1, 2^24)), or with neither (every
        cost 1: the fewest words).  Entries that are equal after folding are merged: their counts add, the smallest cost stays.  An
        entry that is empty, holds whitespace or has more than `max_syllables` syllables is refused (ValueError here for the first
        two, `_native.GzError` naming the entry from the library)."""
        if isinstance(words, (str, bytes, bytearray, memoryview)):
            raise TypeError("words must be a sequence of str, not one %s" % type(words).__name__)
        words = list(words)
        if counts is not None and costs is not None:
            raise TypeError("give counts or costs, not both")
        given = counts if counts is not None else costs
        values = [1] * len(words) if given is None else [int(v) for v in (given.tolist() if isinstance(given, np.ndarray) else given)]
        if len(values) != len(words):
            raise ValueError("%d words but %d %s" % (len(words), len(values), "counts" if counts is not None else "costs"))
        merged = {}
        for w, v in zip(words, values):
            if not isinstance(w, str):
                raise TypeError("expected string or bytes-like object")
            if w.split() != [w]:
                raise ValueError("%r is not one word: entries are not empty and hold no whitespace" % (w,))
            if counts is not None and v < 0:
                raise ValueError("count %d of %r is negative" % (v, w))
            if costs is not None and not 1 <= v < COST_LIMIT:
                raise ValueError("cost %d of %r is outside [1, 2**24)" % (v, w))
            key = _fold(w) if fold_case else w
            if key not in merged:
                merged[key] = v
            else:
                merged[key] = merged[key] + v if counts is not None else min(merged[key], v)
        keys = list(merged)
        if counts is not None:
            total = sum(merged.values())
            cost = [cost_of_count(merged[k], total, len(keys)) for k in keys]
            unk = cost_of_count(0, total, len(keys))
        else:
            cost = [merged[k] for k in keys]
            unk = max(cost, default=1)                                   # (an unknown word costs what the rarest entry costs; 1 at equal costs)
        return cls(keys, cost, max_syllables, fold_case, unk, ctx)

    @classmethod
    def from_tokenizer(cls, tok=None, max_syllables: int = 8, ctx=None) -> "Lexicon":
        """The entries of the tokenizer's vocabulary file that hold '_' and are no BPE pieces ('@@'), plus its single-syllable whole
        words, at equal costs.  `tok` None: the bundled vocab.txt.  Entries of more than `max_syllables` syllables are left out."""
        path = getattr(tok, "vocab_file", None) or os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "vocab.txt")
        words = []
        with open(path, encoding="utf-8") as f:
            for line in f:
                parts = line.split()
                if not parts or "@@" in parts[0]:
                    continue
                w = parts[0]
                if all(w.split("_")) and w.count("_") < max_syllables:            # (no empty syllable: "_", "a__b", "_a" are no words)
                    words.append(w)
        return cls.from_words(words, max_syllables=max_syllables, ctx=ctx)

    @classmethod
    def from_corpus(cls, segmented_documents: Sequence[str], max_syllables: int = 8, fold_case: bool = True, ctx=None) -> "Lexicon":
        """The distinct words of a word-segmented corpus and their counts (`word_counts`, on the GPU) as a lexicon; words of more than
        `max_syllables` syllables are left out."""
        from .learn import word_counts
        words, counts = word_counts(segmented_documents, ctx=ctx)
        keep = [i for i, w in enumerate(words) if w.count("_") < max_syllables]
        return cls.from_words([words[i] for i in keep], counts=[int(counts[i]) for i in keep], max_syllables=max_syllables, fold_case=fold_case, ctx=ctx)


def _flags(split_punct) -> int:
    return _native.GZ_SEG_SPLIT_PUNCT if split_punct else 0


def _lexicon(lex) -> Lexicon:
    if not isinstance(lex, Lexicon):
        raise TypeError("expected a genz_tokenize.segment.Lexicon, not %s" % type(lex).__name__)
    if not lex.handle:
        raise ValueError("the lexicon is closed")
    return lex


def segment_packed(text_u8, offsets, lex: Lexicon, split_punct: bool = True, unk_cost: Optional[int] = None, return_tokens: bool = False):
    """Packed UTF-8 (uint8) + int64 offsets [N+1] in; a dict out: `text` uint8 and `offsets` int64 [N+1] (ready for
    `Tokenize.encode_packed`), `stats` int64 [N, 4] (n_tokens, n_words, n_known, cost) and, with `return_tokens`, `join` uint8
    [tokens] (1: the token is glued to the next one) and `tok_off` int64 [tokens] (the token's first byte in `text_u8`)."""
    lex = _lexicon(lex)
    unk = lex.unk_cost if unk_cost is None else int(unk_cost)
    if not 1 <= unk < COST_LIMIT:
        raise ValueError("unk_cost must lie in [1, 2**24)")
    text, off, stats, join, tok_off = lex.ctx.segment(lex.handle, text_u8, offsets, _flags(split_punct), unk, bool(return_tokens))
    out = dict(text=text, offsets=off, stats=stats)
    if return_tokens:
        out["join"], out["tok_off"] = join, tok_off
    return out


def segment_batch(texts: Sequence[str], lex: Lexicon, split_punct: bool = True, unk_cost: Optional[int] = None, return_stats: bool = False):
    """Every text segmented into lexicon words: a list of `str` in which the syllables of a word are joined by '_' and words are
    separated by one space.  `unk_cost` None: the lexicon's.  `return_stats`: (texts, stats int64 [N, 4])."""
    if isinstance(texts, (str, bytes, bytearray, memoryview)):
        raise TypeError("texts must be a sequence of str, not one %s" % type(texts).__name__)
    texts = list(texts)
    for t in texts:
        if not isinstance(t, str):
            raise TypeError("expected string or bytes-like object")
    r = segment_packed(*_pack(texts), lex, split_punct, unk_cost)
    raw, oo = r["text"].tobytes(), r["offsets"]
    out = [raw[oo[i]:oo[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(texts))]
    return (out, r["stats"]) if return_stats else out


def segment_to_device(texts: Sequence[str], lex: Lexicon, split_punct: bool = True, unk_cost: Optional[int] = None):
    """`segment_batch` whose text and offsets STAY in HBM: a dict of `handoff.DeviceArray`s `text` (uint8 [bytes]) and `offsets`
    (int64 [N+1], from 0) -- what `gz_encode_batch_device` (`Context.encode_device`) takes as its text -- and `stats` (int64 [N, 4]);
    `n_bytes` is the text's size."""
    from .handoff import DeviceArray
    lex = _lexicon(lex)
    texts = list(texts)
    for t in texts:
        if not isinstance(t, str):
            raise TypeError("expected string or bytes-like object")
    unk = lex.unk_cost if unk_cost is None else int(unk_cost)
    buf, off = _pack(texts)
    c, n = lex.ctx, len(texts)
    cap = max((2 if split_punct else 1) * len(buf), 1)
    made, out = [], {}
    try:
        for name, nbytes, shape, dtype in (("text", cap + 64, (cap,), np.uint8), ("offsets", 8 * (n + 1), (n + 1,), np.int64),
                                           ("stats", 32 * max(n, 1), (n, 4), np.int64)):
            d = c.alloc(nbytes)
            made.append(d)
            out[name] = DeviceArray(c, d, shape, dtype)
            made.pop()
        d_text, d_off = c.alloc(max(len(buf), 1)), c.alloc(8 * (n + 1))
        made += [d_text, d_off]
        if len(buf):
            c.h2d(d_text, buf)
        c.h2d(d_off, off)
        out["n_bytes"] = c.segment_device(lex.handle, d_text, d_off, n, _flags(split_punct), unk, out["text"].ptr, cap, out["offsets"].ptr,
                                          out["stats"].ptr)
        return out
    finally:
        for d in made:
            c.free(d)
