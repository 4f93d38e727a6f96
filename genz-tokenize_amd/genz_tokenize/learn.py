"""Learn BPE merges and a vocabulary from a corpus, on the GPU: the two files `Tokenize.fromFile(vocab, codes)` takes.

    words, counts = word_counts(documents)                       # distinct str.split() words, first-occurrence order; int64 counts
    t = learn_bpe(documents, n_merges=32000, min_frequency=2)
    t = learn_bpe(words=words, counts=counts, n_merges=32000)    # shard counts added on the host, learnt once
    t.codes, t.vocab, t.merges, t.n_words, t.n_symbols
    t.save(vocab_path, codes_path); tok = t.tokenizer()

The reference has no learner; the rule is stated at "learn" in include/genz_tokenize.h and in DESIGN.md section 8.  It is pinned by
closure: `t.tokenizer().bpe(word)` is the learner's own final segmentation of every training word.  The result is a pure function
of the multiset of words: document order and boundaries do not matter, and shards concatenate through `word_counts`.  There is no
CPU fallback."""
from __future__ import annotations

import os
import tempfile
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from ._packing import pack as _pack
from .tokenize import Tokenize, _integer, _require_str

MERGES_MAX = 1 << 20                    # GZ_BPE_MERGES_MAX
COUNT_LIMIT = 1 << 62

__all__ = ["learn_bpe", "learn_bpe_packed", "word_counts", "word_counts_packed", "LearnedBPE"]


def _context(ctx):
    if ctx is not None:
        return ctx
    from .ranking import _context as shared
    return shared()


def _documents(documents) -> list:
    if isinstance(documents, (str, bytes, bytearray, memoryview)):
        raise TypeError("documents must be a sequence of str, not one %s" % type(documents).__name__)
    documents = list(documents)
    for d in documents:
        _require_str(d)
    return documents


def _packed(text_u8, offsets) -> Tuple[np.ndarray, np.ndarray]:
    text_u8, offsets = np.asarray(text_u8), np.asarray(offsets)
    if text_u8.dtype != np.uint8 or text_u8.ndim != 1:
        raise TypeError("text must be a 1-D uint8 array")
    if offsets.dtype != np.int64 or offsets.ndim != 1 or len(offsets) < 1:
        raise TypeError("offsets must be a 1-D int64 array of n + 1 entries")
    if len(offsets) > 1 and (np.diff(offsets) < 0).any() or offsets[0] < 0 or offsets[-1] > len(text_u8):
        raise ValueError("offsets must not decrease and must lie inside the text")
    return text_u8, offsets


def _rule(n_merges, min_frequency) -> Tuple[int, int]:
    return _integer("n_merges", n_merges, 0, MERGES_MAX + 1), _integer("min_frequency", min_frequency, 1, COUNT_LIMIT)


def _word_list(words, counts) -> Tuple[list, np.ndarray]:
    if isinstance(words, (str, bytes, bytearray, memoryview)):
        raise TypeError("words must be a sequence of str, not one %s" % type(words).__name__)
    words = list(words)
    if counts is None:
        raise TypeError("words need counts")
    counts = list(counts) if not isinstance(counts, np.ndarray) else counts.tolist()
    if len(counts) != len(words):
        raise ValueError("%d words but %d counts" % (len(words), len(counts)))
    total = 0
    for w in words:
        _require_str(w)
        if w.split() != [w]:
            raise ValueError("%r is not one word: words are not empty and hold no whitespace" % (w,))
    for c in counts:
        total += _integer("a count", c, 1, COUNT_LIMIT)
    if total >= COUNT_LIMIT:
        raise ValueError("the counts must sum to less than 2**62")
    return words, np.asarray(counts, dtype=np.int64).reshape(-1)


class _WordSet:
    """a gz_wordset of a context; freed when the object goes (the context is held until then)"""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def close(self):
        if self.handle:
            self.ctx.wordset_destroy(self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def word_counts_packed(text_u8, offsets, ctx: Optional[_native.Context] = None):
    """The distinct `str.split()` words of packed documents (uint8 text, int64 offsets [n + 1], the form `encode_packed` takes) in
    first-occurrence order: (bytes uint8, offsets int64 [words + 1], counts int64 [words])."""
    text_u8, offsets = _packed(text_u8, offsets)
    ctx = _context(ctx)
    ws = _WordSet(ctx, ctx.wordset_build(text_u8, offsets))
    try:
        return ctx.wordset_words(ws.handle)
    finally:
        ws.close()


def word_counts(documents: Sequence[str], ctx: Optional[_native.Context] = None) -> Tuple[List[str], np.ndarray]:
    """(words, counts): the distinct `str.split()` words of the documents in first-occurrence order and how often each occurs
    (int64) -- `collections.Counter` over `d.split()` for every d, made on the GPU.  Counts of shards are added on the host and
    learnt once: `learn_bpe(words=..., counts=...)`."""
    documents = _documents(documents)
    data, off, cnt = word_counts_packed(*_pack(documents), ctx=ctx)
    raw = data.tobytes()
    return [raw[off[i]:off[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(cnt))], cnt


class LearnedBPE:
    """What `learn_bpe` returns: `codes` and `vocab` (the bytes of the two files), `merges` [(left, right), ...] in learning order,
    `n_words` distinct training words, `n_symbols` symbols (initial and merged), `info` (pair-table slots, keys and growths)."""

    def __init__(self, codes: bytes, vocab: bytes, merges, n_words: int, n_symbols: int, info: dict):
        self.codes, self.vocab, self.merges, self.n_words, self.n_symbols, self.info = codes, vocab, merges, n_words, n_symbols, info

    def save(self, vocab_path, codes_path) -> None:
        """Write the two files where `Tokenize.fromFile(vocab_path, codes_path)` reads them."""
        with open(vocab_path, "wb") as f:
            f.write(self.vocab)
        with open(codes_path, "wb") as f:
            f.write(self.codes)

    def tokenizer(self) -> Tokenize:
        """`Tokenize.fromFile` on the saved files (written to a temporary directory that is removed again: the tokenizer reads
        both files when it is made)."""
        with tempfile.TemporaryDirectory(prefix="genz_learn_") as d:
            v, c = os.path.join(d, "vocab.txt"), os.path.join(d, "bpe.codes")
            self.save(v, c)
            return Tokenize.fromFile(v, c)


def _learn(ctx, ws: _WordSet, n_merges: int, min_frequency: int) -> LearnedBPE:
    try:
        n_words = ctx.wordset_info(ws.handle)[0]
        info, mbytes, moff, pbytes, poff, pcnt = ctx.bpe_learn(ws.handle, n_merges, min_frequency)
    finally:
        ws.close()
    mraw, praw = mbytes.tobytes(), pbytes.tobytes()
    strs = [mraw[moff[i]:moff[i + 1]] for i in range(len(moff) - 1)]
    codes = b"#version: 0.2\n" + b"".join(strs[2 * i] + b" " + strs[2 * i + 1] + b"\n" for i in range(len(strs) // 2))
    vocab = b"".join(praw[poff[i]:poff[i + 1]] + b" %d\n" % int(pcnt[i]) for i in range(len(pcnt)))
    merges = [(strs[2 * i].decode("utf-8", "surrogatepass"), strs[2 * i + 1].decode("utf-8", "surrogatepass")) for i in range(len(strs) // 2)]
    return LearnedBPE(codes, vocab, merges, int(n_words), int(info[1]),
                      dict(table_slots=int(info[5]), table_keys=int(info[6]), table_growths=int(info[7])))


def learn_bpe_packed(text_u8, offsets, n_merges: int = 32000, min_frequency: int = 2, ctx: Optional[_native.Context] = None) -> LearnedBPE:
    """`learn_bpe` over packed documents (uint8 text, int64 offsets [n + 1])."""
    n_merges, min_frequency = _rule(n_merges, min_frequency)
    text_u8, offsets = _packed(text_u8, offsets)
    ctx = _context(ctx)
    return _learn(ctx, _WordSet(ctx, ctx.wordset_build(text_u8, offsets)), n_merges, min_frequency)


def learn_bpe(documents: Optional[Sequence[str]] = None, n_merges: int = 32000, min_frequency: int = 2, *, words: Optional[Sequence[str]] = None,
              counts=None, ctx: Optional[_native.Context] = None) -> LearnedBPE:
    """Learn at most `n_merges` BPE merges from `documents` (a sequence of str), or from `words` and `counts` (what `word_counts`
    gives; equal words add up).  A step merges the adjacent pair of symbols with the largest count -- ties: the pair made of the
    older symbols -- in every word; learning stops when the best count is below `min_frequency` (>= 1) or no pair is left.
    TypeError / ValueError for a bad argument before anything runs; `_native.GzError` from the library (the limits: fewer than
    2**32 bytes + documents a call, 2**31 - 1 symbol positions, counts times symbols below 2**62)."""
    n_merges, min_frequency = _rule(n_merges, min_frequency)
    if (documents is None) == (words is None):
        raise TypeError("give either documents, or words and counts")
    if documents is not None:
        if counts is not None:
            raise TypeError("counts belong to words, not to documents")
        return learn_bpe_packed(*_pack(_documents(documents)), n_merges=n_merges, min_frequency=min_frequency, ctx=ctx)
    words, counts = _word_list(words, counts)
    ctx = _context(ctx)
    buf, off = _pack(words)
    return _learn(ctx, _WordSet(ctx, ctx.wordset_from_counts(buf, off, counts)), n_merges, min_frequency)
