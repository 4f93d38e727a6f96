"""Text quality signals on the GPU: the half of the Gopher quality rule (Rae et al., 2021, table A1) that works on text --
word counts and lengths, symbol ratios, bullet and ellipsis lines, the alphabetic-word share, duplicate lines and paragraphs --
where `Tokenize.repetition_filter` serves the half that works on tokens (csrc/gz_quality.inc; the rule is stated in
include/genz_tokenize.h, "---- quality").  There is no CPU fallback.
"""
from typing import Optional, Sequence

import numpy as np

from . import _native
from ._packing import pack as _pack

SIGNALS = _native.GZ_Q_NAMES
# Gopher's bounds (table A1), stated for English web pages: tune them for other languages and sources
GOPHER_BOUNDS = dict(min_words=50, max_words=100_000, min_mean_word_length=3.0, max_mean_word_length=10.0, max_hash_ratio=0.1,
                     max_ellipsis_ratio=0.1, max_bullet_lines=0.9, max_ellipsis_lines=0.3, min_alpha_words=0.8, max_dup_lines=0.30,
                     max_dup_paragraphs=0.30, max_dup_line_chars=0.20, max_dup_paragraph_chars=0.20)
_ctx: Optional[_native.Context] = None


def _context() -> _native.Context:
    global _ctx
    if _ctx is None:
        _ctx = _native.Context()
    return _ctx


def _packed(text_u8, offsets):
    """the refusals of a packed input, before any native call"""
    text = np.asarray(text_u8)
    off = np.asarray(offsets)
    if text.dtype != np.uint8 or text.ndim != 1:
        raise TypeError("text_u8 must be a one-dimensional uint8 array")
    if off.ndim != 1 or len(off) < 1 or off.dtype.kind not in "iu":
        raise TypeError("offsets must be a one-dimensional integer array of n + 1 entries")
    off = off.astype(np.int64, copy=False)
    if off[0] < 0 or off[-1] > len(text) or (np.diff(off) < 0).any():
        raise ValueError("offsets must not decrease and must lie inside the text")
    return np.ascontiguousarray(text), np.ascontiguousarray(off)


def _named(signals, lines, paragraphs):
    out = {k: signals[i] for i, k in enumerate(SIGNALS)}
    for name, arrays in (("line", lines), ("para", paragraphs)):
        if arrays is not None:
            out[name + "_off"], out[name + "_span"], out[name + "_first"] = arrays
    return out


def text_signals_packed(text_u8, offsets, return_lines=False, return_paragraphs=False, ctx: Optional[_native.Context] = None):
    """The fourteen signals of every document of packed UTF-8 (`text_u8` uint8, `offsets` int64 [N+1], absolute), on the GPU.
    Words are the tokenizer's (runs of bytes of no `str.isspace()` character); word k heads a LINE iff k == 0 or a '\\n' stands in
    the gap before it, a PARAGRAPH iff k == 0 or two do; a span runs to the last byte of the last word before the next head
    (trimmed; interior whitespace stays).  A line (paragraph) is a duplicate iff its bytes equal an EARLIER one's of the same
    document -- exact: a hash decides where to look, never whether two spans are equal, nor whether they stand in the same
    document; `text_signals(docs[a:b])` is `text_signals(docs)` cut to [a:b].
    Returns a dict of int32 [N] arrays: n_chars, n_words, word_chars (characters inside words), n_alpha_words (words with a
    letter: A-Z, a-z or a code point >= U+00C0 outside U+00D7, U+00F7, U+2000..U+2BFF, U+3000..U+303F, U+FE00..U+FE0F and
    >= U+1F000 -- a range rule, NOT Unicode's Alphabetic property), n_hash ('#'), n_ellipsis (`count("...")` + U+2026), n_lines,
    n_bullet_lines (first character '-', '*', U+2022, U+25CF), n_ellipsis_lines (ending in "..." or U+2026), dup_lines,
    dup_line_chars, n_paragraphs, dup_paragraphs, dup_paragraph_chars.  `return_lines` adds line_off uint32 [N+1], line_span
    int64 [L, 2] (bytes, relative to the document) and line_first int32 [L] (the document-local index of the earliest equal line,
    the line's own where there is none): what a caller needs to drop the duplicates; `return_paragraphs` the same as para_*."""
    text, off = _packed(text_u8, offsets)
    return _named(*(ctx or _context()).text_signals(text, off, bool(return_lines), bool(return_paragraphs)))


def text_signals(texts: Sequence[str], return_lines=False, return_paragraphs=False, ctx: Optional[_native.Context] = None):
    """`text_signals_packed` over a list of `str`."""
    texts = list(texts)
    for t in texts:
        if not isinstance(t, str):
            raise TypeError("expected string or bytes-like object")
    buf, off = _pack(texts)
    return text_signals_packed(buf, off, return_lines, return_paragraphs, ctx)


def text_signals_to_device(texts: Sequence[str], ctx: Optional[_native.Context] = None):
    """`text_signals` whose int32 [14, N] signals (rows in the order of `SIGNALS`) STAY in HBM as a `handoff.DeviceArray`
    (`torch.from_dlpack(x)` is zero-copy)."""
    from .handoff import DeviceArray
    texts = list(texts)
    for t in texts:
        if not isinstance(t, str):
            raise TypeError("expected string or bytes-like object")
    buf, off = _pack(texts)
    c = ctx or _context()
    n = len(texts)
    d_sig = c.alloc(4 * len(SIGNALS) * max(n, 1))
    try:
        sig = DeviceArray(c, d_sig, (len(SIGNALS), n))
    except BaseException:
        c.free(d_sig)
        raise
    d_text, d_off = c.alloc(max(len(buf), 1)), c.alloc(8 * (n + 1))
    try:
        if len(buf):
            c.h2d(d_text, buf)
        c.h2d(d_off, off)
        c.text_signals_device(d_text, d_off, n, d_sig)
        c.sync()
    finally:
        c.free(d_text)
        c.free(d_off)
    return sig


def gopher_shares(signals, **bounds):
    """The shares and the decision of `gopher_filter` from the counts of `text_signals` (host arithmetic).  A share whose
    denominator is 0 is 0."""
    unknown = set(bounds) - set(GOPHER_BOUNDS)
    if unknown:
        raise TypeError("unknown bound: %s" % ", ".join(sorted(unknown)))
    b = dict(GOPHER_BOUNDS, **bounds)
    s = {k: np.asarray(signals[k], dtype=np.float64) for k in SIGNALS}

    def share(num, den):
        return np.divide(s[num], s[den], out=np.zeros_like(s[num]), where=s[den] > 0)

    out = dict(signals)
    out["mean_word_length"] = share("word_chars", "n_words")
    out["hash_ratio"] = share("n_hash", "n_words")
    out["ellipsis_ratio"] = share("n_ellipsis", "n_words")
    out["bullet_lines"] = share("n_bullet_lines", "n_lines")
    out["ellipsis_lines"] = share("n_ellipsis_lines", "n_lines")
    out["alpha_words"] = share("n_alpha_words", "n_words")
    out["dup_line_fraction"] = share("dup_lines", "n_lines")
    out["dup_paragraph_fraction"] = share("dup_paragraphs", "n_paragraphs")
    out["dup_line_char_fraction"] = share("dup_line_chars", "n_chars")
    out["dup_paragraph_char_fraction"] = share("dup_paragraph_chars", "n_chars")
    keep = (s["n_words"] >= b["min_words"]) & (s["n_words"] <= b["max_words"])
    keep &= (out["mean_word_length"] >= b["min_mean_word_length"]) & (out["mean_word_length"] <= b["max_mean_word_length"])
    keep &= (out["hash_ratio"] <= b["max_hash_ratio"]) & (out["ellipsis_ratio"] <= b["max_ellipsis_ratio"])
    keep &= (out["bullet_lines"] <= b["max_bullet_lines"]) & (out["ellipsis_lines"] <= b["max_ellipsis_lines"])
    keep &= out["alpha_words"] >= b["min_alpha_words"]
    keep &= (out["dup_line_fraction"] <= b["max_dup_lines"]) & (out["dup_paragraph_fraction"] <= b["max_dup_paragraphs"])
    keep &= (out["dup_line_char_fraction"] <= b["max_dup_line_chars"]) & (out["dup_paragraph_char_fraction"] <= b["max_dup_paragraph_chars"])
    out["keep"] = keep
    return out


def gopher_filter(texts: Sequence[str], tok=None, ctx: Optional[_native.Context] = None, **bounds):
    """`text_signals` plus the decision of the Gopher quality rule: the counts, the shares (float64 [N]: mean_word_length,
    hash_ratio and ellipsis_ratio per word, bullet_lines and ellipsis_lines per line, alpha_words per word,
    dup_line_fraction, dup_paragraph_fraction, and the two character shares over n_chars; 0 where the denominator is 0) and
    keep bool [N].  The defaults (`GOPHER_BOUNDS`) are the paper's: 50..100 000 words, mean word length 3..10, '#' and
    ellipsis per word <= 0.1, bullet lines <= 0.9, ellipsis lines <= 0.3, words with a letter >= 0.8, duplicate lines and
    paragraphs <= 0.30 by count and <= 0.20 by characters.  They were stated for ENGLISH WEB PAGES and are to be tuned: pass any
    of them by name.  With `tok` (a `Tokenize`) keep is ANDed with `tok.repetition_filter(texts)["keep"]`, the token half of
    the rule."""
    unknown = set(bounds) - set(GOPHER_BOUNDS)
    if unknown:
        raise TypeError("unknown bound: %s" % ", ".join(sorted(unknown)))
    texts = list(texts)
    out = gopher_shares(text_signals(texts, ctx=ctx), **bounds)
    if tok is not None:
        out["keep"] = out["keep"] & tok.repetition_filter(texts)["keep"]
    return out
