"""The text quality signals of gz_text_signals (include/genz_tokenize.h, "---- quality") in plain Python over `bytes`.  No hash:
"seen earlier" is a dict keyed by the span's bytes.

The rule.  A document is the bytes t = text[off[d]:off[d+1]].  A character begins at every byte outside 0x80..0xBF.  Words are the
tokenizer's: maximal runs of bytes that belong to no whitespace character (the 29 code points of str.isspace()).  gap_k is the bytes
between word k - 1 and word k, nl_k the number of 0x0A bytes in it.  Word k heads a LINE iff k == 0 or nl_k >= 1, a PARAGRAPH iff
k == 0 or nl_k >= 2.  A span runs from its head word's first byte to the last byte of the last word before the next head (trimmed;
interior whitespace stays).  A span is a duplicate iff its bytes equal those of an earlier span of the same kind in the same document.
A hash decides where to look, never whether two spans are equal, nor whether they stand in the same document.
"""
import numpy as np

NAMES = ("n_chars", "n_words", "word_chars", "n_alpha_words", "n_hash", "n_ellipsis", "n_lines", "n_bullet_lines", "n_ellipsis_lines",
         "dup_lines", "dup_line_chars", "n_paragraphs", "dup_paragraphs", "dup_paragraph_chars")
WS = [chr(c).encode("utf-8") for c in range(0x110000) if chr(c).isspace()]        # the 29 code points, as bytes
BULLETS = (b"-", b"*", "•".encode(), "●".encode())
ELLIPSIS = "…".encode()


def chars(t: bytes) -> int:
    return sum(1 for b in t if not 0x80 <= b <= 0xBF)


def words(t: bytes):
    """[(start, end)] of the words of t: every occurrence of a whitespace character's bytes is whitespace"""
    ws = bytearray(len(t))
    for w in WS:
        at = t.find(w)
        while at >= 0:
            ws[at:at + len(w)] = b"\x01" * len(w)
            at = t.find(w, at + 1)
    out, i = [], 0
    while i < len(t):
        if ws[i]:
            i += 1
            continue
        j = i
        while j < len(t) and not ws[j]:
            j += 1
        out.append((i, j))
        i = j
    return out


def is_letter(t: bytes, i: int) -> bool:
    """the character that begins at t[i] is a letter: A-Z, a-z, or a code point >= U+00C0 outside the excluded ranges.  The code point
    of a lead byte is put together from the bytes it announces, whatever they are; absent ones are 0."""
    b = lambda k: t[i + k] if i + k < len(t) else 0  # noqa: E731
    b0 = t[i]
    if b0 < 0x80:
        return chr(b0).isascii() and chr(b0).isalpha()
    if b0 < 0xC0:
        return False
    if b0 < 0xE0:
        cp = (b0 & 0x1F) << 6 | (b(1) & 0x3F)
    elif b0 < 0xF0:
        cp = (b0 & 0x0F) << 12 | (b(1) & 0x3F) << 6 | (b(2) & 0x3F)
    else:
        cp = (b0 & 0x07) << 18 | (b(1) & 0x3F) << 12 | (b(2) & 0x3F) << 6 | (b(3) & 0x3F)
    return (cp >= 0xC0 and cp not in (0xD7, 0xF7) and not 0x2000 <= cp <= 0x2BFF and not 0x3000 <= cp <= 0x303F
            and not 0xFE00 <= cp <= 0xFE0F and cp < 0x1F000)


def spans(t: bytes, ws, need: int):
    """[(start, end)] of the lines (need = 1) or paragraphs (need = 2) of t with words ws"""
    out = []
    for k, (a, b) in enumerate(ws):
        if k == 0 or t[ws[k - 1][1]:a].count(b"\n") >= need:
            out.append([a, b])
        else:
            out[-1][1] = b
    return out


def firsts(t: bytes, sp):
    seen, out = {}, []
    for k, (a, b) in enumerate(sp):
        out.append(seen.setdefault(t[a:b], k))
    return out


def document(t: bytes):
    """(the 14 signals, line spans, line firsts, paragraph spans, paragraph firsts) of one document"""
    ws = words(t)
    lines, paras = spans(t, ws, 1), spans(t, ws, 2)
    lf, pf = firsts(t, lines), firsts(t, paras)
    s = dict.fromkeys(NAMES, 0)
    s["n_chars"] = chars(t)
    s["n_words"] = len(ws)
    s["word_chars"] = sum(chars(t[a:b]) for a, b in ws)
    s["n_alpha_words"] = sum(any(not 0x80 <= t[i] <= 0xBF and is_letter(t, i) for i in range(a, b)) for a, b in ws)
    s["n_hash"] = t.count(b"#")
    s["n_ellipsis"] = t.count(b"...") + t.count(ELLIPSIS)
    s["n_lines"] = len(lines)
    s["n_bullet_lines"] = sum(t[a:b].startswith(BULLETS) for a, b in lines)
    s["n_ellipsis_lines"] = sum(t[a:b].endswith((b"...", ELLIPSIS)) for a, b in lines)
    s["dup_lines"] = sum(f != k for k, f in enumerate(lf))
    s["dup_line_chars"] = sum(chars(t[a:b]) for k, (a, b) in enumerate(lines) if lf[k] != k)
    s["n_paragraphs"] = len(paras)
    s["dup_paragraphs"] = sum(f != k for k, f in enumerate(pf))
    s["dup_paragraph_chars"] = sum(chars(t[a:b]) for k, (a, b) in enumerate(paras) if pf[k] != k)
    return s, lines, lf, paras, pf


def signals(docs):
    """docs: a list of bytes -> the dict text_signals_packed(..., return_lines=True, return_paragraphs=True) returns"""
    res = [document(t) for t in docs]
    out = {k: np.array([r[0][k] for r in res], dtype=np.int32) for k in NAMES}
    for name, at in (("line", 1), ("para", 3)):
        out[name + "_off"] = np.cumsum([0] + [len(r[at]) for r in res]).astype(np.uint32)
        out[name + "_span"] = np.array([s for r in res for s in r[at]], dtype=np.int64).reshape(-1, 2)
        out[name + "_first"] = np.array([f for r in res for f in r[at + 1]], dtype=np.int32)
    return out
