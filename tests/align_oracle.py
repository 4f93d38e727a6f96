"""The oracle and the inputs of the align tests (test_align_inputs.py on the CPU, test_gpu_align.py on the GPU).

Plain Python, straight from the rules of include/genz_tokenize.h ("align"): spans from re.finditer, piece counts from
O.encode_words, rows, labels and owners by loops.  No hashes, no numpy tricks: numpy only carries the results.
"""
import functools
import random
import re

import numpy as np

import corpus as corpus_mod
import gz_oracle as O
import offset_oracle as X

WORD = re.compile(r"\S+\n?")
TILE = X.TILE
IGNORE = -100


def enc(s):
    return s.encode("utf-8", "surrogatepass")


def pack(docs):
    """str documents -> (uint8 text, int64 offsets [N + 1]); lone surrogates pass, as the library's own packing lets them"""
    raw = [enc(d) for d in docs]
    offs = np.zeros(len(raw) + 1, dtype=np.int64)
    at = 0
    for i, b in enumerate(raw):
        at += len(b)
        offs[i + 1] = at
    return np.frombuffer(b"".join(raw), dtype=np.uint8), offs


def spans(text, unit="char"):
    """[begin, end) of the \\S+ part of every word of one document, in code points or in bytes"""
    out = []
    for m in WORD.finditer(text):
        b, e = m.start(), m.end()
        if text[e - 1] == "\n":
            e -= 1                                                      # the glued line feed is not inside
        if unit == "byte":
            b, e = len(enc(text[:b])), len(enc(text[:e]))
        out.append((b, e))
    return out


def batch_spans(docs, unit="char"):
    """(span int32 [W, 2], word_off int64 [N + 1]) of a batch"""
    flat, off = [], [0]
    for d in docs:
        flat.extend(spans(d, unit))
        off.append(len(flat))
    return np.array(flat, dtype=np.int32).reshape(len(flat), 2), np.array(off, dtype=np.int64)


def piece_counts(text, tables):
    return O.encode_words(text, tables)[1]


def rows(counts, row_doc, row_start, max_len, labels=None, continuation="ignore", cont_map=None, ignore_index=IGNORE):
    """counts / labels: a list per document.  -> (word_ids, labels or None, n_real) as lists of rows"""
    room = max_len - 2
    out_w, out_l, out_n = [], [], []
    for d, s in zip(row_doc, row_start):
        word_of, first = [], []
        for j, c in enumerate(counts[d]):
            for k in range(c):
                word_of.append(j)
                first.append(k == 0)
        T = len(word_of)
        chunk = list(range(s, min(s + room, T))) if s < T else []
        wid, lab = [-1] * max_len, [ignore_index] * max_len
        for i, t in enumerate(chunk):
            j = word_of[t]
            wid[1 + i] = j
            if labels is not None:
                v = labels[d][j]
                if first[t] or continuation == "same":
                    lab[1 + i] = v
                elif continuation == "map":
                    lab[1 + i] = cont_map[v] if 0 <= v < len(cont_map) else v
        out_w.append(wid)
        out_l.append(lab)
        out_n.append(len(chunk) + 2)
    return out_w, (out_l if labels is not None else None), out_n


def span_labels(doc_spans, doc_marks, scheme, outside=0):
    """doc_spans: per document a list of (b, e); doc_marks: per document a list of (begin, end, label).
    -> (word labels per document, mark_words per document)"""
    all_labels, all_mw = [], []
    for words, marks in zip(doc_spans, doc_marks):
        owner = [None] * len(words)
        mw = []
        for m, (b, e, _) in enumerate(marks):
            hit = [j for j, (wb, we) in enumerate(words) if e > b and b < we and wb < e]
            mw.append((hit[0], hit[-1] + 1) if hit else (-1, -1))
            for j in hit:
                if owner[j] is None or m < owner[j]:
                    owner[j] = m
        labels = []
        for j, o in enumerate(owner):
            if o is None:
                labels.append(0 if scheme == "bio" else outside)
            elif scheme == "plain":
                labels.append(marks[o][2])
            else:
                begins = j == 0 or owner[j - 1] != o
                labels.append(2 * marks[o][2] + (1 if begins else 2))
        all_labels.append(labels)
        all_mw.append(mw)
    return all_labels, all_mw


# ---- inputs ------------------------------------------------------------------------------------------------------------------
SMALL_DOCS = ("a\n b", "a\n\nb", "\n", "a\r\n", "xin ch\u00e0o\n", "", " ", "x", "\ud800 a\udfffb \udc00", "\U0001F600\u00a0\u00e9\n\u2028\u1ec7",
              "a\u3000b\u1680c\u0085d", "\x1cq\x1fr", "tab\there", "  hai  d\u1ea5u  c\u00e1ch  ")


@functools.lru_cache(maxsize=None)
def straddle_docs():
    """Documents laid out so that a 2-, 3- and 4-byte character lies across every tile edge they reach, at every split of its bytes.
    -> (docs, claims): claims = (edge of the packed text, bytes of the character before the edge, its width)."""
    docs, claims, at = [], [], 0
    r = random.Random(23)

    def add(d):
        nonlocal at
        docs.append(d)
        at += len(enc(d))
    for ch in ("\u00e9", "\u1ec7", "\U0001F600", "\u00a0", "\u2003", "\ud800"):
        w = len(enc(ch))
        for before in range(1, w):
            edge = (at // TILE + 1) * TILE
            fill = edge - before - at                                    # bytes in front of the character
            if fill < 3:
                edge += TILE
                fill += TILE
            add(X._fill(fill - 2, r) + " x" + ch + "y z")              # the character inside a word (or, a space, between two)
            claims.append((edge, before, w))
            add("")                                                     # and an empty document behind it
    return tuple(docs), tuple(claims)


def span_batches():
    """name -> documents: everything the span tests run on"""
    out = {b.name: list(b.docs) for b in X.edges()}
    out["ladder"] = list(X.ladder().docs)
    out["ws"] = list(X.WS_DOCS)
    out["small"] = list(SMALL_DOCS)
    out["straddle"] = list(straddle_docs()[0])
    out["one_empty"] = [""]
    out["none"] = []
    return out


@functools.lru_cache(maxsize=None)
def noisy_corpus(n=300):
    text, offs, _ = corpus_mod.config_corpus(3, n_docs=n, seed=11)
    text, offs = corpus_mod.add_noise(text, offs, seed=11, rate=0.05)
    raw = text.tobytes()
    return tuple(raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(len(offs) - 1))


ALIGN_WORDS = (1, 2, 16, 17, 2500)
ALIGN_LENS = (3, 4, 16, 48)


def synthetic_counts(seed=3):
    """Piece counts per document, made for the align kernel alone: documents of 1, 2, 16, 17 and 2 500 words, empty documents, and for
    every max_len documents whose T is room - 1, room, room + 1, cut exactly at a word boundary and one piece into a word."""
    r = random.Random(seed)
    docs = [[]]
    for w in ALIGN_WORDS:
        docs.append([r.choice((1, 1, 1, 2, 3, 7)) for _ in range(w)])
    for L in ALIGN_LENS:
        room = L - 2
        for T in (room - 1, room, room + 1):
            if T >= 1:
                docs.append([1] * T)                                    # one piece a word
                docs.append([T])                                        # one word of T pieces
        docs.append([1] * room + [3, 1])                                # the cut falls exactly between two words
        docs.append(([1] * (room - 1) if room > 1 else []) + [4, 2])    # ... and one piece into a word (room 1: into its first)
        docs.append([])
    return docs


def random_marks(doc_spans, text_len, r, n_labels=5):
    """Marks around the words of one document: touching on either side, empty, reversed, on whitespace only, past the end, nested,
    overlapping, unsorted."""
    marks = []
    for (b, e) in doc_spans:
        k = r.random()
        if k < 0.25:
            marks.append((b, e, r.randrange(n_labels)))
        elif k < 0.35:
            marks.append((e, e + 1, r.randrange(n_labels)))              # touches the word's end: on the whitespace behind it, if any
        elif k < 0.45:
            marks.append((max(b - 1, 0), b, r.randrange(n_labels)))      # touches its begin
        elif k < 0.5:
            marks.append((e, b, r.randrange(n_labels)))                  # reversed
        elif k < 0.55:
            marks.append((b, b, r.randrange(n_labels)))                  # empty
        elif k < 0.7:
            marks.append((b + (e - b) // 2, e + r.randrange(0, 12), r.randrange(n_labels)))     # from inside a word over its neighbours
    marks.append((text_len, text_len + 5, 1))
    marks.append((text_len + 3, text_len + 9, 2))
    if doc_spans:
        marks.append((doc_spans[0][0], doc_spans[-1][1], 3))             # everything, nested around the rest
    r.shuffle(marks)
    return marks
