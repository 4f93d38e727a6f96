"""The BPE-dropout rule of include/genz_tokenize.h ("BPE-dropout") in plain Python, for the tests.  Imports nothing of the product:
words, ranks and the piece-to-id lookup are the oracle's (oracle/gz_oracle.py), the Philox rounds are tests/mask_oracle.py's.

Only the merge loop of one word differs from the plain call.  Its draws are a pure function of (seed, D, j, t, i): the global
document index D = doc_base + d, the index j of the word within its document, the merge iteration t, the position i in the word's
current symbol list.

  word_key(seed, D, j)   words 0, 1 of Philox4x32-10(counter (D lo, D hi, j, 0), key (seed lo, seed hi))
  u(key, t, i)           word i & 3 of Philox4x32-10(counter (t, i >> 2, 0, 0), key): one call serves four neighbouring positions
  iteration t            position i is live when u(key, t, i) >= thr and (syms[i], syms[i + 1]) is in the ranks; no live position: the
                         word is finished; else the smallest live rank is merged at every live position that holds it, left to right,
                         never overlapping (a dropped occurrence stays unmerged in that iteration)
  thr = int(p * 2**32)   0 <= thr <= 2**32; p = 1.0 drops everything
"""
import numpy as np

import gz_oracle as O
from mask_oracle import philox4x32_10

ONE = 1 << 32
M32 = 0xFFFFFFFF


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on plain ints (the same rounds as mask_oracle.philox4x32_10, without numpy's per-call cost)"""
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def threshold(p):
    return int(p * ONE)


def word_key(seed, D, j):
    x = _philox(D & M32, D >> 32, j, 0, seed & M32, seed >> 32)
    return x[0], x[1]


def u(key, t, i):
    return _philox(t, i >> 2, 0, 0, key[0], key[1])[i & 3]


def draws(key, t, n):
    """[u(key, t, i) for i in range(n)]; long words through numpy"""
    if n <= 256:
        out = []
        for g in range((n + 3) >> 2):
            out.extend(_philox(t, g, 0, 0, key[0], key[1]))
        return out[:n]
    g = np.arange((n + 3) >> 2, dtype=np.uint64)
    z = np.zeros_like(g)
    x = philox4x32_10((np.full_like(g, t), g, z, z), key)
    return [int(v) for v in np.stack(x, axis=1).reshape(-1)[:n]]


def pieces_dropout(word, ranks, thr, key):
    syms = list(word)
    syms[-1] += "</w>"
    if len(syms) == 1:
        return [word]                                            # tokenize.py:66-67
    t = 0
    while len(syms) > 1:
        n = len(syms)
        d = draws(key, t, n - 1)
        live = [i for i in range(n - 1) if d[i] >= thr and (syms[i], syms[i + 1]) in ranks]
        if not live:
            break                                                # nothing survived: the word is finished
        best = min(ranks[(syms[i], syms[i + 1])] for i in live)
        at = {i for i in live if ranks[(syms[i], syms[i + 1])] == best}
        out, k = [], 0
        while k < n:                                             # left to right, never overlapping
            if k in at:
                out.append(syms[k] + syms[k + 1]); k += 2
            else:
                out.append(syms[k]); k += 1
        syms, t = out, t + 1
    return ("@@ ".join(syms)[:-4]).split(" ")


def bpe_string(word, t, thr, seed=0, doc=0, j=0):
    """Tokenize.bpe_dropout(word, p, seed, doc, j)"""
    return " ".join(pieces_dropout(word, t.ranks, thr, word_key(seed, doc, j)))


def encode_pieces(text, t, thr, seed, D):
    """the pieces of every word of document D, word by word"""
    return [pieces_dropout(w, t.ranks, thr, word_key(seed, D, j)) for j, w in enumerate(O.split_words(text))]


def encode(text, t, thr, seed, D):
    """framed ids of document D (bos, pieces, eos)"""
    unk = t.unk_id
    ids = [t.encoder.get(p, unk) for ps in encode_pieces(text, t, thr, seed, D) for p in ps]
    return [t.bos_id] + ids + [t.eos_id]


def rows(t, texts, thr, seed=0, doc_base=0):
    return [encode(x, t, thr, seed, doc_base + d) for d, x in enumerate(texts)]


def shaped(t, framed, max_len=None, padding=True, truncation=True):
    """the rows of `Tokenize.__call__`'s shaping rule (tokenize.py:141-146, :247-249) over framed rows"""
    if max_len is not None and padding:
        return [O.pad_or_cut(list(r), max_len, truncation, t.pad_id, t.eos_id) for r in framed]
    return [list(r) for r in framed]
