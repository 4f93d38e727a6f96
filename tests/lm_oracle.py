"""The rule of the token n-gram language model and its perplexity (include/genz_tokenize.h, "token n-gram language model and
perplexity"), in plain Python: Counters of tuples, no hash, math.log2 in float64, round to the 2^24 grid.

c(g) = occurrences of the k-gram g in the training bodies, k = 1..N (a k-gram never crosses a row); T = training body tokens.  For
a query body q and position i: K = min(i + 1, N); j = the largest k in 0..K with c(q[i-k+1 .. i]) > 0; num = c(q[i-j+1 .. i]),
den = c(q[i-j+1 .. i-1]) (T when j = 1); j = 0: num = 1, den = T; cost = log2(den) - log2(num) + (K - j) * -log2(alpha);
fx = round(cost * 2^24).
Three cases by hand, N = 2, training bodies [1, 2, 1, 2, 3] and [2]: T = 6, c(1) = 2, c(2) = 3, c(3) = 1, c(1 2) = 2, c(2 1) = 1,
c(2 3) = 1; gram positions (6, 4), distinct (3, 3).
  a) query [1, 2], alpha = 0.5 (lam = 1): position 0: K = 1, j = 1, num = 2, den = 6, cost = log2 3.  Position 1: K = 2, j = 2,
     num = c(1 2) = 2, den = c(1) = 2, cost = 0.  bits_fx = round(log2(3) * 2^24) = 26591258; n_order = [0, 1, 1].
  b) query [3, 1], alpha = 0.25 (lam = 2): position 0: j = 1, num = 1, den = 6, cost = log2 6.  Position 1: K = 2, (3 1) unseen,
     j = 1, num = c(1) = 2, den = T = 6, back = 1, cost = log2 3 + 2.  bits_fx = round(log2(6) * 2^24) + round((log2(3) + 2) * 2^24)
     = 43368474 + 60145690 = 103514164; n_order = [0, 2, 0].
  c) query [9], alpha = 1 (lam = 0): K = 1, j = 0, num = 1, den = 6, back = 1, cost = log2 6: bits_fx = 43368474; n_order = [1, 0, 0];
     the empty query: n_tokens = 0, bits_fx = 0."""
import math
from collections import Counter

import numpy as np


def bodies(rows, framed):
    return [list(r)[1:-1] if framed else list(r) for r in rows]


def train(rows, N, framed=False):
    """(counts: a list of Counters indexed by k, entry 0 unused; T)"""
    counts = [Counter() for _ in range(N + 1)]
    T = 0
    for b in bodies(rows, framed):
        T += len(b)
        for k in range(1, N + 1):
            for i in range(len(b) - k + 1):
                counts[k][tuple(b[i:i + k])] += 1
    return counts, T


def grams(model, N):
    """(gram positions per order, distinct grams per order), tuples indexed 0..N as NgramLM.n_grams / n_distinct are"""
    counts, T = model
    return (T,) + tuple(sum(counts[k].values()) for k in range(1, N + 1)), (1,) + tuple(len(counts[k]) for k in range(1, N + 1))


def score(model, N, rows, alpha=0.4, framed=False):
    counts, T = model
    lam, R, skip = -math.log2(alpha), len(rows), 1 if framed else 0
    out = dict(n_tokens=np.zeros(R, np.int32), bits_fx=np.zeros(R, np.uint64), n_order=np.zeros((N + 1, R), np.int32))
    cells = []
    for r, (row, q) in enumerate(zip(rows, bodies(rows, framed))):
        mine = [(0, 0, 0)] * len(row)                                     # (j, num, den) per id of the row; the frame cells stay 0
        for i in range(len(q)):
            K = min(i + 1, N)
            j = 0
            while j < K and counts[j + 1][tuple(q[i - j:i + 1])] > 0:
                j += 1
            num = counts[j][tuple(q[i - j + 1:i + 1])] if j else 1
            den = counts[j - 1][tuple(q[i - j + 1:i])] if j > 1 else T
            out["bits_fx"][r] += np.uint64(round((math.log2(den) - math.log2(num) + (K - j) * lam) * 2.0 ** 24))
            out["n_order"][j, r] += 1
            mine[skip + i] = (j, num, den)
        out["n_tokens"][r] = len(q)
        cells += mine
    for c, (name, dtype) in enumerate((("token_order", np.uint8), ("token_num", np.uint32), ("token_den", np.uint32))):
        out[name] = np.array([x[c] for x in cells], dtype)
    out["row_off"] = np.cumsum([0] + [len(r) for r in rows], dtype=np.int64)
    return out
