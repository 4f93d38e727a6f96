"""The rule of modified Kneser-Ney perplexity (include/genz_tokenize.h, "modified Kneser-Ney perplexity over the n-gram model"), in plain
Python over lm_oracle.train's Counters: sets and dicts of tuples, no hash, every p an exact fractions.Fraction, the cost from
math.log2 of its numerator and denominator, rounded to the 2^24 grid.

For a distinct k-gram g: L(g) = its distinct left neighbours among the (k+1)-grams; a(g) = c(g) if k = N else max(L(g), 1).  For a
context x over the distinct k-grams x.w: A(x) = sum a(x.w), F_j(x) = how many have min(a, 3) = j.  n_j(k) = distinct k-grams with
a = j; Y = n1 / (n1 + 2 n2), D_kj = j - (j + 1) Y n_{j+1} / n_j, or (1/2, 1, 3/2) for the order when an n_j is 0 or a D_kj is not in
(0, j).  p_0 = 1 / (V + 1); for k = 1..K: stop when x = q[i-k+1 .. i-1] is not held or A(x) = 0, else
p_k = (max(a(g) - D_k,min(a,3), 0) + (D_k1 F_1 + D_k2 F_2 + D_k3 F_3)(x) p_{k-1}) / A(x), a(g) = 0 and no discount for an unseen g.
j = the largest k with g seen; cost = -log2 p; fx = round(min(cost, 120) 2^24).
Two cases by hand, N = 2, training bodies [1, 2, 1, 2, 3] and [2] (lm_oracle's): V = 3.  Bigrams (1 2): 2, (2 1): 1, (2 3): 1.  Left
neighbours: 1 <- {2}, 2 <- {1}, 3 <- {2}: a(1) = a(2) = a(3) = 1, the empty context has A = 3, F = (3, 0, 0).  Context (1): A = 2,
F = (0, 1, 0); context (2): A = 2, F = (2, 0, 0); context (3): no follower.  n(1) = (3, 0, 0, 0), n(2) = (2, 1, 0, 0): both orders fall
back to D = (1/2, 1, 3/2).
  a) query [1, 2]: position 0: p_1 = (1 - 1/2 + (3/2)(1/4)) / 3 = 7/24, j = 1.  Position 1: p_1 = 7/24, then x = (1), g = (1 2),
     a = 2: p_2 = (2 - 1 + 1 * 7/24) / 2 = 31/48, j = 2.
  b) query [3, 1, 9]: position 1: p_1 = 7/24, x = (3) is held but has A = 0: stop, p = 7/24, j = 1.  Position 2: 9 unseen:
     p_1 = (0 + (3/2)(1/4)) / 3 = 1/8, then x = (1) is held, g = (1 9) unseen: p_2 = (0 + 1 * 1/8) / 2 = 1/16, j = 0."""
import math
from fractions import Fraction

import numpy as np

import lm_oracle as LO

FALLBACK = (Fraction(1, 2), Fraction(1), Fraction(3, 2))


def derive(model, N):
    """dict(a: per order g -> a(g); ctx: per order k, x -> [A, F1, F2, F3] over the k-grams x.w; n int64 [N, 4]; V; L0: a gram
    below the top order without a left neighbour exists)"""
    counts, _ = model
    left = [dict() for _ in range(N + 1)]
    for k in range(2, N + 1):
        for g in counts[k]:
            left[k - 1].setdefault(g[1:], set()).add(g[0])
    a = [None] + [{g: c if k == N else max(len(left[k].get(g, ())), 1) for g, c in counts[k].items()} for k in range(1, N + 1)]
    ctx, n = [None] + [dict() for _ in range(N)], np.zeros((N, 4), np.int64)
    for k in range(1, N + 1):
        for g, v in a[k].items():
            s = ctx[k].setdefault(g[:-1], [0, 0, 0, 0])
            s[0] += v
            s[min(v, 3)] += 1
            if v <= 4:
                n[k - 1, v - 1] += 1
    return dict(a=a, ctx=ctx, n=n, V=len(counts[1]), L0=any(g not in left[k] for k in range(1, N) for g in counts[k]))


def discounts(n):
    """([N][3] Fractions, [N] fallback flags) from the counts of counts"""
    D, fallback = [], []
    for n1, n2, n3, n4 in np.asarray(n).tolist():
        d = None
        if min(n1, n2, n3, n4) > 0:
            Y = Fraction(n1, n1 + 2 * n2)
            d = (1 - 2 * Y * Fraction(n2, n1), 2 - 3 * Y * Fraction(n3, n2), 3 - 4 * Y * Fraction(n4, n3))
            d = d if all(0 < x < j + 1 for j, x in enumerate(d)) else None
        D.append(d or FALLBACK)
        fallback.append(d is None)
    return D, fallback


def prob(kn, D, N, ctx_ids, w, flags=None):
    """(j, p) of the token w behind the ids ctx_ids (the walk uses the last N - 1 of them)"""
    p, j = Fraction(1, kn["V"] + 1), 0
    for k in range(1, min(len(ctx_ids) + 1, N) + 1):
        x = tuple(ctx_ids[len(ctx_ids) - k + 1:])
        s = kn["ctx"][k].get(x)
        if s is None:                                                     # x is not held, or only at body ends (A = 0)
            if flags is not None and x in kn["a"][k - 1]:
                flags.add("A0")
            break
        v = kn["a"][k].get(x + (w,), 0)
        j = k if v else j
        num = max(v - D[k - 1][min(v, 3) - 1], 0) if v else 0
        p = (num + (D[k - 1][0] * s[1] + D[k - 1][1] * s[2] + D[k - 1][2] * s[3]) * p) / s[0]
    return j, p


def fx_of(p):
    return round(min(math.log2(p.denominator) - math.log2(p.numerator), 120.0) * 2.0 ** 24)


def score(kn, N, rows, D=None, framed=False):
    """lm_oracle.score's outputs under this rule (token_bits_fx for token_num / token_den), plus `flags`: "A0" when a walk stopped at
    a held context without followers.  D: [N][3] numbers (floats are taken exactly); None: the rule's."""
    D = discounts(kn["n"])[0] if D is None else [[Fraction(x) for x in row] for row in np.asarray(D).tolist()]
    R, skip, flags, memo, cells = len(rows), 1 if framed else 0, set(), {}, []
    out = dict(n_tokens=np.zeros(R, np.int32), bits_fx=np.zeros(R, np.uint64), n_order=np.zeros((N + 1, R), np.int32))
    for r, (row, q) in enumerate(zip(rows, LO.bodies(rows, framed))):
        mine = [(0, 0)] * len(row)
        for i in range(len(q)):
            key = tuple(q[max(i - N + 1, 0):i + 1])
            if key not in memo:
                j, p = prob(kn, D, N, key[:-1], key[-1], flags)
                memo[key] = (j, fx_of(p))
            mine[skip + i] = memo[key]
            out["bits_fx"][r] += np.uint64(memo[key][1])
            out["n_order"][memo[key][0], r] += 1
        out["n_tokens"][r] = len(q)
        cells += mine
    out["token_order"] = np.array([c[0] for c in cells], np.uint8)
    out["token_bits_fx"] = np.array([c[1] for c in cells], np.uint32)
    out["row_off"] = np.cumsum([0] + [len(r) for r in rows], dtype=np.int64)
    out["flags"] = flags
    return out
