"""The rule of the hashed n-gram class models (include/genz_tokenize.h, "hashed n-gram class models"), in plain Python.

A feature is a k-gram, k = 1..N, that ends at body position i with k <= i + 1.  Its bucket is the low `bits` bits of the second
MurmurHash3_x86_32 stream (seed 0x9E3779B9) of the language model's backward chain: H_1 = mix(seed, q[i]), H_k = mix(H_{k-1},
q[i-k+1]), bucket = fmix32(H_k ^ 4 k) & (B - 1).  count[b][c] = the features with bucket b in rows of label c; total[c] their sum;
w[b][c] = round(2^24 (log2(total[c] + a B) - log2(count[b][c] + a))) in float64; a row's bits_fx[c] = the sum of w[bucket][c] over
its features; best = the class with the smallest sum, the smallest class on ties, -1 for a row without features."""
import math

import numpy as np

M = 0xFFFFFFFF
SEED2 = 0x9E3779B9


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def _mix(h, x):
    k = ((x & M) * 0xCC9E2D51) & M
    k = (_rotl(k, 15) * 0x1B873593) & M
    return (_rotl(h ^ k, 13) * 5 + 0xE6546B64) & M


def _fmix(x):
    x ^= x >> 16; x = (x * 0x85EBCA6B) & M
    x ^= x >> 13; x = (x * 0xC2B2AE35) & M
    return x ^ (x >> 16)


def bodies(rows, framed):
    return [list(r)[1:-1] if framed else list(r) for r in rows]


def features(q, N, bits):
    """[(bucket, gram)] of the body q: for every end position the grams of order 1..min(i + 1, N)"""
    out = []
    for i in range(len(q)):
        h = SEED2
        for k in range(1, min(i + 1, N) + 1):
            h = _mix(h, q[i - k + 1])
            out.append((_fmix(h ^ (4 * k)) & ((1 << bits) - 1), tuple(q[i - k + 1:i + 1])))
    return out


def fit(rows, labels, N, bits, C, framed=False):
    """(count int64 [B, C], the set of distinct grams of every bucket)"""
    count, grams = np.zeros((1 << bits, C), np.int64), {}
    for q, c in zip(bodies(rows, framed), labels):
        for b, g in features(q, N, bits):
            count[b, c] += 1
            grams.setdefault(b, set()).add(g)
    return count, grams


def weights(count, a=1.0):
    B, C = count.shape
    total = count.sum(axis=0)
    w = np.zeros((B, C), np.int64)
    for c in range(C):
        top = math.log2(float(total[c]) + a * B)
        for v in np.unique(count[:, c]):                                  # (few distinct counts: one log2 each)
            w[count[:, c] == v, c] = round(2.0 ** 24 * (top - math.log2(float(v) + a)))
    return w


def score(w, N, bits, rows, framed=False):
    """n_features, bits_fx [C, R], best, and `buckets`: per row the array of its features' buckets (for sums over another table)"""
    C, R = w.shape[1], len(rows)
    out = dict(n_features=np.zeros(R, np.int32), bits_fx=np.zeros((C, R), np.int64), best=np.full(R, -1, np.int32), buckets=[])
    for r, q in enumerate(bodies(rows, framed)):
        bs = np.array([b for b, _ in features(q, N, bits)], dtype=np.int64)
        out["buckets"].append(bs)
        out["n_features"][r] = len(bs)
        out["bits_fx"][:, r] = w[bs].sum(axis=0) if len(bs) else 0
        if len(bs):
            out["best"][r] = int(np.argmin(out["bits_fx"][:, r]))      # (the first of equal minima)
    return out


def decided(want):
    """rows whose two smallest class sums differ by more than 2 n_features: a weight off by one a feature cannot change their best
    (rows of one class or without features have nothing to decide)"""
    s, n = np.sort(want["bits_fx"], axis=0), want["n_features"].astype(np.int64)
    return np.ones(len(n), bool) if len(s) < 2 else ((s[1] - s[0]) > 2 * n) | (n == 0)
