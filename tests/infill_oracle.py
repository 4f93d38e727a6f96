"""The span-corruption rule of include/genz_tokenize.h ("span-corruption inputs and targets") in plain Python / numpy, for the tests.
Imports nothing of the product: Philox, heads and continuation ids come from mask_oracle, the length laws are restated here.

  protected, continuation, start(r, c), head(r, c), g(r, c), D(g)    as in mask_oracle (the mask rule, unchanged)
  n(r, c)          starts of row r at columns <= c: the cell's word ordinal (counts across protected cells)
  span at a start  begins when D(g(s)).x0 < t_start; len(s) = 1 + #{k : D(g(s)).x1 >= len_t[k]} words, k < n_len - 1
  reach(s)         n(s) + len(s) at a span's start, 0 elsewhere;  far(c) = max of reach over columns <= c
  chosen(r, c)     unprotected and far(head(c)) > n(c)
  run              a maximal stretch of consecutive chosen columns
  E(r)             columns in order: pad -> nothing; not chosen -> the id; first cell of a run -> mask_id; rest of a run -> nothing
  T(r)             per run: mask_id, then the run's ids; one eos closes it: len(T) = n_chosen + n_spans + 1
  input_ids        E then pad;  attention_mask 1 over E then 0;  labels T[:dec_width] then ignore_index;
  decoder_input_ids ([bos] + T[:-1])[:dec_width] then pad;  enc_len = len(E);  dec_len = len(T), unclipped;  n_spans = runs
"""
import math

import numpy as np

import mask_oracle as MO

ONE = 2 ** 32
KEYS = ("input_ids", "attention_mask", "labels", "decoder_input_ids", "enc_len", "dec_len", "n_spans")


def length_law(lengths="geometric", mean_span=3.0, max_span=10):
    """P(len = 1 .. n_len) as a list of floats: the law truncated at max_span and renormalised ("fixed": all mass on mean_span)"""
    if lengths == "fixed":
        m = int(mean_span)
        return [0.0] * (m - 1) + [1.0]
    if lengths == "geometric":
        r = 1.0 / mean_span
        w = [r * (1.0 - r) ** (k - 1) for k in range(1, max_span + 1)]
    elif lengths == "poisson":
        w = [math.exp(-mean_span) * mean_span ** k / math.factorial(k) for k in range(1, max_span + 1)]
    else:
        raise ValueError(lengths)
    s = sum(w)
    return [x / s for x in w]


def tail_of(pmf):
    """P(len > k) for k = 0 .. n_len - 1"""
    return [max(0.0, 1.0 - sum(pmf[:k])) if k else 1.0 for k in range(len(pmf))]


def coverage(q, tail, m=None):
    """the probability that a word with m - 1 words before it in its row (m >= n_len: the whole product) lies inside a span"""
    m = len(tail) if m is None else min(m, len(tail))
    prod = 1.0
    for k in range(m):
        prod *= 1.0 - q * tail[k]
    return 1.0 - prod


def start_share(p, tail):
    """q with coverage(q, tail) == p, by bisection (coverage rises with q from 0 to 1; the two ends are exact)"""
    if p <= 0.0 or p >= 1.0:
        return float(p)
    lo, hi = 0.0, 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if coverage(mid, tail) < p:
            lo = mid
        else:
            hi = mid
    return hi


def rule_ints(p=0.15, mean_span=3.0, max_span=10, lengths="geometric"):
    """(t_start, len_t list of n_len - 1 integers, n_len) the way Tokenize.infill_rows makes them"""
    pmf = length_law(lengths, mean_span, max_span)
    q = start_share(p, tail_of(pmf))
    len_t, acc, last = [], 0.0, 0
    for k in range(len(pmf) - 1):
        acc += pmf[k]
        last = max(last, min(int(min(acc, 1.0) * ONE), ONE))
        len_t.append(last)
    return int(q * ONE), len_t, len(pmf)


def chosen_cells(ids, cont_ids, protected, seed, t_start, len_t, n_len, whole_word, row_base):
    """(prot, start, n, chosen) as [R, L] arrays"""
    ids = np.asarray(ids, dtype=np.int64)
    R, L = ids.shape
    assert 1 <= n_len <= 16 and len(len_t) >= n_len - 1 and 0 <= t_start <= ONE
    assert all(0 <= a <= ONE for a in len_t) and all(a <= b for a, b in zip(len_t[:n_len - 1], len_t[1:n_len - 1]))
    prot, head = MO.heads(ids, cont_ids, protected, whole_word)
    cols = np.arange(L, dtype=np.int64)[None, :]
    start = ~prot & (head == cols)
    n = np.cumsum(start, axis=1).astype(np.int64)
    g = (np.uint64(row_base * L) + (np.arange(R, dtype=np.uint64) * np.uint64(L))[:, None] + np.arange(L, dtype=np.uint64)[None, :]) \
        if R else np.zeros((0, L), dtype=np.uint64)
    x0, x1, _, _ = MO.draw(g, seed)
    length = np.ones((R, L), dtype=np.int64)
    for k in range(n_len - 1):
        length += (x1 >= np.uint64(len_t[k])).astype(np.int64)
    reach = np.where(start & (x0 < np.uint64(t_start)), n + length, 0)
    far = np.maximum.accumulate(reach, axis=1) if L else reach
    return prot, start, n, ~prot & (far > n)                            # (far(head(c)) == far(c): reach is 0 between a head and its cells)


def infill(ids, cont_ids, pad_id, bos_id, eos_id, mask_id, seed=0, t_start=0, len_t=(), n_len=1, whole_word=True, row_base=0,
           ignore_index=-100, dec_width=None):
    """dict of the seven outputs (KEYS), int32"""
    ids = np.asarray(ids, dtype=np.int64)
    R, L = ids.shape
    W = L if dec_width is None else dec_width
    assert W >= 1 and row_base >= 0 and (row_base + R) * L < 2 ** 63
    _, _, _, chosen = chosen_cells(ids, cont_ids, (pad_id, bos_id, eos_id, mask_id), seed, t_start, list(len_t), n_len, whole_word, row_base)
    out = dict(input_ids=np.full((R, L), pad_id, np.int32), attention_mask=np.zeros((R, L), np.int32),
               labels=np.full((R, W), ignore_index, np.int32), decoder_input_ids=np.full((R, W), pad_id, np.int32),
               enc_len=np.zeros(R, np.int32), dec_len=np.zeros(R, np.int32), n_spans=np.zeros(R, np.int32))
    for r in range(R):
        E, T, runs = [], [], 0
        for c in range(L):
            v = int(ids[r, c])
            if chosen[r, c]:
                if c == 0 or not chosen[r, c - 1]:
                    E.append(mask_id)
                    T.append(mask_id)
                    runs += 1
                T.append(v)
            elif v != pad_id:
                E.append(v)
        T.append(eos_id)
        D = [bos_id] + T[:-1]
        out["input_ids"][r, :len(E)] = E
        out["attention_mask"][r, :len(E)] = 1
        out["labels"][r, :min(len(T), W)] = T[:W]
        out["decoder_input_ids"][r, :min(len(D), W)] = D[:W]
        out["enc_len"][r], out["dec_len"][r], out["n_spans"][r] = len(E), len(T), runs
    return out
