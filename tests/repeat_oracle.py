"""The rule of the n-gram repetition calls (include/genz_tokenize.h, "repeats: n-gram repetition inside a document") in plain Python:
collections.Counter over tuples.  Nothing of the product is imported and no hash is used.

The body q of a row is the row without its skips, exactly as in MinHash and n-gram overlap (skip_front, skip_back in {0, 1}).  It has
m ids.  widths is a list of 1..16 distinct integers, each in 1..32, in the caller's order; k indexes it.

For width n, the n-grams of the body are the G = max(0, m - n + 1) runs q[i:i+n].  A body shorter than n has none.  c(g) is the number
of positions whose n-gram is g; occurrences may overlap, so [5, 5, 5] holds (5, 5) twice.  first(g) is the smallest such position.

Per row r and width k, all int32 and laid out [K, N]:

n_grams[k, r]     G.
n_distinct[k, r]  number of different n-grams.  G - n_distinct is then the number of later occurrences, which is what some
                  implementations of the Gopher rule count.
n_repeated[k, r]  positions i with c(q[i:i+n]) >= 2.  The first occurrence counts too.
n_covered[k, r]   body tokens t with some repeated position i, i <= t < i + n.  Each token counts once.
top_count[k, r]   max c(g), or 0 when G == 0.
top_pos[k, r]     first(g) of the n-gram with the largest count.  Among equal counts it is the one with the smallest first.  It is -1
                  when G == 0.
covered           optionally: one uint16 per id of the input in the input's own layout.  Bit k is set when the token is covered at
                  widths[k].  It is 0 on frame cells.

A row's outputs depend on its own body and widths alone, never on another row, even an identical neighbour:
repetition(rows[a:b]) == repetition(rows)[:, a:b], so shards concatenate; they are a pure function of (rows, widths), not of launch
geometry, scheduling or the hash.  A hash decides where to look, never whether two n-grams are equal, nor whether they stand in the
same row.
"""
from collections import Counter

import numpy as np

KEYS = ("n_grams", "n_distinct", "n_repeated", "n_covered", "top_count", "top_pos")


def body(row, framed):
    row = [int(v) for v in row]
    return row[1:-1] if framed else row


def grams(b, n):
    return [tuple(b[i:i + n]) for i in range(len(b) - n + 1)]


def one(b, n):
    """the six outputs of one body at one width, in KEYS' order, and its covered flags (0 / 1 per body token)"""
    g = grams(b, n)
    c = Counter(g)
    first = {}
    for i, x in enumerate(g):
        first.setdefault(x, i)
    cov = [0] * len(b)
    repeated = 0
    for i, x in enumerate(g):
        if c[x] >= 2:
            repeated += 1
            for t in range(i, i + n):
                cov[t] = 1
    if g:
        top = max(c.values())
        pos = min(first[x] for x in c if c[x] == top)
    else:
        top, pos = 0, -1
    return (len(g), len(c), repeated, sum(cov), top, pos), cov


def repetition(rows, widths, framed=False):
    """dict of int32 [K, N] arrays under KEYS, body_len int32 [N], covered (uint16 over the rows back to back) and row_off (int64 [N + 1])"""
    K, N = len(widths), len(rows)
    out = {k: np.zeros((K, N), dtype=np.int32) for k in KEYS}
    flat, off, lens = [], [0], []
    for r, row in enumerate(rows):
        row = [int(v) for v in row]
        b = body(row, framed)
        bits = [0] * len(b)
        for k, n in enumerate(widths):
            vals, cov = one(b, n)
            for key, v in zip(KEYS, vals):
                out[key][k, r] = v
            bits = [x | (y << k) for x, y in zip(bits, cov)]
        cells = ([0] + bits + [0] if len(row) >= 2 else [0] * len(row)) if framed else bits
        assert len(cells) == len(row)
        flat += cells
        off.append(len(flat))
        lens.append(len(b))
    out["body_len"] = np.array(lens, dtype=np.int32)
    out["covered"] = np.array(flat, dtype=np.uint16)
    out["row_off"] = np.array(off, dtype=np.int64)
    return out
