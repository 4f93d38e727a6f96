"""The rule of the n-gram overlap calls (include/genz_tokenize.h, "token n-gram overlap against a held-out set") in plain Python:
sets and dicts of tuples.  Nothing of the product is imported and no hash is used.

body of a row      the row without its first and last entry when framed (a row shorter than its frame has an empty body)
n-grams            the max(0, m - n + 1) runs body[i : i + n]; a body shorter than n has none
index              first[g] = the smallest reference row that holds n-gram g
query, per row     n_grams, n_hits (positions whose n-gram is in the index), n_covered (body tokens inside some such n-gram),
                   first_hit (smallest such position, -1), first_ref (first of that n-gram, -1), body_len; covered: one 0 / 1 per id
                   of the row, frame cells 0
"""
import numpy as np

KEYS = ("n_grams", "n_hits", "n_covered", "first_hit", "first_ref", "body_len")


def body(row, framed):
    row = [int(v) for v in row]
    return row[1:-1] if framed else row


def grams(b, n):
    return [tuple(b[i:i + n]) for i in range(len(b) - n + 1)]


def index(ref_rows, n, framed=False):
    """dict: n-gram -> the smallest reference row that holds it"""
    first = {}
    for r, row in enumerate(ref_rows):
        for g in grams(body(row, framed), n):
            first.setdefault(g, r)
    return first


def positions(ref_rows, n, framed=False):
    return sum(len(grams(body(row, framed), n)) for row in ref_rows)


def row(first, n, b):
    """the outputs of one body, and its covered flags"""
    g = grams(b, n)
    hit = [x in first for x in g]
    cov = [0] * len(b)
    for i, h in enumerate(hit):
        if h:
            for t in range(i, i + n):
                cov[t] = 1
    fh = hit.index(True) if any(hit) else -1
    return (len(g), sum(hit), sum(cov), fh, first[g[fh]] if fh >= 0 else -1, len(b)), cov


def overlap(first, n, rows, framed=False):
    """dict of int32 [N] arrays under KEYS, plus covered (uint8 over the rows back to back) and row_off (int64 [N + 1])"""
    out, flat, off = [], [], [0]
    for r in rows:
        r = [int(v) for v in r]
        vals, cov = row(first, n, body(r, framed))
        out.append(vals)
        cells = ([0] + cov + [0] if len(r) >= 2 else [0] * len(r)) if framed else cov
        assert len(cells) == len(r)
        flat += cells
        off.append(len(flat))
    a = np.array(out, dtype=np.int32).reshape(len(rows), len(KEYS))
    res = {k: a[:, i].copy() for i, k in enumerate(KEYS)}
    res["covered"] = np.array(flat, dtype=np.uint8)
    res["row_off"] = np.array(off, dtype=np.int64)
    return res
