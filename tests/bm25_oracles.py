"""Oracles shared by the BM25 GPU tests (numpy only; nothing here touches the GPU).

    restate(m, queries)              get_scores: bm25_restate.scores row by row, the reference's arithmetic in its order
    topk_oracle / topk_check         top_k: np.argsort(-S, kind="stable")[:k'] and the scores' original bits
    matched / oracle / check         search, count_matches: with R = set(query.split()), X = set(exclude.split()) and W(d) the words of
                                     document d,  "any": R & W(d) and not X & W(d)    "all": R and R <= W(d) and not X & W(d);
                                     row q = [i for i in argsort(-S[q], stable) if matched[q, i]][:k'], -1 / the NaN PAD behind it
    gather / check_rows              the same for a batch that repeats a few distinct (query, exclude) pairs: the oracle once per
                                     pair, its rows gathered
ids and counts are compared with ==, scores as uint64 bit patterns: there are no tolerances."""
import numpy as np

import bm25_restate as R
from genz_tokenize.ranking import BM25, BM25Plus

PAD = np.uint64(0x7FF8000000000000)
MODES = ("any", "all")
CLASSES = ("BM25", "BM25Plus")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model(cls, docs, ctx=None):
    """BM25 with its defaults, BM25Plus with b=0.3, k1=2.0, delta=0.5"""
    return BM25Plus(docs, 0.3, 2.0, 0.5, ctx=ctx) if cls == "BM25Plus" else BM25(docs, ctx=ctx)


def restate(m, queries, post=None):
    """float64 [len(queries), num_doc]: what get_scores(queries) must return, to the bit"""
    if post is None:
        post = R.Postings(m.frequency_word_in_doc)
    lens = m.fieldLens
    avg = R.avg_field_len(lens)
    delta = getattr(m, "delta", None)
    idf = {}
    out = np.zeros((len(queries), m.num_doc), dtype=np.float64)
    for q, text in enumerate(queries):
        words = text.split()
        for w in words:
            if w not in idf:
                idf[w] = R.idf(m.num_doc, post.df(w))
        if words:
            out[q] = R.scores(lens, post, avg, words, [idf[w] for w in words], m.b, m.k1, delta)
    return out


def topk_oracle(S, k):
    S = np.asarray(S, dtype=np.float64)
    kk = min(k, S.shape[1])
    ids = np.argsort(-S, axis=1, kind="stable")[:, :kk].astype(np.int64)
    return ids, bits(np.take_along_axis(S, ids, 1))


def topk_check(got, S, k, what=""):
    ids, sc = got
    want_ids, want_sc = topk_oracle(S, k)
    assert ids.dtype == np.int64 and sc.dtype == np.float64, what
    assert ids.shape == want_ids.shape and sc.shape == want_sc.shape, (what, ids.shape, want_ids.shape)
    assert np.array_equal(ids, want_ids), what
    assert np.array_equal(bits(sc), want_sc), what


def matched(post, queries, match="any", exclude=None):
    m = np.zeros((len(queries), post.n), dtype=bool)
    for q, text in enumerate(queries):
        need = set(text.split())
        if match == "any":
            for w in need:
                if w in post.p:
                    m[q, post.p[w][0]] = True
        elif need and all(w in post.p for w in need):
            m[q] = True
            for w in need:
                has = np.zeros(post.n, dtype=bool)
                has[post.p[w][0]] = True
                m[q] &= has
        if exclude is not None:
            for w in set(exclude[q].split()):
                if w in post.p:
                    m[q, post.p[w][0]] = False
    return m


def oracle(S, m, k):
    """(ids int64, scores as uint64 bits, counts int64) of search(queries, k) for the score rows S and the matched sets m"""
    S = np.asarray(S, dtype=np.float64)
    nq, n = S.shape
    kk = min(k, n)
    ids = np.full((nq, kk), -1, dtype=np.int64)
    sc = np.full((nq, kk), PAD, dtype=np.uint64)
    order = np.argsort(-S, axis=1, kind="stable")
    for q in range(nq):
        o = order[q][m[q][order[q]]][:kk]
        ids[q, :len(o)] = o
        sc[q, :len(o)] = bits(S[q, o])
    return ids, sc, m.sum(axis=1).astype(np.int64)


def gather(want, rows):
    """the oracle of a batch whose row r is the oracle's row rows[r]"""
    return tuple(x[rows] for x in want)


def check_rows(got, want, what=""):
    ids, sc, cnt = got
    want_ids, want_sc, want_cnt = want
    assert ids.dtype == np.int64 and sc.dtype == np.float64 and cnt.dtype == np.int64, what
    assert ids.shape == want_ids.shape and sc.shape == want_sc.shape and cnt.shape == want_cnt.shape, (what, ids.shape, want_ids.shape)
    assert np.array_equal(cnt, want_cnt), (what, np.flatnonzero(cnt != want_cnt)[:10].tolist())
    assert np.array_equal(ids, want_ids), (what, np.flatnonzero((ids != want_ids).any(axis=1))[:10].tolist())
    assert np.array_equal(bits(sc), want_sc), (what, np.flatnonzero((bits(sc) != want_sc).any(axis=1))[:10].tolist())


def check(got, S, m, k, what=""):
    check_rows(got, oracle(S, m, k), what)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))
