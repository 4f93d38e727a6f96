"""GPU: gz_topk_kernel (csrc/gz_topk.inc), and the search that ranks through it, over score rows that BM25 does not produce: keys that
differ only in their lowest bytes, denormals, +-DBL_MAX, rows that rise or fall strictly with the document index.

The caller supplies idf, so any finite row can be made a score row: N one-word documents w0 .. wN-1, k1 = 1 and b = 0 (params
[2.0, 1.0, 1.0, 0.0, avg, 0.0]: K = 1, t = (1 * 2) / (1 + 1) = 1 where the word is present, t0 = 0 where it is not) and a query of
all N words.  Document d's score is 0.0 + (+-0.0) ... + idf[d] * 1 + (+-0.0) ...: the idf array bit for bit, -0.0 becoming +0.0.  The
identity needs finite values (inf * 0 poisons the row); NaN and -inf rows are in test_gpu_bm25_topk.py and test_gpu_bm25_search_bool.py.
With plus = 1 and delta = 0.0 the kernel takes the BM25Plus path (t + delta) and the identity still holds.

Oracle: np.argsort(-row, kind="stable") and the row's bits; for the search every document matches, so it is the same order and the
count is N.  Compared with == and as uint64 bit patterns."""
import numpy as np
import pytest

import bm25_restate as R
from bm25_oracles import bits, check, same, topk_check
from genz_tokenize import _native
from genz_tokenize.ranking import BM25

pytestmark = pytest.mark.gpu

N = 4500                         # with the largest tile (4096): two tiles, the second of 404 elements -- fewer than k = 1024
KS = (1, 2, 255, 256, 257, 1000, 1024)
TILES = (0, 64, 300, 4096)
DBL_MAX = np.finfo(np.float64).max


def make_rows():
    r = np.random.default_rng(61)
    i = np.arange(N, dtype=np.uint64)
    one = np.float64(1.0).view(np.uint64)
    b = r.integers(0, 2**64, N, dtype=np.uint64)
    b[(b >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF)] &= ~np.uint64(1 << 62)        # (inf and NaN patterns made finite)
    rising = np.arange(N) * 0.5 - 1000.0
    rows = {
        "standard normal": r.standard_normal(N),
        "random finite bit patterns": b.view(np.float64),
        "1 + (i % 256) ulp": (one + i % np.uint64(256)).view(np.float64),
        "1 + i ulp": (one + i).view(np.float64),
        "i * 5e-324, signs mixed": np.arange(N) * 5e-324 * np.where(r.random(N) < 0.5, -1.0, 1.0),
        "-DBL_MAX then +DBL_MAX": np.where(np.arange(N) < N // 2, -DBL_MAX, DBL_MAX),
        "all equal": np.full(N, 0.375),
        "strictly ascending": rising,
        "strictly descending": -rising,
        "zeros, one positive at N - 1": np.concatenate([np.zeros(N - 1), [3.0]]),
    }
    for name, v in rows.items():
        assert v.dtype == np.float64 and v.shape == (N,) and np.isfinite(v).all(), name
    assert len(np.unique(bits(rows["1 + i ulp"]) >> np.uint64(16))) == 1                      # distinct in the lowest two bytes only
    assert (rows["i * 5e-324, signs mixed"][1:] != 0).all() and np.signbit(rows["i * 5e-324, signs mixed"]).any()
    assert (np.diff(rising) > 0).all() and rising[0] < 0 < rising[-1]
    return rows


@pytest.fixture(scope="module")
def rows():
    return make_rows()


def index(tile):
    """(context, model) over the N one-word documents, with the first selection level's tile forced (0: chosen by the library)"""
    ctx = _native.Context()
    _native.debug_set("bm25_topk_tile", tile, ctx)
    m = BM25(["w%d" % i for i in range(N)], b=0.0, k1=1.0, ctx=ctx)
    return ctx, m


def query_arrays(m, n_rows):
    terms = m._lookup(["w%d" % i for i in range(N)])[0]
    assert sorted(terms.tolist()) == list(range(N))
    return np.tile(terms, n_rows), np.arange(n_rows + 1, dtype=np.int64) * N


@pytest.mark.parametrize("plus", [False, True])
def test_topk_and_search_over_arbitrary_rows(rows, plus):
    names = list(rows)
    idf = np.stack([rows[x] for x in names])
    S = idf + 0.0
    every = np.ones((len(names), N), dtype=bool)
    first = {}
    for tile in TILES:
        ctx, m = index(tile)
        P = m._params()
        assert P == [2.0, 1.0, 1.0, 0.0, 1.0, 0.0]
        terms, qoff = query_arrays(m, len(names))
        got = ctx.bm25_score(m._index, terms, idf.ravel(), qoff, P, plus)
        for q, name in enumerate(names):                                 # the identity: the score rows are the idf rows
            assert np.array_equal(bits(got[q]), bits(S[q])), (name, tile)
        if tile == 0:                                                    # ... and one row restated, to anchor it
            q = names.index("random finite bit patterns")
            post = R.Postings(m.frequency_word_in_doc)
            one = R.scores(m.fieldLens, post, R.avg_field_len(m.fieldLens), ["w%d" % i for i in range(N)], idf[q], 0.0, 1.0, 0.0 if plus else None)
            assert np.array_equal(bits(one), bits(S[q]))
        for k in KS:
            top = ctx.bm25_topk(m._index, terms, idf.ravel(), qoff, P, plus, k)
            for q, name in enumerate(names):
                topk_check((top[0][q:q + 1], top[1][q:q + 1]), S[q:q + 1], k, (name, tile, k))
            found = ctx.bm25_search(m._index, terms, idf.ravel(), qoff, P, plus, k)
            assert found[2].tolist() == [N] * len(names), (tile, k)
            for q, name in enumerate(names):
                check(tuple(x[q:q + 1] for x in found), S[q:q + 1], every[q:q + 1], k, (name, tile, k))
            assert same(found[:2], top), (tile, k)
            if tile == TILES[0]:
                first[k] = top
            else:
                assert same(top, first[k]), (tile, k)                    # every tile setting: the same answer
        del m
        ctx.close()
    # what the rows are there for
    top = first[1024]
    q = names.index("1 + (i % 256) ulp")                                 # ties that the last digit resolves: 255 first, each in index order
    assert top[0][q, :36].tolist() == [i for v in (255, 254, 253) for i in range(v, N, 256)][:36]
    q = names.index("all equal")
    assert top[0][q].tolist() == list(range(1024))
    q = names.index("strictly ascending")
    assert top[0][q].tolist() == list(range(N - 1, N - 1025, -1))
    q = names.index("strictly descending")
    assert top[0][q].tolist() == list(range(1024))
    q = names.index("zeros, one positive at N - 1")
    assert top[0][q].tolist() == [N - 1] + list(range(1023))
    q = names.index("-DBL_MAX then +DBL_MAX")
    assert top[0][q].tolist() == list(range(N // 2, N // 2 + 1024))


def test_bm25plus_rows_through_the_selection(rows):
    """BM25Plus(b=0.3, k1=2.0, delta=0.5) over the same documents and idf rows: the scores are no longer the idf (every word adds
    idf * delta to every document), so the rows are the kernel's own, one of them restated; the selection is checked against them."""
    names = ["standard normal", "1 + i ulp", "strictly descending", "all equal"]
    idf = np.stack([rows[x] for x in names])
    every = np.ones((1, N), dtype=bool)
    first = {}
    for tile in (0, 300):
        ctx, m = index(tile)
        P = [3.0, 2.0, float(1 - 0.3), 0.3, float(m.avgFieldLen), 0.5]
        terms, qoff = query_arrays(m, len(names))
        S = ctx.bm25_score(m._index, terms, idf.ravel(), qoff, P, True)
        if tile == 0:
            post = R.Postings(m.frequency_word_in_doc)
            one = R.scores(m.fieldLens, post, R.avg_field_len(m.fieldLens), ["w%d" % i for i in range(N)], idf[0], 0.3, 2.0, 0.5)
            assert np.array_equal(bits(one), bits(S[0]))
        for k in (1, 257, 1024):
            top = ctx.bm25_topk(m._index, terms, idf.ravel(), qoff, P, True, k)
            found = ctx.bm25_search(m._index, terms, idf.ravel(), qoff, P, True, k)
            for q, name in enumerate(names):
                topk_check((top[0][q:q + 1], top[1][q:q + 1]), S[q:q + 1], k, (name, tile, k))
                check(tuple(x[q:q + 1] for x in found), S[q:q + 1], every, k, (name, tile, k))
            if tile == 0:
                first[k] = top
            else:
                assert same(top, first[k]), (tile, k)
        del m
        ctx.close()
