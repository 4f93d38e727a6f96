"""GPU: the QUERY side of BM25 scoring, top-k and search -- long queries, many queries, offsets that do not start at 0 -- where the other
BM25 test files vary the documents.  What runs here and nowhere else:
    A  gz_bm25_score_kernel's later trips of the query-word staging loop (BM_QW_LDS = 512 words a trip): a query across a trip, a query
       that ends on a trip boundary, empty queries on it, a batch of only empty queries; gz_bm25_sr_driver_kernel past 256 rows
    B  query_off[0] != 0 and ex_off[0] != 0 on the native entry points
    C  gz_bm25_sr_mark_kernel's stride: more slices than its 2048 workgroups
    D  more rows than a grid dimension (65 535): the second chunk of bm25_topk_locked / bm25_search_locked
Oracles (bm25_oracles.py): bm25_restate.scores for get_scores, the stable argsort for top_k, the matched sets for search and
count_matches, both modes, with and without exclusions; BM25 and BM25Plus(b=0.3, k1=2.0, delta=0.5).  Everything is compared as bit
patterns or with ==."""
import numpy as np
import pytest

import bm25_restate as R
from bm25_oracles import CLASSES, MODES, bits, check, check_rows, gather, matched, model, oracle, restate, same, topk_check, topk_oracle
from genz_tokenize import _native

pytestmark = pytest.mark.gpu

N_DOCS = 300                     # one full scoring workgroup (256 documents) and one of 44 with idle lanes
SC_LDS = 4096                    # BM_SC_LDS: the (term, count) entries a scoring workgroup stages in LDS


def make_short():
    r = np.random.default_rng(101)
    vocab = ["s%d" % i for i in range(40)]
    docs = [" ".join(vocab[int(x)] for x in r.integers(0, 40, int(r.integers(1, 9)))) for _ in range(N_DOCS)]
    docs[17] = ""
    return docs, vocab


def make_wide():
    r = np.random.default_rng(102)
    vocab = ["v%d" % i for i in range(200)]
    docs = []
    for i in range(N_DOCS):
        words = [vocab[int(x)] for x in r.choice(200, 24, replace=False)]
        docs.append(" ".join(words + words[:i % 3]))                      # (24 entries; some counts of 2)
    return docs, vocab


def draw(r, vocab, n):
    """n words of the vocabulary, repeats included, about one in ten replaced by a word no document holds"""
    pick, absent = r.integers(0, len(vocab), n), r.random(n) < 0.1
    return " ".join("zz%d" % pick[i] if absent[i] else vocab[int(pick[i])] for i in range(n))


def make_batch(vocab, lengths, seed):
    r = np.random.default_rng(seed)
    queries = [draw(r, vocab, n) for n in lengths]
    exclude = [draw(r, vocab, int(r.integers(0, 3))) for _ in lengths]
    return queries, exclude


BATCHES = {
    "511": [511], "512": [512], "513": [513], "1024": [1024], "1025": [1025], "1537": [1537],
    "512,512,513": [512, 512, 513], "511,1,512,1": [511, 1, 512, 1], "300,212,0,700,0": [300, 212, 0, 700, 0],
    "0,512,0,0,512,0": [0, 512, 0, 0, 512, 0], "600 empty": [0] * 600, "1537 of one word": [1] * 1537,
}


@pytest.fixture(scope="module")
def corpora():
    out = {}
    for name, make in (("short", make_short), ("wide", make_wide)):
        docs, vocab = make()
        out[name] = (docs, vocab, R.Postings(R.stats(docs)[1]))
    return out


def check_batch(m, post, queries, exclude, what):
    """get_scores, top_k(5), search(5) and count_matches of one batch; returns {(mode, exclusions?): matched}"""
    S = restate(m, queries, post)
    got = m.get_scores(queries)
    assert got.dtype == np.float64 and got.shape == S.shape, what
    assert np.array_equal(bits(got), bits(S)), (what, np.flatnonzero((bits(got) != bits(S)).any(axis=1))[:10].tolist())
    topk_check(m.top_k(queries, 5), S, 5, what)
    out = {}
    for mode in MODES:
        for ex in (None, exclude):
            mt = out[mode, ex is not None] = matched(post, queries, mode, ex)
            check(m.search(queries, 5, match=mode, exclude=ex), S, mt, 5, (what, mode, ex is not None))
            assert np.array_equal(m.count_matches(queries, match=mode, exclude=ex), mt.sum(axis=1)), (what, mode, ex is not None)
    return out


def staged_entries(m):
    """the (term, count) entries of each scoring workgroup's documents"""
    n = [len(f) for f in m.frequency_word_in_doc]
    return [sum(n[i:i + 256]) for i in range(0, len(n), 256)]


# ---- A: word-chunk edges of the scoring kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ["short", "wide"])
def test_word_chunk_edges(corpora, name, cls, batch):
    docs, vocab, post = corpora[name]
    m = model(cls, docs)
    e = staged_entries(m)
    if name == "short":
        assert len(e) == 2 and max(e) <= SC_LDS and "" in docs           # both workgroups stage their entries in LDS
    else:
        assert e == [6144, 1056] and e[0] > SC_LDS >= e[1]               # the first takes the pair table, the second stages
    queries, exclude = make_batch(vocab, BATCHES[batch], 1000 + len(batch) + sum(BATCHES[batch]))
    mt = check_batch(m, post, queries, exclude, (name, cls, batch))
    if batch == "1537 of one word":                                      # one word: both modes are the word's documents
        assert np.array_equal(mt["any", False], mt["all", False]) and (mt["all", False].sum(axis=1) > 0).sum() > 1000


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ["short", "wide"])
def test_own_words_repeated_past_a_trip(corpora, name, cls):
    """every query is one document's distinct words, repeated until they pass a trip of 512: match="all" finds that document"""
    docs, vocab, post = corpora[name]
    m = model(cls, docs)
    own = [0, 100, 255, 256, 299] + ([min(range(N_DOCS), key=lambda d: len(set(docs[d].split())) or 99)] if name == "short" else [])
    queries = []
    for d in own:
        words = list(dict.fromkeys(docs[d].split()))
        queries.append(" ".join(words * (22 if name == "wide" else -(-513 // len(words)))))
        assert len(queries[-1].split()) > 512
    if name == "wide":
        assert all(len(q.split()) == 528 for q in queries)
    r = np.random.default_rng(7)
    exclude = ["" if i % 2 == 0 else draw(r, vocab, 1) for i in range(len(own))]
    mt = check_batch(m, post, queries, exclude, (name, cls))
    for q, d in enumerate(own):
        assert mt["all", False][q, d], (name, d)
    got = m.search(queries, 5, match="all")
    for q, d in enumerate(own):
        assert got[2][q] >= 1 and (d in got[0][q].tolist() or got[2][q] > 5), (name, d)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ["short", "wide"])
def test_row_chunks_start_inside_a_trip(corpora, name, cls):
    """bm25_topk_chunk = 2 rows of scores: the chunks' first words are 400, 800, ... -- no multiple of 512; and two-row search chunks"""
    docs, vocab, post = corpora[name]
    queries, exclude = make_batch(vocab, [200] * 9, 77)
    ctx = _native.Context()
    _native.debug_set("bm25_topk_chunk", 2 * N_DOCS, ctx)
    _native.debug_set("bm25_search_chunk", 2 * ((N_DOCS + 63) // 64), ctx)
    m = model(cls, docs, ctx=ctx)
    S = restate(m, queries, post)
    topk_check(m.top_k(queries, 5), S, 5, (name, cls))
    for mode in MODES:
        check(m.search(queries, 5, match=mode, exclude=exclude), S, matched(post, queries, mode, exclude), 5, (name, cls, mode))
    del m
    ctx.close()


# ---- B: offsets that do not start at 0 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", ["short", "wide"])
def test_offsets_not_from_zero(corpora, name, cls):
    docs, vocab, post = corpora[name]
    m = model(cls, docs)
    ctx, ix, P, plus = m._ctx, m._index, m._params(), cls == "BM25Plus"
    queries, _ = make_batch(vocab, [300, 212, 0, 700, 0], 55)
    r = np.random.default_rng(56)
    exclude = [draw(r, vocab, q % 3) for q in range(5)]
    nq, terms, idf, qoff = m._queries(queries)
    xt, xo = m._exclusions(exclude, nq)
    assert qoff[0] == 0 and xo[0] == 0 and xo[-1] > 0
    front, xfront = 37, 11                                               # filler in front (and behind): term -1, idf NaN
    terms2 = np.concatenate([np.full(front, -1, np.int32), terms, np.full(5, -1, np.int32)])
    idf2 = np.concatenate([np.full(front, np.nan), idf, np.full(5, np.nan)])
    xt2 = np.concatenate([np.full(xfront, -1, np.int32), xt, np.full(3, -1, np.int32)])
    qoff2, xo2 = qoff + front, xo + xfront
    S = restate(m, queries, post)
    plain = ctx.bm25_score(ix, terms, idf, qoff, P, plus)
    assert np.array_equal(bits(plain), bits(S))
    assert np.array_equal(bits(ctx.bm25_score(ix, terms2, idf2, qoff2, P, plus)), bits(plain))
    want = ctx.bm25_topk(ix, terms, idf, qoff, P, plus, 5)
    topk_check(want, S, 5, (name, cls))
    assert same(ctx.bm25_topk(ix, terms2, idf2, qoff2, P, plus, 5), want)
    for mode in (0, 1):
        for a, b in ((dict(mode=mode), dict(mode=mode)), (dict(mode=mode, ex_terms=xt, ex_off=xo), dict(mode=mode, ex_terms=xt2, ex_off=xo2))):
            mt = matched(post, queries, MODES[mode], exclude if "ex_off" in a else None)
            want = ctx.bm25_search(ix, terms, idf, qoff, P, plus, 5, **a)
            check(want, S, mt, 5, (name, cls, mode, sorted(a)))
            assert same(ctx.bm25_search(ix, terms2, idf2, qoff2, P, plus, 5, **b), want), (name, cls, mode, sorted(a))
            cnt = ctx.bm25_match_count(ix, terms2, qoff2, **b)
            assert cnt.dtype == np.int64 and np.array_equal(cnt, mt.sum(axis=1)), (name, cls, mode, sorted(a))
        # (only the queries shifted, and only the exclusions)
        full = dict(mode=mode, ex_terms=xt, ex_off=xo)
        want = ctx.bm25_search(ix, terms, idf, qoff, P, plus, 5, **full)
        assert same(ctx.bm25_search(ix, terms2, idf2, qoff2, P, plus, 5, **full), want)
        assert same(ctx.bm25_search(ix, terms, idf, qoff, P, plus, 5, mode=mode, ex_terms=xt2, ex_off=xo2), want)


# ---- C: the marking kernel strides over more slices than it has workgroups ---------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_marking_stride(cls):
    n = 4100
    docs = [" ".join(["ev"] + (["h"] if i % 3 == 0 else []) + ["pad"] * (i % 4)) for i in range(n)]
    distinct = ["ev", "ev h", "h ev"]
    r = np.random.default_rng(31)
    qi = r.integers(0, 3, 720)
    queries = [distinct[int(i)] for i in qi]
    exclude = ["h" if q % 2 else "" for q in range(720)]
    m = model(cls, docs)
    words, df = m.vocabulary()
    df = dict(zip(words, df.tolist()))
    assert df == {"ev": n, "h": (n + 2) // 3, "pad": n - (n + 3) // 4}
    slices = sum(-(-df[w] // 2048) for q in queries for w in q.split())
    assert slices > 2048, slices                                         # gz_bm25_sr_mark_kernel launches 2048 workgroups at the most
    post = R.Postings(m.frequency_word_in_doc)
    # the oracle once per distinct (query, exclusion) pair: pair p = query p // 2, "h" excluded when p is odd
    pq, px = [distinct[p // 2] for p in range(6)], ["h" if p % 2 else "" for p in range(6)]
    S = restate(m, pq, post)
    rows = 2 * qi + (np.arange(720) % 2)
    for mode in MODES:
        mt = matched(post, pq, mode, px)
        check_rows(m.search(queries, 3, match=mode, exclude=exclude), gather(oracle(S, mt, 3), rows), (cls, mode))
        assert np.array_equal(m.count_matches(queries, match=mode, exclude=exclude), mt.sum(axis=1)[rows]), (cls, mode)
        mt = matched(post, pq, mode)
        check_rows(m.search(queries, 3, match=mode), gather(oracle(S, mt, 3), rows), (cls, mode, "no exclusions"))
        assert np.array_equal(m.count_matches(queries, match=mode), mt.sum(axis=1)[rows]), (cls, mode, "no exclusions")
    cnt = m.count_matches(queries, exclude=exclude)
    assert set(cnt.tolist()) == {n, n - df["h"]} and cnt[-1] == n - df["h"]            # (the last rows are marked too)


# ---- D: more rows than a grid dimension ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_more_rows_than_a_grid_dimension(cls):
    n, nq = 70, 65_537                                                   # two bitmap words, the second partly used; 65 535 + 2 rows
    r = np.random.default_rng(41)
    vocab = ["d%d" % i for i in range(12)]
    docs = [" ".join(vocab[int(x)] for x in r.integers(0, 12, int(r.integers(0, 7)))) for _ in range(n)]
    docs[5] = ""
    distinct = ["d1 d2", "d0", "d3 d0 d3", "", "zz", "d4 zz"]
    while len(distinct) < 40:
        q = " ".join(vocab[int(x)] for x in r.integers(0, 12, int(r.integers(1, 4))))
        if q not in distinct:
            distinct.append(q)
    xdistinct = ["", "d4", "d1 d7", "zz", "d0"]
    qi = (np.arange(nq) * 17 + np.cumsum(r.integers(0, 3, nq))) % 40      # steps of 17, 18 or 19: neighbours differ
    xi = r.integers(0, 5, nq)
    qi[-4:] = [3, 0, 1, 2]                                               # rows 65 534 .. 65 536, behind an empty query
    xi[-3:] = [1, 0, 2]
    if qi[-5] == 3:
        qi[-5] = 4
    assert (qi[1:] != qi[:-1]).all()
    queries, exclude = [distinct[int(i)] for i in qi], [xdistinct[int(i)] for i in xi]
    m = model(cls, docs)
    post = R.Postings(m.frequency_word_in_doc)
    S = restate(m, distinct, post)
    got = m.get_scores(queries)
    assert got.shape == (nq, n) and np.array_equal(bits(got), bits(S)[qi])
    ids, sc = m.top_k(queries, 3)
    want = topk_oracle(S, 3)
    assert ids.shape == (nq, 3) and np.array_equal(ids, want[0][qi]) and np.array_equal(bits(sc), want[1][qi])
    # the oracle once per distinct (query, exclusion) pair
    pq, px = [distinct[p // 5] for p in range(200)], [xdistinct[p % 5] for p in range(200)]
    S5, rows = np.repeat(S, 5, axis=0), 5 * qi + xi
    results = {}
    for mode in MODES:
        mt = matched(post, pq, mode, px)
        results[mode] = m.search(queries, 3, match=mode, exclude=exclude)
        check_rows(results[mode], gather(oracle(S5, mt, 3), rows), (cls, mode))
        assert np.array_equal(m.count_matches(queries, match=mode, exclude=exclude), mt.sum(axis=1)[rows]), (cls, mode)
    mt = matched(post, distinct, "any")
    check_rows(m.search(queries, 3), gather(oracle(S, mt, 3), qi), (cls, "plain"))
    assert np.array_equal(m.count_matches(queries), mt.sum(axis=1)[qi]), (cls, "plain")
    # the last row of the first chunk and both rows of the second, each against an oracle of its own
    for q in (65_534, 65_535, 65_536):
        one = restate(m, [queries[q]], post)
        assert np.array_equal(bits(got[q]), bits(one[0])) and one.any(), q
        topk_check((ids[q:q + 1], sc[q:q + 1]), one, 3, q)
        for mode in MODES:
            mt = matched(post, [queries[q]], mode, [exclude[q]])
            assert mt.any(), (q, mode)
            check(tuple(x[q:q + 1] for x in results[mode]), one, mt, 3, (cls, mode, q))
