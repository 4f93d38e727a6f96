"""GPU: BM25 top-k retrieval (BM25.top_k / get_top_n, gz_bm25_topk[_device], csrc/gz_topk.inc).  The oracle is
np.argsort(-S, axis=1, kind="stable") over score rows whose own correctness is pinned elsewhere (the reference's recorded scores,
get_scores); ids are compared with ==, scores as uint64 bit patterns."""
import ctypes
import warnings

import numpy as np
import pytest

import bm25_restate as R
from conftest import read_jsonl
from genz_tokenize import _native
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

CASES = read_jsonl("g8_bm25.jsonl.gz")


def val(x):
    return int(x["v"]) if x["t"] == "int" else float.fromhex(x["v"])


def rec(s):
    return 0.0 if s.startswith("int:") else float.fromhex(s)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle(S, k):
    S = np.asarray(S, dtype=np.float64)
    kk = min(k, S.shape[1])
    ids = np.argsort(-S, axis=1, kind="stable")[:, :kk].astype(np.int64)
    return ids, np.take_along_axis(S, ids, 1)


def check(got, S, k, what=""):
    ids, sc = got
    want_ids, want_sc = oracle(S, k)
    assert ids.dtype == np.int64 and sc.dtype == np.float64, what
    assert ids.shape == want_ids.shape and sc.shape == want_sc.shape, (what, ids.shape, want_ids.shape)
    assert np.array_equal(ids, want_ids), what
    assert np.array_equal(bits(sc), bits(want_sc)), what


def model(cls, docs, b=0.75, k1=1.2, delta=1.0, ctx=None):
    return BM25Plus(docs, b, k1, delta, ctx=ctx) if cls == "BM25Plus" else BM25(docs, b, k1, ctx=ctx)


def with_switch(ctx, key, value):
    _native.debug_set(key, value, ctx)


@pytest.fixture(scope="module")
def corpus2():
    import corpus
    t, o, _ = corpus.config_corpus(2, n_docs=100_000)
    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    r = np.random.default_rng(8)
    vocab = sorted({w for d in docs[:2000] for w in d.split()})
    queries = []
    for k in range(64):
        words = [vocab[int(r.integers(len(vocab)))] if r.random() < 0.8 else "absent%d" % k for _ in range(int(r.integers(1, 9)))]
        if k % 5 == 0:
            words += words[:2]
        queries.append(" ".join(words))
    queries[7] = ""
    return docs, queries


# ---- 1: every fixture case, the reference's recorded scores as the oracle ----------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_case(i):
    c = CASES[i]
    m = model(c["cls"], c["documents"], val(c["b"]), val(c["k1"]), val(c["delta"]))
    n = c["num_doc"]
    queries = c["queries"]
    recorded = np.array([[rec(s) for s in r["scores"]] for r in c["results"]], dtype=np.float64).reshape(len(queries), n)
    here = m.get_scores(queries)
    assert np.array_equal(np.isnan(here), np.isnan(recorded))
    same_log = all([float(R.idf(n, d)).hex() for d in r["df"]] == r["idf"] for r in c["results"])
    for k in sorted({1, 3, max(n, 1), n + 5}):
        ids, sc = m.top_k(queries, k)
        want_ids, _ = oracle(recorded if same_log else here, k)
        assert np.array_equal(ids, want_ids), (i, k)
        check((ids, sc), here, k, (i, k))


# ---- 2: 100 000 configs[2] documents x 64 queries -------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,b,k1,delta", [("BM25", 0.75, 1.2, None), ("BM25Plus", 0.3, 2.0, 0.5)])
def test_corpus2_100k_x_64(corpus2, cls, b, k1, delta):
    docs, queries = corpus2
    m = model(cls, docs, b, k1, 1.0 if delta is None else delta)
    S = m.get_scores(queries)
    for k in (1, 10, 100, 1024):
        check(m.top_k(queries, k), S, k, (cls, k))
    rows = [0, 3, 7, 40]
    lens, freq = R.stats(docs)
    avg = R.avg_field_len(lens)
    post = R.Postings(freq)
    for q in rows:
        w = queries[q].split()
        want = np.zeros(len(docs)) if not w else R.scores(lens, post, avg, w, [R.idf(len(docs), post.df(x)) for x in w], b, k1, delta)
        check(m.top_k([queries[q]], 10), want[None, :], 10, (cls, q))


# ---- 3: ties across tiles: forced small tiles (many tiles, the later levels) and the default ------------------------------------
def test_ties_across_tiles():
    r = np.random.default_rng(3)
    same = "alpha beta gamma"
    docs = []
    for i in range(12_000):
        x = r.random()
        docs.append(same if x < 0.85 else ("alpha beta gamma delta" if x < 0.9 else "zeta %d eta" % (i % 97)))
    docs[5000] = "alpha alpha alpha"
    docs[11_999] = "beta"
    queries = ["alpha", "beta gamma", "delta", "zeta", "alpha delta", "", "nothing here", "eta zeta alpha"]
    want = {}
    for tile in (0, 1, 7, 64, 300, 4096):
        ctx = _native.Context()
        with_switch(ctx, "bm25_topk_tile", tile)
        m = BM25(docs, ctx=ctx)
        S = m.get_scores(queries)
        for k in (1, 5, 100, 1000, 1024):
            got = m.top_k(queries, k)
            check(got, S, k, (tile, k))
            if k not in want:
                want[k] = got
            else:
                assert np.array_equal(got[0], want[k][0]) and np.array_equal(bits(got[1]), bits(want[k][1]))
        # the k-th score is shared by thousands of documents: the lowest indices win
        ids, sc = m.top_k(["alpha"], 1024)
        tied = np.flatnonzero(S[0] == sc[0, -1])
        assert len(tied) > 1000
        assert np.array_equal(ids[0][sc[0] == sc[0, -1]], tied[:int((sc[0] == sc[0, -1]).sum())])
        del m
        ctx.close()


# ---- 4: chunks of queries ------------------------------------------------------------------------------------------------------
def test_chunking(corpus2):
    docs, queries = corpus2
    docs = docs[:30_000]
    base = BM25(docs)
    want = base.top_k(queries, 50)
    check(want, base.get_scores(queries), 50, "default")
    n = len(docs)
    for chunk in (1, n, n + 1, 5 * n + 3, 17 * n):
        ctx = _native.Context()
        with_switch(ctx, "bm25_topk_chunk", chunk)
        with_switch(ctx, "bm25_topk_tile", 512 if chunk == n else 0)
        m = BM25(docs, ctx=ctx)
        got = m.top_k(queries, 50)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), chunk
        del m
        ctx.close()


# ---- 5: special values and edges ------------------------------------------------------------------------------------------------
def test_all_documents_empty_nan_scores():
    m = BM25(["", " ", "\n", ""] * 250)
    S = m.get_scores(["a", "a b"])
    assert np.isnan(S).all()
    for k in (1, 7, 1000, 5000):
        ids, sc = m.top_k(["a", "a b"], k)
        kk = min(k, 1000)
        assert ids.tolist() == [list(range(kk))] * 2
        check((ids, sc), S, k)


def test_minus_inf_ranks_below_numbers_above_nan():
    docs = ["w w", "w", "x", "w w y", "", "y y", "w x w"] * 40
    m = BM25(docs, b=0.0, k1=-2.0)
    qs = ["w", "w y", "x w", "y"]
    S = m.get_scores(qs)
    assert np.isneginf(S).any() and np.isnan(S).sum() >= 0
    for k in (1, 5, 50, len(docs)):
        check(m.top_k(qs, k), S, k, k)
    ids, sc = m.top_k(["w"], len(docs))
    s = sc[0]
    fin, ninf, nan = np.isfinite(s), np.isneginf(s), np.isnan(s)
    last_fin = np.flatnonzero(fin).max() if fin.any() else -1
    assert ninf.any() and (not ninf.any() or np.flatnonzero(ninf).min() > last_fin)
    assert not nan.any() or np.flatnonzero(nan).min() > np.flatnonzero(ninf).max()


def test_edges():
    m = BM25(["a b", "b c", "c d", "a a", ""])
    S = m.get_scores(["a", "", "zz", "a c"])
    for k in (1, 2, 5, 6, 10**9):
        check(m.top_k(["a", "", "zz", "a c"], k), S, k, k)
    ids, sc = m.top_k(["", "   "], 3)
    assert ids.tolist() == [[0, 1, 2]] * 2 and not sc.any()
    assert [x.shape for x in m.top_k([], 3)] == [(0, 3), (0, 3)]
    assert [x.shape for x in m.top_k([], 10**9)] == [(0, 5), (0, 5)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (np.mean of no fieldLens)
        e = BM25([])
    assert [x.shape for x in e.top_k(["a", ""], 4)] == [(2, 0), (2, 0)]
    assert e.get_top_n("a", n=3) == []
    for bad in (0, -1):
        with pytest.raises(ValueError):
            m.top_k(["a"], bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            m.top_k(["a"], bad)
    with pytest.raises(TypeError):
        m.top_k(["a", 3], 2)


def test_k_limits():
    docs = ["d%d x" % i for i in range(1500)]
    m = BM25(docs)
    S = m.get_scores(["x d7", "d1499"])
    check(m.top_k(["x d7", "d1499"], 1024), S, 1024)
    with pytest.raises(_native.GzError) as e:
        m.top_k(["x"], 1025)
    assert e.value.code == _native.GZ_E_LIMIT
    small = BM25(docs[:1000])
    check(small.top_k(["x d7"], 10**9), small.get_scores(["x d7"]), 10**9)
    ctx = m._ctx
    qoff = np.zeros(2, np.int64)
    P = np.array(m._params())
    ids, sc = np.zeros((1, 4), np.int64), np.zeros((1, 4))
    for k, code in ((0, _native.GZ_E_INVALID), (-3, _native.GZ_E_INVALID), (1025, _native.GZ_E_LIMIT)):
        rc = ctx.lib.gz_bm25_topk(ctypes.c_void_p(m._index), None, None, ctypes.c_void_p(qoff.ctypes.data), 1,
                                  ctypes.c_void_p(P.ctypes.data), 0, k, ctypes.c_void_p(ids.ctypes.data), ctypes.c_void_p(sc.ctypes.data))
        assert rc == code, k


# ---- 6: get_top_n ---------------------------------------------------------------------------------------------------------------
def test_get_top_n():
    docs = ["the cat sat", "a dog", "cat cat cat", "", "the dog and the cat", "birds"]
    for m in (BM25(docs), BM25Plus(docs, delta=0.5)):
        ids, _ = m.top_k(["cat dog"], 3)
        assert m.get_top_n("cat dog", n=3) == [docs[i] for i in ids[0]]
        assert m.get_top_n("cat dog") == [docs[i] for i in m.top_k(["cat dog"], 5)[0][0]]
        objs = [object() for _ in docs]
        got = m.get_top_n("cat dog", objs, n=2)
        assert all(any(g is o for o in objs) for g in got) and got == [objs[i] for i in ids[0][:2]]
        assert m.get_top_n("cat", n=100) == [docs[i] for i in m.top_k(["cat"], 100)[0][0]]
        with pytest.raises(ValueError):
            m.get_top_n("cat", docs[:-1])
        for bad in (None, b"cat", 3, ["cat"]):
            with pytest.raises(TypeError):
                m.get_top_n(bad)
    p = BM25Plus(docs, delta=2.0)
    check(p.top_k(["cat", "birds"], 6), p.get_scores(["cat", "birds"]), 6)


# ---- 7: the device entry point ---------------------------------------------------------------------------------------------------
def test_device_entry_point_guards_and_device_build(corpus2):
    from genz_tokenize._packing import pack
    docs, queries = corpus2
    docs = docs[:20_000]
    ctx = _native.Context()
    buf, off = pack(docs)
    ih = ctx.bm25_build(buf, off)
    pad = 5
    dt, do = ctx.alloc(len(buf) + pad), ctx.alloc(8 * len(off))
    ctx.h2d(dt, np.concatenate([np.full(pad, 32, np.uint8), buf]))
    ctx.h2d(do, off + pad)
    idv = ctx.bm25_build_device(dt, do, len(docs), int(off[-1]))
    ctx.free(dt)
    ctx.free(do)
    m = BM25(docs, ctx=ctx)
    nq, terms, idf, qoff = m._queries(queries)
    P = m._params()
    for plus in (False, True):
        for k in (1, 10, 300):
            host = ctx.bm25_topk(ih, terms, idf, qoff, P, plus, k)
            S = ctx.bm25_score(ih, terms, idf, qoff, P, plus)
            check(host, S, k, (plus, k))
            check(ctx.bm25_topk(idv, terms, idf, qoff, P, plus, k), S, k, ("device build", plus, k))
            g = 256
            nb = nq * k * 8
            d_ids, d_sc = ctx.alloc(nb + 2 * g), ctx.alloc(nb + 2 * g)
            for d in (d_ids, d_sc):
                ctx.h2d(d, np.full(nb + 2 * g, 0xA5, np.uint8))
            ctx.bm25_topk(ih, terms, idf, qoff, P, plus, k, d_ids=d_ids + g, d_scores=d_sc + g)
            ctx.sync()
            raw_i, raw_s = np.empty(nb + 2 * g, np.uint8), np.empty(nb + 2 * g, np.uint8)
            ctx.d2h(raw_i, d_ids)
            ctx.d2h(raw_s, d_sc)
            ctx.free(d_ids)
            ctx.free(d_sc)
            for raw in (raw_i, raw_s):
                assert np.all(raw[:g] == 0xA5) and np.all(raw[g + nb:] == 0xA5)
            assert np.array_equal(raw_i[g:g + nb].view(np.int64).reshape(nq, k), host[0])
            assert np.array_equal(raw_s[g:g + nb].view(np.uint64).reshape(nq, k), bits(host[1]))
    del m
    ctx.bm25_destroy(idv)
    ctx.bm25_destroy(ih)
    ctx.close()


# ---- 8: allocation failures --------------------------------------------------------------------------------------------------------
def test_allocation_failure_sweep(corpus2):
    docs, queries = corpus2
    docs = docs[:5000]
    ctx = _native.Context()
    with_switch(ctx, "bm25_topk_chunk", 3 * len(docs))
    m = BM25(docs, ctx=ctx)
    S = m.get_scores(queries)
    nq, terms, idf, qoff = m._queries(queries)
    P = m._params()
    fresh = _native.Context()                     # (a second context: the sweep runs on one that has no top-k workspace yet)
    with_switch(fresh, "bm25_topk_chunk", 3 * len(docs))
    m2 = BM25(docs, ctx=fresh)
    ok = None
    for k in range(1, 200):
        _native.debug_set("inject_bad_alloc", k, fresh)
        try:
            got = fresh.bm25_topk(m2._index, terms, idf, qoff, P, False, 40)
        except _native.GzError as e:
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            fresh.preprocess([_native.GZ_PP_PUNCT], np.frombuffer(b"a,b", np.uint8), np.array([0, 3], np.int64))
            continue
        ok = k
        break
    _native.debug_set("inject_bad_alloc", 0, fresh)
    assert ok is not None and ok > 5
    check(got, S, 40)
    check(m2.top_k(queries, 40), S, 40)
    del m, m2
    ctx.close()
    fresh.close()


# ---- 9: the tokenizer is unaffected ------------------------------------------------------------------------------------------------
def test_encode_packed_unchanged_around_topk(corpus2):
    from genz_tokenize import Tokenize
    import corpus
    tok = Tokenize()
    t, o, _ = corpus.config_corpus(2, n_docs=5000)
    before = tok.encode_packed(t, o, max_len=64)
    docs, queries = corpus2
    a = BM25(docs[:30_000])
    bb = BM25Plus(docs[30_000:60_000], 0.3, 2.0, 0.5)
    ta = a.top_k(queries, 100)
    during = tok.encode_packed(t, o, max_len=64)
    tb = bb.top_k(queries, 1024)
    during2 = tok.encode_packed(t, o, max_len=64)
    for x, y in ((a.top_k(queries, 100), ta), (bb.top_k(queries, 1024), tb)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))
    del a, bb
    after = tok.encode_packed(t, o, max_len=64)
    for r in (during, during2, after):
        for k in ("input_ids", "attention_mask"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(before[k]))
