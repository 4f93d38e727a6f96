"""GPU: BM25 search over the matching documents (BM25.search / count_matches, gz_bm25_search[_device], gz_bm25_match_count,
csrc/gz_search.inc).  The oracle: S = get_scores(queries), pinned elsewhere; matched[q, d] from frequency_word_in_doc (through
bm25_restate.Postings); row q = [i for i in np.argsort(-S[q], kind="stable") if matched[q, i]][:k'], -1 / the NaN 0x7FF8000000000000
behind it.  ids are compared with ==, scores as uint64 bit patterns, counts with ==."""
import warnings

import numpy as np
import pytest

import bm25_restate as R
from conftest import read_jsonl
from genz_tokenize import _native
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

CASES = read_jsonl("g8_bm25.jsonl.gz")
PAD = np.uint64(0x7FF8000000000000)


def val(x):
    return int(x["v"]) if x["t"] == "int" else float.fromhex(x["v"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model(cls, docs, b=0.75, k1=1.2, delta=1.0, ctx=None):
    return BM25Plus(docs, b, k1, delta, ctx=ctx) if cls == "BM25Plus" else BM25(docs, b, k1, ctx=ctx)


def matched(post, queries):
    m = np.zeros((len(queries), post.n), dtype=bool)
    for q, text in enumerate(queries):
        for w in set(text.split()):
            if w in post.p:
                m[q, post.p[w][0]] = True
    return m


def oracle(S, m, k):
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


def check(got, S, m, k, what=""):
    ids, sc, cnt = got
    want_ids, want_sc, want_cnt = oracle(S, m, k)
    assert ids.dtype == np.int64 and sc.dtype == np.float64 and cnt.dtype == np.int64, what
    assert ids.shape == want_ids.shape and sc.shape == want_sc.shape and cnt.shape == want_cnt.shape, (what, ids.shape, want_ids.shape)
    assert np.array_equal(cnt, want_cnt), what
    assert np.array_equal(ids, want_ids), what
    assert np.array_equal(bits(sc), want_sc), what


def check_model(m, queries, ks, what=""):
    S = m.get_scores(queries)
    mt = matched(R.Postings(m.frequency_word_in_doc), queries)
    for k in ks:
        check(m.search(queries, k), S, mt, k, (what, k))
    assert np.array_equal(m.count_matches(queries), mt.sum(axis=1)), what
    return S, mt


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


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


# ---- 1: every fixture case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_case(i):
    c = CASES[i]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (np.mean of no fieldLens)
        m = model(c["cls"], c["documents"], val(c["b"]), val(c["k1"]), val(c["delta"]))
    n = c["num_doc"]
    check_model(m, c["queries"], sorted({1, 3, max(n, 1), n + 5}), i)


# ---- 2: the bitmap's edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_bitmap_edges(n):
    where = {"all": range(n), "one": [n - 1], "two": [0, n - 1], "three": [0, n // 2, n - 1], "four": [0, 1, n - 2, n - 1]}
    docs = []
    for i in range(n):
        words = [w for w, at in where.items() if i in [x % n for x in at]] + ["f"] * (i % 5)
        docs.append(" ".join(words))
    queries = ["zz", "one", "two", "three", "four", "all", "one one", "zz one yy", "", "   ", "zz yy", "two three", "f"]
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.5)
        S, mt = check_model(m, queries, sorted({1, 2, 3, 4, n, n + 2}), (cls, n))
        cnt = mt.sum(axis=1)
        assert cnt[0] == 0 and cnt[1] == 1 and cnt[5] == n and cnt[6] == 1 and cnt[7] == 1 and not cnt[8:11].any()
        ids, sc, got = m.search(queries, 3)
        for q in range(len(queries)):
            c = min(int(got[q]), ids.shape[1])
            assert (ids[q, :c] >= 0).all() and (ids[q, c:] == -1).all() and (bits(sc[q, c:]) == PAD).all()


# ---- 3: BM25Plus: search differs from top_k exactly in the tail -----------------------------------------------------------------
def test_bm25plus_tail_differs_from_topk():
    docs = ["the cat sat", "a dog", "cat cat cat", "", "the dog and the cat", "birds", "a bird and a cat"] * 3
    m = BM25Plus(docs, delta=1.0)
    queries = ["cat", "birds", "dog zebra", "zebra", "the a"]
    k = 15
    ids, sc, cnt = m.search(queries, k)
    check((ids, sc, cnt), m.get_scores(queries), matched(R.Postings(m.frequency_word_in_doc), queries), k)
    tid, tsc = m.top_k(queries, k)
    assert cnt.tolist() == [12, 3, 6, 0, 12]
    for q in range(len(queries)):
        c = int(cnt[q])
        assert np.array_equal(ids[q, :c], tid[q, :c]) and np.array_equal(bits(sc[q, :c]), bits(tsc[q, :c]))
        assert (ids[q, c:] == -1).all() and (bits(sc[q, c:]) == PAD).all()
        assert (tid[q, c:] >= 0).all() and (tsc[q, c:] > 0).all()       # top_k's fillers: documents without any query word, scored > 0


# ---- 4: ties, and the selection's levels over candidate rows ----------------------------------------------------------------------
def test_ties_and_levels():
    r = np.random.default_rng(3)
    same_doc = "alpha beta gamma"
    docs = []
    for i in range(12_000):
        x = r.random()
        docs.append(same_doc if x < 0.85 else ("alpha beta gamma delta" if x < 0.9 else "zeta %d eta" % (i % 97)))
    docs[5000] = "alpha alpha alpha"
    docs[11_999] = "beta"
    queries = ["alpha", "beta gamma", "delta", "zeta", "alpha delta", "", "nothing here", "eta zeta alpha"]
    want = {}
    mt = None
    for tile in (0, 7, 64, 4096):
        ctx = _native.Context()
        _native.debug_set("bm25_topk_tile", tile, ctx)
        m = BM25(docs, ctx=ctx)
        S = m.get_scores(queries)
        if mt is None:
            mt = matched(R.Postings(m.frequency_word_in_doc), queries)
        for k in (1, 100, 1024):
            got = m.search(queries, k)
            check(got, S, mt, k, (tile, k))
            if k not in want:
                want[k] = got
            else:
                assert same(got, want[k]), (tile, k)
        ids, sc, cnt = m.search(["alpha"], 1024)
        assert cnt[0] > 10_000
        tied = np.flatnonzero(S[0] == sc[0, -1])
        assert len(tied) > 1000
        assert np.array_equal(ids[0][sc[0] == sc[0, -1]], tied[:int((sc[0] == sc[0, -1]).sum())])
        del m
        ctx.close()


# ---- 5: a real NaN candidate beats the padding ----------------------------------------------------------------------------------
def test_nan_candidates_before_padding():
    docs = ["w w", "w", "x", "w w y", "", "y y", "w x w"] * 40
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = BM25(docs, k1=float("nan"))
        queries = ["x", "y", "w", "x y", "q", ""]
        S = m.get_scores(queries)
        assert np.isnan(S[:4]).all()
        mt = matched(R.Postings(m.frequency_word_in_doc), queries)
        for k in (1, 50, 100, len(docs)):
            check(m.search(queries, k), S, mt, k, k)
        ids, sc, cnt = m.search(["x"], 100)
        assert cnt[0] == 80 and ids[0, :80].tolist() == np.flatnonzero(mt[0]).tolist() and (ids[0, 80:] == -1).all()
        assert np.isnan(sc[0]).all() and (bits(sc[0, 80:]) == PAD).all() and np.array_equal(bits(sc[0, :80]), bits(S[0, ids[0, :80]]))
        m2 = BM25(docs, b=0.0, k1=-2.0)
        qs = ["w", "w y", "x w", "y"]
        S2 = m2.get_scores(qs)
        assert np.isneginf(S2).any()
        mt2 = matched(R.Postings(m2.frequency_word_in_doc), qs)
        for k in (1, 5, 50, len(docs)):
            check(m2.search(qs, k), S2, mt2, k, k)


# ---- 6: chunks -------------------------------------------------------------------------------------------------------------------
def test_chunking(corpus2):
    docs, queries = corpus2
    docs = docs[:30_000]
    queries = queries[:30] + ["", "absentx absenty", "   "] + queries[30:61]
    assert len(queries) == 64
    base = BM25(docs)
    want = base.search(queries, 50)
    check(want, base.get_scores(queries), matched(R.Postings(base.frequency_word_in_doc), queries), 50, "default")
    M = int(want[2].max())
    assert M > 1000 and (want[2] == 0).sum() >= 4
    for chunk in (1, M, M + 1, 5 * M + 3):
        ctx = _native.Context()
        _native.debug_set("bm25_search_chunk", chunk, ctx)
        m = BM25(docs, ctx=ctx)
        assert same(m.search(queries, 50), want), chunk
        assert np.array_equal(m.count_matches(queries), want[2]), chunk
        del m
        ctx.close()


# ---- 7: the postings follow the index -----------------------------------------------------------------------------------------
def test_mutation():
    r = np.random.default_rng(11)
    vocab = ["w%d" % i for i in range(60)]
    docs = [" ".join(vocab[int(x)] for x in r.integers(0, 60, int(r.integers(0, 9)))) for _ in range(700)]
    docs[10] = "solo w1"
    docs[400] = "solo solo"
    more = [" ".join(vocab[int(x)] for x in r.integers(0, 60, 5)) for _ in range(130)] + ["fresh w2", "solo again"]
    queries = ["w1", "w2 w3", "solo", "fresh", "w59 w0 w1 absent", "", "again solo"]
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.7)
        cur = list(docs)

        def agree(what):
            f = model(cls, cur, delta=0.7)
            for k in (1, 8, 200):
                assert same(m.search(queries, k), f.search(queries, k)), (cls, what, k)
            assert np.array_equal(m.count_matches(queries), f.count_matches(queries)), (cls, what)
            check_model(m, queries, (8,), (cls, what))
            return f

        before = m.footprint()["device_bytes"]
        m.search(queries, 5)
        assert m.footprint()["device_bytes"] > before                   # the postings exist now
        m.add_documents(more)
        cur += more
        agree("add")
        gone = sorted({int(x) for x in r.integers(0, len(cur), 90)} | {10, 400, len(cur) - 1})     # every document of "solo"
        m.remove_documents(gone)
        cur = [d for i, d in enumerate(cur) if i not in set(gone)]
        agree("remove")
        assert m.count_matches(["solo", "again solo"]).tolist() == [0, 0]
        assert (m.search(["solo"], 3)[0] == -1).all()
        m.search(queries, 5)
        m.compact()
        f = agree("compact")
        m.compact()                                                      # (the searches of agree() built the postings again)
        # a fresh build that never searched: the compacted index holds no more than it, and exactly what it holds once it is
        # compacted too (a build keeps the whole text, a compaction the terms' bytes: every buffer is sized by the counts alone)
        fresh = model(cls, cur, delta=0.7)
        assert m.footprint()["device_bytes"] <= fresh.footprint()["device_bytes"]
        fresh.compact()
        assert m.footprint() == fresh.footprint()
        m.search(queries, 5)
        m.remove_documents([0, 5, 6])
        cur = [d for i, d in enumerate(cur) if i not in (0, 5, 6)]
        m.search(queries, 5)
        m.add_documents(["solo returns w1", "w3"])
        cur += ["solo returns w1", "w3"]
        agree("remove, add")
        assert m.count_matches(["solo"]).tolist() == [1]
        del f, fresh


# ---- 8: forced hash collisions ----------------------------------------------------------------------------------------------------
def test_forced_hash_collisions():
    r = np.random.default_rng(5)
    vocab = ["t%d" % i for i in range(200)]
    docs = [" ".join(vocab[int(x)] for x in r.integers(0, 200, int(r.integers(1, 12)))) for _ in range(300)]
    queries = ["t1 t2", "t199", "t5 t5 nope", "nope", "t7 t8 t9 t10 t11"]
    want = BM25(docs).search(queries, 20)
    ctx = _native.Context()
    _native.debug_set("bm25_hash_bits", 4, ctx)
    m = BM25(docs, ctx=ctx)
    got = m.search(queries, 20)
    assert same(got, want)
    check_model(m, queries, (20,), "hash bits 4")
    del m
    ctx.close()


# ---- 9: scale ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus2_matches(corpus2):
    docs, queries = corpus2
    post = R.Postings(R.stats(docs)[1])
    return post, matched(post, queries)


@pytest.mark.parametrize("cls,b,k1,delta", [("BM25", 0.75, 1.2, None), ("BM25Plus", 0.3, 2.0, 0.5)])
def test_corpus2_100k_x_64(corpus2, corpus2_matches, cls, b, k1, delta):
    docs, queries = corpus2
    post, mt = corpus2_matches
    m = model(cls, docs, b, k1, 1.0 if delta is None else delta)
    S = m.get_scores(queries)
    for k in (1, 10, 1024):
        check(m.search(queries, k), S, mt, k, (cls, k))
    assert np.array_equal(m.count_matches(queries), mt.sum(axis=1))
    words, df = m.vocabulary()
    pick = list(range(0, len(words), max(1, len(words) // 500)))
    one = m.count_matches([words[i] for i in pick])
    assert np.array_equal(one, df[pick].astype(np.int64))
    assert all(int(one[j]) == post.df(words[i]) for j, i in enumerate(pick))


# ---- 10: the device entry point -----------------------------------------------------------------------------------------------------
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
    mt = matched(R.Postings(m.frequency_word_in_doc), queries)
    nq, terms, idf, qoff = m._queries(queries)
    P = m._params()
    g = 256
    for plus in (False, True):
        S = ctx.bm25_score(ih, terms, idf, qoff, P, plus)
        for k in (1, 10, 300):
            host = ctx.bm25_search(ih, terms, idf, qoff, P, plus, k)
            check(host, S, mt, k, (plus, k))
            assert same(ctx.bm25_search(idv, terms, idf, qoff, P, plus, k), host), ("device build", plus, k)
            sizes = (nq * k * 8, nq * k * 8, nq * 8)
            dev = [ctx.alloc(nb + 2 * g) for nb in sizes]
            for d, nb in zip(dev, sizes):
                ctx.h2d(d, np.full(nb + 2 * g, 0xA5, np.uint8))
            ctx.bm25_search(ih, terms, idf, qoff, P, plus, k, d_ids=dev[0] + g, d_scores=dev[1] + g, d_counts=dev[2] + g)
            ctx.sync()
            raw = []
            for d, nb in zip(dev, sizes):
                x = np.empty(nb + 2 * g, np.uint8)
                ctx.d2h(x, d)
                ctx.free(d)
                assert np.all(x[:g] == 0xA5) and np.all(x[g + nb:] == 0xA5)
                raw.append(x[g:g + nb])
            assert np.array_equal(raw[0].view(np.int64).reshape(nq, k), host[0])
            assert np.array_equal(raw[1].view(np.uint64).reshape(nq, k), bits(host[1]))
            assert np.array_equal(raw[2].view(np.int64), host[2])
    assert np.array_equal(ctx.bm25_match_count(idv, terms, qoff), mt.sum(axis=1))
    del m
    ctx.bm25_destroy(idv)
    ctx.bm25_destroy(ih)
    ctx.close()


# ---- 11: allocation failures ---------------------------------------------------------------------------------------------------------
def test_allocation_failure_sweep(corpus2):
    docs, queries = corpus2
    docs = docs[:5000]
    fresh = _native.Context()                     # (no postings, no search workspace yet)
    _native.debug_set("bm25_search_chunk", 3 * len(docs), fresh)
    m = BM25(docs, ctx=fresh)
    S = m.get_scores(queries)
    mt = matched(R.Postings(m.frequency_word_in_doc), queries)
    topk = m.top_k(queries, 40)
    nq, terms, idf, qoff = m._queries(queries)
    P = m._params()
    ok, failed = None, 0
    for k in range(1, 1000):
        _native.debug_set("inject_bad_alloc", k, fresh)
        try:
            got = fresh.bm25_search(m._index, terms, idf, qoff, P, False, 40)
        except _native.GzError as e:
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            failed += 1
            _native.debug_set("inject_bad_alloc", 0, fresh)
            again = m.top_k(queries, 40)                                 # context and index stay usable
            assert np.array_equal(again[0], topk[0]) and np.array_equal(bits(again[1]), bits(topk[1])), k
            continue
        ok = k
        break
    _native.debug_set("inject_bad_alloc", 0, fresh)
    assert ok is not None and failed > 10                                # the postings build and the search workspace
    check(got, S, mt, 40)
    check(m.search(queries, 40), S, mt, 40)
    for k in range(1, 40):                                               # the match count alone, postings in place
        _native.debug_set("inject_bad_alloc", k, fresh)
        try:
            cnt = fresh.bm25_match_count(m._index, terms, qoff)
        except _native.GzError as e:
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            continue
        break
    _native.debug_set("inject_bad_alloc", 0, fresh)
    assert np.array_equal(cnt, mt.sum(axis=1))
    del m
    fresh.close()


# ---- 12: the tokenizer is unaffected --------------------------------------------------------------------------------------------------
def test_encode_packed_unchanged_around_search(corpus2):
    from genz_tokenize import Tokenize
    import corpus
    tok = Tokenize()
    t, o, _ = corpus.config_corpus(2, n_docs=5000)
    before = tok.encode_packed(t, o, max_len=64)
    docs, queries = corpus2
    a = BM25(docs[:30_000])
    bb = BM25Plus(docs[30_000:60_000], 0.3, 2.0, 0.5)
    ta = a.search(queries, 100)
    during = tok.encode_packed(t, o, max_len=64)
    tb = bb.search(queries, 1024)
    during2 = tok.encode_packed(t, o, max_len=64)
    assert same(a.search(queries, 100), ta) and same(bb.search(queries, 1024), tb)
    del a, bb
    after = tok.encode_packed(t, o, max_len=64)
    for r in (during, during2, after):
        for k in ("input_ids", "attention_mask"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(before[k]))


# ---- arguments and empty shapes ------------------------------------------------------------------------------------------------------
def test_arguments_and_empty_shapes():
    import ctypes
    m = BM25(["a b", "b c", "c d", "a a", ""])
    assert [x.shape for x in m.search([], 3)] == [(0, 3), (0, 3), (0,)]
    assert [x.shape for x in m.search([], 10**9)] == [(0, 5), (0, 5), (0,)]
    assert m.count_matches([]).shape == (0,)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        e = BM25([])
    ids, sc, cnt = e.search(["a", ""], 4)
    assert ids.shape == (2, 0) and sc.shape == (2, 0) and cnt.tolist() == [0, 0]
    assert e.count_matches(["a", ""]).tolist() == [0, 0]
    docs = ["d%d x" % i for i in range(1500)]
    big = BM25(docs)
    check_model(big, ["x d7", "d1499"], (1024,))
    with pytest.raises(_native.GzError) as err:
        big.search(["x"], 1025)
    assert err.value.code == _native.GZ_E_LIMIT
    assert big.top_k(["d3"], 2)[0][0, 0] == 3                           # the index answers as before
    qoff = np.zeros(2, np.int64)
    P = np.array(big._params())
    ids, sc, cnt = np.zeros((1, 4), np.int64), np.zeros((1, 4)), np.zeros(1, np.int64)
    for k, code in ((0, _native.GZ_E_INVALID), (-3, _native.GZ_E_INVALID), (1025, _native.GZ_E_LIMIT)):
        rc = big._ctx.lib.gz_bm25_search(ctypes.c_void_p(big._index), None, None, ctypes.c_void_p(qoff.ctypes.data), 1,
                                         ctypes.c_void_p(P.ctypes.data), 0, k, ctypes.c_void_p(ids.ctypes.data),
                                         ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(cnt.ctypes.data))
        assert rc == code, k
