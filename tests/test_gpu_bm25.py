"""GPU: genz_tokenize.ranking (BM25 / BM25Plus, csrc/gz_bm25.inc) against the reference's fixtures and the numpy restatement in
tests/bm25_restate.py.  Scores are compared as bit patterns (nan and -0.0 count); idf comes from the reference's scalar expression
evaluated in this process, as the module computes it."""
import ctypes

import numpy as np
import pytest

import bm25_restate as R
from conftest import read_jsonl
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

CASES = read_jsonl("g8_bm25.jsonl.gz")


def val(x):
    return int(x["v"]) if x["t"] == "int" else float.fromhex(x["v"])


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def model(cls, docs, b, k1, delta=1.0, ctx=None):
    return BM25Plus(docs, b, k1, delta, ctx=ctx) if cls == "BM25Plus" else BM25(docs, b, k1, ctx=ctx)


def restated(docs, queries, b, k1, delta=None):
    """[Q, N] scores of the restatement with idf evaluated here (empty queries: 0.0 rows)."""
    lens, freq = R.stats(docs)
    avg = R.avg_field_len(lens)
    post = R.Postings(freq)
    out = np.zeros((len(queries), len(docs)), dtype=np.float64)
    for i, q in enumerate(queries):
        w = q.split()
        if w and docs:
            out[i] = R.scores(lens, post, avg, w, [R.idf(len(docs), post.df(x)) for x in w], b, k1, delta)
    return out


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
            words += words[:2]                                            # repeats
        queries.append(" ".join(words))
    queries[7] = ""
    return docs, queries


# ---- 1: every fixture case through the Python face ------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_case(i):
    c = CASES[i]
    b, k1 = val(c["b"]), val(c["k1"])
    delta = val(c["delta"])
    m = model(c["cls"], c["documents"], b, k1, delta)
    assert m.num_doc == c["num_doc"] and m.fieldLens == c["fieldLens"] and type(m.fieldLens) is list
    want_avg = float.fromhex(c["avgFieldLen"])
    assert (np.isnan(m.avgFieldLen) and np.isnan(want_avg)) or bits([m.avgFieldLen]) == bits([want_avg])
    assert [[[w, n] for w, n in f.items()] for f in m.frequency_word_in_doc] == c["frequency_word_in_doc"]
    assert m.documents == [d.split() for d in c["documents"]]
    assert (m.b, m.k1) == (b, k1) and (c["cls"] != "BM25Plus" or m.delta == delta)
    lens, freq = R.stats(c["documents"])
    avg = R.avg_field_len(lens)
    for q, r in zip(c["queries"], c["results"]):
        idf_here = [R.idf(c["num_doc"], d) for d in r["df"]]
        got_idf = [m.cal_idf(w) for w in r["words"]]
        assert all(type(v) is np.float64 for v in got_idf) and same_bits(got_idf, idf_here)
        got = m.get_score(q)
        if not c["num_doc"]:
            assert got == []
            continue
        if not r["words"]:
            assert got == [0] * c["num_doc"] and all(type(s) is int for s in got)
            continue
        assert type(got) is list and all(type(s) is np.float64 for s in got)
        want = R.scores(lens, freq, avg, r["words"], idf_here, b, k1, delta if c["cls"] == "BM25Plus" else None)
        assert same_bits(got, want), (i, q)
        if [float(v).hex() for v in idf_here] == r["idf"]:                  # this host's np.log agrees with the recording: the fixture too
            rec = np.array([float.fromhex(s) for s in r["scores"]])
            nan = np.isnan(rec)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(rec)[~nan])


def test_type_errors():
    with pytest.raises(TypeError):
        BM25(["a b", 3])
    m = BM25(["a b"])
    for bad in (None, b"a", 1):
        with pytest.raises(TypeError):
            m.get_score(bad)
        with pytest.raises(TypeError):
            m.cal_idf(bad)


# ---- 2: 100 000 configs[2] documents x 64 queries ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls,b,k1,delta", [("BM25", 0.75, 1.2, None), ("BM25Plus", 0.3, 2.0, 0.5)])
def test_corpus2_100k_x_64(corpus2, cls, b, k1, delta):
    docs, queries = corpus2
    m = model(cls, docs, b, k1, 1.0 if delta is None else delta)
    got = m.get_scores(queries)
    assert got.shape == (64, len(docs)) and got.dtype == np.float64
    want = restated(docs, queries, b, k1, delta)
    for q in range(64):
        assert same_bits(got[q], want[q]), q
    assert same_bits(m.get_score(queries[3]), want[3])


# ---- 3: hash bits truncated: forced collisions, the same results ---------------------------------------------------------------
@pytest.mark.parametrize("hash_bits", [1, 9])
def test_truncated_hash_changes_nothing(corpus2, hash_bits):
    from genz_tokenize import _native
    docs, queries = corpus2
    docs = docs[:20_000] if hash_bits == 9 else docs[:300]
    ref = model("BM25", docs, 0.75, 1.2)
    ctx = _native.Context()
    _native.debug_set("bm25_hash_bits", hash_bits, ctx)
    m = model("BM25", docs, 0.75, 1.2, ctx=ctx)
    assert m.fieldLens == ref.fieldLens
    assert ctx.bm25_info(m._index) == ref._ctx.bm25_info(ref._index)
    assert same_bits(m.get_scores(queries), ref.get_scores(queries))
    words = sorted({w for d in docs[:50] for w in d.split()}) + ["absent", "x" * 70]
    from genz_tokenize._packing import pack
    buf, off = pack(words)
    t1, d1 = ctx.bm25_lookup(m._index, buf, off)
    t0, d0 = ref._ctx.bm25_lookup(ref._index, buf, off)
    assert d1.tolist() == d0.tolist() and t1.tolist() == t0.tolist()      # term ids are first-occurrence order, whatever the hash
    assert len(set(t1[t1 >= 0].tolist())) == int((t1 >= 0).sum())          # distinct words stay distinct terms
    del m
    ctx.close()


# ---- 4: long documents, a document of 10^5+ words, a word over 64 KB ------------------------------------------------------------
def test_long_documents_and_words():
    import corpus
    t, o, _ = corpus.config_corpus(4, n_docs=3000)
    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    r = np.random.default_rng(4)
    pool = sorted({w for d in docs[:200] for w in d.split()})
    huge = " ".join(pool[int(k)] for k in r.integers(len(pool), size=120_000))
    longword = "ư" * 40_000                                                # 80 000 bytes
    docs = docs[:1500] + [huge, longword + " a " + longword, "x " + longword] + docs[1500:]
    queries = [" ".join(pool[int(k)] for k in r.integers(len(pool), size=8)) for _ in range(16)] + [longword, longword + " " + pool[0]]
    for cls, b, k1, delta in (("BM25", 0.75, 1.2, None), ("BM25Plus", 0.3, 2.0, 0.5)):
        m = model(cls, docs, b, k1, 1.0 if delta is None else delta)
        assert m.fieldLens[1500] == 120_000 and m.fieldLens[1501] == 3
        got = m.get_scores(queries)
        want = restated(docs, queries, b, k1, delta)
        for q in range(len(queries)):
            assert same_bits(got[q], want[q]), (cls, q)


# ---- 5: degenerate inputs -------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    import warnings
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        e = BM25([])
        assert np.isnan(e.avgFieldLen) and any(issubclass(x.category, RuntimeWarning) for x in w)
    assert e.get_score("a") == [] and e.fieldLens == [] and e.get_scores(["a", ""]).shape == (2, 0)
    docs = ["a b a", "", "c", "a a a a a a", "b"]
    cases = [(["", " ", "\n"], 0.75, 1.2, None), (["", ""], 0.75, 1.2, 1.0), (docs, 0.75, 0, None), (docs, 0.75, 0, -0.0),
             (docs, 1.5, 1.2, None), (docs, 1.5, -1.0, 0.5), (docs, 2.0, 3.0, -0.0), (docs, 0, 0, None), (docs, 1, 2, 1)]
    queries = ["a", "a b c", "zz a", "b b", "c"]
    for d, b, k1, delta in cases:
        m = BM25(d, b, k1) if delta is None else BM25Plus(d, b, k1, delta)
        got = m.get_scores(queries)
        want = restated(d, queries, b, k1, delta)
        assert same_bits(got, want), (d, b, k1, delta, got, want)
        assert same_bits(m.get_score("a"), want[0])


# ---- 6: allocation failures ----------------------------------------------------------------------------------------------------
def test_allocation_failure_sweep():
    from genz_tokenize import _native
    from genz_tokenize._packing import pack
    import corpus
    t, o, _ = corpus.config_corpus(2, n_docs=500)
    ctx = _native.Context()
    ok = None
    for k in range(1, 200):
        _native.debug_set("inject_bad_alloc", k, ctx)
        try:
            ix = ctx.bm25_build(t, o)
        except _native.GzError as e:
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            ctx.preprocess([_native.GZ_PP_PUNCT], np.frombuffer(b"a,b", np.uint8), np.array([0, 3], np.int64))   # still usable
            continue
        ok = k
        break
    _native.debug_set("inject_bad_alloc", 0, ctx)
    assert ok is not None and ok > 5
    want = ctx.bm25_field_lengths(ix)
    ix2 = ctx.bm25_build(t, o)
    assert ctx.bm25_field_lengths(ix2).tolist() == want.tolist()
    ctx.bm25_destroy(ix)
    ctx.bm25_destroy(ix2)
    ctx.close()


# ---- 7: two live indexes leave the tokenizer's results alone --------------------------------------------------------------------
def test_encode_packed_unchanged_around_live_indexes(corpus2):
    from genz_tokenize import Tokenize
    import corpus
    tok = Tokenize()
    t, o, _ = corpus.config_corpus(2, n_docs=5000)
    before = tok.encode_packed(t, o, max_len=64)
    docs, queries = corpus2
    a = model("BM25", docs[:30_000], 0.75, 1.2)
    during = tok.encode_packed(t, o, max_len=64)
    bb = model("BM25Plus", docs[30_000:60_000], 0.3, 2.0, 0.5)
    sa, sb = a.get_scores(queries[:8]), bb.get_scores(queries[:8])
    during2 = tok.encode_packed(t, o, max_len=64)
    assert same_bits(a.get_scores(queries[:8]), sa) and same_bits(bb.get_scores(queries[:8]), sb)
    del a, bb
    after = tok.encode_packed(t, o, max_len=64)
    for r in (during, during2, after):
        for k in ("input_ids", "attention_mask"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(before[k]))


def test_device_build_and_device_scores():
    """gz_bm25_build_device over text already in HBM (offsets absolute from a base that is not the buffer's start) and
    gz_bm25_score_device into HBM: the same bits as the host entry points."""
    from genz_tokenize import _native
    from genz_tokenize._packing import pack
    docs = ["a b c", "", "b b", "tiếng việt", "c a"] * 50
    queries = ["a", "b c", "việt x", ""]
    ctx = _native.Context()
    buf, off = pack(docs)
    pad = 7
    dt = ctx.alloc(len(buf) + pad)
    do = ctx.alloc(8 * len(off))
    ctx.h2d(dt, np.concatenate([np.full(pad, 32, np.uint8), buf]))
    ctx.h2d(do, off + pad)
    ix = ctx.bm25_build_device(dt, do, len(docs), int(off[-1]))
    ctx.free(dt)
    ctx.free(do)
    ih = ctx.bm25_build(buf, off)
    assert ctx.bm25_info(ix) == ctx.bm25_info(ih)
    assert ctx.bm25_field_lengths(ix).tolist() == ctx.bm25_field_lengths(ih).tolist()
    words = [w for q in queries for w in q.split()]
    qoff = np.array([0] + list(np.cumsum([len(q.split()) for q in queries])), np.int64)
    wb, wo = pack(words)
    terms, df = ctx.bm25_lookup(ix, wb, wo)
    idf = np.array([R.idf(len(docs), int(d)) for d in df])
    params = [2.2, 1.2, 0.25, 0.75, float(np.mean(ctx.bm25_field_lengths(ix))), 0.0]
    host = ctx.bm25_score(ih, terms, idf, qoff, params, False)
    dout = ctx.alloc(host.nbytes)
    ctx.bm25_score(ix, terms, idf, qoff, params, False, d_out=dout)
    ctx.sync()
    dev = np.empty_like(host)
    ctx.d2h(dev, dout)
    ctx.free(dout)
    assert same_bits(dev, host)
    bad, boff = ctypes.c_void_p(), np.array([5, 3], np.int64)
    assert ctx.lib.gz_bm25_build(ctx.handle, None, ctypes.c_void_p(boff.ctypes.data), 1, ctypes.byref(bad)) == _native.GZ_E_INVALID
    ctx.bm25_destroy(ix)
    ctx.bm25_destroy(ih)
    ctx.close()
