"""GPU: BM25.add_documents / gz_bm25_append[_device] (csrc/gz_bm25.inc).  An index that was appended to answers exactly like one
built fresh over old + new documents: the oracles are the numpy restatement in tests/bm25_restate.py (idf evaluated in this process)
and this library's own fresh build of the concatenation, whose code path the append does not touch.  Scores are compared as bit
patterns (nan and -0.0 count)."""
import ctypes

import numpy as np
import pytest

import bm25_restate as R
from conftest import read_jsonl
from genz_tokenize import _native
from genz_tokenize._packing import pack
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

CASES = read_jsonl("g8_bm25.jsonl.gz")
PARAMS = [("BM25", 0.75, 1.2, None), ("BM25Plus", 0.3, 2.0, 0.5)]


def val(x):
    return int(x["v"]) if x["t"] == "int" else float.fromhex(x["v"])


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def model(cls, docs, b=0.75, k1=1.2, delta=1.0, ctx=None):
    return BM25Plus(docs, b, k1, delta, ctx=ctx) if cls == "BM25Plus" else BM25(docs, b, k1, ctx=ctx)


class Restated:
    """the restatement's statistics of a corpus, computed once; scores for any parameters"""

    def __init__(self, docs):
        self.n = len(docs)
        self.lens, freq = R.stats(docs)
        self.avg = R.avg_field_len(self.lens)
        self.post = R.Postings(freq)

    def scores(self, queries, b, k1, delta=None):
        out = np.zeros((len(queries), self.n), dtype=np.float64)
        for i, q in enumerate(queries):
            w = q.split()
            if w and self.n:
                out[i] = R.scores(self.lens, self.post, self.avg, w, [R.idf(self.n, self.post.df(x)) for x in w], b, k1, delta)
        return out


def lookup(m, words):
    buf, off = pack(list(words))
    t, d = m._ctx.bm25_lookup(m._index, buf, off)
    return t.tolist(), d.tolist()


def same_topk(a, b):
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])


def assert_equal_models(m, ref, queries, words, ks=(10,), what=""):
    """everything observable of m equals the fresh model's"""
    assert m.num_doc == ref.num_doc and m.fieldLens == ref.fieldLens and type(m.fieldLens) is list, what
    assert bits([m.avgFieldLen]) == bits([ref.avgFieldLen]), what
    assert m._ctx.bm25_info(m._index) == ref._ctx.bm25_info(ref._index), what
    assert lookup(m, words) == lookup(ref, words), what
    assert same_bits(m.get_scores(queries), ref.get_scores(queries)), what
    for k in ks:
        assert same_topk(m.top_k(queries, k), ref.top_k(queries, k)), (what, k)


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
    # words that only the documents behind 60 000 have rank too
    late = sorted({w for d in docs[60_000:] for w in d.split()} - {w for d in docs[:60_000] for w in d.split()})
    if late:
        queries[11] = " ".join(late[:4])
    return docs, queries


@pytest.fixture(scope="module")
def restated2(corpus2):
    return Restated(corpus2[0])


# ---- 1: every fixture case, built in part and appended to --------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_case(i):
    c = CASES[i]
    b, k1 = val(c["b"]), val(c["k1"])
    delta = val(c["delta"])
    docs = c["documents"]
    N = len(docs)
    lens, freq = R.stats(docs)
    avg = R.avg_field_len(lens)
    for split in sorted({s for s in (0, 1, N // 2, N - 1, N) if 0 <= s <= N}):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                              # (np.mean of no lengths, as the fresh build of [] warns)
            m = model(c["cls"], docs[:split], b, k1, delta)
        m.add_documents(docs[split:])
        assert m.num_doc == c["num_doc"] and m.fieldLens == c["fieldLens"] and type(m.fieldLens) is list, split
        want_avg = float.fromhex(c["avgFieldLen"])
        assert (np.isnan(m.avgFieldLen) and np.isnan(want_avg)) or bits([m.avgFieldLen]) == bits([want_avg]), split
        assert [[[w, n] for w, n in f.items()] for f in m.frequency_word_in_doc] == c["frequency_word_in_doc"], split
        assert m.documents == [d.split() for d in docs], split
        assert (m.b, m.k1) == (b, k1) and (c["cls"] != "BM25Plus" or m.delta == delta)
        for q, r in zip(c["queries"], c["results"]):
            idf_here = [R.idf(c["num_doc"], d) for d in r["df"]]
            got_idf = [m.cal_idf(w) for w in r["words"]]
            assert all(type(v) is np.float64 for v in got_idf) and same_bits(got_idf, idf_here), (split, q)
            got = m.get_score(q)
            if not c["num_doc"]:
                assert got == []
                continue
            if not r["words"]:
                assert got == [0] * c["num_doc"] and all(type(s) is int for s in got)
                continue
            assert type(got) is list and all(type(s) is np.float64 for s in got)
            want = R.scores(lens, freq, avg, r["words"], idf_here, b, k1, delta if c["cls"] == "BM25Plus" else None)
            assert same_bits(got, want), (i, split, q)
            if [float(v).hex() for v in idf_here] == r["idf"]:              # this host's np.log agrees with the recording: the fixture too
                rec = np.array([float.fromhex(s) for s in r["scores"]])
                nan = np.isnan(rec)
                assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(rec)[~nan]), (i, split, q)


def test_lazy_lists_follow_an_append():
    """documents / frequency_word_in_doc that were materialised BEFORE the append cover the new documents after it"""
    m = BM25(["a b a", "c"])
    assert m.documents == [["a", "b", "a"], ["c"]] and m.frequency_word_in_doc == [{"a": 2, "b": 1}, {"c": 1}]
    m.add_documents(["c c d", ""])
    assert m.documents == [["a", "b", "a"], ["c"], ["c", "c", "d"], []]
    assert m.frequency_word_in_doc == [{"a": 2, "b": 1}, {"c": 1}, {"c": 2, "d": 1}, {}]


# ---- 2: 100 000 configs[2] documents: 60 000 built, batches of 30 000, 0, 1 and 9 999 appended -------------------------------
@pytest.mark.parametrize("cls,b,k1,delta", PARAMS)
def test_corpus2_100k_appended(corpus2, restated2, cls, b, k1, delta):
    docs, queries = corpus2
    d = 1.0 if delta is None else delta
    m = model(cls, docs[:60_000], b, k1, d)
    probe = docs[0].split()[0]
    idf_before = m.cal_idf(probe)
    at = 60_000
    for n in (30_000, 0, 1, 9_999):
        m.add_documents(docs[at:at + n])
        at += n
    assert at == 100_000 == m.num_doc
    ref = model(cls, docs, b, k1, d)
    assert probe not in m._idf                                            # (the value computed for 60 000 documents is not served)
    assert same_bits([m.cal_idf(probe)], [ref.cal_idf(probe)]) and type(idf_before) is np.float64
    got = m.get_scores(queries)
    want = restated2.scores(queries, b, k1, delta)
    for q in range(64):
        assert same_bits(got[q], want[q]), q
    sample = docs[:40] + docs[59_990:60_010] + docs[89_995:90_005] + docs[-20:]
    words = sorted({w for x in sample for w in x.split()}) + ["absent", "x" * 70, ""]
    assert_equal_models(m, ref, queries, words, ks=(10, 1000), what=cls)


# ---- 3: hash bits truncated: forced collisions between old terms, new terms and both ---------------------------------------------
@pytest.mark.parametrize("hash_bits", [1, 9])
def test_truncated_hash_changes_nothing(corpus2, hash_bits):
    docs, queries = corpus2
    docs = docs[:20_000] if hash_bits == 9 else docs[:300]
    cut = len(docs) * 2 // 3
    ref = model("BM25", docs)
    words = sorted({w for d in docs[:50] + docs[cut - 10:cut + 40] + docs[-30:] for w in d.split()}) + ["absent", "x" * 70]
    # (a) built and appended under the switch  (b) built under the switch, appended with it off  (c) the other way round: the index
    # keeps the mask of its build
    for at_build, at_append in ((hash_bits, hash_bits), (hash_bits, 0), (0, hash_bits)):
        ctx = _native.Context()
        _native.debug_set("bm25_hash_bits", at_build, ctx)
        m = model("BM25", docs[:cut], ctx=ctx)
        _native.debug_set("bm25_hash_bits", at_append, ctx)
        m.add_documents(docs[cut:cut + 7])
        m.add_documents(docs[cut + 7:])
        assert_equal_models(m, ref, queries, words, what=(at_build, at_append))
        t, _ = lookup(m, words)
        t = np.array(t)
        assert len(set(t[t >= 0].tolist())) == int((t >= 0).sum())          # distinct words stay distinct terms
        del m
        ctx.close()


# ---- 4: many small appends from nothing, then a large one: every buffer grows several times, both tables are re-hashed -----------
def test_many_small_appends(corpus2):
    import warnings
    docs, queries = corpus2
    docs = docs[:20_300]
    rs = Restated(docs)
    for cls, b, k1, delta in PARAMS:
        d = 1.0 if delta is None else delta
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = model(cls, [], b, k1, d)
        assert np.isnan(m.avgFieldLen)
        for i in range(300):
            m.add_documents(docs[i:i + 1])
            if i in (0, 1, 17, 150):
                r = model(cls, docs[:i + 1], b, k1, d)
                words = sorted({w for x in docs[:i + 1] for w in x.split()})[:200] + ["absent"]
                assert_equal_models(m, r, queries[:8], words, what=(cls, i))
        m.add_documents(docs[300:])
        ref = model(cls, docs, b, k1, d)
        words = sorted({w for x in docs[:320] + docs[-50:] for w in x.split()}) + ["absent", "x" * 70]
        assert_equal_models(m, ref, queries, words, ks=(10, 1000), what=cls)
        assert same_bits(m.get_scores(queries), rs.scores(queries, b, k1, delta))


# ---- 5: a document of 120 000 words and 80 000-byte words, on either side of the append ------------------------------------------
def test_long_documents_and_words():
    import corpus
    t, o, _ = corpus.config_corpus(4, n_docs=3000)
    raw = t.tobytes()
    short = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    r = np.random.default_rng(4)
    pool = sorted({w for d in short[:200] for w in d.split()})
    huge = " ".join(pool[int(k)] for k in r.integers(len(pool), size=120_000))
    longword = "ư" * 40_000                                                # 80 000 bytes
    long_docs = [huge, longword + " a " + longword, "x " + longword]
    queries = [" ".join(pool[int(k)] for k in r.integers(len(pool), size=8)) for _ in range(16)] + [longword, longword + " " + pool[0]]
    # the long documents appended to short ones; short ones appended to an index that holds the long ones (twice: the second batch
    # re-hashes the pair table the long document's workgroup reads its counts from)
    for parts in ([short[:1500], long_docs + short[1500:]], [short[:100] + long_docs, short[100:400], short[400:]]):
        docs = [d for p in parts for d in p]
        rs = Restated(docs)
        want_terms = lookup(model("BM25", docs), [longword, "a", "x", pool[0]])
        for cls, b, k1, delta in PARAMS:
            m = model(cls, parts[0], b, k1, 1.0 if delta is None else delta)
            for p in parts[1:]:
                m.add_documents(p)
            k = docs.index(huge)
            assert m.fieldLens[k] == 120_000 and m.fieldLens[k + 1] == 3
            got = m.get_scores(queries)
            want = rs.scores(queries, b, k1, delta)
            for q in range(len(queries)):
                assert same_bits(got[q], want[q]), (cls, len(parts), q)
            assert lookup(m, [longword, "a", "x", pool[0]]) == want_terms


# ---- 6: allocation failures: the index answers as before, the first success equals a fresh build -----------------------------------
def test_allocation_failure_sweep(corpus2):
    docs, queries = corpus2
    old, more = docs[:3000], docs[3000:4500] + ["onlyinthebatch zzz%d" % k for k in range(40)]
    queries = queries[:16]
    ctx = _native.Context()
    m = model("BM25", old, ctx=ctx)
    old_words = sorted({w for d in old[:60] for w in d.split()})
    new_words = sorted({w for d in more for w in d.split()} - {w for d in old for w in d.split()})[:300]
    assert new_words
    words = old_words + new_words
    before = (ctx.bm25_info(m._index), ctx.bm25_field_lengths(m._index).tolist(), lookup(m, words), m.get_scores(queries),
              m.top_k(queries, 10))
    assert all(t == -1 for t in before[2][0][len(old_words):])
    buf, off = pack(more)
    ok = None
    for k in range(1, 200):
        _native.debug_set("inject_bad_alloc", k, ctx)
        try:
            ctx.bm25_append(m._index, buf, off)
        except _native.GzError as e:
            _native.debug_set("inject_bad_alloc", 0, ctx)
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            assert ctx.bm25_info(m._index) == before[0], k
            assert ctx.bm25_field_lengths(m._index).tolist() == before[1], k
            assert lookup(m, words) == before[2], k
            assert same_bits(m.get_scores(queries), before[3]), k
            assert same_topk(m.top_k(queries, 10), before[4]), k
            ctx.preprocess([_native.GZ_PP_PUNCT], np.frombuffer(b"a,b", np.uint8), np.array([0, 3], np.int64))   # still usable
            continue
        ok = k
        break
    _native.debug_set("inject_bad_alloc", 0, ctx)
    assert ok is not None and ok > 5
    ref = model("BM25", old + more, ctx=ctx)
    assert ctx.bm25_info(m._index) == ctx.bm25_info(ref._index)
    assert ctx.bm25_field_lengths(m._index).tolist() == ref.fieldLens
    assert lookup(m, words) == lookup(ref, words)
    # (the Python object did not see the raw append: compare through the C face)
    wb, wo = pack([w for q in queries for w in q.split()])
    qoff = np.array([0] + list(np.cumsum([len(q.split()) for q in queries])), np.int64)
    terms, df = ctx.bm25_lookup(m._index, wb, wo)
    idf = np.array([R.idf(len(old) + len(more), int(x)) for x in df])
    params = ref._params()
    assert same_bits(ctx.bm25_score(m._index, terms, idf, qoff, params, False), ctx.bm25_score(ref._index, terms, idf, qoff, params, False))
    assert same_bits(ctx.bm25_score(ref._index, terms, idf, qoff, params, False), ref.get_scores(queries))
    del m, ref
    ctx.close()


# ---- 7: the device form --------------------------------------------------------------------------------------------------------
def test_device_form():
    old = ["a b c", "", "b b", "tiếng việt", "c a"] * 50
    more = ["việt nam a", "", "mới mới b", "  ", "c"] * 31
    queries = ["a", "b c", "việt x", "", "mới nam"]
    ctx = _native.Context()
    ob, oo = pack(old)
    ix = ctx.bm25_build(ob, oo)
    ih = ctx.bm25_build(ob, oo)
    buf, off = pack(more)
    pad = 7
    dt = ctx.alloc(len(buf) + pad)
    do = ctx.alloc(8 * len(off))
    ctx.h2d(dt, np.concatenate([np.full(pad, 32, np.uint8), buf]))
    ctx.h2d(do, off + pad)

    def state(i):
        words = sorted({w for d in old + more for w in d.split()}) + ["absent"]
        wb, wo = pack(words)
        t, d = ctx.bm25_lookup(i, wb, wo)
        qw = [w for q in queries for w in q.split()]
        qoff = np.array([0] + list(np.cumsum([len(q.split()) for q in queries])), np.int64)
        qb, qo = pack(qw)
        terms, df = ctx.bm25_lookup(i, qb, qo)
        n = ctx.bm25_info(i)[0]
        idf = np.array([R.idf(n, int(x)) for x in df])
        lens = ctx.bm25_field_lengths(i)
        params = [2.2, 1.2, 0.25, 0.75, float(np.mean(lens)), 0.0]
        return (ctx.bm25_info(i), lens.tolist(), t.tolist(), d.tolist(), bits(ctx.bm25_score(i, terms, idf, qoff, params, False)).tolist(),
                [x.tolist() for x in ctx.bm25_topk(i, terms, idf, qoff, params, False, 7)])

    before = state(ix)
    # refused: offsets that decrease, offsets that leave the announced text, a negative first offset
    for bad_off in (np.array([pad, pad + 5, pad + 3], np.int64), np.array([pad, pad + 4, int(off[-1]) + pad + 1], np.int64),
                    np.array([-1, 2, 3], np.int64)):
        db = ctx.alloc(8 * len(bad_off))
        ctx.h2d(db, bad_off)
        with pytest.raises(_native.GzError) as e:
            ctx.bm25_append_device(ix, dt, db, len(bad_off) - 1, int(off[-1]))
        assert e.value.code == _native.GZ_E_INVALID
        ctx.free(db)
        assert state(ix) == before
    # the limit is answered before anything is read: no device memory behind the call
    lib = ctx.lib
    assert lib.gz_bm25_append_device(ctypes.c_void_p(ix), None, None, 1, (1 << 32) - 200) == _native.GZ_E_LIMIT
    assert lib.gz_bm25_append_device(ctypes.c_void_p(ix), ctypes.c_void_p(16), ctypes.c_void_p(16), 5, (1 << 32)) == _native.GZ_E_LIMIT
    assert state(ix) == before
    assert lib.gz_bm25_append_device(ctypes.c_void_p(ix), None, None, 0, 0) == _native.GZ_OK
    assert lib.gz_bm25_append(ctypes.c_void_p(ix), None, None, 0) == _native.GZ_OK
    boff = np.array([5, 3], np.int64)
    assert lib.gz_bm25_append(ctypes.c_void_p(ix), None, ctypes.c_void_p(boff.ctypes.data), 1) == _native.GZ_E_INVALID
    assert state(ix) == before
    # the append itself, against the host form and a fresh build
    ctx.bm25_append_device(ix, dt, do, len(more), int(off[-1]))
    ctx.free(dt)
    ctx.free(do)
    ctx.bm25_append(ih, buf, off)
    fb, fo = pack(old + more)
    fresh = ctx.bm25_build(fb, fo)
    assert state(ix) == state(ih) == state(fresh) and state(ix) != before
    for i in (ix, ih, fresh):
        ctx.bm25_destroy(i)
    ctx.close()


# ---- 8: bystanders ---------------------------------------------------------------------------------------------------------------
def test_bystanders_unchanged_around_appends(corpus2):
    from genz_tokenize import Tokenize
    import corpus
    tok = Tokenize()
    t, o, _ = corpus.config_corpus(2, n_docs=5000)
    before = tok.encode_packed(t, o, max_len=64)
    docs, queries = corpus2
    a = model("BM25", docs[:500], 0.75, 1.2)
    other = model("BM25Plus", docs[30_000:40_000], 0.3, 2.0, 0.5)
    so, to = other.get_scores(queries[:8]), other.top_k(queries[:8], 100)
    a.add_documents(docs[500:20_000])
    during = tok.encode_packed(t, o, max_len=64)
    assert same_bits(other.get_scores(queries[:8]), so) and same_topk(other.top_k(queries[:8], 100), to)
    a.add_documents(docs[20_000:20_001])
    ref = model("BM25", docs[:20_001], 0.75, 1.2)
    assert same_topk(a.top_k(queries, 1000), ref.top_k(queries, 1000))      # k above the 500 documents the index began with
    assert same_bits(a.get_scores(queries[:8]), ref.get_scores(queries[:8]))
    assert same_bits(other.get_scores(queries[:8]), so)
    del a, other, ref
    after = tok.encode_packed(t, o, max_len=64)
    for r in (during, after):
        for k in ("input_ids", "attention_mask"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(before[k]))


# ---- 9: the Python surface ---------------------------------------------------------------------------------------------------------
def test_python_surface():
    docs = ["the cat sat", "dogs bark", "a cat and a dog", ""]
    for m in (BM25(docs), BM25Plus(docs, 0.3, 2.0, 0.5)):
        state = (m.num_doc, list(m.fieldLens), m.avgFieldLen, m.get_scores(["cat dog", "zebra"]))
        idf_cat = m.cal_idf("cat")
        for bad in (["zebra crossing", 3], [None], [b"zebra"]):
            with pytest.raises(TypeError):
                m.add_documents(bad)
            assert (m.num_doc, m.fieldLens, m.avgFieldLen) == state[:3] and same_bits(m.get_scores(["cat dog", "zebra"]), state[3])
            assert lookup(m, ["zebra"]) == ([-1], [0])
        m.add_documents([])
        m.add_documents(())
        assert (m.num_doc, m.fieldLens, m.avgFieldLen) == state[:3] and same_bits(m.get_scores(["cat dog", "zebra"]), state[3])
        more = ["zebra zebra crossing", "a zebra"]
        m.add_documents(iter(more))
        assert m.num_doc == 6 and m.fieldLens == [3, 2, 5, 0, 3, 2]
        assert same_bits([idf_cat], [R.idf(4, 2)]) and same_bits([m.cal_idf("cat")], [R.idf(6, 2)])     # not served from the cache
        assert m.get_top_n("zebra", n=2) == [more[1], more[0]] or m.get_top_n("zebra", n=2) == [more[0], more[1]]
        fresh = type(m)(docs + more, m.b, m.k1, *([m.delta] if isinstance(m, BM25Plus) else []))
        assert m.get_top_n("zebra crossing", n=3) == fresh.get_top_n("zebra crossing", n=3)
        assert m.get_top_n("zebra crossing", n=3)[0] == more[0]
        assert same_bits(m.get_scores(["zebra cat", ""]), fresh.get_scores(["zebra cat", ""]))
        with pytest.raises(ValueError):
            m.get_top_n("zebra", documents=docs)                            # (the old length no longer fits)
