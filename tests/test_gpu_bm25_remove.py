"""GPU: BM25.remove_documents / gz_bm25_remove[_device] (csrc/gz_bm25.inc).  An index that documents were removed from answers
exactly like one built fresh over the remaining documents: the oracles are the numpy restatement in tests/bm25_restate.py (idf
evaluated in this process) and this library's own fresh build of the remaining documents, whose code path the removal does not
touch.  Scores are compared as bit patterns (nan and -0.0 count); no tolerance appears anywhere.  Term ids are the one thing that
may differ from a fresh build: per word, df and "term == -1" are compared."""
import warnings

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


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def model(cls, docs, b=0.75, k1=1.2, delta=1.0, ctx=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (np.mean of no lengths, as the fresh build of [] warns)
        return BM25Plus(docs, b, k1, delta, ctx=ctx) if cls == "BM25Plus" else BM25(docs, b, k1, ctx=ctx)


def remove(m, ids):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert m.remove_documents(ids) is None


def remaining(docs, ids):
    gone = set(int(i) for i in ids)
    return [d for i, d in enumerate(docs) if i not in gone]


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


def lookup_of(ctx, index, words):
    buf, off = pack(list(words))
    t, d = ctx.bm25_lookup(index, buf, off)
    return (t == -1).tolist(), d.tolist()


def lookup(m, words):
    """per word: (no remaining document has it, df) -- not the term ids"""
    return lookup_of(m._ctx, m._index, words)


def same_topk(a, b):
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])


def assert_equal_models(m, ref, queries, words, ks=(10,), what=""):
    """everything observable of m equals the fresh model's"""
    assert m.num_doc == ref.num_doc and m.fieldLens == ref.fieldLens and type(m.fieldLens) is list, what
    assert bits([m.avgFieldLen]) == bits([ref.avgFieldLen]), what
    assert m._ctx.bm25_info(m._index) == ref._ctx.bm25_info(ref._index), what
    assert m._ctx.bm25_field_lengths(m._index).tolist() == ref.fieldLens, what
    absent, df = lookup(m, words)
    assert (absent, df) == lookup(ref, words), what
    assert all(a == (d == 0) for a, d in zip(absent, df)), what
    assert same_bits([m.cal_idf(w) for w in words[:40]], [ref.cal_idf(w) for w in words[:40]]), what
    assert same_bits(m.get_scores(queries), ref.get_scores(queries)), what
    for q in queries[:2]:
        got, want = m.get_score(q), ref.get_score(q)
        assert [type(v) for v in got] == [type(v) for v in want] and same_bits(got, want), (what, q)
    for k in ks:
        assert same_topk(m.top_k(queries, k), ref.top_k(queries, k)), (what, k)


def words_of(docs, extra=()):
    return sorted({w for d in docs for w in d.split()}) + ["absent", "x" * 70, ""] + list(extra)


@pytest.fixture(scope="module")
def corpus2():
    import corpus
    t, o, _ = corpus.config_corpus(2, n_docs=20_000)
    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    r = np.random.default_rng(8)
    vocab = sorted({w for d in docs[:2000] for w in d.split()})
    queries = []
    for k in range(32):
        words = [vocab[int(r.integers(len(vocab)))] if r.random() < 0.8 else "absent%d" % k for _ in range(int(r.integers(1, 9)))]
        if k % 5 == 0:
            words += words[:2]                                            # repeats
        queries.append(" ".join(words))
    queries[7] = ""
    return docs, queries


# ---- 1: every fixture case: nothing, the ends, every second, all but one, everything, a shuffled list with duplicates -----------
def removal_sets(N):
    r = np.random.default_rng(N + 1)
    sets = [[], [0], [N - 1], list(range(0, N, 2)), [i for i in range(N) if i != N // 2], list(range(N))]
    some = r.permutation(N)[:max(1, N // 3)].tolist()
    shuffled = some + some[:len(some) // 2 + 1] + some[:1]
    r.shuffle(shuffled)
    sets.append(shuffled)
    seen, out = set(), []
    for s in sets:
        s = [i for i in s if 0 <= i < N]
        key = tuple(s)
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_case(i):
    c = CASES[i]
    docs, queries = c["documents"], c["queries"]
    N = len(docs)
    words = words_of(docs)
    for ids in removal_sets(N):
        rest = remaining(docs, ids)
        rs = Restated(rest)
        for cls, b, k1, delta in PARAMS:
            d = 1.0 if delta is None else delta
            m = model(cls, docs, b, k1, d)
            remove(m, iter(ids))
            what = (i, cls, ids[:8], len(ids))
            assert m.num_doc == len(rest) == rs.n and m.fieldLens == [int(x) for x in rs.lens], what
            assert bits([m.avgFieldLen]) == bits([rs.avg]) or (np.isnan(m.avgFieldLen) and np.isnan(rs.avg) and not rest), what
            assert same_bits(m.get_scores(queries), rs.scores(queries, b, k1, delta)), what
            assert lookup(m, words)[1] == [rs.post.df(w) for w in words], what
            assert m.documents == [x.split() for x in rest], what
            assert [list(f.items()) for f in m.frequency_word_in_doc] == [list(f.items()) for f in R.stats(rest)[1]], what
            ref = model(cls, rest, b, k1, d)
            assert_equal_models(m, ref, queries, words, ks=(1, 10), what=what)
            if not rest:                                                    # everything: equals BM25([])
                assert m.num_doc == 0 and m.fieldLens == [] and np.isnan(m.avgFieldLen)
                assert all(m.get_score(q) == [] for q in queries)
                ids_k, sc_k = m.top_k(queries, 5)
                assert ids_k.shape == (len(queries), 0) and sc_k.shape == (len(queries), 0)
                m.add_documents(docs)
                assert_equal_models(m, model(cls, docs, b, k1, d), queries, words, ks=(1, 10), what=(what, "refilled"))


# ---- 2: terms that vanish with their last document and come back with an append ------------------------------------------------
def test_vanishing_and_returning_terms():
    docs = ["only here", "a b", "", "here too a", "  ", "b c unique1 unique1", "", "a c", "  ", "c c only"]
    gone = [0, 2, 3, 4, 5, 9]                                               # "only", "here", "too", "unique1" lose every document
    dead = ["only", "here", "too", "unique1"]
    rest = remaining(docs, gone)
    assert "" in rest and "  " in rest and not any(w in d.split() for d in rest for w in dead)
    queries = ["a only", "here b c", "unique1", "", "never a"]
    words = words_of(docs)
    for cls, b, k1, delta in PARAMS:
        d = 1.0 if delta is None else delta
        m = model(cls, docs, b, k1, d)
        assert lookup(m, dead) == ([False] * 4, [2, 2, 1, 1])
        remove(m, gone)
        ref = model(cls, rest, b, k1, d)
        assert lookup(m, dead + ["neverseen"]) == ([True] * 5, [0] * 5)
        assert same_bits([m.cal_idf(w) for w in dead], [m.cal_idf("neverseen")] * 4)
        assert m._ctx.bm25_info(m._index) == ref._ctx.bm25_info(ref._index) == (4, 3, 4)
        assert_equal_models(m, ref, queries, words, ks=(1, 3), what=cls)
        back = ["unique1 a", "", "here here brandnew", "  ", "only"]
        m.add_documents(back)
        ref = model(cls, rest + back, b, k1, d)
        assert lookup(m, dead) == ([False, False, True, False], [1, 1, 0, 1])
        assert m._ctx.bm25_info(m._index)[1] == 7                            # a b c + unique1 here only + brandnew
        assert_equal_models(m, ref, queries + ["brandnew too"], words + ["brandnew"], ks=(1, 3), what=(cls, "back"))
        remove(m, [4, 6])                                                   # "unique1 a", "here here brandnew": dead a second time
        ref = model(cls, remaining(rest + back, [4, 6]), b, k1, d)
        assert_equal_models(m, ref, queries + ["brandnew too"], words + ["brandnew"], ks=(1, 3), what=(cls, "again"))


# ---- 3: appends and removals interleaved -----------------------------------------------------------------------------------------
def test_interleaved_with_appends(corpus2):
    docs, queries = corpus2
    r = np.random.default_rng(3)
    for cls, b, k1, delta in PARAMS:
        d = 1.0 if delta is None else delta
        cur = list(docs[:6000])
        m = model(cls, cur, b, k1, d)

        def check(what):
            ref = model(cls, cur, b, k1, d)
            words = words_of(cur[:40] + cur[-40:] + docs[5990:6010])
            assert_equal_models(m, ref, queries, words, ks=(1, 10, min(1024, len(cur))), what=(cls, what))

        m.add_documents(docs[6000:9000])
        cur += docs[6000:9000]
        check("add 3000")
        ids = r.choice(len(cur), size=2500, replace=False)
        remove(m, ids.tolist())
        cur = remaining(cur, ids)
        check("remove 2500")
        m.add_documents(docs[9000:10_000])
        cur += docs[9000:10_000]
        check("add 1000")
        ids = range(3600, 4600)                                             # (4096 is a scan block's edge)
        remove(m, ids)
        cur = remaining(cur, ids)
        check("remove 3600..4600")
        assert m.num_doc == 6500 and m.get_top_n(queries[0], n=3) == [cur[i] for i in m.top_k([queries[0]], 3)[0][0].tolist()]


# ---- 4: scan and grid boundaries ---------------------------------------------------------------------------------------------------
def test_scan_and_grid_boundaries(corpus2):
    docs, queries = corpus2
    r = np.random.default_rng(4)
    ids = r.choice(20_000, size=6000, replace=False)
    rest = remaining(docs, ids)
    rs = Restated(rest)
    for cls, b, k1, delta in PARAMS:
        d = 1.0 if delta is None else delta
        m = model(cls, docs, b, k1, d)
        remove(m, ids.tolist())
        ref = model(cls, rest, b, k1, d)
        assert_equal_models(m, ref, queries, words_of(docs[:60] + docs[-60:]), ks=(1, 10, 1024), what=cls)
        assert same_bits(m.get_scores(queries), rs.scores(queries, b, k1, delta))
    small = docs[:257]
    for ids in ([255, 256], [255], [256], [0, 255], [256, 0]):
        m = model("BM25", small)
        remove(m, ids)
        assert_equal_models(m, model("BM25", remaining(small, ids)), queries, words_of(small), ks=(1, 10, 255), what=ids)


# ---- 5: hash bits truncated: chains of dead, live and revived terms ----------------------------------------------------------------
@pytest.mark.parametrize("hash_bits", [4, 10])
def test_truncated_hash_changes_nothing(corpus2, hash_bits):
    docs, queries = corpus2
    base = docs[:3000]
    r = np.random.default_rng(hash_bits)
    ids = r.choice(3000, size=1000, replace=False)
    rest = remaining(base, ids)
    dead = sorted({w for d in base for w in d.split()} - {w for d in rest for w in d.split()})
    assert len(dead) > 20
    more = [base[int(i)] for i in ids[:250]] + docs[3000:3250]               # the first half brings dead terms back
    revived = [w for w in dead if any(w in d.split() for d in more)]
    assert revived and len(revived) < len(dead)
    words = words_of(base[:50] + more[-50:], dead[:300])
    ctx = _native.Context()
    try:
        _native.debug_set("bm25_hash_bits", hash_bits, ctx)
        m = model("BM25", base, ctx=ctx)
        remove(m, ids.tolist())
        ref = model("BM25", rest, ctx=ctx)
        assert_equal_models(m, ref, queries, words, what=(hash_bits, "removed"))
        assert lookup(m, dead) == ([True] * len(dead), [0] * len(dead))
        m.add_documents(more)
        ref2 = model("BM25", rest + more, ctx=ctx)
        assert_equal_models(m, ref2, queries, words, what=(hash_bits, "appended"))
        assert not any(lookup(m, revived)[0])
        buf, off = pack(sorted(set(words)))                                 # distinct words stay distinct terms
        t, _ = ctx.bm25_lookup(m._index, buf, off)
        assert len(set(t[t >= 0].tolist())) == int((t >= 0).sum())
        del m, ref, ref2
    finally:
        _native.debug_set("bm25_hash_bits", 0, ctx)
        ctx.close()
    _native.debug_set("bm25_hash_bits", 0)


# ---- 6: a document of 120 000 words and 80 000-byte words: its workgroup reads counts from the pair table -------------------------
def test_long_documents_and_words():
    import corpus
    t, o, _ = corpus.config_corpus(4, n_docs=400)
    raw = t.tobytes()
    short = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    r = np.random.default_rng(4)
    pool = sorted({w for d in short[:200] for w in d.split()})
    huge = " ".join(pool[int(k)] for k in r.integers(len(pool), size=120_000))
    longword = "ư" * 40_000                                                # 80 000 bytes
    long_docs = [huge, longword + " a " + longword, "x " + longword]
    docs = short[:150] + long_docs + short[150:]
    queries = [" ".join(pool[int(k)] for k in r.integers(len(pool), size=8)) for _ in range(16)] + [longword, longword + " " + pool[0]]
    LDS_ENTRIES = 4096                                                      # BM_SC_LDS of gz_bm25_score_kernel: more -> the pair table
    for ids in ([3, 77, 149], [153, 200, 402], [10, 151, 300], [150, 152, 20], [150, 151, 152], list(range(0, 150)) + [160]):
        rest = remaining(docs, ids)
        if huge in rest:
            k = rest.index(huge)
            block = rest[k // 256 * 256:k // 256 * 256 + 256]
            assert sum(len(set(x.split())) for x in block) > LDS_ENTRIES    # the huge document's workgroup does not fit LDS
        rs = Restated(rest)
        for cls, b, k1, delta in PARAMS:
            m = model(cls, docs, b, k1, 1.0 if delta is None else delta)
            remove(m, ids)
            assert m.fieldLens == [int(x) for x in rs.lens]
            got = m.get_scores(queries)
            want = rs.scores(queries, b, k1, delta)
            for q in range(len(queries)):
                assert same_bits(got[q], want[q]), (cls, ids[:4], q)
            ref = model(cls, rest, b, k1, 1.0 if delta is None else delta)
            assert_equal_models(m, ref, queries, [longword, "a", "x", pool[0], "absent"], ks=(1, 10), what=(cls, ids[:4]))


# ---- 7: failures: the index answers as before ----------------------------------------------------------------------------------------
def c_state(ctx, index, words, queries, n_for_idf=None):
    """what the C face answers: info, fieldLens, lookup, scores, top-k"""
    absent, df = lookup_of(ctx, index, words)
    qw = [w for q in queries for w in q.split()]
    qoff = np.array([0] + list(np.cumsum([len(q.split()) for q in queries])), np.int64)
    qb, qo = pack(qw)
    terms, qdf = ctx.bm25_lookup(index, qb, qo)
    n = ctx.bm25_info(index)[0]
    idf = np.array([R.idf(n, int(x)) for x in qdf])
    lens = ctx.bm25_field_lengths(index)
    params = [2.2, 1.2, 0.25, 0.75, float(np.mean(lens)) if n else float("nan"), 0.0]
    scores = ctx.bm25_score(index, terms, idf, qoff, params, False)
    topk = ctx.bm25_topk(index, terms, idf, qoff, params, False, 7)
    return (ctx.bm25_info(index), lens.tolist(), absent, df, bits(scores).tolist(), [x.tolist() for x in topk])


def test_bad_ids_leave_the_index_as_it_was(corpus2):
    docs, queries = corpus2
    docs, queries = docs[:300], queries[:8]
    ctx = _native.Context()
    buf, off = pack(docs)
    ix = ctx.bm25_build(buf, off)
    words = words_of(docs[:30])
    before = c_state(ctx, ix, words, queries)
    for ids in ([300], [-1], [5, 300, 7], [0, 1, -1], [1 << 40], [-(1 << 62)]):
        with pytest.raises(_native.GzError) as e:
            ctx.bm25_remove(ix, np.array(ids, np.int64))
        assert e.value.code == _native.GZ_E_INVALID, ids
        assert c_state(ctx, ix, words, queries) == before, ids
    ctx.bm25_remove(ix, np.zeros(0, np.int64))
    assert c_state(ctx, ix, words, queries) == before
    ctx.bm25_destroy(ix)
    ctx.close()


def test_allocation_failure_sweep(corpus2):
    docs, queries = corpus2
    docs, queries = docs[:3000], queries[:16]
    r = np.random.default_rng(7)
    ids = r.choice(3000, size=1000, replace=False).astype(np.int64)
    rest = remaining(docs, ids)
    ctx = _native.Context()
    m = model("BM25", docs, ctx=ctx)
    dead = sorted({w for d in docs for w in d.split()} - {w for d in rest for w in d.split()})[:200]
    words = words_of(docs[:60], dead)
    before = c_state(ctx, m._index, words, queries)
    ok = None
    for k in range(1, 200):
        _native.debug_set("inject_bad_alloc", k, ctx)
        try:
            ctx.bm25_remove(m._index, ids)
        except _native.GzError as e:
            _native.debug_set("inject_bad_alloc", 0, ctx)
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            assert c_state(ctx, m._index, words, queries) == before, k
            ctx.preprocess([_native.GZ_PP_PUNCT], np.frombuffer(b"a,b", np.uint8), np.array([0, 3], np.int64))   # still usable
            continue
        ok = k
        break
    _native.debug_set("inject_bad_alloc", 0, ctx)
    assert ok is not None and ok > 5
    ref = model("BM25", rest, ctx=ctx)
    # (the Python object did not see the raw removal: compare through the C face)
    after = c_state(ctx, m._index, words, queries)
    assert after == c_state(ctx, ref._index, words, queries) and after != before
    assert same_bits(np.array(after[4], np.uint64).view(np.float64).reshape(len(queries), -1),
                     model("BM25", rest, 0.75, 1.2, ctx=ctx).get_scores(queries))
    ctx.preprocess([_native.GZ_PP_PUNCT], np.frombuffer(b"a,b", np.uint8), np.array([0, 3], np.int64))
    del m, ref
    ctx.close()


# ---- 8: the device form ------------------------------------------------------------------------------------------------------------
def test_device_form():
    docs = ["a b c", "", "b b", "tiếng việt", "c a"] * 50
    docs[17] = "onlyhere b"
    queries = ["a", "b c", "việt x", "", "onlyhere a"]
    ids = np.array([17, 0, 249, 100, 17, 3, 8, 13, 18, 23, 101, 102, 249], np.int64)
    words = words_of(docs)
    ctx = _native.Context()
    buf, off = pack(docs)
    ix = ctx.bm25_build(buf, off)
    ih = ctx.bm25_build(buf, off)
    before = c_state(ctx, ix, words, queries)
    d_ids = ctx.alloc(8 * len(ids))
    bad = ids.copy()
    bad[5] = 250
    ctx.h2d(d_ids, bad)
    with pytest.raises(_native.GzError) as e:
        ctx.bm25_remove_device(ix, d_ids, len(ids))
    assert e.value.code == _native.GZ_E_INVALID and c_state(ctx, ix, words, queries) == before
    ctx.bm25_remove_device(ix, d_ids, 0)
    ctx.bm25_remove_device(ix, None, 0)
    assert c_state(ctx, ix, words, queries) == before
    ctx.h2d(d_ids, ids)
    ctx.bm25_remove_device(ix, d_ids, len(ids))
    ctx.free(d_ids)
    ctx.bm25_remove(ih, ids)
    fb, fo = pack(remaining(docs, ids))
    fresh = ctx.bm25_build(fb, fo)
    s = c_state(ctx, ix, words, queries)
    assert s == c_state(ctx, ih, words, queries) == c_state(ctx, fresh, words, queries) and s != before
    assert s[0][0] == 250 - len(set(ids.tolist())) and lookup_of(ctx, ix, ["onlyhere"]) == ([True], [0])
    for i in (ix, ih, fresh):
        ctx.bm25_destroy(i)
    ctx.close()


# ---- 9: bystanders and the Python surface --------------------------------------------------------------------------------------------
def test_bystanders_unchanged_around_removals(corpus2):
    from genz_tokenize import Tokenize
    import corpus
    tok = Tokenize()
    t, o, _ = corpus.config_corpus(2, n_docs=2000)
    before = tok.encode_packed(t, o, max_len=64)
    docs, queries = corpus2
    a = model("BM25", docs[:5000], 0.75, 1.2)
    other = model("BM25Plus", docs[10_000:14_000], 0.3, 2.0, 0.5)
    so, to = other.get_scores(queries[:8]), other.top_k(queries[:8], 100)
    remove(a, range(100, 2100))
    during = tok.encode_packed(t, o, max_len=64)
    assert same_bits(other.get_scores(queries[:8]), so) and same_topk(other.top_k(queries[:8], 100), to)
    remove(a, [0])
    ref = model("BM25", docs[1:100] + docs[2100:5000], 0.75, 1.2)
    assert same_topk(a.top_k(queries, 1000), ref.top_k(queries, 1000))
    assert same_bits(a.get_scores(queries[:8]), ref.get_scores(queries[:8]))
    assert same_bits(other.get_scores(queries[:8]), so) and same_topk(other.top_k(queries[:8], 100), to)
    del a, other, ref
    after = tok.encode_packed(t, o, max_len=64)
    for r in (during, after):
        for k in ("input_ids", "attention_mask"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(before[k]))


def test_python_surface():
    docs = ["the cat sat", "dogs bark", "a cat and a dog", "", "zebra zebra crossing", "a zebra"]
    q = ["cat dog", "zebra"]
    for m in (BM25(docs), BM25Plus(docs, 0.3, 2.0, 0.5)):
        assert m.documents[4] == ["zebra", "zebra", "crossing"] and m.frequency_word_in_doc[2] == {"a": 2, "cat": 1, "and": 1, "dog": 1}
        state = (m.num_doc, list(m.fieldLens), m.avgFieldLen, m.get_scores(q))
        idf_cat = m.cal_idf("cat")

        def unchanged():
            return (m.num_doc, m.fieldLens, m.avgFieldLen) == state[:3] and same_bits(m.get_scores(q), state[3])

        for bad in (["3"], [1.0], [True], [0, "1"], [2, None], [np.float64(1)]):
            with pytest.raises(TypeError):
                m.remove_documents(bad)
            assert unchanged()
        for bad in ([6], [-1], [0, 6], [1, -6], [10 ** 30]):
            with pytest.raises(IndexError):
                m.remove_documents(bad)
            assert unchanged()
        assert m.remove_documents([]) is None and m.remove_documents(()) is None and m.remove_documents(iter([])) is None
        assert unchanged()
        assert m.remove_documents(iter([np.int64(3), 1, 3])) is None
        rest = [docs[0], docs[2], docs[4], docs[5]]
        fresh = type(m)(rest, m.b, m.k1, *([m.delta] if isinstance(m, BM25Plus) else []))
        assert m.num_doc == 4 and m.fieldLens == [3, 5, 3, 2] == fresh.fieldLens and bits([m.avgFieldLen]) == bits([fresh.avgFieldLen])
        assert same_bits([idf_cat], [R.idf(6, 2)]) and same_bits([m.cal_idf("cat")], [R.idf(4, 2)])      # not served from the cache
        assert m.documents == fresh.documents and m.frequency_word_in_doc == fresh.frequency_word_in_doc
        assert [list(f) for f in m.frequency_word_in_doc] == [list(f) for f in fresh.frequency_word_in_doc]
        assert lookup(m, ["dogs", "bark", "cat"]) == ([True, True, False], [0, 0, 2])
        assert same_bits(m.get_scores(q + [""]), fresh.get_scores(q + [""]))
        assert m.get_top_n("zebra crossing", n=3) == fresh.get_top_n("zebra crossing", n=3)
        assert m.get_top_n("zebra crossing", n=3)[0] == docs[4] and set(m.get_top_n("cat", n=4)) <= set(rest)
        with pytest.raises(ValueError):
            m.get_top_n("zebra", documents=docs)                            # (the old length no longer fits)
        assert m.get_top_n("zebra", documents=["w", "x", "y", "z"], n=2) == fresh.get_top_n("zebra", documents=["w", "x", "y", "z"], n=2)
