"""GPU: BM25.compact / vocabulary / footprint, gz_bm25_compact / gz_bm25_terms / gz_bm25_footprint (csrc/gz_bm25.inc).  A compacted
index answers exactly like one built fresh over its current documents, and now its term ids are that build's as well.  The oracles
are the numpy restatement in tests/bm25_restate.py, this library's own fresh build of the current documents (whose code path the
compaction does not touch) and a vocabulary computed in Python: the words of the current documents in the order of their first
occurrence, df = the documents that contain the word.  Scores are compared as bit patterns; no tolerance appears anywhere."""
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


# ---- helpers (the removal test's, copied) ------------------------------------------------------------------------------------------
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
    """per word: (no current document has it, df) -- not the term ids"""
    return lookup_of(m._ctx, m._index, words)


def ids_of(ctx, index, words):
    """the term ids themselves"""
    buf, off = pack(list(words))
    return ctx.bm25_lookup(index, buf, off)[0].tolist()


def term_ids(m, words):
    return ids_of(m._ctx, m._index, words)


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


def c_state(ctx, index, words, queries):
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
    # (top-k scores as bit patterns too: a corpus of empty documents scores nan, and nan != nan)
    return (ctx.bm25_info(index), lens.tolist(), absent, df, bits(scores).tolist(), [topk[0].tolist(), bits(topk[1]).tolist()])


# ---- the vocabulary oracle ---------------------------------------------------------------------------------------------------------
def py_vocab(docs):
    """(words in the order of their first occurrence, documents that contain each)"""
    df = {}
    for d in docs:
        for w in dict.fromkeys(d.split()):
            df[w] = df.get(w, 0) + 1
    return list(df), list(df.values())


def vocab(m):
    words, df = m.vocabulary()
    assert type(words) is list and all(type(w) is str for w in words)
    assert isinstance(df, np.ndarray) and df.dtype == np.int32 and df.shape == (len(words),)
    return words, df.tolist()


def compact(m):
    assert m.compact() is None


def assert_canonical(m, cur, ref, queries, words, ks=(10,), what=""):
    """m equals the fresh model `ref` of the documents `cur`, the term ids and the vocabulary included"""
    assert_equal_models(m, ref, queries, words, ks=ks, what=what)
    assert term_ids(m, words) == term_ids(ref, words), what
    v = vocab(m)
    assert v == py_vocab(cur), what
    assert v == vocab(ref), what
    live = [t for t in term_ids(m, v[0])]
    assert live == list(range(len(v[0]))), what                             # words[i] is the term with id i


@pytest.fixture(scope="module")
def corpus2():
    import corpus
    t, o, _ = corpus.config_corpus(2, n_docs=10_000)
    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    r = np.random.default_rng(8)
    vocab_ = sorted({w for d in docs[:2000] for w in d.split()})
    queries = []
    for k in range(32):
        words = [vocab_[int(r.integers(len(vocab_)))] if r.random() < 0.8 else "absent%d" % k for _ in range(int(r.integers(1, 9)))]
        if k % 5 == 0:
            words += words[:2]                                            # repeats
        queries.append(" ".join(words))
    queries[7] = ""
    return docs, queries


# ---- 1: every fixture case under the removal test's removal sets -------------------------------------------------------------------
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
        want_vocab = py_vocab(rest)
        for cls, b, k1, delta in PARAMS:
            d = 1.0 if delta is None else delta
            what = (i, cls, ids[:8], len(ids))
            m = model(cls, docs, b, k1, d)
            remove(m, iter(ids))
            before = c_state(m._ctx, m._index, words, queries)
            v_before = vocab(m)                                             # before the compaction: the same answer, nothing modified
            assert v_before == want_vocab, what
            assert c_state(m._ctx, m._index, words, queries) == before, what
            compact(m)
            assert c_state(m._ctx, m._index, words, queries)[:2] == before[:2], what
            assert same_bits(m.get_scores(queries), rs.scores(queries, b, k1, delta)), what
            ref = model(cls, rest, b, k1, d)
            assert_canonical(m, rest, ref, queries, words, ks=(1, 10), what=what)
            assert vocab(m) == v_before, what
            state = (term_ids(m, words), vocab(m), m.footprint(), c_state(m._ctx, m._index, words, queries))
            compact(m)                                                      # a second one changes nothing
            assert (term_ids(m, words), vocab(m), m.footprint(), c_state(m._ctx, m._index, words, queries)) == state, what
            assert m.footprint()["table_terms"] == len(want_vocab[0]) and m.footprint()["text_bytes"] == sum(
                len(w.encode("utf-8", "surrogatepass")) for w in want_vocab[0]), what


# ---- 2: a fresh index is canonical already -----------------------------------------------------------------------------------------
def test_fresh_index_is_canonical(corpus2):
    docs, queries = corpus2
    docs = docs[:3000]
    words = words_of(docs)
    m = model("BM25", docs)
    ids = term_ids(m, words)
    want = py_vocab(docs)
    assert vocab(m) == want
    assert [ids[words.index(w)] for w in want[0][:500]] == list(range(500))
    scores = m.get_scores(queries)
    compact(m)
    assert term_ids(m, words) == ids
    assert vocab(m) == want
    assert same_bits(m.get_scores(queries), scores)
    assert_canonical(m, docs, model("BM25", docs), queries, words, ks=(1, 10), what="fresh")


# ---- 3: compaction gives memory back -------------------------------------------------------------------------------------------------
def test_reclaim(corpus2):
    docs, queries = corpus2
    docs = docs[:6000]
    r = np.random.default_rng(33)
    ids = r.choice(6000, size=4000, replace=False)
    rest = remaining(docs, ids)
    distinct = py_vocab(docs)[0]
    left = py_vocab(rest)[0]
    assert len(left) < len(distinct)
    m = model("BM25", docs)
    f0 = m.footprint()
    assert sorted(f0) == ["device_bytes", "table_terms", "text_bytes"] and all(type(v) is int for v in f0.values())
    assert f0["text_bytes"] == int(pack(docs)[1][-1]) and f0["table_terms"] == len(distinct)
    remove(m, ids.tolist())
    f1 = m.footprint()
    assert (f1["text_bytes"], f1["table_terms"]) == (f0["text_bytes"], f0["table_terms"])      # a removal reclaims neither
    compact(m)
    f2 = m.footprint()
    assert f2["text_bytes"] == sum(len(w.encode("utf-8", "surrogatepass")) for w in left)
    assert f2["table_terms"] == m._ctx.bm25_info(m._index)[1] == len(left)
    assert f2["device_bytes"] < f1["device_bytes"] and f2["device_bytes"] < f0["device_bytes"]
    # another route to the same documents: every buffer is sized by the counts alone, so the footprints are equal
    m2 = model("BM25", docs[:3000])
    m2.add_documents(docs[3000:])
    remove(m2, ids.tolist())
    assert m2.footprint()["device_bytes"] > f2["device_bytes"]
    compact(m2)
    assert m2.footprint() == f2
    words = words_of(docs[:100] + rest[-100:])
    ref = model("BM25", rest)
    assert_canonical(m, rest, ref, queries, words, ks=(1, 10), what="reclaim")
    assert_canonical(m2, rest, ref, queries, words, ks=(1, 10), what="reclaim, other route")


# ---- 4: life after compaction ------------------------------------------------------------------------------------------------------
def test_life_after_compaction_small():
    docs = ["only here", "a b", "", "here too a", "  ", "b c unique1 unique1", "", "a c", "  ", "c c only"]
    gone = [0, 2, 3, 4, 5, 9]                                               # "only", "here", "too", "unique1" lose every document
    dead = ["only", "here", "too", "unique1"]
    rest = remaining(docs, gone)
    queries = ["a only", "here b c", "unique1", "", "never a"]
    words = words_of(docs) + ["brandnew"]
    for cls, b, k1, delta in PARAMS:
        d = 1.0 if delta is None else delta
        m = model(cls, docs, b, k1, d)
        remove(m, gone)
        assert m.footprint()["table_terms"] == 7                            # a b c and the four dead ones: all still held
        compact(m)
        assert (m.footprint()["text_bytes"], m.footprint()["table_terms"]) == (3, 3)
        assert vocab(m) == (["a", "b", "c"], [2, 1, 1])
        assert lookup(m, dead) == ([True] * 4, [0] * 4)
        assert_canonical(m, rest, model(cls, rest, b, k1, d), queries, words, ks=(1, 3), what=cls)
        back = ["unique1 a", "", "here here brandnew", "  ", "only"]       # revives three dead words, brings a new one
        m.add_documents(back)
        cur = rest + back
        assert vocab(m)[0] == ["a", "b", "c", "unique1", "here", "brandnew", "only"]
        assert m.footprint()["text_bytes"] == 3 + int(pack(back)[1][-1])        # the batch lies behind the arena
        assert_canonical(m, cur, model(cls, cur, b, k1, d), queries + ["brandnew too"], words, ks=(1, 3), what=(cls, "back"))
        remove(m, [4, 6])                                                   # "unique1 a", "here here brandnew"
        cur = remaining(cur, [4, 6])
        compact(m)
        assert vocab(m) == (["a", "b", "c", "only"], [2, 1, 1, 1])
        assert_canonical(m, cur, model(cls, cur, b, k1, d), queries + ["brandnew too"], words, ks=(1, 3), what=(cls, "again"))


def test_life_after_compaction_interleaved(corpus2):
    docs, queries = corpus2
    r = np.random.default_rng(3)
    for cls, b, k1, delta in PARAMS:
        d = 1.0 if delta is None else delta
        cur = list(docs[:6000])
        m = model(cls, cur, b, k1, d)

        def check(what):
            ref = model(cls, cur, b, k1, d)
            words = words_of(cur[:40] + cur[-40:] + docs[5990:6010])
            assert_canonical(m, cur, ref, queries, words, ks=(1, 10, min(1024, len(cur))), what=(cls, what))

        m.add_documents(docs[6000:9000])
        cur += docs[6000:9000]
        ids = r.choice(len(cur), size=2500, replace=False)
        remove(m, ids.tolist())
        cur = remaining(cur, ids)
        compact(m)
        check("remove 2500, compact")
        m.add_documents(docs[9000:10_000])
        cur += docs[9000:10_000]
        check("add 1000")
        ids = range(3600, 4600)                                             # (4096 is a scan block's edge)
        remove(m, ids)
        cur = remaining(cur, ids)
        compact(m)
        check("remove 3600..4600, compact")
        assert m.num_doc == 6500


# ---- 5: the scan's rounds (256) and block (4096), in live terms and in live entries ---------------------------------------------------
@pytest.mark.parametrize("K", [255, 256, 257, 4095, 4096, 4097])
def test_scan_and_grid_edges(K):
    queries = ["s0 w7", "w%d s1" % (K + 30), "s2 s2 absent", ""]
    r = np.random.default_rng(K)
    # (a) live TERMS = K: every document brings one new word and one of three shared ones; documents 0 .. 2, where the shared words
    # occur first, go: their first occurrence moves to a later document and their ids with it
    M = K + 40
    docs = ["w%d s%d" % (i, i % 3) for i in range(M)]
    gone = [0, 1, 2] + (3 + r.choice(M - 3, size=M - (K - 3) - 3, replace=False)).tolist()
    rest = remaining(docs, gone)
    assert len(rest) == K - 3 and len(py_vocab(rest)[0]) == K
    m = model("BM25", docs)
    words = words_of(docs)
    assert term_ids(m, ["w0", "s0", "w1", "s1", "w2", "s2"]) == [0, 1, 2, 3, 4, 5]
    remove(m, gone)
    compact(m)
    ref = model("BM25", rest)
    assert m._ctx.bm25_info(m._index)[1] == K == m.footprint()["table_terms"]
    assert_canonical(m, rest, ref, queries, words, ks=(1, 10), what=(K, "terms"))
    first = {w: i for i, w in enumerate(py_vocab(rest)[0])}
    assert term_ids(m, ["s0", "s1", "s2"]) == [first["s0"], first["s1"], first["s2"]] and min(first["s0"], first["s1"], first["s2"]) == 1
    # (b) live ENTRIES = K: documents of one word, five of them with a shared word as well
    M = K + 30
    docs = ["w%d" % i for i in range(M)]
    for j in (0, 5, 300 % M, M - 2, M // 2):
        docs[j] += " s0"
    two = {0, 5, 300 % M, M - 2, M // 2}
    assert len(two) == 5
    gone = [0]                                                              # (s0's first occurrence) ... and 4 entries stay with s0
    pool = [i for i in range(1, M) if i not in two]
    gone += r.choice(pool, size=(M + 5) - 2 - K, replace=False).tolist()
    rest = remaining(docs, gone)
    assert sum(len(set(x.split())) for x in rest) == K
    m = model("BM25", docs)
    words = words_of(docs)
    remove(m, gone)
    compact(m)
    assert_canonical(m, rest, model("BM25", rest), queries, words, ks=(1, 10), what=(K, "entries"))


# ---- 6: hash bits truncated ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_bits", [4, 10])
def test_truncated_hash(corpus2, hash_bits):
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
        compact(m)
        ref = model("BM25", rest, ctx=ctx)
        assert_canonical(m, rest, ref, queries, words, what=(hash_bits, "compacted"))
        assert lookup(m, dead) == ([True] * len(dead), [0] * len(dead))
        assert not set(dead) & set(vocab(m)[0])
        buf, off = pack(sorted(set(words)))                                 # distinct words are distinct terms
        t, _ = ctx.bm25_lookup(m._index, buf, off)
        assert len(set(t[t >= 0].tolist())) == int((t >= 0).sum())
        m.add_documents(more)
        ref2 = model("BM25", rest + more, ctx=ctx)
        assert_canonical(m, rest + more, ref2, queries, words, what=(hash_bits, "appended"))
        assert not any(lookup(m, revived)[0])
        t, _ = ctx.bm25_lookup(m._index, buf, off)
        assert len(set(t[t >= 0].tolist())) == int((t >= 0).sum())
        del m, ref, ref2
    finally:
        _native.debug_set("bm25_hash_bits", 0, ctx)
        ctx.close()
    _native.debug_set("bm25_hash_bits", 0)


# ---- 7: a document of 120 000 words and 80 000-byte words ----------------------------------------------------------------------------
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
    # a neighbour; the first long-word document (the word's first occurrence moves); both of them (the word dies); the long ones
    for ids in ([3, 77, 149], [151, 10], [151, 152, 300], [150, 151, 152]):
        rest = remaining(docs, ids)
        if huge in rest:
            k = rest.index(huge)
            block = rest[k // 256 * 256:k // 256 * 256 + 256]
            assert sum(len(set(x.split())) for x in block) > LDS_ENTRIES    # the huge document's workgroup does not fit LDS
        rs = Restated(rest)
        survives = any(longword in x.split() for x in rest)
        for cls, b, k1, delta in PARAMS:
            m = model(cls, docs, b, k1, 1.0 if delta is None else delta)
            remove(m, ids)
            compact(m)
            assert m.fieldLens == [int(x) for x in rs.lens]
            got = m.get_scores(queries)
            want = rs.scores(queries, b, k1, delta)
            for q in range(len(queries)):
                assert same_bits(got[q], want[q]), (cls, ids[:4], q)
            words, df = vocab(m)
            assert (words, df) == py_vocab(rest), (cls, ids[:4])
            assert (longword in words) == survives and len(set(words)) == len(words), (cls, ids[:4])
            if cls == "BM25":
                ref = model(cls, rest, b, k1)
                assert_canonical(m, rest, ref, queries, [longword, "a", "x", pool[0], "absent"], ks=(1, 10), what=(cls, ids[:4]))


# ---- 8: failures: the index answers as before --------------------------------------------------------------------------------------
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
    ctx.bm25_remove(m._index, ids)
    before = c_state(ctx, m._index, words, queries)
    ids_before = ids_of(ctx, m._index, words)
    foot = ctx.bm25_footprint(m._index)
    want = py_vocab(rest)

    def sweep(call):
        for k in range(1, 200):
            _native.debug_set("inject_bad_alloc", k, ctx)
            try:
                out = call()
            except _native.GzError as e:
                _native.debug_set("inject_bad_alloc", 0, ctx)
                assert e.code == _native.GZ_E_NOMEM, (k, e)
                assert c_state(ctx, m._index, words, queries) == before, k
                assert ids_of(ctx, m._index, words) == ids_before and ctx.bm25_footprint(m._index) == foot, k
                ctx.preprocess([_native.GZ_PP_PUNCT], np.frombuffer(b"a,b", np.uint8), np.array([0, 3], np.int64))   # still usable
                continue
            _native.debug_set("inject_bad_alloc", 0, ctx)
            return k, out
        raise AssertionError("no call succeeded")

    k, (off, data, df) = sweep(lambda: ctx.bm25_terms(m._index))
    assert k > 5
    raw = data.tobytes()
    assert ([raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)], df.tolist()) == want
    assert c_state(ctx, m._index, words, queries) == before and ctx.bm25_footprint(m._index) == foot
    k, _ = sweep(lambda: ctx.bm25_compact(m._index))
    assert k > 10
    ref = model("BM25", rest, ctx=ctx)
    after = c_state(ctx, m._index, words, queries)
    assert after == c_state(ctx, ref._index, words, queries) == before
    assert ids_of(ctx, m._index, words) == ids_of(ctx, ref._index, words) != ids_before
    assert ctx.bm25_footprint(m._index)[2] < foot[2] and ctx.bm25_footprint(m._index)[1] == len(want[0])
    ctx.preprocess([_native.GZ_PP_PUNCT], np.frombuffer(b"a,b", np.uint8), np.array([0, 3], np.int64))
    del m, ref
    ctx.close()


def test_no_documents():
    for cls, b, k1, delta in PARAMS:
        d = 1.0 if delta is None else delta
        m = model(cls, [], b, k1, d)
        compact(m)
        words, df = m.vocabulary()
        assert words == [] and df.dtype == np.int32 and df.shape == (0,)
        f = m.footprint()
        assert f["text_bytes"] == 0 and f["table_terms"] == 0 and f["device_bytes"] > 0
        m.add_documents(["b a", "a"])
        assert vocab(m) == (["b", "a"], [1, 2])
        remove(m, [0, 1])                                                   # everything removed
        assert vocab(m) == ([], []) and m.footprint()["table_terms"] == 2
        compact(m)
        assert vocab(m) == ([], []) and m.footprint() == f
        docs = ["x y", "", "y z z"]
        m.add_documents(docs)
        assert_canonical(m, docs, model(cls, docs, b, k1, d), ["y", "z x", ""], words_of(docs) + ["a", "b"], ks=(1, 3), what=cls)
    ctx = _native.Context()
    buf, off = pack([])
    ix = ctx.bm25_build(buf, off)
    ctx.bm25_compact(ix)
    o, data, df = ctx.bm25_terms(ix)
    assert o.tolist() == [0] and len(data) == 0 and len(df) == 0
    assert ctx.bm25_footprint(ix)[:2] == (0, 0)
    ctx.bm25_destroy(ix)
    ctx.close()


# ---- 9: bystanders -------------------------------------------------------------------------------------------------------------------
def test_bystanders_unchanged_around_compactions(corpus2):
    from genz_tokenize import Tokenize
    import corpus
    tok = Tokenize()
    t, o, _ = corpus.config_corpus(2, n_docs=2000)
    before = tok.encode_packed(t, o, max_len=64)
    docs, queries = corpus2
    a = model("BM25", docs[:5000], 0.75, 1.2)
    other = model("BM25Plus", docs[6000:10_000], 0.3, 2.0, 0.5)
    so, to = other.get_scores(queries[:8]), other.top_k(queries[:8], 100)
    vo = vocab(other)
    remove(a, range(100, 2100))
    compact(a)
    during = tok.encode_packed(t, o, max_len=64)
    assert same_bits(other.get_scores(queries[:8]), so) and same_topk(other.top_k(queries[:8], 100), to)
    remove(a, [0])
    assert vocab(a) == py_vocab(docs[1:100] + docs[2100:5000])
    compact(a)
    ref = model("BM25", docs[1:100] + docs[2100:5000], 0.75, 1.2)
    assert same_topk(a.top_k(queries, 1000), ref.top_k(queries, 1000))
    assert same_bits(a.get_scores(queries[:8]), ref.get_scores(queries[:8]))
    assert same_bits(other.get_scores(queries[:8]), so) and same_topk(other.top_k(queries[:8], 100), to) and vocab(other) == vo
    del a, other, ref
    after = tok.encode_packed(t, o, max_len=64)
    for r in (during, after):
        for k in ("input_ids", "attention_mask"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(before[k]))
