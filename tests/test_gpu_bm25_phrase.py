"""GPU: the positional BM25 index (BM25(..., positions=True), gz_bm25_build_ex / _flags / _sequence) and the phrase search on it
(BM25.search / count_matches with phrase=, gz_bm25_search_phrase[_device], gz_bm25_match_count_phrase; csrc/gz_search.inc,
gz_bm25_sr_phrase_kernel).  The oracle is plain Python, here: S = get_scores(queries), pinned elsewhere; document d matches query q
iff it matches under `match` and `exclude` as search() defines it AND P = phrase[q].split() is empty or
documents[d].split()[i:i+len(P)] == P for some i; row q = [i for i in np.argsort(-S[q], kind="stable") if matched[q, i]][:k'], -1 /
the NaN 0x7FF8000000000000 behind it.  ids are compared with ==, scores as uint64 bit patterns, counts with ==; no tolerance
appears anywhere."""
import warnings

import numpy as np
import pytest

import bm25_restate as R
from bm25_oracles import decoded
from genz_tokenize import _native
from genz_tokenize._packing import pack
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

PAD = np.uint64(0x7FF8000000000000)
MODES = ("any", "all")
CLASSES = ("BM25", "BM25Plus")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model(cls, docs, positions=True, ctx=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (np.mean of no fieldLens)
        return BM25Plus(docs, 0.3, 2.0, 0.5, ctx=ctx, positions=positions) if cls == "BM25Plus" else BM25(docs, ctx=ctx, positions=positions)


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def holds_phrase(words, P):
    return not P or any(words[i:i + len(P)] == P for i in range(len(words) - len(P) + 1))


def matched(docs, queries, match="any", exclude=None, phrase=None):
    split = [d.split() for d in docs]
    sets = [set(w) for w in split]
    m = np.zeros((len(queries), len(docs)), dtype=bool)
    for q, text in enumerate(queries):
        need = set(text.split())
        X = set(exclude[q].split()) if exclude is not None else set()
        P = phrase[q].split() if phrase is not None else []
        for d, W in enumerate(sets):
            ok = bool(need & W) if match == "any" else bool(need) and need <= W
            m[q, d] = ok and not (X & W) and holds_phrase(split[d], P)
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
    assert np.array_equal(cnt, want_cnt), (what, cnt.tolist(), want_cnt.tolist())
    assert np.array_equal(ids, want_ids), what
    assert np.array_equal(bits(sc), want_sc), what


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def check_model(m, docs, queries, phrases, ks, excludes=(None,), modes=MODES, what=""):
    """every mode x every exclude x every k against the oracle, search and count_matches"""
    S = m.get_scores(queries)
    for mode in modes:
        for e, ex in enumerate(excludes):
            mt = matched(docs, queries, mode, ex, phrases)
            for k in ks:
                check(m.search(queries, k, match=mode, exclude=ex, phrase=phrases), S, mt, k, (what, mode, e, k))
            assert np.array_equal(m.count_matches(queries, match=mode, exclude=ex, phrase=phrases), mt.sum(axis=1)), (what, mode, e)


# ---- 1: a random small corpus --------------------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "c", "d", "e"]
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129]


def random_docs(seed, n=131):
    r = np.random.default_rng(seed)
    p = [0.4, 0.3, 0.15, 0.1, 0.05]
    lens = LENGTHS + [int(x) for x in r.integers(0, 12, n - len(LENGTHS))]
    r.shuffle(lens)
    return [" ".join(ALPHABET[int(i)] for i in r.choice(5, size=k, p=p)) for k in lens]


QUERIES = ["a", "e d", "a b c", "c", "b b a", "e", "", "d c a e", "a b", "d"]
PHRASES = ["a", "e d", "a a b", "c c", "b a b a c", "e e", "a b", "", "a b c d e", "nowhere d"]
EXCLUDE = ["", "c", "e", "", "d", "zzz", "a", "", "e d", ""]


@pytest.fixture(scope="module")
def small():
    return random_docs(1)


@pytest.mark.parametrize("cls", CLASSES)
def test_random_small_corpus(small, cls):
    docs = small
    assert len(docs) % 64 and sorted(set(len(d.split()) for d in docs) & set(LENGTHS)) == LENGTHS
    m = model(cls, docs)
    assert m._ctx.bm25_flags(m._index) == _native.GZ_BM25_POSITIONS
    assert decoded(m, compacted=True) == [d.split() for d in docs]
    # (the corpus is worth the test: phrases of 2, 3 and 5 words occur, and not everywhere)
    mt = matched(docs, QUERIES, "any", None, PHRASES)
    assert all(0 < mt[q].sum() < len(docs) for q in (1, 2, 4)), mt.sum(axis=1).tolist()
    check_model(m, docs, QUERIES, PHRASES, (1, 10, len(docs)), (None, EXCLUDE), what=cls)


# ---- 2: boundaries, built by hand ------------------------------------------------------------------------------------------------------
def boundary_docs():
    f = ["f"] * 200
    long_doc = ["g"] * 4995 + ["y", "x", "y"]                            # 4998 words: its only "x y" ends it, in the last trip of 64 (from 4992)
    docs = [
        "x y p q r",                         # 0: the phrase at the very start
        "p q r x y",                         # 1: ... at the very end
        "x y",                               # 2: a document that is exactly the phrase
        "x",                                 # 3: shorter than the phrase
        "",                                  # 4
        "p q x",                             # 5: ends in x ...
        "y p q",                             # 6: ... and the next begins with y: no match across the two
        "p x",                               # 7: the same with empty documents between
        "",                                  # 8
        "",                                  # 9
        "y p",                               # 10
        " ".join(f[:62] + ["x", "y", "z", "w"] + f[:60]),       # 11: the phrase over positions 62 .. 65
        " ".join(f[:63] + ["x", "y"] + f[:3]),                  # 12: x at 63, y at 64: the pair straddles two trips
        " ".join(f[:64] + ["x", "y"]),                          # 13: x at 64
        " ".join(long_doc),                  # 14
        "y x y x",                           # 15: "x y" in the middle only
        "y x",                               # 16: both words, never in this order
        "x x y",                             # 17
        "q y",                               # 18
        "y q x",                             # 19: the LAST document ends in x: the end of seq
    ]
    return docs


B_PHRASES = ["x y", "x y z w", "y z", "z w", "f x", "w f", "x x y", "y x y", "p q x y", "x"]


@pytest.mark.parametrize("cls", CLASSES)
def test_boundaries(cls):
    docs = boundary_docs()
    m = model(cls, docs)
    assert decoded(m, compacted=True) == [d.split() for d in docs]
    queries = list(B_PHRASES)                                            # (the phrase's own words: "any" marks every document with one of them)
    mt = matched(docs, queries, "any", None, B_PHRASES)
    assert np.flatnonzero(mt[0]).tolist() == [0, 1, 2, 11, 12, 13, 14, 15, 17]             # "x y": neither 5|6, 7|10 nor the last document
    assert np.flatnonzero(mt[1]).tolist() == [11] and np.flatnonzero(mt[2]).tolist() == [11] and np.flatnonzero(mt[3]).tolist() == [11]
    assert np.flatnonzero(mt[6]).tolist() == [17] and np.flatnonzero(mt[7]).tolist() == [14, 15] and not mt[8].any()
    check_model(m, docs, queries, B_PHRASES, (1, 10, len(docs)), (None, ["q"] * len(queries)), what=cls)
    # a phrase whose words are not in the query, and a query that is broader than the phrase
    queries2 = ["p q", "f g", "x", "y", "q", "g", "y x", "x y", "r", "p q r x y f g z w"]
    check_model(m, docs, queries2, B_PHRASES, (3, len(docs)), what=(cls, "other queries"))


# ---- 3: equivalences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_equivalences(small, cls):
    docs = small
    m, plain = model(cls, docs), model(cls, docs, positions=False)
    nq = len(QUERIES)
    for mode in MODES:
        for ex in (None, EXCLUDE):
            for k in (1, 10, len(docs)):
                today = plain.search(QUERIES, k, match=mode, exclude=ex)
                assert same(m.search(QUERIES, k, match=mode, exclude=ex), today), (mode, k)
                assert same(m.search(QUERIES, k, match=mode, exclude=ex, phrase=None), today), (mode, k)
                assert same(m.search(QUERIES, k, match=mode, exclude=ex, phrase=[""] * nq), today), (mode, k)
            assert np.array_equal(m.count_matches(QUERIES, match=mode, exclude=ex, phrase=[""] * nq), plain.count_matches(QUERIES, match=mode, exclude=ex))
    # a one-word phrase: "must hold this word"
    for w in ALPHABET + ["nowhere"]:
        with_word = [(q + " " + w).strip() for q in QUERIES]
        want = m.count_matches(with_word, match="all")
        want[[i for i, q in enumerate(QUERIES) if not q.split()]] = 0      # (a query without words matches nothing)
        assert np.array_equal(m.count_matches(QUERIES, match="all", phrase=[w] * nq), want), w
    # a phrase with a word that no document holds
    ids, sc, cnt = m.search(QUERIES, 7, phrase=["a nowhere"] * nq)
    assert not cnt.any() and (ids == -1).all() and (bits(sc) == PAD).all() and ids.shape == (nq, 7)
    ids, sc, cnt = m.search(QUERIES, 7, match="all", phrase=["nowhere"] * nq)
    assert not cnt.any() and (ids == -1).all() and (bits(sc) == PAD).all()
    # the limit: 64 words are a phrase, 65 are not
    long64 = " ".join(["a"] * 64)
    docs2 = docs + [long64 + " b", " ".join(["a"] * 63)]
    m2 = model(cls, docs2)
    got = m2.search(["a"], 5, phrase=[long64])
    check(got, m2.get_scores(["a"]), matched(docs2, ["a"], "any", None, [long64]), 5)
    assert got[2].tolist() == [int(sum(holds_phrase(d.split(), ["a"] * 64) for d in docs2))] and got[2][0] >= 1
    for call in (lambda p: m2.search(["a"], 5, phrase=[p]), lambda p: m2.count_matches(["a"], phrase=[p])):
        with pytest.raises(_native.GzError) as e:
            call(long64 + " a")
        assert e.value.code == _native.GZ_E_LIMIT
    assert same(m2.search(["a"], 5, phrase=[long64]), got)               # (the refused call left everything as it was)
    # an index without positions
    with pytest.raises(ValueError):
        plain.search(QUERIES, 3, phrase=[""] * nq)
    with pytest.raises(ValueError):
        plain.term_sequences()
    _, terms, idf, qoff = plain._queries(QUERIES)
    zero = np.zeros(nq + 1, np.int64)
    for call in (lambda: plain._ctx.bm25_search(plain._index, terms, idf, qoff, plain._params(), cls == "BM25Plus", 3, ph_terms=None, ph_off=zero),
                 lambda: plain._ctx.bm25_match_count(plain._index, terms, qoff, ph_terms=None, ph_off=zero),
                 lambda: plain._ctx.bm25_sequence(plain._index)):
        with pytest.raises(_native.GzError) as e:
            call()
        assert e.value.code == _native.GZ_E_INVALID
    assert plain._ctx.bm25_flags(plain._index) == 0
    # flag bits that do not exist
    buf, off = pack(docs)
    h = _native.C.c_void_p()
    lib = m._ctx.lib
    for flags in (2, 3, -1):
        assert lib.gz_bm25_build_ex(m._ctx.handle, _native._ptr(buf), _native._ptr(off), len(docs), flags, _native.C.byref(h)) == _native.GZ_E_INVALID
        assert not h.value


# ---- 4: the live index -------------------------------------------------------------------------------------------------------------------
L_QUERIES = ["x y", "a b", "x", "c a", "y", "k l m", "a", "e"]
L_PHRASES = ["x y", "a b", "x y", "c a b", "y a", "k l m", "", "e e"]


def check_live(m, texts, cls, what, compacted=False):
    assert m._texts == texts
    assert decoded(m, compacted) == [t.split() for t in texts], what
    fresh = model(cls, texts)
    for mode in MODES:
        for k in (1, 10):
            assert same(m.search(L_QUERIES, k, match=mode, phrase=L_PHRASES), fresh.search(L_QUERIES, k, match=mode, phrase=L_PHRASES)), (what, mode, k)
    check_model(m, texts, L_QUERIES, L_PHRASES, (len(texts),), what=what)
    return fresh


@pytest.mark.parametrize("cls", CLASSES)
def test_live_index(cls):
    base = random_docs(4, 70)
    base[0] = "x y first"                                                 # removed later: the first document, holding a phrase
    base[33] = "c c a b k l m"                                            # removed later: the middle one, the only "k l m"
    base[-1] = "a b tail x"                                               # the last document ENDS in x ...
    more = ["y a starts the batch", "", "inside x y the batch", "e e e", "k l"]      # ... and the batch BEGINS with y
    texts = list(base)
    m = model(cls, texts)
    check_live(m, texts, cls, "built", compacted=True)
    m.add_documents(more)
    texts += more
    check_live(m, texts, cls, "appended")
    mt = matched(texts, ["x y"], "any", None, ["x y"])[0]
    assert not mt[len(base) - 1] and not mt[len(base)] and mt[len(base) + 2] and mt[0]     # not across the boundary; inside the batch
    gone = [0, 33, len(texts) - 1]                                        # first, middle (the phrase's only document), last
    assert m.count_matches(["k"], phrase=["k l m"]).tolist() == [1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.remove_documents(gone)
    texts = [t for i, t in enumerate(texts) if i not in gone]
    check_live(m, texts, cls, "removed")
    assert m.count_matches(["k"], phrase=["k l m"]).tolist() == [0]
    again = ["m k l m x", "tail ends in k", "l m", " ".join(["b"] * 300 + ["x", "y"])]
    m.add_documents(again)
    texts += again
    check_live(m, texts, cls, "appended again")
    assert m.count_matches(["k"], phrase=["k l m"]).tolist() == [1]       # (inside "m k l m x", not across "... k" | "l m")
    m.compact()
    fresh = check_live(m, texts, cls, "compacted", compacted=True)
    a, b = m.term_sequences(), fresh.term_sequences()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert m.vocabulary()[0] == fresh.vocabulary()[0]
    assert m.footprint() == fresh.footprint()                             # (both have been searched: postings and word offsets exist)
    # the index goes on living after the compaction
    m.add_documents(["x y again"])
    texts.append("x y again")
    check_live(m, texts, cls, "appended after the compaction")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.remove_documents(range(len(texts)))
    assert m.term_sequences()[0].shape == (0,) and m.term_sequences()[1].tolist() == [0]
    assert m.count_matches(L_QUERIES, phrase=L_PHRASES).tolist() == [0] * len(L_QUERIES)


def test_compacted_footprint_equals_fresh_build():
    """After compact(), footprint() equals the fresh positions=True build's exactly, all three numbers.  A positional build ends in
    the compacted form -- its text copy is the live terms' bytes, as after gz_bm25_compact -- so the two are the same index.  The
    documents carry 20 000 bytes of blanks: a text copy that kept them would show in text_bytes and, across the allocator's granule,
    in device_bytes."""
    base = random_docs(4, 70)
    more = ["x y", "k" + " " * 12000 + "l m", "", "a b" + "\t" * 8000]
    m = model("BM25", base)
    m.add_documents(more)
    m.remove_documents([0, 33])
    texts = [t for i, t in enumerate(base + more) if i not in (0, 33)]
    assert m.footprint()["text_bytes"] > 20000
    m.compact()
    fresh = model("BM25", texts)
    a, b = m.term_sequences(), fresh.term_sequences()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    print("compacted:", m.footprint(), "fresh:", fresh.footprint())
    assert m.footprint() == fresh.footprint()
    assert fresh.footprint()["text_bytes"] == sum(len(w.encode()) for w in fresh.vocabulary()[0])
    plain = model("BM25", texts, positions=False)                         # (a build without positions keeps the whole text, as ever)
    assert plain.footprint()["text_bytes"] == int(pack(texts)[1][-1]) > 20000


# ---- 5: an index without positions is the index it was ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_non_positional_indexes_are_untouched(small, cls):
    docs = small
    default, off_, on = model(cls, docs, positions=False), None, model(cls, docs)
    off_ = BM25Plus(docs, 0.3, 2.0, 0.5) if cls == "BM25Plus" else BM25(docs)          # (the keyword never mentioned)
    assert default.footprint() == off_.footprint()
    assert on.footprint()["device_bytes"] > off_.footprint()["device_bytes"]
    assert on.footprint()["table_terms"] == off_.footprint()["table_terms"]
    assert off_.footprint()["text_bytes"] == int(pack(docs)[1][-1])       # (the whole text, as ever; a positional build keeps the terms' bytes)
    assert np.array_equal(bits(on.get_scores(QUERIES)), bits(off_.get_scores(QUERIES)))
    for a in (default, on):
        assert same(a.top_k(QUERIES, 9) + (0,), off_.top_k(QUERIES, 9) + (0,))
        for mode in MODES:
            for ex in (None, EXCLUDE):
                assert same(a.search(QUERIES, 9, match=mode, exclude=ex), off_.search(QUERIES, 9, match=mode, exclude=ex)), mode
                assert np.array_equal(a.count_matches(QUERIES, match=mode, exclude=ex), off_.count_matches(QUERIES, match=mode, exclude=ex))
    assert default.footprint() == off_.footprint()                        # (both hold their postings now)
    # a phrase search derives the word offsets: they are counted while they exist
    before = on.footprint()["device_bytes"]
    on.count_matches(QUERIES, phrase=PHRASES)
    assert on.footprint()["device_bytes"] > before


# ---- 6: forced hash collisions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_bits", [1, 3])
def test_forced_hash_collisions(small, hash_bits):
    docs = small[:60] + boundary_docs()
    queries = B_PHRASES + QUERIES
    phrases = B_PHRASES + PHRASES
    ctx = _native.Context()
    try:
        _native.debug_set("bm25_hash_bits", hash_bits, ctx)
        m = model("BM25", docs, ctx=ctx)
        assert decoded(m, compacted=True) == [d.split() for d in docs]
        check_model(m, docs, queries, phrases, (10,), what=hash_bits)
        more = ["x y z", "w f x y", "nowhere d"]
        m.add_documents(more)
        docs = docs + more
        m.remove_documents([2, 61])
        docs = [d for i, d in enumerate(docs) if i not in (2, 61)]
        assert decoded(m) == [d.split() for d in docs]
        check_model(m, docs, queries, phrases, (10,), what=(hash_bits, "changed"))
        m.compact()
        assert decoded(m, compacted=True) == [d.split() for d in docs]
        check_model(m, docs, queries, phrases, (10,), what=(hash_bits, "compacted"))
        del m
    finally:
        _native.debug_set("bm25_hash_bits", 0, ctx)
        ctx.close()
    _native.debug_set("bm25_hash_bits", 0)


# ---- 7: failing allocations ----------------------------------------------------------------------------------------------------------------
def c_state(ctx, index, queries, phrases):
    """what the C face answers: info, flags, the positional store, a phrase search and a phrase count (term ids looked up now)"""
    def ids_of(texts):
        words = [w for t in texts for w in t.split()]
        off = np.array([0] + list(np.cumsum([len(t.split()) for t in texts])), np.int64)
        b, o = pack(words)
        t, df = ctx.bm25_lookup(index, b, o) if words else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        return t, df, off
    terms, qdf, qoff = ids_of(queries)
    pterms, _, poff = ids_of(phrases)
    n = ctx.bm25_info(index)[0]
    idf = np.array([R.idf(n, int(x)) for x in qdf])
    lens = ctx.bm25_field_lengths(index)
    params = [2.2, 1.2, 0.25, 0.75, float(np.mean(lens)) if n else float("nan"), 0.0]
    seq = ctx.bm25_sequence(index)
    got = ctx.bm25_search(index, terms, idf, qoff, params, False, 6, mode=1, ph_terms=pterms, ph_off=poff)
    cnt = ctx.bm25_match_count(index, terms, qoff, ph_terms=pterms, ph_off=poff)
    return (ctx.bm25_info(index), ctx.bm25_flags(index), seq[0].tolist(), seq[1].tolist(), got[0].tolist(), bits(got[1]).tolist(),
            got[2].tolist(), cnt.tolist())


def sweep(ctx, index, call, queries, phrases):
    """call() under inject_bad_alloc = 1, 2, ...: every GZ_E_NOMEM leaves the state as it was; returns the states before and after
    the first success"""
    before = c_state(ctx, index, queries, phrases)
    ok = None
    for k in range(1, 200):
        _native.debug_set("inject_bad_alloc", k, ctx)
        try:
            call()
        except _native.GzError as e:
            _native.debug_set("inject_bad_alloc", 0, ctx)
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            assert c_state(ctx, index, queries, phrases) == before, k
            continue
        ok = k
        break
    _native.debug_set("inject_bad_alloc", 0, ctx)
    assert ok is not None and ok > 3, ok
    return before, c_state(ctx, index, queries, phrases)


def words_state(ctx, index, texts):
    """the positional store as words, through a lookup of the current words"""
    words = sorted({w for t in texts for w in t.split()})
    b, o = pack(words)
    name = dict(zip(ctx.bm25_lookup(index, b, o)[0].tolist(), words))
    t, off = ctx.bm25_sequence(index)
    t, off = t.tolist(), off.tolist()
    return [[name[x] for x in t[off[d]:off[d + 1]]] for d in range(len(off) - 1)]


def test_allocation_failure_sweep():
    base = random_docs(7, 90) + boundary_docs()[:14]
    more = ["y x y", "k l m x y", ""] + random_docs(8, 40)
    gone = np.array([0, 5, 50, len(base) + 1], np.int64)
    queries, phrases = L_QUERIES + ["x y z w"], L_PHRASES + ["x y z w"]
    ctx = _native.Context()
    buf, off = pack(base)
    index = ctx.bm25_build(buf, off, positions=True)
    texts = list(base)

    def fresh_state(texts):
        b, o = pack(texts)
        h = ctx.bm25_build(b, o, positions=True)
        try:
            out = [c_state(ctx, h, queries, phrases), words_state(ctx, h, texts)]
            ctx.bm25_compact(h)                                          # (the footprint a compaction must arrive at: the text copy
            c_state(ctx, h, queries, phrases)                            # shrinks to the terms' bytes, the derived arrays exist again)
            return out + [ctx.bm25_footprint(h)]
        finally:
            ctx.bm25_destroy(h)

    mb, mo = pack(more)
    before, after = sweep(ctx, index, lambda: ctx.bm25_append(index, mb, mo), queries, phrases)
    texts += more
    want = fresh_state(texts)
    # (term ids may differ from the fresh build's until the compaction: the store is compared as words, the answers as they are)
    assert after != before and after[0] == want[0][0] and after[3:] == want[0][3:] and words_state(ctx, index, texts) == want[1]
    before, after = sweep(ctx, index, lambda: ctx.bm25_remove(index, gone), queries, phrases)
    texts = [t for i, t in enumerate(texts) if i not in set(gone.tolist())]
    want = fresh_state(texts)
    assert after != before and after[0] == want[0][0] and after[3:] == want[0][3:] and words_state(ctx, index, texts) == want[1]
    before, after = sweep(ctx, index, lambda: ctx.bm25_compact(index), queries, phrases)
    assert after == want[0]                                              # now the term ids too
    assert ctx.bm25_footprint(index) == want[2]
    # the search itself: a failing allocation of a phrase search leaves the index answering
    state = c_state(ctx, index, queries, phrases)
    ctx.bm25_remove(index, np.array([1], np.int64))                      # (drops the derived arrays: the next search builds them)
    texts = texts[:1] + texts[2:]
    want = fresh_state(texts)
    failures = 0
    for k in range(1, 200):
        _native.debug_set("inject_bad_alloc", k, ctx)
        try:
            got = c_state(ctx, index, queries, phrases)
        except _native.GzError as e:
            _native.debug_set("inject_bad_alloc", 0, ctx)
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            failures += 1
            continue
        break
    _native.debug_set("inject_bad_alloc", 0, ctx)
    assert failures > 3 and got[0] == want[0][0] and got[3:] == want[0][3:] and got != state
    ctx.bm25_destroy(index)
    ctx.close()


# ---- 8: the device form, and a device build ----------------------------------------------------------------------------------------------
def test_device_forms(small):
    docs = small + boundary_docs()
    queries, phrases = QUERIES + B_PHRASES, PHRASES + B_PHRASES
    ctx = _native.Context()
    m = BM25(docs, ctx=ctx, positions=True)
    buf, off = pack(docs)
    pad = 3
    dt, do = ctx.alloc(len(buf) + pad), ctx.alloc(8 * len(off))
    ctx.h2d(dt, np.concatenate([np.full(pad, 32, np.uint8), buf]))
    ctx.h2d(do, off + pad)
    idv = ctx.bm25_build_device(dt, do, len(docs), int(off[-1]), positions=True)
    ctx.free(dt)
    ctx.free(do)
    assert ctx.bm25_flags(idv) == 1 and ctx.bm25_footprint(idv) == ctx.bm25_footprint(m._index)
    a, b = ctx.bm25_sequence(idv), m.term_sequences()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    nq, terms, idf, qoff = m._queries(queries)
    pt, po = m._exclusions(phrases, nq)
    P = m._params()
    S = m.get_scores(queries)
    g = 256
    for mode, k in ((0, 4), (1, 50)):
        mt = matched(docs, queries, MODES[mode], None, phrases)
        host = ctx.bm25_search(m._index, terms, idf, qoff, P, False, k, mode=mode, ph_terms=pt, ph_off=po)
        check(host, S, mt, k, (mode, k))
        assert same(ctx.bm25_search(idv, terms, idf, qoff, P, False, k, mode=mode, ph_terms=pt, ph_off=po), host)
        sizes = (nq * k * 8, nq * k * 8, nq * 8)
        dev = [ctx.alloc(nb + 2 * g) for nb in sizes]
        for d, nb in zip(dev, sizes):
            ctx.h2d(d, np.full(nb + 2 * g, 0xA5, np.uint8))
        ctx.bm25_search(idv, terms, idf, qoff, P, False, k, d_ids=dev[0] + g, d_scores=dev[1] + g, d_counts=dev[2] + g, mode=mode,
                        ph_terms=pt, ph_off=po)
        ctx.sync()
        raw = []
        for d, nb in zip(dev, sizes):
            x = np.empty(nb + 2 * g, np.uint8)
            ctx.d2h(x, d)
            assert np.all(x[:g] == 0xA5) and np.all(x[g + nb:] == 0xA5)
            raw.append(x[g:g + nb])
            ctx.free(d)
        assert np.array_equal(raw[0].view(np.int64).reshape(nq, k), host[0])
        assert np.array_equal(raw[1].view(np.uint64).reshape(nq, k), bits(host[1]))
        assert np.array_equal(raw[2].view(np.int64), host[2])
    del m
    ctx.bm25_destroy(idv)
    ctx.close()


# ---- 9: many bitmap words, rows in several chunks ----------------------------------------------------------------------------------------
def test_many_documents_and_chunks():
    """3 000 documents (47 bitmap words: more than one workgroup of the phrase kernel) and a search chunk of one row's bitmap, so
    that every query is a chunk of its own and the phrase offsets of a later chunk are the absolute ones"""
    docs = random_docs(11, 3000)
    docs[2999] = "e e d c x y"
    ctx = _native.Context()
    try:
        _native.debug_set("bm25_search_chunk", 47, ctx)
        m = BM25(docs, ctx=ctx, positions=True)
        queries = ["x", "e d", "", "a b c", "y e"]
        phrases = ["x y", "e d", "a", "", "e e d c x y"]
        check_model(m, docs, queries, phrases, (1, 20), (None, ["", "b", "", "e", ""]), what="chunks")
        del m
    finally:
        ctx.close()
