"""GPU: proximity search and smallest covering spans on the positional BM25 index (BM25.search_near / count_near / cover,
gz_bm25_search_near[_device], gz_bm25_match_count_near, gz_bm25_cover[_device]; csrc/gz_near.inc).  The oracle is plain Python, here,
over the documents' text.  With W = documents[d].split(): document d matches query q iff it matches under match / exclude / phrase
as search() defines it AND holds_near(W, near[q].split(), window[q]); row q = [i for i in np.argsort(-S[q], kind="stable") if
matched[q, i]][:k'], -1 / the NaN 0x7FF8000000000000 behind it.  cover(W, Q) = (start, length, words) of the smallest (length,
start) among the windows that hold every word of set(Q) & set(W).  ids, counts and covers are compared with ==, scores as uint64
bit patterns; no tolerance appears anywhere."""
import warnings

import numpy as np
import pytest

from genz_tokenize import _native
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


def holds_near(W, P, w):
    S = set(P)
    return not S or any(S <= set(W[i:i + w]) for i in range(max(1, len(W) - w + 1)))


def o_cover(W, Q):
    """(start, length, words): the smallest (length, start) over the windows of W that hold every word of set(Q) & set(W) -- two
    pointers over the counts of the words inside the window"""
    R = set(Q) & set(W)
    if not R:
        return (0, 0, 0)
    inside, have, best, i = {}, 0, None, 0
    for j, x in enumerate(W):
        if x in R:
            inside[x] = inside.get(x, 0) + 1
            have += inside[x] == 1
        while have == len(R):                                            # W[i:j + 1] holds R: the shortest window that starts at i
            if best is None or (j + 1 - i, i) < best:
                best = (j + 1 - i, i)
            if W[i] in R:
                inside[W[i]] -= 1
                have -= inside[W[i]] == 0
            i += 1
    return (best[1], best[0], len(R))


_near_cache = {}


def near_of(text, words, near, w):
    key = (text, near, w)
    if key not in _near_cache:
        _near_cache[key] = holds_near(words, near.split(), w)
    return _near_cache[key]


def matched(docs, queries, match="any", exclude=None, phrase=None, near=None, windows=None):
    split = [d.split() for d in docs]
    sets = [set(w) for w in split]
    m = np.zeros((len(queries), len(docs)), dtype=bool)
    for q, text in enumerate(queries):
        need = set(text.split())
        X = set(exclude[q].split()) if exclude is not None else set()
        P = phrase[q].split() if phrase is not None else []
        for d, W in enumerate(sets):
            ok = bool(need & W) if match == "any" else bool(need) and need <= W
            ok = ok and not (X & W) and holds_phrase(split[d], P)
            m[q, d] = ok and (near is None or near_of(docs[d], split[d], near[q], windows[q]))
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


def check_near(m, docs, queries, near, window, ks, excludes=(None,), phrases=(None,), modes=MODES, what=""):
    """every mode x every exclude x every phrase x every k against the oracle, search_near and count_near"""
    S = m.get_scores(queries)
    windows = [window] * len(queries) if isinstance(window, int) else list(window)
    for mode in modes:
        for e, ex in enumerate(excludes):
            for p, ph in enumerate(phrases):
                mt = matched(docs, queries, mode, ex, ph, near, windows)
                for k in ks:
                    check(m.search_near(queries, k, near, window, match=mode, exclude=ex, phrase=ph), S, mt, k, (what, mode, e, p, k))
                cnt = m.count_near(queries, near, window, match=mode, exclude=ex, phrase=ph)
                assert cnt.dtype == np.int64 and np.array_equal(cnt, mt.sum(axis=1)), (what, mode, e, p)


def all_ids(nq, n, extra=()):
    return np.tile(np.array(list(range(n)) + list(extra), dtype=np.int64), (nq, 1))


def want_cover(docs, queries, ids):
    ids = np.asarray(ids)
    out = np.empty((3,) + ids.shape, dtype=np.int32)
    split = [d.split() for d in docs]
    for q, row in enumerate(ids.tolist()):
        Q = queries[q].split()
        for j, d in enumerate(row):
            out[:, q, j] = (-1, 0, 0) if d < 0 else o_cover(split[d], Q)
    return out


def check_cover(m, docs, queries, ids, what=""):
    got = m.cover(queries, ids)
    want = want_cover(docs, queries, ids)
    assert len(got) == 3
    for g, w, name in zip(got, want, ("starts", "lengths", "words")):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())
    return got


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
NEARS = ["e d", "a b c", "d c a e", "d c a e", "e e d", "a b c d e", "a b c d e", "", "nowhere d", "b a"]
WINDOWS = [2, 3, 4, 6, 2, 5, 9, 3, 50, 1]


@pytest.fixture(scope="module")
def small():
    return random_docs(1)


def test_the_corpus_is_worth_the_test(small):
    docs = small
    assert len(docs) == 131 and sorted(set(len(d.split()) for d in docs) & set(LENGTHS)) == LENGTHS
    n = [sum(holds_near(d.split(), near.split(), w) for d in docs) for near, w in zip(NEARS[:7], WINDOWS[:7])]
    print("documents that hold the near sets:", n)
    assert all(0 < x < 131 for x in n), n


@pytest.mark.parametrize("cls", CLASSES)
def test_random_small_corpus(small, cls):
    docs = small
    m = model(cls, docs)
    ks = (1, 10, len(docs))
    check_near(m, docs, QUERIES, NEARS, WINDOWS, ks, (None, EXCLUDE), (None, PHRASES), what=(cls, "windows"))
    check_near(m, docs, QUERIES, NEARS, 4, ks, (None, EXCLUDE), (None, PHRASES), what=(cls, "scalar"))
    # near words that are not in the query at all, and numpy integers for the windows
    rolled = NEARS[3:] + NEARS[:3]
    check_near(m, docs, QUERIES, rolled, np.array(WINDOWS[3:] + WINDOWS[:3]), (7,), what=(cls, "rolled"))


def test_cover_random_small_corpus(small):
    docs = small
    m = model("BM25Plus", docs)
    queries = QUERIES + ["e d c b a", "nowhere d e", "e e d", "zzz"]
    ids, _ = m.top_k(queries, len(docs))                                 # (every document appears, those without any query word too)
    assert sorted(ids[0].tolist()) == list(range(len(docs)))
    got = check_cover(m, docs, queries, ids, "top_k ids")
    assert (got[2] == 0).any() and (got[2] == 5).any()


# ---- 2: boundaries, built by hand ------------------------------------------------------------------------------------------------------
def boundary_docs():
    f = ["f"] * 300
    return [
        "x y p q r",                                                     # 0
        "p q r y x",                                                     # 1
        "x p y",                                                         # 2
        "x",                                                             # 3
        "",                                                              # 4
        "p q x",                                                         # 5: ends in x ...
        "y p q",                                                         # 6: ... and the next begins with y
        "p x",                                                           # 7: the same with empty documents between
        "",                                                              # 8
        "",                                                              # 9
        "y p",                                                           # 10
        " ".join(f[:63] + ["x", "y"] + f[:3]),                           # 11: x at 63, y at 64: the pair straddles two trips
        " ".join(f[:62] + ["x", "f", "f", "y"] + f[:60]),                # 12
        " ".join(["x"] + f[:3] + ["x"] + f[:195] + ["y"]),               # 13: x at 0 and 4, y at 200
        " ".join(["g"] * 4995 + ["y", "g", "x"]),                        # 14
        "x a x x y",                                                     # 15
        "y q x",                                                         # 16: the last document: the end of seq
    ]


B_MATCH = {1: [], 2: [0, 1, 11, 15], 3: [0, 1, 2, 11, 14, 15, 16], 4: [0, 1, 2, 11, 12, 14, 15, 16], 196: [0, 1, 2, 11, 12, 14, 15, 16],
           197: [0, 1, 2, 11, 12, 13, 14, 15, 16], 198: [0, 1, 2, 11, 12, 13, 14, 15, 16], 2 ** 40: [0, 1, 2, 11, 12, 13, 14, 15, 16]}
B_COVER = {0: (0, 2, 2), 1: (3, 2, 2), 2: (0, 3, 2), 3: (0, 1, 1), 4: (0, 0, 0), 5: (2, 1, 1), 11: (63, 2, 2), 12: (62, 4, 2),
           13: (4, 197, 2), 14: (4995, 3, 2), 15: (3, 2, 2), 16: (0, 3, 2), -1: (-1, 0, 0)}


@pytest.mark.parametrize("cls", CLASSES)
def test_boundaries(cls):
    docs = boundary_docs()
    n = len(docs)
    assert docs[13].split().index("y") == 200 and [i for i, x in enumerate(docs[13].split()) if x == "x"] == [0, 4]
    m = model(cls, docs)
    windows = list(B_MATCH)
    queries, near = ["x y"] * len(windows), ["x y"] * len(windows)
    S = m.get_scores(queries)
    # the table, by hand, and the oracle agree
    mt = matched(docs, queries, "any", None, None, near, windows)
    for q, w in enumerate(windows):
        assert np.flatnonzero(mt[q]).tolist() == B_MATCH[w], w
    got = m.search_near(queries, n, near, windows)
    check(got, S, mt, n, cls)
    for q, w in enumerate(windows):
        assert sorted(got[0][q][:got[2][q]].tolist()) == B_MATCH[w], w
        assert m.count_near(["x y"], ["x y"], w).tolist() == [len(B_MATCH[w])], w
    check_near(m, docs, queries, near, windows, (1, 5), (None, ["q"] * len(windows)), (None, ["x"] * len(windows)), what=cls)
    # queries that are broader or other than the near words
    queries2 = ["p q f g", "x", "y", "g f", "x y p q r f g", "q", "r", "y x"]
    check_near(m, docs, queries2, near, windows, (n,), what=(cls, "other queries"))
    # the covers
    ids = all_ids(1, n, (-1,))
    s, ln, wd = check_cover(m, docs, ["x y zzz x"], ids, cls)
    for d, want in B_COVER.items():
        j = n if d < 0 else d
        assert (int(s[0, j]), int(ln[0, j]), int(wd[0, j])) == want, d
    # the tie rule
    ties = ["a b a b", "a x x b a b", "a x b x a"]
    t = model(cls, ties)
    got = t.cover(["a b", "b a", "a b"], [[0], [1], [2]])
    assert [tuple(int(x[q, 0]) for x in got) for q in range(3)] == [(0, 2, 2), (3, 2, 2), (0, 3, 2)]
    check_cover(t, ties, ["a b", "b a", "a b", "x", "b x a a"], all_ids(5, 3, (-1,)), (cls, "ties"))


# ---- 3: equivalences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_equivalences(small, cls):
    docs = small
    n, nq = len(docs), len(QUERIES)
    m, plain = model(cls, docs), model(cls, docs, positions=False)
    # no near words: search, bit for bit -- also the search of an index without positions
    for mode in MODES:
        for ex in (None, EXCLUDE):
            for k in (1, 10, n):
                today = plain.search(QUERIES, k, match=mode, exclude=ex)
                assert same(m.search_near(QUERIES, k, [""] * nq, 3, match=mode, exclude=ex), today), (mode, k)
                assert same(m.search_near(QUERIES, k, [""] * nq, WINDOWS, match=mode, exclude=ex), m.search(QUERIES, k, match=mode, exclude=ex))
                assert same(m.search_near(QUERIES, k, [""] * nq, 1, match=mode, exclude=ex, phrase=PHRASES),
                            m.search(QUERIES, k, match=mode, exclude=ex, phrase=PHRASES)), (mode, k)
            assert np.array_equal(m.count_near(QUERIES, [""] * nq, 2, match=mode, exclude=ex), plain.count_matches(QUERIES, match=mode, exclude=ex))
    # one near word, window 1: the one-word phrase
    for w in ALPHABET + ["nowhere"]:
        for mode in MODES:
            assert same(m.search_near(QUERIES, 9, [w] * nq, 1, match=mode), m.search(QUERIES, 9, match=mode, phrase=[w] * nq)), (w, mode)
    # two distinct words: window 1 matches nothing, window 2 is the union of the two phrases
    for a, b in (("a", "b"), ("e", "d"), ("c", "e"), ("d", "nowhere")):
        ids, sc, cnt = m.search_near(QUERIES, 5, [a + " " + b] * nq, 1)
        assert not cnt.any() and (ids == -1).all() and (bits(sc) == PAD).all()
        for mode in MODES:
            both = matched(docs, QUERIES, mode, None, [a + " " + b] * nq) | matched(docs, QUERIES, mode, None, [b + " " + a] * nq)
            assert np.array_equal(m.count_near(QUERIES, [b + " " + a + " " + b] * nq, 2, match=mode), both.sum(axis=1)), (a, b, mode)
            check(m.search_near(QUERIES, n, [a + " " + b] * nq, 2, match=mode), m.get_scores(QUERIES), both, n, (a, b, mode))
    # a window of the longest document or more: "holds all of them"
    longest = max(len(d.split()) for d in docs)
    for words in ("e", "d c", "a b c d e", "e e d", "nowhere a"):
        with_words = [(q + " " + words).strip() for q in QUERIES]
        want = m.count_matches(with_words, match="all")
        want[[i for i, q in enumerate(QUERIES) if not q.split()]] = 0      # (a query without words matches nothing)
        for w in (longest, longest + 1, 2 ** 40, 2 ** 62, 2 ** 70):
            assert np.array_equal(m.count_near(QUERIES, [words] * nq, w, match="all"), want), (words, w)
    # near = the query, mode "all": the documents whose cover is complete and no longer than the window
    ids = all_ids(nq, n)
    _, ln, wd = m.cover(QUERIES, ids)
    for w in (1, 2, 3, 4, 5, 8, 13, 64, 200):
        got = m.search_near(QUERIES, n, QUERIES, w, match="all")
        for q, text in enumerate(QUERIES):
            R = set(text.split())
            want = [d for d in range(n) if R and wd[q, d] == len(R) and ln[q, d] <= w]
            assert sorted(got[0][q][:got[2][q]].tolist()) == want, (w, q)
            assert got[2][q] == len(want)
    # a near word that no document holds
    for mode in MODES:
        ids7, sc, cnt = m.search_near(QUERIES, 7, ["a nowhere"] * nq, 50, match=mode)
        assert not cnt.any() and (ids7 == -1).all() and (bits(sc) == PAD).all() and ids7.shape == (nq, 7)
    assert not m.count_near(QUERIES, ["nowhere"] * nq, 1).any()


@pytest.mark.parametrize("cls", CLASSES)
def test_limit_of_64_distinct_words(small, cls):
    words = ["w%d" % i for i in range(65)]
    r = np.random.default_rng(5)
    full = list(words[:64]) * 2
    r.shuffle(full)
    docs = small + [" ".join(full), " ".join(words[:63] + words[:10]), " ".join(words[:64])]
    n = len(docs)
    m = model(cls, docs)
    near64 = " ".join(words[:64] + words[:5])                            # (repeated words count once: 64 DISTINCT words)
    queries = ["w0 a", "w3"]
    for window in (63, 64, 100, 128):
        check_near(m, docs, queries, [near64] * 2, window, (5,), what=(cls, window))
    assert m.count_near(queries, [near64] * 2, 64).tolist() == [1 + holds_near(full, words[:64], 64)] * 2
    assert m.count_near(queries, [near64] * 2, 63).tolist() == [0, 0]
    ids = all_ids(2, n, (-1,))
    got = check_cover(m, docs, [near64, " ".join(words[1:64]) + " a a"], ids, cls)
    assert got[2][0, n - 3:n].tolist() == [64, 63, 64] and got[1][0, n - 1] == 64
    before = (m.search_near(queries, 5, [near64] * 2, 64), m.cover([near64] * 2, ids))
    near65 = " ".join(words)
    for call in (lambda: m.search_near(queries, 5, [near64, near65], 100), lambda: m.count_near(queries, [near65, ""], 100),
                 lambda: m.cover(["a", near65], ids)):
        with pytest.raises(_native.GzError) as e:
            call()
        assert e.value.code == _native.GZ_E_LIMIT
    after = (m.search_near(queries, 5, [near64] * 2, 64), m.cover([near64] * 2, ids))      # (the refused calls left everything as it was)
    assert same(before[0], after[0]) and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))


def test_context_level(small):
    docs = small
    m, plain = model("BM25", docs), model("BM25", docs, positions=False)
    ctx, nq = m._ctx, len(QUERIES)
    _, terms, idf, qoff = m._queries(QUERIES)
    P = m._params()
    e, d = (int(x) for x in m._lookup(["e", "d"])[0])
    # a near range that repeats a term id is the set
    rep_terms = np.array([e, e, d, e] * nq, np.int32)
    rep_off = np.arange(nq + 1, dtype=np.int64) * 4
    set_terms = np.array([e, d] * nq, np.int32)
    set_off = np.arange(nq + 1, dtype=np.int64) * 2
    for w in (1, 2, 3, 7):
        win = np.full(nq, w, np.int64)
        for mode in (0, 1):
            a = ctx.bm25_search(m._index, terms, idf, qoff, P, False, 9, mode=mode, nr_terms=rep_terms, nr_off=rep_off, nr_window=win)
            b = ctx.bm25_search(m._index, terms, idf, qoff, P, False, 9, mode=mode, nr_terms=set_terms, nr_off=set_off, nr_window=win)
            assert same(a, b) and same(a, m.search_near(QUERIES, 9, ["e d"] * nq, w, match=MODES[mode])), (w, mode)
            assert np.array_equal(ctx.bm25_match_count(m._index, terms, qoff, mode=mode, nr_terms=rep_terms, nr_off=rep_off, nr_window=win), a[2])
    assert a[2].any()
    # -1 in a near range: nothing matches the row; in a cover range it is ignored
    none = ctx.bm25_match_count(m._index, terms, qoff, nr_terms=np.array([e, -1] * nq, np.int32), nr_off=set_off, nr_window=np.full(nq, 99, np.int64))
    assert not none.any()
    ids = all_ids(1, len(docs))
    a = ctx.bm25_cover(m._index, np.array([e, -1, d, e, -1], np.int32), np.array([0, 5], np.int64), ids)
    b = m.cover(["e d"], ids)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # what the C face refuses, and that it goes on answering
    zero = np.zeros(nq + 1, np.int64)
    ok_win = np.ones(nq, np.int64)
    bad = [
        (dict(nr_terms=np.array([m._ctx.bm25_info(m._index)[1]] * nq * 2, np.int32), nr_off=set_off, nr_window=ok_win), _native.GZ_E_INVALID),
        (dict(nr_terms=np.array([-2] * nq * 2, np.int32), nr_off=set_off, nr_window=ok_win), _native.GZ_E_INVALID),
        (dict(nr_terms=set_terms, nr_off=set_off[::-1].copy(), nr_window=ok_win), _native.GZ_E_INVALID),
        (dict(nr_terms=None, nr_off=set_off, nr_window=ok_win), _native.GZ_E_INVALID),
        (dict(nr_terms=set_terms, nr_off=set_off, nr_window=np.zeros(nq, np.int64)), _native.GZ_E_INVALID),
        (dict(nr_terms=np.array([e] * 65, np.int32), nr_off=np.array([0] + [65] * nq, np.int64), nr_window=ok_win), _native.GZ_E_LIMIT),
    ]
    for kw, code in bad:
        for call in (lambda: ctx.bm25_search(m._index, terms, idf, qoff, P, False, 3, **kw), lambda: ctx.bm25_match_count(m._index, terms, qoff, **kw)):
            with pytest.raises(_native.GzError) as err:
                call()
            assert err.value.code == code, kw
    # (a window < 1 in a row WITHOUT near terms is not looked at)
    assert same(ctx.bm25_search(m._index, terms, idf, qoff, P, False, 9, nr_terms=None, nr_off=zero, nr_window=np.zeros(nq, np.int64)),
                m.search(QUERIES, 9))
    for bad_ids in ([[len(docs)]], [[-2]]):
        with pytest.raises(_native.GzError) as err:
            ctx.bm25_cover(m._index, np.array([e], np.int32), np.array([0, 1], np.int64), np.array(bad_ids, np.int64))
        assert err.value.code == _native.GZ_E_INVALID
    after = m.search_near(QUERIES, 9, ["d e"] * nq, 7, match="all")      # (the refused calls left everything as it was)
    assert same(m.search_near(QUERIES, 9, ["e d"] * nq, 7, match="all"), after) and after[2].any()
    # an index without positions
    with pytest.raises(ValueError):
        plain.search_near(QUERIES, 3, [""] * nq, 2)
    with pytest.raises(ValueError):
        plain.count_near(QUERIES, [""] * nq, 2)
    with pytest.raises(ValueError):
        plain.cover(QUERIES, all_ids(nq, 3))
    _, terms, idf, qoff = plain._queries(QUERIES)
    for call in (lambda: plain._ctx.bm25_search(plain._index, terms, idf, qoff, plain._params(), False, 3, nr_terms=None, nr_off=zero, nr_window=ok_win),
                 lambda: plain._ctx.bm25_match_count(plain._index, terms, qoff, nr_terms=None, nr_off=zero, nr_window=ok_win),
                 lambda: plain._ctx.bm25_cover(plain._index, terms, qoff, all_ids(nq, 3))):
        with pytest.raises(_native.GzError) as err:
            call()
        assert err.value.code == _native.GZ_E_INVALID


# ---- 4: the live index -------------------------------------------------------------------------------------------------------------------
L_QUERIES = ["x y", "a b", "x", "c a", "y", "k l m", "a", "e"]
L_NEARS = ["x y", "b a", "y x", "c a b", "a y", "m k l", "", "e e"]
L_WINDOWS = [2, 3, 4, 3, 2, 3, 1, 1]


def live_answers(m):
    n = m.num_doc
    out = []
    for mode in MODES:
        if n:
            out += list(m.search_near(L_QUERIES, 10, L_NEARS, L_WINDOWS, match=mode))
        out.append(m.count_near(L_QUERIES, L_NEARS, L_WINDOWS, match=mode))
    out += list(m.cover(L_QUERIES, all_ids(len(L_QUERIES), n, (-1,))))
    return [bits(a) if a.dtype == np.float64 else a for a in out]


def check_live(m, texts, cls, what):
    assert m._texts == texts
    fresh = model(cls, texts)
    a, b = live_answers(m), live_answers(fresh)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), what
    check_near(m, texts, L_QUERIES, L_NEARS, L_WINDOWS, (len(texts),), what=what)
    check_cover(m, texts, L_QUERIES, all_ids(len(L_QUERIES), len(texts)), what)


@pytest.mark.parametrize("cls", CLASSES)
def test_live_index(cls):
    base = random_docs(4, 70)
    base[0] = "x y first"                                                 # removed later: the first document
    base[33] = "c c a b k l m"                                            # removed later: the middle one, the only "k l m"
    base[-1] = "a b tail x"                                               # the last document ENDS in x ...
    more = ["y a starts the batch", "", "inside y x the batch", "e e e", "k l"]      # ... and the batch BEGINS with y
    texts = list(base)
    m = model(cls, texts)
    check_live(m, texts, cls, "built")
    m.add_documents(more)
    texts += more
    check_live(m, texts, cls, "appended")
    mt = matched(texts, ["x y"], "any", None, None, ["x y"], [2])[0]
    assert not mt[len(base) - 1] and not mt[len(base)] and mt[len(base) + 2] and mt[0]     # not across the boundary; inside the batch
    gone = [0, 33, len(texts) - 1]                                        # first, middle, last
    assert m.count_near(["k"], ["m l k"], 3).tolist() == [1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.remove_documents(gone)
    texts = [t for i, t in enumerate(texts) if i not in gone]
    check_live(m, texts, cls, "removed")
    assert m.count_near(["k"], ["m l k"], 3).tolist() == [0]
    again = ["m k l m x", "tail ends in k", "l m", " ".join(["b"] * 300 + ["y", "x"])]
    m.add_documents(again)
    texts += again
    check_live(m, texts, cls, "appended again")
    assert m.count_near(["k"], ["m l k"], 3).tolist() == [1]              # (inside "m k l m x", not across "... k" | "l m")
    m.compact()
    check_live(m, texts, cls, "compacted")
    m.add_documents(["y x again"])
    texts.append("y x again")
    check_live(m, texts, cls, "appended after the compaction")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.remove_documents(range(len(texts)))
    assert m.count_near(L_QUERIES, L_NEARS, L_WINDOWS).tolist() == [0] * len(L_QUERIES)
    got = m.cover(L_QUERIES, np.full((len(L_QUERIES), 2), -1))
    assert (got[0] == -1).all() and not got[1].any() and not got[2].any()


# ---- 5: forced hash collisions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_bits", [1, 3])
def test_forced_hash_collisions(small, hash_bits):
    docs = boundary_docs() + small[:60]
    queries = ["x y", "x", "y p", "f g"] + QUERIES
    near = ["x y", "y x", "x y", "x y"] + NEARS
    windows = [3, 197, 4, 2] + WINDOWS
    ctx = _native.Context()
    try:
        _native.debug_set("bm25_hash_bits", hash_bits, ctx)
        m = model("BM25", docs, ctx=ctx)
        check_near(m, docs, queries, near, windows, (10,), what=hash_bits)
        check_cover(m, docs, queries + ["x y zzz x"], all_ids(len(queries) + 1, len(docs), (-1,)), hash_bits)
        more = ["x y z", "w f y x", "nowhere d"]
        m.add_documents(more)
        docs = docs + more
        m.remove_documents([2, 61])
        docs = [d for i, d in enumerate(docs) if i not in (2, 61)]
        check_near(m, docs, queries, near, windows, (10,), what=(hash_bits, "changed"))
        check_cover(m, docs, queries, all_ids(len(queries), len(docs)), (hash_bits, "changed"))
        del m
    finally:
        _native.debug_set("bm25_hash_bits", 0, ctx)
        ctx.close()
    _native.debug_set("bm25_hash_bits", 0)


# ---- 6: failing allocations ----------------------------------------------------------------------------------------------------------------
def test_allocation_failure_sweep():
    docs = random_docs(7, 90) + boundary_docs()[:14]
    n = len(docs)
    queries, near, windows = L_QUERIES, L_NEARS, [2, 3, 200, 3, 2, 3, 1, 1]
    ids = all_ids(len(queries), n, (-1,))
    ctx = _native.Context()

    def answers(x):
        return [x.search_near(queries, 6, near, windows, match="all", exclude=["q"] * len(queries)), x.count_near(queries, near, windows),
                x.cover(queries, ids)]

    def equal(a, b):
        return same(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))

    want = answers(BM25(docs, ctx=ctx, positions=True))
    check(want[0], BM25(docs, ctx=ctx).get_scores(queries), matched(docs, queries, "all", ["q"] * len(queries), None, near, windows), 6)

    def drop(m):
        """an append and its removal: the documents are the same again, the derived arrays (postings, word offsets) are gone"""
        m.add_documents(["x y gone"])
        m.remove_documents([n])

    calls = (lambda m: m.search_near(queries, 6, near, windows, match="all", exclude=["q"] * len(queries)), lambda m: m.cover(queries, ids))
    for c, call in enumerate(calls):
        m = BM25(docs, ctx=ctx, positions=True)
        failures, ok = 0, None
        for k in range(1, 200):
            drop(m)
            _native.debug_set("inject_bad_alloc", k, ctx)
            try:
                got = call(m)
            except _native.GzError as e:
                _native.debug_set("inject_bad_alloc", 0, ctx)
                assert e.code == _native.GZ_E_NOMEM, (k, e)
                failures += 1
                assert equal(answers(m), want), (c, k)                    # the index answers as a fresh build does
                continue
            ok = k
            break
        _native.debug_set("inject_bad_alloc", 0, ctx)
        assert ok is not None and failures > 3, (c, ok, failures)
        assert same(got, want[0]) if c == 0 else all(np.array_equal(x, y) for x, y in zip(got, want[2]))
        assert equal(answers(m), want), c
        del m
    ctx.close()


# ---- 7: the device forms -------------------------------------------------------------------------------------------------------------------
def test_device_forms(small):
    docs = small + boundary_docs()
    queries = QUERIES + ["x y", "y x p"]
    near = NEARS + ["x y", "y x"]
    windows = np.array(WINDOWS + [3, 197], np.int64)
    ctx = _native.Context()
    m = BM25(docs, ctx=ctx, positions=True)
    nq, terms, idf, qoff = m._queries(queries)
    nt, no = m._sets(near)
    ct, co = m._sets(queries)
    P = m._params()
    S = m.get_scores(queries)
    g = 256

    def guarded(sizes):
        dev = [ctx.alloc(nb + 2 * g) for nb in sizes]
        for d, nb in zip(dev, sizes):
            ctx.h2d(d, np.full(nb + 2 * g, 0xA5, np.uint8))
        return dev

    def read(dev, sizes, free=True):
        raw = []
        for d, nb in zip(dev, sizes):
            x = np.empty(nb + 2 * g, np.uint8)
            ctx.d2h(x, d)
            assert np.all(x[:g] == 0xA5) and np.all(x[g + nb:] == 0xA5)
            raw.append(x[g:g + nb].copy())
            if free:
                ctx.free(d)
        return raw

    for mode, k in ((0, 4), (1, 50)):
        mt = matched(docs, queries, MODES[mode], None, None, near, windows.tolist())
        host = ctx.bm25_search(m._index, terms, idf, qoff, P, False, k, mode=mode, nr_terms=nt, nr_off=no, nr_window=windows)
        check(host, S, mt, k, (mode, k))
        sizes = (nq * k * 8, nq * k * 8, nq * 8)
        dev = guarded(sizes)
        assert ctx.bm25_search(m._index, terms, idf, qoff, P, False, k, d_ids=dev[0] + g, d_scores=dev[1] + g, d_counts=dev[2] + g, mode=mode,
                               nr_terms=nt, nr_off=no, nr_window=windows) is None
        ctx.sync()
        # the cover of what the search found: its doc_out goes straight in, padding and all
        csizes = (nq * k * 4,) * 3
        cdev = guarded(csizes)
        ctx.bm25_cover_device(m._index, ct, co, dev[0] + g, k, cdev[0] + g, cdev[1] + g, cdev[2] + g)
        ctx.sync()
        raw = read(dev, sizes)
        assert np.array_equal(raw[0].view(np.int64).reshape(nq, k), host[0])
        assert np.array_equal(raw[1].view(np.uint64).reshape(nq, k), bits(host[1]))
        assert np.array_equal(raw[2].view(np.int64), host[2])
        craw = read(cdev, csizes)
        hcov = ctx.bm25_cover(m._index, ct, co, host[0])
        want = want_cover(docs, queries, host[0])
        assert (host[0] == -1).any() and (host[0] >= 0).any()
        for a, b, c in zip(craw, hcov, want):
            assert np.array_equal(a.view(np.int32).reshape(nq, k), b) and np.array_equal(b, c)
    # ids that the host form refuses count as -1 in the device form
    bad = np.array([[0, len(docs), -7, 2 ** 40, -1, 5]] * nq, np.int64)
    d_ids = ctx.alloc(bad.nbytes)
    ctx.h2d(d_ids, bad)
    csizes = (bad.size * 4,) * 3
    cdev = guarded(csizes)
    ctx.bm25_cover_device(m._index, ct, co, d_ids, bad.shape[1], cdev[0] + g, cdev[1] + g, cdev[2] + g)
    ctx.sync()
    craw = read(cdev, csizes)
    ctx.free(d_ids)
    want = want_cover(docs, queries, np.where((bad < 0) | (bad >= len(docs)), -1, bad))
    for a, c in zip(craw, want):
        assert np.array_equal(a.view(np.int32).reshape(bad.shape), c)
    del m
    ctx.close()


# ---- 8: many bitmap words, rows in several chunks ----------------------------------------------------------------------------------------
def test_many_documents_and_chunks():
    """3 000 documents (47 bitmap words: more than one workgroup of the near kernel) and a search chunk of one row's bitmap, so that
    every query is a chunk of its own and the near offsets and windows of a later chunk are the absolute ones"""
    docs = random_docs(11, 3000)
    docs[2999] = "e e d c x y"
    ctx = _native.Context()
    try:
        _native.debug_set("bm25_search_chunk", 47, ctx)
        m = BM25(docs, ctx=ctx, positions=True)
        queries = ["x", "e d", "a", "a b c", "y e"]
        near = ["y x", "d e", "", "c b a d", "e d c"]
        windows = [2, 3, 1, 5, 4]
        mt = matched(docs, queries, "any", None, None, near, windows)
        assert mt[0].sum() == 1 and all(0 < mt[q].sum() < 3000 for q in (1, 2, 3, 4)), mt.sum(axis=1).tolist()
        assert len({int(x) for x in mt.sum(axis=1)}) == 5                 # (a row answered with another row's set or window would show)
        check_near(m, docs, queries, near, windows, (1, 20), (None, ["", "b", "", "e", ""]), (None, ["", "e d", "", "b", ""]), what="chunks")
        check_cover(m, docs, queries, m.search_near(queries, 20, near, windows)[0], "chunks")
        del m
    finally:
        ctx.close()
