"""GPU: snippets and query-word positions from the positional BM25 index (BM25.snippets / occurrences / snippet_texts,
gz_bm25_snippets[_device], gz_bm25_occurrences; csrc/gz_snippet.inc).  The oracle is plain Python, here, over the documents' text:
with W = documents[d].split(), Rl = queries[q].split(), R = set(Rl) and h[p] = W[p] in R, the occurrences of (q, d) are the p with
h[p], ascending, each with Rl.index(W[p]); the snippet of (q, d, w) is the smallest start s in range(max(1, len(W) - w + 1)) with
the largest sum(h[s:s+w]), and that sum; id -1 gives (-1, 0) and no occurrences.  Everything is compared with ==; no tolerance
appears anywhere."""
import warnings

import numpy as np
import pytest

from genz_tokenize import _native
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

CLASSES = ("BM25", "BM25Plus")
C = _native.C


def model(cls, docs, positions=True, ctx=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (np.mean of no fieldLens)
        return BM25Plus(docs, 0.3, 2.0, 0.5, ctx=ctx, positions=positions) if cls == "BM25Plus" else BM25(docs, ctx=ctx, positions=positions)


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def o_occurrences(doc, query):
    W, Rl = doc.split(), query.split()
    R = set(Rl)
    return [(p, Rl.index(W[p])) for p in range(len(W)) if W[p] in R]


def o_snippet(doc, query, w):
    W, R = doc.split(), set(query.split())
    h = [1 if x in R else 0 for x in W]
    best_s, best = 0, -1
    for s in range(max(1, len(W) - w + 1)):
        v = sum(h[s:s + w])
        if v > best:
            best_s, best = s, v
    return best_s, best


_cache = {}


def snippet_of(docs, d, query, w):
    """(start, hits) of the oracle, computed once per (document text, query, width)"""
    if d < 0:
        return -1, 0
    key = (docs[d], query, w)
    if key not in _cache:
        _cache[key] = o_snippet(docs[d], query, w)
    return _cache[key]


def want_snippets(docs, queries, ids, w):
    ids = np.asarray(ids)
    s = np.empty(ids.shape, dtype=np.int32)
    h = np.empty(ids.shape, dtype=np.int32)
    for q in range(ids.shape[0]):
        for j in range(ids.shape[1]):
            s[q, j], h[q, j] = snippet_of(docs, int(ids[q, j]), queries[q], w)
    return s, h


def want_occurrences(docs, queries, ids):
    ids = np.asarray(ids)
    pos, words, off = [], [], [0]
    for q in range(ids.shape[0]):
        for j in range(ids.shape[1]):
            d = int(ids[q, j])
            for p, i in (o_occurrences(docs[d], queries[q]) if d >= 0 else []):
                pos.append(p)
                words.append(i)
            off.append(len(pos))
    return np.array(pos, dtype=np.int32), np.array(words, dtype=np.int32), np.array(off, dtype=np.int64)


def check_snippets(m, docs, queries, ids, w, what=""):
    s, h = m.snippets(queries, ids, w)
    ws, wh = want_snippets(docs, queries, ids, w)
    assert s.dtype == np.int32 and h.dtype == np.int32 and s.shape == ws.shape and h.shape == wh.shape, what
    assert np.array_equal(h, wh), (what, w, np.argwhere(h != wh)[:5].tolist())
    assert np.array_equal(s, ws), (what, w, np.argwhere(s != ws)[:5].tolist())


def check_occurrences(m, docs, queries, ids, what=""):
    pos, words, off = m.occurrences(queries, ids)
    wp, ww, wo = want_occurrences(docs, queries, ids)
    assert pos.dtype == np.int32 and words.dtype == np.int32 and off.dtype == np.int64, what
    assert np.array_equal(off, wo), what
    assert np.array_equal(pos, wp), what
    assert np.array_equal(words, ww), what


# ---- 1: a random small corpus --------------------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "c", "d", "e"]
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193]
WIDTHS = [1, 2, 3, 63, 64, 65, 128, 1000, 2 ** 31 - 1]


def random_docs(seed, n=131):
    r = np.random.default_rng(seed)
    p = [0.4, 0.3, 0.15, 0.1, 0.05]
    lens = LENGTHS + [int(x) for x in r.integers(0, 12, n - len(LENGTHS))]
    r.shuffle(lens)
    return [" ".join(ALPHABET[int(i)] for i in r.choice(5, size=k, p=p)) for k in lens]


def unknown(n):
    """n words that no document holds, with repeats"""
    return ["u%d" % (i % 7) for i in range(n)]


QUERIES = [
    "e",                                     # one rare word
    "d e",                                   # two words
    "zzz",                                   # a word no document holds
    "",                                      # the empty query
    "zzz yyy zzz",                           # only unknown words
    " ".join(unknown(63) + ["e"]),           # 64 words: the only known one in the last place
    " ".join(unknown(64) + ["d"]),           # 65 words: the known one alone in the second chunk of 64
    " ".join(unknown(129) + ["c"]),          # 130 words: in the third chunk
    "b a b",                                 # a repeated word
    " ".join(["e"] + unknown(70) + ["d", "e"]),      # known words in both chunks: "e" counts under its first place, 0
]


@pytest.fixture(scope="module")
def small():
    return random_docs(1)


def id_cases(m, docs, queries):
    """(name, ids): search()'s own output with its -1 padding for k in {1, 3, 70}, every document in order, a row of one id"""
    n, nq = len(docs), len(queries)
    out = [("search k=%d" % k, m.search(queries, k)[0]) for k in (1, 3, 70)]
    out.append(("every document", np.tile(np.arange(n, dtype=np.int64), (nq, 1))))
    longest = max(range(n), key=lambda d: len(docs[d].split()))
    out.append(("one id repeated", np.full((nq, 3), longest, dtype=np.int32)))
    return out


@pytest.mark.parametrize("cls", CLASSES)
def test_random_small_corpus(small, cls):
    docs = small
    assert sorted(set(len(d.split()) for d in docs) & set(LENGTHS)) == LENGTHS
    assert [len(q.split()) for q in QUERIES[5:8]] == [64, 65, 130]
    m = model(cls, docs)
    cases = id_cases(m, docs, QUERIES)
    assert any((ids == -1).any() for _, ids in cases[:3]) and any((ids >= 0).all(axis=1).any() for _, ids in cases[:3])
    for name, ids in cases:
        for w in WIDTHS:
            check_snippets(m, docs, QUERIES, ids, w, (cls, name))
    # (the corpus is worth the test: windows tied for the best count occur, and so do best starts behind the first trip's start)
    ties = late = far = 0
    for q in (0, 1, 8):
        R = set(QUERIES[q].split())
        for d in docs:
            h = [1 if x in R else 0 for x in d.split()]
            for w in WIDTHS:
                v = [sum(h[s:s + w]) for s in range(max(1, len(h) - w + 1))]
                ties += max(v) > 0 and v.count(max(v)) > 1
                late += v.index(max(v)) > 0
                far += v.index(max(v)) > 64                   # (the best window lies in a later trip of 64 starts: the carry)
    assert ties > 20 and late > 20 and far > 0, (ties, late, far)


# ---- 2: boundaries, built by hand ------------------------------------------------------------------------------------------------------
def boundary_docs():
    return [
        "p q r s t",                             # 0: no query word ...
        "x y x p q",                             # 1: ... followed by a document that starts with them
        "",                                      # 2
        " ".join(["f"] * 64 + ["x"]),            # 3: the only hit at position 64
        " ".join(["f"] * 128 + ["x"] + ["f"] * 70),      # 4: the only hit at position 128
        "x y y x x y",                           # 5: all words hit
        " ".join(["f"] * 300 + ["x", "f", "x"] + ["f"] * 100 + ["x", "x", "f", "f"]),    # 6: two windows of two hits; the first wins
        "p q r x",                               # 7: the last document: its hit is the last word of seq
    ]


B_QUERIES = ["x y", "x", "y x q"]


@pytest.mark.parametrize("cls", CLASSES)
def test_boundaries(cls):
    docs = boundary_docs()
    m = model(cls, docs)
    ids = np.tile(np.arange(len(docs), dtype=np.int64), (len(B_QUERIES), 1))
    for w in (1, 2, 3, 4, 5, 6, 64, 65, 128, 129, 200, 10 ** 6):
        check_snippets(m, docs, B_QUERIES, ids, w, cls)
    s, h = m.snippets(["x y"], [[0, 1, 2, 7, -1]], 1)
    assert s.tolist() == [[0, 0, 0, 3, -1]] and h.tolist() == [[0, 1, 0, 1, 0]]          # nothing leaks from document 1 into 0
    s, h = m.snippets(["x y"], [[0, 1]], 2)
    assert s.tolist() == [[0, 0]] and h.tolist() == [[0, 2]]
    s, h = m.snippets(["x y"], [[0, 1, 5]], 50)
    assert s.tolist() == [[0, 0, 0]] and h.tolist() == [[0, 3, 6]]
    s, h = m.snippets(["x", "x"], [[3, 4], [6, 6]], 1)
    assert s.tolist() == [[64, 128], [300, 300]] and h.tolist() == [[1, 1], [1, 1]]
    s, h = m.snippets(["x"], [[6, 6]], 3)
    assert s.tolist() == [[300, 300]] and h.tolist() == [[2, 2]]
    check_occurrences(m, docs, B_QUERIES, ids, cls)
    pos, words, off = m.occurrences(["y x q"], [[7, 1, 0]])
    assert pos.tolist() == [1, 3, 0, 1, 2, 4, 1] and words.tolist() == [2, 1, 1, 0, 1, 2, 2] and off.tolist() == [0, 2, 6, 7]


# ---- 3: occurrences --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_occurrences(small, cls):
    docs = small
    m = model(cls, docs)
    for name, ids in id_cases(m, docs, QUERIES):
        check_occurrences(m, docs, QUERIES, ids, (cls, name))
    # a call without any occurrence
    pos, words, off = m.occurrences(["zzz", "", "u1 u2"], [[0, 1, 2, -1]] * 3)
    assert pos.shape == (0,) and words.shape == (0,) and off.tolist() == [0] * 13


def test_occurrences_scan_crosses_a_block(small):
    docs = small
    m = model("BM25", docs)
    queries = [QUERIES[i % len(QUERIES)] for i in range(70)]
    ids = np.array([[(7 * q + j) % len(docs) if (q + j) % 9 else -1 for j in range(64)] for q in range(70)], dtype=np.int64)
    assert ids.size > 4096
    check_occurrences(m, docs, queries, ids, "70 x 64")
    check_snippets(m, docs, queries, ids, 5, "70 x 64")


def native_args(m, queries, ids):
    terms, qoff = m._query_terms(queries)
    terms = np.ascontiguousarray(terms, dtype=np.int32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    keep = (terms, qoff, ids)
    return keep, [C.c_void_p(m._index), _native._ptr(terms) if len(terms) else None, _native._ptr(qoff), len(queries), _native._ptr(ids), ids.shape[1]]


def test_occurrences_native_sizes_and_capacity(small):
    docs = small
    m = model("BM25", docs)
    lib = m._ctx.lib
    queries = ["d e", "b a b"]
    ids = np.array([[3, 9, -1, 40], [5, 5, 77, 0]], dtype=np.int64)
    wp, ww, wo = want_occurrences(docs, queries, ids)
    T = int(wo[-1])
    assert T > 2
    keep, args = native_args(m, queries, ids)
    off = np.full(ids.size + 1, -9, dtype=np.int64)
    assert lib.gz_bm25_occurrences(*args, _native._ptr(off), None, None, 0) == _native.GZ_OK          # sizes first
    assert np.array_equal(off, wo)
    off[:] = -9
    pos = np.full(T + 2, -9, dtype=np.int32)
    words = np.full(T + 2, -9, dtype=np.int32)
    assert lib.gz_bm25_occurrences(*args, _native._ptr(off), _native._ptr(pos), _native._ptr(words), T) == _native.GZ_OK
    assert np.array_equal(off, wo) and np.array_equal(pos[:T], wp) and np.array_equal(words[:T], ww)
    assert pos[T:].tolist() == [-9, -9] and words[T:].tolist() == [-9, -9]
    off[:] = -9
    pos[:] = -9
    words[:] = -9
    assert lib.gz_bm25_occurrences(*args, _native._ptr(off), _native._ptr(pos), _native._ptr(words), T - 1) == _native.GZ_E_CAPACITY
    assert (off == -9).all() and (pos == -9).all() and (words == -9).all()


# ---- 4: the index in every state ---------------------------------------------------------------------------------------------------------
def answers(m, queries, ids, widths=(1, 3, 64, 1000)):
    out = [m.snippets(queries, ids, w) for w in widths]
    return [a for pair in out for a in pair] + list(m.occurrences(queries, ids))


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("cls", CLASSES)
def test_live_index(small, cls):
    docs = ["q0 q1 e q0"] + small                            # (document 0 holds the first two terms of the table alone)
    queries = QUERIES + ["q1 a", "q0"]
    m = model(cls, docs[:60])
    m.add_documents(docs[60:])
    ids = np.tile(np.arange(len(docs), dtype=np.int64), (len(queries), 1))
    got = answers(m, queries, ids)
    assert same(got, answers(model(cls, docs), queries, ids))
    check_snippets(m, docs, queries, ids, 3, (cls, "appended"))
    check_occurrences(m, docs, queries, ids, (cls, "appended"))
    gone = [0, 5, 17, 64, 100, len(docs) - 1]
    m.remove_documents(gone)
    left = [d for i, d in enumerate(docs) if i not in gone]
    fresh = model(cls, left)
    ids = np.tile(np.arange(len(left), dtype=np.int64), (len(queries), 1))
    # (before compaction the term ids are not a fresh build's; the answers are about the texts and must not care)
    assert not np.array_equal(m._lookup(ALPHABET)[0], fresh._lookup(ALPHABET)[0])
    want = answers(fresh, queries, ids)
    assert same(answers(m, queries, ids), want)
    check_snippets(m, left, queries, ids, 2, (cls, "removed"))
    check_occurrences(m, left, queries, ids, (cls, "removed"))
    m.compact()
    assert np.array_equal(m._lookup(ALPHABET)[0], fresh._lookup(ALPHABET)[0])
    assert same(answers(m, queries, ids), want)
    m.add_documents(["e d e", ""])
    left2 = left + ["e d e", ""]
    ids = np.tile(np.arange(len(left2), dtype=np.int64), (len(queries), 1))
    assert same(answers(m, queries, ids), answers(model(cls, left2), queries, ids))


def test_first_call_on_a_fresh_index_builds_no_postings(small):
    docs = small
    ids = [[0, 5, -1], [7, 7, 130]]
    for call in ("snippets", "occurrences"):
        m, twin = model("BM25", docs), model("BM25", docs)
        before = m.footprint()["device_bytes"]
        if call == "snippets":                               # (the first call of all: the index has no word offsets and no postings)
            s, h = m.snippets(["e", "d a"], ids, 4)
            ws, wh = want_snippets(docs, ["e", "d a"], ids, 4)
            assert np.array_equal(s, ws) and np.array_equal(h, wh)
        else:
            check_occurrences(m, docs, ["e", "d a"], ids, "fresh")
        twin.term_sequences()                                # (derives the word offsets and nothing else)
        assert m.footprint()["device_bytes"] == twin.footprint()["device_bytes"] > before
        twin.search(["e"], 3)                                # (what postings would have cost)
        assert twin.footprint()["device_bytes"] > m.footprint()["device_bytes"]


def test_no_documents_and_empty_shapes():
    m = model("BM25", [])
    s, h = m.snippets(["a", "b"], [[-1, -1], [-1, -1]], 3)
    assert s.tolist() == [[-1, -1]] * 2 and h.tolist() == [[0, 0]] * 2
    pos, words, off = m.occurrences(["a", "b"], [[-1, -1], [-1, -1]])
    assert pos.shape == (0,) and off.tolist() == [0] * 5
    m = model("BM25", ["a b", "c"])
    s, h = m.snippets(["a"], np.zeros((1, 0), dtype=np.int64))
    assert s.shape == (1, 0) and h.shape == (1, 0) and s.dtype == np.int32
    assert m.occurrences([], np.zeros((0, 4), dtype=np.int64))[2].tolist() == [0]


# ---- 5: the device form --------------------------------------------------------------------------------------------------------------
def test_device_form(small):
    docs = small
    ctx = _native.Context()
    m = BM25(docs, ctx=ctx, positions=True)
    queries = QUERIES
    nq, terms, idf, qoff = m._queries(queries)
    k, w, g = 10, 5, 256
    host_ids = m.search(queries, k)[0]
    sizes = (nq * k * 8, nq * k * 8, nq * 8, nq * k * 4, nq * k * 4)
    dev = [ctx.alloc(nb + 2 * g) for nb in sizes]
    for d, nb in zip(dev, sizes):
        ctx.h2d(d, np.full(nb + 2 * g, 0xA5, np.uint8))
    ctx.bm25_search(m._index, terms, idf, qoff, m._params(), False, k, d_ids=dev[0] + g, d_scores=dev[1] + g, d_counts=dev[2] + g)
    ctx.bm25_snippets_device(m._index, terms, qoff, dev[0] + g, k, w, dev[3] + g, dev[4] + g)      # search's doc_out, no round trip
    ctx.sync()

    def read(i):
        x = np.empty(sizes[i] + 2 * g, np.uint8)
        ctx.d2h(x, dev[i])
        assert np.all(x[:g] == 0xA5) and np.all(x[g + sizes[i]:] == 0xA5)
        return x[g:g + sizes[i]]

    assert np.array_equal(read(0).view(np.int64).reshape(nq, k), host_ids)
    s, h = m.snippets(queries, host_ids, w)
    assert np.array_equal(read(3).view(np.int32).reshape(nq, k), s) and np.array_equal(read(4).view(np.int32).reshape(nq, k), h)
    ws, wh = want_snippets(docs, queries, host_ids, w)
    assert np.array_equal(s, ws) and np.array_equal(h, wh)
    # ids outside [-1, documents) in device memory count as -1: no error, nothing read through
    bad = host_ids.copy()
    bad[0, 0], bad[1, 1], bad[4, 2] = len(docs), -7, 2 ** 40
    ctx.h2d(dev[0] + g, bad)
    ctx.bm25_snippets_device(m._index, terms, qoff, dev[0] + g, k, w, dev[3] + g, dev[4] + g)
    ctx.sync()
    ok = np.where((bad >= 0) & (bad < len(docs)), bad, -1)
    ws, wh = want_snippets(docs, queries, ok, w)
    assert ws[0, 0] == -1 and ws[1, 1] == -1 and ws[4, 2] == -1
    assert np.array_equal(read(3).view(np.int32).reshape(nq, k), ws) and np.array_equal(read(4).view(np.int32).reshape(nq, k), wh)
    for d in dev:
        ctx.free(d)
    del m
    ctx.close()


# ---- 6: errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(small):
    docs = small
    plain = model("BM25", docs, positions=False)
    for fn in (lambda: plain.snippets(["a"], [[0]]), lambda: plain.occurrences(["a"], [[0]]), lambda: plain.snippet_texts(["a"], [[0]])):
        with pytest.raises(ValueError, match="positions"):
            fn()
    lib = plain._ctx.lib
    keep, args = native_args(plain, ["a"], np.array([[0]]))
    s = np.full(1, -9, dtype=np.int32)
    h = np.full(1, -9, dtype=np.int32)
    off = np.full(2, -9, dtype=np.int64)
    assert lib.gz_bm25_snippets(*args, 3, _native._ptr(s), _native._ptr(h)) == _native.GZ_E_INVALID
    assert lib.gz_bm25_occurrences(*args, _native._ptr(off), None, None, 0) == _native.GZ_E_INVALID
    assert s[0] == -9 and h[0] == -9 and (off == -9).all()
    m = model("BM25", docs)
    with pytest.raises(IndexError):
        m.snippets(["a"], [[len(docs)]])
    ids = np.array([[0, 1, len(docs)], [2, -2, 3]], dtype=np.int64)
    keep, args = native_args(m, ["a", "e d"], ids)
    s = np.full(6, -9, dtype=np.int32)
    h = np.full(6, -9, dtype=np.int32)
    off = np.full(7, -9, dtype=np.int64)
    for bad in (ids, np.array([[0, 1, 2], [2, -2, 3]], dtype=np.int64)):
        a = list(args)
        a[4] = _native._ptr(bad)
        assert lib.gz_bm25_snippets(*a, 3, _native._ptr(s), _native._ptr(h)) == _native.GZ_E_INVALID
        assert lib.gz_bm25_occurrences(*a, _native._ptr(off), None, None, 0) == _native.GZ_E_INVALID
        assert (s == -9).all() and (h == -9).all() and (off == -9).all()          # the outputs keep their fill pattern
    good = np.array([[0, 1, 2], [2, -1, 3]], dtype=np.int64)
    a = list(args)
    a[4] = _native._ptr(good)
    assert lib.gz_bm25_snippets(*a, 0, _native._ptr(s), _native._ptr(h)) == _native.GZ_E_INVALID          # width < 1
    a[5] = -1
    assert lib.gz_bm25_snippets(*a, 3, _native._ptr(s), _native._ptr(h)) == _native.GZ_E_INVALID          # k < 0
    a[5] = 3
    terms = np.array([0, m._ctx.bm25_info(m._index)[1] + 5, 1], dtype=np.int32)
    a[1] = _native._ptr(terms)
    assert lib.gz_bm25_snippets(*a, 3, _native._ptr(s), _native._ptr(h)) == _native.GZ_E_INVALID          # a term outside [-1, n_terms)
    a[1] = args[1]
    down = np.array([0, 3, 1], dtype=np.int64)
    a[2] = _native._ptr(down)
    assert lib.gz_bm25_snippets(*a, 3, _native._ptr(s), _native._ptr(h)) == _native.GZ_E_INVALID          # decreasing query_off
    assert (s == -9).all() and (h == -9).all()
    a[2] = args[2]
    assert lib.gz_bm25_snippets(*a, 3, _native._ptr(s), _native._ptr(h)) == _native.GZ_OK
    ws, wh = want_snippets(docs, ["a", "e d"], good, 3)
    assert np.array_equal(s.reshape(2, 3), ws) and np.array_equal(h.reshape(2, 3), wh)


# ---- 7: snippet_texts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_snippet_texts(small, cls):
    docs = small + boundary_docs()
    queries = ["e", "d e", "x y", "", "zzz a"]
    m = model(cls, docs)
    ids = m.search(queries, 6)[0]
    assert (ids == -1).any()
    all_ids = np.tile(np.arange(len(docs), dtype=np.int64), (len(queries), 1))
    for ids in (ids, all_ids):
        for w in (1, 4, 32, 500):
            plain = m.snippet_texts(queries, ids, w)
            marked = m.snippet_texts(queries, ids, w, mark=("<b>", "</b>"))
            for q, query in enumerate(queries):
                R = set(query.split())
                for j, d in enumerate(ids[q].tolist()):
                    if d < 0:
                        assert plain[q][j] == "" and marked[q][j] == ""
                        continue
                    s, _ = snippet_of(docs, d, query, w)
                    win = docs[d].split()[s:s + w]
                    assert plain[q][j] == " ".join(win), (q, d, w)
                    assert marked[q][j] == " ".join("<b>" + x + "</b>" if x in R else x for x in win), (q, d, w)
    assert m.snippet_texts(["x y"], [[len(small) + 1, -1]], 2, mark=("[", "]")) == [["[x] [y]", ""]]
    assert m._documents is None                              # (the whole corpus was never split)
    assert m.snippet_texts(["x y"], [[len(small) + 1]]) == [["x y x p q"]]          # width defaults to 32
