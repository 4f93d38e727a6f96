"""GPU: boolean BM25 search (BM25.search / count_matches with match= and exclude=, gz_bm25_search_bool[_device],
gz_bm25_match_count_bool, csrc/gz_search.inc).  The oracle: S = get_scores(queries), pinned elsewhere; with R = set(query.split()),
X = set(exclude.split()) and W(d) from frequency_word_in_doc (through bm25_restate.Postings), matched[q, d] is
    "any": R & W(d) and not X & W(d)            "all": R and R <= W(d) and not X & W(d)
and row q = [i for i in np.argsort(-S[q], kind="stable") if matched[q, i]][:k'], -1 / the NaN 0x7FF8000000000000 behind it.  ids are
compared with ==, scores as uint64 bit patterns, counts with ==."""
import ctypes
import itertools
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
MODES = ("any", "all")


def val(x):
    return int(x["v"]) if x["t"] == "int" else float.fromhex(x["v"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model(cls, docs, b=0.75, k1=1.2, delta=1.0, ctx=None):
    return BM25Plus(docs, b, k1, delta, ctx=ctx) if cls == "BM25Plus" else BM25(docs, b, k1, ctx=ctx)


def matched(post, queries, match="any", exclude=None):
    m = np.zeros((len(queries), post.n), dtype=bool)
    for q, text in enumerate(queries):
        need = set(text.split())
        if match == "any":
            for w in need:
                if w in post.p:
                    m[q, post.p[w][0]] = True
        elif need and all(w in post.p for w in need):
            m[q] = True
            for w in need:
                has = np.zeros(post.n, dtype=bool)
                has[post.p[w][0]] = True
                m[q] &= has
        if exclude is not None:
            for w in set(exclude[q].split()):
                if w in post.p:
                    m[q, post.p[w][0]] = False
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


def check_model(m, queries, ks, excludes=(None,), modes=MODES, what="", S=None, post=None):
    """every mode x every exclude x every k against the oracle; returns {(mode, index of the exclude): matched}"""
    if S is None:
        S = m.get_scores(queries)
    if post is None:
        post = R.Postings(m.frequency_word_in_doc)
    out = {}
    for mode in modes:
        for e, ex in enumerate(excludes):
            mt = out[mode, e] = matched(post, queries, mode, ex)
            for k in ks:
                check(m.search(queries, k, match=mode, exclude=ex), S, mt, k, (what, mode, e, k))
            assert np.array_equal(m.count_matches(queries, match=mode, exclude=ex), mt.sum(axis=1)), (what, mode, e)
    return out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def well_formed(got):
    ids, sc, cnt = got
    for q in range(len(cnt)):
        c = min(int(cnt[q]), ids.shape[1])
        assert (ids[q, :c] >= 0).all() and (ids[q, c:] == -1).all() and (bits(sc[q, c:]) == PAD).all()


def next_first_word(queries):
    nq = len(queries)
    return [(queries[(q + 1) % nq].split() or [""])[0] for q in range(nq)]


@pytest.fixture(scope="module")
def corpus30k():
    import corpus
    t, o, _ = corpus.config_corpus(2, n_docs=100_000)
    raw = t.tobytes()
    return [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(30_000)]


# ---- 1: every fixture case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_case(i):
    c = CASES[i]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (np.mean of no fieldLens)
        m = model(c["cls"], c["documents"], val(c["b"]), val(c["k1"]), val(c["delta"]))
    n, queries = c["num_doc"], c["queries"]
    nq = len(queries)
    check_model(m, queries, sorted({1, 3, n + 5}), (None, [""] * nq, next_first_word(queries)), what=i)


# ---- 2: the old and the new paths agree to the bit ---------------------------------------------------------------------------
def test_old_and_new_paths_agree(corpus30k):
    docs = corpus30k[:4000]
    vocab = sorted({w for d in docs[:300] for w in d.split()})
    r = np.random.default_rng(2)
    queries = [" ".join(vocab[int(x)] for x in r.integers(0, len(vocab), int(r.integers(1, 6)))) for _ in range(20)] + ["", "nowhere"]
    nq = len(queries)
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.4)
        for k in (1, 25):
            old = m.search(queries, k)
            assert same(m.search(queries, k, match="any", exclude=None), old), (cls, k)
            assert same(m.search(queries, k, exclude=[""] * nq), old), (cls, k)        # through gz_bm25_search_bool
        cnt = m.count_matches(queries)
        assert np.array_equal(m.count_matches(queries, match="any", exclude=None), cnt)
        assert np.array_equal(m.count_matches(queries, exclude=[""] * nq), cnt)
        one = [q.split()[0] if q.split() else q for q in queries]
        assert same(m.search(one, 25, match="all"), m.search(one, 25)), cls
        assert same(m.search(one, 25, match="all", exclude=[""] * nq), m.search(one, 25)), cls
        assert np.array_equal(m.count_matches(one, match="all"), m.count_matches(one)), cls


# ---- 3: the bitmap's edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_bitmap_edges(n):
    where = {"all": range(n), "one": [n - 1], "two": [0, n - 1], "three": [0, n // 2, n - 1], "four": [0, 1, n - 2, n - 1]}
    docs = []
    for i in range(n):
        words = [w for w, at in where.items() if i in [x % n for x in at]] + ["f"] * (i % 5)
        docs.append(" ".join(words))
    queries = ["two three", "all one", "four two", "all f", "one zz", "", "   ", "two two", "all"]
    nq = len(queries)
    excludes = [None] + [[x] * nq for x in ("one", "all", "zz", "f four")]
    hand = [min(2, n), 1, min(2, n), n - (n + 4) // 5, 0, 0, 0, min(2, n), n]
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.5)
        mt = check_model(m, queries, sorted({1, 2, n, n + 2}), excludes, what=(cls, n))
        assert mt["all", 0].sum(axis=1).tolist() == hand
        assert mt["all", 3].sum(axis=1).tolist() == hand                 # excluding a word that is nowhere
        assert not mt["all", 2].any() and not mt["any", 2].any()         # excluding the word of every document
        # the last document holds "one": it leaves every row
        assert mt["all", 1].sum(axis=1).tolist() == [max(h - 1, 0) if h else 0 for h in hand[:3]] + [hand[3] - ((n - 1) % 5 != 0), 0, 0, 0,
                                                                                                  max(min(2, n) - 1, 0), n - 1]
        for ex in excludes:
            for mode in MODES:
                well_formed(m.search(queries, 2, match=mode, exclude=ex))


# ---- 4: slices of the postings (2048) and tiles of the bitmap (2048 words = 131 072 documents) ----------------------------------
def test_slice_edges():
    n = 4200
    df = {"a": 2047, "b": 2048, "c": 2049, "d": 4097}
    docs = []
    for i in range(n):
        w = ["ev"] + (["h"] if i % 2 == 0 else [])
        if i < 2047:
            w.append("a")
        if 100 <= i < 2148:
            w.append("b")
        if i >= n - 2049:
            w.append("c")
        if i < 4097:
            w.append("d")
        docs.append(" ".join(w + ["pad"] * (i % 3)))
    queries = []
    for e in df:
        queries += ["%s ev h" % e, "ev %s h" % e, "ev h %s" % e]
    queries += ["a b", "b a d", "c d a", "d c", "ev h", "h ev", "c b"]
    nq = len(queries)
    ex = ["h" if q % 2 else "" for q in range(nq)]
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.5)
        assert dict(zip(*m.vocabulary()))["d"] == 4097
        mt = check_model(m, queries, (1, 10), (None, ex), what=cls)
        full = dict(df, ev=n, h=n // 2)
        cnt = mt["all", 0].sum(axis=1)
        for q, text in enumerate(queries):
            assert cnt[q] <= min(full[w] for w in text.split()), text
        assert cnt[:3].tolist() == [1024] * 3 and cnt[12] == 1947 and cnt[16] == n // 2 and cnt[18] == 0


def test_tile_edges():
    n = 131_072 + 65
    docs = ["x y" if i % 3 == 0 else "x" for i in range(n)]
    for i in (0, 131_071, n - 1):
        docs[i] = "p q x"
    docs[131_072] = "p q y"
    docs[5] = docs[131_073] = "p"
    docs[70_000] = "q x"
    queries = ["p q", "p", "q x", "zz p", "q p q", "y q"]
    nq = len(queries)
    m = BM25(docs)
    post = R.Postings(m.frequency_word_in_doc)
    S = m.get_scores(queries)
    mt = check_model(m, queries, (1, 8), (None, ["y"] * nq, ["", "x", "p", "", "zz", "x"]), what="tiles", S=S, post=post)
    assert np.flatnonzero(mt["all", 0][0]).tolist() == [0, 131_071, 131_072, n - 1]
    assert np.flatnonzero(mt["all", 1][0]).tolist() == [0, 131_071, n - 1]
    assert np.flatnonzero(mt["all", 0][5]).tolist() == [131_072]
    assert mt["any", 0][0].sum() == 7 and mt["all", 0][3].sum() == 0 and mt["any", 0][3].sum() == 6
    p = BM25Plus(docs, delta=0.5)
    check_model(p, queries[:2], (3,), (["y", ""],), what="tiles plus", post=post)


# ---- 5: saturated signatures: only the pair table decides ------------------------------------------------------------------------
def test_saturated_signatures():
    r = np.random.default_rng(17)
    vocab = ["v%d" % i for i in range(1000)]
    long_docs = [[vocab[int(x)] for x in r.choice(1000, 400, replace=False)] for _ in range(60)]
    docs = [" ".join(w) for w in long_docs] + [" ".join(vocab[int(x)] for x in r.choice(1000, 3, replace=False)) for _ in range(60)]
    absent0 = [w for w in vocab if w not in set(long_docs[0])]
    queries, ex = [], []
    for i in range(30):
        src = long_docs[i % 60]
        words = [src[int(x)] for x in r.choice(400, 2 + i % 2, replace=False)]
        if i % 5 == 0:
            words[-1] = absent0[int(r.integers(len(absent0)))]           # absent from document 0, which holds the others for i = 0
        queries.append(" ".join(words))
        ex.append("" if i % 3 == 0 else " ".join(vocab[int(x)] for x in r.choice(1000, 1 + i % 2, replace=False)))
    queries += [" ".join(docs[60].split()), " ".join(long_docs[3][:3])]
    ex += [long_docs[5][0], absent0[0]]
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.5)
        mt = check_model(m, queries, (1, 7, 200), (None, ex), what=cls)
        assert mt["all", 0][-2, 60] and mt["all", 0][-1, 3]
        assert mt["all", 0].sum() > 60 and mt["all", 1].sum() < mt["all", 0].sum()


# ---- 6: the driver does not matter ---------------------------------------------------------------------------------------------
def test_driver_permutations():
    n = 300
    docs = []
    for i in range(n):
        w = (["r"] if i % 7 == 0 else []) + (["m"] if i % 3 == 0 else []) + (["c"] if i % 2 == 0 else [])
        w += (["e1"] if i < 100 else []) + (["e2"] if 50 <= i < 150 else [])
        docs.append(" ".join(w + ["pad"] * (i % 4)))
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.5)
        post = R.Postings(m.frequency_word_in_doc)
        assert len({post.df(w) for w in "rmc"}) == 3 and post.df("e1") == post.df("e2")
        for words, ex in ((("r", "m", "c"), None), (("r", "m", "c"), "e1"), (("e1", "e2"), None), (("e1", "e2"), "c")):
            queries = [" ".join(p) for p in itertools.permutations(words)]
            exclude = None if ex is None else [ex] * len(queries)
            check_model(m, queries, (n,), (exclude,), modes=("all",), what=(cls, words, ex), post=post)
            ids, _, cnt = m.search(queries, n, match="all", exclude=exclude)
            assert cnt[0] > 0 and (cnt == cnt[0]).all()
            sets = [frozenset(ids[q, :int(cnt[q])].tolist()) for q in range(len(queries))]
            assert len(set(sets)) == 1 and len(sets[0]) == cnt[0], (cls, words, ex)


# ---- 7: a real NaN candidate beats the padding -----------------------------------------------------------------------------------
def test_nan_candidates_before_padding():
    docs = ["w w", "w", "x", "w w y", "", "y y", "w x w"] * 40
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = BM25(docs, k1=float("nan"))
        queries = ["x", "y", "w", "x y", "q", "", "w x", "w y"]
        S = m.get_scores(queries)
        assert np.isnan(S[:4]).all()
        check_model(m, queries, (1, 50, 100, len(docs)), (None, ["y"] * len(queries)), what="k1=nan", S=S)
        ids, sc, cnt = m.search(["w x"], 100, match="all", exclude=["q"])
        assert cnt[0] == 40 and ids[0, :40].tolist() == list(range(6, len(docs), 7)) and (ids[0, 40:] == -1).all()
        assert np.isnan(sc[0]).all() and (bits(sc[0, 40:]) == PAD).all() and np.array_equal(bits(sc[0, :40]), bits(S[6, ids[0, :40]]))
        m2 = BM25(docs, b=0.0, k1=-2.0)
        qs = ["w", "w y", "x w", "y"]
        S2 = m2.get_scores(qs)
        assert np.isneginf(S2).any()
        check_model(m2, qs, (1, 5, 50, len(docs)), (None, ["x", "", "y", "w"]), what="k1=-2", S=S2)


# ---- 8: chunks -------------------------------------------------------------------------------------------------------------------
def test_chunking(corpus30k):
    """Documents: the first 30 000 of corpus.config_corpus(2, n_docs=100_000), the corpus of the plain search's chunk test."""
    docs = corpus30k
    base = BM25(docs)
    post = R.Postings(base.frequency_word_in_doc)
    r1, r2 = np.random.default_rng(21), np.random.default_rng(22)
    top = sorted(post.p, key=lambda w: (-post.df(w), w))[:50]
    queries, exclude = [], []
    for i in range(48):
        words = list(dict.fromkeys(docs[601 * i].split()))
        pick = [words[int(j)] for j in r1.choice(len(words), min(int(r1.integers(1, 5)), len(words)), replace=False)]
        if i % 6 == 0:
            pick.append(pick[0])
        queries.append(" ".join(pick))
        exclude.append(" ".join(top[int(j)] for j in r2.choice(50, 2 if i % 4 == 0 else 1, replace=False)) if i % 2 == 0 else "")
    plain = {mode: matched(post, queries, mode) for mode in MODES}
    with_ex = {mode: matched(post, queries, mode, exclude) for mode in MODES}
    changed = {mode: int((plain[mode] != with_ex[mode]).any(axis=1).sum()) for mode in MODES}
    emptied = int((plain["all"].any(axis=1) & ~with_ex["all"].any(axis=1)).sum())
    print("exclusions that change the result:", changed, "all rows emptied:", emptied, "all counts:", plain["all"].sum(axis=1).tolist())
    assert changed["all"] >= 8 and changed["any"] >= 16 and emptied >= 1
    S = base.get_scores(queries)
    want = {}
    for mode in MODES:
        want[mode] = base.search(queries, 50, match=mode, exclude=exclude)
        check(want[mode], S, with_ex[mode], 50, ("default", mode))
        check(base.search(queries, 50, match=mode), S, plain[mode], 50, ("default, no exclusions", mode))
    M = int(max(want["any"][2].max(), want["all"][2].max()))
    assert M > 1000
    for chunk in (1, M, M + 1, 5 * M + 3):
        ctx = _native.Context()
        _native.debug_set("bm25_search_chunk", chunk, ctx)
        m = BM25(docs, ctx=ctx)
        for mode in MODES:
            assert same(m.search(queries, 50, match=mode, exclude=exclude), want[mode]), (chunk, mode)
            assert np.array_equal(m.count_matches(queries, match=mode, exclude=exclude), want[mode][2]), (chunk, mode)
        del m
        ctx.close()


# ---- 9: the postings follow the index -----------------------------------------------------------------------------------------
def test_mutation():
    r = np.random.default_rng(11)
    vocab = ["w%d" % i for i in range(60)]
    docs = [" ".join(vocab[int(x)] for x in r.integers(0, 60, int(r.integers(0, 9)))) for _ in range(700)]
    docs[10] = "solo w1"
    docs[400] = "solo solo"
    more = [" ".join(vocab[int(x)] for x in r.integers(0, 60, 5)) for _ in range(130)] + ["fresh w2", "solo again"]
    queries = ["w1", "w2 w3", "solo", "fresh w2", "w59 w0 w1 absent", "", "again solo", "w1 solo", "w4 w5 w4"]
    exclude = ["w2", "w1", "", "w3", "", "w1", "w9", "again", "w6 fresh"]
    for cls in ("BM25", "BM25Plus"):
        m = model(cls, docs, delta=0.7)
        cur = list(docs)

        def agree(what):
            f = model(cls, cur, delta=0.7)
            for mode in MODES:
                for k in (1, 8, 200):
                    assert same(m.search(queries, k, match=mode, exclude=exclude), f.search(queries, k, match=mode, exclude=exclude)), (cls, what, k)
                assert np.array_equal(m.count_matches(queries, match=mode, exclude=exclude),
                                      f.count_matches(queries, match=mode, exclude=exclude)), (cls, what)
            check_model(m, queries, (8,), (exclude,), what=(cls, what))
            return f

        m.search(queries, 5, match="all", exclude=exclude)
        m.add_documents(more)
        cur += more
        agree("add")
        gone = sorted({int(x) for x in r.integers(0, len(cur), 90)} | {10, 400, len(cur) - 1})     # every document of "solo"
        m.remove_documents(gone)
        cur = [d for i, d in enumerate(cur) if i not in set(gone)]
        agree("remove")
        assert m.count_matches(["solo", "w1 solo"], match="all").tolist() == [0, 0]
        assert (m.search(["w1 solo"], 3, match="all")[0] == -1).all()
        m.search(queries, 5, match="all", exclude=exclude)
        m.compact()
        f = agree("compact")
        m.compact()                                                      # (the searches of agree() built the postings again)
        fresh = model(cls, cur, delta=0.7)
        assert m.footprint()["device_bytes"] <= fresh.footprint()["device_bytes"]
        fresh.compact()
        assert m.footprint() == fresh.footprint()
        m.search(queries, 5, match="all", exclude=exclude)
        m.remove_documents([0, 5, 6])
        cur = [d for i, d in enumerate(cur) if i not in (0, 5, 6)]
        m.search(queries, 5, exclude=exclude)
        m.add_documents(["solo returns w1", "w3"])
        cur += ["solo returns w1", "w3"]
        agree("remove, add")
        assert m.count_matches(["w1 solo"], match="all").tolist() == [1]
        assert m.count_matches(["w1 solo"], match="all", exclude=["returns"]).tolist() == [0]
        del f, fresh


# ---- 10: forced hash collisions ----------------------------------------------------------------------------------------------------
def test_forced_hash_collisions():
    r = np.random.default_rng(5)
    vocab = ["t%d" % i for i in range(200)]
    docs = [" ".join(vocab[int(x)] for x in r.integers(0, 200, int(r.integers(1, 12)))) for _ in range(300)]
    queries = ["t1 t2", "t199", "t5 t5 nope", "nope", "t7 t8", "t3 t4 t3", "t10"]
    exclude = ["t3", "", "t1", "t2", "nope t9", "", "t11 t12 t13"]
    plain = BM25(docs)
    ctx = _native.Context()
    _native.debug_set("bm25_hash_bits", 4, ctx)
    m = BM25(docs, ctx=ctx)
    for mode in MODES:
        for ex in (None, exclude):
            assert same(m.search(queries, 20, match=mode, exclude=ex), plain.search(queries, 20, match=mode, exclude=ex)), (mode, ex)
    check_model(m, queries, (20,), (None, exclude), what="hash bits 4")
    del m
    ctx.close()


def _exclusion_arrays(m, exclude):
    return m._exclusions(exclude, len(exclude))


# ---- 11: the device entry point -----------------------------------------------------------------------------------------------------
def test_device_entry_point_guards_and_device_build(corpus30k):
    from genz_tokenize._packing import pack
    docs = corpus30k[:5000]
    vocab = sorted({w for d in docs[:300] for w in d.split()})
    r = np.random.default_rng(9)
    queries = [" ".join(vocab[int(x)] for x in r.integers(0, len(vocab), int(r.integers(1, 4)))) for _ in range(14)] + ["", "nowhere"]
    for i in range(0, 14, 2):                                            # words of one document: "all" finds it
        queries[i] = " ".join(docs[37 * i].split()[:2 + i % 3])
    exclude = [vocab[int(r.integers(len(vocab)))] if i % 2 else "" for i in range(len(queries))]
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
    post = R.Postings(m.frequency_word_in_doc)
    nq, terms, idf, qoff = m._queries(queries)
    xt, xo = _exclusion_arrays(m, exclude)
    P = m._params()
    g = 256
    for plus in (False, True):
        S = ctx.bm25_score(ih, terms, idf, qoff, P, plus)
        for mode, k in ((1, 1), (1, 10), (0, 10), (1, 300)):
            mt = matched(post, queries, MODES[mode], exclude)
            host = ctx.bm25_search(ih, terms, idf, qoff, P, plus, k, mode=mode, ex_terms=xt, ex_off=xo)
            check(host, S, mt, k, (plus, mode, k))
            # (a device build numbers its terms as the host build does: the same ids serve)
            assert same(ctx.bm25_search(idv, terms, idf, qoff, P, plus, k, mode=mode, ex_terms=xt, ex_off=xo), host), ("device build", plus, k)
            sizes = (nq * k * 8, nq * k * 8, nq * 8)
            dev = [ctx.alloc(nb + 2 * g) for nb in sizes]
            for d, nb in zip(dev, sizes):
                ctx.h2d(d, np.full(nb + 2 * g, 0xA5, np.uint8))
            for index in (ih, idv):
                ctx.bm25_search(index, terms, idf, qoff, P, plus, k, d_ids=dev[0] + g, d_scores=dev[1] + g, d_counts=dev[2] + g,
                                mode=mode, ex_terms=xt, ex_off=xo)
                ctx.sync()
                raw = []
                for d, nb in zip(dev, sizes):
                    x = np.empty(nb + 2 * g, np.uint8)
                    ctx.d2h(x, d)
                    assert np.all(x[:g] == 0xA5) and np.all(x[g + nb:] == 0xA5)
                    raw.append(x[g:g + nb])
                assert np.array_equal(raw[0].view(np.int64).reshape(nq, k), host[0])
                assert np.array_equal(raw[1].view(np.uint64).reshape(nq, k), bits(host[1]))
                assert np.array_equal(raw[2].view(np.int64), host[2])
            for d in dev:
                ctx.free(d)
    assert np.array_equal(ctx.bm25_match_count(idv, terms, qoff, mode=1, ex_terms=xt, ex_off=xo),
                          matched(post, queries, "all", exclude).sum(axis=1))
    del m
    ctx.bm25_destroy(idv)
    ctx.bm25_destroy(ih)
    ctx.close()


# ---- 12: allocation failures ---------------------------------------------------------------------------------------------------------
def test_allocation_failure_sweep(corpus30k):
    docs = corpus30k[:5000]
    queries = [" ".join(docs[97 * i].split()[:1 + i % 4]) for i in range(24)] + ["", "nowhere at all"]
    exclude = [docs[97 * i + 1].split()[0] if i % 2 else "" for i in range(len(queries))]

    def sweep(boolean):
        fresh = _native.Context()                 # (no postings, no search workspace yet; the default chunk: one run of rows)
        m = BM25(docs, ctx=fresh)
        S = m.get_scores(queries)
        topk = m.top_k(queries, 40)
        nq, terms, idf, qoff = m._queries(queries)
        kw = {}
        if boolean:
            xt, xo = _exclusion_arrays(m, exclude)
            kw = dict(mode=1, ex_terms=xt, ex_off=xo)
        P = m._params()
        ok, failed = None, 0
        for k in range(1, 1000):
            _native.debug_set("inject_bad_alloc", k, fresh)
            try:
                got = fresh.bm25_search(m._index, terms, idf, qoff, P, False, 40, **kw)
            except _native.GzError as e:
                assert e.code == _native.GZ_E_NOMEM, (k, e)
                failed += 1
                _native.debug_set("inject_bad_alloc", 0, fresh)
                again = m.top_k(queries, 40)                             # context and index stay usable
                assert np.array_equal(again[0], topk[0]) and np.array_equal(bits(again[1]), bits(topk[1])), k
                continue
            ok = k
            break
        _native.debug_set("inject_bad_alloc", 0, fresh)
        assert ok is not None
        mt = matched(R.Postings(m.frequency_word_in_doc), queries, "all" if boolean else "any", exclude if boolean else None)
        check(got, S, mt, 40, boolean)
        if boolean:
            check(m.search(queries, 40, match="all", exclude=exclude), S, mt, 40)
            assert mt.any()
        del m
        fresh.close()
        return failed

    plain, boolean = sweep(False), sweep(True)
    print("failing steps: plain", plain, "boolean", boolean)
    assert plain > 10 and boolean > plain                                # the excluded terms' two buffers are reached


# ---- 13: arguments and empty shapes ------------------------------------------------------------------------------------------------------
def test_arguments_and_empty_shapes():
    m = BM25(["a b", "b c", "c d", "a a", ""])
    assert [x.shape for x in m.search([], 3, match="all")] == [(0, 3), (0, 3), (0,)]
    assert [x.shape for x in m.search([], 10**9, match="all", exclude=[])] == [(0, 5), (0, 5), (0,)]
    assert m.count_matches([], match="all").shape == (0,) and m.count_matches([], exclude=[]).shape == (0,)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        e = BM25([])
    ids, sc, cnt = e.search(["a", ""], 4, match="all", exclude=["b", ""])
    assert ids.shape == (2, 0) and sc.shape == (2, 0) and cnt.tolist() == [0, 0]
    assert e.count_matches(["a", ""], match="all", exclude=["b", ""]).tolist() == [0, 0]
    docs = ["d%d x" % i for i in range(1500)]
    big = BM25(docs)
    check_model(big, ["x d7", "d1499", "x"], (1024,), (None, ["", "", "d3"]))
    with pytest.raises(_native.GzError) as err:
        big.search(["x"], 1025, match="all")
    assert err.value.code == _native.GZ_E_LIMIT
    lib, vp = big._ctx.lib, ctypes.c_void_p
    n_terms = big._ctx.bm25_info(big._index)[1]
    terms, df = big._lookup(["x"])
    idf = np.array([big._idf_of("x", int(df[0]))])
    qoff = np.array([0, 1], np.int64)
    P = np.array(big._params())
    ids, sc, cnt = np.zeros((1, 4), np.int64), np.zeros((1, 4)), np.zeros(1, np.int64)

    def raw(k=4, mode=1, xt=None, xo=None, count=False):
        xt = None if xt is None else np.array(xt, np.int32)
        xo = None if xo is None else np.array(xo, np.int64)
        ex = [None if xt is None else vp(xt.ctypes.data), None if xo is None else vp(xo.ctypes.data)]
        if count:
            return lib.gz_bm25_match_count_bool(vp(big._index), vp(terms.ctypes.data), vp(qoff.ctypes.data), 1, mode, *ex, vp(cnt.ctypes.data))
        return lib.gz_bm25_search_bool(vp(big._index), vp(terms.ctypes.data), vp(idf.ctypes.data), vp(qoff.ctypes.data), 1, vp(P.ctypes.data), 0,
                                       k, mode, *ex, vp(ids.ctypes.data), vp(sc.ctypes.data), vp(cnt.ctypes.data))

    for count in (False, True):
        assert raw(count=count) == _native.GZ_OK and cnt[0] == 1500
        assert raw(xt=[-1, 0], xo=[0, 2], count=count) == _native.GZ_OK and cnt[0] == 1499      # term 0 = "d0"; -1 is ignored
        for mode in (2, -1):
            assert raw(mode=mode, count=count) == _native.GZ_E_INVALID, mode
        for bad in (n_terms, -2):
            assert raw(xt=[bad], xo=[0, 1], count=count) == _native.GZ_E_INVALID, bad
        assert raw(xt=[0, 0], xo=[2, 1], count=count) == _native.GZ_E_INVALID
        assert raw(xt=None, xo=[0, 1], count=count) == _native.GZ_E_INVALID
    assert raw(k=0) == _native.GZ_E_INVALID and raw(k=-3) == _native.GZ_E_INVALID and raw(k=1025) == _native.GZ_E_LIMIT
    assert big.top_k(["d3"], 2)[0][0, 0] == 3                           # the index answers as before
    check_model(big, ["x d7"], (3,), (["d8"],))
