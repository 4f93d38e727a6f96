"""GPU: BM25 search over word groups (BM25.search_groups / count_groups / group_df / expand / search_fuzzy,
gz_bm25_search_groups[_device], gz_bm25_match_count_groups; csrc/gz_groups.inc).  The oracle is plain Python / numpy, here: with
A_g the distinct alternatives of group g that some document holds, f_g = the sum of their count rows (bm25_restate.Postings),
df_g = the documents with f_g > 0, idf_g = bm25_restate.idf(N, df_g), the scores are bm25_restate.scores with the groups standing
where words stand, a document matches when some ("any") or every ("all", and there is a group) f_g > 0 and it holds no excluded
word, and row q = [i for i in np.argsort(-S[q], kind="stable") if matched[q, i]][:k'], -1 / the NaN 0x7FF8000000000000 behind it.
ids and counts are compared with ==, scores as uint64 bit patterns.  Two equalities carry the weight: singleton groups equal
`search`, and a corpus rewritten so that every group is one fresh word gives, through `search`, the grouped result."""
import ctypes
import itertools
import warnings

import numpy as np
import pytest

import bm25_restate as R
from genz_tokenize import _native
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

PAD = np.uint64(0x7FF8000000000000)
MODES = ("any", "all")
CLASSES = ("BM25", "BM25Plus")
B, K1, DELTA = 0.75, 1.2, 0.5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model(cls, docs, ctx=None, **kw):
    return BM25Plus(docs, B, K1, DELTA, ctx=ctx, **kw) if cls == "BM25Plus" else BM25(docs, B, K1, ctx=ctx, **kw)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


class Stats:
    """what the oracle needs of a corpus, computed once"""

    def __init__(self, docs):
        self.lens, freq = R.stats(docs)
        self.n = len(docs)
        self.avg = R.avg_field_len(self.lens)
        self.post = R.Postings(freq)


class _GroupRows(R.Postings):
    """bm25_restate.scores reads a query word's count row through Postings.get: here the "word" is a group's index"""

    def __init__(self, rows):
        self.rows = rows

    def get(self, g):
        return self.rows[g]


def group_rows(st, query):
    """[(f_g float64 [N], df_g, idf_g)] of one query's groups"""
    out = []
    for group in query:
        f = np.zeros(st.n, dtype=np.float64)
        for a in dict.fromkeys(group):
            f = f + st.post.get(a)
        df = int(np.count_nonzero(f))
        out.append((f, df, R.idf(st.n, df)))
    return out


def oracle(st, groups, k, cls, match="any", exclude=None):
    nq = len(groups)
    kk = min(k, st.n)
    ids = np.full((nq, kk), -1, dtype=np.int64)
    sc = np.full((nq, kk), PAD, dtype=np.uint64)
    cnt = np.zeros(nq, dtype=np.int64)
    for q, query in enumerate(groups):
        rows = group_rows(st, query)
        if match == "any":
            m = np.zeros(st.n, dtype=bool)
            for f, _, _ in rows:
                m |= f > 0
        else:
            m = np.full(st.n, bool(rows))
            for f, _, _ in rows:
                m &= f > 0
        if exclude is not None:
            for w in set(exclude[q].split()):
                m &= st.post.get(w) == 0
        cnt[q] = int(m.sum())
        if not rows or not cnt[q]:
            continue
        S = R.scores(st.lens, _GroupRows([f for f, _, _ in rows]), st.avg, range(len(rows)), [v for _, _, v in rows], B, K1,
                     DELTA if cls == "BM25Plus" else None)
        order = np.argsort(-S, kind="stable")
        o = order[m[order]][:kk]
        ids[q, :len(o)] = o
        sc[q, :len(o)] = bits(S[o])
    return ids, sc, cnt


def check(got, want, what=""):
    ids, sc, cnt = got
    assert ids.dtype == np.int64 and sc.dtype == np.float64 and cnt.dtype == np.int64, what
    assert ids.shape == want[0].shape and sc.shape == want[1].shape and cnt.shape == want[2].shape, (what, ids.shape, want[0].shape)
    assert np.array_equal(cnt, want[2]), (what, cnt.tolist(), want[2].tolist())
    assert np.array_equal(ids, want[0]), what
    assert np.array_equal(bits(sc), want[1]), what


def check_model(m, cls, st, groups, ks, excludes=(None,), modes=MODES, what=""):
    """every mode x every exclude x every k against the oracle; returns {(mode, index of the exclude): counts}"""
    out = {}
    for mode in modes:
        for e, ex in enumerate(excludes):
            for k in ks:
                want = oracle(st, groups, k, cls, mode, ex)
                check(m.search_groups(groups, k, match=mode, exclude=ex), want, (what, cls, mode, e, k))
            out[mode, e] = want[2]
            assert np.array_equal(m.count_groups(groups, match=mode, exclude=ex), want[2]), (what, cls, mode, e)
    return out


def singletons(queries):
    return [[[w] for w in q.split()] for q in queries]


@pytest.fixture(scope="module")
def corpus30k():
    import corpus
    t, o, _ = corpus.config_corpus(2, n_docs=100_000)
    raw = t.tobytes()
    return [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(30_000)]


def synthetic(n, n_words, seed, longest=9):
    r = np.random.default_rng(seed)
    vocab = ["w%d" % i for i in range(n_words)]
    return vocab, [" ".join(vocab[int(x)] for x in r.integers(0, n_words, int(r.integers(0, longest)))) for _ in range(n)]


# ---- 1: singleton groups are the plain search, bit for bit -------------------------------------------------------------------
def test_singleton_groups_equal_search(corpus30k):
    docs = corpus30k[:4000]
    vocab = sorted({w for d in docs[:400] for w in d.split()})
    r = np.random.default_rng(3)
    queries = []
    for i in range(300):
        words = [vocab[int(x)] for x in r.integers(0, len(vocab), int(r.integers(1, 6)))]
        if i % 7 == 0:
            words.append("nowhere%d" % i)
        if i % 11 == 0:
            words.append(words[0])
        if i % 5 == 0:
            words = docs[13 * i].split()[:1 + i % 4]              # words of one document: "all" finds it
        queries.append(" ".join(words))
    queries += ["", "   ", "nowhere"]
    exclude = [vocab[int(r.integers(len(vocab)))] if i % 2 else "" for i in range(len(queries))]
    groups = singletons(queries)
    for cls in CLASSES:
        m = model(cls, docs)
        nonempty = 0
        for mode in MODES:
            for ex in (None, exclude):
                for k in (1, 25):
                    want = m.search(queries, k, match=mode, exclude=ex)
                    assert same(m.search_groups(groups, k, match=mode, exclude=ex), want), (cls, mode, k)
                    assert same(m.search_fuzzy(queries, k, max_edits=0, match=mode, exclude=ex), want), (cls, mode, k)
                nonempty += int((want[2] > 0).sum())
                assert np.array_equal(m.count_groups(groups, match=mode, exclude=ex), m.count_matches(queries, match=mode, exclude=ex))
        assert nonempty > 300
    st = Stats(docs)
    check(m.search_groups(groups[:40], 10, match="all", exclude=exclude[:40]), oracle(st, groups[:40], 10, "BM25Plus", "all", exclude[:40]))


# ---- 2: a corpus rewritten so that every group is one fresh word ------------------------------------------------------------------
def test_rewritten_corpus():
    vocab, docs = synthetic(900, 40, 7)
    for i in range(len(docs)):                                    # two pairs of words whose unions coincide
        if i % 5 == 0:
            docs[i] += " p1 q2"
        elif i % 5 == 1:
            docs[i] += " p2 q1 p2"
    docs[17] = "w1 w1 w2 w2 w2 w30"                               # f_g = 2 + 3
    docs[18] = "w3 w1 w3 w2 w9 w1"
    part = {"h1": ["w1", "w2", "w3"], "h2": ["w4", "w5"], "h3": ["w6"], "h4": ["p1", "p2"], "h5": ["q1", "q2"],
            "h6": ["w7", "w8", "w9", "w10", "w11", "w12", "w13"]}
    back = {w: h for h, ws in part.items() for w in ws}
    rewritten = [" ".join(back.get(w, w) for w in d.split()) for d in docs]
    shapes = [["h1"], ["h1", "h2"], ["h2", "h3", "h1"], ["h4", "h5"], ["h5", "h4", "h1"], ["h6", "h3"], ["h1", "h1"], ["h6"], [],
              ["h3", "h6", "h2", "h4"]]
    groups = [[list(part[h]) for h in s] for s in shapes]
    groups[1][0] = ["w3", "nowhere", "w1", "w2", "w1"]            # an unknown alternative and a repeat change nothing
    plain = [" ".join(s) for s in shapes]
    exclude = ["", "w20", "w21 w22", "", "w23", "w24", "nowhere", "", "w20", "w25"]
    st, st2 = Stats(docs), Stats(rewritten)
    assert st.lens == st2.lens and bits(st.avg) == bits(st2.avg)
    for cls in CLASSES:
        m, m2 = model(cls, docs), model(cls, rewritten)
        for mode in MODES:
            for ex in (None, exclude):
                for k in (1, 12, 900):
                    got = m.search_groups(groups, k, match=mode, exclude=ex)
                    assert same(got, m2.search(plain, k, match=mode, exclude=ex)), (cls, mode, k)
                    check(got, oracle(st, groups, k, cls, mode, ex), (cls, mode, k))
                    check(got, oracle(st2, singletons(plain), k, cls, mode, ex), (cls, mode, k, "rewritten"))
        ids, _, cnt = m.search_groups(groups, 900, match="all")
        assert cnt[3] == 360 and cnt[0] > 100 and cnt[8] == 0 and 17 in ids[0, :cnt[0]] and 18 in ids[0, :cnt[0]]
        df = m.group_df(groups)
        assert df[3] == [360, 360] and df[1][0] == df[0][0] == st2.post.df("h1")


# ---- 3: the bitmap's edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_bitmap_edges(n):
    docs = ["x f" if i % 2 else "x" for i in range(n)]
    docs[n - 1] = "x z2 z2"
    groups = [[["z1", "z2", "z3"]], [["z2", "zz"], ["x", "f"]], [["x", "z2"]], [["f", "z1"], ["z2"]], [["zz"], ["x"]], [], [["f"], ["x"], ["z2", "f"]]]
    ex = ["", "", "z2", "", "", "x", "zz"]
    st = Stats(docs)
    for cls in CLASSES:
        m = model(cls, docs)
        cnt = check_model(m, cls, st, groups, sorted({1, 2, n, n + 2}), (None, ex), what=n)
        assert cnt["all", 0].tolist()[:6] == [1, 1, n, 0, 0, 0] and cnt["any", 0][4] == n and cnt["all", 1][2] == n - 1
        ids = m.search_groups(groups[:2], 2, match="all")[0]
        assert ids[:, 0].tolist() == [n - 1, n - 1]


# ---- 4: more than one tile of the bitmap; slices of the postings inside the driver group ---------------------------------------
def test_tile_edge():
    n = 64 * 2048 + 65
    docs = ["a" if i % 3 == 0 else "b" for i in range(n)]
    for i in (0, 131_071, 131_072, n - 1):
        docs[i] = "c"
    docs[70_000] = "d"
    groups = [[["c", "d"]], [["c", "zz"], ["d", "c", "a"]], [["d"], ["c"]], [["a", "c"], ["c", "d", "b"]]]
    st = Stats(docs)
    m = BM25(docs, B, K1)
    cnt = check_model(m, "BM25", st, groups, (1, 8), (None, ["", "", "", "d"]), what="tiles")
    assert cnt["all", 0].tolist() == [5, 4, 0, 4] and cnt["any", 0][2] == 5
    assert m.search_groups(groups[:1], 8)[0][0, :5].tolist() == [0, 70_000, 131_071, 131_072, n - 1]     # (equal scores: by id)
    check(BM25Plus(docs, B, K1, DELTA).search_groups(groups[:2], 3, match="all"), oracle(st, groups[:2], 3, "BM25Plus", "all"))


def test_slice_edges():
    n = 4200
    docs = []
    for i in range(n):
        w = ["ev"] + (["h"] if i % 2 == 0 else [])
        if i < 2047:
            w.append("a")
        if 100 <= i < 2148:
            w.append("b")
        if i >= n - 2049:
            w.append("c")
        docs.append(" ".join(w + ["pad"] * (i % 3)))
    # (mode "all": the driver is the group with the smallest sum -- a + b = 4095, c + nothing = 2049, a + c = 4096 -- before ev = 4200)
    groups = [[["a", "b"], ["ev"]], [["ev", "h"], ["c", "nowhere"]], [["ev"], ["c", "a"], ["h", "pad"]], [["b"], ["a"]], [["a", "b", "c"], ["ev"]]]
    st = Stats(docs)
    for cls in CLASSES:
        m = model(cls, docs)
        assert m.group_df([[["a"], ["b"], ["c"]]]) == [[2047, 2048, 2049]]
        cnt = check_model(m, cls, st, groups, (1, 10), (None, ["h", "", "a", "", "pad"]), what="slices")
        assert cnt["all", 0].tolist()[:2] == [2148, 2049] and cnt["all", 0][3] == 1947


# ---- 5: the sizes of a group -------------------------------------------------------------------------------------------------------
def test_group_sizes():
    n = 500
    r = np.random.default_rng(31)
    vocab = ["t%d" % i for i in range(70)]
    docs = [" ".join(vocab[int(x)] for x in r.integers(0, 70, int(r.integers(1, 6)))) + " all" for _ in range(n)]
    docs += [" ".join(vocab) + " all"]
    st = Stats(docs)
    assert all(st.post.df(w) > 0 for w in vocab)
    groups = [[vocab[:1]], [vocab[:2]], [vocab[:63]], [vocab[:64]], [vocab[1:64], ["all"]], [vocab[:64], vocab[6:70]],
              [vocab[:64] + [vocab[5]]],                                      # 65 entries, 64 distinct
              [["t1", "t1"]], [["t1", "nope", "t2", "", "nope2"]],
              [[], ["t3"]], [["nope"], ["t3"]], [[]], [["nope", "nope2"]], [["t3"], []]]
    for cls in CLASSES:
        m = model(cls, docs)
        cnt = check_model(m, cls, st, groups, (1, 20), (None, ["t69"] * len(groups)), what="sizes")
        assert cnt["all", 0].tolist()[9:] == [0] * 5 and cnt["any", 0][9] == cnt["any", 0][10] == cnt["any", 0][13] == st.post.df("t3")
        assert same(m.search_groups(groups[6:7], 20), m.search_groups(groups[3:4], 20))
        assert same(m.search_groups(groups[7:8], 20), m.search_groups([[["t1"]]], 20))
        assert same(m.search_groups(groups[8:9], 20, match="all"), m.search_groups([[["t2", "t1"]]], 20, match="all"))
        for bad in ([[vocab[:65]]], [[["t1"]], [["t2"], vocab[5:70], ["t3"]]]):
            for mode in MODES:
                with pytest.raises(_native.GzError) as err:
                    m.search_groups(bad, 5, match=mode)
                assert err.value.code == _native.GZ_E_LIMIT
                with pytest.raises(_native.GzError) as err:
                    m.count_groups(bad, match=mode)
                assert err.value.code == _native.GZ_E_LIMIT
        check(m.search_groups(groups[:4], 7, match="all"), oracle(st, groups[:4], 7, cls, "all"), "after the refusals")


# ---- 6: the driver does not show ----------------------------------------------------------------------------------------------------
def test_driver_choice_does_not_show():
    n = 600
    docs = []
    for i in range(n):
        w = (["a1", "a2"] if i < 100 else []) + (["b"] if 50 <= i < 200 else []) + (["c1"] if i % 3 == 0 else []) + (["c2"] if i % 4 == 0 else [])
        w += ["e1"] * (i % 3) if i < 300 else []
        docs.append(" ".join(w + ["pad"] * (i % 4)))
    st = Stats(docs)
    A, Bg, Cg = ["a1", "a2"], ["b"], ["c1", "c2", "nope"]
    # the smallest sum (b: 150 < a1 + a2: 200) and the smallest union (a1 | a2: 100 < b: 150) are different groups
    assert st.post.df("a1") + st.post.df("a2") > st.post.df("b") > int(np.count_nonzero(st.post.get("a1") + st.post.get("a2")))
    for cls in CLASSES:
        m = model(cls, docs)
        for ex in (None, "e1"):
            base = None
            for order in itertools.permutations((A, Bg, Cg)):
                inner = [[list(p) for p in itertools.permutations(g)] for g in order]
                groups = [list(combo) for combo in itertools.product(*inner)]
                exclude = None if ex is None else [ex] * len(groups)
                for mode in MODES:
                    got = m.search_groups(groups, n, match=mode, exclude=exclude)
                    check(got, oracle(st, groups, n, cls, mode, exclude), (cls, mode, ex))
                    for q in range(1, len(groups)):                      # the alternatives' order: identical bits
                        assert np.array_equal(got[0][q], got[0][0]) and np.array_equal(bits(got[1][q]), bits(got[1][0])) and got[2][q] == got[2][0]
                    found = (frozenset(got[0][0, :int(got[2][0])].tolist()), int(got[2][0]))
                    if mode == "all":
                        assert found[1] > 0 and (base is None or base == found), (cls, order)
                        base = found


# ---- 7: saturated signatures: the pair table decides, the mask neither rejects nor accepts wrongly ---------------------------------
def _saturated():
    r = np.random.default_rng(17)
    vocab = ["v%d" % i for i in range(1000)]
    long_docs = [[vocab[int(x)] for x in r.choice(1000, 400, replace=False)] for _ in range(60)]
    docs = [" ".join(w) for w in long_docs] + [" ".join(vocab[int(x)] for x in r.choice(1000, 3, replace=False)) for _ in range(60)]
    groups, ex = [], []
    for i in range(30):
        absent = [w for w in vocab if w not in set(long_docs[i])]
        held = long_docs[i]
        q = [[absent[int(x)] for x in r.choice(len(absent), 1 + i % 9, replace=False)],          # document i holds none of them
             [held[int(x)] for x in r.choice(400, 1 + i % 3, replace=False)] + [absent[int(r.integers(len(absent)))]],
             [vocab[int(x)] for x in r.choice(1000, 1 + i % 20, replace=False)]]
        groups.append(q[:1 + i % 3] if i % 4 else q[1:])
        ex.append("" if i % 3 else vocab[int(r.integers(1000))])
    return docs, groups, ex


def test_saturated_signatures():
    docs, groups, ex = _saturated()
    st = Stats(docs)
    assert max(len(set(d.split())) for d in docs) > 256
    for cls in CLASSES:
        m = model(cls, docs)
        cnt = check_model(m, cls, st, groups, (1, 7, 200), (None, ex), what="saturated")
        assert 0 < cnt["all", 0].sum() < cnt["any", 0].sum()


def test_saturated_signatures_under_forced_hash_collisions():
    docs, groups, ex = _saturated()
    st = Stats(docs)
    ctx = _native.Context()
    _native.debug_set("bm25_hash_bits", 4, ctx)
    for cls in CLASSES:
        m = model(cls, docs, ctx=ctx)
        check_model(m, cls, st, groups, (7,), (None, ex), what="hash bits 4")
        del m
    ctx.close()


# ---- 8: chunks -------------------------------------------------------------------------------------------------------------------
def test_chunking(corpus30k):
    docs = corpus30k
    st = Stats(docs)
    r = np.random.default_rng(23)
    top = sorted(st.post.p, key=lambda w: (-st.post.df(w), w))
    groups, exclude = [], []
    for i in range(40):
        words = list(dict.fromkeys(docs[701 * i].split()))
        query = []
        for g in range(int(r.integers(1, 5))):
            size = (1, 2, 5, 17, 40)[(i + g) % 5]                   # unequal sizes on both sides of every chunk boundary
            alts = [words[int(r.integers(len(words)))]] + [top[int(x)] for x in r.integers(200, 3000, size - 1)]
            query.append(alts)
        if i % 9 == 0:
            query.append([])
        groups.append(query if i % 13 else [])
        exclude.append(top[int(r.integers(0, 50))] if i % 2 == 0 else "")
    base = BM25(docs, B, K1)
    want = {}
    for mode in MODES:
        want[mode] = base.search_groups(groups, 50, match=mode, exclude=exclude)
        check(want[mode], oracle(st, groups, 50, "BM25", mode, exclude), ("default", mode))
    M = int(max(want["any"][2].max(), want["all"][2].max()))
    assert M > 1000 and (want["all"][2] > 0).sum() >= 10
    for chunk in (1, M, 3 * M + 3):
        ctx = _native.Context()
        _native.debug_set("bm25_search_chunk", chunk, ctx)
        m = BM25(docs, B, K1, ctx=ctx)
        for mode in MODES:
            assert same(m.search_groups(groups, 50, match=mode, exclude=exclude), want[mode]), (chunk, mode)
            assert np.array_equal(m.count_groups(groups, match=mode, exclude=exclude), want[mode][2]), (chunk, mode)
        del m
        ctx.close()


# ---- 9: empty shapes -----------------------------------------------------------------------------------------------------------------
def test_empty_shapes():
    docs = ["a b", "b c", "c d", "a a", ""]
    st = Stats(docs)
    for cls in CLASSES:
        m = model(cls, docs)
        for mode in MODES:
            assert [x.shape for x in m.search_groups([], 3, match=mode)] == [(0, 3), (0, 3), (0,)]
            assert [x.shape for x in m.search_groups([], 10 ** 9, match=mode, exclude=[])] == [(0, 5), (0, 5), (0,)]
            assert m.count_groups([], match=mode).shape == (0,)
        assert m.group_df([]) == [] and m.group_df([[], [[]]]) == [[], [0]] and m.expand([]) == [] and m.expand(["", "  "]) == [[], []]
        groups = [[], [[]], [["a", "c"]], [[], []], [["a"], ["b", "d"]]]
        check_model(m, cls, st, groups, (1, 5, 9), (None, ["", "", "d", "", ""]), what="empty")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            e = model(cls, [])
        ids, sc, cnt = e.search_groups([[["a", "b"]], []], 4, match="all", exclude=["b", ""])
        assert ids.shape == (2, 0) and sc.shape == (2, 0) and cnt.tolist() == [0, 0]
        assert e.count_groups([[["a", "b"]], []]).tolist() == [0, 0] and e.group_df([[["a", "b"]]]) == [[0]]
        assert e.expand(["a b"], prefix_last=True) == [[["a"], ["b"]]]
        assert e.search_fuzzy(["a b"], 3)[2].tolist() == [0]


# ---- 10: the states of the index ------------------------------------------------------------------------------------------------------
def test_index_states():
    r = np.random.default_rng(11)
    vocab, docs = synthetic(700, 60, 12)
    docs[10] = "solo w1"
    docs[400] = "solo solo"
    more = [" ".join(vocab[int(x)] for x in r.integers(0, 60, 5)) for _ in range(130)] + ["fresh w2", "solo again"]
    groups = [[["w1", "solo"]], [["w2", "w3"], ["fresh", "w4"]], [["solo", "again"], ["w1", "w5", "w6"]], [["fresh"]], [],
              [["w7", "w8", "w9", "absent"], ["w10"], ["w11", "w7"]]]
    exclude = ["w2", "", "w9", "", "w1", "w12 fresh"]
    for cls in CLASSES:
        m = model(cls, docs)
        cur = list(docs)

        def agree(what):
            f = model(cls, cur)
            st = Stats(cur)
            for mode in MODES:
                for k in (1, 200):
                    got = m.search_groups(groups, k, match=mode, exclude=exclude)
                    assert same(got, f.search_groups(groups, k, match=mode, exclude=exclude)), (cls, what, mode, k)
                    check(got, oracle(st, groups, k, cls, mode, exclude), (cls, what, mode, k))
            assert m.group_df(groups) == f.group_df(groups) == [[df for _, df, _ in group_rows(st, q)] for q in groups], (cls, what)

        m.search_groups(groups, 5, match="all")                           # (fills the cache of the groups' idf: a change must drop it)
        m.add_documents(more)
        cur += more
        agree("add")
        gone = sorted({int(x) for x in r.integers(0, len(cur), 90)} | {10, 400, len(cur) - 1})     # every document of "solo"
        m.remove_documents(gone)
        cur = [d for i, d in enumerate(cur) if i not in set(gone)]
        agree("remove")
        assert m.count_groups([[["solo"]], [["solo", "again"]]]).tolist() == [0, 0]
        m.compact()
        agree("compact")


# ---- 11: the C entry points: the device form and the guards -----------------------------------------------------------------------------
def test_device_form_and_guards(corpus30k):
    docs = corpus30k[:5000]
    st = Stats(docs)
    r = np.random.default_rng(9)
    vocab = sorted({w for d in docs[:300] for w in d.split()})
    groups = []
    for i in range(14):
        words = docs[37 * i].split()
        groups.append([[words[g % len(words)]] + [vocab[int(x)] for x in r.integers(0, len(vocab), (i + g) % 4)] for g in range(1 + i % 3)])
    groups += [[], [["nowhere"]]]
    exclude = [vocab[int(r.integers(len(vocab)))] if i % 2 else "" for i in range(len(groups))]
    ctx = _native.Context()
    m = BM25(docs, B, K1, ctx=ctx)
    nq = len(groups)
    at, ao, go, _, idf = m._group_pack(groups)
    xt, xo = m._exclusions(exclude, nq)
    P = m._params()
    g = 256
    for plus, cls in ((False, "BM25"), (True, "BM25Plus")):
        P[5] = DELTA if plus else 0.0
        for mode, k in ((1, 1), (1, 10), (0, 10), (1, 300)):
            host = ctx.bm25_search_groups(m._index, at, ao, idf, go, P, plus, k, mode=mode, ex_terms=xt, ex_off=xo)
            check(host, oracle(st, groups, k, cls, MODES[mode], exclude), (plus, mode, k))
            sizes = (nq * k * 8, nq * k * 8, nq * 8)
            dev = [ctx.alloc(nb + 2 * g) for nb in sizes]
            for d, nb in zip(dev, sizes):
                ctx.h2d(d, np.full(nb + 2 * g, 0xA5, np.uint8))
            ctx.bm25_search_groups(m._index, at, ao, idf, go, P, plus, k, mode=mode, ex_terms=xt, ex_off=xo, d_ids=dev[0] + g,
                                   d_scores=dev[1] + g, d_counts=dev[2] + g)
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
    # absolute offsets: the same groups behind one other group of three entries, which no query names
    at2, ao2, go2 = np.concatenate([[5, 5, 5], at]).astype(np.int32), np.concatenate([[0], ao + 3]), go + 1
    idf2 = np.concatenate([[9.0], idf])
    assert same(ctx.bm25_search_groups(m._index, at2, ao2, idf2, go2, P, True, 10, mode=1, ex_terms=xt, ex_off=xo),
                ctx.bm25_search_groups(m._index, at, ao, idf, go, P, True, 10, mode=1, ex_terms=xt, ex_off=xo))
    assert np.array_equal(ctx.bm25_match_count_groups(m._index, at2, ao2, go2, mode=1), ctx.bm25_match_count_groups(m._index, at, ao, go, mode=1))

    lib, vp = ctx.lib, ctypes.c_void_p
    n_terms = ctx.bm25_info(m._index)[1]
    Pa = np.array(P)
    ids, sc, cnt = np.full((2, 4), 77, np.int64), np.full((2, 4), 7.5), np.full(2, 77, np.int64)
    d_out = [ctx.alloc(2 * 4 * 8), ctx.alloc(2 * 4 * 8), ctx.alloc(2 * 8)]
    for d in d_out:
        ctx.h2d(d, np.full(64, 0xA5, np.uint8)[:2 * 8 if d is d_out[2] else 64])

    def ptr(a):
        return None if a is None else vp(a.ctypes.data)

    def raw_call(form, at=(0, 1, -1), ao=(0, 2, 3), gi=(1.0, 2.0), go=(0, 1, 2), nqq=2, k=4, mode=1, xt=None, xo=None, params=Pa, outs=True):
        at = None if at is None else np.array(at, np.int32)
        ao = None if ao is None else np.array(ao, np.int64)
        gi = None if gi is None else np.array(gi, np.float64)
        go = None if go is None else np.array(go, np.int64)
        xt = None if xt is None else np.array(xt, np.int32)
        xo = None if xo is None else np.array(xo, np.int64)
        if form == "count":
            return lib.gz_bm25_match_count_groups(vp(m._index), ptr(at), ptr(ao), ptr(go), nqq, mode, ptr(xt), ptr(xo), ptr(cnt) if outs else None)
        fn = lib.gz_bm25_search_groups if form == "host" else lib.gz_bm25_search_groups_device
        o = [ptr(ids), ptr(sc), ptr(cnt)] if form == "host" else [vp(d) for d in d_out]
        return fn(vp(m._index), ptr(at), ptr(ao), ptr(gi), ptr(go), nqq, ptr(params), 0, k, mode, ptr(xt), ptr(xo), *(o if outs else [None] * 3))

    def untouched():
        if not ((ids == 77).all() and (sc == 7.5).all() and (cnt == 77).all()):
            return False
        ctx.sync()
        for d in d_out:
            x = np.empty(2 * 8 if d is d_out[2] else 64, np.uint8)
            ctx.d2h(x, d)
            if not (x == 0xA5).all():
                return False
        return True

    E = _native.GZ_E_INVALID
    for form in ("host", "device", "count"):
        bad = [dict(go=None), dict(ao=None), dict(at=None), dict(go=(0, 2, 1)), dict(go=(-1, 1, 2)), dict(ao=(0, 3, 2)), dict(ao=(-1, 2, 3)),
               dict(at=(0, n_terms, 1)), dict(at=(0, -2, 1)), dict(mode=2), dict(mode=-1), dict(nqq=-1), dict(outs=False),
               dict(xt=[0], xo=[0, 2, 1]), dict(xt=None, xo=[0, 1, 1]), dict(xt=[n_terms], xo=[0, 1, 1])]
        if form != "count":
            bad += [dict(k=0), dict(k=-3), dict(gi=None), dict(params=None)]
        for kw in bad:
            assert raw_call(form, **kw) == E, (form, kw)
        wide = list(range(65)) + [3, -1]                              # 65 distinct terms in the second group
        assert raw_call(form, at=wide, ao=(0, 0, 67)) == _native.GZ_E_LIMIT, form
        if form != "count":
            assert raw_call(form, k=1025) == _native.GZ_E_LIMIT, form
    assert untouched()
    assert raw_call("host", at=list(range(64)) + [3, -1], ao=(0, 1, 66)) == _native.GZ_OK and cnt[0] == st.post.df(m.vocabulary()[0][0]) > 0
    assert raw_call("count", mode=0) == _native.GZ_OK
    for d in d_out:
        ctx.free(d)
    check(m.search_groups(groups, 10, match="all", exclude=exclude), oracle(st, groups, 10, "BM25", "all", exclude), "after the refusals")
    del m
    ctx.close()


# ---- 12: allocation failures ---------------------------------------------------------------------------------------------------------
def test_allocation_failure_sweep(corpus30k):
    docs = corpus30k[:5000]
    st = Stats(docs)
    groups = [[docs[97 * i + g].split()[:1 + (i + g) % 3] for g in range(1 + i % 3)] for i in range(24)] + [[], [["nowhere", "at"], ["all"]]]
    exclude = [docs[97 * i + 5].split()[0] if i % 2 else "" for i in range(len(groups))]

    def sweep(grouped):
        fresh = _native.Context()                 # (no postings, no search workspace yet; the default chunk: one run of rows)
        m = BM25(docs, B, K1, ctx=fresh)
        topk = m.top_k(["nowhere", docs[3]], 40)
        flat = [" ".join(a for g in q for a in g) for q in groups]
        nq, terms, idf, qoff = m._queries(flat)
        at, ao, go, _, gidf = m._group_pack(groups)
        xt, xo = m._exclusions(exclude, len(groups))
        P = m._params()
        ok, failed = None, 0
        for k in range(1, 1000):
            _native.debug_set("inject_bad_alloc", k, fresh)
            try:
                if grouped:
                    got = fresh.bm25_search_groups(m._index, at, ao, gidf, go, P, False, 40, mode=1, ex_terms=xt, ex_off=xo)
                else:
                    got = fresh.bm25_search(m._index, terms, idf, qoff, P, False, 40, mode=1, ex_terms=xt, ex_off=xo)
            except _native.GzError as e:
                assert e.code == _native.GZ_E_NOMEM, (k, e)
                failed += 1
                _native.debug_set("inject_bad_alloc", 0, fresh)
                again = m.top_k(["nowhere", docs[3]], 40)                # context and index stay usable
                assert np.array_equal(again[0], topk[0]) and np.array_equal(bits(again[1]), bits(topk[1])), k
                continue
            ok = k
            break
        _native.debug_set("inject_bad_alloc", 0, fresh)
        assert ok is not None
        if grouped:
            want = oracle(st, groups, 40, "BM25", "all", exclude)
            check(got, want, "after the sweep")
            check(m.search_groups(groups, 40, match="all", exclude=exclude), want)
            assert want[2].any()
        del m
        fresh.close()
        return failed

    plain, grouped = sweep(False), sweep(True)
    print("failing steps: boolean search", plain, "grouped search", grouped)
    assert plain > 10 and grouped >= plain + 5                           # the host packing and the groups' four buffers are reached


# ---- 13: the front ends ------------------------------------------------------------------------------------------------------------------
def lev(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def expand_oracle(m, queries, max_edits=1, limit=8, only_unknown=True, prefix_last=False):
    V, DF = m.vocabulary()
    DF = DF.tolist()
    held = set(V)

    def similar(w):
        d = [(lev(w, v), -DF[i], i) for i, v in enumerate(V)]
        return [V[i] for e, _, i in sorted(x for x in d if x[0] <= max_edits)[:limit]]

    def prefix(w):
        return [V[i] for _, i in sorted((-DF[i], i) for i, v in enumerate(V) if v.startswith(w))[:limit]]

    out = []
    for q in queries:
        ws = q.split()
        gs = []
        for i, w in enumerate(ws):
            if prefix_last and i == len(ws) - 1:
                g = (([w] if w in held else []) + [v for v in prefix(w) if v != w])[:limit]
            elif max_edits == 0 or (only_unknown and w in held):
                g = [w]
            else:
                g = similar(w)
            gs.append(g or [w])
        out.append(gs)
    return out


VI = ["công nghệ thông tin", "công nghệ mới", "cộng nghệ", "công nhân nhà máy", "nghệ thuật", "conh nghệ thông tin", "thông tin mới",
      "công nghệ công nghệ sinh học", "cong", "nghe nhạc", "nhà máy mới", "tin tức công nghệ", "nghề nghiệp", "máy tính", "công ty công nghệ"]


def test_expand_and_group_df():
    docs = VI * 3 + ["thêm công nghệ", "tin"]
    queries = ["cong nghe", "công nghe thong", "nghê", "", "máy tin cong", "xyzxyz nghệ", "c", "công ngh", "tin t"]
    for cls in CLASSES:
        m = model(cls, docs)
        m.add_documents(["máy giặt mới", "côngg nghệ", "tín hiệu"])
        m.remove_documents([8, 13])                               # "cong" stays in the other copies, the state is uncompacted
        cur = [d for i, d in enumerate(docs + ["máy giặt mới", "côngg nghệ", "tín hiệu"]) if i not in (8, 13)]
        for state in ("uncompacted", "compacted"):
            if state == "compacted":
                m.compact()
            st = Stats(cur)
            for kw in (dict(), dict(max_edits=2, limit=3), dict(max_edits=1, limit=64, only_unknown=False), dict(prefix_last=True),
                       dict(max_edits=2, limit=2, only_unknown=False, prefix_last=True), dict(max_edits=0), dict(limit=1)):
                got = m.expand(queries, **kw)
                assert got == expand_oracle(m, queries, **kw), (cls, state, kw)
                assert m.group_df(got) == [[df for _, df, _ in group_rows(st, q)] for q in got], (cls, state, kw)
            assert m.expand(["cong nghe"], max_edits=0) == [[["cong"], ["nghe"]]]
            g = m.expand(["zong nghê"])[0]
            assert g[0] == ["cong"] and set(g[1]) == {"nghệ", "nghề", "nghe"} and g[1][0] == "nghệ", g


def test_search_fuzzy():
    docs = [d for d in VI if d not in ("cong", "nghe nhạc")] + ["tin học", "công"]     # neither "cong" nor "nghe" is a word of it
    st = Stats(docs)
    for cls in CLASSES:
        m = model(cls, docs)
        for kw in (dict(), dict(max_edits=2, limit=4), dict(prefix_last=True), dict(only_unknown=False, match="all"),
                   dict(match="all", exclude=["sinh", "", "mới"])):
            queries = ["cong nghe", "thong tin", "công ngh"]
            groups = expand_oracle(m, queries, **{k: v for k, v in kw.items() if k not in ("match", "exclude")})
            got = m.search_fuzzy(queries, 20, **kw)
            check(got, oracle(st, groups, 20, cls, kw.get("match", "any"), kw.get("exclude")), (cls, kw))
        ids, sc, cnt = m.search_fuzzy(["cong nghe"], 20)
        want = oracle(st, [[["công", "cộng", "conh"], ["nghệ", "nghề"]]], 20, cls)
        check((ids, sc, cnt), want, cls)
        found = ids[0, :int(cnt[0])].tolist()
        assert set(found) == {i for i, d in enumerate(docs) if set(d.split()) & {"công", "cộng", "conh", "nghệ", "nghề"}}
        # the document with the rare misspelling alone ("conh nghệ thông tin") shares its group's df: it ranks below the
        # documents that hold the correct words more often, exactly where the oracle puts it
        assert found.index(docs.index("conh nghệ thông tin")) > found.index(docs.index("công nghệ công nghệ sinh học"))
        qs = ["công nghệ", "nghe cong", "", "máy tính mới"]
        for mode in MODES:
            assert same(m.search_fuzzy(qs, 5, max_edits=0, match=mode, exclude=["", "tin", "", "nhà"]),
                        m.search(qs, 5, match=mode, exclude=["", "tin", "", "nhà"])), (cls, mode)
