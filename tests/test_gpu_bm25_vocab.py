"""GPU: BM25.similar_words / prefix_words / term_texts / suggest / complete / correct, gz_bm25_similar / gz_bm25_prefix /
gz_bm25_term_bytes (csrc/gz_vocab.inc).  The oracle is plain Python: a two-row Levenshtein over str (code points; a lone surrogate is
one), str.startswith, and sorted() by (distance, -df, id) over bm25_oracles.vocab_oracle(documents) -- the words in first-occurrence
order with their document frequencies.  Everything is compared with ==: ids, distances, dfs, counts, padding, strings."""
import random
import warnings

import numpy as np
import pytest

from bm25_oracles import bits, vocab_oracle
from genz_tokenize import _native
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

ALPHA = ["a", "b", "c", "ô", "ộ", "\U0001F600", "\ud800"]      # 1, 1, 1, 2, 3, 4 bytes and a lone surrogate (3 bytes)
TONED = ["cong", "công", "cộng", "cơm", "cõm", "cô", "com", "nghe", "nghệ", "nghề", "co"]
TIE = "0123456789ABCDEFGHIJKL"                                             # 22 terms per group


def rand_word(r, n):
    return "".join(r.choice(ALPHA) for _ in range(n))


def make_corpus(n_random, seed):
    """(documents, the special terms by name): every term in a known number of documents, the documents of five words"""
    r = random.Random(seed)
    special = {n: rand_word(r, n) for n in (31, 32, 33, 63, 64, 65, 200)}
    special[1], special[2] = "b", "ộ\ud800"
    special["1024 bytes"] = "\U0001F600" * 256
    assert len(special["1024 bytes"].encode("utf-8")) == 1024
    terms = dict.fromkeys(special.values())
    terms.update(dict.fromkeys(TONED))
    while len(terms) < len(special) + len(TONED) + n_random:
        terms[rand_word(r, r.randint(1, 6))] = None
    df = {t: r.randint(1, 4) for t in terms}
    df["công"], df["cong"] = 9, 2
    for c in TIE:                                                          # same distance to "tie?" / "une?": equal df, unequal df
        df["tie" + c] = 2
        df["une" + c] = 1 + TIE.index(c) % 5
    slots = [t for t, n in df.items() for _ in range(n)]
    r.shuffle(slots)
    docs = [" ".join(slots[i:i + 5]) for i in range(0, len(slots), 5)]
    return docs, special


def lev(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


_DIST = {}


def ed(a, b):
    d = _DIST.get((a, b))
    if d is None:
        d = _DIST[(a, b)] = lev(a, b)
    return d


def similar_oracle(docs, words, max_edits, k):
    V, DF = vocab_oracle(docs)
    kk = min(k, len(V))
    ids, dist, df, counts = [], [], [], []
    for w in words:
        m = sorted((ed(w, t), -DF[i], i) for i, t in enumerate(V) if ed(w, t) <= max_edits)
        counts.append(len(m))
        m = m[:kk]
        pad = kk - len(m)
        ids.append([x[2] for x in m] + [-1] * pad)
        dist.append([x[0] for x in m] + [-1] * pad)
        df.append([-x[1] for x in m] + [0] * pad)
    return ids, dist, df, counts


def prefix_oracle(docs, prefixes, k):
    V, DF = vocab_oracle(docs)
    kk = min(k, len(V))
    ids, df, counts = [], [], []
    for p in prefixes:
        m = sorted((-DF[i], i) for i, t in enumerate(V) if t.startswith(p))
        counts.append(len(m))
        m = m[:kk]
        pad = kk - len(m)
        ids.append([x[1] for x in m] + [-1] * pad)
        df.append([-x[0] for x in m] + [0] * pad)
    return ids, df, counts


def check_similar(got, docs, words, max_edits, k, what=""):
    ids, dist, df, counts = got
    T = len(vocab_oracle(docs)[0])
    assert ids.dtype == np.int64 and dist.dtype == np.int32 and df.dtype == np.int32 and counts.dtype == np.int64, what
    assert ids.shape == dist.shape == df.shape == (len(words), min(k, T)) and counts.shape == (len(words),), what
    want = similar_oracle(docs, words, max_edits, k)
    for w in range(len(words)):
        assert counts[w] == want[3][w], (what, words[w], "count")
        assert ids[w].tolist() == want[0][w], (what, words[w], "ids")
        assert dist[w].tolist() == want[1][w], (what, words[w], "dist")
        assert df[w].tolist() == want[2][w], (what, words[w], "df")
    return want


def check_prefix(got, docs, prefixes, k, what=""):
    ids, df, counts = got
    T = len(vocab_oracle(docs)[0])
    assert ids.dtype == np.int64 and df.dtype == np.int32 and counts.dtype == np.int64, what
    assert ids.shape == df.shape == (len(prefixes), min(k, T)) and counts.shape == (len(prefixes),), what
    want = prefix_oracle(docs, prefixes, k)
    assert counts.tolist() == want[2], what
    assert ids.tolist() == want[0], what
    assert df.tolist() == want[1], what
    return want


def swap_ends(w):
    return "Z" + w[1:-1] + "Y"


@pytest.fixture(scope="module")
def big():
    """(documents, special terms, model, query words): T > 1024 terms"""
    docs, special = make_corpus(1100, 7)
    V = vocab_oracle(docs)[0]
    assert 1024 < len(V) <= 1400
    assert [len(special[n]) for n in (1, 2, 63, 64, 65, 200)] == [1, 2, 63, 64, 65, 200] and all(t in V for t in special.values())
    r = random.Random(11)
    words = ["", "a", "b", "q", "\ud800", "cong", "công", "côgn", "nghệ", "nghee", "tie?", "une?", "xyzxyzxyz",
             special[32][:-1], special[32], special[32][:16] + "q" + special[32][16:],      # 31, 32 (a term), 33 code points
             special[63], swap_ends(special[63]), special[64], swap_ends(special[64]),        # both ends of the state word
             special[64][1:], special[65][:64], special[65][1:], rand_word(r, 64), rand_word(r, 63), "z" * 64,
             rand_word(r, 3), rand_word(r, 4), rand_word(r, 5) + "q", "\U0001F600" * 64]
    assert sorted({len(w) for w in words} & {0, 1, 31, 32, 33, 63, 64}) == [0, 1, 31, 32, 33, 63, 64] and len(words) <= 40
    return docs, special, BM25(docs), words


def test_similar_words_edits_and_k(big):
    docs, special, m, words = big
    V, DF = vocab_oracle(docs)
    got_v, got_df = m.vocabulary()
    assert got_v == V and got_df.tolist() == DF
    for max_edits, k in ((0, 10), (1, 10), (2, 1), (2, 10), (3, 10), (2, 1024), (64, 10), (64, 1024)):
        want = check_similar(m.similar_words(words, max_edits, k), docs, words, max_edits, k, (max_edits, k))
        counts = dict(zip(words, want[3]))
        if max_edits == 0:                                                 # _lookup's answer and df
            terms, df = m._lookup(words)
            for w, t, d, row, drow in zip(words, terms.tolist(), df.tolist(), want[0], want[2]):
                assert (t >= 0) == (w in V) and ((row[0], drow[0]) == (V.index(w), d) if t >= 0 else counts[w] == 0), w
        if max_edits == 2:
            assert counts["tie?"] >= 22 and counts["une?"] >= 22 and counts["xyzxyzxyz"] == 0 and 0 < counts["nghee"] < 10
            assert counts[swap_ends(special[64])] == 1 and counts[swap_ends(special[63])] == 1
        if max_edits == 64:
            assert counts["a"] > 1024 and counts[""] > 1024
    # the defaults
    got = m.similar_words(words[:6])
    want = m.similar_words(words[:6], 2, 10)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_limits_leave_the_index_answering(big):
    docs, special, m, words = big
    before = m.similar_words(words[:8], 2, 10)
    scores = bits(m.get_scores(["cong b", "công a"]))
    with pytest.raises(_native.GzError) as e:
        m.similar_words(["a", special[65]], 2, 10)                         # 65 code points
    assert e.value.code == _native.GZ_E_LIMIT
    with pytest.raises(_native.GzError) as e:
        m.similar_words(["a"], 2, 1025)                                    # k' = 1025 <= T
    assert e.value.code == _native.GZ_E_LIMIT
    with pytest.raises(_native.GzError) as e:
        m.prefix_words(["a"], 5000)
    assert e.value.code == _native.GZ_E_LIMIT
    after = m.similar_words(words[:8], 2, 10)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(bits(m.get_scores(["cong b", "công a"])), scores)


def test_small_index_k_above_T_and_a_word_longer_than_every_term():
    docs = ["ab abc b", "abc ô ôb", "b"]
    m = BM25Plus(docs)
    words = ["a" * 64, "ab", "", "ô" * 7, "abd"]
    for max_edits in (0, 2, 5, 64):
        check_similar(m.similar_words(words, max_edits, 10), docs, words, max_edits, 10, max_edits)     # k' = T = 5
    check_prefix(m.prefix_words(["", "a", "ab", "abcd", "ô", "x"], 10), docs, ["", "a", "ab", "abcd", "ô", "x"], 10)
    for got in (m.similar_words([], 2, 3), m.prefix_words([], 3)):
        assert got[0].shape == (0, 3) and got[-1].shape == (0,)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        empty = BM25([])
    ids, dist, df, counts = empty.similar_words(["a", ""], 2, 10)
    assert ids.shape == dist.shape == df.shape == (2, 0) and counts.tolist() == [0, 0]
    ids, df, counts = empty.prefix_words(["a", ""], 10)
    assert ids.shape == df.shape == (2, 0) and counts.tolist() == [0, 0]
    assert empty.suggest(["a"]) == [[]] and empty.complete([""]) == [[]] and empty.correct(["a  b", ""]) == ["a b", ""]


def test_chunks_and_tiles_give_the_same_answer(big):
    docs, special, m, words = big
    T = len(vocab_oracle(docs)[0])
    five = ["cong", "tie?", "", special[64], "xyzxyzxyz"]
    pre = ["", "c", "tie", "cô", "nope"]
    want_s = [m.similar_words(five, e, k) for e, k in ((2, 10), (64, 1024))]
    want_p = m.prefix_words(pre, 30)
    check_similar(want_s[0], docs, five, 2, 10)
    for chunk, tile in ((2 * T, 0), (1 << 23, 64), (2 * T + 5, 100), (1, 256)):      # 2 rows a chunk: 3 chunks; a tile < T; one row a chunk
        ctx = _native.Context()
        _native.debug_set("bm25_vocab_chunk", chunk, ctx)
        _native.debug_set("bm25_topk_tile", tile, ctx)
        m2 = BM25(docs, ctx=ctx)
        got = [m2.similar_words(five, e, k) for e, k in ((2, 10), (64, 1024))]
        for a, b in zip(got, want_s):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (chunk, tile)
        assert all(np.array_equal(x, y) for x, y in zip(m2.prefix_words(pre, 30), want_p)), (chunk, tile)
        del m2
        ctx.close()


def test_prefix_words(big):
    docs, special, m, words = big
    V = vocab_oracle(docs)[0]
    prefixes = ["", "c", "ô", "\ud800", "cô", "cong", "công", "tie", "une", special[200], special[200] + "x",
                special["1024 bytes"], special["1024 bytes"] + "\U0001F600", "\U0001F600", "zz", special[64][:40]]
    assert "cơm" in V and "cõm" in V and "cõm".encode()[:2] == "cô".encode()[:2]                  # (õ and ô share their lead byte)
    for k in (1, 10, 1024):
        want = check_prefix(m.prefix_words(prefixes, k), docs, prefixes, k, k)
        counts = dict(zip(prefixes, want[2]))
        assert counts[""] == len(V) and counts[special[200] + "x"] == 0 and counts[special["1024 bytes"]] == 1 and counts["tie"] == 22
        if k == 10:
            row = want[0][prefixes.index("cô")]
            assert V.index("cơm") not in row and V.index("cõm") not in row and V.index("công") in row and 0 < counts["cong"] < 10
    got = m.prefix_words(prefixes[:4])
    assert all(np.array_equal(a, b) for a, b in zip(got, m.prefix_words(prefixes[:4], 10)))


def test_term_texts(big):
    docs, special, m, words = big
    V = vocab_oracle(docs)[0]
    r = random.Random(3)
    ids = [r.randrange(-1, len(V)) for _ in range(300)] + [-1, -1, V.index(special["1024 bytes"]), V.index("ộ\ud800"),
                                                           V.index(special[200]), V.index(special["1024 bytes"]), 0, len(V) - 1]
    r.shuffle(ids)
    name = lambda i: "" if i < 0 else V[i]                                 # noqa: E731
    assert m.term_texts(ids) == [name(i) for i in ids]
    a = np.array(ids[:300], dtype=np.int32).reshape(20, 15)
    assert m.term_texts(a) == [[name(i) for i in row] for row in a.tolist()]
    nested = [[ids[0], [ids[1], ids[2]]], [], [[-1]], ids[3]]
    assert m.term_texts(nested) == [[name(ids[0]), [name(ids[1]), name(ids[2])]], [], [[""]], name(ids[3])]
    assert m.term_texts([]) == [] and m.term_texts(np.zeros((2, 0), dtype=np.int64)) == [[], []] and m.term_texts([-1, -1]) == ["", ""]
    with pytest.raises(IndexError):
        m.term_texts([0, len(V)])
    with pytest.raises(IndexError):
        m.term_texts([-2])
    # the C entry point's own checks: a capacity too small writes nothing, an id out of range
    lib, C = m._ctx.lib, _native.C
    arr = np.array([0, 1], dtype=np.int64)
    off = np.full(3, -7, dtype=np.int64)
    data = np.full(4096, 0xEE, dtype=np.uint8)
    n = len(V[0].encode("utf-8", "surrogatepass")) + len(V[1].encode("utf-8", "surrogatepass"))
    assert lib.gz_bm25_term_bytes(C.c_void_p(m._index), C.c_void_p(arr.ctypes.data), 2, C.c_void_p(off.ctypes.data),
                                  C.c_void_p(data.ctypes.data), n - 1) == _native.GZ_E_CAPACITY
    assert off.tolist() == [-7] * 3 and data.tolist() == [0xEE] * 4096
    arr[1] = len(V)
    assert lib.gz_bm25_term_bytes(C.c_void_p(m._index), C.c_void_p(arr.ctypes.data), 2, C.c_void_p(off.ctypes.data), None, 0) == _native.GZ_E_INVALID
    bad = np.frombuffer(b"a\xffb", dtype=np.uint8)
    woff = np.array([0, 3], dtype=np.int64)
    with pytest.raises(_native.GzError) as e:
        m._ctx.bm25_similar(m._index, bad, woff, 2, 3)
    assert e.value.code == _native.GZ_E_INVALID


def test_suggest_complete_correct(big):
    docs, special, m, words = big
    V, DF = vocab_oracle(docs)
    ws = ["cong", "côgn", "xyzxyzxyz", "tie?", ""]
    ids, dist, df, counts = similar_oracle(docs, ws, 2, 5)
    assert m.suggest(ws, 2, 5) == [[(V[i], d, f) for i, d, f in zip(ids[w], dist[w], df[w]) if i >= 0] for w in range(len(ws))]
    assert m.suggest(ws[:2]) == m.suggest(ws[:2], 2, 10)
    ps = ["cô", "tie", "nope", ""]
    ids, df, counts = prefix_oracle(docs, ps, 4)
    assert m.complete(ps, 4) == [[(V[i], f) for i, f in zip(ids[w], df[w]) if i >= 0] for w in range(len(ps))]
    assert m.complete(ps[:2]) == m.complete(ps[:2], 10)
    queries = ["  cong   nghệ  côgn", "xyzxyzxyz tie? b", "", " \n ", "nghee cong nghee"]
    for max_edits in (0, 1, 2):
        want = []
        for q in queries:
            out = []
            for w in q.split():
                best = similar_oracle(docs, [w], max_edits, 1)
                out.append(w if w in V or not best[3][0] else V[best[0][0][0]])
            want.append(" ".join(out))
        assert m.correct(queries, max_edits) == want, max_edits
    fixed = m.correct(queries)
    assert fixed == m.correct(queries, 2) and fixed[2] == "" and fixed[3] == ""
    assert fixed[0].split()[:2] == ["cong", "nghệ"] and fixed[1].split()[0] == "xyzxyzxyz" and fixed[1].split()[2] == "b"


@pytest.mark.parametrize("positions", [False, True])
def test_every_state_of_the_index(positions):
    docs, special = make_corpus(150, 5)
    docs.append("lastword cong")                                           # a term whose only document goes
    r = random.Random(9)
    words = ["", "a", "cong", "côgn", "tie?", "une?", "lastword", "lastwork", special[64], swap_ends(special[64]), special[32][:-1],
             rand_word(r, 3)]
    prefixes = ["", "c", "cô", "last", "une", "\ud800"]
    queries = ["cong công b", "lastword a"]
    m = BM25(docs, positions=positions)
    cur = list(docs)

    def verify(what):
        V = vocab_oracle(cur)[0]
        before = bits(m.get_scores(queries))
        for max_edits, k in ((1, 10), (2, 40), (64, 300)):
            check_similar(m.similar_words(words, max_edits, k), cur, words, max_edits, k, (what, max_edits, k))
        check_prefix(m.prefix_words(prefixes, 25), cur, prefixes, 25, what)
        ids = list(range(len(V) - 1, -1, -7)) + [-1]
        assert m.term_texts(ids) == [V[i] if i >= 0 else "" for i in ids], what
        assert np.array_equal(bits(m.get_scores(queries)), before), what   # the index was only read
        return V

    V = verify("fresh")
    assert "lastword" in V
    gone = sorted({len(docs) - 1, 0, 3, 10, 11, 12, 40})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.remove_documents(gone)
    cur = [d for i, d in enumerate(cur) if i not in gone]
    V2 = verify("removed")
    assert "lastword" not in V2 and m.similar_words(["lastword"], 0, 1)[3].tolist() == [0]
    more = ["lastword newterm công", "newterm tieZ a", special[63] + "q b"]
    m.add_documents(more)
    cur += more
    V3 = verify("appended")
    assert "newterm" in V3 and "lastword" in V3
    m.compact()
    assert verify("compacted") == V3
    ids = m.similar_words(["newterm", "tieZ"], 0, 1)[0][:, 0].tolist()
    assert ids == m._lookup(["newterm", "tieZ"])[0].tolist()               # compacted: the canonical ids are the table's
