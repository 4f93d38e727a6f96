"""GPU: the DOCUMENT side of the BM25 index -- where str.split() cuts, against the 64-byte tiles in which bm_doc_words (csrc/gz_bm25.inc)
walks a document -- the counterpart of test_gpu_bm25_query_shapes.py.  What runs here and nowhere else:
    1, 2  every whitespace code point and every near miss (bm25_oracles.WS, NEAR) starting at every byte of the first two tiles and at
          the start of the third: the carry of a 2- or 3-byte whitespace and of a running word across a tile edge
    3     runs of multi-byte whitespace over whole tiles, whitespace-only documents, words that end or begin on a tile edge, a random mix
    4     documents per workgroup (BM_WPB = 4) with empty documents at every place of a group
    5     more documents than words, across the scan block (4096), fresh, appended to and removed from
    6     the same boundaries through add_documents, remove_documents and compact, also with forced hash collisions
    7     gz_bm25_build_device over text with the start of a 3-byte space in front of the first document and continuation bytes behind the last
    8     terms of every byte length around 16 (BM_CP_SHORT), 64, 128, 256 and 1024, with neighbours that differ in the last byte
    9     word positions (occurrences, phrase, near, cover) when the separators are 2 and 3 bytes wide
Oracles: d.split() for the words, len(d.split()) for fieldLens, first-occurrence order for vocabulary() and df (bm25_oracles.vocab_oracle),
bm25_oracles.restate for the scores, the phrase and near tests' own oracles for theirs.  Everything is compared with == or as uint64 bit
patterns: no tolerance appears anywhere."""
import warnings

import numpy as np
import pytest

import bm25_restate as R
import test_gpu_bm25_near as NR
import test_gpu_bm25_phrase as PH
from bm25_oracles import NEAR, WS, bits, check, decoded, matched, restate, sweep_docs, topk_check, vocab_oracle
from genz_tokenize import _native
from genz_tokenize._packing import pack
from genz_tokenize.ranking import BM25, BM25Plus

pytestmark = pytest.mark.gpu

WS3 = [c for c in WS if len(c.encode()) == 3]
WS2 = [c for c in WS if len(c.encode()) == 2]


def build(docs, positions=True, ctx=None, cls="BM25"):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (np.mean of no fieldLens)
        if cls == "BM25Plus":
            return BM25Plus(docs, 0.3, 2.0, 0.5, ctx=ctx, positions=positions)
        return BM25(docs, ctx=ctx, positions=positions)


def first_diff(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def check_vocabulary(m, docs, what=""):
    words, df = m.vocabulary()
    want_words, want_df = vocab_oracle(docs)
    assert words == want_words, (what, first_diff(words, want_words))
    assert df.dtype == np.int32 and df.tolist() == want_df, (what, first_diff(df.tolist(), want_df))


def check_index(m, docs, what="", compacted=True):
    """fieldLens, every word of every document in order (count, order and byte range), the vocabulary and its df"""
    split = [d.split() for d in docs]
    lens = [len(w) for w in split]
    assert m.num_doc == len(docs) and m.fieldLens == lens, (what, first_diff(m.fieldLens, lens))
    assert m._ctx.bm25_field_lengths(m._index).tolist() == lens, what
    got = decoded(m, compacted=compacted)
    assert got == split, (what, first_diff(got, split))
    check_vocabulary(m, docs, what)
    assert m._ctx.bm25_info(m._index) == (len(docs), len(vocab_oracle(docs)[0]), sum(lens)), what


# ---- 1, 2: the sweep -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    return sweep_docs()


@pytest.fixture(scope="module")
def sweep_positional(sweep):
    return build(sweep)


def test_sweep_positional(sweep, sweep_positional):
    check_index(sweep_positional, sweep, "sweep")


SWEEP_QUERIES = ["x" * 63, "x" * 64, "y", "z", "xxxxx\u200by", "nowhere", "", "x" * 62 + " " + "x" * 65, "x" * 130, "x" * 131,
                 "x" * 63 + "\u3001", "x" * 62 + "\x84y", "\u200b\u200bz", "x" * 127 + "\u1681\u1681z", "y z", "z y x xx",
                 "x" * 64 + "\u3000z", "x" * 63 + "\xa0" + "x" * 63, "\ud800y y", "x" * 126 + "\u2060", "\u3000"]


@pytest.mark.parametrize("cls", ["BM25", "BM25Plus"])
def test_sweep_non_positional(sweep, sweep_positional, cls):
    m = build(sweep, positions=False, cls=cls)
    lens = [len(d.split()) for d in sweep]
    assert m.fieldLens == lens, first_diff(m.fieldLens, lens)
    check_vocabulary(m, sweep, cls)
    info = m._ctx.bm25_info(m._index)
    assert info == (len(sweep), len(vocab_oracle(sweep)[0]), sum(lens))
    assert info == sweep_positional._ctx.bm25_info(sweep_positional._index)
    assert m.fieldLens == sweep_positional.fieldLens and m.vocabulary()[0] == sweep_positional.vocabulary()[0]
    assert np.array_equal(m.vocabulary()[1], sweep_positional.vocabulary()[1])
    # (the queries are worth it: most of them hold a word of the sweep)
    post = R.Postings(m.frequency_word_in_doc)
    assert len(SWEEP_QUERIES) >= 20 and sum(any(w in post.p for w in q.split()) for q in SWEEP_QUERIES) >= 16
    assert post.df("xxxxx\u200by") == 1 and post.df("nowhere") == 0 and post.df("x" * 131) == 0
    S = restate(m, SWEEP_QUERIES, post)
    got = m.get_scores(SWEEP_QUERIES)
    assert got.dtype == np.float64 and got.shape == S.shape
    assert np.array_equal(bits(got), bits(S)), np.flatnonzero((bits(got) != bits(S)).any(axis=1)).tolist()


# ---- 3: runs, whole tiles of whitespace, words on a tile edge ----------------------------------------------------------------------------
def all_whitespace(n):
    """n bytes of whitespace, going round all 29 code points"""
    s, size, i = "", 0, 0
    while size < n:
        c = WS[i % len(WS)]
        if size + len(c.encode()) <= n:
            s, size = s + c, size + len(c.encode())
        i += 1
    return s


def run_docs():
    r = np.random.default_rng(301)
    docs = []
    # runs of 1 .. 200 copies of one 3-byte whitespace between two words
    docs += ["a" + WS3[n % len(WS3)] * n + "b" for n in range(1, 201)]
    docs += ["x" * (n % 5) + "\u3000" * n + "b" for n in range(19, 46)]  # (the run ends at every lane around byte 64 and 128)
    # runs mixing all 29
    for k in range(70):
        run = "".join(WS[int(i)] for i in r.permutation(len(WS)))
        docs += ["x" * k + run + "b", run * 3 + "x" * k, "x" * k + run + run[::-1]]
    # whitespace-only documents
    for n in (63, 64, 65, 128, 192, 193):
        docs += [" " * n, "\u3000" * (n // 3) + " " * (n % 3), " " * (n % 3) + "\u2028" * (n // 3), "\xa0" * (n // 2) + "\t" * (n % 2),
                 "\x1f" * (n % 2) + "\x85" * (n // 2), all_whitespace(n)]
        assert all(len(d.encode()) == n and not d.split() for d in docs[-6:]), n
    # the last word ends exactly at byte 63, 64, 65, 127, 128, 129: no byte behind it; and a document that ends in whitespace there
    for n in (63, 64, 65, 127, 128, 129):
        docs += ["a " + "x" * (n - 2), "a\u3000" + "x" * (n - 4), "a\x85" + "\xe9" * ((n - 3) // 2) + "x" * ((n - 3) % 2),
                 "x" * (n - 2) + " a", "x" * (n - 4) + "\u2003a", "x" * (n - 5) + "\u1680\xa0"]
        assert all(len(d.encode()) == n for d in docs[-6:]), n
    # a word of exactly 64 and of 128 bytes alone in a document
    docs += ["x" * 64, "x" * 128, "\xe9" * 32, "\xe9" * 64, "ệ" * 21 + "x", "ệ" * 42 + "xx", "x" * 63, "x" * 65, "x" * 129, "x" * 192]
    # a word that begins at byte 63, 64 and 65
    for k in (63, 64, 65, 127, 128, 129):
        docs += [" " * k + "word", "x" * (k - 1) + " word", "x" * (k - 3) + "\u3000word", "x" * (k - 2) + "\x85w", "\u2009" * (k // 3) + " " * (k % 3) + "việt",
                 "\t" * (k % 2) + "\xa0" * (k // 2) + "w" * 70]
        assert all(len(d.encode()) - len(d.split()[-1].encode()) == k for d in docs[-6:]), k
    return docs


def mix_docs(n=3000, seed=302):
    r = np.random.default_rng(seed)
    parts = WS + NEAR + ["a", "b", "việt", "x" * 61, "x" * 62, "x" * 63]
    return ["".join(parts[int(i)] for i in r.integers(0, len(parts), int(r.integers(0, 41)))) for _ in range(n)]


@pytest.fixture(scope="module")
def mix():
    return mix_docs()


def test_runs_and_whole_tiles_of_whitespace():
    docs = run_docs()
    assert max(len(d.encode()) for d in docs) > 600 and sum(not d.split() for d in docs) >= 36
    check_index(build(docs), docs, "runs")


def test_random_mix(mix):
    lens = [len(d.encode("utf-8", "surrogatepass")) for d in mix]
    assert len(mix) == 3000 and min(lens) == 0 and max(lens) > 256 and sum(n > 64 for n in lens) > 1000
    assert "" in mix and any(d and not d.split() for d in mix)
    check_index(build(mix), mix, "mix")


# ---- 4: documents per workgroup, empty documents ----------------------------------------------------------------------------------------
def test_documents_per_workgroup_and_empty_documents():
    full = ["w%d\u3000v%d\x85a" % (i, i % 3) for i in range(9)]
    empties = ["", " \u3000\x85\t" * 9]                                    # no bytes; 63 bytes of whitespace
    assert not empties[1].split() and len(empties[1].encode()) == 63
    for n in (1, 2, 3, 4, 5, 8, 9):
        for e, empty in enumerate(empties):
            for p in range(n):
                docs = full[:n]
                docs[p] = empty
                check_index(build(docs), docs, (n, e, p))
                docs = [empties[(e + i) % 2] for i in range(n)]           # the other way round: one document with words
                docs[p] = full[p]
                check_index(build(docs), docs, (n, e, p, "single"))
            docs = [empties[(e + i) % 2] for i in range(n)]
            check_index(build(docs), docs, (n, e, "no words"))
        check_index(build(full[:n]), full[:n], (n, "full"))
    m = build([])
    assert m.num_doc == 0 and m.fieldLens == [] and m.vocabulary()[0] == [] and m._ctx.bm25_info(m._index) == (0, 0, 0)


# ---- 5: more documents than words ---------------------------------------------------------------------------------------------------------
FEW_QUERIES = ["a", "b", "a b", "zz"]
BLANKS = ["", " ", "\u3000", "\x85\t", "", "\u2028\u2029 \xa0", ""]


def check_few(m, docs, what):
    lens = [len(d.split()) for d in docs]
    assert m.num_doc == len(docs) and m.fieldLens == lens, (what, first_diff(m.fieldLens, lens))
    check_vocabulary(m, docs, what)
    assert m._ctx.bm25_info(m._index) == (len(docs), len(vocab_oracle(docs)[0]), sum(lens)), what
    post = R.Postings(m.frequency_word_in_doc)
    S = restate(m, FEW_QUERIES, post)
    got = m.get_scores(FEW_QUERIES)
    assert got.shape == S.shape and np.array_equal(bits(got), bits(S)), what
    assert np.count_nonzero(S[1]) == post.df("b") > 0, what              # (the appended "b" outlives the removal)
    for k in (1, 5):
        topk_check(m.top_k(FEW_QUERIES, k), S, k, (what, k))
        for mode in ("any", "all"):
            check(m.search(FEW_QUERIES, k, match=mode), S, matched(post, FEW_QUERIES, mode), k, (what, mode, k))


@pytest.mark.parametrize("n", [257, 4095, 4096, 4097, 8193])
def test_more_documents_than_words(n):
    docs = [BLANKS[i % len(BLANKS)] for i in range(n)]
    docs[0], docs[n // 2], docs[n - 1] = "a", "b a", "a"
    assert sum(len(d.split()) for d in docs) == 4 < n
    m = build(docs, positions=False)
    check_few(m, docs, (n, "built"))
    more = [BLANKS[(i + 3) % len(BLANKS)] for i in range(4097)] + ["b"]
    m.add_documents(more)
    docs = docs + more
    check_few(m, docs, (n, "appended"))
    m.remove_documents(range(4096))
    docs = docs[4096:]
    assert len(docs) == n + 2 and docs[-1] == "b" and 1 <= sum(len(d.split()) for d in docs) <= 4 < len(docs)
    check_few(m, docs, (n, "removed"))


def test_more_documents_than_words_positional():
    n = 4097
    docs = [BLANKS[i % len(BLANKS)] for i in range(n)]
    docs[0], docs[n // 2], docs[n - 1] = "a", "b a", "a"
    m = build(docs)
    check_index(m, docs, "built")
    m.add_documents([""] * 4097 + ["b"])
    docs = docs + [""] * 4097 + ["b"]
    check_index(m, docs, "appended", compacted=False)
    m.remove_documents(range(4096))
    docs = docs[4096:]
    check_index(m, docs, "removed", compacted=False)
    m.compact()
    check_index(m, docs, "compacted")


# ---- 6: the live index ----------------------------------------------------------------------------------------------------------------------
def live_round(docs, ctx=None, what=""):
    """build a third, append two thirds in two calls, remove every fifth document, compact: the index against split() after every step"""
    n = len(docs) // 3
    texts = list(docs[:n])
    m = build(texts, ctx=ctx)
    check_index(m, texts, (what, "built"))
    for part in (docs[n:2 * n], docs[2 * n:]):
        m.add_documents(part)
        texts += part
        check_index(m, texts, (what, "appended", len(texts)), compacted=False)
    m.remove_documents(range(0, len(texts), 5))
    texts = [t for i, t in enumerate(texts) if i % 5]
    check_index(m, texts, (what, "removed"), compacted=False)
    m.compact()
    check_index(m, texts, (what, "compacted"))
    fresh = build(texts, ctx=ctx)
    assert m._ctx.bm25_info(m._index) == fresh._ctx.bm25_info(fresh._index), what
    a, b = m.term_sequences(), fresh.term_sequences()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    assert m.vocabulary()[0] == fresh.vocabulary()[0] and np.array_equal(m.vocabulary()[1], fresh.vocabulary()[1]), what


def shuffled_sweep(sweep):
    docs = list(sweep)
    np.random.default_rng(601).shuffle(docs)
    return docs


def test_live_index_over_the_sweep(sweep):
    live_round(shuffled_sweep(sweep), what="sweep")


def test_live_index_over_the_sweep_with_forced_collisions(sweep):
    docs = shuffled_sweep(sweep)[:600]
    ctx = _native.Context()
    try:
        _native.debug_set("bm25_hash_bits", 1, ctx)
        live_round(docs, ctx=ctx, what="hash_bits=1")
    finally:
        _native.debug_set("bm25_hash_bits", 0, ctx)
        ctx.close()
    _native.debug_set("bm25_hash_bits", 0)


# ---- 7: a device build between bytes that would complete a whitespace character ---------------------------------------------------------------
@pytest.mark.parametrize("positions", [True, False])
def test_device_build_between_whitespace_fragments(sweep, positions):
    ctx = _native.Context()
    buf, off = pack(sweep)
    host = ctx.bm25_build(buf, off, positions=positions)
    pad = np.array([0xE2, 0x80] * 4, np.uint8)[:7]                       # ... E2 80 | E2: "x" or 80..8A in front would complete a space
    tail = np.array([0x80, 0x80], np.uint8)                              # behind a last document that ends in E2 80 or C2 they would too
    dt, do = ctx.alloc(len(pad) + len(buf) + len(tail)), ctx.alloc(8 * len(off))
    ctx.h2d(dt, np.concatenate([pad, buf, tail]))
    ctx.h2d(do, off + len(pad))
    dev = ctx.bm25_build_device(dt, do, len(sweep), int(off[-1]), positions=positions)
    ctx.free(dt)
    ctx.free(do)
    lens = [len(d.split()) for d in sweep]
    assert ctx.bm25_info(dev) == ctx.bm25_info(host) == (len(sweep), len(vocab_oracle(sweep)[0]), sum(lens))
    assert ctx.bm25_field_lengths(dev).tolist() == ctx.bm25_field_lengths(host).tolist() == lens
    a, b = ctx.bm25_terms(dev), ctx.bm25_terms(host)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    if positions:
        a, b = ctx.bm25_sequence(dev), ctx.bm25_sequence(host)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ctx.bm25_destroy(dev)
    ctx.bm25_destroy(host)
    ctx.close()


def test_device_build_of_documents_that_end_inside_a_whitespace_character():
    """documents cut in the middle of a whitespace character, each followed by the bytes that would complete it: the first byte of the
    next document, or the tail behind the text.  bytes.decode(errors="surrogateescape") makes the str whose split() is the oracle's."""
    raw = [b"a\xe2\x80", b"\x80b", b"c\xe2", b"\x80\x80d", b"e\xc2", b"\x85f", b"x" * 62 + b"\xe2\x80", b"\x83", b"x" * 63 + b"\xc2",
           b"\xa0", b"x" * 61 + b"\xe3\x80", b"\x80", b"g\xe1\x9a"]
    want = [[w.encode("utf-8", "surrogateescape") for w in r.decode("utf-8", "surrogateescape").split()] for r in raw]
    assert want[0] == [raw[0]] and want[1] == [raw[1]] and want[7] == [raw[7]] and all(len(w) == 1 for w in want)
    ctx = _native.Context()
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    buf = np.frombuffer(b"".join(raw), np.uint8)
    pad, tail = np.array([0xE2, 0x80, 0xE2, 0x80, 0xE2, 0x80, 0xE2], np.uint8), np.array([0x80, 0x80], np.uint8)
    dt, do = ctx.alloc(len(pad) + len(buf) + len(tail)), ctx.alloc(8 * len(off))
    ctx.h2d(dt, np.concatenate([pad, buf, tail]))
    ctx.h2d(do, off + len(pad))
    dev = ctx.bm25_build_device(dt, do, len(raw), int(off[-1]), positions=True)
    ctx.free(dt)
    ctx.free(do)
    assert ctx.bm25_field_lengths(dev).tolist() == [1] * len(raw)
    toff, data, df = ctx.bm25_terms(dev)
    data = data.tobytes()
    assert [data[toff[i]:toff[i + 1]] for i in range(len(raw))] == raw and df.tolist() == [1] * len(raw)
    seq = ctx.bm25_sequence(dev)
    assert seq[0].tolist() == list(range(len(raw))) and seq[1].tolist() == list(range(len(raw) + 1))
    ctx.bm25_destroy(dev)
    ctx.close()


# ---- 8: term byte lengths -------------------------------------------------------------------------------------------------------------------
TERM_LENGTHS = list(range(1, 71)) + [127, 128, 129, 130, 255, 256, 257, 1023, 1024, 1025]


def body(n):
    """n bytes of 3-byte, 2-byte and ASCII characters; never ends in a, b, c or !"""
    s = "ệ" * (n // 9) + "\xe9" * (n // 6)
    return s + "q" * (n - len(s.encode()))


def term_words():
    """per length L: three words that share L - 1 bytes and differ in the last, and those L - 1 bytes as a word of their own"""
    words = []
    for L in TERM_LENGTHS:
        words += [body(L - 1) + "a", body(L - 1) + "b", body(L - 1) + "c"] + ([body(L - 1)] if L > 1 else [])
    return words


def term_docs():
    words = term_words()
    r = np.random.default_rng(801)
    docs = []
    for i in range(400):
        pick = [words[int(x)] for x in r.integers(0, len(words), int(r.integers(0, 6)))]
        if i < len(words):
            pick.insert(int(r.integers(0, len(pick) + 1)), words[i])      # every word stands somewhere
        docs.append("".join(w + WS[int(r.integers(0, len(WS)))] for w in pick))
    return docs, words


def check_lookup(m, docs, words, what):
    vocab, df = vocab_oracle(docs)
    df = dict(zip(vocab, df))
    asked = words + [w + "!" for w in words] + ["!" + w for w in words[:40]] + ["nowhere", "q" * 2000]
    ids, got_df = m._lookup(asked)
    ids, got_df = ids.tolist(), got_df.tolist()
    for w, i, f in zip(asked, ids, got_df):
        assert f == df.get(w, 0) and (i >= 0) == (w in df), (what, len(w.encode()), w[-1], i, f)
    live = [i for i in ids if i >= 0]
    assert len(set(live)) == len(live) == len(vocab), what


def term_round(ctx, what):
    docs, words = term_docs()
    assert len(words) == len(set(words)) == 4 * len(TERM_LENGTHS) - 1
    assert sorted(set(len(w.encode()) for w in words)) == sorted(set(TERM_LENGTHS) | {L - 1 for L in TERM_LENGTHS} - {0})
    assert set(vocab_oracle(docs)[0]) == set(words)
    m = build(docs, ctx=ctx)
    check_index(m, docs, (what, "built"))
    check_lookup(m, docs, words, (what, "built"))
    m.remove_documents(range(0, len(docs), 3))
    docs = [d for i, d in enumerate(docs) if i % 3]
    assert 0 < len(vocab_oracle(docs)[0]) < len(words)                    # (some words left with their documents)
    check_vocabulary(m, docs, (what, "removed"))
    check_lookup(m, docs, words, (what, "removed"))
    m.compact()
    check_index(m, docs, (what, "compacted"))
    check_lookup(m, docs, words, (what, "compacted"))


@pytest.mark.parametrize("hash_bits", [0, 1])
def test_term_byte_lengths(hash_bits):
    ctx = _native.Context()
    try:
        _native.debug_set("bm25_hash_bits", hash_bits, ctx)
        term_round(ctx, hash_bits)
    finally:
        _native.debug_set("bm25_hash_bits", 0, ctx)
        ctx.close()
    _native.debug_set("bm25_hash_bits", 0)


# ---- 9: positions over multi-byte separators ---------------------------------------------------------------------------------------------------
def position_queries(split):
    """(queries, phrases, nears, windows): a few fixed ones, and for six documents of four words and more their words 1 and 2 as the
    phrase (and, the other way round, in the query) and their words 3 and 1 as the near set of a window of 3"""
    rich = [W for W in split if len(W) >= 4][:6]
    assert len(rich) == 6
    queries = ["a", "b a việt", "việt b", "", "nowhere a"] + [" ".join([W[2], W[1]]) for W in rich]
    phrases = ["a", "", "việt", "a", ""] + [" ".join(W[1:3]) for W in rich]
    nears = ["a b", "b", "", "a", "a"] + [" ".join([W[3], W[1]]) for W in rich]
    return queries, phrases, nears, [4, 1, 2, 1, 3] + [3] * len(rich)


def test_positions_over_multi_byte_separators(mix):
    docs = mix[:200]
    m = build(docs)
    split = [d.split() for d in docs]
    assert decoded(m, compacted=True) == split
    # (worth the test: most documents are cut into several words by 2- and 3-byte whitespace)
    assert sum(any(c in d for c in WS2 + WS3) and len(w) > 3 for d, w in zip(docs, split)) > 100
    queries, phrases, nears, windows = position_queries(split)
    nq, n = len(queries), len(docs)
    ids = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    pos, words, off = m.occurrences(queries, ids)
    assert pos.dtype == np.int32 and words.dtype == np.int32 and off.dtype == np.int64 and off.shape == (nq * n + 1,)
    want_pos, want_words, want_off = [], [], [0]
    for q in queries:
        Rl = q.split()
        for W in split:
            at = [p for p, w in enumerate(W) if w in Rl]
            want_pos += at
            want_words += [Rl.index(W[p]) for p in at]
            want_off.append(len(want_pos))
    assert off.tolist() == want_off and pos.tolist() == want_pos and words.tolist() == want_words
    assert max(want_pos) >= 8 and len(want_pos) > 150 and set(want_words) == {0, 1, 2}
    # phrase and near through their own tests' oracles
    S = m.get_scores(queries)
    for mode in ("any", "all"):
        mt = PH.matched(docs, queries, mode, None, phrases)
        assert mt[5:].any(axis=1).all() and not mt.all(axis=1).any(), mt.sum(axis=1).tolist()
        PH.check(m.search(queries, 10, match=mode, phrase=phrases), S, mt, 10, ("phrase", mode))
        assert np.array_equal(m.count_matches(queries, match=mode, phrase=phrases), mt.sum(axis=1)), mode
        mt = NR.matched(docs, queries, mode, None, None, nears, windows)
        assert mt[5:].any(axis=1).all() and not mt.all(axis=1).any(), mt.sum(axis=1).tolist()
        NR.check(m.search_near(queries, 10, nears, windows, match=mode), S, mt, 10, ("near", mode))
        assert np.array_equal(m.count_near(queries, nears, windows, match=mode), mt.sum(axis=1)), mode
    NR.check_cover(m, docs, queries, ids, "cover")
