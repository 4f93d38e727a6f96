"""CPU-only: the vocabulary queries exist on every layer -- the three C entry points are declared with their argument counts,
documented in the header's ranking block, exported and bound; _native.Context routes to them; genz_tokenize.ranking has
similar_words / prefix_words / term_texts / suggest / complete / correct with their defaults; the chunk switch is a typed key; and
every bad argument is refused before any native call.  Nothing is computed here (tests/test_gpu_bm25_vocab.py does that)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_similar": 10, "gz_bm25_prefix": 8, "gz_bm25_term_bytes": 6}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_bm25_lookup": 6, "gz_bm25_terms": 5, "gz_bm25_topk": 10, "gz_bm25_search": 11, "gz_bm25_cover": 9, "gz_bm25_compact": 1}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in dict(NAMES, **OLD).items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        assert len(decl.group(1).split(",")) == argc, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc, n
        assert getattr(lib, n).restype is native.C.c_int, n
    assert lib.gz_version() == 0x010100
    assert native.GZ_BM25_EDIT_MAX == 64
    vp, i32, i64 = native.C.c_void_p, native.C.c_int32, native.C.c_int64
    assert lib.gz_bm25_similar.argtypes == [vp, vp, vp, i64, i32, i64, vp, vp, vp, vp]
    assert lib.gz_bm25_prefix.argtypes == [vp, vp, vp, i64, i64, vp, vp, vp]
    assert lib.gz_bm25_term_bytes.argtypes == [vp, vp, i64, vp, vp, i64]
    for m in ("bm25_similar", "bm25_prefix", "bm25_term_bytes"):
        assert callable(getattr(native.Context, m)), m
    assert list(inspect.signature(native.Context.bm25_similar).parameters) == ["self", "index", "words", "word_off", "max_edits", "k"]
    assert list(inspect.signature(native.Context.bm25_prefix).parameters) == ["self", "index", "words", "word_off", "k"]
    assert list(inspect.signature(native.Context.bm25_term_bytes).parameters) == ["self", "index", "ids"]
    # a null index is refused by the argument checks, before any device is looked for
    for fn, args in ((lib.gz_bm25_similar, (None, None, None, 0, 2, 10, None, None, None, None)),
                     (lib.gz_bm25_prefix, (None, None, None, 0, 10, None, None, None)),
                     (lib.gz_bm25_term_bytes, (None, None, 0, None, None, 0))):
        assert fn(*args) == native.GZ_E_INVALID


def test_header_documents_the_functions():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_VERSION\s+0x010100\b", src, flags=re.M)
    assert re.search(r"^#define GZ_BM25_EDIT_MAX\s+64\b", src, flags=re.M)
    block = src[src.index("BM25 / BM25Plus ranking"):]
    comment = block[:block.index("#define GZ_BM25_TOPK_MAX")]
    for n in NAMES:
        assert re.search(r"^ \*   %s\s" % n, comment, flags=re.M), n
    for word in ("GZ_BM25_EDIT_MAX", "GZ_BM25_TOPK_MAX", "GZ_E_LIMIT", "GZ_E_INVALID", "GZ_E_CAPACITY", "bm25_vocab_chunk", "(distance, -df, id)",
                 "gz_bm25_terms", "not modified"):
        assert word in comment[comment.index(" *   gz_bm25_similar"):], word


def test_chunk_switch_is_a_typed_key():
    native = pytest.importorskip("genz_tokenize._native")
    lib = native.load_library()
    assert re.search(r"bm25_vocab_chunk \(1\.\.2\^30; 2\^23\)", open(HEADER).read())
    for v in (1, 7, 1 << 23, 1 << 30):
        assert lib.gz_debug_set(None, b"bm25_vocab_chunk", v) == native.GZ_OK, v
    for v in (0, -1, (1 << 30) + 1):
        assert lib.gz_debug_set(None, b"bm25_vocab_chunk", v) == native.GZ_E_INVALID, v
    assert lib.gz_debug_set(None, b"bm25_vocab_chunk", 1 << 23) == native.GZ_OK
    import gz_switches
    assert "bm25_vocab_chunk" in gz_switches.__doc__
    assert gz_switches.parse(gz_switches.encode(bm25_vocab_chunk=4096)) == [("bm25_vocab_chunk", 4096)]


def test_ranking_signatures():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    p = inspect.signature(ranking.BM25.similar_words).parameters
    assert list(p) == ["self", "words", "max_edits", "k"] and p["max_edits"].default == 2 and p["k"].default == 10
    p = inspect.signature(ranking.BM25.prefix_words).parameters
    assert list(p) == ["self", "prefixes", "k"] and p["k"].default == 10
    p = inspect.signature(ranking.BM25.term_texts).parameters
    assert list(p) == ["self", "ids"]
    p = inspect.signature(ranking.BM25.suggest).parameters
    assert list(p) == ["self", "words", "max_edits", "k"] and p["max_edits"].default == 2 and p["k"].default == 10
    p = inspect.signature(ranking.BM25.complete).parameters
    assert list(p) == ["self", "prefixes", "k"] and p["k"].default == 10
    p = inspect.signature(ranking.BM25.correct).parameters
    assert list(p) == ["self", "queries", "max_edits"] and p["max_edits"].default == 2
    for name in ("similar_words", "prefix_words", "term_texts", "suggest", "complete", "correct"):
        assert getattr(ranking.BM25Plus, name) is getattr(ranking.BM25, name), name
    # what was there is what it was
    assert list(inspect.signature(ranking.BM25.search).parameters) == ["self", "queries", "k", "match", "exclude", "phrase"]
    assert list(inspect.signature(ranking.BM25.vocabulary).parameters) == ["self"]
    assert list(inspect.signature(ranking.BM25.top_k).parameters) == ["self", "queries", "k"]
    for word in ("Vocabulary lookup:", "similar_words(", "prefix_words(", "term_texts(", "correct("):
        assert word in ranking.__doc__, word


class _InfoOnly:
    """stands in for the context: the term count is host bookkeeping (gz_bm25_info reads two fields); any other native call fails
    the test"""

    def bm25_info(self, index):
        return 3, 5, 9                                    # documents, live terms, words

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare(cls):
    m = cls.__new__(cls)
    m._ctx = _InfoOnly()
    m._index = 0
    m.num_doc = 3
    m._texts = ["a b", "b c d", "e"]
    return m


BAD_WORDS = [(["a", 3], TypeError), ([b"a"], TypeError), (["a", None], TypeError), ([["a"]], TypeError), (3, TypeError)]
BAD_K = [(0, ValueError), (-1, ValueError), (True, TypeError), (2.0, TypeError), ("3", TypeError), (None, TypeError)]
BAD_EDITS = [(-1, ValueError), (65, ValueError), (1 << 40, ValueError), (True, TypeError), (1.0, TypeError), ("2", TypeError), (None, TypeError)]
BAD_IDS = [
    ([0.0, 1.0], TypeError),
    ([True, False], TypeError),
    (["0"], TypeError),
    ([[0, 1], [None]], TypeError),
    (np.array([0.5, 1.0]), TypeError),
    (np.array([True, False]), TypeError),
    (np.array(["a"]), TypeError),
    ([0, 5], IndexError),                               # T = 5
    ([-2], IndexError),
    ([[0, 1], [[2, 7]]], IndexError),
    (np.array([[0, 2 ** 40]]), IndexError),
    (np.array([2 ** 63], dtype=np.uint64), IndexError),
    (-3, IndexError),
]


def test_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls)
        for words, exc in BAD_WORDS:
            for call in (lambda: m.similar_words(words), lambda: m.prefix_words(words), lambda: m.suggest(words),
                         lambda: m.complete(words), lambda: m.correct(words)):
                with pytest.raises(exc):
                    call()
        for k, exc in BAD_K:
            for call in (lambda: m.similar_words(["a"], 2, k), lambda: m.prefix_words(["a"], k), lambda: m.suggest(["a"], 2, k),
                         lambda: m.complete(["a"], k)):
                with pytest.raises(exc):
                    call()
        for e, exc in BAD_EDITS:
            for call in (lambda: m.similar_words(["a"], e), lambda: m.suggest(["a"], e, 3), lambda: m.correct(["a b"], e)):
                with pytest.raises(exc):
                    call()
        for ids, exc in BAD_IDS:
            with pytest.raises(exc):
                m.term_texts(ids)


def test_empty_inputs_need_no_vocabulary_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls)
        for k, kk in ((3, 3), (10, 5), (5, 5)):                             # k' = min(k, T), T = 5
            ids, dist, df, counts = m.similar_words([], 2, k)
            assert ids.shape == dist.shape == df.shape == (0, kk) and counts.shape == (0,)
            assert (ids.dtype, dist.dtype, df.dtype, counts.dtype) == (np.int64, np.int32, np.int32, np.int64)
            ids, df, counts = m.prefix_words([], k)
            assert ids.shape == df.shape == (0, kk) and counts.shape == (0,)
            assert (ids.dtype, df.dtype, counts.dtype) == (np.int64, np.int32, np.int64)
        assert m.term_texts([]) == [] and m.term_texts([[], [[]]]) == [[], [[]]] and m.term_texts(np.zeros((2, 0), dtype=np.int32)) == [[], []]
        assert m.suggest([]) == [] and m.complete([]) == [] and m.correct([]) == [] and m.correct(["", " \n"]) == ["", ""]
