"""CPU-only: snippets and query-word positions exist on every layer -- the three C entry points are declared with their argument
counts, documented in the header's ranking block, exported and bound; _native.Context and genz_tokenize.ranking have the new methods
with their defaults; search / count_matches are what they were; and every bad argument is refused before any native call.
Nothing is computed here (tests/test_gpu_bm25_snippets.py does that)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_snippets": 9, "gz_bm25_snippets_device": 9, "gz_bm25_occurrences": 10}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_bm25_search": 11, "gz_bm25_search_device": 11, "gz_bm25_search_phrase": 16, "gz_bm25_match_count_phrase": 10, "gz_bm25_terms": 5,
       "gz_bm25_sequence": 3}


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
    assert lib.gz_version() == 0x010100
    vp, i64 = native.C.c_void_p, native.C.c_int64
    assert lib.gz_bm25_snippets.argtypes == [vp, vp, vp, i64, vp, i64, i64, vp, vp]
    assert lib.gz_bm25_snippets_device.argtypes == lib.gz_bm25_snippets.argtypes
    assert lib.gz_bm25_occurrences.argtypes == [vp, vp, vp, i64, vp, i64, vp, vp, vp, i64]
    for m in ("bm25_snippets", "bm25_snippets_device", "bm25_occurrences"):
        assert callable(getattr(native.Context, m)), m


def test_header_documents_the_functions():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_VERSION\s+0x010100\b", src, flags=re.M)
    block = src[src.index("BM25 / BM25Plus ranking"):]
    comment = block[:block.index("#define GZ_BM25_TOPK_MAX")]
    for n in NAMES:
        assert re.search(r"^ \*   %s\s" % n, comment, flags=re.M), n
    for word in ("GZ_E_CAPACITY", "GZ_E_LIMIT", "GZ_BM25_POSITIONS", "pair_off_out", "treated as -1"):
        assert word in comment[comment.index(" *   gz_bm25_snippets"):], word


def test_ranking_signatures():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    p = inspect.signature(ranking.BM25.snippets).parameters
    assert list(p) == ["self", "queries", "ids", "width"] and p["width"].default == 32
    p = inspect.signature(ranking.BM25.occurrences).parameters
    assert list(p) == ["self", "queries", "ids"]
    p = inspect.signature(ranking.BM25.snippet_texts).parameters
    assert list(p) == ["self", "queries", "ids", "width", "mark"] and p["width"].default == 32 and p["mark"].default is None
    for name in ("snippets", "occurrences", "snippet_texts"):
        assert getattr(ranking.BM25Plus, name) is getattr(ranking.BM25, name), name
    # search / count_matches are what they were
    p = inspect.signature(ranking.BM25.search).parameters
    assert list(p) == ["self", "queries", "k", "match", "exclude", "phrase"]
    p = inspect.signature(ranking.BM25.count_matches).parameters
    assert list(p) == ["self", "queries", "match", "exclude", "phrase"]
    for name in ("search", "count_matches"):
        p = inspect.signature(getattr(ranking.BM25, name)).parameters
        assert p["match"].default == "any" and p["exclude"].default is None and p["phrase"].default is None, name
    assert "snippets(" in ranking.__doc__ and "occurrences(" in ranking.__doc__


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare(cls, positions):
    m = cls.__new__(cls)
    m._ctx = _NoNative()
    m._index = 0
    m.num_doc = 3
    m._texts = ["a b", "b", ""]
    if positions is not None:
        m._positions = positions
    return m


Q2 = ["a", "b"]
GOOD = [[0, 1, -1], [2, 2, 0]]
# (queries, ids, keywords) -> the exception
BAD = [
    (["a", 3], GOOD, {}, TypeError),
    ([b"a", "b"], GOOD, {}, TypeError),
    (Q2, [[0.0, 1.0], [1.0, 2.0]], {}, TypeError),
    (Q2, [[True, False], [False, True]], {}, TypeError),
    (Q2, [["0", "1"], ["1", "2"]], {}, TypeError),
    (Q2, [0, 1], {}, ValueError),                       # 1-D
    (Q2, [[[0], [1]], [[1], [2]]], {}, ValueError),     # 3-D
    (Q2, 1, {}, ValueError),                            # 0-D
    (Q2, [[0, 1, 2]], {}, ValueError),                  # one row for two queries
    (Q2, [[0], [1], [2]], {}, ValueError),
    (Q2, GOOD, {"width": 0}, ValueError),
    (Q2, GOOD, {"width": -5}, ValueError),
    (Q2, GOOD, {"width": 2.0}, TypeError),
    (Q2, GOOD, {"width": "3"}, TypeError),
    (Q2, GOOD, {"width": True}, TypeError),
    (Q2, [[0, 3], [1, 2]], {}, IndexError),             # num_doc = 3
    (Q2, [[0, -2], [1, 2]], {}, IndexError),
    (Q2, np.array([[0, 2 ** 40], [1, 2]]), {}, IndexError),
    (Q2, np.array([[0, 2 ** 63], [1, 2]], dtype=np.uint64), {}, IndexError),
]


def test_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls, True)
        for queries, ids, kw, exc in BAD:
            with pytest.raises(exc):
                m.snippets(queries, ids, **kw)
            with pytest.raises(exc):
                m.snippet_texts(queries, ids, **kw)
            with pytest.raises(exc):
                m.snippet_texts(queries, ids, mark=("[", "]"), **kw)
            if not kw:
                with pytest.raises(exc):
                    m.occurrences(queries, ids)
        with pytest.raises(TypeError):
            m.snippet_texts(Q2, GOOD, mark=("[", 3))
        with pytest.raises(ValueError):
            m.snippet_texts(Q2, GOOD, mark=("[",))


def test_without_positions_is_refused_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        for positions in (None, False):                 # (None: an object that never heard of the attribute)
            m = _bare(cls, positions)
            for ids in (GOOD, np.zeros((2, 0), dtype=np.int64)):
                with pytest.raises(ValueError, match="positions"):
                    m.snippets(Q2, ids)
                with pytest.raises(ValueError, match="positions"):
                    m.occurrences(Q2, ids)
                with pytest.raises(ValueError, match="positions"):
                    m.snippet_texts(Q2, ids, mark=("<", ">"))


def test_empty_shapes_need_no_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls, True)
        for queries, ids in ((Q2, np.zeros((2, 0), dtype=np.int64)), ([], np.zeros((0, 5), dtype=np.int32)), ([], np.zeros((0, 0), dtype=np.int64))):
            nq, k = ids.shape
            s, h = m.snippets(queries, ids, width=7)
            assert s.shape == (nq, k) and h.shape == (nq, k) and s.dtype == np.int32 and h.dtype == np.int32
            pos, words, off = m.occurrences(queries, ids)
            assert pos.shape == (0,) and words.shape == (0,) and pos.dtype == np.int32 and words.dtype == np.int32
            assert off.dtype == np.int64 and off.tolist() == [0]
            assert m.snippet_texts(queries, ids, mark=("<", ">")) == [[] for _ in range(nq)]
