"""CPU-only: proximity search and covers exist on every layer -- the five C entry points are declared with their argument counts,
documented in the header's ranking block, exported and bound; _native.Context routes to them; genz_tokenize.ranking has
search_near / count_near / cover with their defaults; search / count_matches are what they were; and every bad argument is refused
before any native call.  Nothing is computed here (tests/test_gpu_bm25_near.py does that)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_search_near": 19, "gz_bm25_search_near_device": 19, "gz_bm25_match_count_near": 13, "gz_bm25_cover": 9,
         "gz_bm25_cover_device": 9}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_bm25_search_phrase": 16, "gz_bm25_search_phrase_device": 16, "gz_bm25_match_count_phrase": 10, "gz_bm25_snippets": 9,
       "gz_bm25_snippets_device": 9, "gz_bm25_search": 11}


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
    assert native.GZ_BM25_NEAR_MAX == 64
    vp, i64 = native.C.c_void_p, native.C.c_int64
    # the phrase form's arguments with the three near arguments behind ph_off
    ph = lib.gz_bm25_search_phrase.argtypes
    assert lib.gz_bm25_search_near.argtypes == ph[:13] + [vp, vp, vp] + ph[13:]
    assert lib.gz_bm25_search_near_device.argtypes == lib.gz_bm25_search_near.argtypes
    pc = lib.gz_bm25_match_count_phrase.argtypes
    assert lib.gz_bm25_match_count_near.argtypes == pc[:9] + [vp, vp, vp] + pc[9:]
    assert lib.gz_bm25_cover.argtypes == [vp, vp, vp, i64, vp, i64, vp, vp, vp]
    assert lib.gz_bm25_cover_device.argtypes == lib.gz_bm25_cover.argtypes
    for m in ("bm25_cover", "bm25_cover_device"):
        assert callable(getattr(native.Context, m)), m
    for m in ("bm25_search", "bm25_match_count"):
        p = inspect.signature(getattr(native.Context, m)).parameters
        assert list(p)[-3:] == ["nr_terms", "nr_off", "nr_window"], m
        for name in ("mode", "ex_terms", "ex_off", "ph_terms", "ph_off", "nr_terms", "nr_off", "nr_window"):
            assert p[name].default == (0 if name == "mode" else None), (m, name)


def test_header_documents_the_functions():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_VERSION\s+0x010100\b", src, flags=re.M)
    assert re.search(r"^#define GZ_BM25_NEAR_MAX\s+64\b", src, flags=re.M)
    block = src[src.index("BM25 / BM25Plus ranking"):]
    comment = block[:block.index("#define GZ_BM25_TOPK_MAX")]
    for n in NAMES:
        assert re.search(r"^ \*   %s\s" % n, comment, flags=re.M), n
    for word in ("GZ_BM25_NEAR_MAX", "GZ_BM25_POSITIONS", "GZ_E_LIMIT", "GZ_E_INVALID", "near_window", "treated as -1"):
        assert word in comment[comment.index(" *   gz_bm25_search_near"):], word


def test_ranking_signatures():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    p = inspect.signature(ranking.BM25.search_near).parameters
    assert list(p) == ["self", "queries", "k", "near", "window", "match", "exclude", "phrase"]
    assert p["near"].default is inspect.Parameter.empty and p["window"].default is inspect.Parameter.empty
    assert p["match"].default == "any" and p["exclude"].default is None and p["phrase"].default is None
    p = inspect.signature(ranking.BM25.count_near).parameters
    assert list(p) == ["self", "queries", "near", "window", "match", "exclude", "phrase"]
    assert p["match"].default == "any" and p["exclude"].default is None and p["phrase"].default is None
    p = inspect.signature(ranking.BM25.cover).parameters
    assert list(p) == ["self", "queries", "ids"]
    for name in ("search_near", "count_near", "cover"):
        assert getattr(ranking.BM25Plus, name) is getattr(ranking.BM25, name), name
    # search / count_matches / snippets are what they were
    p = inspect.signature(ranking.BM25.search).parameters
    assert list(p) == ["self", "queries", "k", "match", "exclude", "phrase"]
    p = inspect.signature(ranking.BM25.count_matches).parameters
    assert list(p) == ["self", "queries", "match", "exclude", "phrase"]
    for name in ("search", "count_matches"):
        p = inspect.signature(getattr(ranking.BM25, name)).parameters
        assert p["match"].default == "any" and p["exclude"].default is None and p["phrase"].default is None, name
    p = inspect.signature(ranking.BM25.snippets).parameters
    assert list(p) == ["self", "queries", "ids", "width"] and p["width"].default == 32
    assert "Proximity:" in ranking.__doc__ and "search_near(" in ranking.__doc__ and "cover(" in ranking.__doc__


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
N2 = ["a b", ""]
# (queries, near, window, keywords) -> the exception
BAD_NEAR = [
    (["a", 3], N2, 2, {}, TypeError),
    (Q2, ["a", 3], 2, {}, TypeError),
    (Q2, [b"a", "b"], 2, {}, TypeError),
    (Q2, ["a", None], 2, {}, TypeError),
    (Q2, ["a"], 2, {}, ValueError),
    (Q2, ["a", "b", "c"], 2, {}, ValueError),
    (Q2, [], 2, {}, ValueError),
    (Q2, N2, True, {}, TypeError),
    (Q2, N2, 2.0, {}, TypeError),
    (Q2, N2, "2", {}, TypeError),
    (Q2, N2, None, {}, TypeError),
    (Q2, N2, [2, 2.5], {}, TypeError),
    (Q2, N2, [2, True], {}, TypeError),
    (Q2, N2, [2, "3"], {}, TypeError),
    (Q2, N2, np.array([2.0, 3.0]), {}, TypeError),
    (Q2, N2, 0, {}, ValueError),
    (Q2, N2, -4, {}, ValueError),
    (Q2, N2, [2, 0], {}, ValueError),
    (Q2, N2, [2], {}, ValueError),
    (Q2, N2, [2, 3, 4], {}, ValueError),
    (Q2, N2, [], {}, ValueError),
    (Q2, N2, np.array([1, 2, 3]), {}, ValueError),
    (Q2, N2, 2, {"match": "some"}, ValueError),
    (Q2, N2, 2, {"match": 1}, TypeError),
    (Q2, N2, 2, {"exclude": ["a"]}, ValueError),
    (Q2, N2, 2, {"exclude": ["a", 1]}, TypeError),
    (Q2, N2, 2, {"phrase": ["a"]}, ValueError),
    (Q2, N2, 2, {"phrase": ["a", 1]}, TypeError),
]


def test_near_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls, True)
        for queries, near, window, kw, exc in BAD_NEAR:
            with pytest.raises(exc):
                m.search_near(queries, 3, near, window, **kw)
            with pytest.raises(exc):
                m.count_near(queries, near, window, **kw)
        for k, exc in ((0, ValueError), (-1, ValueError), (True, TypeError), (2.0, TypeError), ("3", TypeError)):
            with pytest.raises(exc):
                m.search_near(Q2, k, N2, 2)


GOOD = [[0, 1, -1], [2, 2, 0]]
BAD_COVER = [
    (["a", 3], GOOD, TypeError),
    ([b"a", "b"], GOOD, TypeError),
    (Q2, [[0.0, 1.0], [1.0, 2.0]], TypeError),
    (Q2, [[True, False], [False, True]], TypeError),
    (Q2, [["0", "1"], ["1", "2"]], TypeError),
    (Q2, [0, 1], ValueError),                           # 1-D
    (Q2, [[[0], [1]], [[1], [2]]], ValueError),         # 3-D
    (Q2, 1, ValueError),                                # 0-D
    (Q2, [[0, 1, 2]], ValueError),                      # one row for two queries
    (Q2, [[0], [1], [2]], ValueError),
    (Q2, [[0, 3], [1, 2]], IndexError),                 # num_doc = 3
    (Q2, [[0, -2], [1, 2]], IndexError),
    (Q2, np.array([[0, 2 ** 40], [1, 2]]), IndexError),
    (Q2, np.array([[0, 2 ** 63], [1, 2]], dtype=np.uint64), IndexError),
]


def test_cover_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls, True)
        for queries, ids, exc in BAD_COVER:
            with pytest.raises(exc):
                m.cover(queries, ids)
            # the same arguments, the same exception as snippets: one set of rules
            with pytest.raises(exc):
                m.snippets(queries, ids)


def test_without_positions_is_refused_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        for positions in (None, False):                 # (None: an object that never heard of the attribute)
            m = _bare(cls, positions)
            for near in (N2, ["", ""]):
                with pytest.raises(ValueError, match="positions"):
                    m.search_near(Q2, 3, near, 2)
                with pytest.raises(ValueError, match="positions"):
                    m.count_near(Q2, near, [2, 5])
            for ids in (GOOD, np.zeros((2, 0), dtype=np.int64)):
                with pytest.raises(ValueError, match="positions"):
                    m.cover(Q2, ids)


def test_empty_cover_shapes_need_no_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls, True)
        for queries, ids in ((Q2, np.zeros((2, 0), dtype=np.int64)), ([], np.zeros((0, 5), dtype=np.int32)), ([], np.zeros((0, 0), dtype=np.int64))):
            out = m.cover(queries, ids)
            assert len(out) == 3
            for a in out:
                assert a.shape == ids.shape and a.dtype == np.int32
