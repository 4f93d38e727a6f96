"""CPU-only: the BM25 search surface exists -- the C entry points are declared, exported and bound, the switch is registered and
documented, genz_tokenize.ranking's classes expose search / count_matches, and their arguments are validated before any native
call.  Nothing is computed here (tests/test_gpu_bm25_search.py does that)."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_search": 11, "gz_bm25_search_device": 11, "gz_bm25_match_count": 5}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        assert len(decl.group(1).split(",")) == argc, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc
    assert lib.gz_version() == 0x010100
    for m in ("bm25_search", "bm25_match_count"):
        assert callable(getattr(native.Context, m, None))


def test_header_documents_search_and_switch():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_BM25_TOPK_MAX 1024\b", src, flags=re.M)
    assert re.search(r"bm25_search_chunk \(1\.\.2\^30; 2\^27\)", src)
    block = src[src.index("BM25 / BM25Plus ranking"):]
    for n in NAMES:
        assert re.search(r"^ \*   %s\s" % n, block, flags=re.M), n


def test_switch_is_registered():
    native = pytest.importorskip("genz_tokenize._native")
    lib = native.load_library()
    for v in (1, 1 << 27, 1 << 30):
        assert lib.gz_debug_set(None, b"bm25_search_chunk", v) == native.GZ_OK, v
    for v in (0, -1, (1 << 30) + 1):
        assert lib.gz_debug_set(None, b"bm25_search_chunk", v) == native.GZ_E_INVALID, v
    assert lib.gz_debug_set(None, b"bm25_search_chunk", 1 << 27) == native.GZ_OK


def test_ranking_classes_expose_search():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        assert callable(getattr(cls, "search", None)) and callable(getattr(cls, "count_matches", None))
    assert ranking.BM25Plus.search is ranking.BM25.search and ranking.BM25Plus.count_matches is ranking.BM25.count_matches


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def test_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = cls.__new__(cls)
        m._ctx = _NoNative()
        m._index = 0
        m.num_doc = 3
        for bad in (0, -1):
            with pytest.raises(ValueError):
                m.search(["a"], bad)
        for bad in (1.0, "3", None, True):
            with pytest.raises(TypeError):
                m.search(["a"], bad)
        with pytest.raises(TypeError):
            m.search(["a", 3], 2)
        with pytest.raises(TypeError):
            m.search([b"a"], 2)
        with pytest.raises(TypeError):
            m.count_matches(["a", None])
