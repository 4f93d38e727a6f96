"""CPU-only: the boolean BM25 search surface exists -- the three C entry points are declared, exported and bound, the header
documents them and the two modes, genz_tokenize.ranking's search / count_matches take match= and exclude=, and those are
validated before any native call.  Nothing is computed here (tests/test_gpu_bm25_search_bool.py does that)."""
import inspect
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_search_bool": 14, "gz_bm25_search_bool_device": 14, "gz_bm25_match_count_bool": 8}


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
        sig = inspect.signature(getattr(native.Context, m))
        assert sig.parameters["mode"].default == 0 and sig.parameters["ex_terms"].default is None and sig.parameters["ex_off"].default is None


def test_header_documents_modes_and_functions():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_BM25_MATCH_ANY 0\b", src, flags=re.M)
    assert re.search(r"^#define GZ_BM25_MATCH_ALL 1\b", src, flags=re.M)
    block = src[src.index("BM25 / BM25Plus ranking"):]
    for n in NAMES:
        assert re.search(r"^ \*   %s\s" % n, block, flags=re.M), n


def test_ranking_signatures():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for name in ("search", "count_matches"):
        p = inspect.signature(getattr(ranking.BM25, name)).parameters
        assert p["match"].default == "any" and p["exclude"].default is None, name
    assert ranking.BM25Plus.search is ranking.BM25.search and ranking.BM25Plus.count_matches is ranking.BM25.count_matches


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


BAD = [
    (dict(match="some"), ValueError),
    (dict(match=1), TypeError),
    (dict(match=None), TypeError),
    (dict(exclude=["a"]), ValueError),                # for two queries
    (dict(exclude=["a", 3]), TypeError),
    (dict(exclude=[b"a", "b"]), TypeError),
]


def test_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = cls.__new__(cls)
        m._ctx = _NoNative()
        m._index = 0
        m.num_doc = 3
        for kw, exc in BAD:
            for mode in ({}, {"match": "all"}):
                args = dict(mode, **kw)
                with pytest.raises(exc):
                    m.search(["a", "b"], 2, **args)
                with pytest.raises(exc):
                    m.count_matches(["a", "b"], **args)
