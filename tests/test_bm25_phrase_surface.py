"""CPU-only: the positional BM25 index and the phrase search exist on every layer -- the C entry points and defines are declared,
documented in the header's ranking block, exported and bound; genz_tokenize.ranking's constructors take positions=, search /
count_matches take phrase=, and a bad phrase (or a phrase on an index without positions) is refused before any native call.
Nothing is computed here (tests/test_gpu_bm25_phrase.py does that)."""
import inspect
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_build_ex": 6, "gz_bm25_build_device_ex": 7, "gz_bm25_flags": 2, "gz_bm25_sequence": 3,
         "gz_bm25_search_phrase": 16, "gz_bm25_search_phrase_device": 16, "gz_bm25_match_count_phrase": 10}
# (what the existing entry points keep: pinned here too, the issue adds functions only)
OLD = {"gz_bm25_build": 5, "gz_bm25_build_device": 6, "gz_bm25_search_bool": 14, "gz_bm25_match_count_bool": 8, "gz_bm25_footprint": 2}


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
    for m in ("bm25_search", "bm25_match_count"):
        p = inspect.signature(getattr(native.Context, m)).parameters
        assert p["ph_terms"].default is None and p["ph_off"].default is None, m
        assert p["mode"].default == 0 and p["ex_terms"].default is None and p["ex_off"].default is None, m
    for m in ("bm25_build", "bm25_build_device"):
        assert inspect.signature(getattr(native.Context, m)).parameters["positions"].default is False, m
    assert callable(native.Context.bm25_flags) and callable(native.Context.bm25_sequence)
    assert native.GZ_BM25_POSITIONS == 1 and native.GZ_BM25_PHRASE_MAX == 64


def test_header_documents_defines_and_functions():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_BM25_POSITIONS 1\b", src, flags=re.M)
    assert re.search(r"^#define GZ_BM25_PHRASE_MAX 64\b", src, flags=re.M)
    assert re.search(r"^#define GZ_BM25_TOPK_MAX 1024\b", src, flags=re.M)
    assert re.search(r"^#define GZ_VERSION\s+0x010100\b", src, flags=re.M)
    block = src[src.index("BM25 / BM25Plus ranking"):]
    for n in NAMES:
        assert re.search(r"^ \*   %s\s" % n, block, flags=re.M), n
    for word in ("GZ_BM25_POSITIONS", "GZ_BM25_PHRASE_MAX"):
        assert word in block[:block.index("#define GZ_BM25_TOPK_MAX")], word       # (in the comment, not only as a define)


def test_ranking_signatures():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for name in ("search", "count_matches"):
        p = inspect.signature(getattr(ranking.BM25, name)).parameters
        assert p["phrase"].default is None and p["match"].default == "any" and p["exclude"].default is None, name
        assert list(p)[-3:] == ["match", "exclude", "phrase"], name
    assert ranking.BM25Plus.search is ranking.BM25.search and ranking.BM25Plus.count_matches is ranking.BM25.count_matches
    for cls in (ranking.BM25, ranking.BM25Plus):
        assert inspect.signature(cls.__init__).parameters["positions"].default is False, cls
    assert ranking.BM25Plus.term_sequences is ranking.BM25.term_sequences


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


BAD = [
    (dict(phrase=["a b"]), ValueError),               # for two queries
    (dict(phrase=["a", "b", "c"]), ValueError),
    (dict(phrase=["a", 3]), TypeError),
    (dict(phrase=[None, "b"]), TypeError),
    (dict(phrase=[b"a b", "b"]), TypeError),
    (dict(phrase=["a", "b"], exclude=["a"]), ValueError),
    (dict(phrase=["a", "b"], match="some"), ValueError),
]


def _bare(cls, positions):
    m = cls.__new__(cls)
    m._ctx = _NoNative()
    m._index = 0
    m.num_doc = 3
    if positions is not None:
        m._positions = positions
    return m


def test_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        for positions in (None, False, True):          # (None: an object that never heard of the attribute)
            m = _bare(cls, positions)
            for kw, exc in BAD:
                for mode in ({}, {"match": "all"}):
                    args = dict(mode, **kw)
                    with pytest.raises(exc):
                        m.search(["a", "b"], 2, **args)
                    with pytest.raises(exc):
                        m.count_matches(["a", "b"], **args)


def test_phrase_without_positions_is_refused_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        for positions in (None, False):
            m = _bare(cls, positions)
            for phrase in (["a b", "c"], ["", ""]):
                for mode in ("any", "all"):
                    with pytest.raises(ValueError, match="positions"):
                        m.search(["a", "b"], 2, match=mode, phrase=phrase)
                    with pytest.raises(ValueError, match="positions"):
                        m.count_matches(["a", "b"], match=mode, phrase=phrase)
            with pytest.raises(ValueError, match="positions"):
                m.term_sequences()
