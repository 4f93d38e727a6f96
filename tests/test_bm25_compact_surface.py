"""CPU-only: the BM25 compaction surface exists -- the C entry points are declared, exported and bound with their argument counts,
and genz_tokenize.ranking's classes expose compact, vocabulary and footprint.  Nothing is computed here
(tests/test_gpu_bm25_compact.py does that)."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_compact": 1, "gz_bm25_terms": 5, "gz_bm25_footprint": 2}
METHODS = ("compact", "vocabulary", "footprint")


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc
        assert callable(getattr(native.Context, n[3:], None)), n
    assert lib.gz_version() == 0x010100


def test_header_documents_the_calls():
    src = open(HEADER).read()
    for n in NAMES:
        assert re.search(r"^ \*\s+%s\b" % n, src, flags=re.M), n


def test_ranking_classes_expose_the_methods():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for name in METHODS:
        assert callable(getattr(ranking.BM25, name, None)), name
        assert getattr(ranking.BM25Plus, name) is getattr(ranking.BM25, name), name
