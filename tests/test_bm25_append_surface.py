"""CPU-only: the BM25 append surface exists -- the C entry points are declared, exported and bound with their argument counts, and
genz_tokenize.ranking's classes expose add_documents.  Nothing is computed here (tests/test_gpu_bm25_append.py does that)."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_append": 4, "gz_bm25_append_device": 5}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc
    assert callable(getattr(native.Context, "bm25_append", None)) and callable(getattr(native.Context, "bm25_append_device", None))
    assert lib.gz_version() == 0x010100


def test_header_documents_the_calls():
    src = open(HEADER).read()
    for n in NAMES:
        assert re.search(r"^ \*\s+%s\b" % n, src, flags=re.M), n


def test_ranking_classes_expose_add_documents():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    assert callable(getattr(ranking.BM25, "add_documents", None))
    assert ranking.BM25Plus.add_documents is ranking.BM25.add_documents
