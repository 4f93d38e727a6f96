"""CPU-only: the BM25 removal surface exists -- the C entry points are declared, exported and bound with their argument counts, and
genz_tokenize.ranking's classes expose remove_documents.  Nothing is computed here (tests/test_gpu_bm25_remove.py does that)."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_remove": 3, "gz_bm25_remove_device": 3}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc
    assert callable(getattr(native.Context, "bm25_remove", None)) and callable(getattr(native.Context, "bm25_remove_device", None))
    assert lib.gz_version() == 0x010100


def test_header_documents_the_calls():
    src = open(HEADER).read()
    for n in NAMES:
        assert re.search(r"^ \*\s+%s\b" % n, src, flags=re.M), n


def test_ranking_classes_expose_remove_documents():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    assert callable(getattr(ranking.BM25, "remove_documents", None))
    assert ranking.BM25Plus.remove_documents is ranking.BM25.remove_documents
