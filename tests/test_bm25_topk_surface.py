"""CPU-only: the BM25 top-k surface exists -- the C entry points are declared, exported and bound, the header carries the limit,
and genz_tokenize.ranking's classes expose top_k / get_top_n.  Nothing is computed here (tests/test_gpu_bm25_topk.py does that)."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = ("gz_bm25_topk", "gz_bm25_topk_device")


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == 10


def test_header_limit():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_BM25_TOPK_MAX 1024\b", src, flags=re.M)
    for switch in ("bm25_topk_chunk", "bm25_topk_tile"):
        assert switch in src


def test_ranking_classes_expose_retrieval():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        assert callable(getattr(cls, "top_k", None)) and callable(getattr(cls, "get_top_n", None))
    assert ranking.BM25Plus.top_k is ranking.BM25.top_k and ranking.BM25Plus.get_top_n is ranking.BM25.get_top_n


def test_switches_are_registered():
    native = pytest.importorskip("genz_tokenize._native")
    lib = native.load_library()
    for key, ok, bad in (("bm25_topk_chunk", (1, 1 << 27, 1 << 30), (0, (1 << 30) + 1)), ("bm25_topk_tile", (0, 1, 4096), (-1, 4097))):
        for v in ok:
            assert lib.gz_debug_set(None, key.encode(), v) == native.GZ_OK, (key, v)
        for v in bad:
            assert lib.gz_debug_set(None, key.encode(), v) == native.GZ_E_INVALID, (key, v)
    assert lib.gz_debug_set(None, b"bm25_topk_chunk", 1 << 27) == native.GZ_OK
    assert lib.gz_debug_set(None, b"bm25_topk_tile", 0) == native.GZ_OK
