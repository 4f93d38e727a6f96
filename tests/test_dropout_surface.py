"""CPU-only: BPE-dropout exists on every layer -- the three C entry points are declared with their argument lists, documented in the
header's own section, exported and bound; _native.Context routes to them; Tokenize has the four calls.  The GZ_E_INVALID cases that
the entry points answer before they touch a device are checked on a GPU (tests/test_gpu_dropout.py: a context needs one); nothing
is computed here."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
ENC = ["gz_ctx *", "const uint8_t *", "const int64_t *", "int64_t", "int32_t", "uint32_t", "int64_t", "uint64_t", "uint64_t", "int64_t",
       "int32_t *", "int32_t *", "int64_t *", "int32_t *"]
WORD = ["gz_ctx *", "const uint8_t *", "int64_t", "uint64_t", "uint64_t", "int64_t", "int64_t", "int32_t *", "int64_t"]
NAMES = {"gz_encode_dropout": ("int", ENC), "gz_encode_dropout_device": ("int", ENC), "gz_bpe_word_dropout": ("int64_t", WORD)}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_encode_batch": 17, "gz_encode_batch_device": 17, "gz_bpe_word": 5, "gz_mask_rows": 17}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, (ret, types) in NAMES.items():
        decl = re.search(r"\b%s\s+%s\s*\(([^;]*?)\)\s*;" % (ret, n), src, flags=re.S)
        assert decl, n
        args = [a.strip() for a in decl.group(1).split(",")]
        assert [re.sub(r"\w+$", "", a).strip() for a in args] == types, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == len(types), n
    for n, argc in OLD.items():
        decl = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == argc, n
        assert len(getattr(lib, n).argtypes) == argc, n
    assert lib.gz_version() == 0x010100
    C = native.C
    vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
    assert lib.gz_encode_dropout.argtypes == [vp, vp, vp, i64, i32, u32, i64, u64, u64, i64, vp, vp, vp, vp]
    assert lib.gz_encode_dropout_device.argtypes == lib.gz_encode_dropout.argtypes
    assert lib.gz_bpe_word_dropout.argtypes == [vp, vp, i64, u64, u64, i64, i64, vp, i64]
    assert lib.gz_encode_dropout.restype is C.c_int and lib.gz_encode_dropout_device.restype is C.c_int
    assert lib.gz_bpe_word_dropout.restype is i64
    for m in ("encode_dropout", "encode_dropout_device", "bpe_word_dropout"):
        assert callable(getattr(native.Context, m)), m
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    for m in ("encode_dropout", "encode_dropout_packed", "encode_dropout_to_device", "bpe_dropout"):
        assert callable(getattr(tokenize.Tokenize, m)), m


def test_null_context_is_refused():
    """The one refusal that needs no device: a NULL context answers GZ_E_INVALID from every entry point."""
    native = pytest.importorskip("genz_tokenize._native")
    lib = native.load_library()
    assert lib.gz_encode_dropout(None, None, None, 0, 8, 3, 0, 0, 0, 0, None, None, None, None) == native.GZ_E_INVALID
    assert lib.gz_encode_dropout_device(None, None, None, 0, 8, 3, 0, 0, 0, 0, None, None, None, None) == native.GZ_E_INVALID
    assert lib.gz_bpe_word_dropout(None, None, 0, 0, 0, 0, 0, None, 0) == native.GZ_E_INVALID


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("---- BPE-dropout"):]
    comment = block[:block.index("int  gz_encode_dropout(")]
    for word in ("Provilkov", "drop_threshold / 2^32", "Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85",
                 "(D lo, D hi, j, 0)", "(t, i >> 2, 0, 0)", "i & 3", "LIVE", "left to right", "never overlapping", "n - 1 iterations",
                 "whole-word tables are never consulted", "GZ_NO_WORD_TABLE", "GZ_KEEP_WORDS", "GZ_E_INVALID", "doc_base", "2^63", "2^32",
                 "sub_batches", "gz_word_token_counts", "gz_sync", "gz_encode_dropout_device:", "gz_bpe_word_dropout:", "word_index",
                 "tests/dropout_oracle.py"):
        assert word in comment, word
    assert src.index("gz_bpe_word(") < src.index("---- BPE-dropout") < src.index("gz_encode_batch_csr(")
