"""CPU-only: masked-LM rows exist on every layer -- the two C entry points are declared with their argument lists, documented in
the header's own section, exported and bound; _native.Context routes to them; Tokenize has mask_rows / mask_rows_to_device with
their defaults; and every bad argument is refused before any native call.  Nothing is computed here (tests/test_gpu_mask.py does
that)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_mask_rows": 17, "gz_mask_rows_device": 17}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_window_rows": 16, "gz_window_rows_device": 16, "gz_pack_rows": 18, "gz_pack_rows_device": 18, "gz_decode_batch_device": 10}
TYPES = ["gz_ctx *", "const int32_t *", "int64_t", "int32_t", "int64_t", "uint64_t", "uint64_t", "uint64_t", "uint64_t", "int32_t", "int32_t",
         "int32_t", "int32_t", "int32_t", "int32_t *", "int32_t *", "int32_t *"]


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in dict(NAMES, **OLD).items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == argc, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc, n
        if n in NAMES:
            assert [re.sub(r"\w+$", "", a).strip() for a in args] == TYPES, n
    assert lib.gz_version() == 0x010100
    C = native.C
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert lib.gz_mask_rows.argtypes == [vp, vp, i64, i32, i64, u64, u64, u64, u64, i32, i32, i32, i32, i32, vp, vp, vp]
    assert lib.gz_mask_rows_device.argtypes == lib.gz_mask_rows.argtypes
    assert lib.gz_mask_rows.restype is C.c_int and lib.gz_mask_rows_device.restype is C.c_int
    for m in ("mask_rows", "mask_rows_device"):
        assert callable(getattr(native.Context, m)), m


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("masked-LM inputs and labels"):]
    comment = block[:block.index("int  gz_mask_rows(")]
    for word in ("PROTECTED", "CONTINUATION", "start(r, c)", "head(r, c)", "g(r, c)", "Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9",
                 "0xBB67AE85", "t_sel", "mulhi32", "ignore_index", "n_chosen", "row_base", "GZ_E_INVALID", "GZ_E_NOTABLES", "gz_decoder_snapshot",
                 "overlap", "gz_mask_rows_device:", "gz_mask_rows:", "2^63", "2^32"):
        assert word in comment, word
    assert src.index("gz_pack_rows_device(") < src.index("masked-LM inputs and labels") < src.index("---- text pre-pass")


def test_switch_is_documented_and_range_checked():
    native = pytest.importorskip("genz_tokenize._native")
    lib = native.load_library()
    assert re.search(r"mask_lds \(0\.\.1; 1\)", open(HEADER).read())
    for v in (0, 1):
        assert lib.gz_debug_set(None, b"mask_lds", v) == native.GZ_OK, v
    for v in (-1, 2):
        assert lib.gz_debug_set(None, b"mask_lds", v) == native.GZ_E_INVALID, v
    assert lib.gz_debug_set(None, b"mask_lds", 1) == native.GZ_OK


def test_tokenize_signatures():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    want = [("input_ids", inspect.Parameter.empty), ("p", 0.15), ("seed", 0), ("whole_word", True), ("mask_prob", 0.8), ("random_prob", 0.1),
            ("random_ids", None), ("row_base", 0), ("ignore_index", -100)]
    for name in ("mask_rows", "mask_rows_to_device"):
        p = inspect.signature(getattr(tokenize.Tokenize, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in want], name
        for k, d in want:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
    for name in ("encode_windows_masked", "encode_packs_masked", "encode_batch_masked"):      # one composable pass, no fused doors
        assert not hasattr(tokenize.Tokenize, name)
    # the neighbours are what they were
    p = inspect.signature(tokenize.Tokenize.encode_windows).parameters
    assert list(p) == ["self", "texts", "max_len", "stride", "word_table"]
    p = inspect.signature(tokenize.Tokenize.encode_packs).parameters
    assert list(p) == ["self", "texts", "max_len", "word_table"]


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = _NoNative()
    t._dirty = True                                                   # (so that any table use would reach the context)
    return t


IDS = np.zeros((2, 4), dtype=np.int32)
BAD = [
    (IDS, dict(p=-0.1), ValueError), (IDS, dict(p=1.0001), ValueError), (IDS, dict(p=float("nan")), ValueError), (IDS, dict(p=True), TypeError),
    (IDS, dict(p="0.1"), TypeError), (IDS, dict(p=None), TypeError),
    (IDS, dict(mask_prob=-1), ValueError), (IDS, dict(mask_prob=2), ValueError), (IDS, dict(mask_prob=False), TypeError),
    (IDS, dict(random_prob=1.5), ValueError), (IDS, dict(random_prob="x"), TypeError),
    (IDS, dict(mask_prob=0.8, random_prob=0.3), ValueError), (IDS, dict(mask_prob=1.0, random_prob=0.01), ValueError),
    (IDS, dict(seed=-1), ValueError), (IDS, dict(seed=2 ** 64), ValueError), (IDS, dict(seed=1.0), TypeError), (IDS, dict(seed=True), TypeError),
    (IDS, dict(seed=None), TypeError),
    (IDS, dict(row_base=-1), ValueError), (IDS, dict(row_base=2 ** 63), ValueError), (IDS, dict(row_base=True), TypeError),
    (IDS, dict(row_base=0.0), TypeError), (IDS, dict(row_base=2 ** 63 // 4 - 1), ValueError),
    (IDS, dict(ignore_index=2 ** 31), ValueError), (IDS, dict(ignore_index=-2 ** 31 - 1), ValueError), (IDS, dict(ignore_index=False), TypeError),
    (IDS, dict(ignore_index=1.5), TypeError),
    (IDS, dict(whole_word=1), TypeError), (IDS, dict(whole_word=None), TypeError), (IDS, dict(whole_word="yes"), TypeError),
    (IDS, dict(random_ids=(5, 5)), ValueError), (IDS, dict(random_ids=(9, 5)), ValueError), (IDS, dict(random_ids=(5, 2 ** 31)), ValueError),
    (IDS, dict(random_ids=(5,)), TypeError), (IDS, dict(random_ids=7), TypeError), (IDS, dict(random_ids=(5, 9.0)), TypeError),
    (IDS, dict(random_ids=(True, 9)), TypeError),
    (IDS.astype(np.float64), {}, TypeError), (IDS.astype(bool), {}, TypeError), ([["a", "b"]], {}, TypeError),
    (IDS[0], {}, ValueError), (IDS.reshape(2, 2, 2), {}, ValueError), (np.zeros((3, 0), dtype=np.int32), {}, ValueError), (7, {}, ValueError),
    (np.array([[2 ** 31]]), {}, ValueError), (np.array([[-2 ** 31 - 1]]), {}, ValueError), (np.array([[2 ** 63]], dtype=np.uint64), {}, ValueError),
]


def test_refusals_before_any_native_call():
    t = _bare()
    for ids, kw, exc in BAD:
        with pytest.raises(exc):
            t.mask_rows(ids, **kw)
    handoff = pytest.importorskip("genz_tokenize.handoff")
    for rows in (IDS, IDS.tolist(), None):
        with pytest.raises(TypeError):
            t.mask_rows_to_device(rows)
    fake = handoff.DeviceArray.__new__(handoff.DeviceArray)           # (no allocation behind it: only its shape and dtype are looked at)
    fake._ctx, fake.ptr, fake._block = t._ctx, 0, None
    for shape, dtype, exc in (((2, 4), np.int64, TypeError), ((8,), np.int32, ValueError), ((2, 0), np.int32, ValueError), ((2, 2, 2), np.int32, ValueError)):
        fake.shape, fake.dtype = shape, np.dtype(dtype)
        with pytest.raises(exc):
            t.mask_rows_to_device(fake)
    fake.shape, fake.dtype = (2, 4), np.dtype(np.int32)
    for _, kw, exc in BAD[:37]:                                       # the rule's own refusals are the same ones
        with pytest.raises(exc):
            t.mask_rows_to_device(fake, **kw)
    fake._ctx = _NoNative()                                           # rows of another context
    with pytest.raises(ValueError):
        t.mask_rows_to_device(fake)
