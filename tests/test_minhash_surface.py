"""CPU-only: MinHash exists on every layer -- the four C entry points are declared with their argument lists, documented in the
header's own section, exported and bound; _native.Context routes to them; Tokenize has minhash_rows, encode_minhash,
encode_minhash_to_device, minhash_groups and near_duplicates with their defaults; every bad argument is refused before any native
call; and the new rules of csrc/gz_rowrules.h hold in a stand-alone program.  Nothing is computed on a GPU here
(tests/test_gpu_minhash.py does that)."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
NAMES = {"gz_minhash_rows": 11, "gz_minhash_rows_device": 11, "gz_minhash_groups": 8, "gz_minhash_groups_device": 8}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_window_rows": 16, "gz_window_rows_device": 16, "gz_pack_rows": 18, "gz_pack_rows_device": 18, "gz_decode_batch_device": 10,
       "gz_mask_rows": 17, "gz_mask_rows_device": 17, "gz_infill_rows": 20, "gz_infill_rows_device": 20}
ROWS_TYPES = ["gz_ctx *", "const int32_t *", "const int64_t *", "int64_t", "int32_t", "int32_t", "int32_t", "int32_t", "uint64_t", "uint32_t *",
              "int32_t *"]
GROUPS_TYPES = ["gz_ctx *", "const uint32_t *", "int64_t", "int32_t", "int32_t", "int32_t", "int32_t *", "int64_t *"]


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
            assert [re.sub(r"\w+$", "", a).strip() for a in args] == (ROWS_TYPES if "rows" in n else GROUPS_TYPES), n
    assert lib.gz_version() == 0x010100
    C = native.C
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert lib.gz_minhash_rows.argtypes == [vp, vp, vp, i64, i32, i32, i32, i32, u64, vp, vp]
    assert lib.gz_minhash_rows_device.argtypes == lib.gz_minhash_rows.argtypes
    assert lib.gz_minhash_groups.argtypes == [vp, vp, i64, i32, i32, i32, vp, C.POINTER(i64)]
    assert lib.gz_minhash_groups_device.argtypes == lib.gz_minhash_groups.argtypes
    for n in NAMES:
        assert getattr(lib, n).restype is C.c_int, n
    for m in ("minhash_rows", "minhash_rows_device", "minhash_groups", "minhash_groups_device"):
        assert callable(getattr(native.Context, m)), m


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("near-duplicate documents by MinHash signatures"):]
    comment = block[:block.index("int  gz_minhash_rows(")]
    for word in ("fmix32", "0x85EBCA6B", "0xC2B2AE35", "MurmurHash3_x86_32", "0xCC9E2D51", "0x1B873593", "0xE6546B64", "0x9E3779B9",
                 "0x9E3779B97F4A7C15", "0xFF51AFD7ED558CCD", "seed_lo", "seed_hi", "bijection", "skip_front", "skip_back", "n_shingles",
                 "0xFFFFFFFF", "EMPTY", "rows_per_band", "key = z | 1", "rep_j(d)", "agree(a, b)", "min_agree", "group[d]", "n_groups_host",
                 "smallest member of a bucket", "GZ_E_INVALID", "GZ_E_LIMIT", "2^31 - 4096", "1..32", "1..256", "divide", "overlap",
                 "row offsets", "n_rows == 0", "gz_minhash_rows_device", "gz_minhash_groups_device", "gz_minhash_rows:", "gz_minhash_groups:",
                 "bytes a document", "minhash(rows[a:b]) == minhash(rows)[a:b]"):
        assert word in comment, word
    assert src.index("gz_infill_rows_device(") < src.index("near-duplicate documents by MinHash signatures") < src.index("---- text pre-pass")
    assert "GZ_E_NOTABLES" not in comment                                  # a bare context is enough


def test_tokenize_signatures():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    empty = inspect.Parameter.empty
    want = {
        "minhash_rows": [("rows", empty), ("num_perm", 128), ("shingle", 5), ("seed", 0), ("framed", True)],
        "encode_minhash": [("texts", empty), ("num_perm", 128), ("shingle", 5), ("seed", 0), ("word_table", True)],
        "encode_minhash_to_device": [("texts", empty), ("num_perm", 128), ("shingle", 5), ("seed", 0)],
        "minhash_groups": [("signatures", empty), ("bands", 16), ("threshold", 0.7), ("min_agree", None)],
        "near_duplicates": [("texts", empty), ("num_perm", 128), ("shingle", 5), ("seed", 0), ("bands", 16), ("threshold", 0.7),
                            ("min_agree", None), ("word_table", True)],
    }
    for name, params in want.items():
        p = inspect.signature(getattr(tokenize.Tokenize, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in params], name
        for k, d in params:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
        doc = getattr(tokenize.Tokenize, name).__doc__
        assert doc and len(doc) > 100, name
    for name in ("minhash_rows", "encode_minhash", "encode_minhash_to_device"):
        assert "shards concatenate" in getattr(tokenize.Tokenize, name).__doc__, name
    assert "minhash_rows(rows[a:b])` is `minhash_rows(rows)[a:b]" in tokenize.Tokenize.minhash_rows.__doc__
    assert isinstance(inspect.getattr_static(tokenize.Tokenize, "_minhash_rule"), staticmethod)
    for name in ("encode_windows_minhash", "encode_packs_minhash", "minhash_mask_rows"):        # one composable pass, no fused doors
        assert not hasattr(tokenize.Tokenize, name)
    # the neighbours are what they were
    assert list(inspect.signature(tokenize.Tokenize.encode_windows).parameters) == ["self", "texts", "max_len", "stride", "word_table"]
    assert list(inspect.signature(tokenize.Tokenize.window_rows).parameters) == ["self", "rows", "max_len", "stride", "framed"]


def test_rule_values():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    rule = tokenize.Tokenize._minhash_rule
    assert rule() == (128, 5, 0, 16, 90)                                   # ceil(0.7 * 128) = 90
    assert rule(64, 1, 2 ** 64 - 1, 64, 1.0) == (64, 1, 2 ** 64 - 1, 64, 64)
    assert rule(256, 32, 2 ** 32, 1, 0.001) == (256, 32, 2 ** 32, 1, 1)
    assert rule(10, 3, 7, 5, 0.5, min_agree=10) == (10, 3, 7, 5, 10)
    assert rule(np.int64(8), np.int32(2), np.uint64(3), np.int16(4), np.float32(0.5), np.int8(3)) == (8, 2, 3, 4, 3)
    assert rule(3, 5, 0, 3, 0.34) == (3, 5, 0, 3, 2)                       # ceil(1.02)


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


BAD_ROWS = [
    (dict(num_perm=0), ValueError), (dict(num_perm=257), ValueError), (dict(num_perm=-1), ValueError), (dict(num_perm=True), TypeError),
    (dict(num_perm=128.0), TypeError), (dict(num_perm=None), TypeError), (dict(num_perm="128"), TypeError),
    (dict(shingle=0), ValueError), (dict(shingle=33), ValueError), (dict(shingle=-5), ValueError), (dict(shingle=True), TypeError),
    (dict(shingle=5.0), TypeError), (dict(shingle=None), TypeError),
    (dict(seed=-1), ValueError), (dict(seed=2 ** 64), ValueError), (dict(seed=1.0), TypeError), (dict(seed=True), TypeError), (dict(seed=None), TypeError),
]
BAD_GROUPS = [
    (dict(bands=0), ValueError), (dict(bands=-2), ValueError), (dict(bands=3), ValueError), (dict(bands=5), ValueError), (dict(bands=True), TypeError),
    (dict(bands=2.0), TypeError), (dict(bands=None), TypeError),
    (dict(threshold=0), ValueError), (dict(threshold=0.0), ValueError), (dict(threshold=-0.5), ValueError), (dict(threshold=1.0001), ValueError),
    (dict(threshold=float("nan")), ValueError), (dict(threshold=True), TypeError), (dict(threshold="0.7"), TypeError), (dict(threshold=None), TypeError),
    (dict(min_agree=0), ValueError), (dict(min_agree=9), ValueError), (dict(min_agree=-1), ValueError), (dict(min_agree=True), TypeError),
    (dict(min_agree=4.0), TypeError), (dict(min_agree="4"), TypeError),
]
SIG = np.zeros((3, 8), dtype=np.uint32)


def test_refusals_before_any_native_call():
    t = _bare()
    for kw, exc in BAD_ROWS:
        with pytest.raises(exc):
            t._minhash_rule(**kw)
        with pytest.raises(exc):
            t.minhash_rows([[1, 2, 3]], **kw)
        for call in (t.encode_minhash, t.encode_minhash_to_device, t.near_duplicates):
            with pytest.raises(exc):
                call(["a b"], **kw)
    for kw, exc in BAD_GROUPS:
        with pytest.raises(exc):
            t._minhash_rule(**dict(dict(num_perm=8, bands=2), **kw))
        with pytest.raises(exc):
            t.minhash_groups(SIG, **dict(dict(bands=2), **kw))
        with pytest.raises(exc):
            t.near_duplicates(["a b"], **dict(dict(num_perm=8, bands=2), **kw))
    with pytest.raises(ValueError):
        t.minhash_groups(SIG)                                             # the default 16 bands do not divide 8 slots
    with pytest.raises(AssertionError, match="native call minhash_rows"):
        t.minhash_rows([[1, 2, 3]], 65)                                   # ... which is nothing to a call that makes signatures only
    for rows, exc in (([["a"]], (TypeError, ValueError)), ([[2 ** 31]], ValueError), ([[-2 ** 31 - 1]], ValueError),
                      (np.zeros((2, 3)), TypeError)):
        with pytest.raises(exc):
            t.minhash_rows(rows)
    for texts in (["a", 3], ["a", None], [b"a"]):
        for call in (t.encode_minhash, t.encode_minhash_to_device, t.near_duplicates):
            with pytest.raises(TypeError):
                call(texts)
    for sig, exc in ((SIG.astype(np.int32), TypeError), (SIG.astype(np.uint64), TypeError), (SIG.astype(np.float32), TypeError),
                     (SIG.tolist(), TypeError), (SIG[0], ValueError), (SIG.reshape(3, 2, 4), ValueError), (np.zeros((3, 0), np.uint32), ValueError),
                     (np.zeros((2, 257), np.uint32), ValueError), (None, TypeError)):
        with pytest.raises(exc):
            t.minhash_groups(sig, bands=1)
    handoff = pytest.importorskip("genz_tokenize.handoff")
    fake = handoff.DeviceArray.__new__(handoff.DeviceArray)           # (no allocation behind it: only its shape and dtype are looked at)
    fake._ctx, fake.ptr, fake._block = t._ctx, 0, None
    for shape, dtype, exc in (((2, 8), np.int32, TypeError), ((16,), np.uint32, ValueError), ((2, 0), np.uint32, ValueError),
                              ((2, 2, 2), np.uint32, ValueError), ((2, 300), np.uint32, ValueError)):
        fake.shape, fake.dtype = shape, np.dtype(dtype)
        with pytest.raises(exc):
            t.minhash_groups(fake, bands=1)
    fake.shape, fake.dtype = (2, 8), np.dtype(np.uint32)
    for kw, exc in BAD_GROUPS:
        with pytest.raises(exc):
            t.minhash_groups(fake, **dict(dict(bands=2), **kw))
    fake._ctx = _NoNative()                                           # signatures of another context
    with pytest.raises(ValueError):
        t.minhash_groups(fake, bands=2)


# ---- the rules of gz_rowrules.h, alone ------------------------------------------------------------------------------------------
MAIN = r"""
#include "gz_rowrules.h"
#include <cstdio>
#include <cstring>
#include <vector>

static void rows(const char* name, int64_t n, int32_t sf, int32_t sb, int32_t w, int32_t k)
{
    const char* why = minhash_rows_fault(n, sf, sb, w, k);
    std::printf("%s|%s\n", name, why ? why : "");
}
static void groups(const char* name, int64_t n, int32_t k, int32_t b, int32_t m)
{
    const char* why = minhash_groups_fault(n, k, b, m);
    std::printf("%s|%s\n", name, why ? why : "");
}

int main()
{
    rows("rows_ok", 5, 1, 1, 5, 128);
    rows("rows_edges", 0, 0, 1, 32, 256);
    rows("rows_edges_low", INT64_MAX, 1, 0, 1, 1);
    rows("rows_negative", -1, 0, 0, 5, 128);
    rows("skip_front_2", 1, 2, 0, 5, 128);
    rows("skip_back_negative", 1, 0, -1, 5, 128);
    rows("shingle_0", 1, 0, 0, 0, 128);
    rows("shingle_33", 1, 0, 0, 33, 128);
    rows("num_perm_0", 1, 0, 0, 5, 0);
    rows("num_perm_257", 1, 0, 0, 5, 257);
    rows("first_of_two", -1, 0, 0, 0, 0);
    groups("groups_ok", 5, 128, 16, 90);
    groups("groups_edges", 0, 256, 256, 256);
    groups("groups_edges_low", (int64_t)INT32_MAX - 4097, 1, 1, 1);
    groups("groups_negative", -1, 128, 16, 90);
    groups("groups_too_many", (int64_t)INT32_MAX - 4096, 128, 16, 90);
    groups("groups_num_perm_0", 1, 0, 1, 1);
    groups("groups_num_perm_257", 1, 257, 1, 1);
    groups("bands_0", 1, 128, 0, 90);
    groups("bands_negative", 1, 128, -16, 90);
    groups("bands_do_not_divide", 1, 128, 24, 90);
    groups("bands_above_num_perm", 1, 8, 16, 4);
    groups("min_agree_0", 1, 128, 16, 0);
    groups("min_agree_above", 1, 128, 16, 129);
    {
        std::vector<int64_t> off = {3, 3, 10, 10 + ((int64_t)1 << 31) + 1, 10 + ((int64_t)1 << 31) + 1};
        std::printf("fit_bare|%d\n", minhash_bodies_fit(off.data(), 4, 0, 0) ? 1 : 0);               // a body of 2^31 + 1
        std::printf("fit_framed_once|%d\n", minhash_bodies_fit(off.data(), 4, 1, 0) ? 1 : 0);        // 2^31
        std::printf("fit_framed|%d\n", minhash_bodies_fit(off.data(), 4, 1, 1) ? 1 : 0);             // 2^31 - 1
        std::printf("fit_before|%d\n", minhash_bodies_fit(off.data(), 2, 0, 0) ? 1 : 0);
        std::printf("fit_none|%d\n", minhash_bodies_fit(off.data(), 0, 0, 0) ? 1 : 0);
    }
    return 0;
}
"""

EXPECTED = {
    "rows_ok": "", "rows_edges": "", "rows_edges_low": "",
    "rows_negative": "minhash rows need n_rows >= 0", "skip_front_2": "minhash rows need skips of 0 or 1",
    "skip_back_negative": "minhash rows need skips of 0 or 1", "shingle_0": "minhash rows need a shingle width in 1..32",
    "shingle_33": "minhash rows need a shingle width in 1..32", "num_perm_0": "minhash rows need num_perm in 1..256",
    "num_perm_257": "minhash rows need num_perm in 1..256", "first_of_two": "minhash rows need n_rows >= 0",
    "groups_ok": "", "groups_edges": "", "groups_edges_low": "",
    "groups_negative": "minhash groups need n_rows >= 0", "groups_too_many": "minhash groups need fewer than 2^31 - 4096 rows",
    "groups_num_perm_0": "minhash groups need num_perm in 1..256", "groups_num_perm_257": "minhash groups need num_perm in 1..256",
    "bands_0": "minhash groups need bands >= 1", "bands_negative": "minhash groups need bands >= 1",
    "bands_do_not_divide": "minhash groups need a number of bands that divides num_perm",
    "bands_above_num_perm": "minhash groups need a number of bands that divides num_perm",
    "min_agree_0": "minhash groups need min_agree in 1..num_perm", "min_agree_above": "minhash groups need min_agree in 1..num_perm",
    "fit_bare": "0", "fit_framed_once": "0", "fit_framed": "1", "fit_before": "1", "fit_none": "1",
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("minhash_rules")
    src, exe = os.path.join(d, "minhash_rules_main.cpp"), os.path.join(d, "minhash_rules_main")
    with open(src, "w") as f:
        f.write(MAIN)
    c = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    if c.returncode != 0 and ("asan" in c.stderr or "ubsan" in c.stderr) and "cannot find" in c.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert c.returncode == 0, c.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)          # (a sanitizer report is a failure)
    out = {}
    for line in r.stdout.splitlines():
        name, value = line.split("|")
        assert name not in out, name
        out[name] = value
    return out


def test_every_rule_case_ran(results):
    assert sorted(results) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_minhash_rule(results, name):
    assert results[name] == EXPECTED[name]


def test_every_refusal_has_its_own_sentence():
    said = [v for k, v in EXPECTED.items() if v and not k.startswith("fit_")]
    assert len(set(said)) == 10
