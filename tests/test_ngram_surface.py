"""CPU-only: the n-gram overlap calls exist on every layer -- the six C entry points are declared with their argument lists,
documented in the header's own section, exported and bound; _native.Context routes to them; Tokenize has ngram_index,
encode_ngram_index, ngram_overlap_rows, encode_ngram_overlap and decontaminate with their defaults, and NgramIndex is exported; the
switch ngram_hash_bits stands in the header's key list; and the new rules of csrc/gz_rowrules.h hold in a stand-alone program.
Nothing is computed on a GPU here (tests/test_gpu_ngram.py does that)."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
BUILD_TYPES = ["gz_ctx *", "const int32_t *", "const int64_t *", "int64_t", "int32_t", "int32_t", "int32_t", "gz_ngram_index **"]
OVERLAP_TYPES = ["gz_ctx *", "gz_ngram_index *", "const int32_t *", "const int64_t *", "int64_t", "int32_t", "int32_t", "int32_t *", "int32_t *",
                 "int32_t *", "int32_t *", "int32_t *", "uint8_t *"]
NAMES = {"gz_ngram_index_build": BUILD_TYPES, "gz_ngram_index_build_device": BUILD_TYPES, "gz_ngram_index_info": ["gz_ngram_index *", "int64_t"],
         "gz_ngram_overlap": OVERLAP_TYPES, "gz_ngram_overlap_device": OVERLAP_TYPES}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_minhash_rows": 11, "gz_minhash_rows_device": 11, "gz_minhash_groups": 8, "gz_minhash_groups_device": 8, "gz_window_rows": 16,
       "gz_pack_rows": 18, "gz_decode_batch_device": 10, "gz_wordset_build": 5, "gz_debug_set": 3}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, types in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        args = [a.strip() for a in decl.group(1).split(",")]
        assert [re.sub(r"\w+(\[8\])?$", "", a).strip() for a in args] == types, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == len(types), n
        assert getattr(lib, n).restype is native.C.c_int, n
    for n, argc in OLD.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == argc, n
        assert len(getattr(lib, n).argtypes) == argc, n
    assert re.search(r"\bvoid\s+gz_ngram_index_destroy\s*\(\s*gz_ngram_index\s*\*\s*\w+\s*\)\s*;", src)
    assert "typedef struct gz_ngram_index gz_ngram_index;" in src
    assert hasattr(lib, "gz_ngram_index_destroy") and "gz_ngram_index_destroy" in native.SYMBOLS
    assert lib.gz_ngram_index_destroy.restype is None
    assert lib.gz_version() == 0x010100
    C = native.C
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.gz_ngram_index_build.argtypes == [vp, vp, vp, i64, i32, i32, i32, C.POINTER(vp)]
    assert lib.gz_ngram_index_build_device.argtypes == lib.gz_ngram_index_build.argtypes
    assert lib.gz_ngram_index_info.argtypes == [vp, vp]
    assert lib.gz_ngram_index_destroy.argtypes == [vp]
    assert lib.gz_ngram_overlap.argtypes == [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp]
    assert lib.gz_ngram_overlap_device.argtypes == lib.gz_ngram_overlap.argtypes
    for m in ("ngram_index_build", "ngram_index_build_device", "ngram_index_info", "ngram_index_destroy", "ngram_overlap", "ngram_overlap_device"):
        assert callable(getattr(native.Context, m)), m
    assert native.Context.NGRAM_OUT == ("n_grams", "n_hits", "n_covered", "first_hit", "first_ref")


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("token n-gram overlap against a held-out set"):]
    comment = block[:block.index("typedef struct gz_ngram_index gz_ngram_index;")]
    for word in ("skip_front", "skip_back", "empty body", "max(0, m - n + 1)", "1..32", "NONE", "first(g)", "smallest reference row",
                 "owns a copy", "n_grams[r]", "n_hits[r]", "n_covered[r]", "first_hit[r]", "first_ref[r]", "i <= t < i + n", "-1",
                 "covered", "frame cells", "overlap(rows[a:b]) == overlap(rows)[a:b]", "pure function", "MurmurHash3_x86_32", "0x9E3779B9",
                 "0xCC9E2D51", "0x1B873593", "0xE6546B64", "fmix32", "tag", "start slot", "ngram_hash_bits", "power of two", "twice",
                 "8 bytes a slot", "position + 1", "0 = free", "compare-and-swap", "atomic minimum", "binary search",
                 "bytes a reference token", "GZ_E_INVALID", "GZ_E_LIMIT", "2^32 - 1", "2^31", "n_rows < 0", "out handle", "overlap the input",
                 "row offsets", "another context", "n_rows == 0", "gz_ngram_index_build:", "gz_ngram_index_build_device:", "ABSOLUTE",
                 "gz_ngram_index_info:", "info[8]", "gz_ngram_index_destroy:", "gz_ngram_overlap:", "gz_ngram_overlap_device:",
                 "swap the roles", "Not here"):
        assert word in comment, word
    assert "GZ_E_NOTABLES" not in comment                                  # a bare context is enough
    # a section of its own, behind the learner's and before the text pre-pass
    assert src.index("gz_bpe_learn_result(") < src.index("token n-gram overlap against a held-out set") < src.index("---- text pre-pass")
    keys = src[src.index("Keys\n * (value range; default):"):src.index("int  gz_debug_set(")]
    assert "ngram_hash_bits (0..32; 0)" in keys
    assert keys.index("bm25_hash_bits (0..62; 0)") < keys.index("ngram_hash_bits (0..32; 0)")


def test_kernels_are_their_own_file():
    hip = open(os.path.join(CSRC, "gz_kernels.hip")).read()
    assert hip.index('#include "gz_pieces.inc"') < hip.index('#include "gz_minhash.inc"') < hip.index('#include "gz_ngram.inc"')   # (the piece rules; fmix32)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "gz_ngram.inc" in make and "gz_ngram_api.inc" in make           # the build identity covers both
    inc = open(os.path.join(CSRC, "gz_ngram.inc")).read()
    for word in ("piece_row", "gz_ngram_insert_kernel", "gz_ngram_query_kernel", "gz_ngram_resolve_kernel", "atomicCAS", "atomicMin",
                 "wballot", "__shfl"):
        assert word in inc, word
    assert "__shared__" not in inc                                         # coverage by ballots and shifts: no LDS


def test_tokenize_signatures():
    import genz_tokenize
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    empty = inspect.Parameter.empty
    want = {
        "ngram_index": [("rows", empty), ("n", 13), ("framed", True)],
        "encode_ngram_index": [("texts", empty), ("n", 13), ("word_table", True)],
        "ngram_overlap_rows": [("rows", empty), ("index", empty), ("framed", True), ("return_covered", False)],
        "encode_ngram_overlap": [("texts", empty), ("index", empty), ("word_table", True)],
        "decontaminate": [("texts", empty), ("index", empty), ("max_fraction", 0.0)],
    }
    for name, params in want.items():
        p = inspect.signature(getattr(tokenize.Tokenize, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in params], name
        for k, d in params:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
        doc = getattr(tokenize.Tokenize, name).__doc__
        assert doc and len(doc) > 100, name
    for name in ("ngram_index", "encode_ngram_index", "decontaminate"):
        assert "swap the roles" in getattr(tokenize.Tokenize, name).__doc__.lower(), name
    assert "ngram_overlap_rows(rows[a:b])` is `ngram_overlap_rows(rows)[a:b]" in tokenize.Tokenize.ngram_overlap_rows.__doc__
    assert "shards concatenate" in tokenize.Tokenize.encode_ngram_overlap.__doc__
    assert isinstance(inspect.getattr_static(tokenize.Tokenize, "_ngram_rule"), staticmethod)
    assert genz_tokenize.NgramIndex is tokenize.NgramIndex and "NgramIndex" in genz_tokenize.__all__
    for prop in ("n", "n_rows", "n_ids", "n_grams", "n_distinct", "device_bytes"):
        assert isinstance(inspect.getattr_static(tokenize.NgramIndex, prop), property), prop
    for m in ("close", "__enter__", "__exit__"):
        assert callable(getattr(tokenize.NgramIndex, m)), m
    # the neighbours are what they were
    assert list(inspect.signature(tokenize.Tokenize.minhash_rows).parameters) == ["self", "rows", "num_perm", "shingle", "seed", "framed"]
    assert list(inspect.signature(tokenize.Tokenize.near_duplicates).parameters) == ["self", "texts", "num_perm", "shingle", "seed", "bands",
                                                                                      "threshold", "min_agree", "word_table"]


# ---- the rules of gz_rowrules.h, alone ------------------------------------------------------------------------------------------
MAIN = r"""
#include "gz_rowrules.h"
#include <cstdio>
#include <vector>

static void build(const char* name, int64_t rows, int32_t sf, int32_t sb, int32_t n)
{
    const char* why = ngram_build_fault(rows, sf, sb, n);
    std::printf("%s|%s\n", name, why ? why : "");
}
static void query(const char* name, int64_t rows, int32_t sf, int32_t sb)
{
    const char* why = ngram_overlap_fault(rows, sf, sb);
    std::printf("%s|%s\n", name, why ? why : "");
}

int main()
{
    build("build_ok", 5, 1, 1, 13);
    build("build_edges", 0, 0, 1, 32);
    build("build_edges_low", (int64_t)INT32_MAX, 1, 0, 1);
    build("build_negative", -1, 0, 0, 13);
    build("build_too_many_rows", (int64_t)INT32_MAX + 1, 0, 0, 13);
    build("build_skip_front_2", 1, 2, 0, 13);
    build("build_skip_back_negative", 1, 0, -1, 13);
    build("build_n_0", 1, 0, 0, 0);
    build("build_n_33", 1, 0, 0, 33);
    build("build_n_negative", 1, 0, 0, -13);
    build("build_first_of_two", -1, 0, 0, 0);
    query("query_ok", 5, 1, 1);
    query("query_edges", 0, 0, 1);
    query("query_many", INT64_MAX, 1, 0);
    query("query_negative", -1, 0, 0);
    query("query_skip_front_2", 1, 2, 0);
    query("query_skip_back_negative", 1, 0, -1);
    std::printf("ids_none|%d\n", ngram_ids_fit(0) ? 1 : 0);
    std::printf("ids_most|%d\n", ngram_ids_fit(((int64_t)1 << 32) - 2) ? 1 : 0);            // position + 1 = 2^32 - 1 still fits 32 bits
    std::printf("ids_limit|%d\n", ngram_ids_fit(((int64_t)1 << 32) - 1) ? 1 : 0);
    std::printf("ids_beyond|%d\n", ngram_ids_fit((int64_t)1 << 40) ? 1 : 0);
    std::printf("ids_negative|%d\n", ngram_ids_fit(-1) ? 1 : 0);
    {
        std::vector<int64_t> off = {3, 3, 10, 10 + ((int64_t)1 << 31) + 1, 10 + ((int64_t)1 << 31) + 1};
        std::printf("body_bare|%d\n", minhash_bodies_fit(off.data(), 4, 0, 0) ? 1 : 0);              // a body of 2^31 + 1
        std::printf("body_framed|%d\n", minhash_bodies_fit(off.data(), 4, 1, 1) ? 1 : 0);            // 2^31 - 1
    }
    return 0;
}
"""

EXPECTED = {
    "build_ok": "", "build_edges": "", "build_edges_low": "",
    "build_negative": "n-gram index needs n_rows >= 0", "build_too_many_rows": "n-gram index needs fewer than 2^31 reference rows",
    "build_skip_front_2": "n-gram index needs skips of 0 or 1", "build_skip_back_negative": "n-gram index needs skips of 0 or 1",
    "build_n_0": "n-gram index needs a width n in 1..32", "build_n_33": "n-gram index needs a width n in 1..32",
    "build_n_negative": "n-gram index needs a width n in 1..32", "build_first_of_two": "n-gram index needs n_rows >= 0",
    "query_ok": "", "query_edges": "", "query_many": "",
    "query_negative": "n-gram overlap needs n_rows >= 0", "query_skip_front_2": "n-gram overlap needs skips of 0 or 1",
    "query_skip_back_negative": "n-gram overlap needs skips of 0 or 1",
    "ids_none": "1", "ids_most": "1", "ids_limit": "0", "ids_beyond": "0", "ids_negative": "0",
    "body_bare": "0", "body_framed": "1",
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("ngram_rules")
    src, exe = os.path.join(d, "ngram_rules_main.cpp"), os.path.join(d, "ngram_rules_main")
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
def test_ngram_rule(results, name):
    assert results[name] == EXPECTED[name]


def test_every_refusal_has_its_own_sentence():
    said = [v for k, v in EXPECTED.items() if v and not k.startswith(("ids_", "body_"))]
    assert len(set(said)) == 6
