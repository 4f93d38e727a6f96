"""CPU-only: the n-gram repetition calls exist on every layer -- the two C entry points are declared with their argument lists,
documented in the header's own section, exported and bound; _native.Context routes to them; Tokenize has repetition_rows,
encode_repetition and repetition_filter with their defaults; the switch repeat_hash_bits stands in the header's key list; the
kernels are their own file; and repeat_fault of csrc/gz_rowrules.h holds in a stand-alone program.  Nothing is computed on a GPU here
(tests/test_gpu_repeat.py does that)."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
TYPES = ["gz_ctx *", "const int32_t *", "const int64_t *", "int64_t", "int32_t", "int32_t", "const int32_t *", "int32_t", "int32_t *", "int32_t *",
         "int32_t *", "int32_t *", "int32_t *", "int32_t *", "uint16_t *"]
NAMES = {"gz_ngram_repeats": TYPES, "gz_ngram_repeats_device": TYPES}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_ngram_index_build": 8, "gz_ngram_index_build_device": 8, "gz_ngram_overlap": 13, "gz_ngram_overlap_device": 13, "gz_minhash_rows": 11,
       "gz_minhash_rows_device": 11, "gz_minhash_groups": 8, "gz_align_rows": 16, "gz_word_spans": 9, "gz_debug_set": 3}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, types in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        args = [a.strip() for a in decl.group(1).split(",")]
        assert [re.sub(r"\w+$", "", a).strip() for a in args] == types, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == len(types), n
        assert getattr(lib, n).restype is native.C.c_int, n
    for n, argc in OLD.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == argc, n
        assert len(getattr(lib, n).argtypes) == argc, n
    assert lib.gz_version() == 0x010100
    C = native.C
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.gz_ngram_repeats.argtypes == [vp, vp, vp, i64, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    assert lib.gz_ngram_repeats_device.argtypes == lib.gz_ngram_repeats.argtypes
    for m in ("ngram_repeats", "ngram_repeats_device"):
        assert callable(getattr(native.Context, m)), m
    assert native.Context.REPEAT_OUT == ("n_grams", "n_distinct", "n_repeated", "n_covered", "top_count", "top_pos")
    assert native.Context.NGRAM_OUT == ("n_grams", "n_hits", "n_covered", "first_hit", "first_ref")


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("---- repeats: n-gram repetition inside a document"):]
    comment = block[:block.index("int  gz_ngram_repeats(")]
    for word in ("Gopher", "MOST FREQUENT", "MORE THAN ONCE", "skip_front", "skip_back", "empty body", "1..16 distinct", "1..32", "caller's order",
                 "G = max(0, m - n + 1)", "shorter than n has none", "occurrences may overlap", "[5, 5, 5]", "first(g)", "[K, N]",
                 "n_grams[k, r]", "n_distinct[k, r]", "later occurrences", "n_repeated[k, r]", "c(q[i:i+n]) >= 2", "first occurrence counts too",
                 "n_covered[k, r]", "i <= t < i + n", "counts once", "top_count[k, r]", "top_pos[k, r]", "smallest first", "-1 when G == 0",
                 "uint16", "Bit k", "frame cells", "repetition(rows[a:b]) == repetition(rows)[:, a:b]", "identical neighbour",
                 "shards concatenate", "pure function",
                 "A hash decides where to look, never whether two n-grams are equal, nor whether they stand in the same row",
                 "cleared per width", "power of two", "twice", "smallest width", "half", "8 bytes", "tag << 32 | (position + 1)", "row_off[0]",
                 "0 = free", "4 bytes in a parallel array", "compare-and-swap", "inside this row's n-gram", "atomic minimum", "incremented",
                 "one key for good", "c << 32 | (0xFFFFFFFF - first)", "ballot", "minimum, maximum or sum", "0x9E3779B97F4A7C15",
                 "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "repeat_hash_bits", "tag = h64 >> 32", "start slot", "does not depend on it",
                 "12 bytes a slot", "16 bytes a row", "widths on the HOST", "may be NULL", "GZ_E_INVALID", "n_rows < 0", "n_widths outside 1..16",
                 "a width outside 1..32", "a repeated width", "decreasing row offsets", "overlap the input", "GZ_E_LIMIT", "2^31", "2^32 - 1",
                 "n_rows == 0", "touches nothing", "gz_ngram_repeats:", "gz_ngram_repeats_device:", "ABSOLUTE", "Not here", "LDS",
                 "line and paragraph duplicates", "across documents", "multi-GPU"):
        assert word in comment, word
    assert "GZ_E_NOTABLES" not in comment                                  # a bare context is enough
    # a section of its own, behind the align section and before the text pre-pass
    assert src.index("gz_span_labels_device(") < src.index("---- repeats: n-gram repetition inside a document") < src.index("---- text pre-pass")
    assert src.index("---- repeats: n-gram repetition inside a document") < src.index("int  gz_ngram_repeats(") < src.index("---- text pre-pass")
    keys = src[src.index("Keys\n * (value range; default):"):src.index("int  gz_debug_set(")]
    assert "repeat_hash_bits (0..32; 0)" in keys
    assert keys.index("ngram_hash_bits (0..32; 0)") < keys.index("repeat_hash_bits (0..32; 0)")


def test_kernels_are_their_own_file():
    hip = open(os.path.join(CSRC, "gz_kernels.hip")).read()
    assert hip.index('#include "gz_ngram.inc"') < hip.index('#include "gz_repeat.inc"')       # (it shares the hash, the comparison and the piece rule)
    api = open(os.path.join(CSRC, "gz_api.cpp")).read()
    assert api.index('#include "gz_ngram_api.inc"') < api.index('#include "gz_repeat_api.inc"')
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "gz_repeat.inc" in make and "gz_repeat_api.inc" in make          # the build identity covers both
    inc = open(os.path.join(CSRC, "gz_repeat.inc")).read()
    for word in ("piece_row", "gz_repeat_insert_kernel", "gz_repeat_query_kernel", "atomicCAS", "atomicMin", "atomicAdd", "atomicMax",
                 "wballot", "ng_trip_hash", "ng_equal", "piece_grams", "GZ_PIECE", "GzRepeatArgs"):
        assert word in inc, word
    assert "__shared__" not in inc                                         # one path: no LDS table
    # rows are divided into pieces in ONE place: the constant, the count kernel and the walk stand in gz_pieces.inc, which the
    # build identity covers and which comes in front of its three users; each of them uses the walk
    pieces = open(os.path.join(CSRC, "gz_pieces.inc")).read()
    for word in ("constexpr int GZ_PIECE = 4096;", "void gz_piece_count_kernel(", "piece_row(const Args& A", "piece_body(", "piece_shingles(", "piece_grams(",
                 "wave_sum", "atomicAdd", "atomicOr"):
        assert word in pieces, word
    hdrs = re.search(r"^HDRS := (.*)$", make, flags=re.M).group(1).split()
    assert "gz_pieces.inc" in hdrs
    assert hip.index('#include "gz_pieces.inc"') < hip.index('#include "gz_minhash.inc"') < hip.index('#include "gz_ngram.inc"')
    for name in ("gz_minhash.inc", "gz_ngram.inc", "gz_repeat.inc"):
        text = open(os.path.join(CSRC, name)).read()
        assert "piece_row(A, p, " in text, name
        assert not re.search(r"constexpr\s+\w+\s+GZ_\w*PIECE\b", text) and "lo + hi + 1" not in text.split("gz_ngram_resolve_kernel")[0], name
    whole = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".inc", ".h", ".hip", ".cpp", ".c"))}
    for name, text in whole.items():
        assert not re.search(r"\bh_pick\b", text), name                    # the pinned block is a struct: no user reaches it by a number
        assert not re.search(r"gz_(minhash|ngram|repeat)_count_kernel|gz_launch_(minhash|ngram|repeat)_count|GZ_(MINHASH|NGRAM)_PIECE", text), name
    assert sum(text.count("void gz_piece_count_kernel(") for text in whole.values()) == 1
    assert sum(len(re.findall(r"^void gz_launch_piece_count\(", text, flags=re.M)) for text in whole.values()) == 2      # declared, defined
    assert "struct GzPinned" in api and "sizeof(GzPinned)" in api
    assert "__shared__" not in open(os.path.join(CSRC, "gz_ngram.inc")).read()
    assert "struct GzRepeatArgs" in open(os.path.join(CSRC, "gz_kernels.h")).read()
    host = open(os.path.join(CSRC, "gz_host_api.cpp")).read()
    assert '{"repeat_hash_bits", &GzOptions::repeat_hash_bits, nullptr, 0, 32}' in host


def test_tokenize_signatures():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    T = tokenize.Tokenize
    empty = inspect.Parameter.empty
    nine = (2, 3, 4, 5, 6, 7, 8, 9, 10)
    want = {
        "repetition_rows": [("rows", empty), ("widths", nine), ("framed", True), ("return_covered", False)],
        "encode_repetition": [("texts", empty), ("widths", nine), ("word_table", True)],
        "repetition_filter": [("texts", empty), ("top_max", None), ("dup_max", None)],
    }
    for name, params in want.items():
        p = inspect.signature(getattr(T, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in params], name
        for k, d in params:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
        doc = getattr(T, name).__doc__
        assert doc and len(doc) > 100, name
    assert "repetition_rows(rows[a:b])` is `repetition_rows(rows)[:, a:b]" in T.repetition_rows.__doc__
    assert "shards concatenate" in T.repetition_rows.__doc__ and "shards concatenate" in T.encode_repetition.__doc__
    assert "term_sequences()" in T.repetition_rows.__doc__ and "word n-grams" in T.repetition_rows.__doc__
    doc = " ".join(T.repetition_filter.__doc__.split())
    for word in ("{2: 0.20, 3: 0.18, 4: 0.16}", "{5: 0.15, 6: 0.14, 7: 0.13, 8: 0.12, 9: 0.11, 10: 0.10}", "Gopher", "CHARACTER shares of WORD",
                 "TOKEN shares", "tunes", "both empty is refused"):
        assert word in doc, word
    assert isinstance(inspect.getattr_static(T, "_repeat_rule"), staticmethod)
    assert list(inspect.signature(T._repeat_rule).parameters) == ["widths"]
    # the neighbours are what they were
    assert list(inspect.signature(T.ngram_overlap_rows).parameters) == ["self", "rows", "index", "framed", "return_covered"]
    assert list(inspect.signature(T.encode_ngram_overlap).parameters) == ["self", "texts", "index", "word_table"]
    assert list(inspect.signature(T.decontaminate).parameters) == ["self", "texts", "index", "max_fraction"]
    assert list(inspect.signature(T.minhash_rows).parameters) == ["self", "rows", "num_perm", "shingle", "seed", "framed"]


# ---- the rule of gz_rowrules.h, alone ---------------------------------------------------------------------------------------
MAIN = r"""
#include "gz_rowrules.h"
#include <cstdio>
#include <vector>

static void call(const char* name, int64_t rows, int32_t sf, int32_t sb, std::vector<int32_t> w, int32_t n_widths = -99, bool null_widths = false)
{
    // (the vector is sized exactly: a read beyond n_widths entries is a sanitizer report)
    const char* why = repeat_fault(rows, sf, sb, null_widths ? nullptr : w.data(), n_widths == -99 ? (int32_t)w.size() : n_widths);
    std::printf("%s|%s\n", name, why ? why : "");
}

int main()
{
    std::vector<int32_t> sixteen, seventeen;
    for (int32_t i = 1; i <= 16; ++i) sixteen.push_back(2 * i);
    for (int32_t i = 1; i <= 17; ++i) seventeen.push_back(i);
    call("ok_default", 5, 1, 1, {2, 3, 4, 5, 6, 7, 8, 9, 10});
    call("ok_one", 0, 0, 1, {13});
    call("ok_sixteen", INT64_MAX, 1, 0, sixteen);
    call("ok_edges_unordered", 1, 0, 0, {32, 1, 31});
    call("negative_rows", -1, 0, 0, {2});
    call("skip_front_2", 1, 2, 0, {2});
    call("skip_back_negative", 1, 0, -1, {2});
    call("no_widths", 1, 0, 0, {});
    call("negative_count", 1, 0, 0, {2}, -1);
    call("seventeen", 1, 0, 0, seventeen);
    call("null_widths", 1, 0, 0, {}, 3, true);
    call("width_0", 1, 0, 0, {2, 0});
    call("width_33", 1, 0, 0, {33, 2});
    call("width_negative", 1, 0, 0, {2, 3, -4});
    call("width_64", 1, 0, 0, {64});
    call("repeated", 1, 0, 0, {5, 6, 5});
    call("repeated_32", 1, 0, 0, {32, 32});
    call("first_of_many", -1, 3, 3, {0, 0}, 40);
    call("list_order", 1, 0, 0, {2, 2, 40});
    std::printf("ids_most|%d\n", ngram_ids_fit(((int64_t)1 << 32) - 2) ? 1 : 0);            // position + 1 = 2^32 - 1 still fits 32 bits
    std::printf("ids_limit|%d\n", ngram_ids_fit(((int64_t)1 << 32) - 1) ? 1 : 0);
    {
        std::vector<int64_t> off = {3, 3, 10, 10 + ((int64_t)1 << 31) + 1};
        std::printf("body_bare|%d\n", minhash_bodies_fit(off.data(), 3, 0, 0) ? 1 : 0);              // a body of 2^31 + 1
        std::printf("body_framed|%d\n", minhash_bodies_fit(off.data(), 3, 1, 1) ? 1 : 0);            // 2^31 - 1
    }
    // the position total a count pass may report: 10 rows, 1000 ids, framed, n = 5: between 1000 - 10 * 6 and 1000
    std::printf("ids_pos_least|%d\n", ngram_positions_possible(940, 1000, 10, 1, 1, 5) ? 1 : 0);
    std::printf("ids_pos_most|%d\n", ngram_positions_possible(1000, 1000, 10, 1, 1, 5) ? 1 : 0);
    std::printf("ids_pos_below|%d\n", ngram_positions_possible(939, 1000, 10, 1, 1, 5) ? 1 : 0);
    std::printf("ids_pos_above|%d\n", ngram_positions_possible(1001, 1000, 10, 1, 1, 5) ? 1 : 0);
    std::printf("ids_pos_short_rows|%d\n", ngram_positions_possible(0, 1000, 500, 0, 0, 32) ? 1 : 0);        // every row may be shorter than n
    std::printf("ids_pos_negative|%d\n", ngram_positions_possible(-1, 1000, 500, 0, 0, 32) ? 1 : 0);
    std::printf("ids_pos_unigrams|%d\n", ngram_positions_possible(1000, 1000, 10, 0, 0, 1) ? 1 : 0);          // n = 1, bare: exactly the ids
    std::printf("ids_pos_unigrams_fewer|%d\n", ngram_positions_possible(999, 1000, 10, 0, 0, 1) ? 1 : 0);
    std::printf("ids_pos_many_rows|%d\n", ngram_positions_possible(0, 5, INT64_MAX, 1, 1, 32) ? 1 : 0);       // (no product wraps)
    return 0;
}
"""

EXPECTED = {
    "ok_default": "", "ok_one": "", "ok_sixteen": "", "ok_edges_unordered": "",
    "negative_rows": "n-gram repeats need n_rows >= 0",
    "skip_front_2": "n-gram repeats need skips of 0 or 1", "skip_back_negative": "n-gram repeats need skips of 0 or 1",
    "no_widths": "n-gram repeats need 1..16 widths", "negative_count": "n-gram repeats need 1..16 widths",
    "seventeen": "n-gram repeats need 1..16 widths",
    "null_widths": "n-gram repeats need the widths",
    "width_0": "n-gram repeats need every width in 1..32", "width_33": "n-gram repeats need every width in 1..32",
    "width_negative": "n-gram repeats need every width in 1..32", "width_64": "n-gram repeats need every width in 1..32",
    "repeated": "n-gram repeats need distinct widths", "repeated_32": "n-gram repeats need distinct widths",
    "first_of_many": "n-gram repeats need n_rows >= 0", "list_order": "n-gram repeats need distinct widths",
    "ids_most": "1", "ids_limit": "0", "body_bare": "0", "body_framed": "1",
    "ids_pos_least": "1", "ids_pos_most": "1", "ids_pos_below": "0", "ids_pos_above": "0", "ids_pos_short_rows": "1", "ids_pos_negative": "0", "ids_pos_unigrams": "1",
    "ids_pos_unigrams_fewer": "0", "ids_pos_many_rows": "1",
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("repeat_rules")
    src, exe = os.path.join(d, "repeat_rules_main.cpp"), os.path.join(d, "repeat_rules_main")
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
def test_repeat_rule(results, name):
    assert results[name] == EXPECTED[name]


def test_every_refusal_has_its_own_sentence():
    said = [v for k, v in EXPECTED.items() if v and not k.startswith(("ids_", "body_"))]
    assert len(set(said)) == 6
