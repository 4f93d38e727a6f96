"""csrc/gz_rowrules.h alone, on the CPU: the check of a host CSR input, the dense-row rule and the pairwise-disjoint check that
every row-shaping call (gz_decode_batch, gz_window_rows, gz_pack_rows, gz_mask_rows, gz_infill_rows, gz_preprocess_batch) goes
through.  A small main that includes the header is built with the host compiler under ASan + UBSan and run as a stand-alone
program; it prints one `case value` line per case, and the expectations are the table below.  No GPU, no Python extension."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")

MAIN = r"""
#include "gz_rowrules.h"
#include <cstdio>

static const uintptr_t TOP = UINTPTR_MAX;
static int two(Span a, Span b) { const Span s[2] = {a, b}; return disjoint(s, 2) ? 1 : 0; }
static void offsets(const char* name, const void* payload, const int64_t* off, int64_t n_rows)
{
    int64_t n = -12345;
    const int f = (int)rows_offsets_check(payload, off, n_rows, &n);
    std::printf("%s %d %lld\n", name, f, (long long)n);
}

int main()
{
    // disjoint
    std::printf("identical %d\n", two(Span{1000, 16}, Span{1000, 16}));
    std::printf("touching %d\n", two(Span{1000, 16}, Span{1016, 16}));
    std::printf("touching_swapped %d\n", two(Span{1016, 16}, Span{1000, 16}));
    std::printf("one_byte %d\n", two(Span{1000, 16}, Span{1015, 16}));
    std::printf("one_byte_swapped %d\n", two(Span{1015, 16}, Span{1000, 16}));
    std::printf("inside %d\n", two(Span{1000, 64}, Span{1020, 4}));
    std::printf("top_apart %d\n", two(Span{TOP - 15, 16}, Span{1000, 16}));              // its end address would wrap to 0
    std::printf("top_touching %d\n", two(Span{TOP - 31, 16}, Span{TOP - 15, 16}));
    std::printf("top_overlap %d\n", two(Span{TOP - 15, 16}, Span{TOP - 7, 8}));
    std::printf("null_address %d\n", two(Span{0, 16}, Span{8, 16}));                    // absent: nothing to overlap
    std::printf("both_null %d\n", two(Span{0, 16}, Span{0, 16}));
    std::printf("zero_bytes %d\n", two(Span{1000, 0}, Span{1000, 16}));
    std::printf("zero_bytes_inside %d\n", two(Span{1000, 16}, Span{1008, 0}));
    {
        const Span s[4] = {Span{1000, 16}, Span{0, 16}, Span{2000, 16}, Span{2015, 1}};   // only the last pair overlaps
        std::printf("last_pair %d\n", disjoint(s, 4) ? 1 : 0);
        std::printf("last_pair_left_out %d\n", disjoint(s, 3) ? 1 : 0);
        std::printf("none %d\n", disjoint(s, 0) ? 1 : 0);
    }
    // dense_rule_ok(n_rows, row_len, row_base, whole_word); 2^63 - 1 = 7 * 1317624576693539401
    const int64_t I63 = INT64_MAX;
    std::printf("plain %d\n", dense_rule_ok(40, 7, 0, 1) ? 1 : 0);
    std::printf("no_rows %d\n", dense_rule_ok(0, 1, 0, 0) ? 1 : 0);
    std::printf("cells_2p63_minus_1 %d\n", dense_rule_ok(1, 1, I63 - 1, 0) ? 1 : 0);
    std::printf("cells_2p63_minus_1_by_7 %d\n", dense_rule_ok(1317624576693539400LL, 7, 1, 1) ? 1 : 0);
    std::printf("cells_2p63 %d\n", dense_rule_ok(1, 2, (I63 >> 1), 0) ? 1 : 0);         // (2^62 - 1 + 1) * 2
    std::printf("cells_2p63_by_rows %d\n", dense_rule_ok(I63 / 2 + 1, 2, 0, 0) ? 1 : 0);
    std::printf("base_top %d\n", dense_rule_ok(1, 1, I63, 0) ? 1 : 0);                  // row_base + n_rows = 2^63: no signed sum is formed
    std::printf("all_top %d\n", dense_rule_ok(I63, INT32_MAX, I63, 1) ? 1 : 0);
    std::printf("row_len_0 %d\n", dense_rule_ok(4, 0, 0, 0) ? 1 : 0);
    std::printf("row_len_negative %d\n", dense_rule_ok(4, -1, 0, 0) ? 1 : 0);
    std::printf("rows_negative %d\n", dense_rule_ok(-1, 8, 0, 0) ? 1 : 0);
    std::printf("base_negative %d\n", dense_rule_ok(1, 8, -1, 0) ? 1 : 0);
    std::printf("whole_word_2 %d\n", dense_rule_ok(4, 8, 0, 2) ? 1 : 0);
    std::printf("whole_word_negative %d\n", dense_rule_ok(4, 8, 0, -1) ? 1 : 0);
    // rows_offsets_check(payload, off, n_rows, &n) -> fault, n
    const int32_t ids[16] = {0};
    { const int64_t off[1] = {5}; offsets("empty_batch", nullptr, off, 0); }
    { const int64_t off[3] = {3, 5, 9}; offsets("base_3", ids, off, 2); }
    { const int64_t off[4] = {0, 4, 9, 8}; offsets("decrease_last", ids, off, 3); }
    { const int64_t off[4] = {0, 9, 4, 8}; offsets("decrease_middle", ids, off, 3); }
    { const int64_t off[3] = {0, 0, 0}; offsets("null_payload_n0", nullptr, off, 2); }
    { const int64_t off[3] = {7, 7, 7}; offsets("null_payload_n0_base_7", nullptr, off, 2); }
    { const int64_t off[3] = {0, 2, 4}; offsets("null_payload_n4", nullptr, off, 2); }
    { const int64_t off[3] = {5, 6, 2}; offsets("total_negative", ids, off, 2); }         // "bad" comes before "decrease"
    { const int64_t off[2] = {INT64_MIN, INT64_MAX}; offsets("total_wraps", ids, off, 1); }
    return 0;
}
"""

OK, BAD, DECREASE = 0, 1, 2
EXPECTED = {
    # disjoint: 1 = no two present arrays share a byte
    "identical": (0,), "touching": (1,), "touching_swapped": (1,), "one_byte": (0,), "one_byte_swapped": (0,), "inside": (0,),
    "top_apart": (1,), "top_touching": (1,), "top_overlap": (0,),
    "null_address": (1,), "both_null": (1,), "zero_bytes": (1,), "zero_bytes_inside": (1,),
    "last_pair": (0,), "last_pair_left_out": (1,), "none": (1,),
    # dense_rule_ok: 1 = accepted
    "plain": (1,), "no_rows": (1,), "cells_2p63_minus_1": (1,), "cells_2p63_minus_1_by_7": (1,), "cells_2p63": (0,),
    "cells_2p63_by_rows": (0,), "base_top": (0,), "all_top": (0,), "row_len_0": (0,), "row_len_negative": (0,), "rows_negative": (0,),
    "base_negative": (0,), "whole_word_2": (0,), "whole_word_negative": (0,),
    # rows_offsets_check: (fault, elements of the batch)
    "empty_batch": (OK, 0), "base_3": (OK, 6), "decrease_last": (DECREASE, 8), "decrease_middle": (DECREASE, 8),
    "null_payload_n0": (OK, 0), "null_payload_n0_base_7": (OK, 0), "null_payload_n4": (BAD, 4), "total_negative": (BAD, -3),
    "total_wraps": (BAD, -1),
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("row_rules")
    src, exe = os.path.join(d, "row_rules_main.cpp"), os.path.join(d, "row_rules_main")
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
        name, *values = line.split()
        assert name not in out, name
        out[name] = tuple(int(v) for v in values)
    return out


def test_every_case_ran(results):
    assert sorted(results) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_row_rule(results, name):
    assert results[name] == EXPECTED[name]
