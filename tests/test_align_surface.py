"""CPU-only: the align calls exist on every layer -- the six C entry points are declared with their argument lists, documented in the
header's own section, exported and bound; _native.Context routes to them; Tokenize has word_spans, align_rows, span_labels and
encode_aligned with their defaults; the Python refusals are raised before any device call; and the new rules of csrc/gz_rowrules.h
hold in a stand-alone program under ASan and UBSan.  Nothing is computed on a GPU here (tests/test_gpu_align.py does that)."""
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
I32, CI32, CI64, I64 = "int32_t *", "const int32_t *", "const int64_t *", "int64_t *"
NAMES = {
    "gz_word_spans": ["gz_ctx *", "const uint8_t *", CI64, "int64_t", "int32_t", I32, I64, "int64_t", I64],
    "gz_word_spans_device": ["gz_ctx *", "const uint8_t *", CI64, "int64_t", "int64_t", "int32_t", I32, I64, "int64_t", I64],
    "gz_align_rows": ["gz_ctx *", CI32, CI64, "int64_t", CI32, CI32, "int64_t", "int32_t", CI32, "int32_t", CI32, "int32_t", "int32_t", I32, I32, I32],
    "gz_align_rows_device": ["gz_ctx *", CI32, CI64, "int64_t", "int64_t", CI32, CI32, "int64_t", "int32_t", CI32, "int32_t", CI32, "int32_t", "int32_t",
                             I32, I32, I32],
    "gz_span_labels": ["gz_ctx *", CI32, CI64, "int64_t", CI32, CI64, "int32_t", "int32_t", I32, I32],
    "gz_span_labels_device": ["gz_ctx *", CI32, CI64, "int64_t", "int64_t", CI32, CI64, "int64_t", "int32_t", "int32_t", I32, I32],
}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_window_rows": 16, "gz_window_rows_device": 16, "gz_wordset_build": 5, "gz_wordset_build_device": 6, "gz_word_token_counts": 6,
       "gz_ngram_overlap": 13, "gz_pack_rows": 18}


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
    assert lib.gz_word_spans.argtypes == [vp, vp, vp, i64, i32, vp, vp, i64, C.POINTER(i64)]
    assert lib.gz_word_spans_device.argtypes == [vp, vp, vp, i64, i64, i32, vp, vp, i64, C.POINTER(i64)]
    assert lib.gz_align_rows.argtypes == [vp, vp, vp, i64, vp, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp, vp]
    assert lib.gz_align_rows_device.argtypes == [vp, vp, vp, i64, i64, vp, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp, vp]
    assert lib.gz_span_labels.argtypes == [vp, vp, vp, i64, vp, vp, i32, i32, vp, vp]
    assert lib.gz_span_labels_device.argtypes == [vp, vp, vp, i64, i64, vp, vp, i64, i32, i32, vp, vp]
    for m in ("word_spans", "word_spans_device", "align_rows", "align_rows_device", "span_labels", "span_labels_device"):
        assert callable(getattr(native.Context, m)), m


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("---- align: word spans, word ids and aligned token labels"):]
    comment = block[:block.index("int  gz_word_spans(")]
    for word in ("\\S+\\n?", "str.isspace", "document boundary ends a word", "c_j >= 1", "exclusive scan", "T_d", "room = max_len - 2",
                 "start >= T_doc", "Cell 0 is bos", "tokenize.py:141-146", "gz_window_rows", "gz_wordset_build", "ABSOLUTE", "text_bytes",
                 "0 code points", "1 bytes", "[begin, end)", "glued line feed", "character at `end`", "word_off [n_docs + 1]",
                 "not 10xxxxxx", "surrogatepass", "lone surrogates", "4-byte", "Nothing leaves its document", "span == NULL sizes only",
                 "GZ_E_CAPACITY", "span is untouched", "2^31 bytes", "W >= 2^31", "GZ_E_LIMIT", "doc_first", "gz_word_token_counts",
                 "row_doc == NULL", "n_rows == n_docs", "row_start == NULL", "max_len >= 3", "0 ignore, 1 same, 2 map", "cont_map [n_map]",
                 "C_j <= t < C_{j+1}", "word_ids = -1", "ignore_index", "t == C_j", "else v unchanged", "per token, not per row",
                 "begins with a continuation cell", "n_real = chunk length + 2", "each with its own sentence", "a count below 1",
                 "decreasing offsets", "a row_doc outside", "a negative row_start", "labels without word_labels", "map mode without a map",
                 "trusts what it cannot read", "marks [S, 3]", "mark_off", "0 plain, 1 BIO", "mark_words [S, 2]", "(-1, -1)", "end <= begin",
                 "begin < e and b < end", "touching is not overlapping", "whitespace only", "past the document's end", "SMALLEST MARK INDEX",
                 "2 * label + 1", "2 * label + 2", "still begins with a B", "negative label under BIO", "Not here", "sentence pairs",
                 "unk piece has no length", "IOBES", "single texts only", "exact integer"):
        assert word in comment, word
    # a section of its own, behind the n-gram overlap and before the text pre-pass
    assert src.index("gz_ngram_overlap_device(") < src.index("---- align: word spans") < src.index("---- text pre-pass")


def test_kernels_are_their_own_file():
    hip = open(os.path.join(CSRC, "gz_kernels.hip")).read()
    assert hip.index('#include "gz_pipeline.inc"') < hip.index('#include "gz_align.inc"')       # (the word rule is the pipeline's)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "gz_align.inc" in make                                          # the build identity covers it
    inc = open(os.path.join(CSRC, "gz_align.inc")).read()
    for word in ("gz_span_scan_kernel", "gz_span_doc_kernel", "gz_span_write_kernel", "gz_align_rows_kernel", "gz_align_rows_lds_kernel", "nt_store4", "gz_spanlab_mark_kernel",
                 "gz_spanlab_word_kernel", "is_ws1(", "is_ws2(", "is_ws3(", "atomicMin", "wave_excl_sum"):
        assert word in inc, word
    assert not re.search(r"\bbool\s+is_ws[123]\s*\(", inc)                 # reused, not restated
    for name in ("gz_hot.inc", "gz_dropout.inc"):
        assert "gz_span" not in open(os.path.join(CSRC, name)).read()


def test_tokenize_signatures():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    empty = inspect.Parameter.empty
    want = {
        "word_spans": [("texts", empty), ("unit", "char")],
        "align_rows": [("counts", empty), ("word_off", empty), ("max_len", empty), ("word_labels", None), ("row_doc", None), ("row_start", None),
                       ("continuation", "ignore"), ("ignore_index", -100)],
        "span_labels": [("span", empty), ("word_off", empty), ("marks", empty), ("scheme", "bio"), ("outside", 0)],
        "encode_aligned": [("texts", empty), ("max_len", empty), ("word_labels", None), ("marks", None), ("stride", None), ("continuation", "ignore"),
                           ("scheme", "bio"), ("ignore_index", -100), ("unit", "char"), ("word_table", True)],
    }
    for name, params in want.items():
        p = inspect.signature(getattr(tokenize.Tokenize, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in params], name
        for k, d in params:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
        doc = getattr(tokenize.Tokenize, name).__doc__
        assert doc and len(doc) > 100, name
    # the neighbours are what they were
    assert list(inspect.signature(tokenize.Tokenize.encode_windows).parameters) == ["self", "texts", "max_len", "stride", "word_table"]
    assert list(inspect.signature(tokenize.Tokenize.window_rows).parameters) == ["self", "rows", "max_len", "stride", "framed"]


class _NoNative:
    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = _NoNative()

    def no_tables():
        raise AssertionError("tables synchronised before the arguments were validated")
    t._sync_tables = no_tables
    return t


def test_python_refusals_come_before_any_device_call():
    t = _bare()
    with pytest.raises(ValueError):
        t.word_spans(["a"], unit="rune")
    with pytest.raises(TypeError):
        t.word_spans(["a"], unit=0)
    with pytest.raises(TypeError):
        t.word_spans([b"a"])
    counts, off = np.array([1, 2, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64)
    for kw, exc in ((dict(max_len=2), ValueError), (dict(max_len=True), TypeError), (dict(max_len=16.0), TypeError),
                    (dict(max_len=16, ignore_index=2 ** 31), ValueError), (dict(max_len=16, continuation="next"), ValueError),
                    (dict(max_len=16, continuation=np.zeros(0, dtype=np.int32)), ValueError),
                    (dict(max_len=16, continuation=np.zeros(3)), TypeError),
                    (dict(max_len=16, word_labels=[1, 2]), ValueError), (dict(max_len=16, word_labels=[1.0, 2.0, 3.0]), TypeError),
                    (dict(max_len=16, row_doc=[0, 2]), ValueError), (dict(max_len=16, row_doc=[-1]), ValueError),
                    (dict(max_len=16, row_doc=[0, 1, 1], row_start=[0, 1]), ValueError), (dict(max_len=16, row_start=[0, -1]), ValueError),
                    (dict(max_len=16, row_start=[0]), ValueError)):
        with pytest.raises(exc):
            t.align_rows(counts, off, **kw)
    for c, o, exc in ((np.array([1, 0, 1]), off, ValueError), (counts, np.array([0, 3, 2]), ValueError), (counts, np.array([1, 2, 3]), ValueError),
                      (counts, np.array([0, 2, 4]), ValueError), (counts, np.array([0.0, 3.0]), TypeError), (np.array([[1, 2, 1]]), off, ValueError),
                      (np.array([1, 2, 2 ** 40]), off, ValueError)):
        with pytest.raises(exc):
            t.align_rows(c, o, 16)
    span, woff = np.array([[0, 1], [2, 3], [0, 4]], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64)
    good = [[(0, 1, 1)], []]
    for a, kw, exc in (((span, woff, good), dict(scheme="iobes"), ValueError), ((span, woff, good), dict(scheme=1), TypeError),
                       ((span, woff, good), dict(outside=1.5), TypeError), ((span[:, :1], woff, good), {}, ValueError),
                       ((span, np.array([0, 2, 4]), good), {}, ValueError), ((span, woff, [[(0, 1, 1)]]), {}, ValueError),
                       ((span, woff, [[(0, 1)], []]), {}, ValueError), ((span, woff, [[(0, 1, -1)], []]), {}, ValueError),
                       ((span, woff, [[(0, 1.5, 1)], []]), {}, TypeError), ((span, woff, [[(0, 2 ** 31, 1)], []]), {}, ValueError),
                       ((span, woff, (np.zeros((2, 2), dtype=np.int32), np.array([0, 1, 2]))), {}, ValueError),
                       ((span, woff, (np.zeros((2, 3), dtype=np.int32), np.array([0, 1, 3]))), {}, ValueError),
                       ((span, woff, (np.zeros((2, 3), dtype=np.int32), np.array([0, 2]))), {}, ValueError)):
        with pytest.raises(exc):
            t.span_labels(*a, **kw)
    for kw, exc in ((dict(max_len=2), ValueError), (dict(max_len=16, stride=14), ValueError), (dict(max_len=16, stride=-1), ValueError),
                    (dict(max_len=16, stride=1.0), TypeError), (dict(max_len=16, word_labels=[1], marks=[[]]), ValueError),
                    (dict(max_len=16, unit="word"), ValueError), (dict(max_len=16, scheme="bilou"), ValueError),
                    (dict(max_len=16, continuation="first"), ValueError), (dict(max_len=16, ignore_index=None), TypeError),
                    (dict(max_len=16, marks=[[], []]), ValueError), (dict(max_len=16, marks=[[(0, 1)]]), ValueError),
                    (dict(max_len=16, word_labels=[[1]]), ValueError)):
        with pytest.raises(exc):
            t.encode_aligned(["xin chao"], **kw)
    with pytest.raises(TypeError):
        t.encode_aligned([b"xin"], 16)


def test_bio_continuation_map():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    mode, m = tokenize.Tokenize._align_continuation("bio", np.array([0, 1, 2, 5, -100], dtype=np.int32))
    assert mode == 2 and m.dtype == np.int32 and m.tolist() == [0, 2, 2, 4, 4, 6]
    assert tokenize.Tokenize._align_continuation("ignore", None) == (0, None)
    assert tokenize.Tokenize._align_continuation("same", None) == (1, None)
    mode, m = tokenize.Tokenize._align_continuation([7, 8, 9], None)
    assert mode == 2 and m.tolist() == [7, 8, 9]


# ---- the rules of gz_rowrules.h, alone ------------------------------------------------------------------------------------------
MAIN = r"""
#include "gz_rowrules.h"
#include <cstdio>
#include <vector>

static void say(const char* name, const char* why) { std::printf("%s|%s\n", name, why ? why : ""); }

int main()
{
    say("spans_ok", word_spans_fault(3, 0, 0));
    say("spans_bytes", word_spans_fault(0, 1, INT64_MAX));
    say("spans_negative_docs", word_spans_fault(-1, 0, 0));
    say("spans_unit_2", word_spans_fault(1, 2, 0));
    say("spans_unit_negative", word_spans_fault(1, -1, 0));
    say("spans_capacity_negative", word_spans_fault(1, 0, -1));
    say("spans_first_of_two", word_spans_fault(-1, 7, -1));
    //   n_docs, n_rows, have_row_doc, max_len, continuation, have_map, n_map, want_labels, have_word_labels
    say("align_ok", align_rows_fault(3, 3, false, 3, 0, false, 0, false, false));
    say("align_windows", align_rows_fault(3, 9, true, 128, 2, true, 5, true, true));
    say("align_empty", align_rows_fault(0, 0, false, 16, 1, false, 0, true, true));
    say("align_negative_docs", align_rows_fault(-1, 0, true, 16, 0, false, 0, false, false));
    say("align_negative_rows", align_rows_fault(1, -1, true, 16, 0, false, 0, false, false));
    say("align_max_len_2", align_rows_fault(1, 1, false, 2, 0, false, 0, false, false));
    say("align_max_len_negative", align_rows_fault(1, 1, false, -5, 0, false, 0, false, false));
    say("align_rows_without_docs", align_rows_fault(3, 4, false, 16, 0, false, 0, false, false));
    say("align_continuation_3", align_rows_fault(1, 1, false, 16, 3, false, 0, false, false));
    say("align_continuation_negative", align_rows_fault(1, 1, false, 16, -1, false, 0, false, false));
    say("align_n_map_negative", align_rows_fault(1, 1, false, 16, 0, true, -1, false, false));
    say("align_map_missing", align_rows_fault(1, 1, false, 16, 2, false, 4, true, true));
    say("align_map_empty", align_rows_fault(1, 1, false, 16, 2, true, 0, true, true));
    say("align_labels_without_word_labels", align_rows_fault(1, 1, false, 16, 0, false, 0, true, false));
    say("align_too_many_cells", align_rows_fault(1, INT64_MAX / 8, true, 16, 0, false, 0, false, false));
    say("align_most_cells", align_rows_fault(1, INT64_MAX / 4 / 16, true, 16, 0, false, 0, false, false));
    {
        std::vector<int32_t> counts = {1, 2, 5}, bad = {1, 0, 5}, doc = {2, 0, 0, 1}, far = {0, 3}, low = {0, -1}, start = {0, 4, 9, 0}, neg = {0, -4};
        say("data_ok", align_data_fault(counts.data(), 3, doc.data(), start.data(), 4, 3));
        say("data_plain", align_data_fault(counts.data(), 3, nullptr, nullptr, 3, 3));
        say("data_none", align_data_fault(nullptr, 0, nullptr, nullptr, 0, 0));
        say("data_count_0", align_data_fault(bad.data(), 3, doc.data(), start.data(), 4, 3));
        say("data_doc_high", align_data_fault(counts.data(), 3, far.data(), nullptr, 2, 3));
        say("data_doc_negative", align_data_fault(counts.data(), 3, low.data(), nullptr, 2, 3));
        say("data_start_negative", align_data_fault(counts.data(), 3, nullptr, neg.data(), 2, 3));
        say("data_first_of_two", align_data_fault(bad.data(), 3, far.data(), neg.data(), 2, 3));
    }
    say("labels_ok", span_labels_fault(3, 1));
    say("labels_plain", span_labels_fault(0, 0));
    say("labels_negative_docs", span_labels_fault(-1, 0));
    say("labels_scheme_2", span_labels_fault(1, 2));
    {
        std::vector<int32_t> marks = {0, 4, 3, 9, 2, 0, 5, 5, 7}, minus = {0, 4, 3, 9, 2, -1}, huge = {0, 4, (1 << 30) - 1}, most = {0, 4, (1 << 30) - 2};
        say("marks_ok", span_labels_data_fault(marks.data(), 3, 1));
        say("marks_none", span_labels_data_fault(nullptr, 0, 1));
        say("marks_plain_negative", span_labels_data_fault(minus.data(), 2, 0));
        say("marks_bio_negative", span_labels_data_fault(minus.data(), 2, 1));
        say("marks_bio_huge", span_labels_data_fault(huge.data(), 1, 1));
        say("marks_bio_most", span_labels_data_fault(most.data(), 1, 1));
    }
    return 0;
}
"""

EXPECTED = {
    "spans_ok": "", "spans_bytes": "",
    "spans_negative_docs": "word spans need n_docs >= 0", "spans_unit_2": "word spans need unit 0 (code points) or 1 (bytes)",
    "spans_unit_negative": "word spans need unit 0 (code points) or 1 (bytes)", "spans_capacity_negative": "word spans need capacity_words >= 0",
    "spans_first_of_two": "word spans need n_docs >= 0",
    "align_ok": "", "align_windows": "", "align_empty": "",
    "align_negative_docs": "aligned rows need n_docs >= 0 and n_rows >= 0", "align_negative_rows": "aligned rows need n_docs >= 0 and n_rows >= 0",
    "align_max_len_2": "aligned rows need max_len >= 3", "align_max_len_negative": "aligned rows need max_len >= 3",
    "align_rows_without_docs": "aligned rows without row_doc need n_rows == n_docs",
    "align_continuation_3": "aligned rows need continuation 0 (ignore), 1 (same) or 2 (map)",
    "align_continuation_negative": "aligned rows need continuation 0 (ignore), 1 (same) or 2 (map)",
    "align_n_map_negative": "aligned rows need n_map >= 0",
    "align_map_missing": "aligned rows in map mode need a cont_map of at least one entry",
    "align_map_empty": "aligned rows in map mode need a cont_map of at least one entry",
    "align_labels_without_word_labels": "aligned rows need word_labels where labels are asked for",
    "align_too_many_cells": "aligned rows need n_rows * max_len * 4 below 2^63", "align_most_cells": "",
    "data_ok": "", "data_plain": "", "data_none": "",
    "data_count_0": "aligned rows: a word's piece count is below 1", "data_doc_high": "aligned rows: a row_doc lies outside [0, n_docs)",
    "data_doc_negative": "aligned rows: a row_doc lies outside [0, n_docs)", "data_start_negative": "aligned rows: a row_start is negative",
    "data_first_of_two": "aligned rows: a word's piece count is below 1",
    "labels_ok": "", "labels_plain": "", "labels_negative_docs": "span labels need n_docs >= 0",
    "labels_scheme_2": "span labels need scheme 0 (plain) or 1 (BIO)",
    "marks_ok": "", "marks_none": "", "marks_plain_negative": "", "marks_bio_negative": "span labels under BIO need labels >= 0",
    "marks_bio_huge": "span labels under BIO need labels below 2^30 - 1", "marks_bio_most": "",
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("align_rules")
    src, exe = os.path.join(d, "align_rules_main.cpp"), os.path.join(d, "align_rules_main")
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
def test_align_rule(results, name):
    assert results[name] == EXPECTED[name]


def test_every_refusal_has_its_own_sentence():
    said = {v for v in EXPECTED.values() if v}
    assert len(said) == 18
