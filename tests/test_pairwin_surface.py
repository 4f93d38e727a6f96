"""CPU-only: the pair window calls exist on every layer -- the four C entry points are declared with their argument lists, documented
in the header's own section (the rule verbatim), exported and bound; _native.Context routes to them; Tokenize has pair_window_rows,
span_tokens, encode_pair_windows, encode_pair_windows_to_device and pair_window_spans with their defaults; the kernels are their own
file; and pairwin_fault of csrc/gz_rowrules.h holds in a stand-alone program under ASan + UBSan.  Nothing is computed on a GPU here
(tests/test_gpu_pairwin.py does that)."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
I32, CI32, CI64 = "int32_t *", "const int32_t *", "const int64_t *"
PAIR = ["gz_ctx *", CI32, CI64, "int64_t", CI32, CI64, "int64_t", CI32, CI32, "int32_t", "int32_t", "int32_t", "int32_t", "int32_t"] + [I32] * 10 + \
       ["int64_t *", "int64_t", "int64_t *"]
NAMES = {"gz_pair_window_rows": PAIR, "gz_pair_window_rows_device": PAIR,
         "gz_span_tokens": ["gz_ctx *", CI32, CI64, "int64_t", CI32, CI64, I32],
         "gz_span_tokens_device": ["gz_ctx *", CI32, CI64, "int64_t", "int64_t", CI32, CI64, "int64_t", I32]}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_window_rows": 16, "gz_window_rows_device": 16, "gz_span_labels": 10, "gz_span_labels_device": 12, "gz_align_rows": 16, "gz_word_spans": 9,
       "gz_pack_rows": 18, "gz_ngram_repeats": 15, "gz_debug_set": 3}


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
    assert lib.gz_pair_window_rows.argtypes == [vp, vp, vp, i64, vp, vp, i64, vp, vp, i32, i32, i32, i32, i32] + [vp] * 11 + [i64, C.POINTER(i64)]
    assert lib.gz_pair_window_rows_device.argtypes == lib.gz_pair_window_rows.argtypes
    assert lib.gz_span_tokens.argtypes == [vp, vp, vp, i64, vp, vp, vp]
    assert lib.gz_span_tokens_device.argtypes == [vp, vp, vp, i64, i64, vp, vp, i64, vp]
    for m in ("pair_window_rows", "pair_window_rows_device", "span_tokens", "span_tokens_device"):
        assert callable(getattr(native.Context, m)), m
    assert native.Context.PAIRWIN_CELLS == ("input_ids", "attention_mask", "token_type_ids")
    assert native.Context.PAIRWIN_META == ("pair", "start", "n_real", "q_len")
    assert native.Context.PAIRWIN_ANSWER == ("start_positions", "end_positions", "has_answer")


RULE = """q      = min(Tq, mq)                    (the question keeps its FIRST q tokens)
room   = L - 4 - q   (>= s + 1)         step = room - s  (>= 1)
n_win  = 1 if T <= room else 1 + ceil((T - room) / step)
window j: start = j * step, chunk = body[start : min(start + room, T)], n = len(chunk)
row    = [bos] + Q[:q] + [eos, eos] + chunk + [eos] + [pad] * (room - n)      n_real = q + 4 + n
mask   = (row != pad)                                    (tokenize.py:148-152, as everywhere)
type   = 0 on columns < q + 2, 1 on columns q + 2 .. n_real - 1, the pad id behind them
ctx_col = q + 3                                          (column of chunk[0])"""


def test_header_states_the_rule_verbatim():
    src = open(HEADER).read()
    block = src[src.index("---- pair windows: question-context windows with answer positions"):]
    comment = block[:block.index("int  gz_pair_window_rows(")]
    lines = [re.sub(r"^ \*\s*", "", l).rstrip() for l in comment.splitlines()]
    for want in RULE.splitlines():
        assert want in lines, want
    flat = " ".join(" ".join(lines).split())
    for word in ("The call is valid iff L >= 5, 0 <= mq <= L - 5 and 0 <= s <= L - 5 - mq", "returns GZ_E_INVALID and writes nothing",
                 "An answer is present iff 0 <= a0 < a1 <= T", "no input is invalid on the device",
                 "Window j holds the answer iff start <= a0 and a1 <= start + n",
                 "start_pos = ctx_col + a0 - start, end_pos = ctx_col + a1 - 1 - start and has_answer = 1",
                 "start_pos = end_pos = 0 (the bos column, the SQuAD convention) and has_answer = 0", "all three outputs may be NULL",
                 "The last window is shorter, not shifted back", "NULL means pair r uses question r, and then NQ == N",
                 "ONE skip_front / skip_back pair", "Equality with the reference", "the ONE deviation", "Chunks rejoin", "Question placement",
                 "a1 - a0 <= s + 1", "longer than room is held by none", "row[start_pos : end_pos + 1] == body[a0:a1]",
                 "ABSOLUTE offsets", "input_ids == NULL sizes only", "GZ_E_CAPACITY: win_off is valid and nothing is written to the other outputs",
                 "may be NULL", "n_rows == 0 is GZ_OK and launches nothing", "context's stream", "EMPTY question", "no address is formed from it",
                 "The host form refuses such an entry", "GZ_E_NOTABLES", "gz_span_tokens / gz_span_tokens_device", "(-1, -1) range stays (-1, -1)",
                 "launches nothing", "Not here", "several answers per pair", "longest first", "16-bit outputs", "shards concatenate"):
        assert word in flat, word
    # a section of its own, behind the align section and before the repeats
    assert src.index("gz_span_labels_device(") < src.index("---- pair windows: question-context windows") < src.index("---- repeats: n-gram repetition")
    assert src.index("int  gz_span_tokens_device(") < src.index("---- repeats: n-gram repetition")


def test_kernels_are_their_own_file():
    hip = open(os.path.join(CSRC, "gz_kernels.hip")).read()
    assert hip.index('#include "gz_window.inc"') < hip.index('#include "gz_pairwin.inc"') < hip.index('#include "gz_packrows.inc"')
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "gz_pairwin.inc" in make                                            # the build identity covers it
    inc = open(os.path.join(CSRC, "gz_pairwin.inc")).read()
    for word in ("gz_pairwin_count_kernel", "gz_pairwin_fill_kernel", "gz_spantok_kernel", "__shfl", "nt_store4", "template <int U>", "int64_t cell",
                 "GzPairWinArgs", "GzSpanTokArgs", "q      = min(Tq, mq)", "ctx_col = q + 3"):
        assert word in inc, word
    assert "__shared__" not in inc and "hipMemset" not in inc                  # no LDS; every cell written once, nothing cleared
    kh = open(os.path.join(CSRC, "gz_kernels.h")).read()
    assert "struct GzPairWinArgs" in kh and "struct GzSpanTokArgs" in kh
    api = open(os.path.join(CSRC, "gz_rows_api.inc")).read()
    tail = api[api.index("int gz_pair_window_rows("):]
    for word in ("pairwin_fault(", "pairwin_data_fault(", "rows_check(", "rows_stage(", "StagedOut S;", "staged_copy_out(c, S)", "read_total("):
        assert word in tail or word in api[api.index("pairwin_device_locked"):], word
    rules = open(os.path.join(CSRC, "gz_rowrules.h")).read()
    assert "inline const char* pairwin_fault(" in rules and rules.index("span_labels_data_fault") < rules.index("pairwin_fault(")


def test_tokenize_signatures():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    T = tokenize.Tokenize
    empty = inspect.Parameter.empty
    want = {
        "pair_window_rows": [("question_rows", empty), ("context_rows", empty), ("max_len", empty), ("stride", 0), ("max_query_len", None),
                             ("q_row", None), ("answers", None), ("framed", True)],
        "span_tokens": [("word_tokens", empty), ("word_off", empty), ("mark_words", empty), ("mark_off", empty)],
        "encode_pair_windows": [("questions", empty), ("contexts", empty), ("max_len", empty), ("stride", 0), ("max_query_len", None), ("q_row", None),
                                ("answers", None), ("unit", "char"), ("word_table", True)],
        "encode_pair_windows_to_device": [("questions", empty), ("contexts", empty), ("max_len", empty), ("stride", 0), ("max_query_len", None),
                                          ("q_row", None), ("answers", None), ("unit", "char"), ("word_table", True)],
    }
    for name, params in want.items():
        p = inspect.signature(getattr(T, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in params], name
        for k, d in params:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
        doc = getattr(T, name).__doc__
        assert doc and len(doc) > 100, name
    assert isinstance(inspect.getattr_static(T, "pair_window_spans"), staticmethod)
    assert list(inspect.signature(T.pair_window_spans).parameters) == ["result", "start_cols", "end_cols"]
    assert isinstance(inspect.getattr_static(T, "_pair_window_rule"), staticmethod)
    assert list(inspect.signature(T._pair_window_rule).parameters) == ["max_len", "stride", "max_query_len"]
    assert "DeviceArray" in T.encode_pair_windows_to_device.__doc__ and "(-1, -1)" in T.pair_window_spans.__doc__
    # the neighbours are what they were
    assert list(inspect.signature(T.encode_windows).parameters) == ["self", "texts", "max_len", "stride", "word_table"]
    assert list(inspect.signature(T.window_rows).parameters) == ["self", "rows", "max_len", "stride", "framed"]
    assert list(inspect.signature(T.span_labels).parameters) == ["self", "span", "word_off", "marks", "scheme", "outside"]
    assert list(inspect.signature(T._window_rule).parameters) == ["max_len", "stride"]


# ---- the rule of gz_rowrules.h, alone ---------------------------------------------------------------------------------------
MAIN = r"""
#include "gz_rowrules.h"
#include <cstdio>
#include <vector>

static void call(const char* name, int64_t rows, int64_t nq, bool q_row, int32_t L, int32_t s, int32_t mq, int32_t sf = 1, int32_t sb = 1, int64_t cap = 0)
{
    const char* why = pairwin_fault(rows, nq, q_row, L, s, mq, sf, sb, cap);
    std::printf("%s|%s\n", name, why ? why : "");
}
static void data(const char* name, std::vector<int32_t> q_row, int64_t nq, bool null_row = false)
{
    // (the vector is sized exactly: a read beyond n_rows entries is a sanitizer report)
    const char* why = pairwin_data_fault(null_row ? nullptr : q_row.data(), (int64_t)q_row.size(), nq);
    std::printf("%s|%s\n", name, why ? why : "");
}
static void tokens(const char* name, std::vector<int32_t> counts, std::vector<int32_t> mw)
{
    const char* why = span_tokens_data_fault(counts.data(), (int64_t)counts.size(), mw.data(), (int64_t)mw.size() / 2);
    std::printf("%s|%s\n", name, why ? why : "");
}

int main()
{
    call("ok_smallest", 0, 0, false, 5, 0, 0, 0, 0);
    call("ok_usual", 7, 7, false, 384, 128, 64);
    call("ok_shared_question", 100, 1, true, 128, 32, 16, 0, 1, INT64_MAX);
    call("ok_no_questions", 3, 0, true, 8, 3, 0);
    call("ok_mq_most", 1, 1, false, 16, 0, 11);
    call("ok_stride_most", 1, 1, false, 16, 11, 0);
    call("ok_both_most", 1, 1, false, 16, 4, 7);
    call("ok_int_max", INT64_MAX, INT64_MAX, false, INT32_MAX, INT32_MAX - 5, 0);
    call("negative_rows", -1, 0, true, 16, 0, 0);
    call("negative_questions", 1, -1, true, 16, 0, 0);
    call("negative_capacity", 1, 1, false, 16, 0, 0, 1, 1, -1);
    call("skip_front_2", 1, 1, false, 16, 0, 0, 2, 0);
    call("skip_back_negative", 1, 1, false, 16, 0, 0, 0, -1);
    call("max_len_4", 1, 1, false, 4, 0, 0);
    call("max_len_negative", 1, 1, false, INT32_MIN, 0, 0);
    call("mq_negative", 1, 1, false, 16, 0, -1);
    call("mq_12", 1, 1, false, 16, 0, 12);
    call("mq_int_max", 1, 1, false, 16, 0, INT32_MAX);
    call("stride_negative", 1, 1, false, 16, -1, 4);
    call("stride_8_mq_4", 1, 1, false, 16, 8, 4);
    call("stride_int_max", 1, 1, false, 16, INT32_MAX, 0);
    call("stride_1_at_5", 1, 1, false, 5, 1, 0);
    call("count_mismatch", 3, 2, false, 16, 0, 4);
    call("first_of_many", -1, 5, false, 3, -2, 99, 7, 7, -1);
    call("rule_order", 1, 2, false, 16, 12, 12);
    data("data_ok", {0, 2, 1, 2}, 3);
    data("data_null", {}, 0, true);
    data("data_empty", {}, 0);
    data("data_negative", {0, -1}, 3);
    data("data_at_nq", {0, 3}, 3);
    data("data_no_questions", {0}, 0);
    std::printf("tokens_docs|%s\n", span_tokens_fault(-1) ? span_tokens_fault(-1) : "");
    std::printf("tokens_docs_ok|%s\n", span_tokens_fault(0) ? "x" : "");
    tokens("tokens_ok", {1, 3, 2}, {0, 3, -1, -1, 2, 2, 1, 2});
    tokens("tokens_zero_count", {1, 0}, {0, 1});
    tokens("tokens_half_none", {1, 1}, {-1, 1});
    tokens("tokens_reversed", {1, 1}, {2, 1});
    tokens("tokens_beyond", {1, 1}, {0, 3});
    return 0;
}
"""

EXPECTED = {
    "ok_smallest": "", "ok_usual": "", "ok_shared_question": "", "ok_no_questions": "", "ok_mq_most": "", "ok_stride_most": "", "ok_both_most": "",
    "ok_int_max": "",
    "negative_rows": "pair windows need n_rows >= 0 and n_questions >= 0", "negative_questions": "pair windows need n_rows >= 0 and n_questions >= 0",
    "negative_capacity": "pair windows need capacity_windows >= 0",
    "skip_front_2": "pair windows need skips of 0 or 1", "skip_back_negative": "pair windows need skips of 0 or 1",
    "max_len_4": "pair windows need max_len >= 5", "max_len_negative": "pair windows need max_len >= 5",
    "mq_negative": "pair windows need max_query_len in [0, max_len - 5]", "mq_12": "pair windows need max_query_len in [0, max_len - 5]",
    "mq_int_max": "pair windows need max_query_len in [0, max_len - 5]",
    "stride_negative": "pair windows need a stride in [0, max_len - 5 - max_query_len]",
    "stride_8_mq_4": "pair windows need a stride in [0, max_len - 5 - max_query_len]",
    "stride_int_max": "pair windows need a stride in [0, max_len - 5 - max_query_len]",
    "stride_1_at_5": "pair windows need a stride in [0, max_len - 5 - max_query_len]",
    "count_mismatch": "pair windows without q_row need n_questions == n_rows",
    "first_of_many": "pair windows need n_rows >= 0 and n_questions >= 0", "rule_order": "pair windows need max_query_len in [0, max_len - 5]",
    "data_ok": "", "data_null": "", "data_empty": "",
    "data_negative": "pair windows: a q_row lies outside [0, n_questions)", "data_at_nq": "pair windows: a q_row lies outside [0, n_questions)",
    "data_no_questions": "pair windows: a q_row lies outside [0, n_questions)",
    "tokens_docs": "span tokens need n_docs >= 0", "tokens_docs_ok": "",
    "tokens_ok": "", "tokens_zero_count": "span tokens: a word's piece count is below 1",
    "tokens_half_none": "span tokens: a word range is neither (-1, -1) nor 0 <= first <= last + 1 <= words",
    "tokens_reversed": "span tokens: a word range is neither (-1, -1) nor 0 <= first <= last + 1 <= words",
    "tokens_beyond": "span tokens: a word range is neither (-1, -1) nor 0 <= first <= last + 1 <= words",
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pairwin_rules")
    src, exe = os.path.join(d, "pairwin_rules_main.cpp"), os.path.join(d, "pairwin_rules_main")
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
def test_pairwin_rule(results, name):
    assert results[name] == EXPECTED[name]


def test_every_refusal_has_its_own_sentence():
    said = {v for k, v in EXPECTED.items() if v and not k.startswith(("data_", "tokens_"))}
    assert len(said) == 7


def test_the_python_rule_and_the_c_rule_agree(results):
    """Every (L, s, mq) the stand-alone program refused or took, Tokenize._pair_window_rule refuses or takes."""
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    for name, (L, s, mq) in {"ok_usual": (384, 128, 64), "ok_mq_most": (16, 0, 11), "ok_stride_most": (16, 11, 0), "ok_both_most": (16, 4, 7),
                             "max_len_4": (4, 0, 0), "mq_negative": (16, 0, -1), "mq_12": (16, 0, 12), "stride_negative": (16, -1, 4),
                             "stride_8_mq_4": (16, 8, 4), "stride_1_at_5": (5, 1, 0)}.items():
        if results[name] == "":
            assert tokenize.Tokenize._pair_window_rule(L, s, mq) == (L, s, mq)
        else:
            with pytest.raises(ValueError):
                tokenize.Tokenize._pair_window_rule(L, s, mq)
