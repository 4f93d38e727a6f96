"""CPU-only: the n-gram language model calls are declared, documented, exported and bound on every layer; the Python refusals come
before any native call; tests/lm_oracle.py agrees with the cases its docstring works by hand; and the new rules of
csrc/gz_rowrules.h hold in a stand-alone program under ASan + UBSan.  Nothing is computed on a GPU here (tests/test_gpu_lm.py)."""
import os
import re
import shutil
import subprocess

import pytest

import lm_oracle as LO
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
NAMES = {"gz_ngram_lm_build": 8, "gz_ngram_lm_build_device": 8, "gz_ngram_lm_info": 2, "gz_ngram_lm_score": 14, "gz_ngram_lm_score_device": 14}


def test_symbols_declared_documented_exported_and_bound():
    from genz_tokenize import _native as native
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = "".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    lib = native.load_library()
    for n, argc in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == argc == len(getattr(lib, n).argtypes) and getattr(lib, n).restype is native.C.c_int, n
        assert n in comments and n in native.SYMBOLS and callable(getattr(native.Context, n[3:])), n
    assert re.search(r"\bvoid\s+gz_ngram_lm_destroy\s*\(\s*gz_ngram_lm\s*\*\s*\w+\s*\)\s*;", src) and lib.gz_ngram_lm_destroy.restype is None
    assert lib.gz_ngram_lm_score.argtypes[7] is native.C.c_double


def test_python_refusals_come_before_any_native_call():
    import genz_tokenize
    from genz_tokenize import tokenize
    assert genz_tokenize.NgramLM is tokenize.NgramLM and "NgramLM" in genz_tokenize.__all__
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    closed, live = tokenize.NgramLM.__new__(tokenize.NgramLM), tokenize.NgramLM.__new__(tokenize.NgramLM)
    closed._handle, closed._ctx, live._handle, live._ctx, t._ctx = None, None, 1, None, None      # no context: a native call would raise AttributeError
    calls = [lambda: t.perplexity_rows([[1]], "lm"), lambda: t.perplexity_rows([[1]], closed), lambda: t.perplexity_filter(["a"], closed, 10.0)]
    for order in (0, 9, 2.0, True):
        calls += [lambda o=order: t.ngram_lm([[1, 2]], o), lambda o=order: t.encode_ngram_lm(["a"], o)]
    calls += [lambda a=alpha: t.perplexity_rows([[1]], live, a) for alpha in (0.0, 1.5, float("nan"), 2.0 ** -9, "0.4")]
    for call in calls:
        with pytest.raises((TypeError, ValueError)):
            call()
    with pytest.raises(TypeError):
        t.perplexity_filter(["a"], live)                                   # max_perplexity has no default


def test_oracle_agrees_with_the_cases_worked_by_hand():
    model = LO.train([[1, 2, 1, 2, 3], [2]], 2)
    assert LO.grams(model, 2) == ((6, 6, 4), (1, 3, 3))
    a = LO.score(model, 2, [[1, 2]], 0.5)
    assert a["bits_fx"].tolist() == [26591258] and a["n_order"][:, 0].tolist() == [0, 1, 1]
    assert (a["token_order"].tolist(), a["token_num"].tolist(), a["token_den"].tolist()) == ([1, 2], [2, 2], [6, 2])
    b = LO.score(model, 2, [[3, 1]], 0.25)
    assert b["bits_fx"].tolist() == [43368474 + 60145690] and b["n_order"][:, 0].tolist() == [0, 2, 0] and b["token_den"].tolist() == [6, 6]
    c = LO.score(model, 2, [[9], []], 1.0)
    assert c["bits_fx"].tolist() == [43368474, 0] and c["n_order"].T.tolist() == [[1, 0, 0], [0, 0, 0]] and c["n_tokens"].tolist() == [1, 0]
    f = LO.score(LO.train([[0, 1, 2, 1, 2, 3, 0], [0, 2, 0]], 2, framed=True), 2, [[7, 1, 2, 7], [7]], 0.5, framed=True)
    assert f["bits_fx"].tolist() == [26591258, 0] and f["token_num"].tolist() == [0, 2, 2, 0, 0] and f["row_off"].tolist() == [0, 4, 5]


# ---- the rules of gz_rowrules.h, alone: a program with its own main that checks them itself ------------------------------------
MAIN = r"""
#include "gz_rowrules.h"
#include <cmath>
#include <cstdio>
#include <cstring>
static int bad = 0;
#define OK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++bad; } } while (0)
static bool is(const char* why, const char* want) { return want ? why && !std::strcmp(why, want) : !why; }
int main()
{
    const char *order = "n-gram model needs an order in 1..8", *alpha = "perplexity needs alpha in [2^-8, 1]";
    OK(is(lm_build_fault(5, 1, 1, 5), 0)); OK(is(lm_build_fault(0, 0, 1, 8), 0)); OK(is(lm_build_fault(INT64_MAX, 1, 0, 1), 0));
    OK(is(lm_build_fault(-1, 0, 0, 0), "n-gram model needs n_rows >= 0")); OK(is(lm_build_fault(1, 2, 0, 5), "n-gram model needs skips of 0 or 1"));
    OK(is(lm_build_fault(1, 0, 0, 0), order)); OK(is(lm_build_fault(1, 0, 0, 9), order));
    OK(is(lm_score_fault(5, 1, 1, 0.4), 0)); OK(is(lm_score_fault(0, 0, 0, 1.0), 0)); OK(is(lm_score_fault(INT64_MAX, 1, 1, 1.0 / 256.0), 0));
    OK(is(lm_score_fault(-1, 0, 0, 0.0), "perplexity needs n_rows >= 0")); OK(is(lm_score_fault(1, 0, -1, 0.4), "perplexity needs skips of 0 or 1"));
    OK(is(lm_score_fault(1, 0, 0, 0.0), alpha)); OK(is(lm_score_fault(1, 0, 0, std::nan("")), alpha));
    OK(is(lm_score_fault(1, 0, 0, std::nextafter(1.0 / 256.0, 0.0)), alpha)); OK(is(lm_score_fault(1, 0, 0, std::nextafter(1.0, 2.0)), alpha));
    OK(lm_grams(0, 1) == 0); OK(lm_grams(4, 5) == 0); OK(lm_grams(5, 5) == 1); OK(lm_grams(INT32_MAX, 8) == 2147483640);
    OK(lm_grams_possible(10, 10, 3, 1)); OK(!lm_grams_possible(9, 10, 3, 1)); OK(lm_grams_possible(4, 10, 3, 3)); OK(!lm_grams_possible(3, 10, 3, 3));
    OK(lm_grams_possible(0, 10, INT64_MAX, 8));
    OK(lm_slots(0) == 1); OK(lm_slots(1) == 2); OK(lm_slots(512) == 1024); OK(lm_slots(513) == 2048); OK(lm_slots((int64_t)8 << 32) == (uint64_t)1 << 36);
    return bad != 0;
}
"""


def test_lm_rules_alone_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = str(tmp_path / "lm_rules_main.cpp"), str(tmp_path / "lm_rules_main")
    with open(src, "w") as f:
        f.write(MAIN)
    c = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    if c.returncode != 0 and ("asan" in c.stderr or "ubsan" in c.stderr) and "cannot find" in c.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert c.returncode == 0, c.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert (r.returncode, r.stdout, r.stderr) == (0, "", "")              # (a failed rule prints its line; a sanitizer report is a failure)
