"""CPU-only: the oracle of the text quality signals against a hand-worked table, the Python-side refusals of genz_tokenize.quality
(before any native call) and gopher_filter's arithmetic on made-up counts."""
import numpy as np
import pytest

import quality_oracle as Q

# document -> the 14 signals in Q.NAMES' order, worked out by hand
TABLE = [
    ("", [0] * 14),
    ("a", [1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]),
    (" \n ", [3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("a b\na b\n\nc", [10, 5, 5, 5, 0, 0, 3, 0, 0, 1, 3, 2, 0, 0]),
    ("- x...\n* y…\n• z .......", [23, 7, 17, 3, 0, 4, 3, 3, 3, 0, 0, 1, 0, 0]),
    ("p\n\np\n \np", [8, 3, 3, 3, 0, 0, 3, 0, 0, 2, 2, 3, 2, 2]),
    ("# 12 #x\r\n# 12 #x", [16, 6, 10, 2, 4, 0, 2, 0, 0, 1, 7, 1, 0, 0]),
    ("é×　ñ", [4, 2, 3, 2, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]),
    ("a  b\na b", [8, 4, 4, 4, 0, 0, 2, 0, 0, 0, 0, 1, 0, 0]),
    (" a b \n\ta b\n\na b", [15, 6, 6, 6, 0, 0, 3, 0, 0, 2, 6, 2, 0, 0]),
    ("\U0001F600 1 ..", [6, 3, 4, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]),
]


@pytest.mark.parametrize("text,want", TABLE)
def test_oracle_against_the_hand_worked_table(text, want):
    got = Q.signals([text.encode()])
    assert [int(got[k][0]) for k in Q.NAMES] == want


def test_oracle_spans_and_firsts():
    got = Q.signals([b" a b \n\ta b\n\na b", b"", b"x\n\nx"])
    assert got["line_off"].tolist() == [0, 3, 3, 5] and got["para_off"].tolist() == [0, 2, 2, 4]
    assert got["line_span"].tolist() == [[1, 4], [7, 10], [12, 15], [0, 1], [3, 4]] and got["line_first"].tolist() == [0, 0, 0, 0, 0]
    assert got["para_span"].tolist() == [[1, 10], [12, 15], [0, 1], [3, 4]] and got["para_first"].tolist() == [0, 1, 0, 0]


class NoNative:
    """a context no refusal may reach"""
    def __getattr__(self, name):
        raise AssertionError("native call: " + name)


@pytest.mark.parametrize("call,error", [
    (lambda q: q.text_signals_packed(np.zeros(4, np.int8), np.array([0, 4]), ctx=NoNative()), TypeError),
    (lambda q: q.text_signals_packed(np.zeros(4, np.uint8), np.array([0.0, 4.0]), ctx=NoNative()), TypeError),
    (lambda q: q.text_signals_packed(np.zeros(4, np.uint8), np.array([0, 3, 2]), ctx=NoNative()), ValueError),
    (lambda q: q.text_signals_packed(np.zeros(4, np.uint8), np.array([0, 5]), ctx=NoNative()), ValueError),
    (lambda q: q.text_signals(["a", b"b"], ctx=NoNative()), TypeError),
    (lambda q: q.text_signals_to_device(["a", None], ctx=NoNative()), TypeError),
    (lambda q: q.gopher_filter(["a"], ctx=NoNative(), max_words_per_line=3), TypeError),
])
def test_python_refusals_come_before_any_native_call(call, error):
    quality = pytest.importorskip("genz_tokenize.quality")
    with pytest.raises(error):
        call(quality)


def test_gopher_arithmetic_on_made_up_counts():
    quality = pytest.importorskip("genz_tokenize.quality")
    assert quality.SIGNALS == Q.NAMES
    rows = {  # good, nothing at all, too few words, '#' heavy, duplicate lines, duplicate characters, long words
        "n_chars": [600, 0, 200, 600, 600, 600, 2000], "n_words": [100, 0, 49, 100, 100, 100, 100], "word_chars": [500, 0, 150, 500, 500, 500, 1001],
        "n_alpha_words": [80, 0, 49, 100, 100, 100, 100], "n_hash": [10, 0, 0, 11, 0, 0, 0], "n_ellipsis": [10, 0, 0, 0, 0, 0, 0],
        "n_lines": [10, 0, 5, 10, 10, 10, 10], "n_bullet_lines": [9, 0, 0, 0, 0, 0, 0], "n_ellipsis_lines": [3, 0, 0, 0, 0, 0, 0],
        "dup_lines": [3, 0, 0, 0, 4, 1, 0], "dup_line_chars": [120, 0, 0, 0, 100, 121, 0], "n_paragraphs": [10, 0, 1, 1, 1, 1, 1],
        "dup_paragraphs": [3, 0, 0, 0, 0, 0, 0], "dup_paragraph_chars": [120, 0, 0, 0, 0, 0, 0]}
    out = quality.gopher_shares({k: np.array(v, np.int32) for k, v in rows.items()})
    assert out["keep"].tolist() == [True, False, False, False, False, False, False]
    assert out["mean_word_length"].tolist() == [5.0, 0.0, 150 / 49, 5.0, 5.0, 5.0, 10.01]
    assert out["hash_ratio"].tolist()[:4] == [0.1, 0.0, 0.0, 0.11] and out["bullet_lines"][0] == 0.9 and out["alpha_words"][0] == 0.8
    assert out["dup_line_fraction"].tolist() == [0.3, 0.0, 0.0, 0.0, 0.4, 0.1, 0.0] and out["dup_line_char_fraction"][0] == 0.2
    for k in ("dup_paragraph_fraction", "dup_paragraph_char_fraction", "ellipsis_lines", "ellipsis_ratio"):
        assert out[k][1] == 0.0                                          # a zero denominator gives 0
    assert quality.gopher_shares({k: np.array(v, np.int32) for k, v in rows.items()}, min_words=10, max_hash_ratio=0.2)["keep"].tolist()[:4] == [True, False, True, True]


RULES_MAIN = r"""
#include "gz_rowrules.h"
#include <cstdio>
#include <vector>
static void say(const char* name, const char* why) { std::printf("%s|%s\n", name, why ? why : ""); }
int main()
{
    std::vector<unsigned char> text(64), outs(4096);
    std::vector<int64_t> off(3, 0);
    unsigned char* const o = outs.data();
    const QualityOut all{(int32_t*)o, (uint32_t*)(o + 256), (int64_t*)(o + 512), (int32_t*)(o + 1024), (uint32_t*)(o + 1280), (int64_t*)(o + 1536), (int32_t*)(o + 2048)};
    QualityOut q = all;
    say("ok", quality_fault(2, text.data(), off.data(), all));
    say("negative", quality_fault(-1, text.data(), off.data(), all));
    say("no_text", quality_fault(2, nullptr, off.data(), all));
    say("no_off", quality_fault(2, text.data(), nullptr, all));
    q.line_off = nullptr; say("line_span_alone", quality_fault(2, text.data(), off.data(), q));
    q = all; q.para_off = nullptr; q.para_span = nullptr; say("para_first_alone", quality_fault(2, text.data(), off.data(), q));
    q.para_first = nullptr; say("para_left_out", quality_fault(2, text.data(), off.data(), q));
    std::printf("apart|%d\n", quality_disjoint(text.data(), 64, off.data(), 2, 14, 8, 4, all) ? 1 : 0);
    std::printf("touching|%d\n", quality_disjoint(text.data(), 64, off.data(), 2, 14, 32, 32, all) ? 1 : 0);      // line_span ends where line_first begins
    std::printf("span_into_first|%d\n", quality_disjoint(text.data(), 64, off.data(), 2, 14, 33, 4, all) ? 1 : 0);
    q = all; q.signals = (int32_t*)(text.data() + 60);
    std::printf("signals_in_text|%d\n", quality_disjoint(text.data(), 64, off.data(), 2, 14, 8, 4, q) ? 1 : 0);
    q = all; q.para_off = (uint32_t*)off.data();
    std::printf("off_reused|%d\n", quality_disjoint(text.data(), 64, off.data(), 2, 14, 8, 4, q) ? 1 : 0);
    std::printf("fit_most|%d\n", quality_spans_fit(0xFFFFFFFEull, 0) ? 1 : 0);
    std::printf("fit_limit|%d\n", quality_spans_fit(0xFFFFFFF0ull, 15) ? 1 : 0);
    return 0;
}
"""
RULES_EXPECTED = {
    "ok": "", "negative": "text signals need n_docs >= 0", "no_text": "text signals need text and offsets", "no_off": "text signals need text and offsets",
    "line_span_alone": "text signals write line_span and line_first only beside line_off",
    "para_first_alone": "text signals write para_span and para_first only beside para_off", "para_left_out": "",
    "apart": "1", "touching": "1", "span_into_first": "0", "signals_in_text": "0", "off_reused": "0", "fit_most": "1", "fit_limit": "0",
}


def test_argument_rules_alone_under_the_sanitizers(tmp_path):
    """gz_rowrules.h's quality rules as a stand-alone program under ASan + UBSan, the way the other calls' rules are checked"""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = str(tmp_path / "quality_rules_main.cpp"), str(tmp_path / "quality_rules_main")
    with open(src, "w") as f:
        f.write(RULES_MAIN)
    c = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "genz-tokenize_amd", "csrc"), src, "-o", exe], capture_output=True, text=True)
    if c.returncode != 0 and ("asan" in c.stderr or "ubsan" in c.stderr) and "cannot find" in c.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert c.returncode == 0, c.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    assert dict(line.split("|") for line in r.stdout.splitlines()) == RULES_EXPECTED
