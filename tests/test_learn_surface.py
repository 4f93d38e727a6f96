"""CPU-only: the BPE learner exists on every layer -- the C entry points are declared with their argument lists, documented in the
header's own section, exported and bound; genz_tokenize exports learn_bpe and word_counts with their defaults; every bad argument is
refused before any native call; the test switch is a typed key; and the host rules of csrc/gz_learn_host.h (initial symbols in byte
order, interning, pieces, their order) equal tests/learn_oracle.py in a stand-alone program under the sanitizers.  Nothing is
computed on a GPU here (tests/test_gpu_learn.py does that)."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import learn_oracle as LO
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
TYPES = {
    "gz_wordset_build": ["gz_ctx *", "const uint8_t *", "const int64_t *", "int64_t", "gz_wordset **"],
    "gz_wordset_build_device": ["gz_ctx *", "const uint8_t *", "const int64_t *", "int64_t", "int64_t", "gz_wordset **"],
    "gz_wordset_from_counts": ["gz_ctx *", "const uint8_t *", "const int64_t *", "const int64_t *", "int64_t", "gz_wordset **"],
    "gz_wordset_info": ["gz_wordset *", "int64_t *", "int64_t *", "int64_t *"],
    "gz_wordset_words": ["gz_wordset *", "int64_t *", "int64_t *", "uint8_t *", "int64_t"],
    "gz_wordset_destroy": ["gz_wordset *"],
    "gz_bpe_learn": ["gz_wordset *", "int64_t", "int64_t", "int64_t"],
    "gz_bpe_learn_result": ["gz_wordset *", "int64_t *", "uint8_t *", "int64_t", "int64_t *", "int64_t *", "uint8_t *", "int64_t"],
}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    C = native.C
    vp, i64 = C.c_void_p, C.c_int64
    ctype = {"int64_t": i64}
    for n, types in TYPES.items():
        decl = re.search(r"\b(int|void)\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        args = [a.strip() for a in decl.group(2).split(",")]
        assert [re.sub(r"\w+(\[\d+\])?$", "", a).strip() for a in args] == types, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        bound = getattr(lib, n).argtypes
        assert len(bound) == len(types), n
        for t, b, a in zip(types, bound, args):
            if t in ctype and not a.endswith("]"):
                assert b is ctype[t], (n, a)
            elif t.endswith("**"):
                assert b is C.POINTER(vp), (n, a)
            else:
                assert b is vp or b is C.POINTER(i64), (n, a)
        assert getattr(lib, n).restype is (None if n == "gz_wordset_destroy" else C.c_int), n
    assert lib.gz_version() == 0x010100                             # functions were added, nothing else moved
    for m in ("wordset_build", "wordset_build_device", "wordset_from_counts", "wordset_info", "wordset_words", "wordset_destroy", "bpe_learn"):
        assert callable(getattr(native.Context, m)), m
    assert re.search(r"#define\s+GZ_BPE_MERGES_MAX\s+\(1 << 20\)", src)


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("---- learn: BPE merges and a vocabulary from a corpus"):]
    comment = block[:block.index("typedef struct gz_wordset gz_wordset;")]
    for word in ("str.split()", "29 whitespace code points", "first-occurrence order", "</w>", "sorted by bytes ascending", "REUSES",
                 "overlaps", "included", "largest n", "smallest (id_l, id_r)", "min_frequency", "left to right and non-overlapping",
                 "aaaaa -> aa aa a", "@@", "final four bytes", "largest count first", "<pad> <s> </s> <mask> <unk>", "#version: 0.2",
                 "CLOSURE", "gz_wordset_build_device", "gz_wordset_from_counts", "add up", "GZ_E_INVALID", "GZ_E_LIMIT", "GZ_E_CAPACITY",
                 "2^31 - 1 symbol positions", "2^62", "GZ_BPE_MERGES_MAX", "info[8]", "order of the atomics", "never a dropped",
                 "readback per merge", "Not here", "destroyed before it"):
        assert word in comment, word
    assert src.index("gz_minhash_groups_device(") < src.index("---- learn: BPE merges") < src.index("---- text pre-pass")
    assert "GZ_E_NOTABLES" not in comment
    assert re.search(r"learn_table_bits \(0\.\.30; 0\)", src)


def test_test_switch_is_a_typed_key():
    native = pytest.importorskip("genz_tokenize._native")
    lib = native.load_library()
    for v in (0, 1, 30):
        assert lib.gz_debug_set(None, b"learn_table_bits", v) == native.GZ_OK, v
    for v in (-1, 31, 1 << 40):
        assert lib.gz_debug_set(None, b"learn_table_bits", v) == native.GZ_E_INVALID, v
    assert lib.gz_debug_set(None, b"learn_table_bits", 0) == native.GZ_OK


def test_python_signatures():
    pkg = pytest.importorskip("genz_tokenize")
    learn = pytest.importorskip("genz_tokenize.learn")
    assert pkg.learn_bpe is learn.learn_bpe and pkg.word_counts is learn.word_counts
    assert "learn_bpe" in pkg.__all__ and "word_counts" in pkg.__all__
    empty = inspect.Parameter.empty
    want = {
        "learn_bpe": [("documents", None), ("n_merges", 32000), ("min_frequency", 2), ("words", None), ("counts", None), ("ctx", None)],
        "learn_bpe_packed": [("text_u8", empty), ("offsets", empty), ("n_merges", 32000), ("min_frequency", 2), ("ctx", None)],
        "word_counts": [("documents", empty), ("ctx", None)],
        "word_counts_packed": [("text_u8", empty), ("offsets", empty), ("ctx", None)],
    }
    for name, params in want.items():
        p = inspect.signature(getattr(learn, name)).parameters
        assert list(p) == [k for k, _ in params], name
        for k, d in params:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
        assert len(getattr(learn, name).__doc__) > 60, name
    assert inspect.signature(learn.learn_bpe).parameters["words"].kind is inspect.Parameter.KEYWORD_ONLY
    for attr in ("save", "tokenizer"):
        assert callable(getattr(learn.LearnedBPE, attr))
    assert learn.MERGES_MAX == 1 << 20


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def test_refusals_before_any_native_call():
    learn = pytest.importorskip("genz_tokenize.learn")
    ctx = _NoNative()
    docs = ["a b"]
    for kw, exc in [(dict(n_merges=-1), ValueError), (dict(n_merges=(1 << 20) + 1), ValueError), (dict(n_merges=True), TypeError),
                    (dict(n_merges=10.0), TypeError), (dict(n_merges=None), TypeError), (dict(n_merges="10"), TypeError),
                    (dict(min_frequency=0), ValueError), (dict(min_frequency=-3), ValueError), (dict(min_frequency=1 << 62), ValueError),
                    (dict(min_frequency=True), TypeError), (dict(min_frequency=2.0), TypeError), (dict(min_frequency=None), TypeError)]:
        with pytest.raises(exc):
            learn.learn_bpe(docs, ctx=ctx, **kw)
        with pytest.raises(exc):
            learn.learn_bpe(words=["a"], counts=[1], ctx=ctx, **kw)
        with pytest.raises(exc):
            learn.learn_bpe_packed(np.zeros(3, np.uint8), np.array([0, 3]), ctx=ctx, **kw)
    for bad in (["a", 3], ["a", None], [b"a"], "a b", b"a b"):
        with pytest.raises(TypeError):
            learn.learn_bpe(bad, ctx=ctx)
        with pytest.raises(TypeError):
            learn.word_counts(bad, ctx=ctx)
    with pytest.raises(TypeError):
        learn.learn_bpe(ctx=ctx)                                          # neither documents nor words
    with pytest.raises(TypeError):
        learn.learn_bpe(docs, words=["a"], counts=[1], ctx=ctx)           # both
    with pytest.raises(TypeError):
        learn.learn_bpe(docs, counts=[1], ctx=ctx)
    with pytest.raises(TypeError):
        learn.learn_bpe(words=["a"], ctx=ctx)                             # words without counts
    for words, counts, exc in ((["a", "b"], [1], ValueError), (["a b"], [1], ValueError), ([""], [1], ValueError), (["a\n"], [1], ValueError),
                               (["a　b"], [1], ValueError), (["a"], [0], ValueError), (["a"], [-1], ValueError), (["a"], [1.0], TypeError),
                               (["a"], [True], TypeError), (["a"], [1 << 62], ValueError), (["a", "b"], [1 << 61, 1 << 61], ValueError),
                               ([3], [1], TypeError), ("ab", [1, 1], TypeError)):
        with pytest.raises(exc):
            learn.learn_bpe(words=words, counts=counts, ctx=ctx)
    for text, off, exc in ((np.zeros(3, np.int8), np.array([0, 3]), TypeError), (np.zeros(3, np.uint8), np.array([0, 3], np.int32), TypeError),
                           (np.zeros(3, np.uint8), np.array([0, 4]), ValueError), (np.zeros(3, np.uint8), np.array([2, 1]), ValueError),
                           (np.zeros(3, np.uint8), np.array([-1, 1]), ValueError), (np.zeros((3, 1), np.uint8), np.array([0, 3]), TypeError),
                           (np.zeros(3, np.uint8), np.zeros(0, np.int64), TypeError)):
        with pytest.raises(exc):
            learn.word_counts_packed(text, off, ctx=ctx)
        with pytest.raises(exc):
            learn.learn_bpe_packed(text, off, ctx=ctx)
    with pytest.raises(AssertionError, match="native call wordset_build"):
        learn.learn_bpe(docs, ctx=ctx)                                    # ... and good arguments do reach the library


# ---- the host rules of gz_learn_host.h, alone ---------------------------------------------------------------------------------------
MAIN = r"""
#include "gz_learn_host.h"
#include <cstdio>
#include <cstdlib>
#include <map>

static void hex(const char* name, const std::string& s)
{
    std::printf("%s|", name);
    for (unsigned char ch : s) std::printf("%02x", ch);
    std::printf("\n");
}

// the rule with a full recount every step, on the ids and strings LearnHost keeps: what the device does with its pair table
int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> bytes;
    std::vector<int64_t> off{0}, cnt;
    long long c;
    char word[4096];
    while (std::fscanf(f, "%lld %4095s", &c, word) == 2) {
        for (const char* p = word; p[0] && p[1]; p += 2) {
            const char h[3] = {p[0], p[1], 0};
            bytes.push_back((uint8_t)std::strtol(h, nullptr, 16));
        }
        off.push_back((int64_t)bytes.size());
        cnt.push_back(c);
    }
    std::fclose(f);
    const long long n_merges = std::atoll(argv[2]), min_frequency = std::atoll(argv[3]);
    const char* why = learn_args_fault(n_merges, min_frequency);
    std::printf("args|%s\n", why ? why : "");
    if (why) return 0;
    LearnHost H;
    why = H.init(bytes.data(), off.data(), cnt.data(), (int64_t)cnt.size(), 64);
    std::printf("init|%s\n", why ? why : "");
    if (why) return 0;
    std::vector<std::vector<int32_t>> seg;
    for (size_t d = 0; d < cnt.size(); ++d) seg.emplace_back(H.flat.begin() + H.woff[d], H.flat.begin() + H.woff[d + 1]);
    std::printf("long|%zu\n", H.longw.size());
    for (long long step = 0; step < n_merges; ++step) {
        std::map<std::pair<int32_t, int32_t>, int64_t> n;
        for (size_t d = 0; d < seg.size(); ++d)
            for (size_t i = 0; i + 1 < seg[d].size(); ++i) n[{seg[d][i], seg[d][i + 1]}] += cnt[d];
        int64_t best = 0;
        std::pair<int32_t, int32_t> key{0, 0};
        for (const auto& kv : n)
            if (kv.second > best) { best = kv.second; key = kv.first; }           // (the map is in (id_l, id_r) order: the first of equals)
        if (best < 1 || best < min_frequency) break;
        const int32_t m = H.merge(key.first, key.second);
        for (auto& s : seg) {
            std::vector<int32_t> o;
            for (size_t i = 0; i < s.size();) {
                if (i + 1 < s.size() && s[i] == key.first && s[i + 1] == key.second) { o.push_back(m); i += 2; }
                else { o.push_back(s[i]); i += 1; }
            }
            s.swap(o);
        }
    }
    std::vector<int64_t> hist(2 * H.sym.size(), 0);
    for (size_t d = 0; d < seg.size(); ++d)
        for (size_t i = 0; i < seg[d].size(); ++i) hist[2 * (size_t)seg[d][i] + (i + 1 == seg[d].size() ? 1 : 0)] += cnt[d];
    std::vector<std::pair<std::string, int64_t>> pieces;
    H.pieces(hist.data(), pieces);
    std::string codes = "#version: 0.2\n", vocab;
    for (const auto& m : H.merges) codes += H.sym[(size_t)m.first] + " " + H.sym[(size_t)m.second] + "\n";
    for (const auto& p : pieces) vocab += p.first + " " + std::to_string(p.second) + "\n";
    hex("codes", codes);
    hex("vocab", vocab);
    std::printf("symbols|%zu\n", H.sym.size());
    return 0;
}
"""

CASES = {
    "known": ({"aaaa": 1, "aaaaa": 2, "ab": 3, "abab": 1, "b": 5}, 10, 2),
    "interning": ({'/a<w/w//>/w': 1, '</>w</w>w/>>>aa': 2, 'a//<w>/<w': 3}, 30, 1),
    "wide": ({"aệ😀aệ": 3, "ệ😀": 2, "\x7f\x80߿ࠀ￿\U00010000\U0010ffff": 2, "é": 9, "aệ": 1}, 50, 1),
    "specials": ({"<s>": 9, "<pad>": 8, "</s>": 7, "<mask>": 6, "<unk>": 5, "<s>x": 4, "ab": 3, "a@@": 2}, 200, 1),
    "big_counts": ({"abab": 3 * 10 ** 9, "abb": 3 * 10 ** 9, "b": 2 ** 40}, 10, 2 ** 31),
    "long_word": ({"ab" * 40: 2, "a" * 65: 1, "b" * 64: 1}, 12, 1),
    "nothing": ({}, 5, 1),
}
REFUSED = {
    "merges_negative": ({"a": 1}, -1, 1, "args", "BPE learner needs n_merges >= 0"),
    "merges_above_cap": ({"a": 1}, (1 << 20) + 1, 1, "args", "BPE learner takes at most 2^20 merges"),
    "frequency_zero": ({"a": 1}, 1, 0, "args", "BPE learner needs min_frequency >= 1"),
    "count_zero": ({"a": 0}, 1, 1, "init", "BPE learner: a word count below 1"),
    "total_2_62": ({"a": 1 << 61, "b": 1 << 61}, 1, 1, "init", "BPE learner: the counts sum to 2^62 or more"),
    "weighted_2_62": ({"abcd": 1 << 60}, 1, 1, "init", "BPE learner: counts times symbols sum to 2^62 or more"),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("learn_rules")
    src, exe = os.path.join(d, "learn_rules_main.cpp"), os.path.join(d, "learn_rules_main")
    with open(src, "w") as f:
        f.write(MAIN)
    c = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    if c.returncode != 0 and ("asan" in c.stderr or "ubsan" in c.stderr) and "cannot find" in c.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert c.returncode == 0, c.stderr

    def run(words, n_merges, min_frequency, raw=None):
        path = os.path.join(d, "corpus.txt")
        with open(path, "w") as f:
            for w, c in (raw if raw is not None else [(k.encode("utf-8"), v) for k, v in words.items()]):
                f.write("%d %s\n" % (c, w.hex()))
        r = subprocess.run([exe, path, str(n_merges), str(min_frequency)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)         # (a sanitizer report is a failure)
        return dict(line.split("|", 1) for line in r.stdout.splitlines())
    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_rules_equal_the_oracle(program, name):
    words, n, f = CASES[name]
    out = program(words, n, f)
    want = LO.learn(list(words), list(words.values()), n, f)
    assert (out["args"], out["init"]) == ("", "")
    assert bytes.fromhex(out["codes"]) == want.codes
    assert bytes.fromhex(out["vocab"]) == want.vocab
    assert int(out["symbols"]) == want.n_symbols
    assert int(out["long"]) == sum(1 for w in words if len(w) > 64)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_host_rules_refuse(program, name):
    words, n, f, where, sentence = REFUSED[name]
    out = program(words, n, f)
    assert out[where] == sentence and "codes" not in out


def test_every_refusal_has_its_own_sentence():
    assert len({v[4] for v in REFUSED.values()}) == len(REFUSED)


def test_a_byte_that_starts_no_sequence_is_a_symbol_of_its_own(program):
    # a stray continuation byte, a lead byte without its tail, a lead byte that is never valid, a byte above F4
    out = program(None, 0, 1, raw=[(b"\x80a\xe1\x80\xc0\xf5", 1)])
    assert out["init"] == "" and int(out["symbols"]) == 5
    assert bytes.fromhex(out["vocab"]).split(b"\n")[:-1] == [b"\x80@@ 2", b"a@@ 1", b"\xc0@@ 1", b"\xe1@@ 1", b"\xf5 1"]
