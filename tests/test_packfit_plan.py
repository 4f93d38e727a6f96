"""csrc/gz_packfit.h alone, on the CPU: the host plan of best-fit packing (the sequential decisions, collapsed onto the length
histogram) against the sequential rule of tests/packfit_oracle.py, document by document.  A small main that includes the header is
built with the host compiler under ASan + UBSan and run as a stand-alone program; it reads batches of lengths, and prints the
events, the final segments and R of each.  Python expands the events into (doc_row, doc_col) the way the place kernel does and
compares.  No GPU, no Python extension."""
import os
import random
import shutil
import subprocess

import pytest

import packfit_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")

MAIN = r"""
#include "gz_packfit.h"
#include <cstdio>
#include <vector>

// stdin: per batch "L n len_0 .. len_{n-1}".  stdout: "B L n", then "E l start row k col0 before n_rows" per event (by length,
// through ev_off), "S row docs base" per final segment, "R rows".
int main()
{
    long long L, n;
    while (std::scanf("%lld %lld", &L, &n) == 2) {
        std::vector<int32_t> h((size_t)L + 1, 0);                       // (sized exactly: a read beyond h[L] is a sanitizer report)
        for (long long i = 0; i < n; ++i) {
            long long l;
            if (std::scanf("%lld", &l) != 1 || l < 2 || l > L) return 2;
            h[(size_t)l] += 1;
        }
        GzFitPlan P;
        gz_packfit_plan(h.data(), (int32_t)L, P);
        std::printf("B %lld %lld\n", L, n);
        if (P.ev_off.size() != (size_t)L + 2 || P.ev_off[(size_t)L + 1] != 0 || P.ev_off[2] != (int32_t)P.ev.size()) return 3;
        for (long long l = L; l >= 2; --l)
            for (int32_t e = P.ev_off[(size_t)l + 1]; e < P.ev_off[(size_t)l]; ++e) {
                const GzFitEvent& v = P.ev[(size_t)e];
                std::printf("E %lld %d %d %d %d %d %d\n", l, v.start, v.row, v.k, v.col0, v.before, v.n_rows);
            }
        for (const GzFitSeg& g : P.seg) std::printf("S %d %d %lld\n", g.row, g.docs, (long long)g.base);
        std::printf("R %lld\n", (long long)P.R);
    }
    return 0;
}
"""


def geometric(rng, L, n):
    out = []
    for _ in range(n):
        l = 2
        while l < L and rng.random() < 0.8:
            l += 1
        out.append(l)
    return out


def cases():
    rng = random.Random(20211)
    out = {}
    for k in range(300):
        L = rng.randint(3, 40)
        out["random_%03d" % k] = (L, [rng.randint(2, L) for _ in range(rng.randint(0, 200))])
    for k in range(20):
        L = rng.randint(3, 40)
        out["geometric_%02d" % k] = (L, geometric(rng, L, rng.randint(1, 200)))
    for L, l in ((10, 3), (10, 5), (12, 4), (7, 7), (9, 4), (40, 13), (128, 43)):
        out["equal_L%d_l%d" % (L, l)] = (L, [l] * 37)
    for L in (3, 4, 5, 8, 9, 33):
        out["all_2_L%d" % L] = (L, [2] * 41)
        out["all_L_L%d" % L] = (L, [L] * 9)
        out["one_L%d" % L] = (L, [min(L, 5)])
        out["none_L%d" % L] = (L, [])
    out["every_length_4096"] = (4096, list(range(2, 4097)))
    out["by_hand"] = (10, [5, 5, 5, 2, 2, 8, 3])
    out["twos_and_rest"] = (12, [2] * 6 + [10] * 6)
    return out


CASES = cases()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("packfit_plan")
    src, exe = os.path.join(d, "packfit_plan_main.cpp"), os.path.join(d, "packfit_plan_main")
    with open(src, "w") as f:
        f.write(MAIN)
    c = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    if c.returncode != 0 and ("asan" in c.stderr or "ubsan" in c.stderr) and "cannot find" in c.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert c.returncode == 0, c.stderr
    names = sorted(CASES)
    text = "".join("%d %d %s\n" % (CASES[k][0], len(CASES[k][1]), " ".join(map(str, CASES[k][1]))) for k in names)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)          # (a sanitizer report is a failure)
    out, cur = [], None
    for line in r.stdout.splitlines():
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "B":
            cur = dict(L=v[0], n=v[1], events={}, segs=[], R=None)
            out.append(cur)
        elif tag == "E":
            cur["events"].setdefault(v[0], []).append(tuple(v[1:]))
        elif tag == "S":
            cur["segs"].append(tuple(v))
        else:
            cur["R"] = v[0]
    assert len(out) == len(names)
    return dict(zip(names, out))


def expand(plan, lens, L):
    """What the place pass does: rank within the length by index, the event by its first rank, row and slot by division."""
    rank, seen = [], {}
    for l in lens:
        rank.append(seen.get(l, 0))
        seen[l] = rank[-1] + 1
    doc_row, doc_col, doc_pos = [], [], []
    for l, j in zip(lens, rank):
        ev = plan["events"][l]
        e = max(k for k in range(len(ev)) if ev[k][0] <= j)
        start, row, k, col0, before, n_rows = ev[e]
        q = j - start
        assert q < n_rows * k                                         # the rank lies inside the event
        doc_row.append(row + q // k)
        doc_col.append(col0 + (q % k) * l)
        doc_pos.append(before + q % k)
    return doc_row, doc_col, doc_pos


def check(plan, lens, L):
    want_row, want_col, want_R = (FO.place if len(lens) <= 400 else FO.place_fast)(lens, L)
    assert (plan["L"], plan["n"], plan["R"]) == (L, len(lens), want_R)
    got_row, got_col, got_pos = expand(plan, lens, L)
    assert got_row == want_row and got_col == want_col
    # events: ranks start at 0 and follow each other without a gap, every event places a document
    for l, ev in plan["events"].items():
        at = 0
        for start, row, k, col0, before, n_rows in ev:
            assert start == at and k >= 1 and n_rows >= 1 and col0 + k * l <= L
            at += k * n_rows
        assert at == lens.count(l)
    assert sum(len(ev) for ev in plan["events"].values()) <= max(len(lens), 0)
    # final segments: sorted by row, they partition [0, R); row_off from them is the packed order's
    segs = plan["segs"]
    assert segs[-1] == (want_R, 0, len(lens)) and [s[0] for s in segs] == sorted({s[0] for s in segs}) and (want_R == 0 or segs[0][0] == 0)
    row_off = []
    for (row, docs, base), nxt in zip(segs[:-1], segs[1:]):
        assert docs >= 1 and nxt[2] == base + (nxt[0] - row) * docs
        row_off += [base + (i - row) * docs for i in range(row, nxt[0])]
    row_off.append(len(lens))
    order = sorted(range(len(lens)), key=lambda d: (want_row[d], want_col[d]))
    for d in range(len(lens)):
        assert order[row_off[got_row[d]] + got_pos[d]] == d
    return want_R


@pytest.mark.parametrize("name", sorted(k for k in CASES if not k.startswith("random_")))
def test_plan_equals_the_sequential_rule(plans, name):
    L, lens = CASES[name]
    check(plans[name], lens, L)


def test_plan_equals_the_sequential_rule_on_random_batches(plans):
    names = [k for k in CASES if k.startswith("random_")]
    assert len(names) == 300
    for name in names:
        L, lens = CASES[name]
        check(plans[name], lens, L)


def test_the_fast_oracle_is_the_oracle():
    rng = random.Random(5)
    for _ in range(60):
        L = rng.randint(3, 40)
        lens = [rng.randint(2, L) for _ in range(rng.randint(0, 150))]
        assert FO.place_fast(lens, L) == FO.place(lens, L)


def test_answer_written_out_by_hand(plans):
    """L = 10, lengths [5, 5, 5, 2, 2, 8, 3].  Order: 8 (doc 5), 5 5 5 (docs 0 1 2), 3 (doc 6), 2 2 (docs 3 4).
    8 opens row 0 (free 2).  5, 5 fill row 1 (free 0); the third 5 opens row 2 (free 5).  3: rows with free >= 3: row 2 only ->
    col 5 (free 2).  2: smallest (free, stamp) with free >= 2: rows 0 and 2 both have 2 free, row 0 was touched earlier -> row 0
    col 8; the next 2 -> row 2 col 8."""
    doc_row, doc_col, R = FO.place([5, 5, 5, 2, 2, 8, 3], 10)
    assert (doc_row, doc_col, R) == ([1, 1, 2, 0, 2, 0, 2], [0, 5, 0, 8, 8, 0, 5], 3)
    got_row, got_col, got_pos = expand(plans["by_hand"], [5, 5, 5, 2, 2, 8, 3], 10)
    assert (got_row, got_col, plans["by_hand"]["R"]) == (doc_row, doc_col, 3)
    assert got_pos == [0, 1, 0, 1, 2, 0, 1]


def test_twos_and_rest_fill_rows_exactly(plans):
    """[2] * k + [L - 2] * k: best-fit puts one of each into a row, k full rows; next-fit lays the 2s together first."""
    import pack_oracle as PO
    L, lens = CASES["twos_and_rest"]
    assert plans["twos_and_rest"]["R"] == 6 and FO.place(lens, L)[2] == 6
    assert PO.place(lens, L)[2] == 7
    got_row, got_col, _ = expand(plans["twos_and_rest"], lens, L)
    assert got_row == [0, 1, 2, 3, 4, 5] * 2 and got_col == [10] * 6 + [0] * 6

