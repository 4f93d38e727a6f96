"""CPU-only: the BPE-dropout oracle (tests/dropout_oracle.py) is pinned -- by known answers worked out on the CPU with the bundled
tables, by the plain oracle at threshold 0, by the code points at threshold 2**32 and by the share of dropped draws -- and the Python
calls refuse every bad argument before anything native runs.  tests/test_gpu_dropout.py compares the device with this oracle."""
import json
import os

import numpy as np
import pytest

import dropout_oracle as DO
import gz_oracle as O
from conftest import DATA, GOLDEN
from mask_oracle import philox4x32_10

TEXT = "sinh_viên công_nghệ thông_tin aaaaaaa hello\nworld"
IDS = {
    0.0: [1, 770, 1444, 800, 41347, 33281, 15117, 3019, 4, 13676, 2],
    0.1: [1, 770, 1444, 17517, 5758, 229, 41347, 33281, 15117, 3019, 4, 13676, 2],
    0.5: [1, 9163, 434, 6907, 1272, 1866, 1701, 1562, 1580, 8312, 2468, 3940, 5758, 2615, 1454, 1696, 22736, 22736, 29843, 1580, 1864, 1883,
          1883, 1742, 4, 13676, 2],
}
PIECES_05 = ["sinh_@@ viên", "cô@@ n@@ g@@ _@@ ng@@ h@@ ệ", "th@@ ô@@ ng_@@ ti@@ n", "a@@ aa@@ aa@@ aa", "h@@ e@@ l@@ l@@ o@@ \n", "world"]


@pytest.fixture(scope="module")
def known():
    with open(os.path.join(GOLDEN, "dropout_known.json"), encoding="ascii") as f:
        return json.load(f)


def test_known_answers(oracle_tables, known):
    t = oracle_tables
    assert known["text"] == TEXT and (known["seed"], known["doc"]) == (7, 3)
    key = DO.word_key(7, 3, 0)
    assert key == (0x63E41616, 0x40086B6F) == tuple(known["word_key"])
    assert DO.u(key, 2, 5) == 0x98A4A03C == known["u_t2_i5"]
    # the plain-int rounds are the numpy ones of the mask oracle
    x = philox4x32_10((3, 0, 0, 0), (7, 0))
    assert (int(x[0]), int(x[1])) == key
    assert DO.draws(key, 4, 1000) == [DO.u(key, 4, i) for i in range(1000)]          # (the numpy form of long words)
    for p, want in IDS.items():
        assert DO.encode(TEXT, t, DO.threshold(p), 7, 3) == want, p
    assert [" ".join(x) for x in DO.encode_pieces(TEXT, t, DO.threshold(0.5), 7, 3)] == PIECES_05
    assert " ".join(DO.encode_pieces(TEXT, t, DO.threshold(0.1), 7, 3)[2]) == "thô@@ ng_@@ tin"
    ones = DO.encode(TEXT, t, DO.threshold(1.0), 7, 3)
    assert len(ones) == 47
    for case in known["cases"]:
        assert DO.encode(TEXT, t, DO.threshold(case["p"]), 7, 3) == case["ids"], case["p"]
        assert [" ".join(x) for x in DO.encode_pieces(TEXT, t, DO.threshold(case["p"]), 7, 3)] == case["pieces"], case["p"]
    assert DO.threshold(0.0) == 0 and DO.threshold(1.0) == 2 ** 32 and DO.threshold(0.1) == int(0.1 * 2 ** 32)
    assert IDS[0.0] == O.encode(TEXT, t)


def test_threshold_zero_is_the_plain_oracle(oracle_tables):
    t = oracle_tables
    words = [w[:-2] if w.endswith("@@") else w for w in list(t.encoder)[:4000]]
    words = [w for w in words if w and O.split_words(w) == [w]]
    assert len(words) > 3500
    bad = [w for j, w in enumerate(words) if DO.pieces_dropout(w, t.ranks, 0, DO.word_key(5, j, j % 7)) != O.bpe_pieces(w, t.ranks)]
    assert bad == []


def test_threshold_one_gives_code_points(oracle_tables):
    t = oracle_tables
    for j, w in enumerate(["a", "hello", "sinh_viên", "hello\n", "aaaaaaa", "x" * 300, "\U0001F600中ô"]):
        got = DO.pieces_dropout(w, t.ranks, 2 ** 32, DO.word_key(1, 2, j))
        assert got == [c + "@@" for c in w[:-1]] + [w[-1]], w
    rows = DO.rows(t, [TEXT, "", "  "], 2 ** 32, seed=9)
    assert rows[1] == rows[2] == [t.bos_id, t.eos_id]
    assert len(rows[0]) == 2 + sum(len(w) for w in O.split_words(TEXT))


def test_drop_share():
    key, thr = DO.word_key(7, 3, 0), int(0.1 * 2 ** 32)
    share = sum(DO.u(key, 0, i) < thr for i in range(20000)) / 20000
    print("dropped share at p = 0.1 over 20000 draws: %.5f" % share)
    assert abs(share - 0.1) <= 0.0085                                 # four binomial standard deviations


def test_a_dropped_occurrence_stays_and_loops_are_bounded(oracle_tables):
    t = oracle_tables
    for n in (2, 3, 7, 64, 65, 130):
        for seed in range(3):
            got = DO.pieces_dropout("a" * n, t.ranks, DO.threshold(0.5), DO.word_key(seed, 0, n))
            assert "".join(p[:-2] if p.endswith("@@") else p for p in got[:-1]) + got[-1] == "a" * n


# ---- the Python calls refuse bad arguments before anything runs ------------------------------------------------------------------
class _NoNative:
    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = _NoNative()
    t._dirty = True
    return t


BAD = [
    (dict(p=-0.1), ValueError), (dict(p=1.0001), ValueError), (dict(p=float("nan")), ValueError), (dict(p=True), TypeError),
    (dict(p="0.1"), TypeError), (dict(p=None), TypeError), (dict(p=float("inf")), ValueError),
    (dict(seed=-1), ValueError), (dict(seed=2 ** 64), ValueError), (dict(seed=1.0), TypeError), (dict(seed=True), TypeError), (dict(seed=None), TypeError),
    (dict(doc_base=-1), ValueError), (dict(doc_base=2 ** 63), ValueError), (dict(doc_base=True), TypeError), (dict(doc_base=0.0), TypeError),
    (dict(doc_base=2 ** 63 - 1), ValueError),                         # doc_base + the batch's documents passes 2**63
]


def test_refusals_before_any_native_call():
    t = _bare()
    for kw, exc in BAD:
        with pytest.raises(exc):
            t.encode_dropout(["a b", "c"], **kw)
        with pytest.raises(exc):
            t.encode_dropout_packed(np.frombuffer(b"a bc", dtype=np.uint8), np.array([0, 3, 4], dtype=np.int64), **kw)
        kw2 = dict(dict(p=0.1, seed=0, max_len=8), **kw)
        with pytest.raises(exc):
            t.encode_dropout_to_device(["a b", "c"], **kw2)
    for ml in (None, 0, -3):
        with pytest.raises(ValueError):
            t.encode_dropout_to_device(["a"], 0.1, 0, ml)
    for kw, exc in [(dict(p=-1), ValueError), (dict(p=2), ValueError), (dict(p=False), TypeError), (dict(p=0.1, seed=-1), ValueError),
                    (dict(p=0.1, seed=2 ** 64), ValueError), (dict(p=0.1, doc=-1), ValueError), (dict(p=0.1, doc=2 ** 63), ValueError),
                    (dict(p=0.1, doc=1.5), TypeError), (dict(p=0.1, word=-1), ValueError), (dict(p=0.1, word=2 ** 32), ValueError),
                    (dict(p=0.1, word=True), TypeError)]:
        with pytest.raises(exc):
            t.bpe_dropout("hello", **kw)
    with pytest.raises(TypeError):
        t.bpe_dropout(b"hello", 0.1)
    with pytest.raises(IndexError):
        t.bpe_dropout("", 0.1)


def test_signatures():
    import inspect
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    T = tokenize.Tokenize
    p = inspect.signature(T.encode_dropout).parameters
    assert list(p) == ["self", "texts", "p", "seed", "max_len", "padding", "truncation", "doc_base"]
    assert (p["p"].default, p["seed"].default, p["max_len"].default, p["padding"].default, p["truncation"].default, p["doc_base"].default) == \
        (0.1, 0, None, True, True, 0)
    p = inspect.signature(T.encode_dropout_packed).parameters
    assert list(p) == ["self", "text_u8", "offsets", "p", "seed", "max_len", "padding", "truncation", "doc_base"]
    p = inspect.signature(T.encode_dropout_to_device).parameters
    assert list(p) == ["self", "texts", "p", "seed", "max_len", "doc_base"] and p["doc_base"].default == 0
    p = inspect.signature(T.bpe_dropout).parameters
    assert list(p) == ["self", "token", "p", "seed", "doc", "word"] and (p["seed"].default, p["doc"].default, p["word"].default) == (0, 0, 0)
    # the neighbours are what they were
    assert list(inspect.signature(T.encode_batch).parameters) == ["self", "texts", "pair_texts", "max_len", "padding", "truncation", "word_table",
                                                                  "return_offset"]
    assert list(inspect.signature(T.bpe).parameters) == ["self", "token"]
