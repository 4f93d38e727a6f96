"""CPU-only: the oracle the GPU tests compare with (tests/repeat_oracle.py) gives the answers worked by hand in the rule's own table;
every bad argument of the repetition calls of Tokenize is refused before any native call -- the widths, the bounds of
repetition_filter, texts that are not str, rows that are not integers; and the arithmetic of repetition_filter holds on made-up
counts."""
import threading

import numpy as np
import pytest

import repeat_oracle as RO


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = _NoNative()
    t._dirty = True                                                   # (so that any table use would reach the context)
    t._batch_lock = threading.Lock()
    return t


# ---- the oracle, on the cases worked by hand: n_grams, n_distinct, n_repeated, n_covered, top_count, top_pos ------------------
HAND = [
    ([1, 2, 1, 2, 1], 1, (5, 2, 5, 5, 3, 0)),
    ([1, 2, 1, 2, 1], 2, (4, 2, 4, 5, 2, 0)),                          # tie between (1, 2) and (2, 1): the smaller first position
    ([1, 2, 1, 2, 1], 3, (3, 2, 2, 5, 2, 0)),
    ([7, 8, 9], 2, (2, 2, 0, 0, 1, 0)),
    ([7, 8, 9], 4, (0, 0, 0, 0, 0, -1)),
    ([5, 5, 5], 2, (2, 1, 2, 3, 2, 0)),
    ([4, 9, 9, 4, 9, 9], 1, (6, 2, 6, 6, 4, 1)),                       # 9 occurs four times and its first position is 1
]


@pytest.mark.parametrize("body,n,want", HAND)
def test_oracle_known_answers(body, n, want):
    vals, cov = RO.one(body, n)
    assert vals == want
    assert sum(cov) == want[3] and len(cov) == len(body)
    got = RO.repetition([body], [n])
    assert tuple(int(got[k][0, 0]) for k in RO.KEYS) == want
    assert all(got[k].dtype == np.int32 and got[k].shape == (1, 1) for k in RO.KEYS)


def test_oracle_layout_frames_and_bits():
    rows = [[0, 1, 2, 1, 2, 1, 0], [7], [], [0, 0], [0, 5, 5, 5, 0]]
    got = RO.repetition(rows, [3, 1, 2], framed=True)
    assert got["body_len"].tolist() == [5, 0, 0, 0, 3] and got["body_len"].dtype == np.int32
    assert got["row_off"].tolist() == [0, 7, 8, 8, 10, 15] and got["covered"].dtype == np.uint16
    assert got["n_grams"].tolist() == [[3, 0, 0, 0, 1], [5, 0, 0, 0, 3], [4, 0, 0, 0, 2]]
    assert got["top_pos"].tolist() == [[0, -1, -1, -1, 0], [0, -1, -1, -1, 0], [0, -1, -1, -1, 0]]
    assert got["top_count"].tolist() == [[2, 0, 0, 0, 1], [3, 0, 0, 0, 3], [2, 0, 0, 0, 2]]
    # bit k belongs to widths[k]: row 0 is covered whole at every width; (5, 5, 5) occurs once at width 3
    assert got["covered"].tolist() == [0, 7, 7, 7, 7, 7, 0] + [0] + [0, 0] + [0, 6, 6, 6, 0]
    bare = RO.repetition([r[1:-1] for r in rows], [3, 1, 2])
    for k in RO.KEYS + ("body_len",):
        assert np.array_equal(bare[k], got[k]), k
    # a row's outputs are its own: slices against the whole
    part = RO.repetition(rows[1:4], [3, 1, 2], framed=True)
    for k in RO.KEYS:
        assert np.array_equal(part[k], got[k][:, 1:4]), k
    # repeats n apart abut, n + 1 apart leave a gap of one token
    assert RO.one([1, 2, 3, 1, 2, 3], 3)[0][3] == 6 and RO.one([1, 2, 3, 0, 1, 2, 3], 3)[0][3] == 6
    # the same n-gram once in each of two rows counts nowhere
    two = RO.repetition([[1, 2, 3], [1, 2, 3]], [2])
    assert two["n_repeated"].tolist() == [[0, 0]] and two["top_count"].tolist() == [[1, 1]]


# ---- refusals before any native call ----------------------------------------------------------------------------------------
BAD_WIDTHS = [((), ValueError), ([], ValueError), (tuple(range(1, 18)), ValueError), ((0,), ValueError), ((33,), ValueError), ((2, -3), ValueError),
              ((2, 3, 2), ValueError), ((2 ** 40,), ValueError), ((True,), TypeError), ((2, False), TypeError), ((2.0,), TypeError),
              ((np.float32(3),), TypeError), ((None,), TypeError), (("2",), TypeError), ("23", TypeError), (b"\x02", TypeError), (5, TypeError),
              (None, TypeError), (([2],), TypeError)]


def test_the_widths_are_refused_before_any_native_call():
    t = _bare()
    for w, exc in BAD_WIDTHS:
        with pytest.raises(exc):
            t._repeat_rule(w)
        with pytest.raises(exc):
            t.repetition_rows([[1, 2, 3]], w)
        with pytest.raises(exc):
            t.repetition_rows([[1, 2, 3]], widths=w, framed=False, return_covered=True)
        with pytest.raises(exc):
            t.encode_repetition(["a b"], w)
    assert t._repeat_rule() == (2, 3, 4, 5, 6, 7, 8, 9, 10)
    assert t._repeat_rule([32, 1, 7]) == (32, 1, 7)                       # the caller's order
    assert t._repeat_rule(range(1, 17)) == tuple(range(1, 17))
    got = t._repeat_rule(np.array([5, 3], dtype=np.int16))
    assert got == (5, 3) and all(type(v) is int for v in got)
    with pytest.raises(AssertionError, match="native call ngram_repeats"):
        t.repetition_rows([[1, 2, 3]], (32, 1))                           # good widths reach the context


def test_rows_and_texts_are_refused_before_any_native_call():
    t = _bare()
    for rows, exc in (([["a"]], (TypeError, ValueError)), ([[1.5, 2.0]], TypeError), ([[2 ** 31]], ValueError), ([[-2 ** 31 - 1]], ValueError),
                      (np.zeros((2, 3)), TypeError)):
        with pytest.raises(exc):
            t.repetition_rows(rows)
    for texts in (["a", 3], ["a", None], [b"a"]):
        with pytest.raises(TypeError):
            t.encode_repetition(texts)
        with pytest.raises(TypeError):
            t.repetition_filter(texts)


BAD_BOUNDS = [({}, {}, ValueError), ([2], None, TypeError), (None, "5", TypeError), ({0: 0.1}, None, ValueError), (None, {33: 0.1}, ValueError),
              ({2.0: 0.1}, None, TypeError), ({True: 0.1}, None, TypeError), ({2: 1.5}, None, ValueError), ({2: -0.1}, None, ValueError),
              (None, {5: float("nan")}, ValueError), (None, {5: "0.1"}, TypeError), ({2: True}, None, TypeError),
              ({n: 0.1 for n in range(1, 10)}, {n: 0.1 for n in range(10, 18)}, ValueError)]          # 17 widths in the union


def test_the_bounds_are_refused_before_any_native_call():
    t = _bare()
    for top, dup, exc in BAD_BOUNDS:
        with pytest.raises(exc):
            t.repetition_filter(["a b"], top, dup)
        with pytest.raises(exc):
            t.repetition_filter(["a b"], top_max=top, dup_max=dup)
    t._dirty = False                                                      # (no table build: the next thing a good call touches is the encode)
    for top, dup in ((None, None), ({}, {5: 0.1}), ({2: 0}, {}), ({2: np.float32(0.5)}, {np.int64(2): 1})):
        with pytest.raises(AssertionError, match="native call"):
            t.repetition_filter(["a b"], top, dup)


# ---- the arithmetic of repetition_filter, on made-up counts ------------------------------------------------------------------
def test_filter_arithmetic():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    T = tokenize.Tokenize
    assert T.REPEAT_TOP_MAX == {2: 0.20, 3: 0.18, 4: 0.16}
    assert T.REPEAT_DUP_MAX == {5: 0.15, 6: 0.14, 7: 0.13, 8: 0.12, 9: 0.11, 10: 0.10}
    widths = (2, 5, 3)
    #                 doc:  0    1    2    3    4 (empty body)
    body = np.array([100, 100, 100, 10, 0], dtype=np.int32)
    top_count = np.array([[10, 11, 1, 1, 0], [0, 0, 0, 0, 0], [6, 1, 7, 1, 0]], dtype=np.int32)
    n_covered = np.array([[0, 0, 0, 0, 0], [15, 16, 0, 10, 0], [0, 0, 0, 0, 0]], dtype=np.int32)
    out = dict(widths=widths, body_len=body, top_count=top_count, n_covered=n_covered)
    got = T._repeat_decide(out, {2: 0.20, 3: 0.18}, {5: 0.15})
    assert got is out
    assert sorted(got["top_fraction"]) == [2, 3] and sorted(got["dup_fraction"]) == [5]
    assert got["top_fraction"][2].tolist() == [0.2, 0.22, 0.02, 0.2, 0.0] and got["top_fraction"][2].dtype == np.float64
    assert got["top_fraction"][3].tolist() == [0.18, 0.03, 0.21, 0.3, 0.0]
    assert got["dup_fraction"][5].tolist() == [0.15, 0.16, 0.0, 1.0, 0.0] and got["dup_fraction"][5].dtype == np.float64
    # at the bound is kept; document 1 fails width 2 and width 5, 2 fails width 3, 3 fails widths 3 and 5; an empty body is kept
    assert got["keep"].tolist() == [True, False, False, False, True] and got["keep"].dtype == bool
    only_dup = T._repeat_decide(dict(out), {}, {5: 0.15})
    assert only_dup["top_fraction"] == {} and only_dup["keep"].tolist() == [True, False, True, False, True]
    only_top = T._repeat_decide(dict(out), {3: 0.18}, {})
    assert only_top["dup_fraction"] == {} and only_top["keep"].tolist() == [True, True, False, False, True]
