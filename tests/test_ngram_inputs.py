"""CPU-only: every bad argument of the n-gram overlap calls of Tokenize is refused before any native call -- the width n, max_fraction,
texts that are not str, rows that are not integers, an object that is not an NgramIndex, a closed index, an index of another
Tokenize object -- and the oracle the GPU tests compare with (tests/ngram_oracle.py) gives known answers on small cases worked
by hand."""
import threading

import numpy as np
import pytest

import ngram_oracle as NO


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


class _InfoOnly:
    """a context that can describe and free an index and nothing else"""

    def __init__(self):
        self.destroyed = []

    def ngram_index_info(self, handle):
        return dict(n=3, n_rows=2, n_ids=9, n_grams=5, n_distinct=4, slots=16, device_bytes=12288, context_bytes=12288)

    def ngram_index_destroy(self, handle):
        self.destroyed.append(handle)

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare(ctx=None):
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = ctx if ctx is not None else _NoNative()
    t._dirty = True                                                   # (so that any table use would reach the context)
    t._batch_lock = threading.Lock()
    return t


def _index(ctx, handle=1234):
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    return tokenize.NgramIndex(ctx, handle)


BAD_N = [(0, ValueError), (33, ValueError), (-13, ValueError), (2 ** 40, ValueError), (True, TypeError), (False, TypeError), (13.0, TypeError),
         (np.float32(13), TypeError), (None, TypeError), ("13", TypeError), ([13], TypeError)]


def test_the_width_is_refused_before_any_native_call():
    t = _bare()
    for n, exc in BAD_N:
        with pytest.raises(exc):
            t._ngram_rule(n)
        with pytest.raises(exc):
            t.ngram_index([[1, 2, 3]], n)
        with pytest.raises(exc):
            t.ngram_index([[1, 2, 3]], n=n, framed=False)
        with pytest.raises(exc):
            t.encode_ngram_index(["a b"], n)
    assert t._ngram_rule() == 13 and t._ngram_rule(1) == 1 and t._ngram_rule(32) == 32
    assert t._ngram_rule(np.int64(8)) == 8 and type(t._ngram_rule(np.int16(8))) is int
    with pytest.raises(AssertionError, match="native call ngram_index_build"):
        t.ngram_index([[1, 2, 3]], 32)                                    # a good width reaches the context


def test_rows_and_texts_are_refused_before_any_native_call():
    ctx = _InfoOnly()
    t = _bare(ctx)
    ix = _index(ctx)
    for rows, exc in (([["a"]], (TypeError, ValueError)), ([[1.5, 2.0]], TypeError), ([[2 ** 31]], ValueError), ([[-2 ** 31 - 1]], ValueError),
                      (np.zeros((2, 3)), TypeError)):
        with pytest.raises(exc):
            t.ngram_index(rows)
        with pytest.raises(exc):
            t.ngram_overlap_rows(rows, ix)
    for texts in (["a", 3], ["a", None], [b"a"]):
        with pytest.raises(TypeError):
            t.encode_ngram_index(texts)
        with pytest.raises(TypeError):
            t.encode_ngram_overlap(texts, ix)
        with pytest.raises(TypeError):
            t.decontaminate(texts, ix)


def test_the_index_is_refused_before_any_native_call():
    ctx = _InfoOnly()
    t = _bare(ctx)
    for bad in (None, 1234, "index", object(), {"n": 13}, np.zeros(3)):
        for call in (lambda: t.ngram_overlap_rows([[1, 2, 3]], bad), lambda: t.encode_ngram_overlap(["a b"], bad),
                     lambda: t.decontaminate(["a b"], bad)):
            with pytest.raises(TypeError, match="NgramIndex"):
                call()
    ix = _index(ctx)
    assert (ix.n, ix.n_rows, ix.n_ids, ix.n_grams, ix.n_distinct, ix.device_bytes) == (3, 2, 9, 5, 4, 12288) and not ix.closed
    other = _bare(_InfoOnly())                                            # another Tokenize object: another context
    for call in (lambda: other.ngram_overlap_rows([[1, 2, 3]], ix), lambda: other.encode_ngram_overlap(["a b"], ix),
                 lambda: other.decontaminate(["a b"], ix)):
        with pytest.raises(ValueError, match="another Tokenize"):
            call()
    ix.close()
    assert ix.closed and ctx.destroyed == [1234]
    ix.close()                                                            # twice is fine, and frees once
    assert ctx.destroyed == [1234]
    for call in (lambda: t.ngram_overlap_rows([[1, 2, 3]], ix), lambda: t.encode_ngram_overlap(["a b"], ix), lambda: t.decontaminate(["a b"], ix)):
        with pytest.raises(ValueError, match="closed"):
            call()
    with _index(ctx, 77) as inner:                                        # a context manager: freed on the way out
        assert not inner.closed
    assert inner.closed and ctx.destroyed == [1234, 77]
    gone = _index(ctx, 78)
    del gone                                                              # garbage collection frees it too
    import gc
    gc.collect()
    assert ctx.destroyed == [1234, 77, 78]


BAD_FRACTION = [(-0.01, ValueError), (1.0001, ValueError), (2, ValueError), (-1, ValueError), (float("nan"), ValueError), (float("inf"), ValueError),
                (True, TypeError), ("0.5", TypeError), (None, TypeError), ([0.5], TypeError)]


def test_max_fraction_is_refused_before_any_native_call():
    ctx = _InfoOnly()
    t = _bare(ctx)
    ix = _index(ctx)
    for f, exc in BAD_FRACTION:
        with pytest.raises(exc):
            t.decontaminate(["a b"], ix, f)
        with pytest.raises(exc):
            t.decontaminate(["a b"], ix, max_fraction=f)
    t._dirty = False                                                      # (no table build: the next thing a good call touches is the encode)
    for f in (0, 0.0, 1, 1.0, 0.25, np.float32(0.5), np.int64(1)):
        with pytest.raises(AssertionError, match="native call"):
            t.decontaminate(["a b"], ix, f)


# ---- the oracle, on cases worked by hand -------------------------------------------------------------------------------------
def test_oracle_known_answers():
    ref = [[1, 2, 3, 4], [9], [2, 3, 4, 5], []]
    first = NO.index(ref, 3)
    assert first == {(1, 2, 3): 0, (2, 3, 4): 0, (3, 4, 5): 2} and NO.positions(ref, 3) == 4
    got = NO.overlap(first, 3, [[0, 1, 2, 3, 0, 3, 4, 5], [3, 4], [], [2, 3, 4, 5, 6], [7, 7, 7]])
    assert got["n_grams"].tolist() == [6, 0, 0, 3, 1]
    assert got["n_hits"].tolist() == [2, 0, 0, 2, 0]
    assert got["n_covered"].tolist() == [6, 0, 0, 4, 0]
    assert got["first_hit"].tolist() == [1, -1, -1, 0, -1]
    assert got["first_ref"].tolist() == [0, -1, -1, 0, -1]
    assert got["body_len"].tolist() == [8, 2, 0, 5, 3]
    assert got["covered"].tolist() == [0, 1, 1, 1, 0, 1, 1, 1] + [0, 0] + [1, 1, 1, 1, 0] + [0, 0, 0]
    assert got["row_off"].tolist() == [0, 8, 10, 10, 15, 18]
    assert all(got[k].dtype == np.int32 for k in NO.KEYS) and got["covered"].dtype == np.uint8


def test_oracle_frames_and_widths():
    first = NO.index([[-1, 5, 6, -2], [-1, -2], [-3]], 2, framed=True)
    assert first == {(5, 6): 0}
    got = NO.overlap(first, 2, [[8, 5, 6, 9], [5, 6], [5], [], [0, 5, 6, 5, 6, 0]], framed=True)
    assert got["n_hits"].tolist() == [1, 0, 0, 0, 2] and got["n_covered"].tolist() == [2, 0, 0, 0, 4]
    assert got["body_len"].tolist() == [2, 0, 0, 0, 4]
    assert got["covered"].tolist() == [0, 1, 1, 0] + [0, 0] + [0] + [0, 1, 1, 1, 1, 0]
    one = NO.index([[4, 4, 7]], 1)
    assert one == {(4,): 0, (7,): 0}
    got = NO.overlap(one, 1, [[7, 1, 4]])
    assert (got["n_grams"][0], got["n_hits"][0], got["n_covered"][0], got["first_hit"][0]) == (3, 2, 2, 0)
    # hits n apart abut, n + 1 apart leave a gap of one token
    first = NO.index([[1, 1, 1]], 3)
    assert NO.overlap(first, 3, [[1, 1, 1, 1, 1, 1]])["n_covered"][0] == 6
    assert NO.overlap(first, 3, [[1, 1, 1, 0, 1, 1, 1]])["n_covered"][0] == 6 and NO.overlap(first, 3, [[1, 1, 1, 0, 1, 1, 1]])["n_hits"][0] == 2
