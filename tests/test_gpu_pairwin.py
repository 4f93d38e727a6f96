"""Question-context windows with answer positions on the GPU (gz_pair_window_rows / gz_pair_window_rows_device, gz_span_tokens[_device];
Tokenize.pair_window_rows, span_tokens, encode_pair_windows, encode_pair_windows_to_device, pair_window_spans) against the rule of
tests/pairwin_oracle.py, which tests/test_pairwin_inputs.py ties to the reference and whose case lists it holds to their edges.
Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest

import pairwin_oracle as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


@pytest.fixture(scope="module")
def sp(tok):
    pad, bos, eos = tok._special_ids()[:3]
    return dict(pad=pad, bos=bos, eos=eos)


def same(got, want, L=None):
    assert set(want) <= set(got), sorted(set(want) - set(got))
    for k in want:
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        assert np.array_equal(g, want[k]), (k, np.argwhere(g != want[k])[:4].tolist())
    if L is not None:
        assert got["input_ids"].shape[1:] == (L,)


def frame(rows):
    return [[-7] + list(r) + [-9] for r in rows]                      # the frame is dropped whatever it holds


def check(tok, sp, questions, bodies, L, s, mq, q_row=None, answers=None):
    """bare bodies and framed rows against the oracle; returns the oracle's arrays"""
    want = P.batch(questions, bodies, L, s, mq, q_row=q_row, answers=answers, **sp)
    a = None if answers is None else np.array(answers, dtype=np.int32).reshape(len(bodies), 2)
    same(tok.pair_window_rows(questions, bodies, L, s, mq, q_row=q_row, answers=a, framed=False), want, L)
    same(tok.pair_window_rows(frame(questions), frame(bodies), L, s, mq, q_row=q_row, answers=a, framed=True), want, L)
    if answers is None:
        assert not set(P.ANSWER_KEYS) & set(tok.pair_window_rows(questions, bodies, L, s, mq, q_row=q_row, framed=False))
    return want


def spread_answers(lengths, seed):
    """an answer per context: present ones of 1..4 tokens all over the body, and every kind of absent one"""
    rng = np.random.default_rng(seed)
    out = []
    for k, T in enumerate(lengths):
        if T == 0 or k % 5 == 4:
            out.append([(-1, -1), (2, 2), (0, T + 1), (3, 1)][k % 4])
        else:
            a0 = int(rng.integers(0, T))
            out.append((a0, min(T, a0 + 1 + int(rng.integers(0, 4)))))
    return out


# ---- the cell rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,mq,s", P.rule_cases())
def test_cell_rule_at_its_edges(tok, sp, L, mq, s):
    tqs, ts = P.rule_pairs(L, mq, s)
    questions, bodies = P.counters(tqs, base=-5000), P.counters(ts)
    want = check(tok, sp, questions, bodies, L, s, mq, answers=spread_answers(ts, L * 1000 + mq * 10 + s))
    assert want["has_answer"].any() or max(ts) < 2
    check(tok, sp, questions, bodies, L, s, mq)
    for Tq, T in sorted(set(zip(tqs, ts)))[::3]:                       # ... and pairs as batches of their own
        check(tok, sp, P.counters([Tq], base=-9), P.counters([T]), L, s, mq, answers=[(0, min(T, 2))])


@pytest.mark.parametrize("L,s,mq", [(8, 0, 3), (9, 2, 1)])
def test_mask_type_and_odd_ids(tok, sp, L, s, mq):
    """The pad id, bos and eos, negative ids and ids above the vocabulary pass through both sources; the mask is 0 exactly at the pad id,
    the type row holds the pad id exactly behind n_real."""
    odd = [sp["pad"], sp["bos"], sp["eos"], -1, -5, 2 ** 31 - 1, -2 ** 31, 70000, tok.vocab_size() + 1, 7]
    rng = np.random.default_rng(3)
    bodies = [rng.choice(odd, size=T).tolist() for T in (0, 1, 5, 6, 7, 13, 40, 3)] + [[sp["pad"]] * 9, odd]
    questions = [rng.choice(odd, size=T).tolist() for T in (3, 0, 1, 4, 2, 3, 3, 5)] + [[sp["pad"]] * 3, odd[:3]]
    got = tok.pair_window_rows(questions, bodies, L, s, mq, framed=False)
    same(got, P.batch(questions, bodies, L, s, mq, **sp), L)
    assert np.array_equal(got["attention_mask"], (got["input_ids"] != sp["pad"]).astype(np.int32))
    real = np.arange(L)[None, :] < got["n_real"][:, None]
    assert ((got["attention_mask"] == 0) & real).any()                # real tokens equal to the pad id: mask 0 there too
    assert (got["token_type_ids"][~real] == sp["pad"]).all() and np.isin(got["token_type_ids"][real], (0, 1)).all()


# ---- work division ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", P.WORK_WS)
def test_window_counts_at_the_waves_edges(tok, sp, W):
    ts = P.work_lengths(W)
    questions, bodies = P.counters([2] * len(ts), base=-900), P.counters(ts)
    want = check(tok, sp, questions, bodies, P.WORK_L, P.WORK_S, P.WORK_MQ, answers=spread_answers(ts, W))
    assert len(want["pair"]) == W


def test_one_long_context_among_short_ones(tok, sp):
    ts = [3, 0, P.LONG_T, 7, 1]
    questions, bodies = P.counters([2, 0, 5, 1, 2], base=-900), P.counters(ts)
    answers = [(1, 3), (-1, -1), (P.LONG_T - 4, P.LONG_T - 1), (6, 7), (0, 1)]
    want = check(tok, sp, questions, bodies, P.WORK_L, P.WORK_S, P.WORK_MQ, answers=answers)
    k = want["win_off"]
    assert k[3] - k[2] > 40 * 64 and (want["pair"][k[2]:k[3]] == 2).all() and want["has_answer"][k[2]:k[3]].sum() == 1
    assert want["has_answer"][k[3] - 1] == 1


def test_no_pairs(tok, sp):
    for questions in ([], [[5, 6]]):
        got = tok.pair_window_rows(questions, [], 16, 2, 3, q_row=np.zeros(0, dtype=np.int32) if questions else None,
                                   answers=np.zeros((0, 2), dtype=np.int32), framed=False)
        same(got, P.batch(questions, [], 16, 2, 3, answers=[], **sp), 16)
        assert got["win_off"].tolist() == [0] and got["input_ids"].shape == (0, 16) and got["has_answer"].shape == (0,)


def test_shared_and_reordered_questions(tok, sp):
    ts = [0, 5, 11, 12, 13, 40, 1]
    bodies = P.counters(ts)
    check(tok, sp, P.counters([4], base=-50), bodies, 16, 3, 6, q_row=[0] * len(ts), answers=spread_answers(ts, 1))       # NQ = 1
    questions = P.counters([0, 1, 2, 3, 6, 7, 9], base=-500)
    check(tok, sp, questions, bodies, 16, 3, 6, q_row=list(range(len(ts)))[::-1], answers=spread_answers(ts, 2))         # reversed
    check(tok, sp, questions, bodies, 16, 3, 6, q_row=[6, 6, 0, 3, 3, 1, 5])
    check(tok, sp, questions + [[1, 2, 3]] * 4, bodies, 16, 3, 6, q_row=[10, 0, 9, 3, 3, 1, 5])                          # more questions than pairs


# ---- the device entry point --------------------------------------------------------------------------------------------------------------
FILL = 0x5A5A5A5A
OUT_KEYS = P.KEYS[:7] + P.ANSWER_KEYS                                  # the ten device outputs, in argument order


class Guarded:
    """n int32 cells on the device between two runs of guard cells, all pre-filled with FILL."""

    def __init__(self, ctx, n, guard):
        self.ctx, self.n, self.guard = ctx, n, guard
        self.base = ctx.alloc(4 * (n + 2 * guard) + 16)
        ctx.h2d(self.base, np.full(n + 2 * guard, FILL, dtype=np.int32))
        self.ptr = self.base + 4 * guard

    def read(self):
        a = np.empty(self.n + 2 * self.guard, dtype=np.int32)
        self.ctx.d2h(a, self.base)
        assert (a[:self.guard] == FILL).all() and (a[self.guard + self.n:] == FILL).all(), "guard cells were written"
        return a[self.guard:self.guard + self.n]


class Device:
    """The inputs of a device call between canary cells (-77 in front, -88 behind: offsets do not start at 0), and guarded outputs."""

    def __init__(self, ctx, questions, bodies, q_row, answers, junk=37):
        self.ctx, self.held = ctx, []
        self.n, self.nq = len(bodies), len(questions)

        def packed(rows):
            flat = np.array([-77] * junk + [v for b in rows for v in b] + [-88] * 5, dtype=np.int32)
            off = np.zeros(len(rows) + 1, dtype=np.int64)
            if rows:
                np.cumsum([len(b) for b in rows], out=off[1:])
            return self.up(flat), self.up(off + junk)
        self.d_q, self.d_qo = packed(questions)
        self.d_c, self.d_co = packed(bodies)
        self.d_qr = 0 if q_row is None else self.up(np.array(q_row, dtype=np.int32))
        self.d_ans = 0 if answers is None else self.up(np.array(answers, dtype=np.int32).reshape(-1))
        self.d_wo = self.up(np.full(self.n + 1, -1, dtype=np.int64))

    def up(self, a):
        d = self.ctx.alloc(max(a.nbytes, 1) + 16)
        self.held.append(d)
        if a.nbytes:
            self.ctx.h2d(d, a)
        return d

    def outputs(self, W, L, guard):
        g = [Guarded(self.ctx, W * L if k < 3 else W, guard) for k in range(10)]
        self.held += [x.base for x in g]
        return g

    def call(self, L, s, mq, ptrs, capacity, skip=0):
        return self.ctx.pair_window_rows_device(self.d_q, self.d_qo, self.nq, self.d_c, self.d_co, self.n, self.d_qr, self.d_ans, L, s, mq, skip, skip,
                                                *ptrs, self.d_wo, capacity)

    def win_off(self):
        wo = np.empty(self.n + 1, dtype=np.int64)
        self.ctx.d2h(wo, self.d_wo)
        return wo

    def free(self):
        for d in self.held:
            self.ctx.free(d)


def read_outputs(g, want, W, L):
    got = {}
    for k, (x, key) in enumerate(zip(g, OUT_KEYS)):
        got[key] = x.read().reshape((W, L) if k < 3 else (W,))
    return got


@pytest.mark.parametrize("L,s,mq,guard", [(8, 1, 2, 64), (8, 1, 2, 65), (12, 0, 3, 67), (13, 4, 2, 64), (128, 32, 16, 65)])
def test_device_form_behind_junk_with_exact_capacity(tok, sp, L, s, mq, guard):
    """Sizing call; capacity W - 1 (GZ_E_CAPACITY, total = W, win_off valid, outputs untouched); exact capacity; every optional output
    left out in turn, and the answers left out while their outputs are asked for.  guard 64: 16-byte aligned outputs; 65 / 67: the
    outputs start 4 and 12 bytes off a 16-byte boundary, so that the one-cell path runs although L % 4 == 0."""
    from genz_tokenize import _native
    tok._sync_tables()
    ts = [0, 3, L - 4 - mq, L - 3 - mq, 5 * L + 1, 0, 1, 2 * L]
    questions, bodies = P.counters([mq, 0, mq + 3, 1, mq, 2, mq + 1, 0], base=-4000), P.counters(ts)
    answers = spread_answers(ts, L)
    want = P.batch(questions, bodies, L, s, mq, answers=answers, **sp)
    W = len(want["pair"])
    if guard != 64 and L % 4 == 0:
        assert (4 * guard) % 16 != 0
    D = Device(tok._ctx, questions, bodies, None, answers)
    try:
        assert D.call(L, s, mq, [0] * 10, 0) == W                                              # sizing
        assert D.win_off().tolist() == want["win_off"].tolist()
        g = D.outputs(W, L, guard)
        tok._ctx.h2d(D.d_wo, np.full(D.n + 1, -1, dtype=np.int64))
        with pytest.raises(_native.GzError) as e:                                              # one window too few
            D.call(L, s, mq, [x.ptr for x in g], W - 1)
        assert e.value.code == _native.GZ_E_CAPACITY and e.value.total == W
        assert D.win_off().tolist() == want["win_off"].tolist()
        for x in g:
            assert (x.read() == FILL).all()
        assert D.call(L, s, mq, [x.ptr for x in g], W) == W                                    # exact capacity
        same(dict(read_outputs(g, want, W, L), win_off=D.win_off()), want, L)
        for drop in [[k] for k in range(1, 10)] + [list(range(1, 10))]:                        # optional outputs left out
            g = D.outputs(W, L, guard)
            assert D.call(L, s, mq, [0 if k in drop else x.ptr for k, x in enumerate(g)], W + 3) == W
            for k, (x, key) in enumerate(zip(g, OUT_KEYS)):
                a = x.read()
                assert (a == FILL).all() if k in drop else np.array_equal(a.reshape(want[key].shape), want[key]), (drop, key)
        # answers left out while their outputs are asked for: the three stay untouched, the rest is the same
        g = D.outputs(W, L, guard)
        D.d_ans, keep = 0, D.d_ans
        assert D.call(L, s, mq, [x.ptr for x in g], W) == W
        D.d_ans = keep
        for k, (x, key) in enumerate(zip(g, OUT_KEYS)):
            a = x.read()
            assert (a == FILL).all() if k >= 7 else np.array_equal(a.reshape(want[key].shape), want[key]), key
    finally:
        D.free()


def test_device_form_reads_a_q_row_outside_the_questions_as_an_empty_question(tok, sp):
    tok._sync_tables()
    L, s, mq = 12, 2, 3
    ts = [9, 0, 4, 30, 5, 6]
    questions, bodies = P.counters([3, 5, 1], base=-4000), P.counters(ts)
    q_row = [-1, 3, 1, -2 ** 31, 2 ** 31 - 1, 0]                       # -1 and NQ among them: no address may be formed from these
    answers = spread_answers(ts, 5)
    want = P.batch(questions, bodies, L, s, mq, q_row=q_row, answers=answers, **sp)
    assert want["q_len"][want["pair"] == 0].tolist() == [0] * 2 and (want["q_len"][want["pair"] == 3] == 0).all() and want["q_len"].max() == 3
    W = len(want["pair"])
    D = Device(tok._ctx, questions, bodies, q_row, answers)
    try:
        assert D.call(L, s, mq, [0] * 10, 0) == W
        g = D.outputs(W, L, 64)
        assert D.call(L, s, mq, [x.ptr for x in g], W) == W
        same(dict(read_outputs(g, want, W, L), win_off=D.win_off()), want, L)
    finally:
        D.free()
    with pytest.raises(ValueError):                                    # the Python layer refuses them
        tok.pair_window_rows(questions, bodies, L, s, mq, q_row=q_row, framed=False)


INVALID = [dict(L=4), dict(L=0), dict(L=-1), dict(mq=-1), dict(mq=12), dict(s=-1), dict(s=6, mq=6), dict(s=12, mq=0), dict(skip=2), dict(skip=-1),
           dict(cap=-1), dict(n=-1), dict(nq=-1), dict(nq=3, q_row=False)]


def test_refusals_at_the_abi_write_nothing_and_leave_the_context_usable(tok, sp):
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    questions, bodies = P.counters([2, 3], base=-40), P.counters([9, 4])
    D = Device(ctx, questions, bodies, [1, 0], [(0, 1), (1, 2)])
    q_flat, q_off = np.array([v for b in questions for v in b], dtype=np.int32), np.array([0, 2, 5], dtype=np.int64)
    c_flat, c_off = np.array([v for b in bodies for v in b], dtype=np.int32), np.array([0, 9, 13], dtype=np.int64)
    q_row, ans = np.array([1, 0], dtype=np.int32), np.array([[0, 1], [1, 2]], dtype=np.int32)
    ptr = _native._ptr
    try:
        g = D.outputs(8, 16, 64)
        for bad in INVALID:
            a = dict(dict(L=16, s=2, mq=4, skip=0, cap=8, n=2, nq=2, q_row=True), **bad)
            ctx.h2d(D.d_wo, np.full(3, -1, dtype=np.int64))
            with pytest.raises(_native.GzError) as e:
                ctx.pair_window_rows_device(D.d_q, D.d_qo, a["nq"], D.d_c, D.d_co, a["n"], D.d_qr if a["q_row"] else 0, D.d_ans, a["L"], a["s"], a["mq"],
                                            a["skip"], a["skip"], *[x.ptr for x in g], D.d_wo, a["cap"])
            assert e.value.code == _native.GZ_E_INVALID, bad
            assert D.win_off().tolist() == [-1] * 3, bad
            for x in g:
                assert (x.read() == FILL).all(), bad
            host = [np.full(8 * 16 if k < 3 else 8, FILL, dtype=np.int32) for k in range(10)]
            wo, total = np.full(3, -1, dtype=np.int64), ctypes.c_int64(-5)
            rc = ctx.lib.gz_pair_window_rows(ctx.handle, ptr(q_flat), ptr(q_off), a["nq"], ptr(c_flat), ptr(c_off), a["n"], ptr(q_row) if a["q_row"] else None,
                                             ptr(ans), a["L"], a["s"], a["mq"], a["skip"], a["skip"], *[ptr(h) for h in host], ptr(wo), a["cap"],
                                             ctypes.byref(total))
            assert rc == _native.GZ_E_INVALID and wo.tolist() == [-1] * 3 and all((h == FILL).all() for h in host), bad
        # the host form alone can read q_row and the offsets: refused there
        for qr, qo, co in (([2, 0], q_off, c_off), ([0, -1], q_off, c_off), ([1, 0], np.array([0, 3, 2]), c_off), ([1, 0], q_off, np.array([0, 9, 8]))):
            host = [np.full(8 * 16 if k < 3 else 8, FILL, dtype=np.int32) for k in range(10)]
            wo, total = np.full(3, -1, dtype=np.int64), ctypes.c_int64(-5)
            qr, qo, co = np.array(qr, dtype=np.int32), np.array(qo, dtype=np.int64), np.array(co, dtype=np.int64)
            rc = ctx.lib.gz_pair_window_rows(ctx.handle, ptr(q_flat), ptr(qo), 2, ptr(c_flat), ptr(co), 2, ptr(qr), ptr(ans), 16, 2, 4, 0, 0,
                                             *[ptr(h) for h in host], ptr(wo), 8, ctypes.byref(total))
            assert rc == _native.GZ_E_INVALID and wo.tolist() == [-1] * 3 and all((h == FILL).all() for h in host)
        assert D.call(16, 2, 4, [0] * 10, 0) == 2
    finally:
        D.free()
    check(tok, sp, questions, bodies, 16, 2, 4, q_row=[1, 0], answers=[(0, 1), (1, 2)])


# ---- answers ----------------------------------------------------------------------------------------------------------------------------
def test_answers_at_the_windows_edges(tok, sp):
    names = sorted(P.ANSWERS)
    questions = P.counters([P.ANSWER_TQ], base=-30)
    bodies = P.counters([P.ANSWER_T] * len(names))
    answers = [P.ANSWERS[k] for k in names]
    want = check(tok, sp, questions, bodies, P.ANSWER_L, P.ANSWER_S, P.ANSWER_MQ, q_row=[0] * len(names), answers=answers)
    held = {k: want["has_answer"][want["win_off"][i]:want["win_off"][i + 1]].tolist() for i, k in enumerate(names)}
    assert held["in_overlap"] == [1, 1, 0, 0, 0] and held["straddles_end"] == [0, 1, 0, 0, 0] and held["longer_than_room"] == [0] * 5
    assert held["whole_tail"] == [0, 0, 0, 0, 1] and held["none"] == held["empty"] == held["past_end"] == [0] * 5
    got = tok.pair_window_rows(questions, bodies, P.ANSWER_L, P.ANSWER_S, P.ANSWER_MQ, q_row=[0] * len(names),
                               answers=np.array(answers, dtype=np.int32), framed=False)
    for w in np.flatnonzero(got["has_answer"]):                        # law 4 on the device's own arrays
        r, a = int(got["pair"][w]), answers[int(got["pair"][w])]
        assert got["input_ids"][w, got["start_positions"][w]:got["end_positions"][w] + 1].tolist() == bodies[r][a[0]:a[1]]


# ---- framed and bare, slices against the whole ------------------------------------------------------------------------------------------
def test_slices_give_the_windows_of_their_pairs(tok, sp):
    L, s, mq = 12, 2, 3
    ts = [0, 20, 5, 6, 7, 33, 1, 0, 14]
    questions, bodies = P.counters([3, 0, 5, 1, 2, 3, 4, 0, 9], base=-700), P.counters(ts)
    answers = np.array(spread_answers(ts, 9), dtype=np.int32)
    whole = tok.pair_window_rows(frame(questions), frame(bodies), L, s, mq, answers=answers)
    same(whole, P.batch(questions, bodies, L, s, mq, answers=answers.tolist(), **sp), L)
    k = whole["win_off"]
    for a, b in ((0, 9), (0, 4), (4, 9), (1, 2), (5, 6), (3, 3), (8, 9)):
        part = tok.pair_window_rows(frame(questions)[a:b], frame(bodies)[a:b], L, s, mq, answers=answers[a:b])
        for key in P.KEYS[:7] + P.ANSWER_KEYS:
            want = whole[key][k[a]:k[b]] - (a if key == "pair" else 0)
            assert np.array_equal(part[key], want), (a, b, key)
        assert np.array_equal(part["win_off"], k[a:b + 1] - k[a])


# ---- span tokens --------------------------------------------------------------------------------------------------------------------------
def span_tokens_want(counts, word_off, mark_words, mark_off):
    cs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    out = np.full((len(mark_words), 2), -1, dtype=np.int32)
    for d in range(len(word_off) - 1):
        for m in range(mark_off[d], mark_off[d + 1]):
            f, e = mark_words[m]
            if f >= 0:
                out[m] = (cs[word_off[d] + f] - cs[word_off[d]], cs[word_off[d] + e] - cs[word_off[d]])
    return out


def test_span_tokens_against_a_cumulative_sum(tok):
    counts = np.array([1, 1, 4, 1, 9, 2, 1, 1, 1, 3, 1, 30, 1], dtype=np.int32)                # words of 1 and many pieces
    word_off = np.array([0, 3, 3, 8, 9, 13], dtype=np.int64)                                  # an empty document among them
    marks = [[(0, 1), (0, 3), (2, 3), (-1, -1)], [(-1, -1)], [(4, 5), (0, 5), (1, 1), (3, 5)], [], [(0, 4), (3, 4), (-1, -1), (2, 3), (0, 0)]]
    mark_words = np.array([m for ms in marks for m in ms], dtype=np.int32)
    mark_off = np.concatenate(([0], np.cumsum([len(ms) for ms in marks]))).astype(np.int64)
    want = span_tokens_want(counts, word_off, mark_words, mark_off)
    assert want[1].tolist() == [0, 6] and want[4].tolist() == [-1, -1] and want[5].tolist() == [13, 14] and want[9].tolist() == [0, 35]
    got = tok.span_tokens(counts, word_off, mark_words, mark_off)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    none = tok.span_tokens(counts, word_off, np.zeros((0, 2), dtype=np.int32), np.zeros(6, dtype=np.int64))       # S = 0
    assert none.shape == (0, 2) and none.dtype == np.int32
    assert tok.span_tokens(np.zeros(0, dtype=np.int32), [0], np.zeros((0, 2), dtype=np.int32), [0]).shape == (0, 2)
    # many words and marks: the scan of several blocks, a mark per document over its last word and over all of it
    rng = np.random.default_rng(5)
    nw = rng.integers(0, 9, size=3000)
    word_off = np.concatenate(([0], np.cumsum(nw))).astype(np.int64)
    counts = rng.integers(1, 6, size=int(word_off[-1])).astype(np.int32)
    mw, moff = [], [0]
    for n in nw.tolist():
        mw += [(n - 1, n), (0, n), (-1, -1)] if n else [(-1, -1)]
        moff.append(len(mw))
    mw, moff = np.array(mw, dtype=np.int32), np.array(moff, dtype=np.int64)
    assert np.array_equal(tok.span_tokens(counts, word_off, mw, moff), span_tokens_want(counts, word_off, mw, moff))
    # the device form behind junk (absolute offsets) between guard cells
    ctx, junk_w, junk_m = tok._ctx, 11, 3
    held = []

    def up(a):
        d = ctx.alloc(max(a.nbytes, 1) + 16)
        held.append(d)
        ctx.h2d(d, a)
        return d
    try:
        d_counts = up(np.concatenate((np.full(junk_w, -77, dtype=np.int32), counts, np.full(4, -88, dtype=np.int32))))
        out = Guarded(ctx, 2 * len(mw), 64)
        held.append(out.base)
        ctx.span_tokens_device(d_counts, up(word_off + junk_w), len(nw), len(counts), up(mw), up(moff + junk_m), len(mw), out.ptr)
        assert np.array_equal(out.read().reshape(-1, 2), span_tokens_want(counts, word_off, mw, moff))
    finally:
        for d in held:
            ctx.free(d)


# ---- text, end to end ---------------------------------------------------------------------------------------------------------------------
def bodies_of(tok, texts):
    r = tok.encode_batch(texts, max_len=None)
    ro = r["row_off"]
    return [r["input_ids"][ro[i] + 1:ro[i + 1] - 1].tolist() for i in range(len(texts))]


@pytest.fixture(scope="module")
def qa(tok):
    contexts = P.texts(48, 1, 60, 7)
    questions = P.texts(12, 0, 9, 8)
    spans, words = P.word_answers(contexts, 3)
    q_row = [i % 12 for i in range(48)]
    return questions, contexts, spans, words, q_row, bodies_of(tok, questions), bodies_of(tok, contexts)


@pytest.mark.parametrize("L,s,mq", [(32, 8, None), (48, 0, 6), (29, 12, 4)])
def test_text_end_to_end(tok, sp, qa, L, s, mq):
    questions, contexts, spans, words, q_row, qb, cb = qa
    got = tok.encode_pair_windows(questions, contexts, L, s, mq, q_row=q_row, answers=spans)
    mq_eff = tok._pair_window_rule(L, s, mq)[2]
    # word-granular answers: the tokens of the words first .. last
    counts = got["word_tokens"]
    want_tok = np.full((48, 2), -1, dtype=np.int32)
    for i, w in enumerate(words):
        if w is not None:
            cs = np.concatenate(([0], np.cumsum(counts[got["word_off"][i]:got["word_off"][i + 1]])))
            want_tok[i] = (cs[w[0]], cs[w[1] + 1])
    assert np.array_equal(got["answer_tokens"], want_tok) and got["answer_tokens"].dtype == np.int32
    assert [int(counts[got["word_off"][i]:got["word_off"][i + 1]].sum()) for i in range(48)] == [len(b) for b in cb]
    want = P.batch(qb, cb, L, s, mq_eff, q_row=q_row, answers=want_tok.tolist(), **sp)
    same(got, want, L)
    assert want["has_answer"].sum() >= 12 and (np.diff(want["win_off"]) > 2).any()
    # decode(row[start : end + 1]) is the answer's words
    rows = [got["input_ids"][w, got["start_positions"][w]:got["end_positions"][w] + 1].tolist() for w in np.flatnonzero(got["has_answer"])]
    said = [" ".join(re.findall(r"\S+", contexts[i])[words[i][0]:words[i][1] + 1]) for i in got["pair"][np.flatnonzero(got["has_answer"])].tolist()]
    assert tok.decode_batch(rows) == tok.decode_batch(bodies_of(tok, said)) and len(rows) >= 12
    # the round trip: positions -> character spans of the words the answer overlaps
    back = tok.pair_window_spans(got, got["start_positions"], got["end_positions"])
    for w in range(len(got["pair"])):
        i = int(got["pair"][w])
        assert back[w].tolist() == (list(spans[i]) if got["has_answer"][w] else [-1, -1]), w
    # the device form
    dev = tok.encode_pair_windows_to_device(questions, contexts, L, s, mq, q_row=q_row, answers=spans)
    W = len(want["pair"])
    for k in ("input_ids", "attention_mask", "token_type_ids"):
        assert not isinstance(dev[k], np.ndarray) and dev[k].shape == (W, L)
    same(dev, want, L)
    for k in ("word_off", "word_span", "word_tokens", "answer_tokens"):
        assert np.array_equal(dev[k], got[k]), k
    # no answers: the same windows, no answer arrays
    bare = tok.encode_pair_windows(questions, contexts, L, s, mq, q_row=q_row)
    same(bare, {k: want[k] for k in P.KEYS}, L)
    assert not (set(P.ANSWER_KEYS) | {"answer_tokens"}) & set(bare)
    if L == 48:
        same(tok.encode_pair_windows(questions, contexts, L, s, mq, q_row=q_row, answers=np.array([x or (-1, -1) for x in spans]), word_table=False), want, L)


def test_law_1_against_encode_batch_itself(tok, sp):
    """A pair that fits makes one window: the row, mask and type row of encode_batch(questions, pair_texts=contexts, max_len=L), but for
    the last cell of a full row, where the reference puts the eos id and the rule puts 1."""
    questions, contexts = P.texts(40, 0, 4, 31), P.texts(40, 1, 5, 32)
    qb, cb = bodies_of(tok, questions), bodies_of(tok, contexts)
    fullest = max(len(q) + 4 + len(c) for q, c in zip(qb, cb))
    seen = {"below": 0, "full": 0}
    for L in (fullest, fullest - 3, 24):
        mq = L - 5
        ref = tok.encode_batch(questions, pair_texts=contexts, max_len=L)
        got = tok.encode_pair_windows(questions, contexts, L, 0, mq)
        for i, (q, c) in enumerate(zip(qb, cb)):
            n_real = len(q) + 4 + len(c)
            if len(q) > mq or n_real > L:
                continue
            assert got["win_off"][i + 1] - got["win_off"][i] == 1
            w = int(got["win_off"][i])
            assert np.array_equal(got["input_ids"][w], ref["input_ids"][i]) and np.array_equal(got["attention_mask"][w], ref["attention_mask"][i])
            if n_real < L:
                assert np.array_equal(got["token_type_ids"][w], ref["token_type_ids"][i]), i
                seen["below"] += 1
            else:
                assert np.array_equal(got["token_type_ids"][w, :-1], ref["token_type_ids"][i, :-1])
                assert ref["token_type_ids"][i, -1] == sp["eos"] and got["token_type_ids"][w, -1] == 1          # the one deviation
                seen["full"] += 1
    assert seen["below"] >= 40 and seen["full"] >= 1


def test_no_texts_and_empty_texts(tok, sp):
    for questions, contexts in (([], []), ([""], [""]), (["xin", ""], ["", "   "])):
        want = P.batch([bodies_of(tok, [q])[0] if q.strip() else [] for q in questions], [[] for _ in contexts], 8, 2, 1, answers=[(-1, -1)] * len(contexts), **sp)
        same(tok.encode_pair_windows(questions, contexts, 8, 2, 1, answers=[None] * len(contexts)), want, 8)
        same(tok.encode_pair_windows_to_device(questions, contexts, 8, 2, 1, answers=[None] * len(contexts)), want, 8)


# ---- other tables ---------------------------------------------------------------------------------------------------------------------------
def test_specials_follow_the_live_table(tmp_path):
    """A vocabulary whose specials moved away from 0..3 (tests/row_tables.py): pad, bos, eos and the type row's padding are the live ids."""
    from genz_tokenize import Tokenize
    import row_tables as RT
    t = RT.moved()
    vocab, merges = os.path.join(tmp_path, "moved.vocab"), os.path.join(tmp_path, "moved.codes")
    for path, data in ((vocab, t.vocab), (merges, t.merges)):
        with open(path, "wb") as f:
            f.write(data)
    tok = Tokenize.__new__(Tokenize)
    tok.vocab_file, tok.bpe_file = vocab, merges
    pad, bos, eos, mask, unk = t.specials
    tok.__init__(pad_token=pad, bos_token=bos, eos_token=eos, mask_token=mask, unk_token=unk)
    assert tuple(tok._special_ids()[:4]) == t.ids and min(t.ids) > 3 and len({t.pad, t.bos, t.eos}) == 3
    sp = dict(pad=t.pad, bos=t.bos, eos=t.eos)
    ts = [0, 5, 9, 10, 25, 1]
    questions, bodies = P.counters([2, 0, 4, 3, 1, 9]), [[0, 1, 2, 3, t.pad, t.eos, t.bos][k % 7:] + list(range(T)) for k, T in enumerate(ts)]
    got = tok.pair_window_rows(questions, bodies, 16, 3, 3, answers=np.array(spread_answers([len(b) for b in bodies], 4), dtype=np.int32), framed=False)
    same(got, P.batch(questions, bodies, 16, 3, 3, answers=spread_answers([len(b) for b in bodies], 4), **sp), 16)
    real = np.arange(16)[None, :] < got["n_real"][:, None]
    assert (got["token_type_ids"][~real] == t.pad).all() and (got["input_ids"][~real] == t.pad).all() and (~real).any()
    assert (got["input_ids"][:, 0] == t.bos).all() and (got["input_ids"][np.arange(len(real)), got["n_real"] - 1] == t.eos).all()
    texts = RT.texts(24, 6)
    qs = RT.texts(24, 7, max_words=3)
    out = tok.encode_pair_windows(qs, texts, 12, 2, 3)
    same(out, P.batch(bodies_of(tok, qs), bodies_of(tok, texts), 12, 2, 3, **sp), 12)
