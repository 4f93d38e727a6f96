"""Exact token n-gram overlap against a held-out set on the GPU (gz_ngram_index_build / _device, gz_ngram_overlap / _device;
Tokenize.ngram_index, encode_ngram_index, ngram_overlap_rows, encode_ngram_overlap, decontaminate) against the rule of
tests/ngram_oracle.py -- sets and dicts of tuples, no hash --, which tests/test_ngram_inputs.py ties to answers worked by hand.
Every comparison is exact, on all five arrays, body_len and the covered bytes."""
import ctypes
import random

import numpy as np
import pytest

import ngram_oracle as NO
import window_oracle as WO

pytestmark = pytest.mark.gpu

PIECE = 4096                                                             # n-gram positions a wave takes (csrc/gz_pieces.inc: GZ_PIECE)
FILL = 0x5A5A5A5A
OUT = ("n_grams", "n_hits", "n_covered", "first_hit", "first_ref")


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


def same(got, want, covered=True):
    keys = NO.KEYS + (("covered", "row_off") if covered else ())
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    assert sorted(got) == sorted(keys)


def check(tok, ref, n, rows, framed=False):
    """index + query against the oracle; the oracle's result and its index"""
    first = NO.index(ref, n, framed)
    want = NO.overlap(first, n, rows, framed)
    with tok.ngram_index(ref, n, framed=framed) as ix:
        flat = sum(len(r) for r in ref)
        assert (ix.n, ix.n_rows, ix.n_ids, ix.n_grams, ix.n_distinct) == (n, len(ref), flat, NO.positions(ref, n, framed), len(first))
        same(tok.ngram_overlap_rows(rows, ix, framed=framed, return_covered=True), want)
        same(tok.ngram_overlap_rows(rows, ix, framed=framed), want, covered=False)
    return want, first


def occur(want, first, ref, n, framed=False):
    """hits, misses and repeated n-grams all occur: the test cannot pass vacuously"""
    assert want["n_hits"].sum() > 0, "no hit"
    assert (want["n_hits"] < want["n_grams"]).any(), "no miss"
    assert NO.positions(ref, n, framed) > len(first), "no repeated n-gram"


def reference(rng, lengths, n):
    """Bodies of the given lengths over the alphabet 0..6; every later body of n ids or more starts with a copy out of an earlier
    one, so that n-grams repeat across rows."""
    out, pool = [], []
    for T in lengths:
        b = rng.integers(0, 7, size=T).tolist()
        if pool and T >= n:
            src = pool[int(rng.integers(0, len(pool)))]
            k = int(rng.integers(n, min(len(src), T) + 1))
            at = int(rng.integers(0, len(src) - k + 1))
            b[:k] = src[at:at + k]
        if T >= n:
            pool.append(b)
        out.append(b)
    return out


def mixture(rng, ref, n, T):
    """A body of T ids: runs copied out of the reference bodies (hits) between random runs over 0..8 (misses)."""
    pool = [b for b in ref if len(b) >= n]
    b = []
    while len(b) < T:
        b += rng.integers(0, 9, size=int(rng.integers(1, n + 6))).tolist()
        if pool:
            src = pool[int(rng.integers(0, len(pool)))]
            k = int(rng.integers(n, min(len(src), 3 * n) + 1))
            at = int(rng.integers(0, len(src) - k + 1))
            b += src[at:at + k]
    return b[:T]


# ---- the rule's edges, the trips' and the pieces' ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 13, 32])
def test_body_lengths_at_the_rules_and_the_trips_edges(tok, n):
    """nothing, one id, around the width; around one and two trips of 64 positions -- on both sides"""
    rng = np.random.default_rng(n)
    lengths = sorted({0, 1, max(n - 1, 0), n, n + 1, 63, 64, 65, 64 + n - 2, 64 + n - 1, 64 + n, 127, 128, 129})
    ref = reference(rng, lengths, n)
    rows = [mixture(rng, ref, n, T) for T in lengths] + [list(b) for b in ref[-3:]]
    want, first = check(tok, ref, n, rows)
    occur(want, first, ref, n)
    assert want["n_grams"].tolist()[:len(lengths)] == [max(T - n + 1, 0) for T in lengths]
    assert (want["n_hits"][-3:] == want["n_grams"][-3:]).all()            # a reference body queried: every position hits
    for T in (0, 1, n, 64 + n - 1, 64 + n):                               # ... and as batches of their own
        check(tok, ref, n, [mixture(rng, ref, n, T)])


def test_body_lengths_around_the_piece(tok):
    """one below, at and above one piece, and two pieces: rows of more than one piece are split over waves and meet by atomics --
    on both sides"""
    n = 13
    rng = np.random.default_rng(5)
    lengths = [PIECE - 1 + n - 1, PIECE + n - 1, PIECE + 1 + n - 1, 2 * PIECE + n]
    ref = reference(rng, [40, 200] + lengths, n)
    rows = [mixture(rng, ref, n, T) for T in lengths] + [mixture(rng, ref, n, 30), []]
    want, first = check(tok, ref, n, rows)
    occur(want, first, ref, n)
    assert want["n_grams"].tolist()[:4] == [PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 1]
    for T in (PIECE + n - 1, PIECE + n):                                  # one piece alone; two pieces alone
        check(tok, ref[:2], n, [mixture(rng, ref[:2], n, T)])


def test_one_long_body_between_short_ones(tok):
    """A body of five pieces between short ones.  One reference n-gram is planted so that it straddles a piece boundary, ends on a
    boundary's first token (the farthest look-back), starts on a piece's last position and on a piece's first: coverage looks
    back across the boundary and no hit is counted twice."""
    n = 13
    rng = np.random.default_rng(8)
    g = list(range(100, 100 + n))
    ref = reference(rng, [50, 300], n) + [[5] + g + [6]] + reference(rng, [80], n) + [[1] + g]
    long = rng.integers(0, 7, size=20000).tolist()
    planted = [PIECE - 6, 2 * PIECE - 1, 3 * PIECE - (n - 1), 4 * PIECE]
    for p in planted:
        long[p:p + n] = g
    rows = [[7, 8, 9], mixture(rng, ref, n, 90), long, g, [], mixture(rng, ref, n, 200)]
    want, first = check(tok, ref, n, rows)
    occur(want, first, ref, n)
    assert want["n_grams"][2] == 20000 - n + 1 and want["n_hits"][2] >= len(planted)
    cov = want["covered"][want["row_off"][2]:want["row_off"][3]]
    for p in planted:
        assert cov[p:p + n].all()
    assert first[tuple(g)] == 2 and want["first_ref"][3] == 2


def test_coverage_carry(tok):
    """hits at positions 63 and 64 (the carry from one trip into the next), a run of hits over a whole trip, hits exactly n apart
    (coverage abuts) and n + 1 apart (a gap of one token), a hit at the body's last n-gram (the tail is covered)"""
    n = 5
    g = [100, 101, 102, 103, 104]
    ref = [[9] * n, g, [9] * (n + 2)]

    def body(T, *plants):
        b = [(i * 7 + 3) % 6 for i in range(T)]                           # (holds no 9 and no id of g)
        for p, run in plants:
            b[p:p + len(run)] = run
        return b
    rows = [body(200, (63, g)), body(200, (64, g)), body(200, (63, [9] * (n + 1))), body(200, (64, [9] * (64 + n - 1))), [9] * 300,
            body(200, (20, g), (20 + n, g)), body(200, (20, g), (20 + n + 1, g)), body(200, (59, g), (59 + n + 1, g)), body(100, (100 - n, g)),
            body(64 + n - 1, (63, g)), body(128, (60, g)), body(70)]
    want, first = check(tok, ref, n, rows)
    occur(want, first, ref, n)
    assert want["n_hits"].tolist() == [1, 1, 2, 64, 296, 2, 2, 2, 1, 1, 1, 0]
    assert want["n_covered"].tolist() == [5, 5, 6, 68, 300, 10, 10, 10, 5, 5, 5, 0]
    assert want["first_hit"].tolist() == [63, 64, 63, 64, 0, 20, 20, 59, 95, 63, 60, -1]
    assert want["first_ref"].tolist() == [1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, -1]
    gap = want["covered"][want["row_off"][6]:want["row_off"][7]]
    assert gap[19:33].tolist() == [0] + [1] * 5 + [0] + [1] * 5 + [0, 0]


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_one_ngram_contends_for_one_slot(tok):
    n = 13
    ref = [[3] * 5000]
    want, first = check(tok, ref, n, [[3] * 40, [3] * 12, [3] * 13 + [4], [4] * 20, [2] + [3] * 13])
    assert len(first) == 1 and NO.positions(ref, n) == 5000 - n + 1
    assert want["n_hits"].tolist() == [28, 0, 1, 0, 1] and want["first_ref"].tolist() == [0, -1, 0, -1, 0]


def test_first_ref_follows_the_smallest_row(tok):
    n = 13
    rng = np.random.default_rng(21)
    g = list(range(200, 200 + n))
    rows = [rng.integers(0, 7, size=int(T)).tolist() for T in rng.integers(0, 90, size=10)]
    rows[7] = rows[7][:20] + g + rows[7][20:]
    rows[9] = g + rows[9] + g
    query = [[8, 8] + g + [8], g + g, rows[2][:40]]
    want, first = check(tok, rows, n, query)
    assert first[tuple(g)] == 7 and want["first_ref"][:2].tolist() == [7, 7]
    order = [0, 1, 2, 9, 4, 5, 6, 3, 8, 7]                                # the rows shuffled: g now in rows 3 and 9
    shuffled = [rows[i] for i in order]
    want, first = check(tok, shuffled, n, query)
    assert first[tuple(g)] == 3 and want["first_ref"][:2].tolist() == [3, 3]
    occur(want, first, shuffled, n)


def test_forced_collisions_change_nothing(tok):
    """about 300 distinct n-grams with only the low k bits of the hash kept: with k = 1 every probe starts in one of two slots with
    the same tag, and the result is the full hash's and the oracle's"""
    from genz_tokenize import _native
    n = 4
    rng = np.random.default_rng(13)
    ref = reference(rng, [70, 0, 140, 3, 170], n)
    rows = [mixture(rng, ref, n, int(T)) for T in (0, 3, 4, 70, 200, 64)]
    first = NO.index(ref, n)
    want = NO.overlap(first, n, rows)
    assert len(first) == 301 and NO.positions(ref, n) == 371
    occur(want, first, ref, n)
    results = {}
    try:
        for k in (0, 1, 4, 32):
            _native.debug_set("ngram_hash_bits", k, tok._ctx)
            with tok.ngram_index(ref, n, framed=False) as ix:
                assert ix.n_distinct == len(first) and ix.n_grams == NO.positions(ref, n)
                results[k] = tok.ngram_overlap_rows(rows, ix, framed=False, return_covered=True)
            same(results[k], want)
        with tok.ngram_index(ref, n, framed=False) as ix:                 # an index keeps the bits it was built with
            _native.debug_set("ngram_hash_bits", 0, tok._ctx)
            same(tok.ngram_overlap_rows(rows, ix, framed=False, return_covered=True), want)
    finally:
        _native.debug_set("ngram_hash_bits", 0, tok._ctx)
    for k in (1, 4, 32):
        for key in results[0]:
            assert np.array_equal(results[k][key], results[0][key]), (k, key)
    with pytest.raises(ValueError):
        _native.debug_set("ngram_hash_bits", 33, tok._ctx)


@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 4097])
def test_reference_positions_at_table_sizes(tok, P):
    """2 P at a power of two and beside it; the empty index answers no hit anywhere"""
    n = 3
    rng = np.random.default_rng(P)
    ref = [rng.integers(0, 7, size=P + n - 1).tolist()]
    rows = [mixture(rng, ref, n, int(T)) for T in (0, 2, 3, 50, 130)]
    want, first = check(tok, ref, n, rows)
    with tok.ngram_index(ref, n, framed=False) as ix:
        info = tok._ctx.ngram_index_info(ix._handle)
        slots = 1
        while slots < 2 * P:
            slots *= 2
        assert info["n_grams"] == P and info["slots"] == slots and info["device_bytes"] == ix.device_bytes >= 8 * slots + 4 * (P + n - 1) + 16
    if P == 0:
        assert not first and (want["n_hits"] == 0).all() and (want["first_hit"] == -1).all() and (want["first_ref"] == -1).all()
        assert (want["covered"] == 0).all()
        for empty in ([], [[]], [[1, 2], []]):                            # no rows; rows without n-grams
            w2, f2 = check(tok, empty, n, rows)
            assert not f2 and (w2["n_hits"] == 0).all()
    if P >= 255:
        occur(want, first, ref, n)


@pytest.mark.parametrize("N", [63, 64, 65, 257])
def test_reference_positions_summed_over_waves(tok, N):
    """The position total that sizes the table is a wave's sum of the rows' counts in 16-bit halves and one atomic a wave: N rows of
    about 5000 ids (64 of them carry out of the low half; 63, 65 and 257 rows leave partial waves and a partial block) and one row
    of 70 000 ids, whose own count has a high half.  A total that came out too small would size a table too small for its n-grams."""
    n = 5
    rng = np.random.default_rng(300 + N)
    ref = [rng.integers(0, 50000, size=int(T)).astype(np.int32) for T in rng.integers(4990, 5011, size=N)]
    ref.insert(N // 2, rng.integers(0, 50000, size=70000).astype(np.int32))
    P = NO.positions(ref, n)
    assert P == sum(len(b) - n + 1 for b in ref) > 64 * 4990
    slots = 1
    while slots < 2 * P:
        slots *= 2
    with tok.ngram_index(ref, n, framed=False) as ix:
        info = tok._ctx.ngram_index_info(ix._handle)
        assert info["n_grams"] == P and info["slots"] == slots and info["n_rows"] == N + 1 and info["n_ids"] == P + (N + 1) * (n - 1)
        got = tok.ngram_overlap_rows(ref, ix, framed=False)                # the reference against its own index: every position hits
    assert got["n_grams"].tolist() == [len(b) - n + 1 for b in ref]
    assert np.array_equal(got["n_hits"], got["n_grams"]) and np.array_equal(got["n_covered"], got["body_len"])
    assert (got["first_hit"] == 0).all() and (got["first_ref"] <= np.arange(N + 1)).all() and (got["first_ref"] >= 0).all()


@pytest.mark.parametrize("N", [511, 513, 2047, 2048, 2049, 4100])
def test_reference_row_counts_at_the_count_blocks_edges(tok, N):
    """Where the position total is asked for, a thread of the count pass takes 8 rows, 256 apart, so a block covers 2048 rows: one
    below, at and above a block, two blocks and a few rows, and row counts at which the threads of one block leave their loop after
    different numbers of rows.  Short rows, some shorter than n; the total, the distinct n-grams and every row's count are the
    oracle's, and the reference queried against its own index hits at every position."""
    n = 5
    rng = np.random.default_rng(500 + N)
    ref = [rng.integers(0, 50000, size=int(T)).astype(np.int32) for T in rng.integers(0, 61, size=N)]
    first = NO.index(ref, n)
    P = NO.positions(ref, n)
    slots = 1
    while slots < 2 * P:
        slots *= 2
    with tok.ngram_index(ref, n, framed=False) as ix:
        info = tok._ctx.ngram_index_info(ix._handle)
        assert (info["n_rows"], info["n_grams"], info["n_distinct"], info["slots"]) == (N, P, len(first), slots)
        got = tok.ngram_overlap_rows(ref, ix, framed=False)
    assert got["n_grams"].tolist() == [max(len(b) - n + 1, 0) for b in ref] and got["n_grams"].sum() == P
    assert np.array_equal(got["n_hits"], got["n_grams"]) and (got["n_grams"] == 0).any()


@pytest.mark.parametrize("N", [0, 1, 255, 256, 257])
def test_row_counts_at_block_edges(tok, N):
    n = 3
    rng = np.random.default_rng(100 + N)
    ref = reference(rng, [40, 60, 5], n)
    rows = [mixture(rng, ref, n, int(T)) for T in rng.integers(0, 40, size=N)]
    want, first = check(tok, ref, n, rows)
    assert all(want[k].shape == (N,) for k in NO.KEYS)
    if N > 1:
        occur(want, first, ref, n)


# ---- shapes of the call ---------------------------------------------------------------------------------------------------
def test_framed_against_bare_bodies(tok):
    n = 4
    rng = np.random.default_rng(31)
    ref = reference(rng, [0, 1, 3, 4, 5, 70], n)
    bodies = [mixture(rng, ref, n, T) for T in (0, 1, 3, 4, 5, 70, 130)]
    first = NO.index(ref, n)
    bare = NO.overlap(first, n, bodies)
    occur(bare, first, ref, n)
    framed_ref = [[-7] + b + [-9] for b in ref]                           # the frame is dropped whatever it holds
    framed = [[-7] + b + [-9] for b in bodies]
    with tok.ngram_index(framed_ref, n) as ix, tok.ngram_index(ref, n, framed=False) as ix_bare:      # framed is the default
        assert (ix.n_grams, ix.n_distinct) == (ix_bare.n_grams, ix_bare.n_distinct) and ix.n_ids == ix_bare.n_ids + 2 * len(ref)
        got = tok.ngram_overlap_rows(framed, ix, return_covered=True)
        same(got, NO.overlap(first, n, framed, framed=True))
        for k in NO.KEYS:
            assert np.array_equal(got[k], bare[k]), k
        for r, b in enumerate(bodies):                                    # the frame cells are 0, the body's cells the bare call's
            lo, hi = got["row_off"][r], got["row_off"][r + 1]
            assert got["covered"][lo] == 0 and got["covered"][hi - 1] == 0
            assert np.array_equal(got["covered"][lo + 1:hi - 1], bare["covered"][bare["row_off"][r]:bare["row_off"][r + 1]])
        same(tok.ngram_overlap_rows(bodies, ix, framed=False, return_covered=True), bare)     # the skips are the call's own
        short = tok.ngram_overlap_rows([[], [5], [5, 6], [5, 7, 6]], ix_bare, framed=True, return_covered=True)   # rows shorter than their frame
        same(short, NO.overlap(first, n, [[], [5], [5, 6], [5, 7, 6]], framed=True))
        assert short["body_len"].tolist() == [0, 0, 0, 1] and (short["covered"] == 0).all()
        rows = np.array([ref[5][:11], ref[5][20:31], [8] * 11], dtype=np.int64)       # a 2-D array of rows
        same(tok.ngram_overlap_rows(rows, ix_bare, return_covered=True), NO.overlap(first, n, rows.tolist(), framed=True))


def test_slices_equal_the_whole(tok):
    n = 5
    rng = np.random.default_rng(12)
    ref = reference(rng, [30, 100, 200], n)
    rows = [mixture(rng, ref, n, int(T)) for T in rng.integers(0, 150, size=90)] + [mixture(rng, ref, n, PIECE + 300)]
    with tok.ngram_index(ref, n, framed=False) as ix:
        whole = tok.ngram_overlap_rows(rows, ix, framed=False, return_covered=True)
        same(whole, NO.overlap(NO.index(ref, n), n, rows))
        for a, b in ((0, 91), (0, 1), (17, 64), (64, 91), (90, 91), (5, 5)):
            part = tok.ngram_overlap_rows(rows[a:b], ix, framed=False, return_covered=True)
            for k in NO.KEYS:
                assert np.array_equal(part[k], whole[k][a:b]), (k, a, b)
            assert np.array_equal(part["covered"], whole["covered"][whole["row_off"][a]:whole["row_off"][b]])
        cat = np.concatenate([tok.ngram_overlap_rows(rows[:40], ix, framed=False)["n_covered"], tok.ngram_overlap_rows(rows[40:], ix, framed=False)["n_covered"]])
        assert np.array_equal(cat, whole["n_covered"])


class Guarded:
    """n cells on the device between two runs of guard cells, all pre-filled with the bytes of FILL."""

    def __init__(self, ctx, n, guard=64, dtype=np.int32):
        self.ctx, self.n, self.guard, self.dtype = ctx, n, guard, np.dtype(dtype)
        self.fill = np.frombuffer(np.array([FILL], dtype=np.uint32).tobytes(), dtype=dtype)[0]
        self.base = ctx.alloc(self.dtype.itemsize * (n + 2 * guard) + 16)
        ctx.h2d(self.base, np.full(n + 2 * guard, self.fill, dtype=dtype))
        self.ptr = self.base + self.dtype.itemsize * guard

    def read(self):
        a = np.empty(self.n + 2 * self.guard, dtype=self.dtype)
        self.ctx.d2h(a, self.base)
        assert (a[:self.guard] == self.fill).all() and (a[self.guard + self.n:] == self.fill).all(), "guard cells were written"
        return a[self.guard:self.guard + self.n]

    def untouched(self):
        return (self.read() == self.fill).all()

    def free(self):
        self.ctx.free(self.base)


def test_device_form_behind_junk(tok):
    """Reference and query rows lie behind a prefix of junk (row_off_dev[0] != 0) and before a tail of it; outputs left out stay
    out; nothing outside the outputs is written; covered is laid out like the ids."""
    ctx = tok._ctx
    n = 6
    rng = np.random.default_rng(41)
    ref = reference(rng, [0, 30, 7, 90], n)
    bodies = [mixture(rng, ref, n, T) for T in (0, 3, 70, PIECE + 9, 0, 1, 130)]
    first = NO.index(ref, n)
    want = NO.overlap(first, n, bodies)
    occur(want, first, ref, n)

    def up(rows, junk):
        flat = np.array([-77] * junk + [v for b in rows for v in b] + [-88] * 5, dtype=np.int32)
        ro = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in rows], out=ro[1:])
        ro += junk
        d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
        ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
        return d_ids, d_ro, flat, ro
    N, junk = len(bodies), 37
    r_ids, r_ro, r_flat, _ = up(ref, 11)
    q_ids, q_ro, q_flat, ro = up(bodies, junk)
    g = [Guarded(ctx, N) for _ in OUT]
    g_cov = Guarded(ctx, len(q_flat), dtype=np.uint8)
    g_one = Guarded(ctx, N)
    index = ctx.ngram_index_build_device(r_ids, r_ro, len(ref), 0, 0, n)
    try:
        ctx.h2d(r_ids, np.full(len(r_flat), 3, dtype=np.int32))           # the index owns a copy: the caller's ids may change
        info = ctx.ngram_index_info(index)
        assert (info["n_rows"], info["n_ids"], info["n_grams"], info["n_distinct"]) == (len(ref), sum(map(len, ref)), NO.positions(ref, n), len(first))
        ctx.ngram_overlap_device(index, q_ids, q_ro, N, 0, 0, *[x.ptr for x in g], g_cov.ptr)
        for k, x in zip(OUT, g):
            assert np.array_equal(x.read(), want[k]), k
        cov = g_cov.read()
        fill8 = g_cov.fill
        assert (cov[:junk] == fill8).all() and (cov[int(ro[-1]):] == fill8).all()      # the junk's cells are nobody's
        assert np.array_equal(cov[junk:int(ro[-1])], want["covered"])
        ctx.ngram_overlap_device(index, q_ids, q_ro, N, 0, 0, 0, 0, 0, 0, g_one.ptr, 0)          # first_ref alone: first_hit from the workspace
        assert np.array_equal(g_one.read(), want["first_ref"])
        # with skips: the junk's last word and the first tail word are a frame nobody reads
        ctx.h2d(q_ro, np.array([junk - 1, int(ro[-1]) + 1], dtype=np.int64))
        ctx.ngram_overlap_device(index, q_ids, q_ro, 1, 1, 1, *[x.ptr for x in g], g_cov.ptr)
        one = NO.overlap(first, n, [[v for b in bodies for v in b]])
        for k, x in zip(OUT, g):
            assert x.read()[0] == one[k][0], k
        cov = g_cov.read()
        assert cov[junk - 1] == 0 and cov[int(ro[-1])] == 0 and np.array_equal(cov[junk:int(ro[-1])], one["covered"])
    finally:
        ctx.ngram_index_destroy(index)
        for x in g + [g_cov, g_one]:
            x.free()
        for d in (r_ids, r_ro, q_ids, q_ro):
            ctx.free(d)


def test_index_lifetime(tok):
    """the caller's reference arrays are overwritten after the build; two indexes live at once; back-to-back queries; close() gives
    the device bytes back (the context's count of live n-gram index bytes, as gz_ngram_index_info reports it)"""
    ctx = tok._ctx
    rng = np.random.default_rng(51)
    ref_a, ref_b = reference(rng, [50, 90], 4), reference(rng, [300, 20, 64], 7)
    rows = [mixture(rng, ref_a + ref_b, 7, int(T)) for T in (0, 5, 64, 200, PIECE + 40)]
    want_a, want_b = NO.overlap(NO.index(ref_a, 4), 4, rows), NO.overlap(NO.index(ref_b, 7), 7, rows)
    occur(want_a, NO.index(ref_a, 4), ref_a, 4)
    occur(want_b, NO.index(ref_b, 7), ref_b, 7)
    arr = np.array([ref_a[0][:40], ref_a[1][:40]], dtype=np.int32)        # a caller's own array
    want_arr = NO.overlap(NO.index(arr.tolist(), 4), 4, rows)
    keeper = tok.ngram_index([[1, 2, 3, 4, 5]], 4, framed=False)          # (lives through the test: its info reads the context's count)
    base = ctx.ngram_index_info(keeper._handle)["context_bytes"]
    ix_arr = tok.ngram_index(arr, 4, framed=False)
    arr[:] = 5
    a = tok.ngram_index(ref_a, 4, framed=False)
    b = tok.ngram_index(ref_b, 7, framed=False)
    assert ctx.ngram_index_info(keeper._handle)["context_bytes"] == base + ix_arr.device_bytes + a.device_bytes + b.device_bytes
    for _ in range(2):                                                    # back to back, the two indexes in turn
        same(tok.ngram_overlap_rows(rows, a, framed=False, return_covered=True), want_a)
        same(tok.ngram_overlap_rows(rows, b, framed=False, return_covered=True), want_b)
        same(tok.ngram_overlap_rows(rows, ix_arr, framed=False, return_covered=True), want_arr)
    a.close()
    assert a.closed and ctx.ngram_index_info(keeper._handle)["context_bytes"] == base + ix_arr.device_bytes + b.device_bytes
    with pytest.raises(ValueError):
        tok.ngram_overlap_rows(rows, a, framed=False)
    same(tok.ngram_overlap_rows(rows, b, framed=False, return_covered=True), want_b)
    b.close(); ix_arr.close()
    assert ctx.ngram_index_info(keeper._handle)["context_bytes"] == base == keeper.device_bytes
    twin = tok.ngram_index(ref_b, 7, framed=False)                        # the same build takes the same bytes
    assert twin.device_bytes == b.device_bytes
    del twin
    import gc
    gc.collect()                                                          # garbage collection frees it too
    assert ctx.ngram_index_info(keeper._handle)["context_bytes"] == base
    keeper.close()
    from genz_tokenize import Tokenize
    other = Tokenize()
    with tok.ngram_index(ref_a, 4, framed=False) as ix, pytest.raises(ValueError, match="another Tokenize"):
        other.ngram_overlap_rows(rows, ix, framed=False)


def test_a_bare_context_is_enough():
    """neither the build nor the query needs the tables or the decoder snapshot"""
    from genz_tokenize import _native
    ctx = _native.Context()
    try:
        ref, n = [[1, 2, 3, 4, 5], [], [3, 4, 5, 6]], 3
        bodies = [[0, 2, 3, 4, 9], [], [4, 5, 6, 4, 5, 6], [1, 2]]
        flat = np.array([v for b in ref for v in b], dtype=np.int32)
        off = np.array([0, 5, 5, 9], dtype=np.int64)
        index = ctx.ngram_index_build(flat, off, n, False)
        q = np.array([v for b in bodies for v in b], dtype=np.int32)
        qo = np.array([0, 5, 5, 11, 13], dtype=np.int64)
        got = ctx.ngram_overlap(index, q, qo, False, True)
        want = NO.overlap(NO.index(ref, n), n, bodies)
        for k in OUT + ("covered",):
            assert np.array_equal(got[k], want[k]), k
        assert want["n_hits"].tolist() == [1, 0, 2, 0] and want["first_ref"].tolist() == [0, -1, 2, -1]
        left = ctx.ngram_index_build(flat, off, n, False)                 # an index nobody destroys goes with its context
        assert ctx.ngram_index_info(left)["context_bytes"] == 2 * ctx.ngram_index_info(index)["device_bytes"]
        ctx.ngram_index_destroy(index)
    finally:
        ctx.close()


# ---- texts, end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tok):
    """(reference texts, corpus texts, their rows, the 20 documents that quote a reference document)"""
    r = random.Random(7)
    refs = [" ".join(r.choice(WO.WORDS) for _ in range(r.randint(20, 40))) for _ in range(10)] + ["", "xin chào"]
    texts = WO.texts(200, 60, 9)
    planted = sorted(r.sample(range(200), 20))
    for i in planted:
        words = texts[i].split(" ") if texts[i] else []
        k = r.randint(0, len(words))
        texts[i] = " ".join(words[:k] + [refs[r.randrange(10)]] + words[k:])

    def rows_of(ts):
        e = tok.encode_batch(ts, max_len=None)
        ro = e["row_off"]
        return [e["input_ids"][ro[i]:ro[i + 1]].tolist() for i in range(len(ts))]
    return refs, texts, rows_of(refs), rows_of(texts), planted


def test_text_end_to_end(tok, corpus):
    refs, texts, ref_rows, rows, planted = corpus
    n = 13
    first = NO.index(ref_rows, n, framed=True)
    want = NO.overlap(first, n, rows, framed=True)
    hit_docs = np.flatnonzero(want["n_hits"]).tolist()                    # the planted ones (and whatever random text shares by chance)
    assert set(planted) <= set(hit_docs) and len(hit_docs) < 40 and (want["n_grams"] == 0).any()
    with tok.encode_ngram_index(refs) as ix, tok.ngram_index(ref_rows) as ix_rows:        # n = 13 is the default
        assert (ix.n, ix.n_rows, ix.n_ids, ix.n_grams, ix.n_distinct) == (13, len(refs), sum(map(len, ref_rows)), NO.positions(ref_rows, n, True), len(first))
        assert (ix_rows.n_grams, ix_rows.n_distinct, ix_rows.n_ids) == (ix.n_grams, ix.n_distinct, ix.n_ids)
        got = tok.encode_ngram_overlap(texts, ix)
        same(got, want, covered=False)
        same(tok.encode_ngram_overlap(texts, ix_rows, word_table=False), want, covered=False)
        same(tok.ngram_overlap_rows(rows, ix, return_covered=True), want)
        part = tok.encode_ngram_overlap(texts[40:90], ix)
        for k in NO.KEYS:
            assert np.array_equal(part[k], want[k][40:90]), k
        # the decision
        clean = tok.decontaminate(texts, ix)
        same({k: clean[k] for k in NO.KEYS}, want, covered=False)
        assert clean["keep"].dtype == bool and clean["fraction"].dtype == np.float64 and sorted(clean) == sorted(NO.KEYS + ("fraction", "keep"))
        assert np.array_equal(clean["keep"], want["n_hits"] == 0) and int((~clean["keep"]).sum()) == len(hit_docs)
        assert np.array_equal(clean["fraction"], want["n_covered"] / np.maximum(want["body_len"], 1))
        share = np.unique(clean["fraction"][hit_docs])
        assert len(share) >= 4
        cut = float((share[len(share) // 2 - 1] + share[len(share) // 2]) / 2)       # between two documents' shares: some go, some stay
        some = tok.decontaminate(texts, ix, max_fraction=cut)
        assert np.array_equal(some["keep"], want["n_covered"] <= cut * want["body_len"])
        assert 200 - len(hit_docs) < int(some["keep"].sum()) < 200
        assert tok.decontaminate(texts, ix, 1.0)["keep"].all() and tok.decontaminate(texts, ix, 1)["keep"].all()
        for empty in ([], [""], ["", "   "]):
            got = tok.decontaminate(empty, ix)
            assert all(got[k].shape == (len(empty),) for k in got) and got["keep"].all() and (got["first_hit"] == -1).all()
    with tok.encode_ngram_index([], 5) as none, tok.encode_ngram_index(["", " "], 5) as blank:
        assert (none.n_rows, none.n_grams, blank.n_rows, blank.n_grams) == (0, 0, 2, 0)
        assert (tok.encode_ngram_overlap(texts[:30], none)["n_hits"] == 0).all() and (tok.encode_ngram_overlap(texts[:30], blank)["n_hits"] == 0).all()
    # the roles swapped: which reference documents leaked
    with tok.encode_ngram_index(texts) as shard:
        leaked = tok.encode_ngram_overlap(refs, shard)
        same(leaked, NO.overlap(NO.index(rows, n, framed=True), n, ref_rows, framed=True), covered=False)
        assert (leaked["n_hits"][:10] > 0).sum() >= 5 and (leaked["n_hits"][10:] == 0).all()


# ---- refusals at the ABI ----------------------------------------------------------------------------------------------------
def test_refusals_of_the_build_calls(tok):
    from genz_tokenize import _native
    ctx, lib, P, vp = tok._ctx, tok._ctx.lib, _native._ptr, ctypes.c_void_p
    h, INV = ctx.handle, _native.GZ_E_INVALID
    ids = np.arange(10, dtype=np.int32)
    ro = np.array([0, 4, 10], dtype=np.int64)
    d_ids, d_ro = ctx.alloc(64), ctx.alloc(64)
    said = set()

    def refused(call, device=True):
        out = vp(0xDEAD)
        assert call(lib.gz_ngram_index_build, P(ids), P(ro), ctypes.byref(out)) == INV
        said.add(lib.gz_last_error(h))
        assert out.value == 0xDEAD
        if device:
            assert call(lib.gz_ngram_index_build_device, vp(d_ids), vp(d_ro), ctypes.byref(out)) == INV
            assert lib.gz_last_error(h) in said and out.value == 0xDEAD
    try:
        ctx.h2d(d_ids, ids); ctx.h2d(d_ro, ro)
        refused(lambda f, i, o, out: f(h, i, o, -1, 0, 0, 13, out))
        refused(lambda f, i, o, out: f(h, i, o, 2 ** 31, 0, 0, 13, out))
        for sf, sb in ((2, 0), (0, 2), (-1, 0), (0, -1)):
            refused(lambda f, i, o, out: f(h, i, o, 2, sf, sb, 13, out))
        for n in (0, 33, -1):
            refused(lambda f, i, o, out: f(h, i, o, 2, 0, 0, n, out))
        refused(lambda f, i, o, out: f(h, i, o, 2, 0, 0, 13, None))
        refused(lambda f, i, o, out: f(h, i, None, 2, 0, 0, 13, out))
        assert len(said) == 6                                             # each rule has its own sentence
        refused(lambda f, i, o, out: f(h, None, o, 2, 0, 0, 13, out))
        assert len(said) == 6                                             # (ids and row_off share theirs)
        out = vp(0xDEAD)
        for bad, words in ((np.array([0, 7, 4], dtype=np.int64), b"row offsets must not decrease"), (np.array([5, 6, 2], dtype=np.int64), b"bad row offsets")):
            assert lib.gz_ngram_index_build(h, P(ids), P(bad), 2, 0, 0, 13, ctypes.byref(out)) == INV
            assert words in lib.gz_last_error(h) and out.value == 0xDEAD
        assert lib.gz_ngram_index_build(None, P(ids), P(ro), 2, 0, 0, 13, ctypes.byref(out)) == INV
        assert lib.gz_ngram_index_info(None, P(np.zeros(8, dtype=np.int64))) == INV
        lib.gz_ngram_index_destroy(None)                                  # nothing to free is fine
        # no rows is no error: the empty index, from no pointers at all
        for f in (lib.gz_ngram_index_build, lib.gz_ngram_index_build_device):
            out = vp()
            assert f(h, None, None, 0, 1, 1, 13, ctypes.byref(out)) == _native.GZ_OK and out.value
            assert ctx.ngram_index_info(out.value)["n_grams"] == 0 and lib.gz_ngram_index_info(out, None) == INV
            ctx.ngram_index_destroy(out.value)
    finally:
        ctx.free(d_ids); ctx.free(d_ro)
    check(tok, [[1, 2, 3, 4]], 2, [[2, 3], [9]])                           # the context is usable afterwards


def test_refusals_of_the_overlap_calls(tok):
    from genz_tokenize import _native
    ctx, lib, P, vp = tok._ctx, tok._ctx.lib, _native._ptr, ctypes.c_void_p
    h, INV = ctx.handle, _native.GZ_E_INVALID
    ids = np.arange(10, dtype=np.int32)
    ro = np.array([0, 4, 10], dtype=np.int64)
    d_ids, d_ro = ctx.alloc(64), ctx.alloc(64)
    g = [Guarded(ctx, 2) for _ in OUT]
    g_cov = Guarded(ctx, 10, dtype=np.uint8)
    index = vp(ctx.ngram_index_build(ids, ro, 3, False))
    other = _native.Context()
    said = set()

    def refused(call, device=True):
        out = [np.full(2, FILL, dtype=np.int32) for _ in OUT]
        cov = np.full(10, 0x5A, dtype=np.uint8)
        assert call(lib.gz_ngram_overlap, P(ids), P(ro), [P(a) for a in out], P(cov)) == INV
        said.add(lib.gz_last_error(h))
        assert all((a == FILL).all() for a in out) and (cov == 0x5A).all()
        if device:
            assert call(lib.gz_ngram_overlap_device, vp(d_ids), vp(d_ro), [vp(x.ptr) for x in g], vp(g_cov.ptr)) == INV
            assert lib.gz_last_error(h) in said
            assert all(x.untouched() for x in g) and g_cov.untouched()
    try:
        ctx.h2d(d_ids, ids); ctx.h2d(d_ro, ro)
        refused(lambda f, i, o, a, c: f(h, index, i, o, -1, 0, 0, *a, c))
        for sf, sb in ((2, 0), (0, 2), (-1, 0), (0, -1)):
            refused(lambda f, i, o, a, c: f(h, index, i, o, 2, sf, sb, *a, c))
        refused(lambda f, i, o, a, c: f(h, None, i, o, 2, 0, 0, *a, c))
        refused(lambda f, i, o, a, c: f(h, index, i, None, 2, 0, 0, *a, c))
        refused(lambda f, i, o, a, c: f(h, index, i, o, 2, 0, 0, a[0], a[0], a[2], a[3], a[4], c))       # two outputs in one array
        assert len(said) == 5                                             # each rule has its own sentence
        refused(lambda f, i, o, a, c: f(h, index, None, o, 2, 0, 0, *a, c))
        refused(lambda f, i, o, a, c: f(h, index, i, o, 2, 0, 0, i, a[1], a[2], a[3], a[4], c))          # an output over the ids
        refused(lambda f, i, o, a, c: f(h, index, i, o, 2, 0, 0, a[0], a[1], a[2], a[3], o, c))          # an output over the offsets
        refused(lambda f, i, o, a, c: f(h, index, i, o, 2, 0, 0, *a, i), device=False)                   # covered over the ids
        assert len(said) == 5
        # an index of another context
        out = [np.full(2, FILL, dtype=np.int32) for _ in OUT]
        assert lib.gz_ngram_overlap(other.handle, index, P(ids), P(ro), 2, 0, 0, *[P(a) for a in out], None) == INV
        assert b"another context" in lib.gz_last_error(other.handle) and all((a == FILL).all() for a in out)
        assert lib.gz_ngram_overlap_device(other.handle, index, vp(d_ids), vp(d_ro), 2, 0, 0, *[vp(x.ptr) for x in g], None) == INV
        assert b"another context" in lib.gz_last_error(other.handle) and all(x.untouched() for x in g)
        # the host form's own: offsets
        for bad, words in ((np.array([0, 7, 4], dtype=np.int64), b"row offsets must not decrease"), (np.array([5, 6, 2], dtype=np.int64), b"bad row offsets")):
            assert lib.gz_ngram_overlap(h, index, P(ids), P(bad), 2, 0, 0, *[P(a) for a in out], None) == INV
            assert words in lib.gz_last_error(h) and all((a == FILL).all() for a in out)
        # nothing to do is no error: nothing is written, no pointer is needed
        assert lib.gz_ngram_overlap(h, index, None, None, 0, 0, 0, None, None, None, None, None, None) == _native.GZ_OK
        assert lib.gz_ngram_overlap_device(h, index, None, None, 0, 1, 1, None, None, None, None, None, None) == _native.GZ_OK
        assert lib.gz_ngram_overlap(None, index, P(ids), P(ro), 2, 0, 0, *[P(a) for a in out], None) == INV
        # every output may be left out
        assert lib.gz_ngram_overlap(h, index, P(ids), P(ro), 2, 0, 0, None, None, None, None, None, None) == _native.GZ_OK
        assert lib.gz_ngram_overlap(h, index, P(ids), P(ro), 2, 0, 0, None, P(out[1]), None, None, None, None) == _native.GZ_OK
        assert out[1].tolist() == [2, 4] and (out[0] == FILL).all()
    finally:
        ctx.ngram_index_destroy(index.value)
        other.close()
        for x in g + [g_cov]:
            x.free()
        ctx.free(d_ids); ctx.free(d_ro)
    check(tok, [[1, 2, 3, 4]], 2, [[2, 3], [9]])                           # the context is usable afterwards
