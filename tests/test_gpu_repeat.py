"""n-gram repetition inside a document on the GPU (gz_ngram_repeats / _device; Tokenize.repetition_rows, encode_repetition,
repetition_filter) against the rule of tests/repeat_oracle.py -- collections.Counter over tuples, no hash --, which
tests/test_repeat_inputs.py ties to answers worked by hand.  Every comparison is exact, on all six [K, N] arrays, body_len and the
covered bits."""
import ctypes
import random

import numpy as np
import pytest

import repeat_oracle as RO
import window_oracle as WO

pytestmark = pytest.mark.gpu

PIECE = 4096                                                             # n-gram positions a wave takes (csrc/gz_pieces.inc: GZ_PIECE)
FILL = 0x5A5A5A5A
OUT = RO.KEYS


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


def same(got, want, covered=True):
    keys = OUT + ("body_len",) + (("covered", "row_off") if covered else ())
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    assert sorted(got) == sorted(keys + ("widths",))


def check(tok, rows, widths, framed=False):
    """the call, with and without covered, against the oracle; the oracle's result"""
    want = RO.repetition(rows, widths, framed)
    got = tok.repetition_rows(rows, widths, framed=framed, return_covered=True)
    assert got["widths"] == tuple(widths)
    same(got, want)
    same(tok.repetition_rows(rows, widths, framed=framed), want, covered=False)
    return want


def looped(rng, T, n, alphabet=3):
    """A body of T ids over a small alphabet in which runs of n ids or more are copied from earlier in the same body: repeats and
    ties at every width"""
    b = rng.integers(0, alphabet, size=T).tolist()
    at = n
    while at + n <= T:
        k = int(rng.integers(n, min(3 * n, T - at) + 1))
        src = int(rng.integers(0, at))
        b[at:at + k] = b[src:src + k]                                     # (src + k may reach beyond `at`: the copy then repeats itself)
        at += k + int(rng.integers(0, 2 * n + 3))
    return b[:T]


def distinct(rng, T):
    """T different ids out of 2^20: no n-gram occurs twice"""
    return rng.choice(2 ** 20, size=T, replace=False).tolist()


def plain(T, base=1000):
    return list(range(base, base + T))                                    # different ids: the background of the planted cases


def planted(T, *plants):
    b = plain(T)
    for p, run in plants:
        assert 0 <= p and p + len(run) <= T
        b[p:p + len(run)] = run
    return b


# ---- the rule's edges, the trips' and the pieces' ------------------------------------------------------------------------
def test_piece_workspace_shared_with_minhash_and_overlap(tok):
    """MinHash signatures, the n-gram index, its queries and this call count their pieces into ONE workspace buffer of the context.
    Five calls on one context whose row counts grow and shrink and whose long rows follow short ones, each against its own oracle:
    offsets left over from an earlier call, or a buffer too small for a later one, would show."""
    import minhash_oracle as MO
    import ngram_oracle as NO
    rng = np.random.default_rng(77)

    def signed(bodies):
        want = MO.batch(bodies, 64, 5, 9)
        got = tok.minhash_rows(bodies, 64, 5, 9, framed=False)
        assert np.array_equal(got["signatures"], want["signatures"]) and np.array_equal(got["n_shingles"], want["n_shingles"])
    signed([rng.integers(5, 48423, size=int(T)).tolist() for T in rng.integers(0, 60, size=300)])
    n = 4
    ref = [rng.integers(0, 7, size=T).tolist() for T in (40, 0, 90, 3, 200)]
    first = NO.index(ref, n)
    with tok.ngram_index(ref, n, framed=False) as ix:
        assert (ix.n_rows, ix.n_grams, ix.n_distinct) == (5, NO.positions(ref, n), len(first))
        check(tok, [looped(rng, int(T), 3) for T in rng.integers(0, 41, size=4097)] + [looped(rng, PIECE + 9, 3)], (2, 5))
        rows = [rng.integers(0, 7, size=2 * PIECE + 12).tolist()]
        want = NO.overlap(first, n, rows)
        got = tok.ngram_overlap_rows(rows, ix, framed=False, return_covered=True)
        assert want["n_hits"][0] > 0
        for k in NO.KEYS + ("covered", "row_off"):
            assert np.array_equal(got[k], want[k]), k
    signed([[7, 8, 9], rng.integers(5, 48423, size=PIECE + 70).tolist(), []])


@pytest.mark.parametrize("n", [1, 2, 13, 32])
def test_body_lengths_at_the_rules_the_trips_and_the_pieces_edges(tok, n):
    """nothing, one id, around the width; around one trip of 64 positions; exactly one piece and two pieces -- over an alphabet of
    3 (repeats and ties everywhere) and of 2^20 (none)"""
    rng = np.random.default_rng(n)
    lengths = sorted({0, 1, max(n - 1, 0), n, n + 1, 63, 64, 65, 64 + n - 1, PIECE + n - 1, PIECE + n})
    some = check(tok, [looped(rng, T, n) for T in lengths], [n])
    none = check(tok, [distinct(rng, T) for T in lengths], [n])
    assert some["n_grams"][0].tolist() == [max(T - n + 1, 0) for T in lengths] == none["n_grams"][0].tolist()
    # both kinds of outcome occur
    long = some["n_grams"][0] >= 2 * n + 32
    assert (some["n_repeated"][0][long] > 0).all() and (some["top_count"][0][long] >= 2).all()
    assert (some["n_distinct"][0] < some["n_grams"][0]).any()
    if n >= 13:                                                           # (at widths 1 and 2 an alphabet of 3 repeats everywhere)
        assert (some["n_covered"][0][long] < some["body_len"][long]).all() and (some["n_repeated"][0][long] < some["n_grams"][0][long]).all()
    assert (none["n_repeated"][0] == 0).all() and (none["n_covered"][0] == 0).all() and (none["covered"] == 0).all()
    assert np.array_equal(none["n_distinct"], none["n_grams"]) and set(none["top_count"][0].tolist()) == {0, 1}
    assert set(none["top_pos"][0].tolist()) == {-1, 0}
    for T in (0, 1, n, PIECE + n - 1, PIECE + n):                         # ... and as batches of their own
        check(tok, [looped(rng, T, n)], [n])


def test_pieces_are_those_of_the_smallest_width(tok):
    """a row's pieces are cut at the call's smallest width: at a larger width a piece's last positions, or the whole last piece, lie
    beyond the last n-gram and are tail tokens"""
    rng = np.random.default_rng(77)
    for widths in ((2, 13, 32), (32, 1, 9), (13, 12)):
        lengths = [PIECE + 1, PIECE + 5, PIECE + 31, PIECE + 32, PIECE + 33, 2 * PIECE + 12, 2 * PIECE + 40, 70, 0]
        rows = [looped(rng, T, 32) for T in lengths]
        g = list(range(50, 82))                                           # a repeat that ends on the body's last token, at every width
        rows.append(planted(PIECE + 20, (10, g), (PIECE + 20 - 32, g)))
        want = check(tok, rows, widths)
        assert (want["n_repeated"][:, :7] > 0).all()
        for k, n in enumerate(widths):
            assert want["n_repeated"][k, -1] == 2 * (32 - n + 1) and want["n_covered"][k, -1] == 64


def test_one_long_body_between_short_ones(tok):
    """A body of five pieces between short ones.  Repeated n-grams are planted across a piece boundary, with their two occurrences in
    different pieces, on a piece's last and first position, and in the reach of the last n - 1 tail tokens."""
    n = 13
    T = 4 * PIECE + 3000
    g = [list(range(100 * (i + 1), 100 * (i + 1) + n)) for i in range(4)]
    long = planted(T,
                   (PIECE - 6, g[0]), (50, g[0]),                         # across a boundary; its twin in the same piece
                   (100, g[1]), (3 * PIECE + 50, g[1]),                   # the two occurrences in different pieces
                   (2 * PIECE - 1, g[2]), (3 * PIECE, g[2]),              # starts on a piece's last position / on a piece's first
                   (T - n, g[3]), (4 * PIECE - (n - 1), g[3]))            # the body's last n-gram: the tail; the farthest look-back
    rng = np.random.default_rng(8)
    rows = [[7, 8, 9], looped(rng, 90, n), long, g[0], [], looped(rng, 200, n)]
    for widths in ((n,), (n, 5), (20, n, 14)):
        want = check(tok, rows, widths)
        k = widths.index(n)
        assert want["n_grams"][k, 2] == T - n + 1 and want["n_repeated"][k, 2] == 8 and want["n_covered"][k, 2] == 8 * n
        assert want["n_distinct"][k, 2] == T - n + 1 - 4 and want["top_count"][k, 2] == 2 and want["top_pos"][k, 2] == 50
        cov = want["covered"][want["row_off"][2]:want["row_off"][3]] >> k & 1
        for p in (PIECE - 6, 50, 100, 3 * PIECE + 50, 2 * PIECE - 1, 3 * PIECE, T - n, 4 * PIECE - (n - 1)):
            assert cov[p:p + n].all() and not cov[p - 1] and (p + n == T or not cov[p + n])
        assert want["n_repeated"][k, 3] == 0                              # g[0] alone in its row: the neighbour's copies do not count


def test_coverage_carry(tok):
    """repeats at positions 63 and 64 (the carry from one trip into the next), a whole trip of repeated positions, repeats exactly n
    apart (coverage abuts) and n + 1 apart (a gap of one token), a repeat at the body's last n-gram (the tail is covered)"""
    n = 5
    g = [100, 101, 102, 103, 104]
    rows = [planted(200, (63, g), (150, g)), planted(200, (64, g), (150, g)), planted(200, (63, [9] * (n + 1))),
            planted(200, (64, [9] * (64 + n - 1))), [9] * 300, planted(200, (20, g), (20 + n, g)), planted(200, (20, g), (20 + n + 1, g)),
            planted(200, (59, g), (59 + n + 1, g)), planted(100, (100 - n, g), (10, g)), planted(64 + n - 1, (63, g), (3, g)),
            planted(128, (60, g), (123, g)), plain(70)]
    want = check(tok, rows, [n])
    assert want["n_repeated"][0].tolist() == [2, 2, 2, 64, 296, 2, 2, 2, 2, 2, 2, 0]
    assert want["n_covered"][0].tolist() == [10, 10, 6, 68, 300, 10, 10, 10, 10, 10, 10, 0]
    assert want["top_count"][0].tolist() == [2, 2, 2, 64, 296, 2, 2, 2, 2, 2, 2, 1]
    assert want["top_pos"][0].tolist() == [63, 64, 63, 64, 0, 20, 20, 59, 10, 3, 60, 0]
    gap = want["covered"][want["row_off"][6]:want["row_off"][7]]
    assert gap[19:33].tolist() == [0] + [1] * 5 + [0] + [1] * 5 + [0, 0]
    check(tok, rows, [n, 1, 2 * n, 64 - 32])                              # the same rows at widths whose carries differ


# ---- the table ----------------------------------------------------------------------------------------------------------
class hash_bits:
    """the switch repeat_hash_bits on the object's context; back to 0 on the way out"""

    def __init__(self, tok, k):
        self.ctx, self.k = tok._ctx, k

    def __enter__(self):
        from genz_tokenize import _native
        _native.debug_set("repeat_hash_bits", self.k, self.ctx)

    def __exit__(self, *exc):
        from genz_tokenize import _native
        _native.debug_set("repeat_hash_bits", 0, self.ctx)


@pytest.mark.parametrize("bits", [1, 4, 0])
def test_the_same_ngram_once_in_each_of_many_rows_counts_nowhere(tok, bits):
    """identical adjacent rows and identical rows far apart: a key is (row, n-gram), and neither the hash nor a forced collision of
    every probe (bits = 1: two start slots, one tag) makes two rows one"""
    n = 3
    rng = np.random.default_rng(bits)
    a = plain(n + 2, 10)                                                  # three positions, all different
    adjacent = [list(a) for _ in range(100)]                              # 300 positions
    far = [list(a)] + [distinct(rng, n + 1) for _ in range(90)] + [list(a)] + [distinct(rng, n + 1) for _ in range(20)] + [list(a)]
    mixed = [looped(rng, int(T), n) for T in (0, 2, 3, 40, 70, 64)] + [list(a), [5, 5, 5, 5], list(a)]
    with hash_bits(tok, bits):
        for rows in (adjacent, far):
            want = check(tok, rows, [n])
            assert (want["n_repeated"] == 0).all() and (want["top_count"] == 1).all() and (want["top_pos"] == 0).all()
            assert np.array_equal(want["n_distinct"], want["n_grams"]) and (want["covered"] == 0).all()
        want = check(tok, mixed, [n, 2])                                  # ... and repeats inside a row still count, ties too
        assert (want["n_repeated"][0, 3:6] > 0).all() and want["n_repeated"][0, 6:].tolist() == [0, 2, 0]
    from genz_tokenize import _native
    with pytest.raises(ValueError):
        _native.debug_set("repeat_hash_bits", 33, tok._ctx)


@pytest.mark.parametrize("n", [1, 13])
def test_one_key_under_contention(tok, n):
    """a constant row: one key, 5 000 occurrences in two pieces, every one of them ending in the same slot"""
    want = check(tok, [[3] * (5000 + n - 1), [3] * (n + 1), [4] * 40], [n])
    assert want["top_count"][0].tolist() == [5000, 2, 40 - n + 1] and want["top_pos"][0].tolist() == [0, 0, 0]
    assert want["n_distinct"][0].tolist() == [1, 1, 1] and want["n_repeated"][0].tolist() == [5000, 2, 40 - n + 1]
    assert want["n_covered"][0].tolist() == [5000 + n - 1, n + 1, 40]


def test_top_ties_go_to_the_smallest_first_position(tok):
    n = 4
    g1, g2, g3 = [1, 2, 3, 4], [5, 6, 7, 8], [9, 9, 8, 7]
    T = 2 * PIECE + 500
    rows = [planted(T, (500, g1), (900, g1), (5000, g2), (6000, g2)),             # a tie, its n-grams in different pieces: the earlier piece's
            planted(T, (5000, g1), (6000, g1), (500, g2), (900, g2)),             # ... whichever n-gram that is
            planted(T, (4000, g1), (2 * PIECE + 100, g1), (4500, g2), (4600, g2)),     # the first position decides, not the last
            planted(T, (100, g1), (200, g1), (5000, g2), (6000, g2), (2 * PIECE + 10, g2)),    # three beat two, wherever they stand
            planted(200, (150, g1), (160, g1), (20, g2), (90, g2), (40, g3), (60, g3)),        # one piece, three n-grams tie
            [1, 2, 1, 2, 1], [4, 9, 9, 4, 9, 9], plain(30)]
    want = check(tok, rows, [n, 1, 2])
    assert want["top_count"][0].tolist() == [2, 2, 2, 3, 2, 1, 1, 1] and want["top_pos"][0].tolist() == [500, 500, 4000, 5000, 20, 0, 0, 0]
    assert want["top_count"][1, 5:7].tolist() == [3, 4] and want["top_pos"][1, 5:7].tolist() == [0, 1]      # the rule's own table
    assert want["top_count"][2, 5:7].tolist() == [2, 2] and want["top_pos"][2, 5:7].tolist() == [0, 0]


@pytest.mark.parametrize("widths", [(7,), (2, 3, 4, 5, 6, 7, 8, 9, 10), (9, 3, 32, 1, 17, 2, 30, 4, 11, 5, 6, 31, 7, 8, 10, 16), (10, 2, 6)])
def test_widths_one_nine_sixteen_in_any_order(tok, widths):
    rng = np.random.default_rng(len(widths))
    rows = [looped(rng, int(T), max(widths)) for T in (0, 1, 5, 40, 64, 130, 300, PIECE + 77)] + [distinct(rng, 50)]
    want = check(tok, rows, widths)
    if len(widths) == 9:
        got = tok.repetition_rows(rows, framed=False, return_covered=True)        # nine widths are the default
        same(got, want)
    assert want["n_repeated"][:, 5:8].all()
    for k, n in enumerate(widths):                                        # bit k belongs to widths[k]
        alone = tok.repetition_rows(rows, [n], framed=False, return_covered=True)
        assert np.array_equal(alone["covered"], want["covered"] >> k & 1)
        for key in OUT:
            assert np.array_equal(alone[key][0], want[key][k]), (key, n)
    assert (want["covered"] >> len(widths) == 0).all()


@pytest.mark.parametrize("N", [0, 1, 255, 256, 257])
def test_row_counts_at_block_edges(tok, N):
    rng = np.random.default_rng(100 + N)
    rows = [looped(rng, int(T), 3) for T in rng.integers(0, 40, size=N)]
    want = check(tok, rows, [3, 2])
    assert all(want[k].shape == (2, N) for k in OUT) and want["body_len"].shape == (N,)
    if N > 1:
        assert (want["n_repeated"] > 0).any() and (want["n_repeated"] == 0).any()


@pytest.mark.parametrize("P", [0, 1, 127, 128, 129, 255, 256, 257, 4097])
def test_positions_at_table_sizes(tok, P):
    """2 P at a power of two and beside it, in one row and spread over rows; no position at all"""
    n = 3
    rng = np.random.default_rng(P)
    want = check(tok, [looped(rng, P + n - 1 if P else 0, n)], [n, 5])
    assert want["n_grams"][0, 0] == P
    parts = [P // 3, P // 3, P - 2 * (P // 3)]
    want = check(tok, [looped(rng, p + n - 1 if p else 1, n) for p in parts], [n])
    assert want["n_grams"].sum() == P
    if P == 0:
        for empty in ([[]], [[1, 2], []], [[], [], [3]]):
            want = check(tok, empty, [n, 4])
            assert (want["n_grams"] == 0).all() and (want["top_count"] == 0).all() and (want["top_pos"] == -1).all()


# ---- shapes of the call ---------------------------------------------------------------------------------------------------
def test_framed_against_bare_bodies(tok):
    widths = (4, 2)
    rng = np.random.default_rng(31)
    bodies = [looped(rng, T, 4) for T in (0, 1, 3, 4, 5, 70, 130)]
    bare = check(tok, bodies, widths)
    framed = [[-7] + b + [-9] for b in bodies]                            # the frame is dropped whatever it holds
    got = tok.repetition_rows(framed, widths, return_covered=True)        # framed is the default
    same(got, RO.repetition(framed, widths, framed=True))
    for k in OUT + ("body_len",):
        assert np.array_equal(got[k], bare[k]), k
    for r in range(len(bodies)):                                          # the frame cells are 0, the body's cells the bare call's
        lo, hi = got["row_off"][r], got["row_off"][r + 1]
        assert got["covered"][lo] == 0 and got["covered"][hi - 1] == 0
        assert np.array_equal(got["covered"][lo + 1:hi - 1], bare["covered"][bare["row_off"][r]:bare["row_off"][r + 1]])
    short = [[], [5], [5, 6], [5, 7, 6], [5, 5, 5, 5]]                    # rows shorter than their frame
    want = check(tok, short, (1, 2), framed=True)
    assert want["body_len"].tolist() == [0, 0, 0, 1, 2] and want["covered"].tolist() == [0] * 7 + [1, 1, 0]
    rows = np.array([bodies[5][:11], bodies[5][20:31], [8] * 11], dtype=np.int64)         # a 2-D array of rows
    same(tok.repetition_rows(rows, widths, return_covered=True), RO.repetition(rows.tolist(), widths, framed=True))


def test_slices_equal_the_whole(tok):
    widths = (5, 2, 9)
    rng = np.random.default_rng(12)
    rows = [looped(rng, int(T), 5) for T in rng.integers(0, 150, size=90)] + [looped(rng, PIECE + 300, 5)]
    rows[30] = list(rows[29])                                             # identical neighbours
    whole = check(tok, rows, widths)
    for a, b in ((0, 91), (0, 1), (17, 64), (29, 31), (64, 91), (90, 91), (5, 5)):
        part = tok.repetition_rows(rows[a:b], widths, framed=False, return_covered=True)
        for k in OUT:
            assert np.array_equal(part[k], whole[k][:, a:b]), (k, a, b)
        assert np.array_equal(part["covered"], whole["covered"][whole["row_off"][a]:whole["row_off"][b]])
    cat = np.concatenate([tok.repetition_rows(rows[:40], widths, framed=False)["n_covered"],
                          tok.repetition_rows(rows[40:], widths, framed=False)["n_covered"]], axis=1)
    assert np.array_equal(cat, whole["n_covered"])                        # shards concatenate


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
    """The rows lie behind a prefix of junk (row_off_dev[0] != 0) and before a tail of it; outputs left out stay out; nothing outside
    the outputs is written; covered is laid out like the ids."""
    ctx = tok._ctx
    widths = (6, 2, 11)
    K = len(widths)
    rng = np.random.default_rng(41)
    bodies = [looped(rng, T, 6) for T in (0, 3, 70, PIECE + 9, 0, 1, 130)]
    want = RO.repetition(bodies, widths)
    assert (want["n_repeated"] > 0).any()
    N, junk = len(bodies), 37
    flat = np.array([-77] * junk + [v for b in bodies for v in b] + [-88] * 5, dtype=np.int32)
    ro = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bodies], out=ro[1:])
    ro += junk
    d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
    g = [Guarded(ctx, K * N) for _ in OUT]
    g_cov = Guarded(ctx, len(flat), dtype=np.uint16)
    g_one = Guarded(ctx, N)
    try:
        ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
        ctx.ngram_repeats_device(d_ids, d_ro, N, 0, 0, widths, *[x.ptr for x in g], g_cov.ptr)
        for k, x in zip(OUT, g):
            assert np.array_equal(x.read().reshape(K, N), want[k]), k
        cov = g_cov.read()
        fill16 = g_cov.fill
        assert (cov[:junk] == fill16).all() and (cov[int(ro[-1]):] == fill16).all()       # the junk's cells are nobody's
        assert np.array_equal(cov[junk:int(ro[-1])], want["covered"])
        ctx.ngram_repeats_device(d_ids, d_ro, N, 0, 0, (11,), 0, 0, 0, 0, 0, g_one.ptr, 0)           # top_pos alone, a long row among them
        assert np.array_equal(g_one.read(), want["top_pos"][2])
        ctx.ngram_repeats_device(d_ids, d_ro, N, 0, 0, (2,), 0, 0, 0, g_one.ptr, 0, 0, 0)            # n_covered alone
        assert np.array_equal(g_one.read(), want["n_covered"][1])
        # with skips: the junk's last word and the first tail word are a frame nobody reads
        ctx.h2d(d_ro, np.array([junk - 1, int(ro[-1]) + 1], dtype=np.int64))
        ctx.ngram_repeats_device(d_ids, d_ro, 1, 1, 1, widths, *[x.ptr for x in g], g_cov.ptr)
        one = RO.repetition([[v for b in bodies for v in b]], widths)
        for k, x in zip(OUT, g):
            assert x.read()[:K].tolist() == one[k][:, 0].tolist(), k      # (laid out [K, 1] now: the first K cells)
        cov = g_cov.read()
        assert cov[junk - 1] == 0 and cov[int(ro[-1])] == 0 and np.array_equal(cov[junk:int(ro[-1])], one["covered"])
    finally:
        for x in g + [g_cov, g_one]:
            x.free()
        ctx.free(d_ids); ctx.free(d_ro)


def test_a_bare_context_is_enough():
    """the call needs neither the tables nor the decoder snapshot"""
    from genz_tokenize import _native
    ctx = _native.Context()
    try:
        bodies = [[1, 2, 1, 2, 1], [], [7, 8, 9], [4, 9, 9, 4, 9, 9]]
        q = np.array([v for b in bodies for v in b], dtype=np.int32)
        qo = np.array([0, 5, 5, 8, 14], dtype=np.int64)
        got = ctx.ngram_repeats(q, qo, (2, 1), False, True)
        want = RO.repetition(bodies, (2, 1))
        for k in OUT + ("covered",):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        assert want["top_count"].tolist() == [[2, 0, 1, 2], [3, 0, 1, 4]] and want["top_pos"].tolist() == [[0, -1, 0, 0], [0, -1, 0, 1]]
    finally:
        ctx.close()


# ---- texts, end to end ------------------------------------------------------------------------------------------------------
def test_text_end_to_end(tok):
    r = random.Random(7)
    texts = [" ".join(r.sample(WO.WORDS, len(WO.WORDS))) for _ in range(40)]      # ordinary: every word once, in some order
    sentence = "xin chào Việt_Nam học máy"
    spam = {3: " ".join([sentence] * 6), 17: texts[17] + " " + " ".join(["sinh_viên công_nghệ hello"] * 12), 31: "a " * 40,
            38: " ".join([texts[38]] * 3)}
    for i, t in spam.items():
        texts[i] = t
    texts += ["", "xin", "xin chào Việt_Nam"]
    e = tok.encode_batch(texts, max_len=None)
    ro = e["row_off"]
    rows = [e["input_ids"][ro[i]:ro[i + 1]].tolist() for i in range(len(texts))]
    nine = (2, 3, 4, 5, 6, 7, 8, 9, 10)
    want = RO.repetition(rows, nine, framed=True)
    got = tok.encode_repetition(texts)
    assert got["widths"] == nine
    same(got, want, covered=False)
    same(tok.encode_repetition(texts, word_table=False), want, covered=False)
    same(tok.repetition_rows(rows, return_covered=True), want)
    part = tok.encode_repetition(texts[10:35], (7, 3))
    assert np.array_equal(part["n_covered"], want["n_covered"][[5, 1], 10:35]) and np.array_equal(part["top_pos"], want["top_pos"][[5, 1], 10:35])
    # the decision
    out = tok.repetition_filter(texts)
    same({k: out[k] for k in OUT + ("body_len", "widths")}, want, covered=False)
    assert sorted(out) == sorted(OUT + ("body_len", "widths", "top_fraction", "dup_fraction", "keep"))
    assert sorted(out["top_fraction"]) == [2, 3, 4] and sorted(out["dup_fraction"]) == [5, 6, 7, 8, 9, 10]
    body = np.maximum(want["body_len"], 1).astype(np.float64)
    keep = np.ones(len(texts), dtype=bool)
    for n, bound in {2: 0.20, 3: 0.18, 4: 0.16}.items():
        assert np.array_equal(out["top_fraction"][n], n * want["top_count"][n - 2] / body)
        keep &= n * want["top_count"][n - 2] / body <= bound
    for n, bound in {5: 0.15, 6: 0.14, 7: 0.13, 8: 0.12, 9: 0.11, 10: 0.10}.items():
        assert np.array_equal(out["dup_fraction"][n], want["n_covered"][n - 2] / body)
        keep &= want["n_covered"][n - 2] / body <= bound
    assert out["keep"].dtype == bool and np.array_equal(out["keep"], keep)
    dropped = np.flatnonzero(~out["keep"]).tolist()
    assert dropped == sorted(spam) + [42]                                 # exactly the planted ones go, every ordinary document stays -- and
    assert want["body_len"][40:42].tolist() == [0, 1] and 2 <= want["body_len"][42] < 10      # a document of a few tokens, whose every 2-gram is
                                                                          # more than a fifth of it: the shares
                                                                          # are Gopher's as stated, and a caller tunes the bounds for short texts
    only = tok.repetition_filter(texts, top_max={}, dup_max={5: 0.15})
    assert only["widths"] == (5,) and np.flatnonzero(~only["keep"]).tolist() == sorted(spam)
    loose = tok.repetition_filter(texts, top_max={2: 1.0}, dup_max={})
    assert loose["widths"] == (2,) and np.array_equal(loose["keep"], 2 * want["top_count"][0] / body <= 1.0)
    for empty in ([], [""], ["", "   "]):
        got = tok.repetition_filter(empty)
        assert all(got[k].shape == (9, len(empty)) for k in OUT) and got["keep"].shape == (len(empty),) and got["keep"].all()
        assert (got["top_pos"] == -1).all()


# ---- refusals at the ABI ----------------------------------------------------------------------------------------------------
def test_refusals(tok):
    from genz_tokenize import _native
    ctx, lib, P, vp = tok._ctx, tok._ctx.lib, _native._ptr, ctypes.c_void_p
    h, INV, LIM = ctx.handle, _native.GZ_E_INVALID, _native.GZ_E_LIMIT
    ids = np.arange(10, dtype=np.int32)
    ro = np.array([0, 4, 10], dtype=np.int64)
    two = np.array([2, 3], dtype=np.int32)
    d_ids, d_ro = ctx.alloc(64), ctx.alloc(64)
    g = [Guarded(ctx, 4) for _ in OUT]
    g_cov = Guarded(ctx, 10, dtype=np.uint16)
    said = set()

    def refused(call, device=True, code=INV):
        out = [np.full(4, FILL, dtype=np.int32) for _ in OUT]
        cov = np.full(10, 0x5A5A, dtype=np.uint16)
        assert call(lib.gz_ngram_repeats, P(ids), P(ro), [P(a) for a in out], P(cov)) == code
        said.add(lib.gz_last_error(h))
        assert all((a == FILL).all() for a in out) and (cov == 0x5A5A).all()
        if device:
            assert call(lib.gz_ngram_repeats_device, vp(d_ids), vp(d_ro), [vp(x.ptr) for x in g], vp(g_cov.ptr)) == code
            assert lib.gz_last_error(h) in said
            assert all(x.untouched() for x in g) and g_cov.untouched()

    def widths(*w):
        a = np.array(w, dtype=np.int32)
        return lambda f, i, o, out, c: f(h, i, o, 2, 0, 0, P(a), len(w), *out, c)
    try:
        ctx.h2d(d_ids, ids); ctx.h2d(d_ro, ro)
        refused(lambda f, i, o, a, c: f(h, i, o, -1, 0, 0, P(two), 2, *a, c))
        for sf, sb in ((2, 0), (0, 2), (-1, 0), (0, -1)):
            refused(lambda f, i, o, a, c: f(h, i, o, 2, sf, sb, P(two), 2, *a, c))
        for count in (0, 17, -1):
            refused(lambda f, i, o, a, c: f(h, i, o, 2, 0, 0, P(two), count, *a, c))
        refused(lambda f, i, o, a, c: f(h, i, o, 2, 0, 0, None, 2, *a, c))
        for w in ((0, 2), (2, 33), (-5,)):
            refused(widths(*w))
        for w in ((2, 2), (5, 6, 7, 5)):
            refused(widths(*w))
        refused(lambda f, i, o, a, c: f(h, i, None, 2, 0, 0, P(two), 2, *a, c))
        refused(lambda f, i, o, a, c: f(h, i, o, 2, 0, 0, P(two), 2, a[0], a[0], a[2], a[3], a[4], a[5], c))      # two outputs in one array
        assert len(said) == 8                                             # each rule has its own sentence
        refused(lambda f, i, o, a, c: f(h, None, o, 2, 0, 0, P(two), 2, *a, c))
        refused(lambda f, i, o, a, c: f(h, i, o, 2, 0, 0, P(two), 2, i, a[1], a[2], a[3], a[4], a[5], c))         # an output over the ids
        refused(lambda f, i, o, a, c: f(h, i, o, 2, 0, 0, P(two), 2, a[0], a[1], a[2], a[3], a[4], o, c))         # an output over the offsets
        refused(lambda f, i, o, a, c: f(h, i, o, 2, 0, 0, P(two), 2, *a, i))                                       # covered over the ids
        assert len(said) == 8
        # the host form's own: offsets, and the limits it can read from them
        out = [np.full(4, FILL, dtype=np.int32) for _ in OUT]
        for bad, words in ((np.array([0, 7, 4], dtype=np.int64), b"row offsets must not decrease"), (np.array([5, 6, 2], dtype=np.int64), b"bad row offsets")):
            assert lib.gz_ngram_repeats(h, P(ids), P(bad), 2, 0, 0, P(two), 2, *[P(a) for a in out], None) == INV
            assert words in lib.gz_last_error(h) and all((a == FILL).all() for a in out)
        for big, words in ((np.array([0, 2 ** 31, 2 ** 31 + 4], dtype=np.int64), b"2^31"), (np.array([0, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.int64), b"2^32 - 1")):
            assert lib.gz_ngram_repeats(h, P(ids), P(big), 2, 0, 0, P(two), 2, *[P(a) for a in out], None) == LIM
            assert words in lib.gz_last_error(h) and all((a == FILL).all() for a in out)
        ctx.h2d(d_ro, np.array([0, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.int64))                # the device form reads the extent before it launches
        assert lib.gz_ngram_repeats_device(h, vp(d_ids), vp(d_ro), 2, 0, 0, P(two), 2, *[vp(x.ptr) for x in g], None) == LIM
        assert b"2^32 - 1" in lib.gz_last_error(h) and all(x.untouched() for x in g)
        ctx.h2d(d_ro, np.array([5, 6, 2], dtype=np.int64))
        assert lib.gz_ngram_repeats_device(h, vp(d_ids), vp(d_ro), 2, 0, 0, P(two), 2, *[vp(x.ptr) for x in g], None) == INV
        assert b"bad row offsets" in lib.gz_last_error(h) and all(x.untouched() for x in g)
        ctx.h2d(d_ro, ro)
        # nothing to do is no error: nothing is written, no pointer is needed
        assert lib.gz_ngram_repeats(h, None, None, 0, 0, 0, P(two), 2, None, None, None, None, None, None, None) == _native.GZ_OK
        assert lib.gz_ngram_repeats_device(h, None, None, 0, 1, 1, P(two), 2, None, None, None, None, None, None, None) == _native.GZ_OK
        assert lib.gz_ngram_repeats(None, P(ids), P(ro), 2, 0, 0, P(two), 2, *[P(a) for a in out], None) == INV
        # every output may be left out
        assert lib.gz_ngram_repeats(h, P(ids), P(ro), 2, 0, 0, P(two), 2, None, None, None, None, None, None, None) == _native.GZ_OK
        assert lib.gz_ngram_repeats(h, P(ids), P(ro), 2, 0, 0, P(two), 2, None, P(out[1]), None, None, None, None, None) == _native.GZ_OK
        assert out[1].tolist() == [3, 5, 2, 4] and (out[0] == FILL).all()
        assert lib.gz_ngram_repeats_device(h, vp(d_ids), vp(d_ro), 2, 0, 0, P(two), 2, None, None, None, None, None, None, None) == _native.GZ_OK
    finally:
        for x in g + [g_cov]:
            x.free()
        ctx.free(d_ids); ctx.free(d_ro)
    check(tok, [[1, 2, 3, 4, 1, 2]], [2], framed=False)                   # the context is usable afterwards
