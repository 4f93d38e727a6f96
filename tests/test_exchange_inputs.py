"""CPU-only: the exchange rule of tests/exchange_oracle.py against answers written out by hand, the refusal rule at each of its
edges, expand as the inverse of compact, the block's length against distributed.block_words, and the shape lists of the GPU tests
against the cases they are named for.  tests/test_gpu_exchange.py relies on all of it."""
import numpy as np
import pytest

import exchange_oracle as X
from genz_tokenize.distributed import GatherRound, block_words

PAD = 0


def shapes():
    """(name, n_real, L) of every generated batch but the largest."""
    for L in X.ROW_LS:
        yield "rows L=%d" % L, X.edge_batch(L), L
    for n in X.ROW_COUNTS:
        yield "counts n=%d" % n, X.count_batch(n), X.ROW_COUNT_L
    for n in X.SCAN_NS:
        yield "scan n=%d" % n, X.scan_batch(n, X.SCAN_L), X.SCAN_L


# ---- known answers ---------------------------------------------------------------------------------------------------------------
ROWS = [[11, 12, 13, 14],
        [21, 22, 23, 24],
        [31, 32, 33, 34],
        [41, 42, 43, 44]]
N_REAL = [2, 0, 4, 1]


def test_compact_by_hand():
    entries, first, total = X.compact(ROWS, N_REAL)
    assert entries.tolist() == [11, 12, 31, 32, 33, 34, 41] and entries.dtype == np.int32
    assert first.tolist() == [0, 2, 2, 6, 7] and first.dtype == np.uint32 and total == 7
    entries, first, total = X.compact(np.zeros((0, 4), np.int32), [])
    assert entries.tolist() == [] and first.tolist() == [0] and total == 0
    entries, first, total = X.compact([[5, 6]], [0])
    assert entries.tolist() == [] and first.tolist() == [0, 0] and total == 0


def test_block_by_hand_at_both_widths():
    words, defined = X.block(ROWS, N_REAL, 32)
    assert words.tolist() == [2, 0, 4, 1, 0, 2, 2, 6, 11, 12, 31, 32, 33, 34, 41] and defined == 4 and words.dtype == np.int32
    # 16 bits, an odd entry count: two to a word, the first in the low half; the last word's high half is not the block's
    words, defined = X.block(ROWS, N_REAL, 16)
    assert words.tolist() == [2, 0, 4, 1, 0, 2, 2, 6, 11 | 12 << 16, 31 | 32 << 16, 33 | 34 << 16, 41] and defined == 2
    assert words.tobytes()[32:36] == bytes([11, 0, 12, 0])                                           # little-endian
    # 16 bits, an even entry count, values with bit 15 set: the word is negative, the entry is not
    words, defined = X.block([[0x8000, 0xFFFF, 7]], [2], 16)
    assert words.tolist() == [2, 0, 0x8000 + (0xFFFF << 16) - (1 << 32)] and defined == 4
    n_real, first, entries = X.split(words, 1, 2, 16)
    assert n_real.tolist() == [2] and first.tolist() == [0] and entries.tolist() == [0x8000, 0xFFFF]
    words, defined = X.block([[-1, -2 ** 31, 2 ** 31 - 1]], [3], 32)
    assert words.tolist() == [3, 0, -1, -2 ** 31, 2 ** 31 - 1]
    assert X.block(np.zeros((0, 3), np.int32), [], 16)[0].tolist() == []


def test_layout_takes_rows_in_any_order():
    # row 0 lies behind row 2, row 1 is empty and points past the end
    words, defined = X.layout([2, 0, 3], [3, 5, 0], [31, 32, 33, 11, 12], 32)
    assert words.tolist() == [2, 0, 3, 3, 5, 0, 31, 32, 33, 11, 12]
    e = X.expand([31, 32, 33, 11, 12], [3, 5, 0], [2, 0, 3], 4, PAD, 5)
    assert e.ids.tolist() == [[11, 12, 0, 0], [0, 0, 0, 0], [31, 32, 33, 0]] and not e.bad and e.max_read == 4


def test_expand_by_hand():
    e = X.expand([11, 12, 31, 32, 33, 34, 41], [0, 2, 2, 6, 7], N_REAL, 4, 9, 7)
    assert e.ids.tolist() == [[11, 12, 9, 9], [9, 9, 9, 9], [31, 32, 33, 34], [41, 9, 9, 9]] and e.ids.dtype == np.int32
    assert e.mask.tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0]] and e.mask.dtype == np.int32
    assert not e.bad and e.max_read == 6
    # an accepted entry equal to the pad id gets mask 0; its neighbours keep 1
    e = X.expand([5, 9, 6], [0], [3], 4, 9, 3)
    assert e.ids.tolist() == [[5, 9, 6, 9]] and e.mask.tolist() == [[1, 0, 1, 0]]
    # 16-bit entries are values 0 .. 65535
    e = X.expand(np.array([0x7FFF, 0x8000, 0xFFFF], np.uint16), [0], [3], 3, PAD, 3)
    assert e.ids.tolist() == [[32767, 32768, 65535]]
    e = X.expand_scanned([11, 12, 31, 32, 33, 34, 41], N_REAL, 4, 9)
    assert e.ids.tolist() == [[11, 12, 9, 9], [9, 9, 9, 9], [31, 32, 33, 34], [41, 9, 9, 9]] and not e.bad
    e = X.expand([], [], [], 4, 9, 0)
    assert e.ids.shape == (0, 4) and not e.bad and e.max_read == -1


# ---- the refusal rule ------------------------------------------------------------------------------------------------------------
ENTRIES = list(range(100, 112))          # 12 entries


def one(first, n_real, L, total):
    """The row under test between two ordinary ones: (row, bad, max_read)."""
    e = X.expand(ENTRIES, [0, first, 2], [2, n_real, 1], L, PAD, total)
    assert e.ids[0].tolist() == [100, 101] + [PAD] * (L - 2) and e.ids[2].tolist() == [102] + [PAD] * (L - 1)
    return e.ids[1].tolist(), e.bad, e.max_read


def test_a_row_may_claim_row_len_entries_and_not_one_more():
    assert one(3, 4, 4, 12) == ([103, 104, 105, 106], False, 6)
    assert one(3, 5, 4, 12) == ([PAD] * 4, True, 2)


def test_a_row_may_end_at_the_total_and_not_one_past_it():
    assert one(9, 3, 4, 12) == ([109, 110, 111, PAD], False, 11)
    assert one(9, 3, 4, 11) == ([PAD] * 4, True, 2)
    assert one(10, 3, 4, 12) == ([PAD] * 4, True, 2)
    assert one(12, 0, 4, 12) == ([PAD] * 4, False, 2)                # an empty row at the very end reads nothing and fits
    assert one(13, 0, 4, 12) == ([PAD] * 4, True, 2)


def test_a_negative_count_is_a_huge_one():
    assert one(3, -1, 4, 12) == ([PAD] * 4, True, 2)
    assert one(3, -2 ** 31, 4, 12) == ([PAD] * 4, True, 2)
    assert one(0, -1, 4, X.U32) == ([PAD] * 4, True, 2)


def test_the_sum_is_formed_in_64_bits():
    assert one(X.U32, 0, 4, 12) == ([PAD] * 4, True, 2)
    assert one(X.U32, 1, 4, 12) == ([PAD] * 4, True, 2)              # (0xFFFFFFFF + 1 is not 0)
    assert one(X.U32, 1, 4, X.U32) == ([PAD] * 4, True, 2)
    assert one(X.U32 - 1, 2, 4, 12) == ([PAD] * 4, True, 2)


def test_a_total_of_nothing_refuses_every_row_that_holds_something():
    e = X.expand(ENTRIES, [0, 0, 1], [0, 1, 0], 4, PAD, 0)
    assert e.bad and (e.ids == PAD).all() and e.max_read == -1
    assert not X.expand(ENTRIES, [0, 0, 0], [0, 0, 0], 4, PAD, 0).bad
    assert X.expand(ENTRIES, [0, 0, 1], [0, 0, 0], 4, PAD, 0).bad    # an empty row that starts past the total is refused too


def test_expand_never_reads_past_the_entries_it_is_given():
    with pytest.raises(IndexError):
        X.expand(ENTRIES, [10], [3], 4, PAD, 13)                     # announced 13, 12 present


def test_scanned_offsets_wrap_like_uint32():
    assert X.scan([2, -1, 3]).tolist() == [0, 2, 1, 4]
    e = X.expand_scanned(ENTRIES, [2, 5, 3], 4, PAD)                 # a claim of L + 1 in the middle: the rows around it stay whole
    assert e.ids.tolist() == [[100, 101, PAD, PAD], [PAD] * 4, [107, 108, 109, PAD]] and e.bad and e.max_read == 9
    e = X.expand_scanned(ENTRIES, [2, 3, -1], 4, PAD)                # a negative claim in the last row
    assert e.ids.tolist() == [[100, 101, PAD, PAD], [102, 103, 104, PAD], [PAD] * 4] and e.bad and e.max_read == 4


# ---- properties over every generated shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_real,L", list(shapes()), ids=[s[0] for s in shapes()])
def test_expand_inverts_compact_and_the_block_has_its_length(name, n_real, L):
    assert n_real.dtype == np.int32 and ((n_real >= 0) & (n_real <= L)).all()
    n = len(n_real)
    ids = X.counting_rows(n_real, L)
    keep = np.arange(L)[None, :] < n_real[:, None]
    assert (ids[keep] >= 1000).all() and (ids[~keep] < 0).all() and len(np.unique(ids)) == ids.size     # every cell its own value
    entries, first, total = X.compact(ids, n_real)
    assert total == int(n_real.sum()) == len(entries) and len(first) == n + 1 and int(first[-1]) == total
    assert (entries >= 1000).all() and (np.diff(entries) > 0).all()
    want = X.dense(ids, n_real, PAD)
    assert (want[~keep] == PAD).all() and np.array_equal(want[keep], ids[keep])
    for e in (X.expand(entries, first, n_real, L, PAD, total), X.expand_scanned(entries, n_real, L, PAD)):
        assert np.array_equal(e.ids, want) and np.array_equal(e.mask, keep.astype(np.int32)) and not e.bad
        assert e.max_read == total - 1
    for bits in (16, 32):
        if bits == 16 and ids[keep].size and ids[keep].max() > 0xFFFF:
            continue
        words, defined = X.block(ids, n_real, bits)
        assert len(words) == block_words(n, total, bits) and defined == (2 if bits == 16 and total % 2 else 4)
        nr2, f2, e2 = X.split(words, n, total, bits)
        assert np.array_equal(nr2, n_real) and np.array_equal(f2, first[:-1]) and np.array_equal(e2.astype(np.int32), entries)


@pytest.mark.parametrize("n", X.SCAN_BIG_NS)
def test_the_largest_scan_shapes(n):
    L = X.SCAN_BIG_L
    assert X.SCAN_BIG_N == 1024 * 4096 + 1 and X.SCAN_BIG_NS == (1024 * 4096, 1024 * 4096 + 1) and L == 1
    assert n // X.SCAN_TRIP + 1 == X.BASES_TRIP + 1                  # blocks of the (n + 1)-element problem: one more than a trip
    assert (X.SCAN_BIG_NS[0] - 1) // X.SCAN_TRIP + 1 == X.BASES_TRIP # ... and with one row fewer than the smaller, a single trip
    n_real = X.scan_batch(n, L)
    assert set(np.unique(n_real).tolist()) == {0, 1} and n_real[-1] == 1
    ids = X.counting_rows(n_real, L)
    entries, first, total = X.compact(ids, n_real)
    assert total == int(n_real.sum()) and np.array_equal(entries, ids[n_real == 1, 0])
    assert np.array_equal(X.expand(entries, first, n_real, L, PAD, total).ids, X.dense(ids, n_real, PAD))


# ---- the generators deliver what their names promise -----------------------------------------------------------------------------
def test_row_lengths_and_their_edge_values():
    assert X.ROW_LS == (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200)
    assert X.AROUND_WAVE == (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)
    assert (X.WAVE, X.ROWS_PER_WAVE, X.WAVES) == (64, 8, 4)
    for L in X.ROW_LS:
        want = {0, 1, L - 1, L} | {v for v in X.AROUND_WAVE if 0 <= v <= L}
        assert set(X.edge_counts(L)) == want
        b = X.edge_batch(L)
        assert ((b >= 0) & (b <= L)).all()
        for v in want:
            assert (b == v).sum() >= 3, (L, v)                       # several times each
        assert b[0] == 0 and b[-1] == 0                              # an empty row at the start and at the end
        k = np.flatnonzero((b[1:-1] == 0) & (b[:-2] == L) & (b[2:] == L))
        assert len(k) >= 1                                           # ... and between two full ones
        assert b.tolist() != sorted(b.tolist())                      # shuffled
    assert X.edge_counts(200) == [0, 1, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 199, 200]
    assert X.edge_counts(64) == [0, 1, 62, 63, 64] and X.edge_counts(1) == [0, 1]


def test_row_counts_and_their_batches():
    assert X.ROW_COUNTS == (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257) and X.ROW_COUNT_L == 5
    per_wave, per_group = X.ROWS_PER_WAVE, X.ROWS_PER_WAVE * X.WAVES
    assert {per_wave - 1, per_wave, per_wave + 1, per_group - 1, per_group, per_group + 1} <= set(X.ROW_COUNTS)
    assert {n % per_wave for n in X.ROW_COUNTS} >= {0, 1, 7}
    seen = set()
    for n in X.ROW_COUNTS:
        b = X.count_batch(n)
        assert len(b) == n and ((b >= 0) & (b <= 5)).all()
        seen |= set(b.tolist())
        if n >= per_wave:
            assert b[per_wave - 1] > 0                               # the first wave's eighth row holds something
    assert seen == {0, 1, 2, 3, 4, 5}


def test_scan_sizes_are_the_ones_listed():
    assert X.SCAN_NS == (4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 36863, 36864, 36865) and X.SCAN_L == 2
    assert (X.SCAN_TRIP, X.SCAN_SWITCH, X.BASES_TRIP) == (4096, 32768, 1024)
    T, S = X.SCAN_TRIP, X.SCAN_SWITCH
    assert {T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, S - 1, S, S + 1, S + T - 1, S + T, S + T + 1} == set(X.SCAN_NS)
    assert sum(n < S for n in X.SCAN_NS) == 7 and sum(n >= S for n in X.SCAN_NS) == 5
    for n in X.SCAN_NS:
        b = X.scan_batch(n, X.SCAN_L)
        assert len(b) == n and set(np.unique(b).tolist()) == {0, 1, 2} and b[-1] == 2
        if n >= S:                                                   # the slots the add kernel must and must not touch hold live sums
            first = X.scan(b)
            assert first[T] > 0 and first[T + 1] >= first[T] and first[n] == b.sum()


def test_emit_texts(oracle_tables):
    import gz_oracle as O
    assert X.EMIT_NS == (1, 7, 8, 9, 33) and X.EMIT_LS == (4, 6, 8)
    for n in X.EMIT_NS:
        t = X.emit_texts(n)
        assert len(t) == n and t[:3] == X.EMIT_TEXTS[:min(n, 3)]
        if n >= 7:
            assert "" in t and any(s and not s.strip() for s in t)
    lens = [len(O.encode(s, oracle_tables)) for s in X.emit_texts(33)]
    assert lens[0] > max(X.EMIT_LS) and lens[1] == 2 and lens[2] == 2                  # cut at every L; bos and eos alone
    assert min(lens) == 2 and any(2 < v <= min(X.EMIT_LS) for v in lens)               # ... and rows that fit whole


def test_two_blocks_back_to_back_start_at_whole_words():
    g = GatherRound(2, 16, [3, 2])
    g.announce([5, 4])
    assert g.word_offset(0) == 0 and g.word_offset(1) == block_words(3, 5, 16) == 6 + 3
    assert len(X.layout([2, 2, 1], [0, 2, 4], [1, 2, 3, 4, 5], 16)[0]) == g.word_offset(1)
