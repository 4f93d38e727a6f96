"""The exchange step on the GPU (gz_compact_rows[16], gz_expand_rows[16], gz_compact_block, gz_expand_block, gz_encode_emit_block /
gz_block_total, and the 32-bit row-offset scan behind them) against the rule of tests/exchange_oracle.py, which
tests/test_exchange_inputs.py ties to answers written out by hand.  Every comparison is exact; every output stands between guard
cells that must come back untouched; the inputs count (every cell its own value) and hold junk, not the pad id, behind a row's real
entries.  Before every expansion the test asserts that the largest entry index the rule reads lies inside the buffer it passes.

Written for the constants exchange_oracle names: a wave of gz_compact_kernel takes 8 rows and the first 64 entries of each side by
side, 4 waves a workgroup; the scan walks trips of 4 096 and switches to three kernels at 8 * 4 096 rows."""
import ctypes

import numpy as np
import pytest

import exchange_oracle as X
from genz_tokenize.distributed import GatherRound

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
GUARD = 64


class Guarded:
    """n cells of `dtype` on the device between two runs of guard cells, all pre-filled with FILL bytes."""

    def __init__(self, ctx, n, guard=GUARD, dtype=np.int32):
        self.ctx, self.n, self.guard, self.dtype = ctx, n, guard, np.dtype(dtype)
        self.fill = np.frombuffer(np.full(2, FILL, dtype=np.int32).tobytes(), dtype=self.dtype)[0]
        self.base = ctx.alloc(self.dtype.itemsize * (n + 2 * guard) + 16)
        ctx.h2d(self.base, np.full(n + 2 * guard, self.fill, dtype=self.dtype))
        self.ptr = self.base + self.dtype.itemsize * guard

    def read(self):
        a = np.empty(self.n + 2 * self.guard, dtype=self.dtype)
        self.ctx.d2h(a, self.base)
        assert (a[:self.guard] == self.fill).all() and (a[self.guard + self.n:] == self.fill).all(), "guard cells were written"
        return a[self.guard:self.guard + self.n]

    def untouched(self):
        return bool((self.read() == self.fill).all())


class Arena:
    """Device buffers of one test, freed together."""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.ctx.alloc(arr.nbytes + 16)
        self.held.append(d)
        if arr.nbytes:
            self.ctx.h2d(d, arr)
        return d

    def raw(self, nbytes):
        d = self.ctx.alloc(nbytes + 16)
        self.held.append(d)
        return d

    def guarded(self, n, dtype=np.int32):
        g = Guarded(self.ctx, n, GUARD, dtype)
        self.held.append(g.base)
        return g

    def close(self):
        for d in self.held:
            self.ctx.free(d)
        self.held = []


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    t = Tokenize()
    t._sync_tables()
    return t


@pytest.fixture(scope="module")
def sp(tok):
    pad, bos, eos = tok._special_ids()[:3]
    return dict(pad=pad, bos=bos, eos=eos)


@pytest.fixture
def A(tok):
    a = Arena(tok._ctx)
    yield a
    a.close()


def entry_type(bits):
    return np.uint16 if bits == 16 else np.int32


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def same_block(got, n, total, bits, want_words, defined):
    """A block read back from between its guards, part by part; the bytes of the last word the block does not define stay FILL."""
    assert len(got) == len(want_words)
    g, w = X.split(got, n, total, bits), X.split(want_words, n, total, bits)
    for part, a, b in zip(("n_real", "first", "entries"), g, w):
        same(a, b, part)
    tail = got.view(np.uint8)[4 * (len(got) - 1) + defined:] if len(got) else np.zeros(0, np.uint8)
    assert (tail == 0x5A).all(), "bytes behind an odd number of 16-bit entries were written"


def expanded(ctx, A, call, n, L, want):
    """Runs one expansion into guarded outputs; (ids, mask) after a clean or a refusing synchronisation, as `want` says."""
    from genz_tokenize import _native
    gi, gm = A.guarded(n * L), A.guarded(n * L)
    call(gi.ptr, gm.ptr)
    if want.bad:
        with pytest.raises(_native.GzError) as e:
            ctx.sync()
        assert e.value.code == _native.GZ_E_INVALID and "exchange block" in str(e.value)
    else:
        ctx.sync()
    ctx.sync()                                                       # (reported once, then cleared)
    ids, mask = gi.read().reshape(n, L), gm.read().reshape(n, L)
    same(ids, want.ids, "ids")
    same(mask, want.mask, "mask")
    return ids, mask


def expand_block(ctx, A, d_block, cells, n_real, first, entries, L, bits, total, pad):
    """gz_expand_block of a block that lies at d_block with `cells` entry cells behind its two arrays, against the rule."""
    want = X.expand(entries, first, n_real, L, pad, total)
    assert want.max_read < cells                                     # what the rule reads lies inside the buffer
    n = len(n_real)
    return expanded(ctx, A, lambda i, m: ctx.expand_block(d_block, n, L, i, m, bits=bits, total=total), n, L, want), want


def four_calls(ctx, A, ids, n_real, L, bits, pad, rows_calls=True):
    """compact_rows, expand_rows of its output, compact_block, expand_block of its output: each against the rule, and the expansions
    against the dense rows themselves.  Returns what expand_block gave."""
    n = len(n_real)
    E = entry_type(bits)
    entries, first, total = X.compact(ids, n_real)
    back = X.dense(ids, n_real, pad)
    d_rows, d_nr = A.put(ids), A.put(n_real)
    if rows_calls:
        g = A.guarded(total, E)
        assert ctx.compact_rows(d_rows, d_nr, n, L, g.ptr, bits=bits) == total
        got = g.read()
        same(got, entries.astype(E), "compact_rows entries")
        want = X.expand_scanned(got, n_real, L, pad)
        assert want.max_read < total                                 # what the rule reads lies inside the buffer
        assert not want.bad and np.array_equal(want.ids, back)
        expanded(ctx, A, lambda i, m: ctx.expand_rows(g.ptr, d_nr, n, L, i, m, bits=bits), n, L, want)
    words, defined = X.block(ids, n_real, bits)
    gb = A.guarded(len(words))
    assert ctx.compact_block(d_rows, d_nr, n, L, gb.ptr, bits=bits) == total
    got = gb.read()
    same_block(got, n, total, bits, words, defined)
    nr2, f2, e2 = X.split(got, n, total, bits)
    (ids2, mask2), want = expand_block(ctx, A, gb.ptr, (len(words) - 2 * n) * 32 // bits, nr2, f2, e2, L, bits, total, pad)
    assert not want.bad and np.array_equal(want.ids, back)
    return ids2, mask2


# ---- a. row lengths around the wave ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("L", X.ROW_LS)
def test_row_lengths_around_the_wave(tok, sp, A, L, bits):
    n_real = X.edge_batch(L)
    four_calls(tok._ctx, A, X.counting_rows(n_real, L), n_real, L, bits, sp["pad"])


# ---- b. row counts around a wave's 8 rows and a workgroup's 32 -------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n_rows", X.ROW_COUNTS)
def test_row_counts_around_the_wave_and_the_workgroup(tok, sp, A, n_rows, bits):
    """No rows at all: valid pointers, a total of 0, no output cell written (every output is zero cells between its guards)."""
    n_real = X.count_batch(n_rows)
    four_calls(tok._ctx, A, X.counting_rows(n_real, X.ROW_COUNT_L), n_real, X.ROW_COUNT_L, bits, sp["pad"])


# ---- c. the scan, read from first[] of compact_block -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", X.SCAN_NS)
def test_scan_trips_and_the_switch_to_three_kernels(tok, sp, A, n_rows):
    n_real = X.scan_batch(n_rows, X.SCAN_L)
    four_calls(tok._ctx, A, X.counting_rows(n_real, X.SCAN_L), n_real, X.SCAN_L, 32, sp["pad"], rows_calls=n_rows in (4097, 36865))


@pytest.mark.parametrize("n_rows", X.SCAN_BIG_NS)
def test_scan_whose_bases_take_a_second_trip(tok, sp, A, n_rows):
    n_real = X.scan_batch(n_rows, X.SCAN_BIG_L)
    four_calls(tok._ctx, A, X.counting_rows(n_real, X.SCAN_BIG_L), n_real, X.SCAN_BIG_L, 32, sp["pad"], rows_calls=False)


@pytest.mark.parametrize("n_rows", X.SCAN_NS + X.SCAN_BIG_NS[1:])
def test_expand_rows_scans_the_row_lengths_again(tok, sp, A, n_rows):
    """The receiving side's own scan: gz_expand_rows of entries the rule laid out on the host, so the scan's offsets are used as they
    are (no compact call on the same offsets comes before)."""
    ctx, L = tok._ctx, X.SCAN_L if n_rows in X.SCAN_NS else X.SCAN_BIG_L
    n_real = X.scan_batch(n_rows, L)
    ids = X.counting_rows(n_real, L)
    entries, _, total = X.compact(ids, n_real)
    want = X.expand_scanned(entries, n_real, L, sp["pad"])
    assert want.max_read < total and not want.bad and np.array_equal(want.ids, X.dense(ids, n_real, sp["pad"]))
    d_e, d_nr = A.put(entries), A.put(n_real)
    expanded(ctx, A, lambda i, m: ctx.expand_rows(d_e, d_nr, n_rows, L, i, m), n_rows, L, want)


# ---- d. values -------------------------------------------------------------------------------------------------------------------
def test_values_pass_through_32_bit_entries(tok, sp, A):
    pad, bos, eos = sp["pad"], sp["bos"], sp["eos"]
    vals = [-1, -2 ** 31, 2 ** 31 - 1, 70000, pad, bos, eos, 7]
    ids = np.array([vals, vals[::-1], [pad, pad, pad, -5, -5, -5, -5, -5], [5, pad, 6, pad, pad, -6, -6, -6]], dtype=np.int32)
    n_real = np.array([8, 8, 3, 5], dtype=np.int32)
    ids2, mask2 = four_calls(tok._ctx, A, ids, n_real, 8, 32, pad)
    assert ids2[0].tolist() == vals and ids2[1].tolist() == vals[::-1]
    # the pad id inside a real run: mask 0 at that cell, its neighbours keep 1
    assert mask2[0].tolist() == [int(v != pad) for v in vals] and mask2[0].tolist().count(0) == 1
    assert mask2[3].tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and ids2[3].tolist() == [5, pad, 6] + [pad] * 5
    assert not mask2[2].any()


def test_values_pass_through_16_bit_entries(tok, sp, A):
    """Bit 15 is a value bit: 0x8000 and 0xFFFF come back as 32768 and 65535."""
    pad = sp["pad"]
    assert pad == 0
    vals = [0, 1, 0x7FFF, 0x8000, 0xFFFF, 5]
    ids = np.array([vals, vals[::-1], [0x8000, -5, -5, -5, -5, -5], [0xFFFF, 0x8000, 0xFFFF, -6, -6, -6], [7, 0, 0x8001, 0, -7, -7]],
                   dtype=np.int32)
    n_real = np.array([6, 6, 1, 3, 4], dtype=np.int32)
    ctx = tok._ctx
    ids2, mask2 = four_calls(ctx, A, ids, n_real, 6, 16, pad)
    assert ids2[0].tolist() == [0, 1, 32767, 32768, 65535, 5] and mask2[0].tolist() == [0, 1, 1, 1, 1, 1]
    assert ids2[3].tolist() == [65535, 32768, 65535, 0, 0, 0] and ids2[2].tolist() == [32768, 0, 0, 0, 0, 0]
    assert ids2[4].tolist() == [7, 0, 0x8001, 0, 0, 0] and mask2[4].tolist() == [1, 0, 1, 0, 0, 0]
    g = A.guarded(20, np.uint16)
    assert ctx.compact_rows(A.put(ids), A.put(n_real), 5, 6, g.ptr, bits=16) == 20
    assert g.read().tolist() == vals + vals[::-1] + [0x8000, 0xFFFF, 0x8000, 0xFFFF, 7, 0, 0x8001, 0]


# ---- e. blocks written by hand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_a_blocks_rows_may_lie_in_any_order(tok, sp, A, order, bits):
    L = 65
    n_real = X.edge_batch(L)
    n = len(n_real)
    ids = X.counting_rows(n_real, L)
    rows = list(range(n))[::-1] if order == "reversed" else np.random.default_rng(5).permutation(n).tolist()
    first, at = np.zeros(n, dtype=np.int64), 0
    for r in rows:
        first[r] = at
        at += int(n_real[r])
    entries = np.concatenate([ids[r, :n_real[r]] for r in rows]).astype(entry_type(bits))
    assert (np.diff(first[n_real > 0]) < 0).any()                    # not the order gz_compact_block writes
    words, _ = X.layout(n_real, first, entries, bits)
    (ids2, _), want = expand_block(tok._ctx, A, A.put(words), (len(words) - 2 * n) * 32 // bits, n_real, first, entries, L, bits, at, sp["pad"])
    assert not want.bad
    same(ids2, X.dense(ids, n_real, sp["pad"]), "rows in row order")


def test_two_blocks_back_to_back_in_one_buffer(tok, sp, A):
    """The receive buffer of a round: the first block has an odd number of 16-bit entries, so the second starts behind half a word
    that belongs to nobody (junk here)."""
    L, ctx = 5, tok._ctx
    nr = [np.array([3, 0, 5, 1], dtype=np.int32), np.array([2, 5, 0, 4, 1], dtype=np.int32)]
    ids = [X.counting_rows(nr[0], L, base=1000), X.counting_rows(nr[1], L, base=5000)]
    blocks = [X.block(ids[p], nr[p], 16) for p in (0, 1)]
    totals = [int(nr[p].sum()) for p in (0, 1)]
    assert totals[0] % 2 == 1 and blocks[0][1] == 2
    g = GatherRound(2, 16, [len(nr[0]), len(nr[1])])
    capacity = g.announce(totals)
    buf = np.full(capacity, -0x21524111, dtype=np.int32)
    for p in (0, 1):
        buf[g.word_offset(p):g.word_offset(p) + len(blocks[p][0])] = blocks[p][0]
    assert g.word_offset(1) == len(blocks[0][0])
    buf.view(np.uint16)[2 * g.word_offset(1) - 1] = 0xBEEF
    d = A.put(buf)
    for p in (0, 1):
        n = len(nr[p])
        n_real, first, entries = X.split(blocks[p][0], n, totals[p], 16)
        cells = (capacity - g.word_offset(p) - 2 * n) * 2
        (ids2, _), want = expand_block(ctx, A, d + 4 * g.word_offset(p), cells, n_real, first, entries, L, 16, totals[p], sp["pad"])
        assert not want.bad
        same(ids2, X.dense(ids[p], nr[p], sp["pad"]), "block %d" % p)


# ---- f. what gz_expand_kernel refuses --------------------------------------------------------------------------------------------
ENTRIES = list(range(100, 112))
GOOD = (3, 4, 12)
# (first, n_real of the row under test, announced total, refused)
EDGES = [((3, 4, 12), False),            # n_real == row_len
         ((3, 5, 12), True),             # row_len + 1
         ((9, 3, 12), False),            # first + n_real == total
         ((9, 3, 11), True),             # total + 1
         ((10, 3, 12), True),
         ((3, -1, 12), True),            # a negative count
         ((X.U32, 0, 12), True),         # the sum is formed in 64 bits
         ((X.U32, 1, 12), True),
         ((2, 1, 0), True)]              # a total of nothing, rows that hold something


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("edge,refused", EDGES, ids=["f%d_n%d_t%d" % e for e, _ in EDGES])
def test_expand_block_refuses_rows_at_the_rules_edges(tok, sp, A, edge, refused, bits):
    ctx, L, pad = tok._ctx, 4, sp["pad"]
    entries = np.array(ENTRIES, dtype=entry_type(bits))

    def run(first, n_real, total):
        nr, f = np.array([2, n_real, 1], dtype=np.int64), np.array([0, first, 2], dtype=np.int64)
        words, _ = X.layout(nr, f, entries, bits)
        return expand_block(ctx, A, A.put(words), len(entries), nr, f, entries, L, bits, total, pad)
    (ids, mask), want = run(*edge)
    assert want.bad == refused
    if edge[2] >= 3:                                                 # the good rows of the same block are intact
        assert ids[0].tolist() == [100, 101, pad, pad] and ids[2].tolist() == [102, pad, pad, pad]
        assert mask[0].tolist() == [1, 1, 0, 0] and mask[2].tolist() == [1, 0, 0, 0]
        assert (ids[1] == pad).all() == refused
    else:
        assert (ids == pad).all() and not mask.any()
    (ids, _), want = run(*GOOD)                                      # a good expansion afterwards, and a clean synchronisation
    assert not want.bad and ids[1].tolist() == [103, 104, 105, 106]


def test_a_total_of_nothing_accepts_empty_rows(tok, sp, A):
    ctx, pad = tok._ctx, sp["pad"]
    nr, f = np.array([0, 0, 0], dtype=np.int64), np.array([0, 0, 0], dtype=np.int64)
    words, _ = X.layout(nr, f, ENTRIES, 32)
    (ids, _), want = expand_block(ctx, A, A.put(words), len(ENTRIES), nr, f, ENTRIES, 4, 32, 0, pad)
    assert not want.bad and (ids == pad).all()


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("claims,n_entries", [([2, 5, 3], 10), ([5, 2, 3], 10), ([2, 3, 5], 10), ([2, 3, -1], 5), ([-1], 1)],
                         ids=["middle", "first", "last", "negative_last", "negative_alone"])
def test_expand_rows_refuses_a_claim_beyond_the_row(tok, sp, A, claims, n_entries, bits):
    """A claim of row_len + 1 may stand anywhere (the entry buffer holds the claimed sum); a negative one only in the last row, so
    that no later row's offset wraps into the buffer."""
    ctx, L, pad = tok._ctx, 4, sp["pad"]
    n_real = np.array(claims, dtype=np.int32)
    entries = np.arange(100, 100 + n_entries).astype(entry_type(bits))
    want = X.expand_scanned(entries, n_real, L, pad)
    assert want.bad and want.max_read < n_entries
    d_e, d_nr = A.put(entries), A.put(n_real)
    ids, _ = expanded(ctx, A, lambda i, m: ctx.expand_rows(d_e, d_nr, len(claims), L, i, m, bits=bits), len(claims), L, want)
    good = (n_real >= 0) & (n_real <= L)
    assert (ids[~good] == pad).all() and (ids[good][:, 0] >= 100).all()
    ok, nine = np.array([2, 3, 4], dtype=np.int32), np.arange(50, 59).astype(entry_type(bits))
    want = X.expand_scanned(nine, ok, L, pad)                        # a good expansion afterwards, and a clean synchronisation
    assert not want.bad and want.max_read == 8
    d_e, d_ok = A.put(nine), A.put(ok)
    expanded(ctx, A, lambda i, m: ctx.expand_rows(d_e, d_ok, 3, L, i, m, bits=bits), 3, L, want)


# ---- g. gz_encode_emit_block on tiny batches -------------------------------------------------------------------------------------
def pack(texts):
    raw = [t.encode("utf-8") for t in texts]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) + b"\0" * 64, dtype=np.uint8).copy(), off


def emit_case(ctx, A, sp, texts, L, bits, pair_texts=None):
    """One armed encode call; its block against the layout of the same call's dense input_ids and n_real."""
    from genz_tokenize import _native
    n = len(texts)
    ta, oa = pack(texts)
    d_t, d_o = A.put(ta), A.put(oa)
    d_i, d_m, d_tt, d_sq = (A.raw(4 * n * L) for _ in range(4))
    d_pl, d_r, d_st = A.raw(8 * n + 8), A.raw(4 * n + 4), A.raw(4 * n + 4)
    kw, d_p, d_po = {}, 0, 0
    if pair_texts is not None:
        tp, op = pack(pair_texts)
        d_p, d_po = A.put(tp), A.put(op)
        kw = dict(d_tt=d_tt, d_seq=d_sq, d_pair_len=d_pl, d_status=d_st, h_pair_off=op)
    gb = A.guarded(2 * n + n * L)                                    # (what the header says a block takes at most, for 32-bit entries)
    ctx.encode_emit_block(gb.ptr, bits)
    ctx.encode_device(d_t, d_o, d_p, d_po, n, L, _native.GZ_PADDING | _native.GZ_TRUNCATION, n * L, d_i, d_m, d_n_real=d_r, h_text_off=oa, **kw)
    total = ctx.block_total(0)
    ctx.sync()
    ids, nr = np.empty((n, L), dtype=np.int32), np.empty(n, dtype=np.int32)
    ctx.d2h(ids, d_i)
    ctx.d2h(nr, d_r)
    assert ((nr >= 2) & (nr <= L)).all() and (ids[:, 0] == sp["bos"]).all()
    assert np.array_equal(ids != sp["pad"], np.arange(L)[None, :] < nr[:, None])
    words, defined = X.block(ids, nr, bits)
    assert total == int(nr.sum()) == X.compact(ids, nr)[2]
    got = gb.read()
    same_block(got[:len(words)], n, total, bits, words, defined)
    assert (got[len(words):] == FILL).all(), "words behind the block were written"
    return nr


@pytest.mark.parametrize("L", X.EMIT_LS)
@pytest.mark.parametrize("n", X.EMIT_NS)
def test_encode_emits_the_block_of_a_tiny_batch(tok, sp, A, n, L):
    batches = [[t] for t in X.EMIT_TEXTS[:3]] if n == 1 else [X.emit_texts(n)]
    for texts in batches:
        for bits in (16, 32):
            nr = emit_case(tok._ctx, A, sp, texts, L, bits)
            if n > 1:
                assert nr[0] == L and nr[1] == 2 and nr[2] == 2      # one document cut at L; "" and whitespace: bos and eos alone


def test_encode_emits_the_block_of_a_tiny_batch_of_pairs(tok, sp, A):
    texts = X.emit_texts(9)
    for bits in (16, 32):
        nr = emit_case(tok._ctx, A, sp, texts, 8, bits, pair_texts=texts[1:] + texts[:1])
        assert nr.max() == 8 and nr.min() < 8                        # rows cut at L and rows that fit


# ---- h. entry points -------------------------------------------------------------------------------------------------------------
def refused(code, call, *args, **kw):
    from genz_tokenize import _native
    with pytest.raises(_native.GzError) as e:
        call(*args, **kw)
    assert e.value.code == code, (args, kw, str(e.value))


def test_entry_points_refuse_bad_arguments_and_write_nothing(tok, sp, A):
    from genz_tokenize import _native
    ctx, INV = tok._ctx, _native.GZ_E_INVALID
    n, L = 3, 4
    n_real = np.array([2, 0, 3], dtype=np.int32)
    ids = X.counting_rows(n_real, L)
    words, _ = X.block(ids, n_real, 32)
    d_rows, d_nr, d_blk = A.put(ids), A.put(n_real), A.put(words)
    out, blk, gi, gm = A.guarded(n * L), A.guarded(2 * n + n * L), A.guarded(n * L), A.guarded(n * L)
    for bits in (32, 16):
        for bad_L in (0, -1):
            refused(INV, ctx.compact_rows, d_rows, d_nr, n, bad_L, out.ptr, bits=bits)
            refused(INV, ctx.expand_rows, d_blk + 8 * n, d_nr, n, bad_L, gi.ptr, gm.ptr, bits=bits)
            refused(INV, ctx.compact_block, d_rows, d_nr, n, bad_L, blk.ptr, bits=bits)
            refused(INV, ctx.expand_block, d_blk, n, bad_L, gi.ptr, gm.ptr, bits=bits, total=5)
        refused(INV, ctx.compact_rows, d_rows, d_nr, -1, L, out.ptr, bits=bits)
        refused(INV, ctx.expand_rows, d_blk + 8 * n, d_nr, -1, L, gi.ptr, gm.ptr, bits=bits)
        refused(INV, ctx.compact_block, d_rows, d_nr, -1, L, blk.ptr, bits=bits)
        refused(INV, ctx.expand_block, d_blk, -1, L, gi.ptr, gm.ptr, bits=bits, total=5)
        for k in range(3):                                           # each required pointer NULL
            p = [d_rows, d_nr, out.ptr]
            p[k] = 0
            refused(INV, ctx.compact_rows, p[0], p[1], n, L, p[2], bits=bits)
            p = [d_rows, d_nr, blk.ptr]
            p[k] = 0
            refused(INV, ctx.compact_block, p[0], p[1], n, L, p[2], bits=bits)
        for k in range(4):
            p = [d_blk + 8 * n, d_nr, gi.ptr, gm.ptr]
            p[k] = 0
            refused(INV, ctx.expand_rows, p[0], p[1], n, L, p[2], p[3], bits=bits)
        for k in range(3):
            p = [d_blk, gi.ptr, gm.ptr]
            p[k] = 0
            refused(INV, ctx.expand_block, p[0], n, L, p[1], p[2], bits=bits, total=5)
        for total in (-1, 2 ** 32):
            refused(INV, ctx.expand_block, d_blk, n, L, gi.ptr, gm.ptr, bits=bits, total=total)
    vp = ctypes.c_void_p                                             # no place for the total
    assert ctx.lib.gz_compact_rows(ctx.handle, vp(d_rows), vp(d_nr), n, L, vp(out.ptr), None) == INV
    assert ctx.lib.gz_compact_rows16(ctx.handle, vp(d_rows), vp(d_nr), n, L, vp(out.ptr), None) == INV
    for bits in (32, 16):
        assert ctx.lib.gz_compact_block(ctx.handle, vp(d_rows), vp(d_nr), n, L, bits, vp(blk.ptr), None) == INV
    for bits in (0, 8, 24):
        refused(INV, ctx.compact_block, d_rows, d_nr, n, L, blk.ptr, bits=bits)
        refused(INV, ctx.expand_block, d_blk, n, L, gi.ptr, gm.ptr, bits=bits, total=5)
        refused(INV, ctx.encode_emit_block, blk.ptr, bits)
    ctx.sync()
    for g, what in ((out, "entries"), (blk, "block"), (gi, "ids"), (gm, "mask")):
        assert g.untouched(), what
    four_calls(ctx, A, ids, n_real, L, 32, sp["pad"])                # the context still answers
    four_calls(ctx, A, ids, n_real, L, 16, sp["pad"])


def test_a_context_without_tables(sp):
    """compact_impl needs no tables for 32-bit entries; the 16-bit forms cannot know that the ids fit; an expansion has no pad id."""
    from genz_tokenize import _native
    ctx = _native.Context()
    A = Arena(ctx)
    try:
        n_real = X.edge_batch(65)
        n, L = len(n_real), 65
        ids = X.counting_rows(n_real, L)
        entries, first, total = X.compact(ids, n_real)
        words, defined = X.block(ids, n_real, 32)
        d_rows, d_nr = A.put(ids), A.put(n_real)

        def plain():
            g, gb = A.guarded(total), A.guarded(len(words))
            assert ctx.compact_rows(d_rows, d_nr, n, L, g.ptr) == total
            same(g.read(), entries, "entries")
            assert ctx.compact_block(d_rows, d_nr, n, L, gb.ptr, bits=32) == total
            same_block(gb.read(), n, total, 32, words, defined)
            return g
        g = plain()
        out16, blk, gi, gm = A.guarded(total, np.uint16), A.guarded(len(words)), A.guarded(n * L), A.guarded(n * L)
        refused(_native.GZ_E_LIMIT, ctx.compact_rows, d_rows, d_nr, n, L, out16.ptr, bits=16)
        refused(_native.GZ_E_LIMIT, ctx.compact_block, d_rows, d_nr, n, L, blk.ptr, bits=16)
        refused(_native.GZ_E_LIMIT, ctx.encode_emit_block, blk.ptr, 16)
        for bits in (32, 16):
            refused(_native.GZ_E_NOTABLES, ctx.expand_rows, g.ptr, d_nr, n, L, gi.ptr, gm.ptr, bits=bits)
            refused(_native.GZ_E_NOTABLES, ctx.expand_block, A.put(words), n, L, gi.ptr, gm.ptr, bits=bits, total=total)
        ctx.sync()
        for x, what in ((out16, "entries"), (blk, "block"), (gi, "ids"), (gm, "mask")):
            assert x.untouched(), what
        plain()
    finally:
        A.close()
        ctx.close()
