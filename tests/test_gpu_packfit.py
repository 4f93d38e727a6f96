"""Best-fit packing on the GPU (gz_pack_rows_fit / gz_pack_rows_fit_device; Tokenize.pack_rows, encode_packs_fit and
encode_packs_to_device with order="fit", unpack_rows) against the sequential rule of tests/packfit_oracle.py, which
tests/test_packfit_inputs.py ties to pack_oracle and tests/test_packfit_plan.py to the host plan.  Every comparison is exact.

Written for the constants packfit_oracle names: TILE = 1024 documents per workgroup of the rank pass, WAVE_DOCS = 256 consecutive
documents per wave, FILL_DOCS = 256 packed slots per workgroup of the fill; the 64-bit scan switches kernels at 8 * 2048."""
import ctypes

import numpy as np
import pytest

import pack_oracle as PO
import packfit_oracle as FO

pytestmark = pytest.mark.gpu

CELLS = ("input_ids", "attention_mask", "segment_ids", "position_ids")
MAPS = ("doc_row", "doc_col", "doc_len", "row_docs")
KEYS = CELLS + MAPS + ("row_off", "seg_off")


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


@pytest.fixture(scope="module")
def sp(tok):
    pad, bos, eos = tok._special_ids()[:3]
    return dict(pad=pad, bos=bos, eos=eos)


def same(got, want, L):
    assert sorted(got) == sorted(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    assert got["input_ids"].shape[1:] == (L,)


def counters(lengths, base=1000):
    """Bodies whose ids count up across the batch: a cell taken from the wrong place shows."""
    out, at = [], base
    for T in lengths:
        out.append(list(range(at, at + T)))
        at += T
    return out


def check_bodies(tok, sp, bodies, L, framed_too=False):
    want = FO.batch(bodies, L, fast=len(bodies) > 300, **sp)
    same(tok.pack_rows(bodies, L, framed=False, order="fit"), want, L)
    if framed_too:
        framed = [[-7] + b + [-9] for b in bodies]                   # the frame is dropped whatever it holds
        same(tok.pack_rows(framed, L, order="fit"), want, L)
    return want


# ---- rank edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FO.RANK_NS)
def test_one_length_across_every_wave_and_tile(tok, sp, n):
    """All documents one length: the rank runs through every round, wave and tile, and the rows take them in index order."""
    want = check_bodies(tok, sp, counters(FO.one_length(n, 10)), 10)
    assert want["row_docs"].tolist() == list(range(n)) and want["doc_row"].tolist() == [d // 3 for d in range(n)]


@pytest.mark.parametrize("n", [65, FO.WAVE_DOCS + 1, FO.TILE + 1, 2 * FO.TILE + 1])
def test_two_lengths_alternating(tok, sp, n):
    check_bodies(tok, sp, counters(FO.two_lengths(n)), 10)


@pytest.mark.parametrize("L,times", [(10, 1), (10, 2), (130, 1), (130, 2), (4096, 1), (4096, 2)])
def test_every_length_once_and_twice(tok, sp, L, times):
    lengths = FO.every_length(L, times)
    bodies = counters(lengths)
    want = FO.batch(bodies, L, fast=True, **sp)
    got = tok.pack_rows(bodies, L, framed=False, order="fit")
    same(got, want, L)
    assert sorted(set(want["doc_len"].tolist())) == list(range(2, L + 1))


@pytest.mark.parametrize("n", [FO.TILE - 1, FO.TILE, 2 * FO.TILE + 1, FO.SCAN_SWITCH + 1])
@pytest.mark.parametrize("L", [12, 128])
def test_random_lengths_at_tile_edges(tok, sp, n, L):
    rng = np.random.default_rng(n * 31 + L)
    bodies = counters(rng.integers(0, L + 3, size=n).tolist())
    check_bodies(tok, sp, bodies, L)


# ---- event edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", FO.EVENT_LS)
def test_events_of_every_kind(tok, sp, L):
    """Old rows filled k a row, the one partial row of a length, newly opened rows behind old ones (packfit_oracle.event_edges)."""
    check_bodies(tok, sp, counters(FO.event_edges(L)), L, framed_too=True)


@pytest.mark.parametrize("L", FO.EVENT_LS)
def test_lengths_at_the_rules_edges(tok, sp, L):
    Ts = PO.edge_lengths(L)
    check_bodies(tok, sp, counters(Ts + Ts[::-1] + [0, 0] + Ts), L)
    for T in Ts:                                                     # ... and each length as a batch of its own
        check_bodies(tok, sp, counters([T]), L)


@pytest.mark.parametrize("guard", [65, 67])
def test_outputs_off_a_16_byte_boundary(tok, sp, guard):
    """L % 4 == 0 but the outputs start 4 / 12 bytes off a 16-byte boundary: the one-cell form of the fill."""
    device_form(tok, sp, 8, guard, counters(FO.event_edges(8)))


# ---- fill edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 4, 5, 10, 127, 128])
def test_all_empty_bodies(tok, sp, L):
    """L / 2 documents a row, segment ids up to L / 2; L odd: one pad cell a row."""
    n = 3 * (L // 2) + 1
    want = check_bodies(tok, sp, [[] for _ in range(n)], L)
    assert len(want["row_off"]) - 1 == 4 and want["segment_ids"].max() == L // 2
    assert ((want["input_ids"][:3] == sp["pad"]).sum(axis=1) == L % 2).all()


@pytest.mark.parametrize("L", [6, 10, 127, 128, 130])
def test_rows_that_fill_exactly(tok, sp, L):
    """[2] * k + [L - 2] * k: exactly k full rows where next-fit makes more."""
    k = 7
    bodies = counters(FO.exact_rows(L, k))
    want = check_bodies(tok, sp, bodies, L)
    assert len(want["row_off"]) - 1 == k and (want["segment_ids"] > 0).all()
    assert len(PO.batch(bodies, L, **sp)["row_off"]) - 1 > k


@pytest.mark.parametrize("L", [4, 7, 10, 128, 130])
def test_a_tail_of_one_cell(tok, sp, L):
    want = check_bodies(tok, sp, counters(FO.one_cell_tail(L)), L)
    assert ((want["segment_ids"] == 0).sum(axis=1) == 1).all()


@pytest.mark.parametrize("L", [5, 8, 130])
def test_documents_longer_than_the_row_are_cut(tok, sp, L):
    want = check_bodies(tok, sp, counters([L - 2, 3 * L, 1, L - 1, 0, 2 * L + 1, 2]), L, framed_too=True)
    assert (want["doc_len"] == L).sum() == 4


@pytest.mark.parametrize("L", [8, 9])
def test_a_real_token_equal_to_the_pad_id(tok, sp, L):
    """The mask is 0 exactly at the pad id; segment_ids is non-zero on every real cell -- a pad id inside a body too."""
    odd = [sp["pad"], sp["bos"], sp["eos"], -1, -5, 2 ** 31 - 1, -2 ** 31, 70000, 7]
    rng = np.random.default_rng(3)
    bodies = [rng.choice(odd, size=T).tolist() for T in (0, 1, 5, 6, 7, 13, 40, 3, 2, 2, 1)] + [[sp["pad"]] * 4, [sp["pad"]], odd]
    got = tok.pack_rows(bodies, L, framed=False, order="fit")
    same(got, FO.batch(bodies, L, **sp), L)
    used = np.zeros(len(got["row_off"]) - 1, dtype=np.int64)
    np.add.at(used, got["doc_row"], got["doc_len"])
    real = np.arange(L)[None, :] < used[:, None]
    assert (got["segment_ids"][real] > 0).all() and (got["segment_ids"][~real] == 0).all() and (~real).any()
    assert ((got["attention_mask"] == 0) & real).any()


# ---- the device entry point: sizing, capacity, optional outputs ----------------------------------------------------------------------
FILL = 0x5A5A5A5A


class Guarded:
    """n cells of `dtype` on the device between two runs of guard cells, all pre-filled with FILL bytes."""

    def __init__(self, ctx, n, guard, dtype=np.int32):
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

    def free(self):
        self.ctx.free(self.base)


def device_form(tok, sp, L, guard, bodies, full=False):
    """The rows lie behind a prefix of junk (row_off_dev[0] != 0).  Sizing call; capacity R - 1 (GZ_E_CAPACITY, total = R, maps valid,
    cell arrays untouched); exact capacity; with `full`, each optional output NULL."""
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    junk = 37
    flat = np.array([-77] * junk + [v for b in bodies for v in b] + [-88] * 5, dtype=np.int32)
    ro = np.zeros(len(bodies) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bodies], out=ro[1:])
    ro += junk
    want = FO.batch(bodies, L, **sp)
    R, n = len(want["row_off"]) - 1, len(bodies)
    d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
    ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
    bufs = []

    def outputs():
        g = [Guarded(ctx, R * L, guard) for _ in CELLS] + [Guarded(ctx, n, guard) for _ in MAPS]
        g += [Guarded(ctx, n + 1, guard, np.int64), Guarded(ctx, n + 1, guard, np.int64)]
        bufs.extend(g)
        return g

    def maps_match(g, skip=()):
        for k, key in enumerate(KEYS):
            if k < 4 or k in skip:
                continue
            a = g[k].read()
            assert np.array_equal(a[:len(want[key])], want[key]), key
            assert (a[len(want[key]):] == g[k].fill).all(), key        # row_off: R + 1 entries, the rest of its n + 1 untouched
    try:
        g = outputs()
        assert ctx.pack_rows_fit_device(d_ids, d_ro, n, L, 0, 0, 0, 0, 0, 0, *[x.ptr for x in g[4:]], 0) == R          # sizing
        maps_match(g)
        assert all(x.untouched() for x in g[:4])
        g = outputs()
        with pytest.raises(_native.GzError) as e:
            ctx.pack_rows_fit_device(d_ids, d_ro, n, L, 0, 0, *[x.ptr for x in g], R - 1)
        assert e.value.code == _native.GZ_E_CAPACITY and e.value.total == R
        maps_match(g)
        assert all(x.untouched() for x in g[:4])
        assert ctx.pack_rows_fit_device(d_ids, d_ro, n, L, 0, 0, *[x.ptr for x in g], R) == R
        maps_match(g)
        for x, key in zip(g[:4], CELLS):
            assert np.array_equal(x.read().reshape(R, L), want[key]), key
        # optional outputs left out, one at a time and all at once (row_off, index 8, is not optional)
        for drop in ([1], [2], [3], [4], [5], [6], [7], [9], [1, 2, 3, 4, 5, 6, 7, 9]) if full else ():
            g = outputs()
            ptrs = [0 if k in drop else x.ptr for k, x in enumerate(g)]
            assert ctx.pack_rows_fit_device(d_ids, d_ro, n, L, 0, 0, *ptrs, R + 3) == R
            maps_match(g, skip=drop)
            for k, x in enumerate(g):
                if k in drop:
                    assert x.untouched(), KEYS[k]
                elif k < 4:
                    assert np.array_equal(x.read().reshape(R, L), want[KEYS[k]]), KEYS[k]
    finally:
        for x in bufs:
            x.free()
        for d in (d_ids, d_ro):
            ctx.free(d)


@pytest.mark.parametrize("L,guard", [(8, 64), (7, 64), (16, 64)])
def test_device_form_between_guard_cells(tok, sp, L, guard):
    device_form(tok, sp, L, guard, counters([0, 3, L - 2, L - 1, 0, 0, 5 * L + 1, 0, 1, 2 * L, 1, 1, 0, 2]), full=True)


def test_refusals_at_the_abi_leave_the_context_usable(tok, sp):
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    ro = np.array([0, 4], dtype=np.int64)
    d_ids, d_ro, d_po = ctx.alloc(16), ctx.alloc(16), ctx.alloc(16)
    try:
        ctx.h2d(d_ids, np.arange(4, dtype=np.int32)); ctx.h2d(d_ro, ro)
        for L, sf, sb in ((2, 0, 0), (4097, 0, 0), (0, 0, 0), (-1, 0, 0), (8, 2, 0), (8, 0, -1), (8, 0, 2)):
            with pytest.raises(_native.GzError) as e:
                ctx.pack_rows_fit_device(d_ids, d_ro, 1, L, sf, sb, 0, 0, 0, 0, 0, 0, 0, 0, d_po, 0, 0)
            assert e.value.code == _native.GZ_E_INVALID, (L, sf, sb)
            out = np.zeros(8, dtype=np.int32); po = np.zeros(2, dtype=np.int64); total = ctypes.c_int64()
            rc = ctx.lib.gz_pack_rows_fit(ctx.handle, _native._ptr(out), _native._ptr(ro), 1, L, sf, sb, _native._ptr(out), None, None, None,
                                          None, None, None, None, _native._ptr(po), None, 1, ctypes.byref(total))
            assert rc == _native.GZ_E_INVALID, (L, sf, sb)
        with pytest.raises(_native.GzError) as e:                        # no row_off to write to
            ctx.pack_rows_fit_device(d_ids, d_ro, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert e.value.code == _native.GZ_E_INVALID
        total = ctypes.c_int64()
        po = np.zeros(2, dtype=np.int64)
        assert ctx.lib.gz_pack_rows_fit(ctx.handle, None, None, 1, 8, 0, 0, None, None, None, None, None, None, None, None, _native._ptr(po), None, 0,
                                        ctypes.byref(total)) == _native.GZ_E_INVALID                                  # no row offsets
        assert ctx.lib.gz_pack_rows_fit(ctx.handle, None, _native._ptr(ro), 1, 8, 0, 0, None, None, None, None, None, None, None, None,
                                        _native._ptr(po), None, 0, None) == _native.GZ_E_INVALID                      # nowhere to put R
        assert ctx.lib.gz_pack_rows_fit(ctx.handle, None, _native._ptr(ro), 1, 8, 0, 0, None, None, None, None, None, None, None, None,
                                        _native._ptr(po), None, 0, ctypes.byref(total)) == _native.GZ_E_INVALID       # ids NULL with 4 entries
        assert ctx.pack_rows_fit_device(d_ids, d_ro, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_po, 0, 0) == 1
        assert ctx.pack_rows_fit_device(d_ids, d_ro, 1, 4096, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_po, 0, 0) == 1
    finally:
        for d in (d_ids, d_ro, d_po):
            ctx.free(d)
    check_bodies(tok, sp, counters([9, 0, 4]), 5)


def test_refusals_in_python_come_before_any_device_work(tok, sp):
    calls = (lambda **k: tok.pack_rows([[1, 2, 3]], **k), lambda **k: tok.encode_packs_to_device(["a b"], **k))
    for call in calls:
        for order in ("best", "", None, "FIT", 1):
            with pytest.raises(ValueError):
                call(max_len=8, order=order)
        for L in (2, 4097, 2 ** 31):
            with pytest.raises(ValueError):
                call(max_len=L, order="fit")
        with pytest.raises(TypeError):
            call(max_len=8.0, order="fit")
    for L in (2, 4097):
        with pytest.raises(ValueError):
            tok.encode_packs_fit(["a b"], L)
    assert tok.pack_rows([[1, 2, 3]], 4097, order="kept")["input_ids"].shape == (1, 4097)        # the limit is the fit order's
    check_bodies(tok, sp, counters([9]), 5)


# ---- small inputs, the default path ------------------------------------------------------------------------------------------------
def test_no_documents_and_one(tok, sp):
    got = tok.pack_rows([], 8, order="fit")
    same(got, FO.batch([], 8, **sp), 8)
    assert got["row_off"].tolist() == [0] and got["seg_off"].tolist() == [0] and got["input_ids"].shape == (0, 8)
    check_bodies(tok, sp, counters([4]), 8, framed_too=True)
    for texts in ([], [""], ["", "   ", ""]):
        want = FO.batch([[] for _ in texts], 8, **sp)
        same(tok.encode_packs_fit(texts, 8), want, 8)
        same(host(tok.encode_packs_to_device(texts, 8, order="fit")), want, 8)


def test_order_kept_is_the_call_without_the_argument(tok, sp):
    bodies = counters([3, 0, 9, 4, 4, 1, 7, 2, 30, 5])
    a, b = tok.pack_rows(bodies, 12, framed=False), tok.pack_rows(bodies, 12, framed=False, order="kept")
    assert sorted(a) == sorted(b) == sorted(set(KEYS) - {"row_docs"})
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    want = PO.batch(bodies, 12, **sp)
    for k in a:
        assert np.array_equal(a[k], want[k]), k
    texts = PO.texts(40, 9, 2)
    c, d = tok.encode_packs_to_device(texts, 16), tok.encode_packs_to_device(texts, 16, order="kept")
    e = tok.encode_packs(texts, 16)
    for k in e:
        assert np.array_equal(host(c)[k], host(d)[k]) and np.array_equal(host(c)[k], e[k]), k
    assert "row_docs" not in e and "row_docs" not in c


# ---- text, end to end; stream ordering; composition ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_rows(tok):
    texts = PO.texts(300, 14, 5)
    return texts, [tok.encode(t, False) for t in texts]


def host(dev):
    return dict(dev, **{k: dev[k].numpy() for k in CELLS})


@pytest.mark.parametrize("L", [16, 13])
def test_text_end_to_end_right_behind_the_encode(tok, sp, corpus_rows, L):
    """encode_packs_fit enqueues the fit call right behind a ragged encode with no sync in between."""
    texts, rows = corpus_rows
    want = FO.batch([r[1:-1] for r in rows], L, **sp)
    got = tok.encode_packs_fit(texts, L)
    same(got, want, L)
    if L == 16:
        same(tok.encode_packs_fit(texts, L, word_table=False), want, L)
    dev = tok.encode_packs_to_device(texts, L, order="fit")
    R = len(want["row_off"]) - 1
    assert all(dev[k].shape == (R, L) for k in CELLS) and R <= len(PO.batch([r[1:-1] for r in rows], L, **sp)["row_off"]) - 1
    same(host(dev), want, L)
    # unpack_rows gives back each text's own row without its padding, in DOCUMENT order
    flat, off = tok.unpack_rows(got)
    assert flat.dtype == np.int32 and off.tolist() == [0] + np.cumsum(want["doc_len"]).tolist()
    for r in range(0, len(texts), 7):
        one = tok(texts[r], max_len=L)["input_ids"]
        n_real = min(len(rows[r]), L)
        assert flat[off[r]:off[r + 1]].tolist() == one[:n_real]


def test_mask_rows_over_a_fit_result(tok, sp, corpus_rows):
    """mask_rows runs over the fit rows as over any dense rows: equal to mask_rows over the oracle's rows, frames and tails kept."""
    texts, rows = corpus_rows
    got = tok.encode_packs_fit(texts, 32)
    want = FO.batch([r[1:-1] for r in rows], 32, **sp)
    a = tok.mask_rows(got["input_ids"], p=0.3, seed=11)
    b = tok.mask_rows(want["input_ids"], p=0.3, seed=11)
    for k in ("input_ids", "labels", "n_chosen"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_chosen"].sum() > 0
    special = np.isin(got["input_ids"], [sp["pad"], sp["bos"], sp["eos"]])
    assert np.array_equal(a["input_ids"][special], got["input_ids"][special])            # the segment structure is intact


def test_chained_calls(tok, sp, corpus_rows):
    """A fit call, a kept call and a plain encode_to_device on one context: each result is its own."""
    texts, rows = corpus_rows
    a = tok.encode_packs_to_device(texts[:120], 16, order="fit")
    b = tok.encode_packs_to_device(texts[120:], 24)
    c = tok.encode_packs_to_device(texts[120:], 24, order="fit")
    same(host(a), FO.batch([x[1:-1] for x in rows[:120]], 16, **sp), 16)
    same(host(c), FO.batch([x[1:-1] for x in rows[120:]], 24, **sp), 24)
    wb = PO.batch([x[1:-1] for x in rows[120:]], 24, **sp)
    for k in wb:
        assert np.array_equal(host(b)[k], wb[k]), k
