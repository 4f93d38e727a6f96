"""Short documents packed into rows of max_len on the GPU (gz_pack_rows / gz_pack_rows_device; Tokenize.pack_rows, encode_packs,
encode_packs_to_device, unpack_rows) against the rule of tests/pack_oracle.py, which tests/test_pack_inputs.py ties to the
reference.  Every comparison is exact.

Written for the constants of csrc/gz_packrows.inc as pack_oracle names them: TILE = 1024 documents per tile of the break chain
(= the workgroup of the tile and mark kernels), GROUP = 16 tiles, FILL_DOCS = 256 documents per workgroup of the fill; the
per-document kernels run 256 threads a workgroup, the scan switches kernels at 8 * 2048 documents."""
import ctypes

import numpy as np
import pytest

import pack_oracle as PO

pytestmark = pytest.mark.gpu

CELLS = ("input_ids", "attention_mask", "segment_ids", "position_ids")
MAPS = ("doc_row", "doc_col", "doc_len")
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


def check_bodies(tok, sp, bodies, L, framed_too=True):
    want = PO.batch(bodies, L, **sp)
    same(tok.pack_rows(bodies, L, framed=False), want, L)
    if framed_too:
        framed = [[-7] + b + [-9] for b in bodies]                   # the frame is dropped whatever it holds
        same(tok.pack_rows(framed, L, framed=True), want, L)
    return want


@pytest.mark.parametrize("L", PO.RULE_LS)
def test_lengths_at_the_rules_edges(tok, sp, L):
    Ts = PO.edge_lengths(L)
    check_bodies(tok, sp, counters(Ts + Ts[::-1] + [0, 0] + Ts), L)
    for T in Ts:                                                     # ... and each length as a batch of its own
        check_bodies(tok, sp, counters([T]), L)
        check_bodies(tok, sp, counters([T] * 5), L, framed_too=False)


@pytest.mark.parametrize("L", PO.RULE_LS)
def test_rows_that_fill_exactly_and_one_past(tok, sp, L):
    want = check_bodies(tok, sp, counters(PO.exact_fill(L) * 3), L)
    used = np.add.reduceat(want["doc_len"], want["row_off"][:-1])
    assert (used == L).any()


@pytest.mark.parametrize("L", PO.RULE_LS)
def test_all_empty_bodies(tok, sp, L):
    """L even: L / 2 documents a row and no tail; L odd: one pad cell a row."""
    n = 3 * (L // 2) + 1
    want = check_bodies(tok, sp, [[] for _ in range(n)], L)
    assert len(want["row_off"]) - 1 == 4 and ((want["input_ids"][:3] == sp["pad"]).sum(axis=1) == L % 2).all()


@pytest.mark.parametrize("L", PO.RULE_LS)
def test_every_document_fills_its_row(tok, sp, L):
    want = check_bodies(tok, sp, counters([L - 2, L - 1, L - 2, 3 * L, L - 2]), L)
    assert want["doc_row"].tolist() == [0, 1, 2, 3, 4] and (want["segment_ids"] == 1).all()


@pytest.mark.parametrize("lead", [False, True])
def test_chains_that_never_merge(tok, sp, lead):
    """Two documents a row throughout: a pass that restarts at a tile's first document, or counts on chains from different
    entries running together, puts the heads on the wrong parity."""
    want = check_bodies(tok, sp, counters(PO.never_merge(lead)), 10, framed_too=False)
    heads = want["row_off"][1:-1]
    assert (heads % 2 == (1 if lead else 0)).all() and len(heads) > PO.TILE


def test_a_row_longer_than_a_tile(tok, sp):
    L, Ts = PO.long_row()
    want = check_bodies(tok, sp, [[] for _ in Ts], L, framed_too=False)
    assert want["row_off"].tolist() == [0, PO.TILE + 3, 2 * PO.TILE + 6, 3 * PO.TILE + 5]


def test_a_chain_that_passes_over_a_tile(tok, sp):
    L, Ts = PO.skipped_tile()
    want = check_bodies(tok, sp, [[] for _ in Ts], L, framed_too=False)
    assert want["row_off"].tolist() == [0, 2 * PO.TILE + 3, 3 * PO.TILE + 5]


def test_a_chain_that_passes_over_a_group_of_tiles(tok, sp):
    """Two rows: the second head lies in the third group, so no chain enters the second one."""
    L, n = 4 * PO.GROUP + 6, 3 * PO.GROUP + 5
    want = check_bodies(tok, sp, [[] for _ in range(n)], L, framed_too=False)
    assert want["row_off"].tolist() == [0, 2 * PO.GROUP + 3, n]


@pytest.mark.parametrize("n_rows", PO.BLOCK_EDGE_NS)
@pytest.mark.parametrize("L", PO.BLOCK_EDGE_LS)
def test_document_counts_at_block_edges(tok, sp, n_rows, L):
    rng = np.random.default_rng(n_rows * 31 + L)
    bodies = counters(rng.integers(0, 2 * L, size=n_rows).tolist())
    got = tok.pack_rows(bodies, L, framed=False)
    same(got, PO.batch(bodies, L, **sp), L)
    if n_rows == 0:
        assert got["row_off"].tolist() == [0] and got["seg_off"].tolist() == [0] and got["input_ids"].shape == (0, L)


@pytest.mark.parametrize("L", PO.ALIGN_LS)
def test_body_sources_at_every_alignment(tok, sp, L):
    check_bodies(tok, sp, counters(PO.ALIGN_LENGTHS), L)


@pytest.mark.parametrize("L", [8, 9])
def test_mask_segments_and_odd_ids(tok, sp, L):
    """The pad id, bos and eos, negative ids and ids above the vocabulary pass through; the mask is 0 exactly at the pad id;
    segment_ids is non-zero on every real cell -- a pad id inside a body too -- and 0 on every tail cell."""
    odd = [sp["pad"], sp["bos"], sp["eos"], -1, -5, 2 ** 31 - 1, -2 ** 31, 70000, tok.vocab_size(), tok.vocab_size() + 1, 7]
    rng = np.random.default_rng(3)
    bodies = [rng.choice(odd, size=T).tolist() for T in (0, 1, 5, 6, 7, 13, 40, 3, 2, 2, 1)] + [[sp["pad"]] * 4, [sp["pad"]], odd]
    want = PO.batch(bodies, L, **sp)
    got = tok.pack_rows(bodies, L, framed=False)
    same(got, want, L)
    assert np.array_equal(got["attention_mask"], (got["input_ids"] != sp["pad"]).astype(np.int32))
    used = np.add.reduceat(got["doc_len"], got["row_off"][:-1])
    real = np.arange(L)[None, :] < used[:, None]
    assert (got["segment_ids"][real] > 0).all() and (got["segment_ids"][~real] == 0).all() and (~real).any()
    assert ((got["attention_mask"] == 0) & real).any()               # real tokens equal to the pad id: mask 0, segment kept


def test_surface_framed_rows_and_two_dimensional_input(tok, sp):
    """Rows of 0 and 1 entries with framed=True have no body: bos and eos."""
    got = tok.pack_rows([[], [5], [5, 6], [5, 7, 6]], 6, framed=True)
    same(got, PO.batch([[], [], [], [7]], 6, **sp), 6)
    rows = np.arange(5 * 11, dtype=np.int64).reshape(5, 11) + 50
    same(tok.pack_rows(rows, 24), PO.batch([r[1:-1].tolist() for r in rows], 24, **sp), 24)
    same(tok.pack_rows(rows, 6), PO.batch([r[1:-1].tolist() for r in rows], 6, **sp), 6)


# ---- the device entry point ------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("L,guard", [(8, 64), (8, 65), (7, 64), (16, 67)])
def test_device_form_behind_junk_with_exact_capacity(tok, sp, L, guard):
    """The rows lie behind a prefix of junk (row_off_dev[0] != 0).  Sizing call; exact capacity; capacity R - 1 (GZ_E_CAPACITY,
    total = R, maps valid, cell arrays untouched); each optional output NULL.  guard 64: 16-byte aligned outputs; 65 / 67: the
    outputs start 4 / 12 bytes off a 16-byte boundary (the one-cell form although L % 4 == 0)."""
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    bodies = counters([0, 3, L - 2, L - 1, 0, 0, 5 * L + 1, 0, 1, 2 * L, 1, 1, 0, 2])
    junk = 37
    flat = np.array([-77] * junk + [v for b in bodies for v in b] + [-88] * 5, dtype=np.int32)
    ro = np.zeros(len(bodies) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bodies], out=ro[1:])
    ro += junk
    want = PO.batch(bodies, L, **sp)
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
        assert ctx.pack_rows_device(d_ids, d_ro, n, L, 0, 0, 0, 0, 0, 0, *[x.ptr for x in g[4:]], 0) == R          # sizing
        maps_match(g)
        assert all(x.untouched() for x in g[:4])
        # one row too few: refused, R reported, the maps valid, nothing written to the cell arrays
        g = outputs()
        with pytest.raises(_native.GzError) as e:
            ctx.pack_rows_device(d_ids, d_ro, n, L, 0, 0, *[x.ptr for x in g], R - 1)
        assert e.value.code == _native.GZ_E_CAPACITY and e.value.total == R
        maps_match(g)
        assert all(x.untouched() for x in g[:4])
        # exact capacity
        assert ctx.pack_rows_device(d_ids, d_ro, n, L, 0, 0, *[x.ptr for x in g], R) == R
        maps_match(g)
        for x, key in zip(g[:4], CELLS):
            assert np.array_equal(x.read().reshape(R, L), want[key]), key
        # optional outputs left out, one at a time and all at once (row_off, index 7, is not optional)
        for drop in ([1], [2], [3], [4], [5], [6], [8], [1, 2, 3, 4, 5, 6, 8]):
            g = outputs()
            ptrs = [0 if k in drop else x.ptr for k, x in enumerate(g)]
            assert ctx.pack_rows_device(d_ids, d_ro, n, L, 0, 0, *ptrs, R + 3) == R
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


def test_refusals_at_the_abi_leave_the_context_usable(tok, sp):
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    ro = np.array([0, 4], dtype=np.int64)
    d_ids, d_ro, d_po = ctx.alloc(16), ctx.alloc(16), ctx.alloc(16)
    try:
        ctx.h2d(d_ids, np.arange(4, dtype=np.int32)); ctx.h2d(d_ro, ro)
        for L, sf, sb in ((2, 0, 0), (0, 0, 0), (-1, 0, 0), (8, 2, 0), (8, 0, -1), (8, 0, 2)):
            with pytest.raises(_native.GzError) as e:
                ctx.pack_rows_device(d_ids, d_ro, 1, L, sf, sb, 0, 0, 0, 0, 0, 0, 0, d_po, 0, 0)
            assert e.value.code == _native.GZ_E_INVALID, (L, sf, sb)
            out = np.zeros(8, dtype=np.int32); po = np.zeros(2, dtype=np.int64); total = ctypes.c_int64()
            rc = ctx.lib.gz_pack_rows(ctx.handle, _native._ptr(out), _native._ptr(ro), 1, L, sf, sb, _native._ptr(out), None, None, None,
                                      None, None, None, _native._ptr(po), None, 1, ctypes.byref(total))
            assert rc == _native.GZ_E_INVALID, (L, sf, sb)
        with pytest.raises(_native.GzError) as e:                        # no row_off to write the heads to
            ctx.pack_rows_device(d_ids, d_ro, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert e.value.code == _native.GZ_E_INVALID
        assert ctx.pack_rows_device(d_ids, d_ro, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_po, 0, 0) == 1
    finally:
        for d in (d_ids, d_ro, d_po):
            ctx.free(d)
    check_bodies(tok, sp, counters([9, 0, 4]), 5)


def test_refusals_in_python_come_before_any_device_work(tok, sp):
    for call in (lambda **k: tok.pack_rows([[1, 2, 3]], **k), lambda **k: tok.encode_packs(["a b"], **k),
                 lambda **k: tok.encode_packs_to_device(["a b"], **k)):
        for bad in (dict(max_len=2), dict(max_len=0), dict(max_len=-4), dict(max_len=2 ** 31)):
            with pytest.raises(ValueError):
                call(**bad)
        for bad in (dict(max_len=8.0), dict(max_len=None), dict(max_len="8"), dict(max_len=True)):
            with pytest.raises(TypeError):
                call(**bad)
    for call in (tok.encode_packs, tok.encode_packs_to_device):
        for bad in (["a", 3], ["a", None], [b"a"]):
            with pytest.raises(TypeError):
                call(bad, 8)
    with pytest.raises(TypeError):
        tok.pack_rows(np.zeros((2, 4)), 8)
    same(tok.encode_packs(["a"], np.int64(8)), tok.encode_packs(["a"], 8), 8)
    check_bodies(tok, sp, counters([9]), 5)


# ---- text, end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_rows(tok):
    texts = PO.texts(300, 14, 5)
    return texts, [tok.encode(t, False) for t in texts]


def host(dev):
    return dict(dev, **{k: dev[k].numpy() for k in CELLS})


@pytest.mark.parametrize("L", [16, 32, 13])
def test_text_end_to_end(tok, sp, corpus_rows, L):
    texts, rows = corpus_rows
    assert all(r[0] == sp["bos"] and r[-1] == sp["eos"] for r in rows) and "" in texts
    want = PO.batch([r[1:-1] for r in rows], L, **sp)
    got = tok.encode_packs(texts, L)
    same(got, want, L)
    if L == 16:
        same(tok.encode_packs(texts, L, word_table=False), want, L)
    dev = tok.encode_packs_to_device(texts, L)
    R = len(want["row_off"]) - 1
    assert all(dev[k].shape == (R, L) for k in CELLS) and R < len(texts)
    same(host(dev), want, L)
    # unpack_rows gives back each text's own row without its padding; some are cut, some are not
    flat, off = tok.unpack_rows(got)
    assert flat.dtype == np.int32 and off.tolist() == want["seg_off"].tolist()
    cut = 0
    for r in range(0, len(texts), 7):
        one = tok(texts[r], max_len=L)["input_ids"]
        n_real = min(len(rows[r]), L)
        assert flat[off[r]:off[r + 1]].tolist() == one[:n_real] and one[n_real:] == [sp["pad"]] * (L - n_real)
        cut += len(rows[r]) > L
    assert 0 < cut < len(range(0, len(texts), 7))


def test_no_texts_and_empty_texts(tok, sp):
    for texts in ([], [""], ["", "   ", ""]):
        want = PO.batch([[] for _ in texts], 8, **sp)
        same(tok.encode_packs(texts, 8), want, 8)
        same(host(tok.encode_packs_to_device(texts, 8)), want, 8)
        flat, off = tok.unpack_rows(want)
        assert flat.tolist() == [sp["bos"], sp["eos"]] * len(texts) and off.tolist() == [2 * k for k in range(len(texts) + 1)]


def test_chained_calls(tok, sp, corpus_rows):
    """Two pack calls with different batches, then a plain encode_to_device, on one context: each result is its own."""
    texts, rows = corpus_rows
    a_t, b_t = texts[:120], texts[120:]
    a = tok.encode_packs_to_device(a_t, 16)
    b = tok.encode_packs_to_device(b_t, 24)
    c = tok.encode_to_device(a_t, max_len=16)
    for r, lo, hi, L in ((a, 0, 120, 16), (b, 120, 300, 24)):
        same(host(r), PO.batch([x[1:-1] for x in rows[lo:hi]], L, **sp), L)
    assert np.array_equal(c["input_ids"].numpy(), tok.encode_batch(a_t, max_len=16)["input_ids"])
