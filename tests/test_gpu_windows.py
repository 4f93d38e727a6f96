"""Overlapping max_len windows on the GPU (gz_window_rows / gz_window_rows_device; Tokenize.window_rows, encode_windows,
encode_windows_to_device, join_windows) against the rule of tests/window_oracle.py, which tests/test_window_inputs.py ties to
the reference.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import window_oracle as WO

pytestmark = pytest.mark.gpu

KEYS = ("input_ids", "attention_mask", "doc", "start", "n_real", "win_off")


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


def check_bodies(tok, sp, bodies, L, s):
    want = WO.batch(bodies, L, s, **sp)
    same(tok.window_rows(bodies, L, s, framed=False), want, L)
    framed = [[-7] + b + [-9] for b in bodies]                       # the frame is dropped whatever it holds
    same(tok.window_rows(framed, L, s, framed=True), want, L)


@pytest.mark.parametrize("L,s", WO.RULE_CASES)
def test_lengths_at_the_rules_edges(tok, sp, L, s):
    Ts = WO.edge_lengths(L, s)
    check_bodies(tok, sp, counters(Ts), L, s)
    for T in Ts:                                                     # ... and each length as a batch of its own
        check_bodies(tok, sp, counters([T]), L, s)


def test_framed_rows_shorter_than_their_frame(tok, sp):
    """Rows of 0 and 1 entries with framed=True have no body: one window of bos, eos and padding."""
    got = tok.window_rows([[], [5], [5, 6], [5, 7, 6]], 6, 1, framed=True)
    same(got, WO.batch([[], [], [], [7]], 6, 1, **sp), 6)


@pytest.mark.parametrize("L,s", WO.ALIGN_CASES)
def test_chunk_sources_at_every_alignment(tok, sp, L, s):
    check_bodies(tok, sp, counters(WO.ALIGN_LENGTHS), L, s)


@pytest.mark.parametrize("L,s", [(8, 5), (64, 0)])
def test_many_windows_from_one_row(tok, sp, L, s):
    bodies = counters([0, 1, 0, 5000, 0, 1, 1, 0], base=-2500)
    want = WO.batch(bodies, L, s, **sp)
    got = tok.window_rows(bodies, L, s, framed=False)
    if (L, s) == (8, 5):
        assert want["win_off"].tolist() == [0, 1, 2, 3, 4998, 4999, 5000, 5001, 5002]
    same(got, want, L)
    k, step = want["win_off"], L - 2 - s
    assert (got["doc"][k[3]:k[4]] == 3).all() and got["start"][k[3]:k[4]].tolist() == list(range(0, int(k[4] - k[3]) * step, step))


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 256, 257, 1025])
@pytest.mark.parametrize("L,s", [(12, 3), (7, 2)])
def test_row_counts_at_block_edges(tok, sp, n_rows, L, s):
    rng = np.random.default_rng(n_rows * 31 + L)
    lengths = rng.integers(0, 4 * (L - 2), size=n_rows).tolist()
    for k in range(0, n_rows, 5):
        lengths[k] = 0 if k % 2 else L - 2
    bodies = counters(lengths)
    got = tok.window_rows(bodies, L, s, framed=False)
    same(got, WO.batch(bodies, L, s, **sp), L)
    if n_rows == 0:
        assert got["win_off"].tolist() == [0] and got["input_ids"].shape == (0, L) and got["doc"].shape == (0,)


def test_two_dimensional_input(tok, sp):
    rows = np.arange(5 * 11, dtype=np.int64).reshape(5, 11) + 50
    got = tok.window_rows(rows, 6, 2, framed=True)
    same(got, WO.batch([r[1:-1].tolist() for r in rows], 6, 2, **sp), 6)


@pytest.mark.parametrize("L,s", [(8, 0), (9, 3)])
def test_mask_and_odd_ids(tok, sp, L, s):
    """The pad id, bos and eos, negative ids and ids above the vocabulary pass through; the mask is 0 exactly at the pad id."""
    odd = [sp["pad"], sp["bos"], sp["eos"], -1, -5, 2 ** 31 - 1, -2 ** 31, 70000, tok.vocab_size(), tok.vocab_size() + 1, 7]
    rng = np.random.default_rng(3)
    bodies = [rng.choice(odd, size=T).tolist() for T in (0, 1, 5, 6, 7, 13, 40, 3)] + [[sp["pad"]] * 9, odd]
    want = WO.batch(bodies, L, s, **sp)
    got = tok.window_rows(bodies, L, s, framed=False)
    same(got, want, L)
    assert np.array_equal(got["attention_mask"], (got["input_ids"] != sp["pad"]).astype(np.int32))
    real = np.arange(L)[None, :] < got["n_real"][:, None]
    assert ((got["attention_mask"] == 0) & real).any()               # real tokens equal to the pad id: mask 0 there too


# ---- the device entry point ------------------------------------------------------------------------------------------
FILL = 0x5A5A5A5A


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

    def free(self):
        self.ctx.free(self.base)


@pytest.mark.parametrize("L,s,guard", [(8, 2, 64), (8, 2, 65), (7, 0, 64), (16, 13, 67)])
def test_device_form_behind_junk_with_exact_capacity(tok, sp, L, s, guard):
    """The rows lie behind a prefix of junk (row_off_dev[0] != 0).  Sizing call; exact capacity; capacity W - 1 (GZ_E_CAPACITY,
    total = W, outputs untouched); NULL optional outputs.  guard 64: 16-byte aligned outputs; 65 / 67: the outputs start off
    a 16-byte boundary."""
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    bodies = counters([0, 3, L - 2, L - 1, 5 * L + 1, 0, 1, 2 * L])
    junk = 37
    flat = np.array([-77] * junk + [v for b in bodies for v in b] + [-88] * 5, dtype=np.int32)
    ro = np.zeros(len(bodies) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bodies], out=ro[1:])
    ro += junk
    want = WO.batch(bodies, L, s, **sp)
    W, n = len(want["doc"]), len(bodies)
    d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
    ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
    d_wo = ctx.alloc(8 * (n + 1))
    bufs = []
    try:
        assert ctx.window_rows_device(d_ids, d_ro, n, L, s, 0, 0, 0, 0, 0, 0, 0, d_wo, 0) == W          # sizing
        wo = np.empty(n + 1, dtype=np.int64); ctx.d2h(wo, d_wo)
        assert wo.tolist() == want["win_off"].tolist()

        def outputs():
            g = [Guarded(ctx, W * L, guard), Guarded(ctx, W * L, guard), Guarded(ctx, W, guard), Guarded(ctx, W, guard), Guarded(ctx, W, guard)]
            bufs.extend(g)
            return g
        # one window too few: refused, W reported, win_off valid, nothing else written
        g = outputs()
        ctx.h2d(d_wo, np.full(n + 1, -1, dtype=np.int64))
        with pytest.raises(_native.GzError) as e:
            ctx.window_rows_device(d_ids, d_ro, n, L, s, 0, 0, *[x.ptr for x in g], d_wo, W - 1)
        assert e.value.code == _native.GZ_E_CAPACITY and e.value.total == W
        ctx.d2h(wo, d_wo)
        assert wo.tolist() == want["win_off"].tolist()
        for x in g:
            assert (x.read() == FILL).all()
        # exact capacity
        assert ctx.window_rows_device(d_ids, d_ro, n, L, s, 0, 0, *[x.ptr for x in g], d_wo, W) == W
        got = dict(input_ids=g[0].read().reshape(W, L), attention_mask=g[1].read().reshape(W, L), doc=g[2].read(), start=g[3].read(),
                   n_real=g[4].read(), win_off=wo)
        same(got, want, L)
        # optional outputs left out, one at a time and all at once
        for drop in ([1], [2], [3], [4], [1, 2, 3, 4]):
            g = outputs()
            ptrs = [0 if k in drop else x.ptr for k, x in enumerate(g)]
            assert ctx.window_rows_device(d_ids, d_ro, n, L, s, 0, 0, *ptrs, d_wo, W + 3) == W
            for k, (x, key) in enumerate(zip(g, KEYS)):
                a = x.read()
                if k in drop:
                    assert (a == FILL).all()
                else:
                    assert np.array_equal(a.reshape(want[key].shape), want[key]), key
    finally:
        for x in bufs:
            x.free()
        for d in (d_ids, d_ro, d_wo):
            ctx.free(d)


def test_refusals_at_the_abi_leave_the_context_usable(tok, sp):
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    ro = np.array([0, 4], dtype=np.int64)
    d_ids, d_ro, d_wo = ctx.alloc(16), ctx.alloc(16), ctx.alloc(16)
    try:
        ctx.h2d(d_ids, np.arange(4, dtype=np.int32)); ctx.h2d(d_ro, ro)
        for L, s in ((2, 0), (0, 0), (-1, 0), (8, 6), (8, -1), (3, 1)):
            with pytest.raises(_native.GzError) as e:
                ctx.window_rows_device(d_ids, d_ro, 1, L, s, 0, 0, 0, 0, 0, 0, 0, d_wo, 0)
            assert e.value.code == _native.GZ_E_INVALID, (L, s)
            out = np.zeros(8, dtype=np.int32); wo = np.zeros(2, dtype=np.int64); total = ctypes.c_int64()
            rc = ctx.lib.gz_window_rows(ctx.handle, _native._ptr(out), _native._ptr(ro), 1, L, s, 0, 0, _native._ptr(out), None, None, None,
                                        None, _native._ptr(wo), 1, ctypes.byref(total))
            assert rc == _native.GZ_E_INVALID, (L, s)
        assert ctx.window_rows_device(d_ids, d_ro, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, d_wo, 0) == 4
    finally:
        for d in (d_ids, d_ro, d_wo):
            ctx.free(d)
    check_bodies(tok, sp, counters([9, 0, 4]), 5, 2)


def test_refusals_in_python_come_before_any_device_work(tok, sp):
    for call in (lambda **k: tok.window_rows([[1, 2, 3]], **k), lambda **k: tok.encode_windows(["a b"], **k),
                 lambda **k: tok.encode_windows_to_device(["a b"], **k)):
        for bad in (dict(max_len=2), dict(max_len=0), dict(max_len=-4), dict(max_len=8, stride=6), dict(max_len=8, stride=-1),
                    dict(max_len=3, stride=1)):
            with pytest.raises(ValueError):
                call(**bad)
        for bad in (dict(max_len=8.0), dict(max_len=None), dict(max_len="8"), dict(max_len=8, stride=1.5), dict(max_len=8, stride=None),
                    dict(max_len=True)):
            with pytest.raises(TypeError):
                call(**bad)
    for call in (tok.encode_windows, tok.encode_windows_to_device):
        for bad in (["a", 3], ["a", None], [b"a"]):
            with pytest.raises(TypeError):
                call(bad, 8)
    with pytest.raises(TypeError):
        tok.window_rows(np.zeros((2, 4)), 8)
    same(tok.encode_windows(["a"], np.int64(8), np.int32(0)), tok.encode_windows(["a"], 8), 8)
    check_bodies(tok, sp, counters([9]), 5, 2)


# ---- text, end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_rows(tok):
    texts = WO.texts(300, 60, 5)
    r = tok.encode_batch(texts, max_len=None)
    ro = r["row_off"]
    return texts, [r["input_ids"][ro[i]:ro[i + 1]].tolist() for i in range(len(texts))]


def capsule_shape(arr):
    """(shape, data pointer) out of the DLManagedTensor of arr.__dlpack__() (dlpack.h: data, device, ndim, dtype, shape, ...)."""
    class DLTensor(ctypes.Structure):
        _fields_ = [("data", ctypes.c_void_p), ("device_type", ctypes.c_int32), ("device_id", ctypes.c_int32), ("ndim", ctypes.c_int32),
                    ("code", ctypes.c_uint8), ("bits", ctypes.c_uint8), ("lanes", ctypes.c_uint16), ("shape", ctypes.POINTER(ctypes.c_int64)),
                    ("strides", ctypes.POINTER(ctypes.c_int64)), ("byte_offset", ctypes.c_uint64)]
    cap = arr.__dlpack__()
    get = ctypes.pythonapi.PyCapsule_GetPointer
    get.restype, get.argtypes = ctypes.c_void_p, [ctypes.py_object, ctypes.c_char_p]
    t = DLTensor.from_address(get(cap, b"dltensor"))
    out = (tuple(t.shape[k] for k in range(t.ndim)), t.data, t.bits, t.device_type)
    del cap
    return out


@pytest.mark.parametrize("L,s", [(16, 4), (32, 0), (13, 10)])
def test_text_end_to_end(tok, sp, corpus_rows, L, s):
    texts, rows = corpus_rows
    assert all(r[0] == sp["bos"] and r[-1] == sp["eos"] for r in rows)
    bodies = [r[1:-1] for r in rows]
    want = WO.batch(bodies, L, s, **sp)
    got = tok.encode_windows(texts, L, s)
    same(got, want, L)
    if L == 16:
        same(tok.encode_windows(texts, L, s, word_table=False), want, L)
    dev = tok.encode_windows_to_device(texts, L, s)
    W = len(want["doc"])
    assert dev["input_ids"].shape == (W, L) and dev["attention_mask"].shape == (W, L)
    shape, data, bits, devtype = capsule_shape(dev["input_ids"])
    assert shape == (W, L) and data == dev["input_ids"].ptr and bits == 32 and devtype == 10
    same(dict(dev, input_ids=dev["input_ids"].numpy(), attention_mask=dev["attention_mask"].numpy()), want, L)
    # window 0 is the dense call's row; a text that fits has one window
    dense = tok.encode_batch(texts, max_len=L)
    first = got["win_off"][:-1]
    assert np.array_equal(got["input_ids"][first], dense["input_ids"]) and np.array_equal(got["attention_mask"][first], dense["attention_mask"])
    n_win = np.diff(got["win_off"])
    fits = np.array([len(b) <= L - 2 for b in bodies])
    assert fits.any() and (~fits).any() and (n_win[fits] == 1).all() and (n_win[~fits] > 1).all()
    # join_windows gives the bodies back
    flat, ro = tok.join_windows(got, s)
    assert flat.dtype == np.int32 and ro.tolist() == [0] + np.cumsum([len(b) for b in bodies]).tolist()
    assert flat.tolist() == [v for b in bodies for v in b]


def test_no_texts_and_empty_texts(tok, sp):
    for texts in ([], [""], ["", "   ", ""]):
        want = WO.batch([[] for _ in texts], 8, 2, **sp)
        same(tok.encode_windows(texts, 8, 2), want, 8)
        dev = tok.encode_windows_to_device(texts, 8, 2)
        same(dict(dev, input_ids=dev["input_ids"].numpy(), attention_mask=dev["attention_mask"].numpy()), want, 8)
        flat, ro = tok.join_windows(want, 2)
        assert flat.shape == (0,) and ro.tolist() == [0] * (len(texts) + 1)


def test_chained_calls(tok, sp, corpus_rows):
    """Two window calls with different batches, then a plain encode_to_device, on one context: each result is its own."""
    texts, rows = corpus_rows
    a_t, b_t = texts[:120], texts[120:]
    a = tok.encode_windows_to_device(a_t, 16, 4)
    b = tok.encode_windows_to_device(b_t, 24, 21)
    c = tok.encode_to_device(a_t, max_len=16)
    for r, lo, hi, L, s in ((a, 0, 120, 16, 4), (b, 120, 300, 24, 21)):
        want = WO.batch([x[1:-1] for x in rows[lo:hi]], L, s, **sp)
        same(dict(r, input_ids=r["input_ids"].numpy(), attention_mask=r["attention_mask"].numpy()), want, L)
    assert np.array_equal(c["input_ids"].numpy(), a["input_ids"].numpy()[a["win_off"][:-1]])
    assert np.array_equal(c["input_ids"].numpy(), tok.encode_batch(a_t, max_len=16)["input_ids"])
