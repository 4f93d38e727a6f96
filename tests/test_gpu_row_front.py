"""The row front of csrc/gz_rows_api.inc on the GPU: the host forms of the row-shaping calls share one staging path and one set of
workspace buffers, so what is checked here is what sharing could break -- a stale, aliased or wrongly sized shared buffer, offsets
that do not start at 0, the order of the refusals, and outputs the caller leaves out.  The oracles are the calls' own
(window_oracle, pack_oracle, mask_oracle, infill_oracle, gz_oracle.decode); every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import gz_oracle as O
import infill_oracle as IO
import mask_oracle as MO
import pack_oracle as PO
import window_oracle as WO
from conftest import DATA

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
WINDOW_RULE = "windows need max_len >= 3, 0 <= stride <= max_len - 3 and skips of 0 or 1"
MASK_RULE = ("masked rows need row_len >= 1, n_rows >= 0, row_base >= 0, (row_base + n_rows) * row_len < 2^63, thresholds in "
             "[0, 2^32] with t1 <= t2, rand_lo < rand_hi and whole_word 0 or 1")
MASK_OVERLAP = "masked rows need ids, input_ids and labels, and buffers that do not overlap"


def new_tok():
    from genz_tokenize import Tokenize
    t = Tokenize()
    t._sync_tables()                                                  # (tables and decoder snapshot are on the device from here on)
    return t


@pytest.fixture(scope="module")
def tok():
    return new_tok()


@pytest.fixture(scope="module")
def env(tok):
    pad, bos, eos, mask = tok._special_ids()[:4]
    return dict(pad=pad, bos=bos, eos=eos, mask=mask, cont=MO.continuation_ids(DATA + "/vocab.txt"), n_ids=tok.vocab_size())


def framed_rows(env, rng, R, L):
    """random vocabulary ids, half of them continuation pieces, each row [bos] body [eos] pad*"""
    ids = np.where(rng.random((R, L)) < 0.5, rng.choice(env["cont"], (R, L)), rng.integers(5, env["n_ids"], (R, L)))
    n = rng.integers(0, L - 1, R)
    cols = np.arange(L)[None, :]
    ids = np.where(cols == 0, env["bos"], np.where(cols == (n + 1)[:, None], env["eos"], np.where(cols > (n + 1)[:, None], env["pad"], ids)))
    return ids.astype(np.int32)


def counters(lengths, base=1000):
    out, at = [], base
    for T in lengths:
        out.append(list(range(at, at + T)))
        at += T
    return out


def same(got, want, keys=None):
    for k in (keys or want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())


def mask_want(env, ids, p, seed):
    t_sel, t1, t2 = MO.thresholds(p, 0.8, 0.1)
    return MO.mask(ids, env["cont"], env["pad"], env["bos"], env["eos"], env["mask"], seed=seed, t_sel=t_sel, t1=t1, t2=t2, rand_lo=5,
                   rand_hi=env["n_ids"], whole_word=True, row_base=0, ignore_index=-100)


def infill_want(env, ids, p, seed, dec_width=None):
    t_start, len_t, n_len = IO.rule_ints(p, 3.0, 10, "geometric")
    return IO.infill(ids, env["cont"], env["pad"], env["bos"], env["eos"], env["mask"], seed=seed, t_start=t_start, len_t=len_t, n_len=n_len,
                     whole_word=True, row_base=0, ignore_index=-100, dec_width=dec_width)


# ---- shared workspace -----------------------------------------------------------------------------------------------------
def test_host_forms_one_after_the_other_on_one_object(tok, env, oracle_tables):
    """Every host form stages through the same buffers: each result is its oracle's whatever ran before it, and a small call behind
    larger ones equals the same call on a fresh object (nothing stale, nothing aliased, no size kept from a larger buffer)."""
    sp = dict(pad=env["pad"], bos=env["bos"], eos=env["eos"])
    rng = np.random.default_rng(11)
    ids40, ids5, ids2 = framed_rows(env, rng, 40, 7), framed_rows(env, rng, 5, 8), framed_rows(env, rng, 2, 8)
    got = tok.mask_rows(ids40, p=0.4, seed=3)                         # L = 7: one cell a lane, rows straddle the 64-lane trips
    same(got, mask_want(env, ids40, 0.4, 3))
    assert got["n_chosen"].sum() > 0
    bodies = counters([0, 5, 23])
    same(tok.window_rows(bodies, 8, 2, framed=False), WO.batch(bodies, 8, 2, **sp))
    same(tok.infill_rows(ids5, p=0.5, seed=5), infill_want(env, ids5, 0.5, 5))            # L = 8: 16-byte aligned rows
    bodies = counters([3, 0, 6, 1, 9, 2])
    same(tok.pack_rows(bodies, 8, framed=False), PO.batch(bodies, 8, **sp))
    rows = [[env["bos"], 770, 1444, env["eos"]], [], [env["bos"]] + list(range(5, 90)) + [env["eos"]]]
    assert tok.decode_batch(rows) == [O.decode(r, oracle_tables) for r in rows]
    again = tok.mask_rows(ids2, p=0.4, seed=9)
    same(again, mask_want(env, ids2, 0.4, 9))
    same(again, new_tok().mask_rows(ids2, p=0.4, seed=9))


# ---- offsets with a base --------------------------------------------------------------------------------------------------
def test_host_offsets_that_do_not_start_at_zero(tok):
    """row_off[0] = 3 behind three junk ids: the host forms stage ids[row_off[0]:] and bias the device pointer, so the result is
    the one of the arrays without the prefix.  (The device forms: test_device_form_behind_junk_with_exact_capacity of
    test_gpu_windows.py and test_gpu_packs.py.)"""
    ctx = tok._ctx
    bodies = counters([4, 0, 17, 9], base=6)
    flat = np.array([v for b in bodies for v in b], dtype=np.int32)
    off = np.zeros(len(bodies) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bodies], out=off[1:])
    junk = np.concatenate([np.array([-77, 2 ** 31 - 1, 0], dtype=np.int32), flat])
    same(ctx.window_rows(junk, off + 3, 8, 2, False), ctx.window_rows(flat, off, 8, 2, False))
    same(ctx.pack_rows(junk, off + 3, 8, False), ctx.pack_rows(flat, off, 8, False))
    data, out_off = ctx.decode(flat, off, b"<unk>")
    data3, out_off3 = ctx.decode(junk, off + 3, b"<unk>")
    assert data.tobytes() == data3.tobytes() and len(data) > 0 and np.array_equal(out_off, out_off3)


# ---- refusal precedence through ctypes ------------------------------------------------------------------------------------
def test_which_refusal_a_call_with_several_faults_reports(tok, env):
    from genz_tokenize import _native
    lib, h = _native.load_library(), tok._ctx.handle
    ptr = _native._ptr

    def last():
        return lib.gz_last_error(h).decode("utf-8")
    ids = np.arange(16, dtype=np.int32) + 100
    falling = np.array([0, 9, 4, 12], dtype=np.int64)                 # a decreasing pair
    win_off, total = np.zeros(4, dtype=np.int64), C.c_int64(-1)

    def window(L):
        return lib.gz_window_rows(h, ptr(ids), ptr(falling), 3, L, 0, 0, 0, None, None, None, None, None, ptr(win_off), 0, C.byref(total))
    assert window(2) == _native.GZ_E_INVALID and last() == WINDOW_RULE                    # the rule comes before the offsets
    assert window(8) == _native.GZ_E_INVALID and last() == "row offsets must not decrease"

    rows = framed_rows(env, np.random.default_rng(2), 4, 8)
    out, cnt = np.empty_like(rows), np.empty(4, dtype=np.int32)
    t_sel, t1, t2 = MO.thresholds(0.15, 0.8, 0.1)

    def mask(whole_word):                                             # input_ids and labels are one array
        return lib.gz_mask_rows(h, ptr(rows), 4, 8, 0, 0, t_sel, t1, t2, 5, env["n_ids"], env["mask"], whole_word, -100, ptr(out), ptr(out),
                                ptr(cnt))
    assert mask(2) == _native.GZ_E_INVALID and last() == MASK_RULE                        # the rule comes before the buffers
    assert mask(1) == _native.GZ_E_INVALID and last() == MASK_OVERLAP

    len_t = np.zeros(1, dtype=np.uint64)
    assert lib.gz_infill_rows(h, None, 0, 8, 0, 0, 0, ptr(len_t), 1, env["mask"], 1, -100, 8, None, None, None, None, None, None,
                              None) == _native.GZ_OK                                      # no rows: no buffer is looked at

    row_off, pack_off = np.zeros(1, dtype=np.int64), np.full(1, -1, dtype=np.int64)
    assert lib.gz_pack_rows(h, None, ptr(row_off), 0, 8, 0, 0, None, None, None, None, None, None, None, ptr(pack_off), None, 0,
                            C.byref(total)) == _native.GZ_OK
    assert total.value == 0 and pack_off[0] == 0


# ---- optional outputs absent ----------------------------------------------------------------------------------------------
def carve(sizes, guard=16):
    """int32 views of the given sizes inside ONE host allocation pre-filled with FILL, guard cells around each; the allocation"""
    whole = np.full(sum(sizes) + guard * (len(sizes) + 1), FILL, dtype=np.int32)
    views, at = [], guard
    for n in sizes:
        views.append(whole[at:at + n])
        at += n + guard
    return whole, views


def untouched(whole, views):
    """every cell of the allocation outside the views still holds FILL"""
    keep = np.ones(whole.shape, dtype=bool)
    for v in views:
        lo = (v.__array_interface__["data"][0] - whole.__array_interface__["data"][0]) // 4
        keep[lo:lo + v.size] = False
    return bool((whole[keep] == FILL).all())


def test_window_rows_without_mask_doc_and_n_real(tok):
    from genz_tokenize import _native
    lib, ctx, ptr = _native.load_library(), tok._ctx, _native._ptr
    bodies = counters([0, 5, 23, 6])
    flat = np.array([v for b in bodies for v in b], dtype=np.int32)
    off = np.zeros(len(bodies) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bodies], out=off[1:])
    full = ctx.window_rows(flat, off, 8, 2, False)
    W = len(full["doc"])
    assert W > len(bodies)
    whole, (out_ids, start) = carve([W * 8, W])
    win_off, total = np.zeros(len(bodies) + 1, dtype=np.int64), C.c_int64()
    ctx._check(lib.gz_window_rows(ctx.handle, ptr(flat), ptr(off), len(bodies), 8, 2, 0, 0, ptr(out_ids), None, None, ptr(start), None,
                                  ptr(win_off), W, C.byref(total)))
    assert total.value == W and np.array_equal(win_off, full["win_off"])
    assert np.array_equal(out_ids.reshape(W, 8), full["input_ids"]) and np.array_equal(start, full["start"])
    assert untouched(whole, (out_ids, start))


def test_infill_rows_with_dec_len_alone(tok, env):
    from genz_tokenize import _native
    lib, ctx, ptr = _native.load_library(), tok._ctx, _native._ptr
    R, L = 5, 8
    ids = framed_rows(env, np.random.default_rng(4), R, L)
    t_start, len_t, n_len = IO.rule_ints(0.5, 3.0, 10, "geometric")
    rule = (7, t_start, len_t, n_len, env["mask"], 1, -100, L)
    full = ctx.infill_rows(ids, rule)
    same(full, infill_want(env, ids, 0.5, 7))
    args, keep = ctx._infill_args(rule)
    whole, (out_ids, labels, dec_len) = carve([R * L, R * L, R])
    ctx._check(lib.gz_infill_rows(ctx.handle, ptr(ids), R, L, 0, *args, ptr(out_ids), None, ptr(labels), None, None, ptr(dec_len), None))
    del keep
    assert np.array_equal(out_ids.reshape(R, L), full["input_ids"]) and np.array_equal(labels.reshape(R, L), full["labels"])
    assert np.array_equal(dec_len, full["dec_len"]) and full["dec_len"].max() > 1
    assert untouched(whole, (out_ids, labels, dec_len))
