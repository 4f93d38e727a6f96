"""Span-corruption inputs and targets on the GPU (gz_infill_rows / gz_infill_rows_device; Tokenize.infill_rows,
infill_rows_to_device) against the rule of tests/infill_oracle.py, which tests/test_infill_inputs.py ties to a second restatement.
Every comparison with the oracle is exact, on all seven outputs.

Written for csrc/gz_infill.inc: every workgroup stages the continuation bitmap in LDS (switch mask_lds = 0: read from memory); a
wave walks its rows' cells in trips of 64 cells, one a lane, and takes about 4096 cells, so several rows share a trip when L < 64,
a row spans trips when L > 64, and 257 rows of any L here are more than one wave and, from L = 64 on, more than one workgroup."""
import ctypes

import numpy as np
import pytest

import infill_oracle as IO
import mask_oracle as MO
from conftest import DATA

pytestmark = pytest.mark.gpu

KEYS = IO.KEYS
LS = (1, 2, 3, 5, 63, 64, 65, 127, 128, 130, 200)
RS = (0, 1, 2, 63, 64, 65, 257)
ONE = 2 ** 32


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


@pytest.fixture(scope="module")
def env(tok):
    """the special ids, the snapshot's size, the continuation ids (from the vocab file, not from the product), the plain ids"""
    pad, bos, eos, mask = tok._special_ids()[:4]
    cont = MO.continuation_ids(DATA + "/vocab.txt")
    n_ids = tok.vocab_size()
    plain = np.setdiff1d(np.arange(5, n_ids), cont)
    return dict(pad=pad, bos=bos, eos=eos, mask=mask, cont=cont, n_ids=n_ids, plain=plain)


def want_of(env, ids, p=0.15, mean_span=3.0, max_span=10, lengths="geometric", seed=0, whole_word=True, dec_len=None, row_base=0,
            ignore_index=-100):
    t_start, len_t, n_len = IO.rule_ints(p, mean_span, max_span, lengths)
    return IO.infill(ids, env["cont"], env["pad"], env["bos"], env["eos"], env["mask"], seed=seed, t_start=t_start, len_t=len_t, n_len=n_len,
                     whole_word=whole_word, row_base=row_base, ignore_index=ignore_index, dec_width=dec_len)


def same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())


def check(tok, env, ids, **kw):
    want = want_of(env, ids, **kw)
    same(tok.infill_rows(ids, **kw), want)
    return want


def check_raw(tok, env, ids, seed, t_start, len_t, n_len, whole_word=True, dec_width=None, row_base=0):
    """through _native.Context.infill_rows: any thresholds"""
    W = ids.shape[1] if dec_width is None else dec_width
    want = IO.infill(ids, env["cont"], env["pad"], env["bos"], env["eos"], env["mask"], seed=seed, t_start=t_start, len_t=len_t, n_len=n_len,
                     whole_word=whole_word, row_base=row_base, dec_width=W)
    tok._sync_tables()
    same(tok._ctx.infill_rows(ids, (seed, t_start, len_t, n_len, env["mask"], int(whole_word), -100, W), row_base), want)
    return want


def framed_rows(env, rng, R, L):
    """random vocabulary ids, half of them continuation pieces, each row [bos] body [eos] pad*"""
    ids = np.where(rng.random((R, L)) < 0.5, rng.choice(env["cont"], (R, L)), rng.integers(5, env["n_ids"], (R, L)))
    if L >= 3:
        n = rng.integers(0, L - 1, R)                                # body length 0 .. L - 2
        cols = np.arange(L)[None, :]
        ids = np.where(cols == 0, env["bos"], np.where(cols == (n + 1)[:, None], env["eos"], np.where(cols > (n + 1)[:, None], env["pad"], ids)))
    return ids.astype(np.int32)


def widths(L):
    return (1, max(1, L // 2), L, L + 2)


@pytest.mark.parametrize("L", LS)
def test_row_lengths_and_row_counts_at_trip_and_wave_edges(tok, env, L):
    rng = np.random.default_rng(100 + L)
    for i, R in enumerate(RS):
        ids = framed_rows(env, rng, R, L)
        for ww in (True, False):
            for W in (widths(L) if R == 65 else widths(L)[(i + ww) % 4:][:1]):
                want = check(tok, env, ids, p=0.4, seed=7 * L + R, whole_word=ww, dec_len=W)
                if R >= 63 and L >= 5:
                    assert 0 < want["n_spans"].sum() and (want["enc_len"] < (ids != env["pad"]).sum(axis=1)).any()


def test_continuation_bits_read_from_memory_give_the_same(tok, env):
    """switch mask_lds = 0: the bitmap is not staged in LDS (the path of a vocabulary too large for it)"""
    from genz_tokenize import _native
    rng = np.random.default_rng(21)
    _native.debug_set("mask_lds", 0, tok._ctx)
    try:
        for R, L in ((70, 128), (70, 65), (3, 200), (130, 7)):
            check(tok, env, framed_rows(env, rng, R, L), p=0.4, seed=R + L, dec_len=max(1, L // 2))
        ids, _ = long_rows(env)
        check(tok, env, ids, p=0.3, seed=2, lengths="fixed", mean_span=3, max_span=3)
    finally:
        _native.debug_set("mask_lds", 1, tok._ctx)


@pytest.mark.parametrize("L", [3, 63, 65])
def test_a_span_does_not_continue_into_the_next_row(tok, env, L):
    """rows without a protected cell, spans of 16 tokens: a span that reaches its row's last cell ends there -- in the middle of a
    trip (L = 3, 63: the next row's cells are the next lanes) or where the carries would hand it on (L = 65)"""
    rng = np.random.default_rng(30 + L)
    ids = rng.choice(env["plain"], (140, L)).astype(np.int32)
    t_start = ONE // 40 if L > 3 else ONE // 4
    cut = 0
    for seed in range(3):
        want = check_raw(tok, env, ids, seed, t_start, [0] * 15, 16, whole_word=False, dec_width=L + 2)
        _, _, n, chosen = IO.chosen_cells(ids, env["cont"], (env["pad"], env["bos"], env["eos"], env["mask"]), seed, t_start, [0] * 15, 16, False, 0)
        x0 = MO.draw(np.arange(ids.size, dtype=np.uint64).reshape(ids.shape), seed)[0]
        begins = x0 < np.uint64(t_start)
        # rows whose last cell lies in a span that had words left, and whose successor's first cell begins none: that cell stays
        for r in range(len(ids) - 1):
            tail = begins[r, max(0, L - 15):]
            if tail.any() and not begins[r + 1, :1].any():
                assert chosen[r, L - 1] and not chosen[r + 1, 0]
                assert want["input_ids"][r + 1, 0] == ids[r + 1, 0]
                cut += 1
    assert cut >= 3


def long_rows(env, L=333):
    """rows of L cells (a trip is 64) that hold a 150-piece word and words of ten pieces each; the 150-piece word as (row, first, last)"""
    c, d = (int(v) for v in env["cont"][:2])
    x, y = (int(v) for v in env["plain"][:2])
    pad, bos, eos = env["pad"], env["bos"], env["eos"]
    rows = []

    def row(cells):
        assert len(cells) <= L
        rows.append(cells + [pad] * (L - len(cells)))
    row([bos] + [y] * 9 + [c] * 149 + [x] + [y, d, x] * 8 + [eos])                        # a word over cells 10 .. 159: two whole trips inside it
    row([bos] + ([c, d] * 4 + [c, x]) * 30 + [eos])                                      # 30 words of ten pieces: 16 of them are 160 cells
    row(([d] * 9 + [y]) * 33 + [x] * 3)                                                  # the same without a protected cell in the row
    row([x] * (L - 10) + [c] * 10)                                                       # the last cell is a continuation ...
    row([d, x] + [y] * (L - 2))                                                          # ... and cell 0 of the next row is a start all the same
    return np.array(rows * 3, dtype=np.int32), (0, 10, 159)


def startless_trips(env, ids, chosen):
    """trips of the kernel's walk over `ids` that hold chosen cells and no start at all: their cells know their ordinal, their span's
    reach and their place in E and T from the carries alone.  The geometry is csrc/gz_infill.inc's: a wave owns max(1, 4096 // L)
    rows as one flat range and a trip is 64 cells."""
    R, L = ids.shape
    prot, head = MO.heads(ids, env["cont"], (env["pad"], env["bos"], env["eos"], env["mask"]), True)
    start = head == np.arange(L)[None, :]
    rpw, n = max(1, 4096 // L), 0
    for r0 in range(0, R, rpw):
        s, ch = start[r0:r0 + rpw].reshape(-1), chosen[r0:r0 + rpw].reshape(-1)
        n += sum(1 for b in range(0, len(s), 64) if not s[b:b + 64].any() and ch[b:b + 64].any())
    return n


def test_a_word_longer_than_a_trip_inside_a_span(tok, env):
    ids, (r, a, b) = long_rows(env)
    prot_ids = (env["pad"], env["bos"], env["eos"], env["mask"])
    seen, startless = set(), 0
    for seed in range(8):
        kw = dict(p=0.3, seed=seed, lengths="fixed", mean_span=3, max_span=3, dec_len=200)
        want = check(tok, env, ids, **kw)
        t_start, len_t, n_len = IO.rule_ints(0.3, 3, 3, "fixed")
        _, _, _, chosen = IO.chosen_cells(ids, env["cont"], prot_ids, seed, t_start, len_t, n_len, True, 0)
        startless += startless_trips(env, ids, chosen)
        for rr in (r, r + 5, r + 10):                                # all of the long word or nothing of it
            assert chosen[rr, a:b + 1].all() or not chosen[rr, a:b + 1].any()
            seen.add(bool(chosen[rr, a]))
        check(tok, env, ids, **dict(kw, whole_word=False))
    assert seen == {False, True} and startless >= 6


def test_a_sixteen_word_span_longer_than_two_trips(tok, env):
    """spans of 16 words of ten pieces: 160 cells.  From the oracle's starts first: some span is alone (no other span begins inside
    it), so `far` alone carries it over two trip edges, and a trip in it holds no span start of its own"""
    ids, _ = long_rows(env)
    prot_ids = (env["pad"], env["bos"], env["eos"], env["mask"])
    t_start, lone = ONE // 25, 0
    for seed in range(6):
        check_raw(tok, env, ids, seed, t_start, [0] * 15, 16, dec_width=170)
        _, start, n, chosen = IO.chosen_cells(ids, env["cont"], prot_ids, seed, t_start, [0] * 15, 16, True, 0)
        x0 = MO.draw(np.arange(ids.size, dtype=np.uint64).reshape(ids.shape), seed)[0]
        begins = start & (x0 < np.uint64(t_start))
        for r in (1, 2, 6, 7, 11, 12):
            for c in np.flatnonzero(begins[r]):
                inside = (n[r] >= n[r, c]) & (n[r] < n[r, c] + 16) & ~np.isin(ids[r], prot_ids)
                if inside.sum() == 160 and begins[r][inside].sum() == 1:
                    assert chosen[r][inside].all()
                    cells = np.flatnonzero(inside) + (r % 12) * ids.shape[1]         # (12 rows a wave: the flat index decides the trips)
                    lone += int(cells[-1] // 64 - cells[0] // 64 >= 2)
    assert lone >= 2


def test_every_word_chosen(tok, env):
    """t_start = 2^32: with whole words a framed row becomes bos <mask> eos; per token with protected cells interleaved every other
    cell is a run of its own -- the maximal number of runs"""
    rng = np.random.default_rng(40)
    for L in (9, 64, 130):
        ids = framed_rows(env, rng, 66, L)
        n = rng.integers(1, L - 1, 66)                               # a body of 1 .. L - 2 cells behind bos, then eos, then pad
        cols = np.arange(L)[None, :]
        body = np.where(rng.random((66, L)) < 0.5, rng.choice(env["cont"], (66, L)), rng.integers(5, env["n_ids"], (66, L)))
        ids = np.where(cols == 0, env["bos"], np.where(cols <= n[:, None], body, np.where(cols == (n + 1)[:, None], env["eos"], env["pad"]))).astype(np.int32)
        want = check(tok, env, ids, p=1.0, dec_len=L + 2)
        assert (want["enc_len"] == 3).all() and (want["n_spans"] == 1).all() and np.array_equal(want["dec_len"], n + 2)
        assert (want["input_ids"][:, :3] == [env["bos"], env["mask"], env["eos"]]).all() and (want["input_ids"][:, 3:] == env["pad"]).all()
        alt = np.empty((66, L), dtype=np.int32)
        alt[:, 0::2] = rng.choice(env["cont"], (66, (L + 1) // 2))
        alt[:, 1::2] = rng.choice([env["eos"], env["bos"], env["mask"]], (66, L // 2))
        for ww in (True, False):
            want = check(tok, env, alt, p=1.0, whole_word=ww, dec_len=L + 2)
            assert (want["n_spans"] == (L + 1) // 2).all() and (want["dec_len"] == 2 * ((L + 1) // 2) + 1).all() and (want["enc_len"] == L).all()
    nine = np.arange(100, 109, dtype=np.int32)[None, :].repeat(3, axis=0)               # the header's example: len(T) = 11
    for W in (9, 10, 11):
        want = check(tok, env, nine, p=1.0, whole_word=False, dec_len=W)
        assert want["dec_len"].tolist() == [11] * 3 and want["labels"][1].tolist() == ([env["mask"]] + list(range(100, 109)) + [env["eos"]])[:W]


def test_rows_longer_than_the_decoder_width(tok, env):
    """dec_len > dec_width: the clipped arrays are the oracle's (so the cells of the next row are intact), dec_len is unclipped"""
    rng = np.random.default_rng(41)
    for L, W in ((64, 5), (70, 1), (130, 64), (37, 20)):
        ids = framed_rows(env, rng, 90, L)
        for ww in (True, False):
            want = check(tok, env, ids, p=0.6, seed=L, whole_word=ww, dec_len=W)
            over = want["dec_len"] > W
            assert over.any() and (want["labels"][over] != -100).all()
    # the raw device call into arrays with a guard row on either side
    ids = framed_rows(env, rng, 20, 64)
    want = want_of(env, ids, p=0.6, seed=3, dec_len=7)
    ctx = tok._ctx
    t_start, len_t, n_len = IO.rule_ints(0.6, 3.0, 10, "geometric")
    bufs = [ctx.alloc(n) for n in (ids.nbytes, ids.nbytes, 4 * 22 * 7, 4 * 22 * 7, 4 * 20)]
    d_ids, d_out, d_lab, d_dec, d_len = bufs
    try:
        guard = np.full((22, 7), -9, np.int32)
        ctx.h2d(d_ids, ids); ctx.h2d(d_lab, guard); ctx.h2d(d_dec, guard)
        ctx.infill_rows_device(d_ids, 20, 64, 0, (3, t_start, len_t, n_len, env["mask"], 1, -100, 7), d_out, 0, d_lab + 28, d_dec + 28, 0, d_len, 0)
        lab, dec, dl = np.empty((22, 7), np.int32), np.empty((22, 7), np.int32), np.empty(20, np.int32)
        ctx.d2h(lab, d_lab); ctx.d2h(dec, d_dec); ctx.d2h(dl, d_len)
    finally:
        for d in bufs:
            ctx.free(d)
    assert (lab[[0, 21]] == -9).all() and (dec[[0, 21]] == -9).all()
    assert np.array_equal(lab[1:21], want["labels"]) and np.array_equal(dec[1:21], want["decoder_input_ids"]) and np.array_equal(dl, want["dec_len"])
    assert (dl > 7).any()


def test_ids_outside_the_snapshot_are_plain_tokens(tok, env):
    n, c = env["n_ids"], int(env["cont"][0])
    odd = [-1, -5, n, n + 1, 2 ** 31 - 1, -2 ** 31, n + 7, -1]
    ids = np.array([odd, [c, -1, c, n, c, 2 ** 31 - 1, c, -2 ** 31], [env["bos"], -1, n, env["eos"], env["pad"], env["pad"], -3, n]], dtype=np.int32)
    for ww in (True, False):
        for seed in range(4):
            check(tok, env, ids, p=0.5, seed=seed, whole_word=ww, dec_len=10)
    got = tok.infill_rows(ids, p=1.0, dec_len=10)
    assert got["labels"][0].tolist() == [env["mask"]] + odd + [env["eos"]] and got["labels"][2].tolist()[:7] == [env["mask"], -1, n, env["mask"], -3, n, env["eos"]]
    # none of them continues a word: each starts one, so row 0 holds eight words
    t_start, len_t, n_len = IO.rule_ints(0.3, 1.0, 1, "fixed")
    x0 = MO.draw(np.arange(8, dtype=np.uint64), 3)[0]
    got = tok.infill_rows(ids[:1], p=0.3, seed=3, lengths="fixed", mean_span=1, max_span=1)
    assert got["enc_len"][0] + (x0 < t_start).sum() - got["n_spans"][0] == 8 and got["dec_len"][0] == (x0 < t_start).sum() + got["n_spans"][0] + 1


def test_a_real_token_equal_to_the_pad_id_drops_out(tok, env):
    x, c = int(env["plain"][0]), int(env["cont"][0])
    ids = np.array([[env["bos"], x, env["pad"], x, c, env["pad"], x, env["eos"], env["pad"]]], dtype=np.int32)
    for seed in range(4):
        check(tok, env, ids, p=0.5, seed=seed)
    got = tok.infill_rows(ids, p=0.0)
    assert got["input_ids"][0].tolist() == [env["bos"], x, x, c, x, env["eos"], 0, 0, 0] and got["enc_len"].tolist() == [6]
    got = tok.infill_rows(ids, p=1.0)
    assert got["input_ids"][0].tolist()[:6] == [env["bos"], env["mask"], env["mask"], env["mask"], env["eos"], env["pad"]] and got["n_spans"].tolist() == [3]


def test_rows_and_trips_of_padding(tok, env):
    """a trip that holds padding alone takes a shortcut in the kernel: all-pad rows, rows whose body ends before a trip edge, a pad
    stretch of a whole trip in mid-row with words behind it (the carries must come through), rows that begin inside a padding trip"""
    rng = np.random.default_rng(50)
    pad, x, c = env["pad"], int(env["plain"][0]), int(env["cont"][0])
    for L in (5, 31, 64, 130, 200):
        ids = framed_rows(env, rng, 70, L)
        ids[rng.random(70) < 0.3] = pad                              # all-pad rows among the others
        ids[3], ids[4] = pad, pad
        if L >= 130:
            ids[7, 20:L - 20] = pad                                  # mid-row padding, words on either side: at L = 200 a stretch of 160 cells,
            ids[7, L - 20:] = x                                      # which holds a whole trip of 64 wherever the row lies in its wave's range
            ids[8, :L - 3] = pad                                     # the row's only words behind trips of padding
            ids[8, L - 3:] = [c, c, x]
        for ww in (True, False):
            want = check(tok, env, ids, p=0.5, seed=L, whole_word=ww, dec_len=max(1, L // 2))
            assert (want["enc_len"][[3, 4]] == 0).all() and (want["dec_len"][[3, 4]] == 1).all() and (want["labels"][[3, 4], 0] == env["eos"]).all()
            assert (want["decoder_input_ids"][[3, 4], 0] == env["bos"]).all()
    check(tok, env, np.full((300, 64), pad, dtype=np.int32), p=0.5)
    check(tok, env, np.full((3, 1000), pad, dtype=np.int32), p=0.5, dec_len=7)


def test_laws_and_end_shares(tok, env):
    rng = np.random.default_rng(5)
    ids = framed_rows(env, rng, 40, 70)
    want = check(tok, env, ids, p=0.0)
    assert (want["dec_len"] == 1).all() and not want["n_spans"].any() and np.array_equal(want["enc_len"], (ids != env["pad"]).sum(axis=1))
    assert np.array_equal(want["input_ids"], ids)                    # (framed rows: the pads are behind)
    for kw in (dict(lengths="poisson"), dict(lengths="poisson", mean_span=7.5, max_span=16), dict(lengths="fixed", mean_span=16, max_span=16),
               dict(lengths="fixed", mean_span=1, max_span=1), dict(mean_span=1.0, max_span=16), dict(mean_span=16.0, max_span=16),
               dict(ignore_index=-7, dec_len=33), dict(ignore_index=2 ** 31 - 1)):
        for ww in (True, False):
            check(tok, env, ids, p=0.3, seed=4, whole_word=ww, **kw)
    check_raw(tok, env, ids, 1, ONE // 3, [ONE, ONE, ONE], 4)         # thresholds of 2^32: never -- every span one word
    check_raw(tok, env, ids, 1, ONE // 3, [0, ONE // 2, ONE], 4)
    check_raw(tok, env, ids, 1, ONE - 1, [ONE - 1] * 15, 16)


def test_counter_width(tok, env):
    rng = np.random.default_rng(6)
    ids = framed_rows(env, rng, 3, 5)
    base = 2 ** 32 // 5 - 1                                          # g runs from 2^32 - 6 to 2^32 + 8 inside the call
    assert base * 5 < 2 ** 32 < (base + 3) * 5
    for ww in (True, False):
        check(tok, env, ids, p=0.5, row_base=base, whole_word=ww)
    for L, R in ((5, 3), (64, 70), (200, 9)):
        ids = framed_rows(env, rng, R, L)
        check(tok, env, ids, p=0.5, row_base=2 ** 62 // L - 2, seed=1)
        check(tok, env, ids, p=0.5, row_base=2 ** 63 // L - R - 1, seed=1)              # the last index the rule allows
    ids = framed_rows(env, rng, 20, 64)
    hi = 0xDEADBEEF12345678
    a = check(tok, env, ids, p=0.5, seed=hi)
    b = check(tok, env, ids, p=0.5, seed=hi & 0xFFFFFFFF)
    c = check(tok, env, ids, p=0.5, seed=2 ** 64 - 1)
    assert not np.array_equal(a["labels"], b["labels"]) and not np.array_equal(a["labels"], c["labels"])
    one, two = tok.infill_rows(ids, p=0.5, seed=hi), tok.infill_rows(ids, p=0.5, seed=hi)
    for k in KEYS:
        assert np.array_equal(one[k], two[k])


def test_slices_with_row_base_are_the_slices_of_the_batch(tok, env):
    rng = np.random.default_rng(8)
    for L in (64, 37):
        ids = framed_rows(env, rng, 130, L)
        whole = check(tok, env, ids, p=0.3, seed=11, row_base=5, dec_len=20)
        cuts = [0, 1, 64, 65, 130]
        parts = [tok.infill_rows(ids[a:b], p=0.3, seed=11, row_base=5 + a, dec_len=20) for a, b in zip(cuts[:-1], cuts[1:])]
        for k in KEYS:
            assert np.array_equal(np.concatenate([q[k] for q in parts]), whole[k]), k


def raw_args(env, len_t, R=2, L=8, row_base=0, seed=1, t_start=2 ** 31, n_len=3, whole_word=1, ignore=-100, W=6):
    return [R, L, row_base, seed, t_start, len_t, n_len, env["mask"], whole_word, ignore, W]


def test_each_optional_output_may_be_null(tok, env):
    tok._sync_tables()
    ctx, lib = tok._ctx, tok._ctx.lib
    rng = np.random.default_rng(9)
    ids = framed_rows(env, rng, 70, 33)
    lt = np.array([ONE // 3, ONE // 3 * 2, 0], dtype=np.uint64)
    want = IO.infill(ids, env["cont"], env["pad"], env["bos"], env["eos"], env["mask"], seed=1, t_start=2 ** 31, len_t=[int(v) for v in lt[:2]],
                     n_len=3, dec_width=12)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)                     # noqa: E731
    vp = ctypes.c_void_p
    sizes = dict(input_ids=(70, 33), attention_mask=(70, 33), labels=(70, 12), decoder_input_ids=(70, 12), enc_len=(70,), dec_len=(70,), n_spans=(70,))
    d_ids = ctx.alloc(ids.nbytes)
    dev = {k: ctx.alloc(4 * int(np.prod(s))) for k, s in sizes.items()}
    try:
        ctx.h2d(d_ids, ids)
        for skip in (None, "attention_mask", "decoder_input_ids", "enc_len", "dec_len", "n_spans", "all"):
            off = ("attention_mask", "decoder_input_ids", "enc_len", "dec_len", "n_spans") if skip == "all" else (skip,)
            host = {k: np.full(s, -9, np.int32) for k, s in sizes.items()}
            rc = lib.gz_infill_rows(ctx.handle, P(ids), *raw_args(env, P(lt), R=70, L=33, W=12), *[None if k in off else P(host[k]) for k in KEYS])
            assert rc == 0, skip
            rc = lib.gz_infill_rows_device(ctx.handle, vp(d_ids), *raw_args(env, P(lt), R=70, L=33, W=12),
                                           *[None if k in off else vp(dev[k]) for k in KEYS])
            assert rc == 0, skip
            for k in KEYS:
                if k in off:
                    assert (host[k] == -9).all()
                    continue
                assert np.array_equal(host[k], want[k]), (skip, k)
                back = np.empty(sizes[k], np.int32)
                ctx.d2h(back, dev[k])
                assert np.array_equal(back, want[k]), (skip, k)
    finally:
        ctx.free(d_ids)
        for d in dev.values():
            ctx.free(d)


TEXTS = ["công nghệ thông tin và truyền thông", "xin chào thế giới", "", "trăm中 phần trăm 中", "một hai ba bốn năm sáu bảy tám chín mười " * 6,
         "internationalization antidisestablishmentarianism", "a"] * 9


def test_device_rows_of_window_and_pack_calls(tok, env):
    for make, L in ((lambda: tok.encode_windows_to_device(TEXTS, 16, 4), 16), (lambda: tok.encode_packs_to_device(TEXTS, 24), 24),
                    (lambda: tok.encode_to_device(TEXTS, max_len=13), 13)):
        rows = make()["input_ids"]                                   # (no sync between the encode call and the infill call)
        got_dev = tok.infill_rows_to_device(rows, p=0.4, seed=3, row_base=17, dec_len=9)
        host = rows.numpy()
        assert host.shape[1] == L and host.shape[0] > 8
        for ww, dl in ((True, 9), (False, None)):
            got = got_dev if ww else tok.infill_rows_to_device(rows, p=0.4, seed=3, whole_word=False, row_base=17)
            W = L if dl is None else dl
            assert got["input_ids"].shape == host.shape and got["attention_mask"].shape == host.shape
            assert got["labels"].shape == (len(host), W) and got["decoder_input_ids"].shape == (len(host), W)
            got = {k: (got[k] if k in ("enc_len", "dec_len", "n_spans") else got[k].numpy()) for k in KEYS}
            same(got, tok.infill_rows(host, p=0.4, seed=3, whole_word=ww, row_base=17, dec_len=dl))
            same(got, want_of(env, host, p=0.4, seed=3, whole_word=ww, row_base=17, dec_len=dl))
        assert np.array_equal(rows.numpy(), host)                    # the source rows are not changed
    empty = tok.infill_rows(np.zeros((0, 7), dtype=np.int32), dec_len=3)
    assert empty["input_ids"].shape == (0, 7) and empty["labels"].shape == (0, 3) and empty["dec_len"].shape == (0,)


def test_raw_device_call_directly_behind_the_window_call(tok, env):
    """gz_infill_rows_device enqueued behind gz_window_rows_device on the context's stream, no gz_sync in between"""
    ctx = tok._ctx
    rng = np.random.default_rng(12)
    bodies = [framed_rows(env, rng, 1, n)[0] for n in (3, 40, 7, 90, 5)]
    flat = np.concatenate(bodies).astype(np.int32)
    off = np.zeros(len(bodies) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in bodies])
    L, s, Wd = 16, 3, 8
    want_rows = tok.window_rows(bodies, L, s)["input_ids"]
    W = len(want_rows)
    t_start, len_t, n_len = IO.rule_ints(0.5, 3.0, 10, "geometric")
    rule = (5, t_start, len_t, n_len, env["mask"], 1, -100, Wd)
    sizes = dict(input_ids=(W, L), attention_mask=(W, L), labels=(W, Wd), decoder_input_ids=(W, Wd), enc_len=(W,), dec_len=(W,), n_spans=(W,))
    bufs = [ctx.alloc(n) for n in (flat.nbytes + 64, off.nbytes, off.nbytes, 4 * W * L)] + [ctx.alloc(4 * int(np.prod(v))) for v in sizes.values()]
    d_ids, d_off, d_wo, d_rows = bufs[:4]
    try:
        ctx.h2d(d_ids, flat)
        ctx.h2d(d_off, off)
        assert ctx.window_rows_device(d_ids, d_off, len(bodies), L, s, 1, 1, d_rows, 0, 0, 0, 0, d_wo, W) == W
        ctx.infill_rows_device(d_rows, W, L, 0, rule, *bufs[4:])
        got = {k: np.empty(v, np.int32) for k, v in sizes.items()}
        for k, d in zip(KEYS, bufs[4:]):
            ctx.d2h(got[k], d)
    finally:
        for d in bufs:
            ctx.free(d)
    same(got, want_of(env, want_rows, p=0.5, seed=5, dec_len=Wd))


def test_refusals_leave_the_outputs_untouched(tok, env):
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    lib = ctx.lib
    ids = np.full((2, 8), int(env["plain"][0]), dtype=np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)                     # noqa: E731
    lt = np.array([5, 9, 0], dtype=np.uint64)
    outs = [np.full(n, -9, np.int32) for n in (16, 16, 12, 12, 2, 2, 2)]
    bad = [dict(L=0), dict(L=-1), dict(R=-1), dict(row_base=-1), dict(row_base=2 ** 63 // 8 - 2), dict(row_base=2 ** 63 - 1),
           dict(t_start=2 ** 32 + 1), dict(W=0), dict(W=-1), dict(n_len=0), dict(n_len=17), dict(n_len=-1), dict(whole_word=2), dict(whole_word=-1)]
    for kw in bad:
        assert lib.gz_infill_rows(ctx.handle, P(ids), *raw_args(env, P(lt), **kw), *[P(o) for o in outs]) == _native.GZ_E_INVALID, kw
    assert lib.gz_infill_rows(ctx.handle, P(ids), *raw_args(env, None), *[P(o) for o in outs]) == _native.GZ_E_INVALID      # len_t NULL, n_len 3
    for words in ([9, 5, 0], [2 ** 32 + 1, 2 ** 32 + 1, 0], [5, 2 ** 32 + 1, 0]):                                              # decreasing; above 2^32
        assert lib.gz_infill_rows(ctx.handle, P(ids), *raw_args(env, P(np.array(words, dtype=np.uint64))), *[P(o) for o in outs]) == _native.GZ_E_INVALID
    for k in (None, 0, 2):                                           # ids, input_ids, labels NULL
        ptrs = [P(o) for o in outs]
        if k is not None:
            ptrs[k] = None
        assert lib.gz_infill_rows(ctx.handle, None if k is None else P(ids), *raw_args(env, P(lt)), *ptrs) == _native.GZ_E_INVALID
    big = np.full(80, -9, np.int32)                                  # overlapping buffers, by one cell
    at = lambda k: ctypes.c_void_p(big.ctypes.data + 4 * k)          # noqa: E731
    for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (0, 6), (1, 3)):
        ptrs = [P(o) for o in outs]
        ptrs[a], ptrs[b] = at(0), at((16, 16, 12, 12, 2, 2, 2)[a] - 1)
        assert lib.gz_infill_rows(ctx.handle, P(ids), *raw_args(env, P(lt)), *ptrs) == _native.GZ_E_INVALID, (a, b)
    ptrs = [P(o) for o in outs]
    ptrs[4] = ctypes.c_void_p(ids.ctypes.data + 4 * 15)              # enc_len on the last cell of ids
    assert lib.gz_infill_rows(ctx.handle, P(ids), *raw_args(env, P(lt)), *ptrs) == _native.GZ_E_INVALID
    assert (big == -9).all() and all((o == -9).all() for o in outs)
    # the device form refuses the same things, before anything is launched
    bufs = [ctx.alloc(4 * 80) for _ in range(8)]
    d_ids, d_outs = bufs[0], bufs[1:]
    vp = ctypes.c_void_p
    try:
        for d in d_outs:
            ctx.h2d(d, big)
        ctx.h2d(d_ids, ids)
        for kw in bad:
            assert lib.gz_infill_rows_device(ctx.handle, vp(d_ids), *raw_args(env, P(lt), **kw), *[vp(d) for d in d_outs]) == _native.GZ_E_INVALID, kw
        assert lib.gz_infill_rows_device(ctx.handle, vp(d_ids), *raw_args(env, None), *[vp(d) for d in d_outs]) == _native.GZ_E_INVALID
        for k in (None, 0, 2):
            ptrs = [vp(d) for d in d_outs]
            if k is not None:
                ptrs[k] = None
            assert lib.gz_infill_rows_device(ctx.handle, None if k is None else vp(d_ids), *raw_args(env, P(lt)), *ptrs) == _native.GZ_E_INVALID
        for a, b in ((0, 1), (2, 3), (3, 6), (4, 5)):                # 16 cells are 64 bytes, 12 are 48, 2 are 8: one cell of overlap
            ptrs = [vp(d) for d in d_outs]
            ptrs[b] = vp(d_outs[a] + 4 * ((16, 16, 12, 12, 2, 2, 2)[a] - 1))
            assert lib.gz_infill_rows_device(ctx.handle, vp(d_ids), *raw_args(env, P(lt)), *ptrs) == _native.GZ_E_INVALID, (a, b)
        ptrs = [vp(d) for d in d_outs]
        ptrs[0] = vp(d_ids + 60)
        assert lib.gz_infill_rows_device(ctx.handle, vp(d_ids), *raw_args(env, P(lt)), *ptrs) == _native.GZ_E_INVALID
        back = np.empty(80, np.int32)
        for d in d_outs:
            ctx.d2h(back, d)
            assert (back == -9).all()
        # R == 0 is fine and writes nothing; NULL pointers are allowed then, and len_t with n_len == 1
        assert lib.gz_infill_rows_device(ctx.handle, None, *raw_args(env, None, R=0, n_len=1), *[None] * 7) == _native.GZ_OK
        assert lib.gz_infill_rows(ctx.handle, None, *raw_args(env, P(lt), R=0), *[None] * 7) == _native.GZ_OK
        assert lib.gz_infill_rows(ctx.handle, P(ids), *raw_args(env, None, n_len=1, t_start=2 ** 32), *[P(o) for o in outs]) == _native.GZ_OK
        assert outs[0].tolist() == [env["mask"]] + [env["pad"]] * 7 + [env["mask"]] + [env["pad"]] * 7 and outs[5].tolist() == [10, 10]
    finally:
        for d in bufs:
            ctx.free(d)
    # a context without a decoder snapshot gives the decode call's error
    fresh = _native.Context()
    canary = [np.full(n, -9, np.int32) for n in (16, 16, 12, 12, 2, 2, 2)]
    try:
        rc = fresh.lib.gz_infill_rows(fresh.handle, P(ids), *raw_args(env, P(lt)), *[P(o) for o in canary])
        assert rc == _native.GZ_E_NOTABLES and all((o == -9).all() for o in canary)
    finally:
        fresh.close()


def test_python_refusals_come_before_any_launch(tok):
    ids = np.zeros((2, 4), dtype=np.int32)
    for kw, exc in ((dict(p=1.5), ValueError), (dict(p=True), TypeError), (dict(seed=-1), ValueError), (dict(seed=1.0), TypeError),
                    (dict(max_span=17), ValueError), (dict(mean_span=0.5), ValueError), (dict(lengths="zipf"), ValueError),
                    (dict(dec_len=0), ValueError), (dict(row_base=True), TypeError)):
        with pytest.raises(exc):
            tok.infill_rows(ids, **kw)
    with pytest.raises(TypeError):
        tok.infill_rows_to_device(ids)
    with pytest.raises(TypeError):
        tok.infill_rows(ids.astype(np.float32))
    with pytest.raises(ValueError):
        tok.infill_rows(ids[0])
    with pytest.raises(ValueError):
        tok.infill_rows(ids, row_base=2 ** 63 // 4)
