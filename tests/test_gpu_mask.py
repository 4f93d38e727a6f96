"""Masked-LM inputs and labels on the GPU (gz_mask_rows / gz_mask_rows_device; Tokenize.mask_rows, mask_rows_to_device) against the
rule of tests/mask_oracle.py, which tests/test_mask_inputs.py ties to the Philox known answers and to a second restatement.
Every comparison with the oracle is exact, on input_ids, labels and n_chosen.

Written for csrc/gz_mask.inc: every workgroup stages the continuation bitmap in LDS (switch mask_lds = 0: read from memory); a wave walks its rows' cells in trips of 64 units -- 4 cells a unit where L % 4 == 0, one otherwise --
and takes about 4096 cells, so several rows share a trip when L is small, a row spans trips when L > 64 (or 256), and 257 rows of
any L here are more than one wave and, from L = 64 on, more than one workgroup."""
import ctypes

import numpy as np
import pytest

import mask_oracle as MO
from conftest import DATA

pytestmark = pytest.mark.gpu

KEYS = ("input_ids", "labels", "n_chosen")
LS = (1, 2, 3, 5, 63, 64, 65, 127, 128, 130, 200)
RS = (0, 1, 2, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


@pytest.fixture(scope="module")
def env(tok):
    """the special ids, the snapshot's size, the continuation ids (from the vocab file, not from the product), two plain ids"""
    pad, bos, eos, mask = tok._special_ids()[:4]
    cont = MO.continuation_ids(DATA + "/vocab.txt")
    n_ids = tok.vocab_size()
    plain = np.setdiff1d(np.arange(5, n_ids), cont)
    return dict(pad=pad, bos=bos, eos=eos, mask=mask, cont=cont, n_ids=n_ids, plain=plain)


def want_of(env, ids, p=0.15, seed=0, whole_word=True, mask_prob=0.8, random_prob=0.1, random_ids=None, row_base=0, ignore_index=-100):
    t_sel, t1, t2 = MO.thresholds(p, mask_prob, random_prob)
    lo, hi = random_ids if random_ids is not None else (5, env["n_ids"])
    return MO.mask(ids, env["cont"], env["pad"], env["bos"], env["eos"], env["mask"], seed=seed, t_sel=t_sel, t1=t1, t2=t2, rand_lo=lo,
                   rand_hi=hi, whole_word=whole_word, row_base=row_base, ignore_index=ignore_index)


def same(got, want):
    for k in KEYS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())


def check(tok, env, ids, **kw):
    want = want_of(env, ids, **kw)
    got = tok.mask_rows(ids, **kw)
    same(got, want)
    return want


def framed_rows(env, rng, R, L):
    """random vocabulary ids, half of them continuation pieces, each row [bos] body [eos] pad*"""
    ids = np.where(rng.random((R, L)) < 0.5, rng.choice(env["cont"], (R, L)), rng.integers(5, env["n_ids"], (R, L)))
    if L >= 3:
        n = rng.integers(0, L - 1, R)                                # body length 0 .. L - 2
        cols = np.arange(L)[None, :]
        ids = np.where(cols == 0, env["bos"], np.where(cols == (n + 1)[:, None], env["eos"], np.where(cols > (n + 1)[:, None], env["pad"], ids)))
    return ids.astype(np.int32)


@pytest.mark.parametrize("L", LS)
def test_row_lengths_and_row_counts_at_trip_and_wave_edges(tok, env, L):
    rng = np.random.default_rng(100 + L)
    for R in RS:
        ids = framed_rows(env, rng, R, L)
        for ww in (True, False):
            want = check(tok, env, ids, p=0.4, seed=7 * L + R, whole_word=ww)
            if R >= 63 and L >= 5:
                assert 0 < want["n_chosen"].sum() < (ids != env["pad"]).sum()


def test_continuation_bits_read_from_memory_give_the_same(tok, env):
    """switch mask_lds = 0: the bitmap is not staged in LDS (the path of a vocabulary too large for it)"""
    from genz_tokenize import _native
    rng = np.random.default_rng(21)
    _native.debug_set("mask_lds", 0, tok._ctx)
    try:
        for R, L in ((70, 128), (70, 65), (3, 200)):
            check(tok, env, framed_rows(env, rng, R, L), p=0.4, seed=R + L)
        ids, _ = word_rows(env)
        check(tok, env, ids, p=0.5, seed=2)
    finally:
        _native.debug_set("mask_lds", 1, tok._ctx)


def word_rows(env, L=200):
    """rows of L >= 200 built from known continuation ids (c, d) and plain ids (x, y); the words they hold, as (row, first, last).
    L = 200 takes the kernel of four cells a lane (a trip is 256 cells), an odd L the kernel of one cell a lane (a trip is 64 cells:
    the 150-cell word then covers whole trips that hold no start at all, and the carried bit has to survive them)."""
    c, d = (int(v) for v in env["cont"][:2])
    x, y = (int(v) for v in env["plain"][:2])
    pad, bos, eos, mask = env["pad"], env["bos"], env["eos"], env["mask"]
    rows, words = [], []

    def row(cells):
        assert len(cells) <= L
        rows.append(cells + [pad] * (L - len(cells)))
        return len(rows) - 1
    r = row([bos] + [x] * 59 + [c, d, c, d, c, d, c, x] + [y] * 20 + [eos])              # a word over cells 60 .. 67: crosses 63 -> 64
    words.append((r, 60, 67))
    r = row([bos] + [y] * 9 + [c] * 149 + [x] + [y] * 5 + [eos])                         # 150 cells, 10 .. 159: the carry runs over two trips
    words.append((r, 10, 159))
    r = row([x] * (L - 10) + [c] * 10)                                                   # no protected cell; the last cell is a continuation ...
    words.append((r, L - 10, L - 1))
    r = row([d, x] + [y] * (L - 2))                                                        # ... and cell 0 of the next row is a start all the same
    words.append((r, 0, 1))
    r = row([bos, x, c, eos, bos, c, d, mask, d, y, eos, c, c])                          # a continuation before eos, before <mask>, before pad
    words += [(r, 2, 2), (r, 5, 6), (r, 8, 9), (r, 11, 12)]
    r = row([c] * L)                                                                     # one word, the whole row, no protected cell at all
    words.append((r, 0, L - 1))
    row([pad, bos, eos, mask] * 50)                                                      # protected cells only
    row([])
    return np.array(rows, dtype=np.int32), words


@pytest.mark.parametrize("L", [200, 201, 203])
def test_word_edges_from_known_continuation_ids(tok, env, L):
    ids, words = word_rows(env, L)
    assert ids.shape == (8, L) and startless_trips(env, ids) >= (4 if L % 4 else 1)      # (at 200 a trip is 256 cells: the 150-cell word crosses one edge)
    seen = {w: set() for w in words}
    for seed in range(8):
        got = check(tok, env, ids, p=0.5, seed=seed)
        for (r, a, b) in words:                                      # all of a word or nothing of it
            picked = got["labels"][r, a:b + 1] != -100
            assert picked.all() or not picked.any(), (seed, r, a, b)
            seen[(r, a, b)].add(bool(picked[0]))
        assert (got["labels"][-2:] == -100).all() and (got["n_chosen"][-2:] == 0).all()
        assert np.array_equal(got["input_ids"][-2:], ids[-2:])
        check(tok, env, ids, p=0.5, seed=seed, whole_word=False)
        assert got["n_chosen"][5] in (0, L)
    assert all(v == {False, True} for v in seen.values()), seen      # eight seeds show both outcomes for every word
    split = tok.mask_rows(ids, p=0.5, seed=0, whole_word=False)["labels"][1, 10:160] != -100
    assert split.any() and not split.all()


def long_word_rows(env):
    """rows of 400 (four cells a lane: a trip is 256 cells) and of 401 (one cell a lane) with words of 300 and 330 cells, placed so
    that trips without any start lie inside them, and after them a short word whose decision must not be the carried one"""
    c, d = (int(v) for v in env["cont"][:2])
    x, y = (int(v) for v in env["plain"][:2])
    pad, bos, eos = env["pad"], env["bos"], env["eos"]
    out = {}
    for L in (400, 401):
        rows, words = [], []
        for cells, span in (([bos] + [y] * 9 + [c] * 299 + [x] + [d, x] + [y] * 20 + [eos], (10, 309)),     # 300 cells; then the word (310, 311)
                            ([y] * 60 + [c, d] * 164 + [c, x] + [y] * (L - 390), (60, 389)),                 # 330 cells, no protected cell in the row
                            ([d] * (L - 1) + [x], (0, L - 1)),                                               # the whole row, over every trip of it
                            ([y] * 3 + [c] * 300 + [eos] + [c] * 90 + [x], (3, 302))):                       # ended by eos, not by a plain id
            rows.append(cells + [pad] * (L - len(cells)))
            words.append((len(rows) - 1, *span))
        words += [(0, 310, 311), (3, 304, 394)]
        out[L] = (np.array(rows * 3, dtype=np.int32), words + [(r + 4, a, b) for r, a, b in words] + [(r + 8, a, b) for r, a, b in words])
    return out


def startless_trips(env, ids):
    """trips of the kernel's walk over `ids` that hold unprotected cells and no start: each must take the carried decision and hand
    it on.  The geometry is csrc/gz_mask.inc's: a wave owns max(1, 4096 // L) rows as one flat range and a trip is 64 units of 4
    cells where L % 4 == 0 (the host path's buffers are aligned), of one cell otherwise."""
    R, L = ids.shape
    prot, head = MO.heads(ids, env["cont"], (env["pad"], env["bos"], env["eos"], env["mask"]), True)
    start = head == np.arange(L)[None, :]
    rpw, trip, n = max(1, 4096 // L), 64 * (4 if L % 4 == 0 else 1), 0
    for r0 in range(0, R, rpw):
        s, p = start[r0:r0 + rpw].reshape(-1), prot[r0:r0 + rpw].reshape(-1)
        n += sum(1 for b in range(0, len(s), trip) if not s[b:b + trip].any() and not p[b:b + trip].all())
    return n


@pytest.mark.parametrize("L", [400, 401])
def test_words_longer_than_a_trip_keep_the_carried_decision(tok, env, L):
    """A trip that holds no start must hand the carried bit on unchanged: a 300-cell word in a row of 400 covers a whole 256-cell trip
    of the four-cells-a-lane kernel only when it is placed across one, so the rows are laid three times over (12 rows: the flat
    range of a wave shifts them against the trips), and at L = 401 the one-cell-a-lane kernel meets four startless trips a word."""
    ids, words = long_word_rows(env)[L]
    assert startless_trips(env, ids) >= (3 if L == 400 else 30)
    seen = {w: set() for w in words}
    for seed in range(10):
        got = check(tok, env, ids, p=0.5, seed=seed)
        for (r, a, b) in words:
            picked = got["labels"][r, a:b + 1] != -100
            assert picked.all() or not picked.any(), (seed, r, a, b)
            seen[(r, a, b)].add(bool(picked[0]))
        check(tok, env, ids, p=0.5, seed=seed, whole_word=False)
    assert all(v == {False, True} for v in seen.values()), seen


def test_ids_outside_the_snapshot_are_plain_tokens(tok, env):
    n, c = env["n_ids"], int(env["cont"][0])
    odd = [-1, -5, n, n + 1, 2 ** 31 - 1, -2 ** 31, n + 7, -1]
    ids = np.array([odd, [c, -1, c, n, c, 2 ** 31 - 1, c, -2 ** 31], [env["bos"], -1, n, env["eos"], env["pad"], env["pad"], -3, n]], dtype=np.int32)
    for ww in (True, False):
        for seed in range(4):
            check(tok, env, ids, p=0.5, seed=seed, whole_word=ww)
        got = tok.mask_rows(ids, p=1.0, mask_prob=0.0, random_prob=0.0, whole_word=ww)
        assert np.array_equal(got["input_ids"], ids)
        assert np.array_equal(got["labels"][0], ids[0]) and np.array_equal(got["labels"][1], ids[1])     # chosen, and the label is the id itself
        assert got["labels"][2].tolist() == [-100, -1, n, -100, -100, -100, -3, n]
    # none of them continues a word: each starts one, so with whole_word the cells of row 0 decide one by one
    t_sel = MO.thresholds(0.5)[0]
    x0 = MO.draw(np.arange(8, dtype=np.uint64), 3)[0]
    assert ((tok.mask_rows(ids[:1], p=0.5, seed=3)["labels"][0] != -100) == (x0 < t_sel)).all()


def test_a_real_token_equal_to_the_pad_id_is_protected(tok, env):
    x, c = int(env["plain"][0]), int(env["cont"][0])
    ids = np.array([[env["bos"], x, env["pad"], x, c, env["pad"], x, env["eos"], env["pad"]]], dtype=np.int32)
    for seed in range(4):
        check(tok, env, ids, p=0.5, seed=seed)
    got = tok.mask_rows(ids, p=1.0)
    assert got["labels"][0].tolist() == [-100, x, -100, x, c, -100, x, -100, -100] and got["n_chosen"].tolist() == [4]
    assert (got["input_ids"][0][[0, 2, 5, 7, 8]] == ids[0][[0, 2, 5, 7, 8]]).all()


def test_thresholds(tok, env):
    rng = np.random.default_rng(5)
    ids = framed_rows(env, rng, 40, 70)
    real = ~np.isin(ids, [env["pad"], env["bos"], env["eos"], env["mask"]])
    got = tok.mask_rows(ids, p=0.0)
    same(got, want_of(env, ids, p=0.0))
    assert np.array_equal(got["input_ids"], ids) and (got["labels"] == -100).all() and not got["n_chosen"].any()
    for ww in (True, False):
        got = tok.mask_rows(ids, p=1.0, whole_word=ww)
        same(got, want_of(env, ids, p=1.0, whole_word=ww))
        assert np.array_equal(got["labels"] != -100, real) and np.array_equal(got["n_chosen"], real.sum(axis=1))
    got = tok.mask_rows(ids, p=1.0, mask_prob=1.0, random_prob=0.0)
    same(got, want_of(env, ids, p=1.0, mask_prob=1.0, random_prob=0.0))
    assert (got["input_ids"][real] == env["mask"]).all() and np.array_equal(got["input_ids"][~real], ids[~real])
    wide = (0, 2 ** 31 - 1)                                          # x2 shows through the ids
    got = tok.mask_rows(ids, p=1.0, mask_prob=0.0, random_prob=1.0, random_ids=wide, seed=9)
    same(got, want_of(env, ids, p=1.0, mask_prob=0.0, random_prob=1.0, random_ids=wide, seed=9))
    g = np.arange(ids.size, dtype=np.uint64).reshape(ids.shape)
    x2 = MO.draw(g, 9)[2]
    assert np.array_equal(got["input_ids"][real], ((x2[real] * np.uint64(2 ** 31 - 1)) >> np.uint64(32)).astype(np.int32))
    assert len(np.unique(got["input_ids"][real])) > real.sum() // 2
    got = tok.mask_rows(ids, p=1.0, mask_prob=0.0, random_prob=1.0, random_ids=(7, 8))
    same(got, want_of(env, ids, p=1.0, mask_prob=0.0, random_prob=1.0, random_ids=(7, 8)))
    assert (got["input_ids"][real] == 7).all()
    got = tok.mask_rows(ids, p=0.3, ignore_index=-7, seed=2)
    same(got, want_of(env, ids, p=0.3, ignore_index=-7, seed=2))
    assert (got["labels"][~real] == -7).all() and (got["labels"] == -7).sum() > (~real).sum()
    check(tok, env, ids, p=0.3, mask_prob=0.5, random_prob=0.5, seed=4)                  # t2 = 2^32: "always"
    check(tok, env, ids, p=0.3, mask_prob=0.25, random_prob=0.25, random_ids=(-40, -3), seed=4)


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
    one, two = tok.mask_rows(ids, p=0.5, seed=hi), tok.mask_rows(ids, p=0.5, seed=hi)
    for k in KEYS:
        assert np.array_equal(one[k], two[k])


def test_slices_with_row_base_are_the_slices_of_the_batch(tok, env):
    rng = np.random.default_rng(8)
    for L in (64, 37):
        ids = framed_rows(env, rng, 130, L)
        whole = check(tok, env, ids, p=0.3, seed=11, row_base=5)
        cuts = [0, 1, 64, 65, 130]
        parts = [tok.mask_rows(ids[a:b], p=0.3, seed=11, row_base=5 + a) for a, b in zip(cuts[:-1], cuts[1:])]
        for k in KEYS:
            assert np.array_equal(np.concatenate([q[k] for q in parts]), whole[k]), k


TEXTS = ["công nghệ thông tin và truyền thông", "xin chào thế giới", "", "trăm中 phần trăm 中", "một hai ba bốn năm sáu bảy tám chín mười " * 6,
         "internationalization antidisestablishmentarianism", "a"] * 9


def test_device_rows_of_window_and_pack_calls(tok, env):
    for make, L in ((lambda: tok.encode_windows_to_device(TEXTS, 16, 4), 16), (lambda: tok.encode_packs_to_device(TEXTS, 24), 24),
                    (lambda: tok.encode_to_device(TEXTS, max_len=13), 13)):
        rows = make()["input_ids"]
        host = rows.numpy()
        assert host.shape[1] == L and host.shape[0] > 8
        for ww in (True, False):
            got = tok.mask_rows_to_device(rows, p=0.4, seed=3, whole_word=ww, row_base=17)
            assert got["input_ids"].shape == host.shape and got["labels"].shape == host.shape
            got = dict(input_ids=got["input_ids"].numpy(), labels=got["labels"].numpy(), n_chosen=got["n_chosen"])
            same(got, tok.mask_rows(host, p=0.4, seed=3, whole_word=ww, row_base=17))
            same(got, want_of(env, host, p=0.4, seed=3, whole_word=ww, row_base=17))
        assert np.array_equal(rows.numpy(), host)                    # the source rows are not changed


def test_raw_device_call_directly_behind_the_window_call(tok, env):
    """gz_mask_rows_device enqueued behind gz_window_rows_device on the context's stream, no gz_sync in between"""
    ctx = tok._ctx
    rng = np.random.default_rng(12)
    bodies = [framed_rows(env, rng, 1, n)[0] for n in (3, 40, 7, 90, 5)]
    flat = np.concatenate(bodies).astype(np.int32)
    off = np.zeros(len(bodies) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in bodies])
    L, s = 16, 3
    want_rows = tok.window_rows(bodies, L, s)["input_ids"]
    W = len(want_rows)
    rule = (5, *MO.thresholds(0.5), 5, env["n_ids"], env["mask"], 1, -100)
    bufs = [ctx.alloc(n) for n in (flat.nbytes + 64, off.nbytes, off.nbytes, 4 * W * L, 4 * W * L, 4 * W * L, 4 * W)]
    d_ids, d_off, d_wo, d_rows, d_out, d_lab, d_cnt = bufs
    try:
        ctx.h2d(d_ids, flat)
        ctx.h2d(d_off, off)
        assert ctx.window_rows_device(d_ids, d_off, len(bodies), L, s, 1, 1, d_rows, 0, 0, 0, 0, d_wo, W) == W
        ctx.mask_rows_device(d_rows, W, L, 0, rule, d_out, d_lab, d_cnt)
        got = dict(input_ids=np.empty((W, L), np.int32), labels=np.empty((W, L), np.int32), n_chosen=np.empty(W, np.int32))
        ctx.d2h(got["input_ids"], d_out); ctx.d2h(got["labels"], d_lab); ctx.d2h(got["n_chosen"], d_cnt)
    finally:
        for d in bufs:
            ctx.free(d)
    same(got, want_of(env, want_rows, p=0.5, seed=5))


def test_words_of_real_texts_go_together(tok, env):
    split_seen = False
    for text in TEXTS[:7]:
        r = tok(text, return_offset=True)
        ids = np.array([r["input_ids"]], dtype=np.int32)
        spans = [(a, b) for a, b in r["offset"][1:-1]]
        for seed in range(4):
            want = check(tok, env, ids, p=0.5, seed=seed)
            picked = want["labels"][0] != -100
            for a, b in spans:
                assert picked[a:b + 1].all() or not picked[a:b + 1].any(), (text, seed, a, b)
            loose = check(tok, env, ids, p=0.5, seed=seed, whole_word=False)["labels"][0] != -100
            split_seen |= any(loose[a:b + 1].any() and not loose[a:b + 1].all() for a, b in spans)
    assert split_seen


def raw_args(env, R=2, L=8, row_base=0, seed=1, t_sel=2 ** 31, t1=2 ** 31, t2=2 ** 32, lo=5, hi=9, whole_word=1, ignore=-100):
    return [R, L, row_base, seed, t_sel, t1, t2, lo, hi, env["mask"], whole_word, ignore]


def test_refusals_leave_the_outputs_untouched(tok, env):
    from genz_tokenize import _native
    tok._sync_tables()
    ctx = tok._ctx
    lib = ctx.lib
    ids = np.full((2, 8), int(env["plain"][0]), dtype=np.int32)
    out, lab, cnt = np.full((2, 8), -9, np.int32), np.full((2, 8), -9, np.int32), np.full(2, -9, np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)                     # noqa: E731
    bad = [dict(L=0), dict(L=-1), dict(R=-1), dict(row_base=-1), dict(row_base=2 ** 63 // 8 - 2), dict(row_base=2 ** 63 - 1),
           dict(t_sel=2 ** 32 + 1), dict(t1=2 ** 32 + 1, t2=2 ** 32 + 1), dict(t2=2 ** 32 + 1), dict(t1=9, t2=8), dict(lo=9, hi=9), dict(lo=9, hi=3),
           dict(whole_word=2), dict(whole_word=-1)]
    for kw in bad:
        rc = lib.gz_mask_rows(ctx.handle, P(ids), *raw_args(env, **kw), P(out), P(lab), P(cnt))
        assert rc == _native.GZ_E_INVALID, kw
    for trio in ((None, P(out), P(lab)), (P(ids), None, P(lab)), (P(ids), P(out), None)):
        assert lib.gz_mask_rows(ctx.handle, trio[0], *raw_args(env), trio[1], trio[2], P(cnt)) == _native.GZ_E_INVALID
    big = np.full(40, -9, np.int32)                                  # overlapping buffers: out on ids, labels on out, by one cell
    at = lambda k: ctypes.c_void_p(big.ctypes.data + 4 * k)          # noqa: E731
    for a, b, c in ((at(0), at(0), P(lab)), (at(0), at(15), P(lab)), (P(ids), at(0), at(15)), (at(0), P(out), at(15)), (at(15), at(0), P(lab))):
        assert lib.gz_mask_rows(ctx.handle, a, *raw_args(env), b, c, P(cnt)) == _native.GZ_E_INVALID
    assert (big == -9).all() and (out == -9).all() and (lab == -9).all() and (cnt == -9).all()
    # the device form refuses the same things, before anything is launched
    bufs = [ctx.alloc(4 * 40) for _ in range(4)]
    d_ids, d_out, d_lab, d_cnt = bufs
    vp = ctypes.c_void_p
    try:
        for d in (d_out, d_lab, d_cnt):
            ctx.h2d(d, big)
        ctx.h2d(d_ids, ids)
        for kw in bad:
            assert lib.gz_mask_rows_device(ctx.handle, vp(d_ids), *raw_args(env, **kw), vp(d_out), vp(d_lab), vp(d_cnt)) == _native.GZ_E_INVALID, kw
        for trio in ((None, vp(d_out), vp(d_lab)), (vp(d_ids), None, vp(d_lab)), (vp(d_ids), vp(d_out), None)):
            assert lib.gz_mask_rows_device(ctx.handle, trio[0], *raw_args(env), trio[1], trio[2], vp(d_cnt)) == _native.GZ_E_INVALID
        # 16 cells are 64 bytes: + 60 overlaps by one cell; the last case puts n_chosen inside labels
        for a, b, c, n in ((d_ids, d_ids, d_lab, d_cnt), (d_ids, d_ids + 60, d_lab, d_cnt), (d_ids, d_out, d_out + 60, d_cnt),
                           (d_ids, d_out, d_ids + 60, d_cnt), (d_ids, d_out, d_lab, d_lab + 60)):
            assert lib.gz_mask_rows_device(ctx.handle, vp(a), *raw_args(env), vp(b), vp(c), vp(n)) == _native.GZ_E_INVALID
        back = np.empty(40, np.int32)
        for d in (d_out, d_lab, d_cnt):
            ctx.d2h(back, d)
            assert (back == -9).all()
        # R == 0 is fine and writes nothing; NULL pointers are allowed then
        assert lib.gz_mask_rows_device(ctx.handle, None, *raw_args(env, R=0), None, None, None) == _native.GZ_OK
        assert lib.gz_mask_rows(ctx.handle, None, *raw_args(env, R=0), None, None, None) == _native.GZ_OK
        # n_chosen may be NULL
        assert lib.gz_mask_rows_device(ctx.handle, vp(d_ids), *raw_args(env), vp(d_out), vp(d_lab), None) == _native.GZ_OK
        got = np.empty((2, 8), np.int32)
        ctx.d2h(got, d_lab)
        assert np.array_equal(got, want_of(env, ids, p=0.5, mask_prob=0.5, random_prob=0.5, random_ids=(5, 9), seed=1)["labels"])
    finally:
        for d in bufs:
            ctx.free(d)
    # a context without a decoder snapshot gives the decode call's error
    fresh = _native.Context()
    try:
        rc = fresh.lib.gz_mask_rows(fresh.handle, P(ids), *raw_args(env), P(out), P(lab), P(cnt))
        assert rc == _native.GZ_E_NOTABLES and (out == -9).all()
    finally:
        fresh.close()


def test_python_refusals_come_before_any_launch(tok):
    ids = np.zeros((2, 4), dtype=np.int32)
    for kw, exc in ((dict(p=1.5), ValueError), (dict(p=True), TypeError), (dict(seed=-1), ValueError), (dict(seed=1.0), TypeError),
                    (dict(mask_prob=0.8, random_prob=0.3), ValueError), (dict(random_ids=(5, 5)), ValueError), (dict(row_base=True), TypeError)):
        with pytest.raises(exc):
            tok.mask_rows(ids, **kw)
    with pytest.raises(TypeError):
        tok.mask_rows_to_device(ids)
    with pytest.raises(TypeError):
        tok.mask_rows(ids.astype(np.float32))
    with pytest.raises(ValueError):
        tok.mask_rows(ids[0])
    with pytest.raises(ValueError):
        tok.mask_rows(np.array([[2 ** 31]]))
    with pytest.raises(ValueError):
        tok.mask_rows(ids, row_base=2 ** 63 // 4)
    out = tok.mask_rows(np.zeros((0, 7), dtype=np.int32))
    assert out["input_ids"].shape == (0, 7) and out["labels"].shape == (0, 7) and out["n_chosen"].shape == (0,)
