"""MinHash signatures and near-duplicate groups on the GPU (gz_minhash_rows / _device, gz_minhash_groups / _device;
Tokenize.minhash_rows, encode_minhash, encode_minhash_to_device, minhash_groups, near_duplicates) against the rule of
tests/minhash_oracle.py, which tests/test_minhash_inputs.py ties to known answers, to a second restatement and to the Jaccard index
it estimates.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import minhash_oracle as MO
import window_oracle as WO

pytestmark = pytest.mark.gpu

PIECE = 4096                                                             # shingle positions a wave takes (csrc/gz_pieces.inc: GZ_PIECE)
M32 = 0xFFFFFFFF
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


def counters(lengths, base=1000):
    """Bodies whose ids count up across the batch: a token taken from the wrong place shows."""
    out, at = [], base
    for T in lengths:
        out.append(list(range(at, at + T)))
        at += T
    return out


def same(got, want):
    for k in ("signatures", "n_shingles"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())


def check(tok, bodies, K=128, w=5, seed=0):
    want = MO.batch(bodies, K, w, seed)
    same(tok.minhash_rows(bodies, K, w, seed, framed=False), want)
    return want


# ---- signatures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 5, 32])
def test_body_lengths_at_the_rules_and_the_trips_edges(tok, w):
    """nothing, one id, around the shingle width; around one and two trips of 64 shingle positions"""
    lengths = sorted({0, 1, max(w - 1, 0), w, w + 1} | {s + w - 1 for s in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)})
    want = check(tok, counters(lengths), 65, w, 3)
    assert want["n_shingles"].tolist() == [0 if n == 0 else max(n - w + 1, 1) for n in lengths]
    for n in (0, 1, w, 64 + w - 1, 65 + w - 1):                          # ... and as batches of their own
        check(tok, counters([n]), 65, w, 3)


@pytest.mark.parametrize("w", [1, 5])
def test_body_lengths_around_the_piece(tok, w):
    """one below, at and above one piece and two: rows of more than one piece are split over waves and meet by atomicMin"""
    lengths = [s + w - 1 for s in (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1)]
    check(tok, counters(lengths) + counters([3, 0, PIECE + 70]), 64, w, 1)
    for n in (PIECE + w - 1, PIECE + w):                                 # one piece alone; two pieces alone
        check(tok, counters([n]), 3, w, 1)


def test_one_long_body_between_short_ones(tok):
    rng = np.random.default_rng(8)
    bodies = [[7, 8, 9], rng.integers(5, 48423, size=200000).tolist(), [9, 8, 7], [], [7, 8, 9]]
    want = check(tok, bodies, 32, 5, 11)
    assert want["n_shingles"].tolist() == [1, 199996, 1, 0, 1] and np.array_equal(want["signatures"][0], want["signatures"][4])


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128, 255, 256])
def test_signature_widths(tok, K):
    rng = np.random.default_rng(K)
    check(tok, [[], [5], rng.integers(5, 48423, size=3).tolist(), rng.integers(5, 48423, size=70).tolist(), rng.integers(5, 48423, size=200).tolist()],
          K, 5, K)


@pytest.mark.parametrize("N", [0, 1, 2, 63, 64, 65, 257])
def test_row_counts_at_block_edges(tok, N):
    rng = np.random.default_rng(N)
    lengths = rng.integers(0, 90, size=N).tolist()
    got = tok.minhash_rows(counters(lengths), 16, 5, 2, framed=False)
    same(got, MO.batch(counters(lengths), 16, 5, 2))
    assert got["signatures"].shape == (N, 16) and got["n_shingles"].shape == (N,)


def test_odd_ids_and_counting_ids(tok):
    odd = [-1, 0, -2 ** 31, 2 ** 31 - 1, 5, 48422, 70000]
    rng = np.random.default_rng(4)
    check(tok, [rng.choice(odd, size=n).tolist() for n in (1, 4, 5, 6, 70, 300)] + [odd, [-1], [0], [-2 ** 31], [2 ** 31 - 1]], 64, 5, 0)
    check(tok, counters([70, 1, 130, 64, 5], base=-100), 64, 5, 0)


def test_framed_against_bare_bodies(tok):
    bodies = counters([0, 1, 4, 5, 6, 70])
    want = MO.batch(bodies, 32, 5, 6)
    framed = [[-7] + b + [-9] for b in bodies]                           # the frame is dropped whatever it holds
    same(tok.minhash_rows(framed, 32, 5, 6, framed=True), want)
    same(tok.minhash_rows(framed, 32, 5, 6), want)                       # framed is the default
    got = tok.minhash_rows([[], [5], [5, 6], [5, 7, 6]], 32, 5, 6, framed=True)            # rows shorter than their frame: empty bodies
    same(got, MO.batch([[], [], [], [7]], 32, 5, 6))
    assert (got["signatures"][:3] == M32).all()
    rows = np.arange(5 * 11, dtype=np.int64).reshape(5, 11) + 50         # a 2-D array of rows
    same(tok.minhash_rows(rows, 32, 5, 6), MO.batch([r[1:-1].tolist() for r in rows], 32, 5, 6))


@pytest.mark.parametrize("seed", [0, 2 ** 32, 2 ** 64 - 1, 0x123456789ABCDEF0])
def test_seeds(tok, seed):
    want = check(tok, counters([0, 3, 70, 200]), 128, 5, seed)
    if seed:
        assert not np.array_equal(want["signatures"][2], MO.batch(counters([0, 3, 70, 200]), 128, 5, 0)["signatures"][2])


def test_slices_equal_the_whole(tok):
    rng = np.random.default_rng(12)
    bodies = [rng.integers(5, 48423, size=int(n)).tolist() for n in rng.integers(0, 150, size=90)] + counters([PIECE + 300])
    whole = tok.minhash_rows(bodies, 64, 5, 9, framed=False)
    for a, b in ((0, 91), (0, 1), (17, 64), (64, 91), (90, 91), (5, 5)):
        part = tok.minhash_rows(bodies[a:b], 64, 5, 9, framed=False)
        assert np.array_equal(part["signatures"], whole["signatures"][a:b]) and np.array_equal(part["n_shingles"], whole["n_shingles"][a:b])
    cat = np.concatenate([tok.minhash_rows(bodies[:40], 64, 5, 9, framed=False)["signatures"], tok.minhash_rows(bodies[40:], 64, 5, 9, framed=False)["signatures"]])
    assert np.array_equal(cat, whole["signatures"])


def test_a_bare_context_is_enough():
    """neither pass needs the tables or the decoder snapshot"""
    from genz_tokenize import _native
    ctx = _native.Context()
    try:
        bodies = counters([0, 3, 70])
        flat = np.array([v for b in bodies for v in b], dtype=np.int32)
        off = np.array([0, 0, 3, 73], dtype=np.int64)
        got = ctx.minhash_rows(flat, off, 16, 5, 0, False)
        same(got, MO.batch(bodies, 16, 5, 0))
        sig = np.concatenate([got["signatures"], got["signatures"]])
        group, n = ctx.minhash_groups(sig, 4, 16)
        assert group.tolist() == [0, 1, 2, 3, 1, 2] and n == 4
    finally:
        ctx.close()


class Guarded:
    """n 32-bit cells on the device between two runs of guard cells, all pre-filled with FILL."""

    def __init__(self, ctx, n, guard=64, dtype=np.int32):
        self.ctx, self.n, self.guard, self.dtype = ctx, n, guard, dtype
        self.base = ctx.alloc(4 * (n + 2 * guard) + 16)
        ctx.h2d(self.base, np.full(n + 2 * guard, FILL, dtype=dtype))
        self.ptr = self.base + 4 * guard

    def read(self):
        a = np.empty(self.n + 2 * self.guard, dtype=self.dtype)
        self.ctx.d2h(a, self.base)
        assert (a[:self.guard] == FILL).all() and (a[self.guard + self.n:] == FILL).all(), "guard cells were written"
        return a[self.guard:self.guard + self.n]

    def free(self):
        self.ctx.free(self.base)


def test_device_form_behind_junk(tok):
    """The rows lie behind a prefix of junk (row_off_dev[0] != 0); n_shingles left out; nothing outside the outputs is written."""
    ctx = tok._ctx
    bodies = counters([0, 3, 70, PIECE + 9, 0, 1, 130])
    junk, K, n = 37, 65, 7
    flat = np.array([-77] * junk + [v for b in bodies for v in b] + [-88] * 5, dtype=np.int32)
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bodies], out=ro[1:])
    ro += junk
    want = MO.batch(bodies, K, 5, 3)
    d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
    g = [Guarded(ctx, n * K, dtype=np.uint32), Guarded(ctx, n), Guarded(ctx, n * K, dtype=np.uint32)]
    try:
        ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
        ctx.minhash_rows_device(d_ids, d_ro, n, 0, 0, 5, K, 3, g[0].ptr, g[1].ptr)
        same(dict(signatures=g[0].read().reshape(n, K), n_shingles=g[1].read()), want)
        ctx.minhash_rows_device(d_ids, d_ro, n, 0, 0, 5, K, 3, g[2].ptr, 0)
        assert np.array_equal(g[2].read().reshape(n, K), want["signatures"])
        # with skips: the junk's last word and the first tail word are a frame nobody reads
        ro2 = np.array([junk - 1, int(ro[-1]) + 1], dtype=np.int64)
        ctx.h2d(d_ro, ro2)
        ctx.minhash_rows_device(d_ids, d_ro, 1, 1, 1, 5, K, 3, g[0].ptr, g[1].ptr)
        one = MO.batch([[v for b in bodies for v in b]], K, 5, 3)
        assert np.array_equal(g[0].read()[:K], one["signatures"][0]) and g[1].read()[0] == one["n_shingles"][0]
    finally:
        for x in g:
            x.free()
        ctx.free(d_ids); ctx.free(d_ro)


@pytest.fixture(scope="module")
def corpus_rows(tok):
    from genz_tokenize._packing import pack
    texts = WO.texts(300, 60, 5)
    t, o = pack(texts)
    r = tok.encode_packed(t, o, max_len=None)
    ro = r["row_off"]
    return texts, [r["input_ids"][ro[i]:ro[i + 1]].tolist() for i in range(len(texts))]


def test_text_end_to_end(tok, corpus_rows):
    texts, rows = corpus_rows
    want = MO.batch(rows, 128, 5, 0, framed=True)
    assert (want["n_shingles"] == 0).any() and (want["n_shingles"] > 1).any()
    got = tok.encode_minhash(texts)
    assert got.dtype == np.uint32 and np.array_equal(got, want["signatures"])
    assert np.array_equal(tok.encode_minhash(texts, word_table=False), want["signatures"])
    same(tok.minhash_rows(rows), want)
    assert np.array_equal(tok.encode_minhash(texts[40:90], 64, 3, 7), MO.batch(rows[40:90], 64, 3, 7, framed=True)["signatures"])
    dev = tok.encode_minhash_to_device(texts)
    assert dev.shape == (300, 128) and dev.dtype == np.uint32 and dev.nbytes == 300 * 128 * 4
    assert np.array_equal(dev.numpy(), want["signatures"])
    for empty in ([], [""], ["", "   "]):
        got = tok.encode_minhash(empty, 8)
        assert got.shape == (len(empty), 8) and (got == M32).all()
        assert tok.encode_minhash_to_device(empty, 8).numpy().shape == (len(empty), 8)
        assert tok.near_duplicates(empty, 8, bands=2)["group"].tolist() == list(range(len(empty)))


# ---- groups: signatures crafted so that the graph is known ------------------------------------------------------------------
def device_sig(tok, sig):
    from genz_tokenize.handoff import DeviceArray
    ctx = tok._ctx
    d = ctx.alloc(max(sig.nbytes, 1) + 64)
    if sig.nbytes:
        ctx.h2d(d, np.ascontiguousarray(sig))
    return DeviceArray(ctx, d, sig.shape, dtype=np.uint32)


def both(tok, sig, **kw):
    """the host form and the device form agree; the result of either"""
    sig = np.ascontiguousarray(sig, dtype=np.uint32)
    a = tok.minhash_groups(sig, **kw)
    b = tok.minhash_groups(device_sig(tok, sig), **kw)
    N = len(sig)
    for r in (a, b):
        assert r["group"].dtype == np.int32 and r["group"].shape == (N,) and r["keep"].dtype == bool and type(r["n_groups"]) is int
        assert np.array_equal(r["keep"], r["group"] == np.arange(N)) and r["n_groups"] == int(r["keep"].sum())
    assert np.array_equal(a["group"], b["group"])
    return a


def distinct(rng, N, K):
    """rows without a common value in any slot: no two share a band"""
    return (rng.permutation(N * K).reshape(N, K) + 1).astype(np.uint32)


def test_all_distinct(tok):
    r = both(tok, distinct(np.random.default_rng(1), 500, 16), bands=4, min_agree=1)
    assert r["group"].tolist() == list(range(500)) and r["n_groups"] == 500


def test_identical_rows_contend_for_one_slot(tok):
    sig = np.tile(np.arange(7, 7 + 32, dtype=np.uint32), (4096, 1))
    r = both(tok, sig, bands=8, min_agree=32)
    assert (r["group"] == 0).all() and r["n_groups"] == 1


@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025])
def test_row_counts_at_table_sizes(tok, N):
    """2 N at a power of two and beside it; rows drawn from few values a slot, so that buckets are shared and some pairs agree"""
    rng = np.random.default_rng(N)
    sig = rng.integers(0, 3, size=(N, 8)).astype(np.uint32)
    sig[rng.integers(0, N, size=N // 10)] = M32
    want = MO.groups(sig, bands=4, min_agree=6)
    r = both(tok, sig, bands=4, min_agree=6)
    assert np.array_equal(r["group"], want["group"]) and r["n_groups"] == want["n_groups"]
    if N > 2:
        assert 1 < want["n_groups"] < N


def test_chain(tok):
    """row i shares exactly slot i % K with row i - 1 and nothing else: one group whose label is 0, in either order"""
    N, K = 5000, 16
    sig = (np.arange(N * K, dtype=np.uint32).reshape(N, K) + 1)
    for i in range(1, N):
        sig[i, i % K] = sig[i - 1, i % K]
    assert all(int((sig[i] == sig[i - 1]).sum()) == 1 for i in range(1, N)) and int((sig[2] == sig[0]).sum()) == 0
    for s in (sig, sig[::-1]):
        r = both(tok, s, bands=K, min_agree=1)
        assert (r["group"] == 0).all() and r["n_groups"] == 1
    assert both(tok, sig, bands=K, min_agree=2)["n_groups"] == N


def test_bucket_refusal(tok):
    """b and c agree everywhere and with the smaller a in one band only: at min_agree = K the band they share with a asks a alone
    and refuses, the other bands join b and c"""
    a = [1, 2, 3, 4, 5, 6, 7, 8]
    b = [1, 2, 13, 14, 15, 16, 17, 18]
    r = both(tok, np.array([a, b, b]), bands=4, min_agree=8)
    assert r["group"].tolist() == [0, 1, 1]
    # with that band alone nothing joins them: c = b but for one slot outside the band, and min_agree = 3 refuses a
    r = both(tok, np.array([[1, 1, 5, 6], [1, 1, 7, 8], [1, 1, 7, 9]]), bands=2, min_agree=3)
    assert r["group"].tolist() == [0, 1, 2]


def test_min_agree_at_its_edge(tok):
    K = 16
    x = np.arange(100, 100 + K, dtype=np.uint32)
    y = x.copy(); y[K - 1] = 999                                         # K - 1 agreements, every band but the last shared
    filler = distinct(np.random.default_rng(2), 5, K) + 5000
    sig = np.concatenate([filler[:2], x[None], filler[2:], y[None]])
    assert both(tok, sig, bands=4, min_agree=K)["group"].tolist() == list(range(7))
    assert both(tok, sig, bands=4, min_agree=K - 1)["group"].tolist() == [0, 1, 2, 3, 4, 5, 2]


def test_empty_rows(tok):
    rng = np.random.default_rng(3)
    sig = distinct(rng, 40, 8)
    sig[[0, 7, 8, 39]] = M32                                             # empty rows among the rest: each stays alone
    sig[20] = sig[3]; sig[30] = sig[3]
    sig[12, :7] = M32                                                    # one real slot: not empty
    sig[13] = sig[12]
    want = list(range(40)); want[20] = want[30] = 3; want[13] = 12
    assert both(tok, sig, bands=2, min_agree=8)["group"].tolist() == want
    only = np.full((70, 8), M32, dtype=np.uint32)
    r = both(tok, only, bands=2, min_agree=1)
    assert r["group"].tolist() == list(range(70)) and r["n_groups"] == 70


@pytest.mark.parametrize("bands", [1, 8])
def test_one_band_and_a_band_a_slot(tok, bands):
    rng = np.random.default_rng(bands)
    sig = rng.integers(0, 3, size=(300, 8)).astype(np.uint32)
    sig[100:150] = sig[:50]
    for m in (1, 5, 8):
        want = MO.groups(sig, bands=bands, min_agree=m)
        assert np.array_equal(both(tok, sig, bands=bands, min_agree=m)["group"], want["group"]), m


def test_back_to_back_calls_reset_the_table(tok):
    rng = np.random.default_rng(5)
    big = rng.integers(0, 4, size=(3000, 8)).astype(np.uint32)
    small = big[1000:1100][::-1].copy()
    for sig in (big, small, big[:7], small):
        want = MO.groups(sig, bands=4, min_agree=5)
        assert np.array_equal(both(tok, sig, bands=4, min_agree=5)["group"], want["group"])


def test_default_min_agree_is_the_thresholds(tok):
    sig = distinct(np.random.default_rng(6), 6, 128)
    sig[4] = sig[1]; sig[4, :38] = 0                                     # 90 of 128 slots agree, bands 5 .. 15 shared (no row holds a 0)
    sig[5] = sig[2]; sig[5, :39] = 0                                     # 89 of 128
    assert both(tok, sig)["group"].tolist() == [0, 1, 2, 3, 1, 5]        # bands = 16, threshold = 0.7: min_agree = 90
    assert both(tok, sig, threshold=0.69)["group"].tolist() == [0, 1, 2, 3, 1, 2]


# ---- planted families, end to end from texts --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_token_words(tok):
    """(words, ids): vocabulary words that encode to exactly one token, so that a text of them has a known body"""
    dec = tok.decoder
    cand = [(i, dec[i]) for i in range(5, min(tok.vocab_size(), 6000)) if i in dec and not dec[i].endswith("@@") and dec[i].strip() == dec[i] and dec[i]]
    r = tok.encode_batch([w for _, w in cand], max_len=None)
    ro, ids = r["row_off"], r["input_ids"]
    good = [(w, i) for k, (i, w) in enumerate(cand) if ro[k + 1] - ro[k] == 3 and ids[ro[k] + 1] == i]
    assert len(good) >= 1000
    return [w for w, _ in good], np.array([i for _, i in good], dtype=np.int64)


@pytest.mark.parametrize("threshold", [0.5, 0.7])
def test_planted_families_from_texts(tok, one_token_words, threshold):
    words, ids = one_token_words
    picks, fam = MO.families(0, lo=0, hi=len(words))
    texts = [" ".join(words[i] for i in b) for b in picks]
    bodies = [ids[b].tolist() if b else [] for b in picks]
    assert np.array_equal(tok.encode_minhash(texts), MO.batch(bodies, 128, 5, 0)["signatures"])
    r = tok.near_duplicates(texts, threshold=threshold)
    assert r["group"].tolist() == MO.family_groups(fam).tolist()
    assert r["n_groups"] == 42 and int(r["keep"].sum()) == 42


# ---- refusals at the ABI ----------------------------------------------------------------------------------------------------
def test_refusals_of_the_rows_calls(tok):
    from genz_tokenize import _native
    ctx, lib, P = tok._ctx, tok._ctx.lib, _native._ptr
    ids = np.arange(10, dtype=np.int32)
    ro = np.array([0, 4, 10], dtype=np.int64)
    d_ids, d_ro = ctx.alloc(64), ctx.alloc(64)
    g_sig, g_cnt = Guarded(ctx, 2 * 256, dtype=np.uint32), Guarded(ctx, 2)
    said = set()

    def refused(code, call):
        sig = np.full((2, 256), FILL, dtype=np.uint32); cnt = np.full(2, FILL, dtype=np.int32)
        assert call(lib.gz_minhash_rows, P(ids), P(ro), P(sig), P(cnt)) == code
        said.add(lib.gz_last_error(ctx.handle))
        assert (sig == FILL).all() and (cnt == FILL).all()
        vp = ctypes.c_void_p
        assert call(lib.gz_minhash_rows_device, vp(d_ids), vp(d_ro), vp(g_sig.ptr), vp(g_cnt.ptr)) == code
        assert lib.gz_last_error(ctx.handle) in said
        assert (g_sig.read() == FILL).all() and (g_cnt.read() == FILL).all()
    try:
        ctx.h2d(d_ids, ids); ctx.h2d(d_ro, ro)
        h = ctx.handle
        INV = _native.GZ_E_INVALID
        refused(INV, lambda f, i, o, s, c: f(h, i, o, -1, 0, 0, 5, 128, 0, s, c))
        for sf, sb in ((2, 0), (0, 2), (-1, 0), (0, -1)):
            refused(INV, lambda f, i, o, s, c: f(h, i, o, 2, sf, sb, 5, 128, 0, s, c))
        for w in (0, 33, -1):
            refused(INV, lambda f, i, o, s, c: f(h, i, o, 2, 0, 0, w, 128, 0, s, c))
        for K in (0, 257, -1):
            refused(INV, lambda f, i, o, s, c: f(h, i, o, 2, 0, 0, 5, K, 0, s, c))
        assert len(said) == 4                                             # each rule has its own sentence
        refused(INV, lambda f, i, o, s, c: f(h, i, None, 2, 0, 0, 5, 128, 0, s, c))
        refused(INV, lambda f, i, o, s, c: f(h, i, o, 2, 0, 0, 5, 128, 0, None, c))
        refused(INV, lambda f, i, o, s, c: f(h, i, o, 2, 0, 0, 5, 128, 0, s, s))                 # n_shingles inside signatures
        refused(INV, lambda f, i, o, s, c: f(h, i, o, 2, 0, 0, 5, 1, 0, i, c))                   # signatures over the ids
        refused(INV, lambda f, i, o, s, c: f(h, i, o, 2, 0, 0, 5, 1, 0, o, c))                   # signatures over the offsets
        # the host form's own: offsets
        sig = np.full((2, 8), FILL, dtype=np.uint32)
        for bad, words in ((np.array([0, 7, 4], dtype=np.int64), b"row offsets must not decrease"), (np.array([5, 6, 2], dtype=np.int64), b"bad row offsets")):
            assert lib.gz_minhash_rows(h, P(ids), P(bad), 2, 0, 0, 5, 8, 0, P(sig), None) == INV
            assert words in lib.gz_last_error(h) and (sig == FILL).all()
        assert lib.gz_minhash_rows(h, None, P(ro), 2, 0, 0, 5, 8, 0, P(sig), None) == INV and b"bad row offsets" in lib.gz_last_error(h)
        # nothing to do is no error: nothing is written, no pointer is needed
        assert lib.gz_minhash_rows(h, None, None, 0, 0, 0, 5, 8, 0, None, None) == _native.GZ_OK
        assert lib.gz_minhash_rows_device(h, None, None, 0, 1, 1, 5, 8, 0, None, None) == _native.GZ_OK
        assert lib.gz_minhash_rows(None, P(ids), P(ro), 2, 0, 0, 5, 8, 0, P(sig), None) == INV
    finally:
        g_sig.free(); g_cnt.free(); ctx.free(d_ids); ctx.free(d_ro)
    check(tok, counters([9, 0, 4]), 8, 5, 0)                             # the context is usable afterwards


def test_refusals_of_the_group_calls(tok):
    from genz_tokenize import _native
    ctx, lib, P = tok._ctx, tok._ctx.lib, _native._ptr
    h, INV, vp = ctx.handle, _native.GZ_E_INVALID, ctypes.c_void_p
    sig = np.arange(3 * 8, dtype=np.uint32).reshape(3, 8)
    d_sig = ctx.alloc(sig.nbytes)
    g = Guarded(ctx, 3)
    said = set()

    def refused(call):
        group = np.full(3, FILL, dtype=np.int32); n = ctypes.c_int64(77)
        assert call(lib.gz_minhash_groups, P(sig), P(group), ctypes.byref(n)) == INV
        said.add(lib.gz_last_error(h))
        assert (group == FILL).all() and n.value == 77
        assert call(lib.gz_minhash_groups_device, vp(d_sig), vp(g.ptr), ctypes.byref(n)) == INV
        assert lib.gz_last_error(h) in said
        assert (g.read() == FILL).all() and n.value == 77
    try:
        ctx.h2d(d_sig, sig)
        refused(lambda f, s, gr, n: f(h, s, -1, 8, 2, 4, gr, n))
        refused(lambda f, s, gr, n: f(h, s, 2 ** 31 - 4096, 8, 2, 4, gr, n))
        for K in (0, 257):
            refused(lambda f, s, gr, n: f(h, s, 3, K, 1, 1, gr, n))
        for B in (0, -1):
            refused(lambda f, s, gr, n: f(h, s, 3, 8, B, 4, gr, n))
        for B in (3, 16):
            refused(lambda f, s, gr, n: f(h, s, 3, 8, B, 4, gr, n))
        for m in (0, 9, -1):
            refused(lambda f, s, gr, n: f(h, s, 3, 8, 2, m, gr, n))
        assert len(said) == 6                                             # each rule has its own sentence
        refused(lambda f, s, gr, n: f(h, None, 3, 8, 2, 4, gr, n))
        refused(lambda f, s, gr, n: f(h, s, 3, 8, 2, 4, None, n))
        refused(lambda f, s, gr, n: f(h, s, 3, 8, 2, 4, s, n))            # group over the signatures
        group = np.full(3, FILL, dtype=np.int32)
        assert lib.gz_minhash_groups(h, P(sig), 3, 8, 2, 4, P(group), None) == INV and (group == FILL).all()
        assert lib.gz_minhash_groups_device(h, vp(d_sig), 3, 8, 2, 4, vp(g.ptr), None) == INV and (g.read() == FILL).all()
        for f in (lib.gz_minhash_groups, lib.gz_minhash_groups_device):  # nothing to do is no error
            n = ctypes.c_int64(77)
            assert f(h, None, 0, 8, 2, 4, None, ctypes.byref(n)) == _native.GZ_OK and n.value == 0
        n = ctypes.c_int64(77)
        assert lib.gz_minhash_groups(None, P(sig), 3, 8, 2, 4, P(group), ctypes.byref(n)) == INV
    finally:
        g.free(); ctx.free(d_sig)
    assert both(tok, sig, bands=2, min_agree=4)["group"].tolist() == [0, 1, 2]          # the context is usable afterwards
