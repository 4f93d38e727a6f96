"""Duplicate substrings across the rows of a call and the cut of marked ids on the GPU (gz_substr_dups / _device, gz_cut_rows /
_device; Tokenize.substring_dup_rows, cut_rows, encode_substring_dups, dedup_substrings) against the rule in a dozen lines of
Python below -- a dict from n-gram to its first (row, i), then the definitions of include/genz_tokenize.h -- and, for planted
runs, against values known by hand.  Everything is an integer and compared exactly."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIECE = 4096                                                             # n-gram positions a wave takes (csrc/gz_pieces.inc: GZ_PIECE)
FILL = 0x5A5A5A5A
OUT = ("n_grams", "n_later", "n_dup", "first_dup", "first_src")


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


def reference(rows, n, framed):
    """The rule: per row the five numbers and body_len, `dup` over the rows back to back, `later` the positions per row."""
    skip, first = (1 if framed else 0), {}
    out = {k: [] for k in OUT + ("body_len",)}
    dup, later = [], []
    for r, row in enumerate(rows):
        row = np.asarray(row, dtype=np.int32)
        body = row[skip:len(row) - skip] if len(row) > 2 * skip else row[:0]
        d, lat = np.zeros(len(row), dtype=np.uint8), []
        for i in range(max(0, len(body) - n + 1)):
            if first.setdefault(body[i:i + n].tobytes(), (r, i)) != (r, i):
                lat.append(i)
                d[skip + i:skip + i + n] = 1
        src = first[body[lat[0]:lat[0] + n].tobytes()][0] if lat else -1
        for k, v in zip(OUT + ("body_len",), (max(0, len(body) - n + 1), len(lat), int(d.sum()), lat[0] if lat else -1, src, len(body))):
            out[k].append(v)
        dup.append(d)
        later.append(lat)
    out = {k: np.array(v, dtype=np.int32) for k, v in out.items()}
    out["dup"] = np.concatenate(dup) if dup else np.zeros(0, dtype=np.uint8)
    return out, later


def same(got, want):
    for k in OUT + ("body_len", "dup"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())


# ---- 1. planted runs: the expectation is known by hand -----------------------------------------------------------------------
PLANTED = {                                                              # name -> (K, s, k, pieces of the target) from n: the later positions are s .. s + k - 1
    "ends_one_before_the_trip_edge": lambda n: (n + 104, 58, 5, 1),
    "ends_at_the_trip_edge": lambda n: (n + 104, 59, 5, 1),
    "ends_one_after_the_trip_edge": lambda n: (n + 104, 60, 5, 1),
    "straddles_the_piece_edge_by_one": lambda n: (PIECE + 2 * n + 100, PIECE - 1, 2, 2),
    "straddles_the_piece_edge_widely": lambda n: (PIECE + 2 * n + 100, PIECE - (n - 1), n - 1 + 70, 2),
    "last_window_at_4095_carry_alone": lambda n: (2 * PIECE + n + 5, PIECE - 3, 3, 3),
    "ends_at_the_bodys_last_position": lambda n: (n + 200, 197, 4, 1),
}


@pytest.mark.parametrize("case", sorted(PLANTED))
@pytest.mark.parametrize("n", [1, 2, 32, 33, 50, 64, 65, 256])
def test_planted_run(tok, n, case):
    K, s, k, pieces = PLANTED[case](n)
    base, target = np.arange(K, dtype=np.int32), np.arange(K, 2 * K, dtype=np.int32)
    target[s:s + n + k - 1] = base[3:3 + n + k - 1]
    assert s + n + k - 1 <= K and len(set(target.tolist())) == K
    want, later = reference([base, target], n, False)
    G = K - n + 1
    assert (G + PIECE - 1) // PIECE == pieces
    assert later == [[], list(range(s, s + k))]                          # the reference agrees with the hand values ...
    hand = {"n_grams": [G, G], "n_later": [0, k], "n_dup": [0, n + k - 1], "first_dup": [-1, s], "first_src": [-1, 0]}
    got = tok.substring_dup_rows([base, target], n=n, framed=False, return_dup=True)
    for key, v in hand.items():
        assert want[key].tolist() == v and got[key].tolist() == v, key   # ... and so does the device
    same(got, want)
    assert got["dup"][K + s:K + s + n + k - 1].all() and got["dup"].sum() == n + k - 1


# ---- 2. mixed rows against the reference -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed(n, framed):
    """Bodies of the lengths at the rule's, the trips' and the pieces' edges: random runs over 0..8 between copies of n..3n ids out
    of earlier bodies and out of the same body; rows shorter than their skips and a periodic row among them.  With the reference."""
    rng = np.random.default_rng(1000 + n + framed)
    lengths = [0, n - 1, n, n + 1, n + 63, n + 64, 2 * n + 130, PIECE + n, 2 * PIECE + n + 5]
    bodies = []
    for T in (lengths[i] for i in (6, 0, 3, 8, 1, 4, 7, 2, 5)):
        b = []
        while len(b) < T:
            b += rng.integers(0, 9, size=int(rng.integers(1, n + 6))).tolist()
            pool = [x for x in bodies + [b] if len(x) >= n]
            if pool:
                src = pool[int(rng.integers(0, len(pool)))]
                k = int(rng.integers(n, min(len(src), 3 * n) + 1))
                at = int(rng.integers(0, len(src) - k + 1))
                b += src[at:at + k]
        bodies.append(b[:T])
    bodies.insert(5, [4] * (3 * n))                                       # periodic: every window but the first is later
    rows = [[1] + b + [2] for b in bodies] + [[], [7]] if framed else bodies
    want, later = reference(rows, n, framed)
    # not vacuous: later and first positions, dup and clean tokens (on the CPU: about 30 % later, 70 % dup)
    assert 0 < want["n_later"].sum() < want["n_grams"].sum() and 0 < want["n_dup"].sum() < want["body_len"].sum()
    assert want["n_later"][5] == 2 * n and want["n_dup"][5] == 3 * n - 1 and want["first_src"][5] == 5
    return rows, want


@pytest.mark.parametrize("n,framed", [(50, True), (50, False), (65, False), (256, True)])
def test_mixed_rows(tok, n, framed):
    rows, want = mixed(n, framed)
    same(tok.substring_dup_rows(rows, n=n, framed=framed, return_dup=True), want)
    got = tok.substring_dup_rows(rows, n=n, framed=framed)
    assert "dup" not in got and all(np.array_equal(got[k], want[k]) for k in OUT)


# ---- 3. exactness under collisions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 4, 0])
def test_forced_collisions_change_nothing(tok, bits):
    from genz_tokenize import _native
    rows, want = mixed(50, True)
    _native.debug_set("substr_hash_bits", bits, tok._ctx)
    try:
        same(tok.substring_dup_rows(rows, n=50, framed=True, return_dup=True), want)
    finally:
        _native.debug_set("substr_hash_bits", 0, tok._ctx)


# ---- 4. device forms ---------------------------------------------------------------------------------------------------------
class Guarded:
    """n cells on the device between two runs of guard cells, all pre-filled with the bytes of FILL."""

    def __init__(self, ctx, n, dtype=np.int32, guard=64):
        self.ctx, self.n, self.guard, self.dtype = ctx, n, guard, np.dtype(dtype)
        self.fill = np.frombuffer(np.array([FILL, FILL], dtype=np.uint32).tobytes(), dtype=dtype)[0]
        self.base = ctx.alloc(self.dtype.itemsize * (n + 2 * guard) + 16)
        ctx.h2d(self.base, np.full(n + 2 * guard, self.fill, dtype=dtype))
        self.ptr = self.base + self.dtype.itemsize * guard

    def read(self):
        a = np.empty(self.n + 2 * self.guard, dtype=self.dtype)
        self.ctx.d2h(a, self.base)
        assert (a[:self.guard] == self.fill).all() and (a[self.guard + self.n:] == self.fill).all(), "guard cells were written"
        return a[self.guard:self.guard + self.n]


def test_device_forms_behind_junk(tok):
    """The rows lie behind a prefix of junk (row_off_dev[0] != 0) and before a tail of it; outputs left out stay out; nothing outside
    the outputs is written; dup and drop are laid out like the ids; the cut's output starts at its first cell."""
    ctx, n, junk = tok._ctx, 50, 37
    rows, want = mixed(n, True)
    N = len(rows)
    flat = np.array([-77] * junk + [v for r in rows for v in r] + [-88] * 5, dtype=np.int32)
    ro = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=ro[1:])
    ro += junk
    end = int(ro[-1])
    d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
    g = [Guarded(ctx, N) for _ in OUT]
    g_dup, g_one = Guarded(ctx, len(flat), np.uint8), Guarded(ctx, N)
    g_ids, g_off, g_kept = Guarded(ctx, end - junk), Guarded(ctx, N + 1, np.int64), Guarded(ctx, N)
    try:
        ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
        ctx.substr_dups_device(d_ids, d_ro, N, 1, 1, n, *[x.ptr for x in g], g_dup.ptr)
        for k, x in zip(OUT, g):
            assert np.array_equal(x.read(), want[k]), k
        dup = g_dup.read()
        assert (dup[:junk] == g_dup.fill).all() and (dup[end:] == g_dup.fill).all()       # the junk's cells are nobody's
        assert np.array_equal(dup[junk:end], want["dup"])
        for i, k in enumerate(OUT):                                      # one output at a time; first_src alone takes first_dup from the workspace
            ctx.substr_dups_device(d_ids, d_ro, N, 1, 1, n, *[g_one.ptr if j == i else 0 for j in range(5)], 0)
            assert np.array_equal(g_one.read(), want[k]), k
        ctx.cut_rows_device(d_ids, d_ro, N, g_dup.ptr, g_ids.ptr, g_off.ptr, g_kept.ptr)
        keep = want["dup"] == 0
        off, kept = g_off.read(), g_kept.read()
        assert off[0] == 0 and np.array_equal(np.diff(off), kept) and kept.tolist() == [int(keep[a - junk:b - junk].sum()) for a, b in zip(ro, ro[1:])]
        ids = g_ids.read()
        assert np.array_equal(ids[:off[-1]], flat[junk:end][keep]) and (ids[off[-1]:] == g_ids.fill).all()
    finally:
        for x in g + [g_dup, g_one, g_ids, g_off, g_kept]:
            ctx.free(x.base)
        ctx.free(d_ids); ctx.free(d_ro)


# ---- 5. the cut --------------------------------------------------------------------------------------------------------------
CUT_LENGTHS = [0, 1, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 3]


def check_cut(tok, rows, drop):
    got = tok.cut_rows(rows, drop)
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    kept = [np.asarray(r, dtype=np.int32)[np.asarray(drop[a:b]) == 0] for r, a, b in zip(rows, off, off[1:])]
    assert got["ids"].dtype == np.int32 and got["row_off"].dtype == np.int64 and got["n_kept"].dtype == np.int32
    assert got["row_off"][0] == 0 and got["n_kept"].tolist() == [len(x) for x in kept] and np.array_equal(np.diff(got["row_off"]), got["n_kept"])
    assert np.array_equal(got["ids"], np.concatenate(kept) if kept else np.zeros(0, np.int32))


@pytest.mark.parametrize("density", [0.0, 0.5, 1.0])
def test_cut_random_masks(tok, density):
    rng = np.random.default_rng(7)
    rows = [rng.integers(0, 60000, size=T).astype(np.int32) for T in CUT_LENGTHS[4:] + CUT_LENGTHS[:4]]
    check_cut(tok, rows, (rng.random(sum(CUT_LENGTHS)) < density).astype(np.uint8))
    for T in (0, 1, PIECE, PIECE + 1):                                    # ... and as batches of their own
        check_cut(tok, [rows[(CUT_LENGTHS[4:] + CUT_LENGTHS[:4]).index(T)]], (rng.random(T) < density).astype(np.uint8))


def test_cut_of_the_dup_bytes(tok):
    rows, want = mixed(50, True)
    check_cut(tok, rows, want["dup"])
    check_cut(tok, [], np.zeros(0, dtype=np.uint8))


def test_dedup_substrings_of_texts(tok):
    """encode -> dups -> cut on the device equals encode -> reference -> numpy cut, and the cleaned rows decode"""
    rng = np.random.default_rng(3)
    words = "anh em nha cua hoc sinh truong lop thay co ban be di ve an uong ngu nghi lam viec choi".split()
    sentences = [" ".join(rng.choice(words, size=int(rng.integers(6, 15)))) + " ." for _ in range(12)]
    texts = [" ".join(sentences[int(j)] for j in rng.integers(0, 12, size=int(rng.integers(1, 6)))) for _ in range(40)] + ["", "anh"]
    n = 8
    e = tok.encode_batch(texts, max_len=None)
    rows = [np.asarray(e["input_ids"][a:b], dtype=np.int32) for a, b in zip(e["row_off"], e["row_off"][1:])]
    want, _ = reference(rows, n, True)
    assert 0 < want["n_dup"].sum() < want["body_len"].sum()
    got = tok.encode_substring_dups(texts, n=n)
    assert sorted(got) == sorted(OUT + ("body_len",)) and all(np.array_equal(got[k], want[k]) for k in OUT + ("body_len",))
    out = tok.dedup_substrings(texts, n=n, max_fraction=0.5)
    assert all(np.array_equal(out[k], want[k]) for k in OUT + ("body_len",))
    assert np.array_equal(out["fraction"], want["n_dup"] / np.maximum(want["body_len"], 1.0))
    assert np.array_equal(out["keep"], want["n_dup"] <= 0.5 * want["body_len"]) and tok.dedup_substrings(texts, n=n)["keep"].all()
    flat = np.concatenate(rows)
    assert np.array_equal(out["ids"], flat[want["dup"] == 0])
    assert np.array_equal(np.diff(out["row_off"]), [len(r) for r in rows] - want["n_dup"]) and out["row_off"][0] == 0
    cleaned = [out["ids"][a:b] for a, b in zip(out["row_off"], out["row_off"][1:])]
    assert all(len(r) >= 2 and r[0] == rows[i][0] and r[-1] == rows[i][-1] for i, r in enumerate(cleaned))     # the frames are kept
    assert len(tok.decode_batch(cleaned)) == len(texts)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
BIG = 2 ** 32 - 1
REFUSALS = {                                                             # name -> (status, words, changes to the argument list)
    "negative_rows": ("INVALID", b"n_rows >= 0", dict(n_rows=-1)),
    "n_0": ("INVALID", b"1..256", dict(n=0)),
    "n_257": ("INVALID", b"1..256", dict(n=257)),
    "skip_front_2": ("INVALID", b"skips of 0 or 1", dict(sf=2)),
    "skip_back_negative": ("INVALID", b"skips of 0 or 1", dict(sb=-1)),
    "null_ids": ("INVALID", b"need ids and row_off", dict(ids=None)),
    "null_row_off": ("INVALID", b"need ids and row_off", dict(ro=None)),
    "two_outputs_in_one_array": ("INVALID", b"overlap neither", dict(alias=(1, 0))),
    "an_output_over_the_ids": ("INVALID", b"overlap neither", dict(alias=(2, "ids"))),
    "decreasing_offsets": ("INVALID", b"must not decrease", dict(off=[0, 7, 4], host_only=True)),
    "bad_offsets": ("INVALID", b"bad row offsets", dict(off=[5, 6, 2])),
    "too_many_ids": ("LIMIT", b"2^32 - 1 ids", dict(off=[0, 4, BIG])),
    "body_too_long": ("LIMIT", b"2^31 ids or more", dict(off=[0, 4, 4 + 2 ** 31], host_only=True)),   # (on the device 8 GiB of "ids" reach over the outputs)
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(tok, name):
    from genz_tokenize import _native
    status, words, ch = REFUSALS[name]
    code = {"INVALID": _native.GZ_E_INVALID, "LIMIT": _native.GZ_E_LIMIT}[status]
    ctx, lib, P, vp = tok._ctx, tok._ctx.lib, _native._ptr, ctypes.c_void_p
    ids = np.arange(10, dtype=np.int32)
    ro = np.array(ch.get("off", [0, 4, 10]), dtype=np.int64)
    n_rows, sf, sb, n = ch.get("n_rows", 2), ch.get("sf", 0), ch.get("sb", 0), ch.get("n", 3)
    d_ids, d_ro = ctx.alloc(64), ctx.alloc(64)
    g = [Guarded(ctx, 2) for _ in OUT] + [Guarded(ctx, 10, np.uint8)]
    try:
        ctx.h2d(d_ids, ids); ctx.h2d(d_ro, ro)
        out = [np.full(2, FILL, dtype=np.int32) for _ in OUT] + [np.full(10, 0x5A, dtype=np.uint8)]
        for device in (False, True):
            if device and ch.get("host_only"):
                continue
            a = [vp(x.ptr) for x in g] if device else [P(x) for x in out]
            i, o = (vp(d_ids), vp(d_ro)) if device else (P(ids), P(ro))
            if "alias" in ch:
                a[ch["alias"][0]] = i if ch["alias"][1] == "ids" else a[ch["alias"][1]]
            i, o = (None if "ids" in ch else i), (None if "ro" in ch else o)
            f = lib.gz_substr_dups_device if device else lib.gz_substr_dups
            assert f(ctx.handle, i, o, n_rows, sf, sb, n, *a) == code
            assert words in lib.gz_last_error(ctx.handle), lib.gz_last_error(ctx.handle)
            assert all((x.read() == x.fill).all() for x in g) and all((x == FILL).all() for x in out[:5]) and (out[5] == 0x5A).all()
        # nothing to do is no error; the context is usable afterwards
        assert lib.gz_substr_dups(ctx.handle, None, None, 0, 0, 0, 50, None, None, None, None, None, None) == _native.GZ_OK
        assert lib.gz_cut_rows_device(ctx.handle, None, None, 0, None, None, None, None) == _native.GZ_OK
        assert tok.substring_dup_rows([[1, 2, 3, 1, 2, 3]], n=3, framed=False)["n_later"].tolist() == [1]
    finally:
        for x in g:
            ctx.free(x.base)
        ctx.free(d_ids); ctx.free(d_ro)
