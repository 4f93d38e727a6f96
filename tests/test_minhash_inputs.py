"""CPU-only: the MinHash rule of tests/minhash_oracle.py against known answers, against a second restatement written differently
(plain Python ints, MurmurHash3 over the ids' little-endian BYTES, slot by slot), against the truth it estimates (the Jaccard index
of the shingle sets) and on planted families of near-duplicates.  tests/test_gpu_minhash.py compares the GPU with this oracle."""
import math
import struct

import numpy as np
import pytest

import minhash_oracle as MO

M32 = 0xFFFFFFFF


# ---- the second restatement ----------------------------------------------------------------------------------------------
def _fmix(x):
    x ^= x >> 16; x = (x * 0x85EBCA6B) & M32; x ^= x >> 13; x = (x * 0xC2B2AE35) & M32; x ^= x >> 16
    return x


def murmur3_bytes(data, seed=0):
    """MurmurHash3_x86_32 of a byte string whose length is a multiple of 4 (no tail)"""
    h = seed
    for (k,) in struct.iter_unpack("<I", data):
        k = (k * 0xCC9E2D51) & M32
        k = ((k << 15) | (k >> 17)) & M32
        k = (k * 0x1B873593) & M32
        h ^= k
        h = ((h << 13) | (h >> 19)) & M32
        h = (h * 5 + 0xE6546B64) & M32
    return _fmix(h ^ len(data))


def slow_H(ids, seed=0):
    return murmur3_bytes(b"".join(struct.pack("<I", int(v) & M32) for v in ids), seed)


def slow_signature(body, K, w, seed):
    body = list(body)
    if not body:
        return [M32] * K, 0
    runs = [body[i:i + w] for i in range(len(body) - w + 1)] if len(body) >= w else [body]
    hashes = [slow_H(r) for r in runs]
    lo, hi = seed & M32, seed >> 32
    sig = []
    for k in range(K):
        c = _fmix(lo ^ _fmix((hi + 0x9E3779B9 * (k + 1)) & M32))
        sig.append(min(_fmix(h ^ c) for h in hashes))
    return sig, len(runs)


def slow_groups(sig, bands, min_agree):
    """the rule read literally: rep by a scan over all smaller rows, edges collected, components by repeated relabelling"""
    N, K = len(sig), len(sig[0]) if len(sig) else 0
    rpb = K // bands
    empty = [all(v == M32 for v in row) for row in sig]

    def key(d, j):
        z = (0x9E3779B97F4A7C15 * (j + 1)) & (2 ** 64 - 1)
        for v in sig[d][j * rpb:(j + 1) * rpb]:
            z = ((z ^ v) * 0xFF51AFD7ED558CCD) & (2 ** 64 - 1)
            z ^= z >> 32
        return z | 1
    edges = []
    for d in range(N):
        if empty[d]:
            continue
        for j in range(bands):
            rep = next((a for a in range(d) if not empty[a] and key(a, j) == key(d, j)), d)
            if rep != d and sum(x == y for x, y in zip(sig[d], sig[rep])) >= min_agree:
                edges.append((d, rep))
    label = list(range(N))
    changed = True
    while changed:
        changed = False
        for a, b in edges:
            m = min(label[a], label[b])
            if label[a] != m or label[b] != m:
                label[a] = label[b] = m
                changed = True
    return label


# ---- known answers ---------------------------------------------------------------------------------------------------------
def test_known_hashes():
    assert MO.H([]) == 0 and murmur3_bytes(b"", 1) == 0x514E28B7
    for ids, want in (([0xFFFFFFFF], 0x76293B50), ([0x87654321], 0xF55B516B), ([0], 0x2362F9DE), ([1, 2, 3, 4, 5], 0xC41CBA6A),
                      ([-1, 5, 48422], 0x14F297F6), ([3, 4], 0xE68B97C2)):
        assert MO.H(ids) == want, ids
        assert slow_H(ids) == want, ids
    assert MO.H([-1]) == MO.H([0xFFFFFFFF])                              # the bit pattern of the int32


def test_known_constants():
    assert MO.constants(4, 0).tolist() == [0xAA3E5B61, 0x99401FAC, 0x9D4F32B0, 0x471A8EFF]
    assert MO.constants(4, 0x123456789ABCDEF0).tolist() == [0xBFBC22DA, 0xD85D58B5, 0xFD1BFF20, 0xF9491C1F]
    assert MO.constants(256, 7)[:4].tolist() == MO.constants(4, 7).tolist()


FIRST = [0xFD7E773F, 0x13C489DB, 0xAD687A84, 0xA04A2BE6]
SECOND = [0x9AE1595C, 0x3D1EADA3, 0x1ECB5045, 0x0E33EB4E]
THIRD = [0x81D0D0A1, 0x96945386, 0x7040DED3, 0x98D44C23]


def test_known_signatures_keys_and_groups():
    assert MO.signature([7, 8, 9, 10, 11, 12], 4, 5, 0)[0].tolist() == FIRST
    assert MO.signature([7, 8, 9, 10, 11, 13], 4, 5, 0)[0].tolist() == SECOND
    assert MO.signature([3, 4], 4, 5, 0)[0].tolist() == THIRD
    assert MO.band_keys(np.array(FIRST, dtype=np.uint32), 2) == [0x5832A9387F05C015, 0xD6E1A92EDDB9E3BD]
    assert MO.band_keys(np.full(4, M32, dtype=np.uint32), 2) == [0x552319F92997C88D, 0x7031DED3AF847A43]
    sig = np.array([FIRST, SECOND, [M32] * 4, FIRST, THIRD], dtype=np.uint32)
    for m in (2, 4):
        r = MO.groups(sig, bands=2, min_agree=m)
        assert r["group"].tolist() == [0, 1, 2, 0, 4] and r["n_groups"] == 4 and r["keep"].tolist() == [True, True, True, False, True]
        assert slow_groups(sig.tolist(), 2, m) == [0, 1, 2, 0, 4]


# ---- the oracle against the second restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("K,w,seed", [(1, 1, 0), (4, 5, 0), (7, 2, 2 ** 32), (16, 32, 2 ** 64 - 1), (65, 3, 0x123456789ABCDEF0)])
def test_signatures_against_the_slot_by_slot_loop(K, w, seed):
    rng = np.random.default_rng(K * 100 + w)
    odd = [-1, 0, -2 ** 31, 2 ** 31 - 1, 5, 48422]
    bodies = [[]] + [rng.choice(odd, size=n).tolist() for n in (1, w - 1, w, w + 1, 40)] + [rng.integers(5, 48423, size=n).tolist() for n in (1, w, 70)]
    got = MO.batch(bodies, K, w, seed)
    for r, b in enumerate(bodies):
        sig, n = slow_signature(b, K, w, seed)
        assert got["signatures"][r].tolist() == sig and got["n_shingles"][r] == n, r
    assert got["signatures"].dtype == np.uint32 and got["n_shingles"].dtype == np.int32


@pytest.mark.parametrize("bands,min_agree", [(1, 1), (2, 3), (4, 8), (8, 1), (8, 5)])
def test_groups_against_the_literal_rule(bands, min_agree):
    """rows drawn from a few values a slot, so that buckets are shared, some pairs agree enough and some do not"""
    rng = np.random.default_rng(bands * 10 + min_agree)
    sig = rng.integers(0, 2, size=(60, 8)).astype(np.uint32)
    sig[rng.integers(0, 60, size=6)] = M32                                # empty rows among the rest
    sig[40:50] = sig[10:20]                                               # exact copies
    want = slow_groups(sig.tolist(), bands, min_agree)
    got = MO.groups(sig, bands=bands, min_agree=min_agree)
    assert got["group"].tolist() == want
    assert got["n_groups"] == sum(1 for d, g in enumerate(want) if d == g)


def test_the_smallest_bucket_mate_alone_is_asked():
    """b and c agree in 3 of 4 slots but share their only common band with a smaller row a that resembles neither: at min_agree = 3
    nothing joins them.  When they agree in the second band too, that band joins them."""
    sig = np.array([[1, 1, 5, 6], [1, 1, 7, 8], [1, 1, 7, 9]], dtype=np.uint32)
    assert MO.groups(sig, bands=2, min_agree=3)["group"].tolist() == [0, 1, 2]
    assert slow_groups(sig.tolist(), 2, 3) == [0, 1, 2]
    assert MO.groups(sig[1:], bands=2, min_agree=3)["group"].tolist() == [0, 0]              # without a, b is the one c is compared with
    sig[2, 3] = 8
    assert MO.groups(sig, bands=2, min_agree=4)["group"].tolist() == [0, 1, 1]
    assert slow_groups(sig.tolist(), 2, 4) == [0, 1, 1]


# ---- slicing, short bodies, framed -----------------------------------------------------------------------------------------
def test_slices_and_concatenation():
    rng = np.random.default_rng(11)
    bodies = [rng.integers(5, 48423, size=int(n)).tolist() for n in rng.integers(0, 90, size=40)]
    whole = MO.batch(bodies, 32, 5, 9)
    for a, b in ((0, 40), (0, 1), (7, 19), (39, 40), (5, 5)):
        part = MO.batch(bodies[a:b], 32, 5, 9)
        assert np.array_equal(part["signatures"], whole["signatures"][a:b]) and np.array_equal(part["n_shingles"], whole["n_shingles"][a:b])
    cat = np.concatenate([MO.batch(bodies[:13], 32, 5, 9)["signatures"], MO.batch(bodies[13:], 32, 5, 9)["signatures"]])
    assert np.array_equal(cat, whole["signatures"])
    g = MO.groups(whole["signatures"], bands=8, min_agree=16)
    assert g["group"].shape == (40,) and g["n_groups"] == int(g["keep"].sum())


def test_short_and_empty_bodies_and_framed():
    w, K = 5, 8
    r = MO.batch([[], [9], [9, 8, 7, 6], [9, 8, 7, 6, 5], [9, 8, 7, 6, 5, 4]], K, w, 0)
    assert r["n_shingles"].tolist() == [0, 1, 1, 1, 2]
    assert (r["signatures"][0] == M32).all() and not (r["signatures"][1:] == M32).all(axis=1).any()
    c = MO.constants(K, 0)
    assert r["signatures"][1].tolist() == MO.fmix32(np.uint32(MO.H([9])) ^ c).tolist()
    assert r["signatures"][2].tolist() == MO.fmix32(np.uint32(MO.H([9, 8, 7, 6])) ^ c).tolist()
    # a short body's one shingle is kept apart from the runs of w by its length: [9, 8, 7, 6] is no prefix match of [9, 8, 7, 6, 5]
    assert not np.array_equal(r["signatures"][2], r["signatures"][3])
    # framed: the first and last entry go, whatever they hold; rows shorter than their frame have an empty body
    framed = MO.batch([[1, 2], [1, 9, 2], [-5, 9, 8, 7, 6, 5, 4, -6], [], [3]], K, w, 0, framed=True)
    bare = MO.batch([[], [9], [9, 8, 7, 6, 5, 4], [], []], K, w, 0)
    assert np.array_equal(framed["signatures"], bare["signatures"]) and np.array_equal(framed["n_shingles"], bare["n_shingles"])


# ---- the estimate against the truth ---------------------------------------------------------------------------------------
def test_share_of_equal_slots_estimates_the_jaccard_index():
    """300 pairs from a fixed generator (seed 20): bodies of 40 / 100 / 400 random ids, the copy with 0, 1, 2, 5, 10 or 30
    substitutions, K = 128, w = 5, a different seed a pair.  Every pair with 0 < J < 1 lies within 4.0 binomial standard deviations
    sqrt(J (1 - J) / K) of J; J = 0 and J = 1 are met exactly.  Observed with this generator: 233 pairs with 0 < J < 1,
    largest deviation 3.29 standard deviations, mean -0.05, spread 0.95.  200 unrelated bodies of 60 ids agree in 0 of
    128 slots pairwise."""
    rng = np.random.default_rng(20)
    K, w = 128, 5
    devs = []
    for pair in range(300):
        n = (40, 100, 400)[pair % 3]
        subs = (0, 1, 2, 5, 10, 30)[(pair // 3) % 6]
        a = rng.integers(5, 48423, size=n).tolist()
        b = list(a)
        for at in rng.choice(n, size=subs, replace=False):
            b[at] = int(rng.integers(5, 48423))
        seed = int(rng.integers(0, 2 ** 63)) * 2 + pair % 2
        J = MO.jaccard(a, b, w)
        est = float((MO.signature(a, K, w, seed)[0] == MO.signature(b, K, w, seed)[0]).mean())
        if J == 0.0 or J == 1.0:
            assert est == J, (pair, J, est)
        else:
            devs.append((est - J) / math.sqrt(J * (1 - J) / K))
            assert abs(devs[-1]) <= 4.0, (pair, J, est, devs[-1])
    assert len(devs) >= 200
    print("pairs %d  largest %.2f  mean %.2f  spread %.2f" % (len(devs), max(abs(d) for d in devs), np.mean(devs), np.std(devs)))
    bodies = [rng.integers(5, 48423, size=60).tolist() for _ in range(200)]
    sig = MO.batch(bodies, K, w, 5)["signatures"]
    for i in range(200):
        assert int((sig[i + 1:] == sig[i]).sum()) == 0, i


# ---- planted families -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.5, 0.7])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_planted_families_are_recovered(seed, threshold):
    bodies, fam = MO.families(seed)
    assert sum(1 for b in bodies if not b) == 2 and len(set(fam)) == 42
    sig = MO.batch(bodies, 128, 5, seed)["signatures"]
    got = MO.groups(sig, bands=16, threshold=threshold)
    assert got["group"].tolist() == MO.family_groups(fam).tolist()
    for i, b in enumerate(bodies):
        if not b:
            assert got["group"][i] == i                                   # each empty body stays alone
    if seed == 0:                                                         # the copies really are near: one substitution of 120 or 300 ids
        want = MO.family_groups(fam)
        js = [MO.jaccard(bodies[want[i]], bodies[i]) for i in range(len(bodies)) if want[i] != i]
        assert len(js) == 13 * 1 + 13 * 3 and 0.84 <= min(js) < 1
