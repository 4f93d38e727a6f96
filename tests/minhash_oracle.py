"""The MinHash rule of include/genz_tokenize.h ("near-duplicate documents by MinHash signatures") in plain Python / numpy; nothing of
the product is imported.  Signatures are vectorised with numpy, groups are a plain union-find.  All arithmetic is unsigned and wraps
at 32 or 64 bits.

    fmix32(x)   x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
    H(t[0..m))  MurmurHash3_x86_32, seed 0, over the m ids as little-endian 32-bit words, closed with h ^= 4 m and fmix32
    c_k         fmix32(seed_lo ^ fmix32(seed_hi + 0x9E3779B9 * (k + 1)))
    g_k(x)      fmix32(x ^ c_k)
    sig[r][k]   min over the shingles s of the body of g_k(H(s)); 0xFFFFFFFF without shingles
    band key    z = 0x9E3779B97F4A7C15 * (j + 1); per slot v of the band: z = (z ^ v) * 0xFF51AFD7ED558CCD; z ^= z >> 32; key = z | 1
    rep_j(d)    the smallest non-empty row with d's key in band j
    edge        d -- rep_j(d) when they differ and agree in at least min_agree slots
    group[d]    the smallest row of d's connected component
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
EMPTY = 0xFFFFFFFF


def _u32(a):
    return np.asarray(a).astype(np.uint32)


def fmix32(x):
    x = _u32(x).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def murmur_runs(body, m):
    """H of every run body[i : i + m], i = 0 .. len(body) - m, as one uint32 array (m >= 0; m == 0: H([]) once)"""
    body = np.asarray(body, dtype=np.int64).astype(np.int32).view(np.uint32)
    n_runs = len(body) - m + 1
    h = np.zeros(n_runs, dtype=np.uint32)
    with np.errstate(over="ignore"):
        for i in range(m):
            k = body[i:i + n_runs] * np.uint32(0xCC9E2D51)
            k = _rotl(k, 15) * np.uint32(0x1B873593)
            h = _rotl(h ^ k, 13) * np.uint32(5) + np.uint32(0xE6546B64)
        h ^= np.uint32((4 * m) & M32)
        return fmix32(h)


def H(ids):
    return int(murmur_runs(list(ids), len(ids))[0])


def constants(num_perm, seed):
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    k = np.arange(1, num_perm + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        inner = fmix32(((np.uint64(seed_hi) + np.uint64(0x9E3779B9) * k) & np.uint64(M32)).astype(np.uint32))
        return fmix32(inner ^ np.uint32(seed_lo))


def shingle_hashes(body, shingle):
    n = len(body)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    return murmur_runs(body, shingle if n >= shingle else n)


def signature(body, num_perm=128, shingle=5, seed=0):
    """(sig uint32 [K], n_shingles)"""
    h = shingle_hashes(body, shingle)
    if len(h) == 0:
        return np.full(num_perm, EMPTY, dtype=np.uint32), 0
    c = constants(num_perm, seed)
    with np.errstate(over="ignore"):
        return fmix32(h[None, :] ^ c[:, None]).min(axis=1).astype(np.uint32), len(h)


def bodies_of(rows, framed):
    return [list(r)[1:-1] if framed else list(r) for r in rows]           # (a row shorter than its skips has an empty body)


def batch(rows, num_perm=128, shingle=5, seed=0, framed=False):
    """dict(signatures uint32 [N, K], n_shingles int32 [N]) of a batch of rows"""
    bodies = bodies_of(rows, framed)
    sig = np.full((len(bodies), num_perm), EMPTY, dtype=np.uint32)
    cnt = np.zeros(len(bodies), dtype=np.int32)
    for r, b in enumerate(bodies):
        sig[r], cnt[r] = signature(b, num_perm, shingle, seed)
    return dict(signatures=sig, n_shingles=cnt)


def band_keys(sig_row, bands):
    K = len(sig_row)
    rpb = K // bands
    keys = []
    for j in range(bands):
        z = (0x9E3779B97F4A7C15 * (j + 1)) & M64
        for v in sig_row[j * rpb:(j + 1) * rpb]:
            z = ((z ^ int(v)) * 0xFF51AFD7ED558CCD) & M64
            z ^= z >> 32
        keys.append(z | 1)
    return keys


def groups(sig, bands=16, min_agree=None, threshold=0.7):
    """dict(group int32 [N], keep bool [N], n_groups) of a [N, K] signature matrix"""
    sig = np.asarray(sig, dtype=np.uint32)
    N, K = sig.shape
    if min_agree is None:
        min_agree = max(1, int(np.ceil(threshold * K)))
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    empty = (sig == EMPTY).all(axis=1) if K else np.ones(N, dtype=bool)
    keys = [band_keys(sig[d], bands) if not empty[d] else None for d in range(N)]
    for j in range(bands):
        rep = {}
        for d in range(N):                                            # ascending: the first row with a key is the smallest
            if empty[d]:
                continue
            a = rep.setdefault(keys[d][j], d)
            if a != d and int((sig[d] == sig[a]).sum()) >= min_agree:
                ra, rd = find(a), find(d)
                if ra != rd:
                    parent[max(ra, rd)] = min(ra, rd)
    group = np.array([find(d) for d in range(N)], dtype=np.int32).reshape(N)
    return dict(group=group, keep=group == np.arange(N, dtype=np.int32), n_groups=int((group == np.arange(N)).sum()))


def jaccard(a, b, shingle=5):
    """the true Jaccard index of the shingle sets of two bodies (sets of id tuples, not of their hashes)"""
    def sh(x):
        x = list(x)
        if len(x) == 0:
            return set()
        if len(x) < shingle:
            return {tuple(x)}
        return {tuple(x[i:i + shingle]) for i in range(len(x) - shingle + 1)}
    A, B = sh(a), sh(b)
    return len(A & B) / len(A | B) if A or B else 1.0


def families(seed, n_bases=40, lo=5, hi=48423):
    """The planted families of the tests: n_bases bodies of 120 or 300 random ids, each with 0, 1 or 3 copies that differ in one
    substitution, two empty bodies, everything shuffled.  Returns (bodies, family) -- family[i] the index of body i's base, -1 - e
    for the e-th empty body."""
    rng = np.random.default_rng(1000 + seed)
    bodies, fam = [], []
    for b in range(n_bases):
        base = rng.integers(lo, hi, size=(120, 300)[b % 2]).tolist()
        bodies.append(base); fam.append(b)
        for _ in range((0, 1, 3)[b % 3]):
            c = list(base)
            at = int(rng.integers(0, len(c)))
            c[at] = int(c[at] - lo + 1 + rng.integers(0, hi - lo - 1)) % (hi - lo) + lo          # another id in [lo, hi)
            bodies.append(c); fam.append(b)
    bodies += [[], []]; fam += [-1, -2]
    order = rng.permutation(len(bodies))
    return [bodies[i] for i in order], [fam[i] for i in order]


def family_groups(fam):
    """the labels the planted families must get: the smallest row of each family"""
    first = {}
    for i, f in enumerate(fam):
        first.setdefault(f, i)
    return np.array([first[f] for f in fam], dtype=np.int32)
