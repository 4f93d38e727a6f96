// gz_minhash.inc -- MinHash signatures of ragged token rows and near-duplicate groups from signatures (included by gz_kernels.hip
// behind gz_pieces.inc).
//
// The rule (include/genz_tokenize.h, "near-duplicate documents by MinHash signatures"): the body of a row is the row without its skips;
// its shingles are the runs of w ids (one run, the whole body, when it is shorter), each hashed with H = MurmurHash3_x86_32 over the
// ids; sig[r][k] = min over the shingles of g_k(H) with g_k(x) = fmix32(x ^ c_k).  A band's key is a 64-bit mix of its slots;
// rep_j(d) is the smallest non-empty row with d's key in band j; d and rep_j(d) are joined when they agree in min_agree slots;
// group[d] is the smallest row of d's component.
//
// SIGNATURES.  Work is divided over PIECES of GZ_PIECE = 4096 shingle positions, never over documents (gz_pieces.inc: the body rule,
// the count pass and the walk from a wave's piece to its row are the ones the n-gram kernels use).  A trip is 64 shingle
// positions: lane l loads id t + l (and id t + 64 + l for the w - 1 ids beyond the trip) -- one coalesced load each, not w loads a
// lane --, takes the ids of its own run from its neighbours by wave shuffles and computes ONE H.  The lanes then own the k: lane l
// keeps slots l, l + 64, ... (at most 4 with K <= 256) in registers and folds each of the trip's hashes, read out of the owning lane
// as a wave-uniform value (v_readlane: no LDS, nothing to synchronise), into them with g_k and min.  The store is a coalesced row of K
// words and there is no cross-lane reduction.  A row of one piece is stored plainly; the pieces of a longer row combine with the
// 32-bit atomicMin on global memory into a row the launcher filled with 0xFFFFFFFF: min does not depend on order, so the result is exact.
// Work per (shingle, k): one xor, fmix32 (three shift-xor pairs, two 32-bit multiplies) and one min -- ten VALU instructions of which
// the two v_mul_lo_u32 dominate; per shingle 2 w multiplies for H.  Body positions are 64-bit (rows lie anywhere in a batch of any
// size); a body itself is shorter than 2^31 ids (the count pass raises a flag otherwise and nothing is written).
//
// GROUPS.  One band at a time through ONE open-addressing table of `cap` slots (a power of two, at least twice the rows): 64-bit keys
// claimed by atomicCAS (0 = free: a key has its lowest bit set), 32-bit row indices lowered by atomicMin, which fixes rep whatever the
// order.  Per band: clear the table; insert (a thread a row); link (a lane a row looks its key up; the rows whose rep is another row
// are then taken one by one by the whole wave, which compares the two K-word rows 64 slots at a time and counts the equal ones).  A pair
// that agrees is joined in the label array itself, a forest whose pointers only ever go to smaller rows: find both roots, hang the
// larger under the smaller by atomicCAS on the larger root's own cell, start over when another thread got there first.  Every failed
// CAS is some other thread's successful one and a success lowers the number of roots, so the loop ends; a root is the smallest row
// of its tree.  One last pass replaces every label by its root (pointer jumping to the end: nothing hooks any more) and counts the
// roots.  The labels are the components' minima, so they do not depend on scheduling.
// Workspace: 12 * cap bytes of table (24 to 48 bytes a document), one byte a document (EMPTY) and the 8-byte counter.

__device__ __forceinline__ uint32_t mh_fmix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t mh_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// NK slots a lane: K <= 64 * NK
template <int NK>
__global__ __launch_bounds__(WAVE * 4) void gz_minhash_sig_kernel(GzMinhashArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t j, n_pc, n;
    const int64_t r = piece_row(A, p, &j, &n_pc);
    const int64_t a = piece_body(A.row_off, r, A.skip_front, A.skip_back, &n);
    const int64_t n_sh = piece_shingles(n, A.shingle);
    const int m = n >= A.shingle ? A.shingle : (int)n;                               // ids of a shingle of this body
    const bool alone = n_pc == 1;
    const int64_t s0 = j * GZ_PIECE, s1 = s0 + GZ_PIECE < n_sh ? s0 + GZ_PIECE : n_sh;
    if (j == 0 && lane == 0 && A.n_shingles) A.n_shingles[r] = (int32_t)n_sh;
    uint32_t c[NK], mn[NK];
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        const uint32_t k1 = (uint32_t)(lane + WAVE * i) + 1u;
        c[i] = mh_fmix32(A.seed_lo ^ mh_fmix32(A.seed_hi + 0x9E3779B9u * k1));
        mn[i] = 0xFFFFFFFFu;
    }
    const int32_t* const body = A.ids + a;                                           // (never read when n == 0)
    for (int64_t t = s0; t < s1; t += WAVE) {                                        // (wave-uniform bounds: every lane stays for the shuffles)
        const int cnt = s1 - t < WAVE ? (int)(s1 - t) : WAVE;
        const int64_t q0 = t + lane, q1 = t + WAVE + lane;
        const uint32_t id0 = q0 < n ? (uint32_t)body[q0] : 0u;
        const uint32_t id1 = (lane < m - 1 && q1 < n) ? (uint32_t)body[q1] : 0u;
        uint32_t h = 0u;
        for (int i = 0; i < m; ++i) {
            const int src = lane + i;
            const uint32_t x = (uint32_t)__shfl((int)id0, src & (WAVE - 1), WAVE), y = (uint32_t)__shfl((int)id1, src & (WAVE - 1), WAVE);
            uint32_t k = (src < WAVE ? x : y) * 0xCC9E2D51u;
            k = mh_rotl(k, 15) * 0x1B873593u;
            h = mh_rotl(h ^ k, 13) * 5u + 0xE6546B64u;
        }
        h = mh_fmix32(h ^ (uint32_t)(4 * m));
        for (int s = 0; s < cnt; ++s) {                                              // lanes at or beyond cnt hold no shingle: never read
            const uint32_t hs = (uint32_t)__builtin_amdgcn_readlane((int)h, s);
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const uint32_t g = mh_fmix32(hs ^ c[i]);
                mn[i] = g < mn[i] ? g : mn[i];
            }
        }
    }
    uint32_t* const row = A.sig + r * (int64_t)A.num_perm;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        const int k = lane + WAVE * i;
        if (k < A.num_perm) {
            if (alone) row[k] = mn[i];
            else if (mn[i] != 0xFFFFFFFFu) atomicMin(row + k, mn[i]);
        }
    }
}

// ---- groups ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mh_band_key(const uint32_t* __restrict__ row, int j, int rpb)
{
    uint64_t z = 0x9E3779B97F4A7C15ull * (uint64_t)(j + 1);
    for (int i = 0; i < rpb; ++i) {
        z = (z ^ (uint64_t)row[j * rpb + i]) * 0xFF51AFD7ED558CCDull;
        z ^= z >> 32;
    }
    return z | 1ull;
}
__device__ __forceinline__ uint64_t mh_slot(uint64_t key, uint64_t mask) { return (key >> 17) & mask; }

// label[d] = d, empty[d] = every slot of the row is 0xFFFFFFFF; the counter is cleared
__global__ __launch_bounds__(256) void gz_minhash_init_kernel(GzMinhashGroupArgs A)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d == 0) *A.n_groups = 0ull;
    if (d >= A.n_rows) return;
    const uint32_t* const row = A.sig + d * (int64_t)A.num_perm;
    int k = 0;
    while (k < A.num_perm && row[k] == 0xFFFFFFFFu) ++k;
    A.empty[d] = k == A.num_perm ? 1 : 0;
    A.group[d] = (int32_t)d;
}

__global__ __launch_bounds__(256) void gz_minhash_insert_kernel(GzMinhashGroupArgs A, int band)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= A.n_rows || A.empty[d]) return;
    const uint64_t key = mh_band_key(A.sig + d * (int64_t)A.num_perm, band, A.num_perm / A.bands), mask = A.cap - 1;
    for (uint64_t s = mh_slot(key, mask);; s = (s + 1) & mask) {                      // (ends: the table holds at most n_rows <= cap / 2 keys)
        const unsigned long long seen = atomicCAS(A.keys + s, 0ull, (unsigned long long)key);
        if (seen == 0ull || seen == key) { atomicMin(A.reps + s, (uint32_t)d); return; }
    }
}

__device__ __forceinline__ int32_t mh_label(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t mh_root(const int32_t* group, int32_t x)
{
    for (int32_t up = mh_label(group + x); up != x; up = mh_label(group + x)) x = up;      // (pointers go to smaller rows: no cycle)
    return x;
}
__device__ __forceinline__ void mh_join(int32_t* group, int32_t a, int32_t b)
{
    for (;;) {
        a = mh_root(group, a); b = mh_root(group, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        if (atomicCAS(group + a, a, b) == a) return;                                 // (a was still a root; otherwise somebody hooked it: again)
    }
}

__global__ __launch_bounds__(WAVE * 4) void gz_minhash_link_kernel(GzMinhashGroupArgs A, int band)
{
    const int lane = lane_id();
    const int64_t d = (int64_t)blockIdx.x * (WAVE * 4) + threadIdx.x;
    const int K = A.num_perm;
    int64_t rep = d;
    if (d < A.n_rows && !A.empty[d]) {
        const uint64_t key = mh_band_key(A.sig + d * (int64_t)K, band, K / A.bands), mask = A.cap - 1;
        for (uint64_t s = mh_slot(key, mask);; s = (s + 1) & mask) {
            const unsigned long long seen = A.keys[s];
            if (seen == key) { rep = (int64_t)A.reps[s]; break; }
            if (seen == 0ull) break;                                                 // (cannot happen: the insert pass put the key there)
        }
    }
    bool join = false;
    for (uint64_t todo = wballot(rep != d); todo; todo &= todo - 1) {                // (wave-uniform: every lane stays for the shuffles)
        const int s = __builtin_ctzll(todo);
        const int64_t d_s = __shfl(d, s, WAVE), rep_s = __shfl(rep, s, WAVE);
        const uint32_t* const x = A.sig + d_s * (int64_t)K;
        const uint32_t* const y = A.sig + rep_s * (int64_t)K;
        int eq = 0;
        for (int k = lane; k < K; k += WAVE) eq += x[k] == y[k] ? 1 : 0;
        eq = wave_sum(eq);
        if (lane == s) join = eq >= A.min_agree;
    }
    if (join) mh_join(A.group, (int32_t)d, (int32_t)rep);
}

__global__ __launch_bounds__(256) void gz_minhash_flatten_kernel(GzMinhashGroupArgs A)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_root = false;
    if (d < A.n_rows) {
        const int32_t root = mh_root(A.group, (int32_t)d);
        is_root = root == (int32_t)d;
        if (!is_root) __hip_atomic_store(A.group + d, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t roots = wballot(is_root);
    if (lane_id() == 0 && roots) atomicAdd(A.n_groups, (unsigned long long)__builtin_popcountll(roots));
}
