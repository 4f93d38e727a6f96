// gz_learn.inc -- the word counts of a corpus and the merge loop of a BPE learner, included by gz_kernels.hip behind gz_bm25.inc
// (whose split, hash, de-duplication and numbering kernels make the distinct words; bm_mix64 is its mixer).
//
//   gz_wordset_count_kernel    behind GZ_BM25_FIRST and the scan of its flags: one int64 atomicAdd per word onto its term id (16 counters
//                              a term, summed by gz_wordset_sum_kernel); the representatives describe their term (tstart, tlen)
//   gz_wordset_gather_kernel   the distinct words' bytes into one arena, in term order
//   gz_learn_pairs_kernel      n(l, r) of the initial symbols into the pair table: + c_w for every adjacent position
//   gz_learn_best_a/_b_kernel  arg-best over the table: largest count, then smallest key; counts <= 0 never win
//   gz_learn_apply_kernel      a lane per word of at most GZ_LEARN_LANE_MAX initial symbols: a word that holds (l, r) takes all of its
//                              adjacent pairs off the table (- c_w each), rewrites its symbols in place -- every l r, left to right
//                              and non-overlapping, becomes m -- and puts all of its new pairs on (+ c_w).  Other words are left alone.
//   gz_learn_apply_long_kernel the same for the longer words, a wave each: 64 positions a step, the matches by ballot (a self-
//                              overlapping pair l == r takes every other match of a run, the parity carried across the tiles), the
//                              kept positions compacted by popcount
//   gz_learn_hist_kernel       after the last step: hist[2 * symbol + (last position of its word)] += c_w
//   gz_learn_rehash_kernel     the table into a larger one
//
// Vector stores and vector atomics only.  Every count is an integer sum: the table's contents as a set of (key, count) do not
// depend on the order in which the atomics land, and the arg-best is a function of that set.  Which slot a key sits in varies
// from run to run; no answer reads it.  A probe visits at most every slot once: a full table raises ctl[3] and the host refuses
// the result, no lane ever waits for another.

namespace {

__device__ __forceinline__ unsigned long long ln_key(int32_t a, int32_t b)
{
    return (((unsigned long long)(uint32_t)a << 32) | (unsigned long long)(uint32_t)b) + 1ull;
}

// count of (a, b) += v; the key is claimed by CAS where it is new
__device__ __forceinline__ void ln_add(const GzLearn& L, int32_t a, int32_t b, long long v)
{
    const unsigned long long key = ln_key(a, b);
    unsigned long long s = bm_mix64(key) & L.mask;
    for (unsigned long long n = 0; n <= L.mask; ++n) {
        unsigned long long old = __hip_atomic_load(&L.tab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0ull) {
            old = atomicCAS(&L.tab[s].key, 0ull, key);
            if (old == 0ull) atomicAdd(&L.ctl[2], 1ull);
        }
        if (old == 0ull || old == key) {
            atomicAdd((unsigned long long*)&L.tab[s].cnt, (unsigned long long)v);
            return;
        }
        s = (s + 1) & L.mask;
    }
    atomicOr(&L.ctl[3], 1ull);
}

// (count, key) a beats b: larger count, then smaller key; "nothing" is (0, ~0)
__device__ __forceinline__ bool ln_better(long long ca, unsigned long long ka, long long cb, unsigned long long kb)
{
    return ca > cb || (ca == cb && ka < kb);
}

// the best of a workgroup of 256 in thread 0
__device__ __forceinline__ void ln_block_best(long long& c, unsigned long long& k, long long* sc, unsigned long long* sk)
{
    for (int o = 32; o >= 1; o >>= 1) {
        const long long c2 = __shfl_xor(c, o, WAVE);
        const unsigned long long k2 = __shfl_xor(k, o, WAVE);
        if (ln_better(c2, k2, c, k)) { c = c2; k = k2; }
    }
    const int wv = (int)(threadIdx.x / WAVE);
    if (lane_id() == 0) { sc[wv] = c; sk[wv] = k; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < 4; ++i)
            if (ln_better(sc[i], sk[i], c, k)) { c = sc[i]; k = sk[i]; }
}

}  // namespace

// (GZ_BM25_DF_SHARDS counters per term, picked by the word's index: a frequent word is millions of adds, and they would all queue
// on one address; gz_wordset_sum_kernel adds the shards up.  Sums of integers: the order does not matter.)
__global__ __launch_bounds__(256) void gz_wordset_count_kernel(GzBm25Args A, const long long* weight, long long* cnt, int64_t n_terms, int strict)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    const uint32_t r = A.rep[w], t = A.scan[r], d = A.wdoc[w];
    atomicAdd((unsigned long long*)&cnt[(w & (GZ_BM25_DF_SHARDS - 1)) * n_terms + t], (unsigned long long)(weight ? weight[d] : 1ll));
    if (strict && (A.wstart[w] != A.off[d] + A.obase || A.wend[w] != A.off[d + 1] + A.obase)) atomicOr(&A.ctl[1], 2u);
    if (r != (uint32_t)w) return;
    A.tstart[t] = A.wstart[w];
    A.tlen[t] = (uint32_t)(A.wend[w] - A.wstart[w]);
}

__global__ __launch_bounds__(256) void gz_wordset_sum_kernel(long long* cnt, int64_t n_terms)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_terms) return;
    long long n = 0;
    for (int k = 0; k < GZ_BM25_DF_SHARDS; ++k) n += cnt[k * n_terms + t];
    cnt[t] = n;
}

// a lane per word; a word of more than 16 bytes is then copied by the whole wave, 64 bytes a step (gz_bm25_cp_gather_kernel's way)
__global__ __launch_bounds__(256) void gz_wordset_gather_kernel(const uint8_t* tb, const int64_t* tstart, const uint32_t* tlen, const uint32_t* toff,
                                                                uint8_t* arena, int64_t n)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    int64_t src = 0;
    uint32_t len = 0, dst = 0;
    if (t < n) { src = tstart[t]; len = tlen[t]; dst = toff[t]; }
    if (len <= 16u)
        for (uint32_t i = 0; i < len; ++i) arena[(int64_t)dst + i] = tb[src + i];
    uint64_t m = wballot(len > 16u);
    while (m) {                                               // (uniform)
        const int k = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int64_t s = __shfl(src, k, WAVE), d = (int64_t)(uint32_t)__shfl((int)dst, k, WAVE);
        const uint32_t l = (uint32_t)__shfl((int)len, k, WAVE);
        for (uint32_t i = (uint32_t)lane; i < l; i += WAVE) arena[d + i] = tb[s + i];
    }
}

__global__ __launch_bounds__(256) void gz_learn_pairs_kernel(GzLearn L)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= L.n_words) return;
    const int32_t* p = L.sym + L.woff[d];
    const uint32_t n = L.wlen[d];
    const long long c = L.cw[d];
    for (uint32_t i = 0; i + 1 < n; ++i) ln_add(L, p[i], p[i + 1], c);
}

__global__ __launch_bounds__(256) void gz_learn_best_a_kernel(GzLearn L)
{
    __shared__ long long sc[4];
    __shared__ unsigned long long sk[4];
    long long c = 0;
    unsigned long long k = ~0ull;
    const unsigned long long slots = L.mask + 1;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < slots; i += (unsigned long long)gridDim.x * 256) {
        const GzLearnSlot o = L.tab[i];
        if (o.key != 0ull && o.cnt > 0 && ln_better(o.cnt, o.key, c, k)) { c = o.cnt; k = o.key; }
    }
    ln_block_best(c, k, sc, sk);
    if (threadIdx.x == 0) { L.part[2 * blockIdx.x] = k; L.part[2 * blockIdx.x + 1] = (unsigned long long)c; }
}

__global__ __launch_bounds__(256) void gz_learn_best_b_kernel(GzLearn L)
{
    __shared__ long long sc[4];
    __shared__ unsigned long long sk[4];
    long long c = 0;
    unsigned long long k = ~0ull;
    for (int i = (int)threadIdx.x; i < L.n_part; i += 256) {
        const unsigned long long k2 = L.part[2 * i];
        const long long c2 = (long long)L.part[2 * i + 1];
        if (ln_better(c2, k2, c, k)) { c = c2; k = k2; }
    }
    ln_block_best(c, k, sc, sk);
    if (threadIdx.x == 0) { L.ctl[0] = k; L.ctl[1] = (unsigned long long)c; }
}

__global__ __launch_bounds__(256) void gz_learn_apply_kernel(GzLearn L)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= L.n_words) return;
    const uint32_t o = L.woff[d];
    if (L.woff[d + 1] - o > (uint32_t)GZ_LEARN_LANE_MAX) return;          // (a wave's: gz_learn_apply_long_kernel)
    const uint32_t n = L.wlen[d];
    int32_t* p = L.sym + o;
    bool found = false;
    for (uint32_t i = 0; i + 1 < n; ++i)
        if (p[i] == L.l && p[i + 1] == L.r) { found = true; break; }
    if (!found) return;
    const long long c = L.cw[d];
    for (uint32_t i = 0; i + 1 < n; ++i) ln_add(L, p[i], p[i + 1], -c);
    uint32_t j = 0;
    for (uint32_t i = 0; i < n;) {
        if (i + 1 < n && p[i] == L.l && p[i + 1] == L.r) { p[j++] = L.m; i += 2; }
        else { p[j++] = p[i]; i += 1; }
    }
    L.wlen[d] = j;
    for (uint32_t i = 0; i + 1 < j; ++i) ln_add(L, p[i], p[i + 1], c);
}

__global__ __launch_bounds__(256) void gz_learn_apply_long_kernel(GzLearn L)
{
    const int64_t wv = (int64_t)blockIdx.x * 4 + (int64_t)(threadIdx.x / WAVE);
    if (wv >= L.n_long) return;
    const uint32_t d = L.longw[wv];
    const uint32_t n = L.wlen[d];
    int32_t* p = L.sym + L.woff[d];
    const int lane = lane_id();
    bool any = false;
    for (uint32_t t = 0; t + 1 < n && !any; t += WAVE) {                   // (uniform)
        const uint32_t i = t + (uint32_t)lane;
        any = wballot(i + 1 < n && p[i] == L.l && p[i + 1] == L.r) != 0ull;
    }
    if (!any) return;
    const long long c = L.cw[d];
    for (uint32_t i = (uint32_t)lane; i + 1 < n; i += WAVE) ln_add(L, p[i], p[i + 1], -c);
    // The rewrite, a tile of 64 positions at a time.  A kept position's new index is at most its old one and lies before the tile's
    // end, so a tile's stores never reach what a later tile still has to read; inside a tile every lane has loaded before any stores.
    uint32_t out = 0;
    uint64_t carry = 0;                                                   // the tile before ended in a match: this tile's position 0 is its right half
    for (uint32_t t = 0; t < n; t += WAVE) {
        const uint32_t i = t + (uint32_t)lane;
        const int32_t a = i < n ? p[i] : -1, b = i + 1 < n ? p[i + 1] : -1;
        const uint64_t M = wballot(i + 1 < n && a == L.l && b == L.r);
        uint64_t T = M;                                                   // l != r: matches cannot overlap
        if (L.l == L.r) {                                                 // a run of matches: the first, the third, ...
            T = 0;
            uint64_t prev = carry;
            for (int k = 0; k < WAVE; ++k) {
                const uint64_t tk = ((M >> k) & 1ull) & ~prev & 1ull;
                T |= tk << k;
                prev = tk;
            }
        }
        const uint64_t dropped = (T << 1) | carry;
        carry = T >> 63;
        const uint64_t keep = wballot(i < n) & ~dropped;
        if ((keep >> lane) & 1ull) p[out + (uint32_t)__popcll(keep & lt_mask(lane))] = ((T >> lane) & 1ull) ? L.m : a;
        out += (uint32_t)__popcll(keep);
    }
    if (lane == 0) L.wlen[d] = out;
    __threadfence();                                                      // the wave reads what its other lanes stored
    for (uint32_t i = (uint32_t)lane; i + 1 < out; i += WAVE) ln_add(L, p[i], p[i + 1], c);
}

__global__ __launch_bounds__(256) void gz_learn_hist_kernel(GzLearn L)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= L.n_words) return;
    const int32_t* p = L.sym + L.woff[d];
    const uint32_t n = L.wlen[d];
    const long long c = L.cw[d];
    for (uint32_t i = 0; i < n; ++i)
        atomicAdd((unsigned long long*)&L.hist[2 * (int64_t)p[i] + (i + 1 == n ? 1 : 0)], (unsigned long long)c);
}

__global__ __launch_bounds__(256) void gz_learn_rehash_kernel(const GzLearnSlot* from, int64_t n_slots, GzLearn L)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_slots) return;
    const GzLearnSlot o = from[i];
    if (o.key == 0ull) return;
    unsigned long long s = bm_mix64(o.key) & L.mask;
    for (unsigned long long n = 0; n <= L.mask; ++n) {
        if (atomicCAS(&L.tab[s].key, 0ull, o.key) == 0ull) {
            atomicAdd(&L.ctl[2], 1ull);
            L.tab[s].cnt = o.cnt;
            return;
        }
        s = (s + 1) & L.mask;
    }
    atomicOr(&L.ctl[3], 1ull);
}

void gz_launch_learn(int step, const GzLearn& L, hipStream_t s)
{
    const unsigned wg = bm_grid(L.n_words, 256);
    switch (step) {
    case GZ_LEARN_PAIRS: if (L.n_words > 0) hipLaunchKernelGGL(gz_learn_pairs_kernel, dim3(wg), dim3(256), 0, s, L); break;
    case GZ_LEARN_BEST:
        hipLaunchKernelGGL(gz_learn_best_a_kernel, dim3((unsigned)L.n_part), dim3(256), 0, s, L);
        hipLaunchKernelGGL(gz_learn_best_b_kernel, dim3(1), dim3(256), 0, s, L);
        break;
    case GZ_LEARN_APPLY:
        if (L.n_words > 0) hipLaunchKernelGGL(gz_learn_apply_kernel, dim3(wg), dim3(256), 0, s, L);
        if (L.n_long > 0) hipLaunchKernelGGL(gz_learn_apply_long_kernel, dim3(bm_grid(L.n_long, 4)), dim3(256), 0, s, L);
        break;
    case GZ_LEARN_HIST: if (L.n_words > 0) hipLaunchKernelGGL(gz_learn_hist_kernel, dim3(wg), dim3(256), 0, s, L); break;
    default: break;
    }
}

void gz_launch_learn_rehash(const GzLearnSlot* from, int64_t n_slots, const GzLearn& to, hipStream_t s)
{
    if (n_slots > 0) hipLaunchKernelGGL(gz_learn_rehash_kernel, dim3(bm_grid(n_slots, 256)), dim3(256), 0, s, from, n_slots, to);
}

void gz_launch_wordset_count(const GzBm25Args& A, const long long* weight, long long* cnt, int64_t n_terms, int strict, hipStream_t s)
{
    if (A.n_words <= 0) return;
    hipLaunchKernelGGL(gz_wordset_count_kernel, dim3(bm_grid(A.n_words, 256)), dim3(256), 0, s, A, weight, cnt, n_terms, strict);
    hipLaunchKernelGGL(gz_wordset_sum_kernel, dim3(bm_grid(n_terms, 256)), dim3(256), 0, s, cnt, n_terms);
}

void gz_launch_wordset_gather(const uint8_t* tb, const int64_t* tstart, const uint32_t* tlen, const uint32_t* toff, uint8_t* arena, int64_t n,
                              hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(gz_wordset_gather_kernel, dim3(bm_grid(n, 256)), dim3(256), 0, s, tb, tstart, tlen, toff, arena, n);
}
