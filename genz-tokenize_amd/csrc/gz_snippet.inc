// gz_snippet.inc -- BM25 snippets (gz_bm25_snippets[_device], gz_bm25_occurrences): where the words of a query stand INSIDE given
// documents of a positional index; included by gz_kernels.hip after gz_search.inc.  The second reader of the positional store
// (seq = the term id of every word, doc-major; woff = the scan of fieldLens; document d = seq[woff[d] .. woff[d + 1])): nothing
// else of the index is read, no postings, no pair table.
//
// A pair r = (query r / k, document ids[r]); a wave per pair, BM_WPB pairs per workgroup.  With h[p] = 1 where word p of the
// document is one of the query's terms:
//   gz_bm25_sn_window_kernel the window of `width` words with the most hits, the SMALLEST start among the best.  hits(0) is counted
//                           over the first min(width, n) words; then the wave walks the starts 1 .. n - width, 64 a trip: lane l
//                           looks at start s = t + l, whose count differs from the one before by h[s - 1 + width] - h[s - 1] (the
//                           word that enters, the word that leaves; both inside the document, positions formed in 64 bits).  A
//                           wave prefix sum of these deltas plus the carry of the trips before gives hits(s); a wave arg-max with
//                           ties to the lower lane replaces the best so far only when STRICTLY greater.  No per-document buffer.
//   gz_bm25_sn_count_kernel the occurrences of every pair: popcounts of the ballots of h, 64 words a trip; their sum over all pairs
//                           goes into a 64-bit counter (the host refuses 2^32 or more before the 32-bit scan is believed)
//   (gz_bm25_scan_*)        the exclusive scan of the pair counts
//   gz_bm25_sn_fill_kernel  position and word index of every occurrence at base + (set bits of the ballot below my lane): ascending
//                           inside a pair by construction, pairs in order by the scan
// Membership ("is seq[p] a term of the query, and which is the first") is asked with the lanes HOLDING the query's terms, 64 at a
// time, each handed round with __shfl -- the phrase kernel's pattern, looped over chunks of 64 for a longer query; the lowest
// matching index wins, a term -1 (a word no document holds) matches nothing.
//
// Every read of seq lies in [woff[d], woff[d + 1]) of the pair's own document, and that range is checked against n_words first
// (ctl[1] is raised otherwise, as the phrase kernel does): a window never reaches into the next document.  An id outside
// [0, n_docs) is never read through: the pair has no words.  Vector stores only; the one atomic is the 64-bit sum, which no
// answer reads.  Nothing an answer reads varies from run to run.

namespace {
struct SnPair {
    int64_t s0, s1;                                           // the document's words: seq[s0 .. s1)
    int64_t j0, L;                                            // the query's terms: qterm[j0 .. j0 + L)
};

__device__ __forceinline__ int64_t sn_uniform(int64_t v)      // (every lane holds the same value: into scalar registers)
{
    return (int64_t)((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
                     (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long long)v >> 32)) << 32);
}

// the pair's query and document; false: no document (id outside [0, n_docs), or word offsets that contradict the index)
__device__ __forceinline__ bool sn_pair(const GzBm25Snip& A, int64_t r, int lane, SnPair& P)
{
    const int64_t q = r / A.k;
    P.j0 = sn_uniform(A.qoff[q]);
    P.L = sn_uniform(A.qoff[q + 1]) - P.j0;
    P.s0 = P.s1 = 0;
    const int64_t d = sn_uniform(A.ids[r]);
    if (d < 0 || d >= A.n_docs) return false;
    const uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.woff[d]);
    const uint32_t w1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.woff[d + 1]);
    if (w1 < w0 || (int64_t)w1 > A.n_words) {
        if (lane == 0) atomicOr(&A.ctl[1], 1u);
        return false;
    }
    P.s0 = w0; P.s1 = w1;
    return true;
}

// lane j's term of the query's first chunk (-1 behind the query's end): loaded once per pair
__device__ __forceinline__ int32_t sn_chunk0(const GzBm25Snip& A, const SnPair& P, int lane)
{
    return (int64_t)lane < P.L ? A.qterm[P.j0 + lane] : -1;
}

// idx[i] = the first place in the query of the term v[i] (in[i]: the lane has such a word), -1: none.  The whole wave calls it.
template <int N>
__device__ __forceinline__ void sn_member(const GzBm25Snip& A, const SnPair& P, int32_t t0, int lane, const bool (&in)[N], const uint32_t (&v)[N],
                                          int32_t (&idx)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) idx[i] = -1;
    for (int64_t c = 0; c < P.L; c += WAVE) {                 // (uniform)
        const int32_t tj = c == 0 ? t0 : (c + lane < P.L ? A.qterm[P.j0 + c + lane] : -1);
        const int m = P.L - c < WAVE ? (int)(P.L - c) : WAVE;
        for (int k = 0; k < m; ++k) {
            const int32_t tk = __shfl(tj, k, WAVE);
#pragma unroll
            for (int i = 0; i < N; ++i)
                if (idx[i] < 0 && in[i] && tk >= 0 && v[i] == (uint32_t)tk) idx[i] = (int32_t)(c + k);
        }
        bool open = false;
#pragma unroll
        for (int i = 0; i < N; ++i) open = open || (in[i] && idx[i] < 0);
        if (!wballot(open)) break;                            // every word of this trip is placed
    }
}
}  // namespace

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_sn_window_kernel(GzBm25Snip A)
{
    const int64_t r = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (r >= A.n_pairs) return;
    // (everything below is uniform in the wave unless it says "lane")
    const int lane = lane_id();
    SnPair P;
    int32_t start = -1, best = 0;
    if (sn_pair(A, r, lane, P)) {
        start = 0;
        const int64_t n = P.s1 - P.s0, w = A.width;
        if (n > 0 && P.L > 0) {
            const int32_t t0 = sn_chunk0(A, P, lane);
            // hits(0): the first min(w, n) words
            const int64_t e0 = P.s0 + (w < n ? w : n);
            for (int64_t t = P.s0; t < e0; t += WAVE) {
                const int64_t p = t + lane;                   // (lane)
                const bool in[1] = {p < e0};
                const uint32_t v[1] = {in[0] ? A.seq[p] : 0u};
                int32_t idx[1];
                sn_member<1>(A, P, t0, lane, in, v, idx);
                best += (int32_t)__popcll(wballot(idx[0] >= 0));
            }
            // the starts 1 .. n - w: hits(s) = hits(s - 1) + h[s - 1 + w] - h[s - 1]
            const int64_t ns = n > w ? n - w + 1 : 1;
            int32_t carry = best;                             // hits of the start before this trip's first
            for (int64_t t = 1; t < ns; t += WAVE) {
                const int64_t s = t + lane;                   // (lane) a start
                const int64_t pa = P.s0 + s - 1, pb = pa + w; // the word that leaves, the word that enters (64 bits)
                const bool in[2] = {s < ns && pa < P.s1, s < ns && pb < P.s1};
                const uint32_t v[2] = {in[0] ? A.seq[pa] : 0u, in[1] ? A.seq[pb] : 0u};
                int32_t idx[2];
                sn_member<2>(A, P, t0, lane, in, v, idx);
                const int delta = (idx[1] >= 0 ? 1 : 0) - (idx[0] >= 0 ? 1 : 0);
                int total;
                const int32_t hv = carry + wave_excl_sum(delta, lane, total) + delta;      // (lane) hits(s)
                carry += total;
                const bool better = s < ns && hv > best;
                if (wballot(better)) {                        // the largest count, ties to the lower lane = the smaller start
                    unsigned long long key = better ? ((unsigned long long)(uint32_t)hv << 8) | (unsigned long long)(WAVE - 1 - lane) : 0ull;
                    for (int o = 32; o >= 1; o >>= 1) {
                        const unsigned long long other = __shfl_xor(key, o, WAVE);
                        key = other > key ? other : key;
                    }
                    best = (int32_t)(key >> 8);
                    start = (int32_t)(t + (WAVE - 1 - (int)(key & 255ull)));
                }
            }
        }
    }
    if (lane == 0) {
        A.start_out[r] = start;
        A.hits_out[r] = best;
    }
}

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_sn_count_kernel(GzBm25Snip A)
{
    const int64_t r = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (r >= A.n_pairs) return;
    const int lane = lane_id();
    SnPair P;
    uint32_t n = 0;
    if (sn_pair(A, r, lane, P) && P.L > 0) {
        const int32_t t0 = sn_chunk0(A, P, lane);
        for (int64_t t = P.s0; t < P.s1; t += WAVE) {
            const int64_t p = t + lane;                       // (lane)
            const bool in[1] = {p < P.s1};
            const uint32_t v[1] = {in[0] ? A.seq[p] : 0u};
            int32_t idx[1];
            sn_member<1>(A, P, t0, lane, in, v, idx);
            n += (uint32_t)__popcll(wballot(idx[0] >= 0));
        }
    }
    if (lane == 0) {
        A.cnt[r] = n;
        if (n) atomicAdd(reinterpret_cast<unsigned long long*>(A.ctl + 4), (unsigned long long)n);
    }
}

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_sn_fill_kernel(GzBm25Snip A)
{
    const int64_t r = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (r >= A.n_pairs) return;
    const int lane = lane_id();
    SnPair P;
    if (!sn_pair(A, r, lane, P) || P.L <= 0) return;
    uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.base[r]);
    const uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.base[r + 1]);
    const int32_t t0 = sn_chunk0(A, P, lane);
    for (int64_t t = P.s0; t < P.s1; t += WAVE) {
        const int64_t p = t + lane;                           // (lane)
        const bool in[1] = {p < P.s1};
        const uint32_t v[1] = {in[0] ? A.seq[p] : 0u};
        int32_t idx[1];
        sn_member<1>(A, P, t0, lane, in, v, idx);
        const uint64_t b = wballot(idx[0] >= 0);
        const uint32_t mine = at + (uint32_t)below(b);        // (lane)
        if (idx[0] >= 0 && mine >= at && mine < end) {        // (inside the pair's own range: what the count kernel found)
            A.pos_out[mine] = (int32_t)(p - P.s0);
            A.word_out[mine] = idx[0];
        }
        at += (uint32_t)__popcll(b);
    }
}

void gz_launch_bm25_snippet(int step, const GzBm25Snip& A, hipStream_t s)
{
    if (A.n_pairs <= 0) return;
    const dim3 grid(bm_grid(A.n_pairs, BM_WPB)), block(WAVE * BM_WPB);
    switch (step) {
    case GZ_BM25_SN_WINDOW: hipLaunchKernelGGL(gz_bm25_sn_window_kernel, grid, block, 0, s, A); break;
    case GZ_BM25_SN_COUNT: hipLaunchKernelGGL(gz_bm25_sn_count_kernel, grid, block, 0, s, A); break;
    case GZ_BM25_SN_FILL: hipLaunchKernelGGL(gz_bm25_sn_fill_kernel, grid, block, 0, s, A); break;
    default: break;
    }
}
