// gz_near.inc -- BM25 proximity (gz_bm25_search_near[_device], gz_bm25_match_count_near, gz_bm25_cover[_device]): the smallest
// window of a document that holds every term of a set; included by gz_kernels.hip after gz_snippet.inc.  The third reader of the
// positional store (seq = the term id of every word, doc-major; woff = the scan of fieldLens; document d = seq[woff[d] ..
// woff[d + 1])).  Which terms of the set a document holds AT ALL comes from its signature and the pair table (bm_pair_count, the
// phrase kernel's first step); no postings are read.
//
// A set has at most GZ_NEAR_MAX = 64 terms: lane j holds term j, the phrase kernel's layout.  A lane whose term repeats an
// earlier lane's, or is -1, is switched off: the LIVE lanes hold distinct terms, and a set is a set.
//   nr_walk                 the wave walks seq[s0 .. s1) 64 positions a trip.  For every live term k (a uniform loop over the live
//                           mask) b_k = the ballot of "my word is term k"; a lane's last occurrence of k at or before its position
//                           is the highest set bit of b_k at or below the lane, else the CARRY that lane k keeps from the trips
//                           before (-1: none yet).  The minimum over k of these is the start of the shortest window that ENDS at
//                           the lane's position, p - start + 1 its length; it exists once every term has occurred.  (A position
//                           whose own word is no term of the set gives the window of the last hit before it, one word longer: it
//                           never wins.)  Then lane k's carry becomes the highest set bit of b_k.  The filter leaves at the first
//                           trip in which a lane's length is <= the limit; the cover keeps the wave minimum of (length << 32) |
//                           start -- the shortest, ties to the smallest start.  Positions are formed in 64 bits.
//   gz_bm25_sr_near_kernel  (a near search only: the stage behind GZ_BM25_SR_PHRASE) a WAVE per 64-bit word of a row's bitmap, the
//                           phrase kernel's launch shape: a zero word costs one load, a row without near terms returns at once.
//                           A row with a term -1, or a window smaller than its live terms, loses every document.  For every set
//                           bit d: a document that lacks a live term goes before seq is touched; else the walk with the limit
//                           min(window, words of d).  One owner per word, the stages before have finished: a plain 64-bit store,
//                           only of a word that changed
//   gz_bm25_cover_kernel    a wave per pair r = (query r / k, document ids[r]), BM_WPB pairs per workgroup (the snippet kernels'
//                           shape).  The terms the document lacks leave the set -- their number is words_out -- and the walk over
//                           the rest gives start_out / len_out; (0, 0, 0) for a document with none of them, (-1, 0, 0) for an id
//                           outside [0, n_docs).  Lane 0 writes the three outputs
//
// Every read of seq lies in [woff[d], woff[d + 1]) of the bit's or pair's own document, and that range is checked against n_words
// first (ctl[1] is raised otherwise, and where the pair table names a term that the document's words do not hold): a window never
// reaches into the next document.  An id outside [0, n_docs) is never read through.  Vector stores and vector atomics only; the
// one atomic is the OR into ctl[1], which no answer reads.  Nothing an answer reads varies from run to run.

namespace {
constexpr unsigned long long NR_NONE = ~0ull;

// lane j's term of the set sterm[h0 .. h0 + L) (L <= 64): -1 where the lane has none, where the term is -1 (a word no document
// holds; unknown: the set has one) and where an earlier lane holds the same term.  The whole wave calls it.
__device__ __forceinline__ int32_t nr_terms(const GzBm25Near& A, int64_t h0, int L, int lane, bool& unknown)
{
    int32_t tj = lane < L ? A.sterm[h0 + lane] : -1;
    if ((int64_t)tj >= A.n_terms) tj = -1;
    unknown = wballot(lane < L && tj < 0) != 0ull;
    bool dup = false;
    for (int k = 0; k + 1 < L; ++k) {                         // (uniform)
        const int32_t tk = __shfl(tj, k, WAVE);
        dup = dup || (k < lane && tk == tj);
    }
    return dup ? -1 : tj;
}

// bit j: document d (inside [0, n_docs)) holds lane j's term at all -- signature, then pair table
__device__ __forceinline__ uint64_t nr_held(const GzBm25Score& S, int64_t d, int32_t tj)
{
    const unsigned long long sg[4] = {S.sig[d * 4], S.sig[d * 4 + 1], S.sig[d * 4 + 2], S.sig[d * 4 + 3]};
    return wballot(tj >= 0 && bm_pair_count(S, sg, (unsigned long long)d << 32, (uint32_t)tj) != 0);
}

// the document's words seq[s0 .. s1), checked against n_words; false (ctl[1] raised): the word offsets contradict the index
__device__ __forceinline__ bool nr_range(const GzBm25Near& A, int64_t d, int lane, int64_t& s0, int64_t& s1)
{
    const uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.woff[d]);
    const uint32_t w1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.woff[d + 1]);
    s0 = w0; s1 = w1;
    if (w1 < w0 || (int64_t)w1 > A.n_words) {
        if (lane == 0) atomicOr(&A.ctl[1], 1u);
        return false;
    }
    return true;
}

// The smallest window of seq[s0 .. s1) that holds every live term (live: bit j = lane j's term tj counts; not empty, the terms
// differ).  COVER: the wave minimum of (length << 32) | start over all windows, NR_NONE without one.  Else 0 as soon as a trip has
// a window of at most `limit` words, NR_NONE when the document has none.  Uniform result; the whole wave calls it.
template <bool COVER>
__device__ __forceinline__ unsigned long long nr_walk(const uint32_t* seq, int64_t s0, int64_t s1, int32_t tj, uint64_t live, int64_t limit,
                                                      int lane)
{
    const uint64_t upto = (2ull << lane) - 1ull;              // (lane) the lanes at or below me
    long long carry = -1;                                     // (lane k) the last place so far of term k, from s0; -1: none yet
    unsigned long long best = NR_NONE;
    for (int64_t t = s0; t < s1; t += WAVE) {
        const int64_t p = t + lane;                           // (lane) 64 bits
        const bool in = p < s1;
        const uint32_t v = in ? seq[p] : 0u;
        const long long rel = (long long)(t - s0);
        long long lo = 0x7FFFFFFFFFFFFFFFll;                  // (lane) the earliest of the terms' last places at or before p
        for (uint64_t m = live; m; m &= m - 1) {              // (uniform)
            const int k = __ffsll((unsigned long long)m) - 1;
            const uint32_t tk = (uint32_t)__shfl(tj, k, WAVE);
            const long long ck = __shfl(carry, k, WAVE);
            const uint64_t b = wballot(in && v == tk);
            const uint64_t mine = b & upto;
            const long long last = mine ? rel + (63 - __clzll((long long)mine)) : ck;
            lo = last < lo ? last : lo;
            if (lane == k && b) carry = rel + (63 - __clzll((long long)b));
        }
        const bool ok = in && lo >= 0;                        // every term has occurred
        const long long len = (long long)(p - s0) - lo + 1;
        if (!COVER) {
            if (wballot(ok && len <= (long long)limit)) return 0ull;
        } else {
            unsigned long long key = ok ? ((unsigned long long)len << 32) | (unsigned long long)lo : NR_NONE;
            if (wballot(key < best)) {
                for (int o = 32; o >= 1; o >>= 1) {
                    const unsigned long long other = __shfl_xor(key, o, WAVE);
                    key = other < key ? other : key;
                }
                best = key;
            }
        }
    }
    return best;
}
}  // namespace

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_sr_near_kernel(GzBm25Near A)
{
    const int64_t row = blockIdx.y, w = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (w >= A.w64) return;
    // (everything below is uniform in the wave unless it says "lane")
    const int64_t h0 = sn_uniform(A.soff[row]);
    const int64_t L = sn_uniform(A.soff[row + 1]) - h0;
    if (L <= 0 || L > GZ_NEAR_MAX) return;                    // no near terms: the row stays as the stages before left it
    unsigned long long* at = A.bm + row * A.w64 + w;
    const unsigned long long x0 = (unsigned long long)sn_uniform((int64_t)*at);
    if (!x0) return;
    const int lane = lane_id();
    bool unknown;
    const int32_t tj = nr_terms(A, h0, (int)L, lane, unknown);
    const uint64_t live = wballot(tj >= 0);
    const int64_t win = sn_uniform(A.win[row]);
    if (unknown || win < (int64_t)__popcll(live)) {           // a word no document holds, or a window too small for the set
        if (lane == 0) *at = 0ull;
        return;
    }
    unsigned long long x = x0, keep = x0;
    while (x) {
        const int b = __ffsll(x) - 1;
        x &= x - 1;
        const int64_t d = w * 64 + b;
        bool ok = d < A.n_docs;
        if (ok) ok = nr_held(A.S, d, tj) == live;             // a document that lacks a term goes before seq is touched
        if (ok) {
            int64_t s0, s1;
            ok = nr_range(A, d, lane, s0, s1);
            if (ok) {
                const int64_t n = s1 - s0;
                ok = nr_walk<false>(A.seq, s0, s1, tj, live, win < n ? win : n, lane) == 0ull;
            }
        }
        if (!ok) keep &= ~(1ull << b);
    }
    if (keep != x0 && lane == 0) *at = keep;
}

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_cover_kernel(GzBm25Near A)
{
    const int64_t r = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (r >= A.n_pairs) return;
    // (everything below is uniform in the wave unless it says "lane")
    const int lane = lane_id();
    const int64_t q = r / A.k;
    const int64_t h0 = sn_uniform(A.soff[q]);
    const int64_t L = sn_uniform(A.soff[q + 1]) - h0;
    const int64_t d = sn_uniform(A.ids[r]);
    int32_t start = -1, len = 0, words = 0;
    int64_t s0, s1;
    if (d >= 0 && d < A.n_docs && nr_range(A, d, lane, s0, s1)) {
        start = 0;
        if (L > 0 && L <= GZ_NEAR_MAX && s1 > s0) {
            bool unknown;
            const int32_t tj = nr_terms(A, h0, (int)L, lane, unknown);
            const uint64_t held = nr_held(A.S, d, tj);        // the terms the document lacks leave the set
            if (held) {
                const unsigned long long key = nr_walk<true>(A.seq, s0, s1, tj, held, 0, lane);
                if (key == NR_NONE) {                         // (the pair table names a term that the words do not hold)
                    if (lane == 0) atomicOr(&A.ctl[1], 1u);
                } else {
                    words = (int32_t)__popcll(held);
                    start = (int32_t)(uint32_t)key;
                    len = (int32_t)(uint32_t)(key >> 32);
                }
            }
        }
    }
    if (lane == 0) {
        A.start_out[r] = start;
        A.len_out[r] = len;
        A.words_out[r] = words;
    }
}

void gz_launch_bm25_near(int step, const GzBm25Near& A, int64_t rows, hipStream_t s)
{
    switch (step) {
    case GZ_BM25_SR_NEAR:
        if (rows > 0 && A.w64 > 0)
            hipLaunchKernelGGL(gz_bm25_sr_near_kernel, dim3(bm_grid(A.w64, BM_WPB), (unsigned)rows), dim3(WAVE * BM_WPB), 0, s, A);
        break;
    case GZ_BM25_NR_COVER:
        if (A.n_pairs > 0) hipLaunchKernelGGL(gz_bm25_cover_kernel, dim3(bm_grid(A.n_pairs, BM_WPB)), dim3(WAVE * BM_WPB), 0, s, A);
        break;
    default: break;
    }
}
