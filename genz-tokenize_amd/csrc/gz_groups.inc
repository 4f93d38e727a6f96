// gz_groups.inc -- BM25 search over WORD GROUPS (gz_bm25_search_groups[_device], gz_bm25_match_count_groups); included by
// gz_kernels.hip after gz_search.inc.  A group is a set of alternative terms that counts as ONE query word: a document holds the
// group when it holds any alternative, the group's f is the sum of the alternatives' counts, and its idf (host-computed, from the
// documents that hold any alternative) is one number.  Fuzzy, prefix and synonym search are host front ends over it.
//
// Layout (GzBm25Group, absolute indices like qoff / xoff): row r = groups goff[r] .. goff[r + 1]; group g = the alternatives
// qterm[aoff[g] .. aoff[g + 1]) of the chunk's GzBm25Search with idf gidf[g] and signature mask gmask[4 g .. 4 g + 4).  The entry
// point hands the alternatives over DISTINCT and valid (no -1, no repeat, at most GZ_GROUP_MAX a group), so a sum over a group's
// range counts every alternative once.  The flat alternative list is a word list whose row boundaries are qoff[r] = aoff[goff[r]]:
// gz_bm25_sr_words_kernel and gz_bm25_sr_mark_kernel run on it unchanged, and so does everything behind the bitmap (count, rows,
// cand, gz_launch_topk, out).  New here:
//   gz_bm25_gr_mask_kernel   a thread per group (once per call): the OR of its alternatives' signature bits (bm_sig_bit), 256 bits.
//                            A document whose signature ANDs to zero with the mask holds no alternative: four ANDs instead of up to
//                            64 probes.  A non-zero AND proves nothing (a saturated signature passes every mask): the pair table
//                            decides, alternative by alternative
//   gz_bm25_gr_driver_kernel (mode "all" only, before the scan) a thread per row: only the alternatives of the row's DRIVER group
//                            keep their slices -- the group with the smallest SUM of postings-list lengths (an upper bound of its
//                            union), ties to the first; a row with a group without alternatives keeps none.  Every match holds some
//                            alternative of the driver, so the marked union is a superset of the answer and the filter makes it exact
//   gz_bm25_gr_filter_kernel (mode "all" or excluded terms only) gz_bm25_sr_filter_kernel's shape, a thread per 64-bit word of a
//                            row's bitmap: for every set bit d, mode "all" asks every group for (mask, then) one alternative that d
//                            holds; an excluded term that d holds clears it.  One owner per word: a plain 64-bit store
//   gz_bm25_gr_score_kernel  gz_bm25_sr_score_kernel's shape, a thread per (row, candidate): per group f = the sum of bm_pair_count
//                            over its alternatives (skipped where the mask says none), then bm_word_score with the group's idf --
//                            the same functions in the same order, so singleton groups give the plain search's bits
// A row's groups are uniform across a workgroup in the filter and the score stage, as a row's words are in gz_search.inc.
// Vector stores only; no atomics.

// does document d (signature sg) possibly hold an alternative of group g?  false: certainly none
__device__ __forceinline__ bool gr_maybe(const GzBm25Group& G, int64_t g, const unsigned long long (&sg)[4])
{
    const unsigned long long* m = G.gmask + g * 4;
    return ((sg[0] & m[0]) | (sg[1] & m[1]) | (sg[2] & m[2]) | (sg[3] & m[3])) != 0ull;
}

__global__ __launch_bounds__(256) void gz_bm25_gr_mask_kernel(GzBm25Group G)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= G.n_groups) return;
    unsigned long long m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;
    const int64_t a1 = G.aoff[g + 1];
    for (int64_t a = G.aoff[g]; a < a1; ++a) {
        const int32_t t = G.A.qterm[a];
        if (t < 0) continue;
        const uint32_t bit = bm_sig_bit((uint32_t)t), w = bit >> 6;
        const unsigned long long b = 1ull << (bit & 63u);
        m0 |= w == 0u ? b : 0ull; m1 |= w == 1u ? b : 0ull; m2 |= w == 2u ? b : 0ull; m3 |= w == 3u ? b : 0ull;
    }
    G.gmask[g * 4] = m0; G.gmask[g * 4 + 1] = m1; G.gmask[g * 4 + 2] = m2; G.gmask[g * 4 + 3] = m3;
}

__global__ __launch_bounds__(256) void gz_bm25_gr_driver_kernel(GzBm25Group G)
{
    const GzBm25Search& A = G.A;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= A.rows) return;
    const int64_t g0 = G.goff[row], g1 = G.goff[row + 1], base = A.qoff[0];
    int64_t best = -1;
    unsigned long long len = 0;
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t a0 = G.aoff[g], a1 = G.aoff[g + 1];
        unsigned long long n = 0;
        bool known = false;
        for (int64_t a = a0; a < a1; ++a) {
            const int32_t t = A.qterm[a];
            if (t < 0 || (int64_t)t >= A.n_terms) continue;
            known = true;
            n += A.poff[t + 1] - A.poff[t];
        }
        if (!known) { best = -1; break; }                     // a group no document holds: nothing matches
        if (best < 0 || n < len) { best = g; len = n; }
    }
    const int64_t k0 = best < 0 ? 0 : G.aoff[best], k1 = best < 0 ? 0 : G.aoff[best + 1];
    const int64_t j1 = A.qoff[row + 1];
    for (int64_t j = A.qoff[row]; j < j1; ++j)
        if (j < k0 || j >= k1) A.wns[j - base] = 0;
}

__global__ __launch_bounds__(256) void gz_bm25_gr_filter_kernel(GzBm25Group G)
{
    const GzBm25Search& A = G.A;
    const GzBm25Score& S = A.S;
    const int64_t row = blockIdx.y, w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.w64) return;
    unsigned long long* at = A.bm + row * A.w64 + w;
    const unsigned long long x0 = *at;
    if (!x0) return;
    // (uniform: the workgroup's threads share the row)
    const int64_t g0 = G.goff[row], g1 = A.mode == 1 ? G.goff[row + 1] : g0;
    const int64_t e0 = A.xoff ? A.xoff[row] : 0, e1 = A.xoff ? A.xoff[row + 1] : 0;
    unsigned long long x = x0, keep = x0;
    while (x) {
        const int b = __ffsll(x) - 1;
        x &= x - 1;
        const int64_t d = w * 64 + b;
        bool ok = d < S.n_docs;
        if (ok) {
            const unsigned long long sg[4] = {S.sig[d * 4], S.sig[d * 4 + 1], S.sig[d * 4 + 2], S.sig[d * 4 + 3]};
            const unsigned long long pkey = (unsigned long long)d << 32;
            for (int64_t g = g0; ok && g < g1; ++g) {
                ok = false;
                if (!gr_maybe(G, g, sg)) continue;            // (ok stays false: the loop ends)
                const int64_t a1 = G.aoff[g + 1];
                for (int64_t a = G.aoff[g]; !ok && a < a1; ++a) {
                    const int32_t t = A.qterm[a];
                    ok = t >= 0 && bm_pair_count(S, sg, pkey, (uint32_t)t) != 0;
                }
            }
            for (int64_t j = e0; ok && j < e1; ++j) {
                const int32_t t = A.xterm[j];
                if (t >= 0) ok = bm_pair_count(S, sg, pkey, (uint32_t)t) == 0;
            }
        }
        if (!ok) keep &= ~(1ull << b);
    }
    if (keep != x0) *at = keep;
}

__global__ __launch_bounds__(256) void gz_bm25_gr_score_kernel(GzBm25Group G)
{
    const GzBm25Search& A = G.A;
    const GzBm25Score& S = A.S;
    const int64_t row = A.row0 + blockIdx.y, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.M) return;
    double* out = A.csc + (int64_t)blockIdx.y * A.M + i;
    if (i >= (int64_t)A.cnt[row]) { *out = __longlong_as_double((long long)SR_NAN); return; }
    const int64_t d = A.cand[(int64_t)blockIdx.y * A.M + i];
    if (d >= S.n_docs) { *out = __longlong_as_double((long long)SR_NAN); return; }
    double K, t0;
    bm_doc_factors(S, (double)S.dl[d], K, t0);
    const unsigned long long sg[4] = {S.sig[d * 4], S.sig[d * 4 + 1], S.sig[d * 4 + 2], S.sig[d * 4 + 3]};
    const unsigned long long pkey = (unsigned long long)d << 32;
    double score = 0.0;
    const int64_t g1 = G.goff[row + 1];
    for (int64_t g = G.goff[row]; g < g1; ++g) {              // (uniform: the workgroup's threads share the row)
        uint32_t f = 0;
        if (gr_maybe(G, g, sg)) {
            const int64_t a1 = G.aoff[g + 1];
            for (int64_t a = G.aoff[g]; a < a1; ++a) {
                const int32_t t = A.qterm[a];
                if (t >= 0) f += bm_pair_count(S, sg, pkey, (uint32_t)t);
            }
        }
        score = bm_word_score(S, score, f, K, t0, G.gidf[g]);
    }
    *out = score;
}

void gz_launch_bm25_groups(int step, const GzBm25Group& G, int64_t rows, hipStream_t s)
{
    const GzBm25Search& A = G.A;
    switch (step) {
    case GZ_BM25_GR_MASK: if (G.n_groups > 0) hipLaunchKernelGGL(gz_bm25_gr_mask_kernel, dim3(bm_grid(G.n_groups, 256)), dim3(256), 0, s, G); break;
    case GZ_BM25_GR_DRIVER: if (rows > 0 && A.n_qw > 0) hipLaunchKernelGGL(gz_bm25_gr_driver_kernel, dim3(bm_grid(rows, 256)), dim3(256), 0, s, G); break;
    case GZ_BM25_GR_FILTER:
        if (rows > 0) hipLaunchKernelGGL(gz_bm25_gr_filter_kernel, dim3(bm_grid(A.w64, 256), (unsigned)rows), dim3(256), 0, s, G);
        break;
    case GZ_BM25_GR_SCORE:
        if (rows > 0 && A.M > 0) hipLaunchKernelGGL(gz_bm25_gr_score_kernel, dim3(bm_grid(A.M, 256), (unsigned)rows), dim3(256), 0, s, G);
        break;
    default: break;
    }
}
