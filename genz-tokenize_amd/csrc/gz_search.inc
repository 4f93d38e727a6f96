// gz_search.inc -- BM25 search (gz_bm25_search[_device], gz_bm25_match_count, their _bool and _phrase forms): the documents that
// match a query, counted, scored and ranked; included by gz_kernels.hip after gz_topk.inc.  A document matches when it holds at
// least one word of the query (mode "any") or every word of it (mode "all"), none of the query's excluded words and, where the
// query has a phrase, the phrase's words next to each other in this order.
//
// Postings, a term-major view of the doc-major (term, count) entries: poff[T + 1] = exclusive scan of df over every table term
// (a dead term's list is empty), pdoc[n_ent] = the documents of every term.
//   gz_bm25_post_kernel     a wave per document: every entry puts its document id into its term's list through a per-term cursor
// A query chunk (rows = queries, a bitmap of ceil(N / 64) 64-bit words per row, cleared by the caller):
//   gz_bm25_sr_words_kernel a thread per query word: its row, and the slices (SR_SLICE postings each) its list is cut into
//                           (term -1: none); the slice counts are scanned (gz_bm25_scan_*)
//   gz_bm25_sr_driver_kernel (mode "all" only, before the scan) a thread per row: only the row's DRIVER keeps its slices -- the word
//                           with the shortest postings list, ties to the first; a row with a term -1 keeps none.  Every match
//                           holds the driver, so its list is a superset of the answer and the filter makes it exact
//   gz_bm25_sr_mark_kernel  workgroups stride over ALL slices of the chunk (a list of a million documents is hundreds of slices on
//                           as many workgroups, a list of three is one slice; no workgroup is spent on a slice that does not exist):
//                           bit d of the row's bitmap is set for every document d of the slice -- a plain load first, the 64-bit
//                           atomicOr only where the bit is still clear
//   gz_bm25_sr_filter_kernel (mode "all" or excluded words only) a thread per 64-bit word of a row's bitmap: a zero word costs one
//                           load; for every set bit d, d's signature and then the pair table (bm_pair_count, the score kernel's
//                           probe) tell whether d holds a term: the bit goes when a required term is absent (mode "all") or an
//                           excluded one present.  One owner per word, the marking has finished: a plain 64-bit store, only of a
//                           word that changed
//   gz_bm25_sr_phrase_kernel (a phrase search only, on a positional index: seq = the term id of every word, doc-major, woff = the
//                           scan of fieldLens) a WAVE per 64-bit word of a row's bitmap: a zero word costs one load, a row
//                           without a phrase returns at once.  Lane j holds phrase term j (at most 64).  For every set bit d:
//                           one ballot of bm_pair_count tells whether d holds every phrase term at all; then the wave walks
//                           seq[woff[d] .. woff[d + 1]) 64 start positions a trip -- a lane compares the ANCHOR's position (the
//                           phrase term with the shortest postings list, ties to the first) and only on a hit the other terms --
//                           and leaves the document at the first trip with a match.  Every read lies inside the document's own
//                           range: a phrase never matches across two documents.  One owner per word, marking and filter have
//                           finished: a plain 64-bit store, only of a word that changed
//   gz_bm25_sr_count_kernel popcount of every tile (SR_TILE bitmap words) of every row
//   gz_bm25_sr_rows_kernel  a workgroup per row: exclusive scan of its tiles' counts, count[row] = their sum
//   gz_bm25_sr_cand_kernel  the set bits of a tile, in ASCENDING document id, into the row's candidate list (stride M = the largest
//                           count of the rows scored together) at the ranks the scans give
//   gz_bm25_sr_score_kernel a thread per (row, candidate): gz_bm25_score_kernel's operation sequence (bm_doc_factors, bm_word_score:
//                           the same functions) with f from the signature and the pair table; positions behind the row's count are
//                           padded with NaN
//   gz_launch_topk          the unchanged selection over the [rows, M] candidate scores: element = position in the candidate list
//   gz_bm25_sr_out_kernel   position -> document id through the candidate list; -1 / NaN behind the row's count
//
// Vector stores and vector atomics only.  The order of the documents inside a term's list is whatever order the cursor's
// atomics land in, and no answer reads it: a list is only ever turned into bits of a bitmap (an OR), and everything behind the
// bitmap -- counts, ranks, the candidates in ascending id, their scores, the selection's tie rule (the lower position = the lower
// document id) -- is a function of the bits alone.

namespace {
constexpr uint32_t SR_SLICE = 2048;          // postings per slice of the marking kernel (8 per thread)
constexpr int SR_TILE = GZ_SEARCH_TILE;
constexpr unsigned long long SR_NAN = 0x7FF8000000000000ull;       // padding of the candidate scores, and of unfilled outputs
}  // namespace

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_post_kernel(GzBm25Post P)
{
    const int64_t d = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= P.n_docs) return;
    const uint32_t e0 = P.eoff[d], e1 = P.eoff[d + 1];
    for (uint32_t e = e0 + (uint32_t)lane_id(); e < e1; e += WAVE) {
        const uint32_t t = P.ent[e].x;
        if ((int64_t)t >= P.n_terms) { atomicOr(&P.ctl[1], 1u); continue; }
        const uint32_t at = P.poff[t] + atomicAdd(&P.cur[t], 1u);
        if (at >= P.poff[t + 1] || (int64_t)at >= P.n_ent) { atomicOr(&P.ctl[1], 1u); continue; }      // (df and the entries disagree)
        P.pdoc[at] = (uint32_t)d;
    }
}

__global__ __launch_bounds__(256) void gz_bm25_sr_words_kernel(GzBm25Search A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_qw) return;
    const int64_t j = A.qoff[0] + i;                          // the word's absolute index
    int64_t lo = 0, hi = A.rows;                              // the row r with qoff[r] <= j < qoff[r + 1]: the last r with qoff[r] <= j
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.qoff[mid] <= j) lo = mid; else hi = mid;
    }
    const int32_t t = A.qterm[j];
    uint32_t ns = 0;
    if (t >= 0 && (int64_t)t < A.n_terms) ns = (A.poff[t + 1] - A.poff[t] + SR_SLICE - 1) / SR_SLICE;
    A.wrow[i] = (uint32_t)lo;
    A.wns[i] = ns;
}

__global__ __launch_bounds__(256) void gz_bm25_sr_mark_kernel(GzBm25Search A)
{
    const uint32_t total = A.wsoff[A.n_qw];
    for (uint32_t s = blockIdx.x; s < total; s += gridDim.x) {           // (uniform)
        int64_t lo = 0, hi = A.n_qw;                          // the word i with wsoff[i] <= s < wsoff[i + 1]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (A.wsoff[mid] <= s) lo = mid; else hi = mid;
        }
        const uint32_t t = (uint32_t)A.qterm[A.qoff[0] + lo];
        const uint32_t p0 = A.poff[t] + (s - A.wsoff[lo]) * SR_SLICE, pe = A.poff[t + 1];
        const uint32_t p1 = pe - p0 < SR_SLICE ? pe : p0 + SR_SLICE;
        unsigned long long* bm = A.bm + (int64_t)A.wrow[lo] * A.w64;
        for (uint32_t p = p0 + threadIdx.x; p < p1; p += 256) {
            const uint32_t d = A.pdoc[p];
            if ((int64_t)d >= A.n_docs) continue;
            unsigned long long* w = bm + (d >> 6);
            const unsigned long long bit = 1ull << (d & 63u);
            // (a bit, once set, stays: a stale load just costs the atomic)
            if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
        }
    }
}

__global__ __launch_bounds__(256) void gz_bm25_sr_count_kernel(GzBm25Search A)
{
    __shared__ uint32_t wt[4];
    const int64_t row = blockIdx.y, w0 = (int64_t)blockIdx.x * SR_TILE;
    const unsigned long long* bm = A.bm + row * A.w64;
    uint32_t n = 0;
    for (int r = 0; r < SR_TILE / 256; ++r) {
        const int64_t w = w0 + r * 256 + threadIdx.x;
        if (w < A.w64) n += (uint32_t)__popcll(bm[w]);
    }
    uint32_t all;
    (void)bm_block_scan(n, all, wt);
    if (threadIdx.x == 0) A.tcnt[row * A.n_tiles + blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void gz_bm25_sr_rows_kernel(GzBm25Search A)
{
    __shared__ uint32_t wt[4];
    const int64_t row = blockIdx.x;
    uint32_t carry = 0;
    for (int64_t r = 0; r < A.n_tiles; r += 256) {
        const int64_t i = r + threadIdx.x;
        const uint32_t v = i < A.n_tiles ? A.tcnt[row * A.n_tiles + i] : 0u;
        uint32_t all;
        const uint32_t ex = bm_block_scan(v, all, wt);
        if (i < A.n_tiles) A.tbase[row * A.n_tiles + i] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) {
        A.cnt[row] = carry;
        if (A.cnt_out) A.cnt_out[row] = (int64_t)carry;
    }
}

// rows row0 .. row0 + grid.y of the chunk, into candidate lists of stride M.  A thread owns 8 consecutive bitmap words: the ranks
// of its bits follow from one block scan, and it writes them in ascending id.
__global__ __launch_bounds__(256) void gz_bm25_sr_cand_kernel(GzBm25Search A)
{
    __shared__ uint32_t wt[4];
    const int64_t row = A.row0 + blockIdx.y;
    const int64_t w0 = (int64_t)blockIdx.x * SR_TILE + (int64_t)threadIdx.x * (SR_TILE / 256);
    const unsigned long long* bm = A.bm + row * A.w64;
    unsigned long long v[SR_TILE / 256];
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < SR_TILE / 256; ++k) {
        v[k] = w0 + k < A.w64 ? bm[w0 + k] : 0ull;
        n += (uint32_t)__popcll(v[k]);
    }
    uint32_t all;
    uint32_t at = A.tbase[row * A.n_tiles + blockIdx.x] + bm_block_scan(n, all, wt);
    uint32_t* cand = A.cand + (int64_t)blockIdx.y * A.M;
#pragma unroll
    for (int k = 0; k < SR_TILE / 256; ++k) {
        unsigned long long x = v[k];
        while (x) {
            const int b = __ffsll((unsigned long long)x) - 1;
            x &= x - 1;
            if ((int64_t)at < A.M) cand[at] = (uint32_t)((w0 + k) * 64 + b);
            ++at;
        }
    }
}

// occurrences of term t (>= 0) in document d: sg = d's four signature words, pkey = d << 32.  The signature bit first, the pair
// table only where it is set; 0 = d does not hold t (a pair in the table has a count of 1 at least)
__device__ __forceinline__ uint32_t bm_pair_count(const GzBm25Score& S, const unsigned long long (&sg)[4], unsigned long long pkey, uint32_t t)
{
    const uint32_t bit = bm_sig_bit(t);
    const unsigned long long word = bit < 64 ? sg[0] : bit < 128 ? sg[1] : bit < 192 ? sg[2] : sg[3];
    if (!((word >> (bit & 63u)) & 1ull)) return 0;
    const unsigned long long key = (pkey | t) + 1ull;
    unsigned long long sl = bm_mix64(key) & S.pmask;
    for (;;) {
        const unsigned long long kk = S.ptab[sl].key;
        if (kk == key) return S.ptab[sl].a;
        if (kk == 0ull) return 0;
        sl = (sl + 1) & S.pmask;
    }
}

__global__ __launch_bounds__(256) void gz_bm25_sr_driver_kernel(GzBm25Search A)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= A.rows) return;
    const int64_t j0 = A.qoff[row], j1 = A.qoff[row + 1], base = A.qoff[0];
    int64_t best = -1;
    uint32_t len = 0;
    for (int64_t j = j0; j < j1; ++j) {
        const int32_t t = A.qterm[j];
        if (t < 0 || (int64_t)t >= A.n_terms) { best = -1; break; }       // a word no document holds: nothing matches
        const uint32_t n = A.poff[t + 1] - A.poff[t];
        if (best < 0 || n < len) { best = j; len = n; }
    }
    for (int64_t j = j0; j < j1; ++j)
        if (j != best) A.wns[j - base] = 0;
}

__global__ __launch_bounds__(256) void gz_bm25_sr_filter_kernel(GzBm25Search A)
{
    const GzBm25Score& S = A.S;
    const int64_t row = blockIdx.y, w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.w64) return;
    unsigned long long* at = A.bm + row * A.w64 + w;
    const unsigned long long x0 = *at;
    if (!x0) return;
    // (uniform: the workgroup's threads share the row)
    const int64_t r0 = A.qoff[row], r1 = A.mode == 1 ? A.qoff[row + 1] : r0;
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
            for (int64_t j = r0; ok && j < r1; ++j) {
                const int32_t t = A.qterm[j];
                ok = t >= 0 && bm_pair_count(S, sg, pkey, (uint32_t)t) != 0;
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

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_sr_phrase_kernel(GzBm25Search A)
{
    const GzBm25Score& S = A.S;
    const int64_t row = blockIdx.y, w = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (w >= A.w64) return;
    // (everything below is uniform in the wave unless it says "lane")
    const int64_t h0 = A.phoff[row];
    const int L = (int)(A.phoff[row + 1] - h0);
    if (L <= 0 || L > GZ_PHRASE_MAX) return;                  // no phrase: the row stays as the marking and the filter left it
    unsigned long long* at = A.bm + row * A.w64 + w;
    const unsigned long long xv = *at;                        // (every lane the same address; made a scalar: the bit loop is the wave's)
    const unsigned long long x0 = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xv) |
                                  (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(xv >> 32)) << 32;
    if (!x0) return;
    const int lane = lane_id();
    const bool mine = lane < L;
    const int32_t tj = mine ? A.phterm[h0 + lane] : 0;        // lane j: phrase term j
    if (wballot(mine && (tj < 0 || (int64_t)tj >= A.n_terms))) {      // a word no document holds: nothing matches
        if (lane == 0) *at = 0ull;
        return;
    }
    // the anchor: the smallest (list length, position in the phrase) -- a minimum over the lanes
    unsigned long long key = mine ? ((unsigned long long)(A.poff[tj + 1] - A.poff[tj]) << 8) | (unsigned long long)lane : ~0ull;
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, WAVE);
        key = other < key ? other : key;
    }
    const int a = (int)(key & 255ull);
    const uint32_t ta = (uint32_t)__shfl(tj, a, WAVE);
    unsigned long long x = x0, keep = x0;
    while (x) {
        const int b = __ffsll(x) - 1;
        x &= x - 1;
        const int64_t d = w * 64 + b;
        bool ok = d < S.n_docs;
        if (ok) {                                             // 1. does d hold every phrase term at all?  (lane j asks for term j)
            const unsigned long long sg[4] = {S.sig[d * 4], S.sig[d * 4 + 1], S.sig[d * 4 + 2], S.sig[d * 4 + 3]};
            const bool lacks = mine && bm_pair_count(S, sg, (unsigned long long)d << 32, (uint32_t)tj) == 0;
            ok = wballot(lacks) == 0ull;
        }
        if (ok) {                                             // 2. the document's words, 64 start positions a trip
            const int64_t s0 = A.woff[d], s1 = A.woff[d + 1];
            if (s1 < s0 || s1 > A.n_words) {
                if (lane == 0) atomicOr(&A.ctl[1], 1u);
                ok = false;
            } else {
                bool found = false;
                for (int64_t t = s0; !found && t + L <= s1; t += WAVE) {
                    const int64_t p = t + lane;               // (lane) a start: the phrase would be seq[p .. p + L), inside the document
                    bool cand = p + L <= s1 && A.seq[p + a] == ta;
                    if (wballot(cand)) {
                        for (int k = 0; k < L; ++k) {
                            const uint32_t tk = (uint32_t)__shfl(tj, k, WAVE);
                            if (k != a && cand) cand = A.seq[p + k] == tk;
                            if (!wballot(cand)) break;
                        }
                        found = wballot(cand) != 0ull;
                    }
                }
                ok = found;
            }
        }
        if (!ok) keep &= ~(1ull << b);
    }
    if (keep != x0 && lane == 0) *at = keep;
}

__global__ __launch_bounds__(256) void gz_bm25_sr_score_kernel(GzBm25Search A)
{
    const GzBm25Score& S = A.S;                               // (the index's arrays and the parameters; the query arrays are A's)
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
    const int64_t j1 = A.qoff[row + 1];
    for (int64_t j = A.qoff[row]; j < j1; ++j) {              // (uniform: the workgroup's threads share the row)
        const int32_t t = A.qterm[j];
        const uint32_t f = t >= 0 ? bm_pair_count(S, sg, pkey, (uint32_t)t) : 0u;
        score = bm_word_score(S, score, f, K, t0, A.qidf[j]);
    }
    *out = score;
}

// pos / psc: [rows, k2] the selection's positions and scores (k2 = min(kk, M); null when M == 0) -> doc_out / score_out [rows, kk]
__global__ __launch_bounds__(256) void gz_bm25_sr_out_kernel(GzBm25Search A)
{
    const int64_t row = A.row0 + blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= A.kk) return;
    int64_t id = -1;
    double sc = __longlong_as_double((long long)SR_NAN);
    if (j < A.k2 && j < (int64_t)A.cnt[row]) {
        const int64_t p = A.pos[(int64_t)blockIdx.y * A.k2 + j];
        if (p >= 0 && p < A.M) {
            id = (int64_t)A.cand[(int64_t)blockIdx.y * A.M + p];
            sc = A.psc[(int64_t)blockIdx.y * A.k2 + j];
        }
    }
    A.doc_out[(int64_t)blockIdx.y * A.kk + j] = id;
    A.score_out[(int64_t)blockIdx.y * A.kk + j] = sc;
}

void gz_launch_bm25_post(const GzBm25Post& P, hipStream_t s)
{
    if (P.n_docs > 0) hipLaunchKernelGGL(gz_bm25_post_kernel, dim3(bm_grid(P.n_docs, BM_WPB)), dim3(WAVE * BM_WPB), 0, s, P);
}

void gz_launch_bm25_search(int step, const GzBm25Search& A, int64_t rows, hipStream_t s)
{
    if (rows <= 0) return;
    switch (step) {
    case GZ_BM25_SR_WORDS: if (A.n_qw > 0) hipLaunchKernelGGL(gz_bm25_sr_words_kernel, dim3(bm_grid(A.n_qw, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_SR_MARK: {
        // at most one slice per word and SR_SLICE postings, a workgroup each up to 2048 of them; the rest is strided over
        const int64_t most = A.n_qw + (A.n_ent / SR_SLICE + 1) * (A.n_qw < 64 ? A.n_qw : 64);
        if (A.n_qw > 0) hipLaunchKernelGGL(gz_bm25_sr_mark_kernel, dim3((unsigned)(most < 2048 ? most : 2048)), dim3(256), 0, s, A);
        break;
    }
    case GZ_BM25_SR_DRIVER: if (A.n_qw > 0) hipLaunchKernelGGL(gz_bm25_sr_driver_kernel, dim3(bm_grid(rows, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_SR_FILTER: hipLaunchKernelGGL(gz_bm25_sr_filter_kernel, dim3(bm_grid(A.w64, 256), (unsigned)rows), dim3(256), 0, s, A); break;
    case GZ_BM25_SR_PHRASE:
        hipLaunchKernelGGL(gz_bm25_sr_phrase_kernel, dim3(bm_grid(A.w64, BM_WPB), (unsigned)rows), dim3(WAVE * BM_WPB), 0, s, A);
        break;
    case GZ_BM25_SR_COUNT: hipLaunchKernelGGL(gz_bm25_sr_count_kernel, dim3((unsigned)A.n_tiles, (unsigned)rows), dim3(256), 0, s, A); break;
    case GZ_BM25_SR_ROWS: hipLaunchKernelGGL(gz_bm25_sr_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, A); break;
    case GZ_BM25_SR_CAND: if (A.M > 0) hipLaunchKernelGGL(gz_bm25_sr_cand_kernel, dim3((unsigned)A.n_tiles, (unsigned)rows), dim3(256), 0, s, A); break;
    case GZ_BM25_SR_SCORE: if (A.M > 0) hipLaunchKernelGGL(gz_bm25_sr_score_kernel, dim3(bm_grid(A.M, 256), (unsigned)rows), dim3(256), 0, s, A); break;
    case GZ_BM25_SR_OUT: if (A.kk > 0) hipLaunchKernelGGL(gz_bm25_sr_out_kernel, dim3(bm_grid(A.kk, 256), (unsigned)rows), dim3(256), 0, s, A); break;
    default: break;
    }
}
