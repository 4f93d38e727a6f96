// gz_clf.inc -- hashed n-gram class models resident in HBM: bags of hashed k-grams counted per class, the weights of a multinomial a
// class derived from the counts, and the per-class bits of ragged rows under them (included by gz_kernels.hip behind gz_lm.inc, whose
// predecessor shuffle and 64-bit wave sum it uses, gz_pieces.inc, whose body rule and piece walk it uses, and gz_ngram.inc, whose hash).
//
// THE RULE (include/genz_tokenize.h, "hashed n-gram class models").  The body of a row is the row without its skips.  Every k-gram,
// k = 1..N, that ends at body position i with k <= i + 1 is one FEATURE: a body of m ids has sum_k max(0, m - k + 1).  Its bucket is
// the low `bits` bits of the second stream's word of gz_lm.inc's backward chain (H_1 = mix(seed, q[i]), H_k = mix(H_{k-1}, q[i-k+1]),
// h = ng_finish(H_k, k)); B = 2^bits.  The hash decides the bucket and nothing else: two grams in one bucket ARE one feature.
// FIT: count[b][c] += the features with bucket b of the rows with label c (uint32, [B][C] bucket-major); total[c] their sum.
// WEIGHTS: w[b][c] = rint(2^24 (log2(total[c] + a B) - log2(count[b][c] + a))) in float64, int32.  SCORE: n_features[r]; bits_fx[c][r] =
// the sum of w[bucket(f)][c] over the row's features (int64: an integer, no order of addition changes it); best[r] = the class with the
// smallest sum, the smallest class on ties, -1 for a row without features.
//
// THE WALK is gz_lm.inc's: pieces of GZ_PIECE END positions, a wave a piece, a trip 64 positions, lane l owns end position t + l and
// takes its up to N - 1 predecessor ids from the lanes below (lm_pred), the previous trip's ids carried in a register; a piece that
// is not its row's first loads the 64 ids before its start.  Workgroups of CLF_WAVES waves.
// FIT.  The piece list is ORDERED BY CLASS first -- a counting sort over at most 8 keys: the rows pass counts the pieces of every
// class (and the features, which are the class totals: no second pass over the table; and checks the labels), the sort pass hands
// every row its place behind its class's start, one atomicAdd a wave and class -- and a workgroup takes a RUN of consecutive pieces
// of ONE class.  LDS: the workgroup keeps a private uint32 [B] histogram (4 B bytes <= GZ_CLF_LDS_BYTES), adds a trip's features by
// LDS atomics and flushes its non-zero bins once, one global atomicAdd a bin into count[b C + c].  Otherwise features go straight to
// global atomics, a trip's equal unigrams and bigrams combined first by the ballot-match loop of gz_lm_build_kernel<COMBINE>.
// SCORE.  The weights are kept as [B][CP], CP = the classes rounded up to 1, 2, 4, 8, so a bucket's row is one aligned load (two of 16
// bytes at CP = 8).  LDS: 4 B CP bytes <= GZ_CLF_LDS_BYTES: a persistent grid, a workgroup copies the whole table into LDS with
// 16-byte coalesced loads and then takes pieces blockIdx, + gridDim, ...; every gather is an LDS read.  Otherwise the gathers are global
// loads.  CP int64 accumulators a lane, one wave reduction a piece.  A row of one piece stores plainly (and its best); the pieces of a
// longer row meet by 64-bit atomicAdd in rows the launcher preset, and gz_clf_best_kernel follows.
// Bounds: a gram of order k at end i is touched only when k <= K <= i + 1, so body[i - k + 1 .. i] lies inside the body; a bucket is
// below B by its mask.

constexpr int CLF_WAVES = 16;                                                         // waves a workgroup: with 128 KB of LDS a CU holds one

// the features of a body of m ids at order N
__device__ __forceinline__ int64_t clf_features(int64_t m, int N)
{
    int64_t f = 0;
    for (int k = 1; k <= N; ++k) f += m >= k ? m - k + 1 : 0;
    return f;
}

// ROWS: a thread a row.  stats[c] += the row's features, stats[8 + c] += its pieces, c its label; stats[16] |= 1 for a label outside 0..C-1
__global__ __launch_bounds__(256) void gz_clf_rows_kernel(GzClfArgs A, unsigned long long* __restrict__ stats)
{
    __shared__ unsigned long long sum[2 * GZ_CLF_MAX_CLASSES];
    if (threadIdx.x < 2 * GZ_CLF_MAX_CLASSES) sum[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < A.n_rows) {
        const int32_t c = A.labels[r];
        if (c < 0 || c >= A.n_classes) atomicOr(reinterpret_cast<uint32_t*>(stats + 2 * GZ_CLF_MAX_CLASSES), 1u);
        else {
            int64_t m;
            piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
            if (m >= ((int64_t)1 << 31)) m = 0;                                      // (the piece count refuses the call)
            const int64_t f = clf_features(m, A.order), n_pc = A.one_each ? 1 : A.piece_off[r + 1] - A.piece_off[r];
            if (f) atomicAdd(&sum[c], (unsigned long long)f);
            atomicAdd(&sum[GZ_CLF_MAX_CLASSES + c], (unsigned long long)n_pc);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * GZ_CLF_MAX_CLASSES && sum[threadIdx.x]) atomicAdd(stats + threadIdx.x, sum[threadIdx.x]);
}

// SORT: a thread a row.  The row's pieces go to sorted[cls_start[c] + ...]: per class a wave adds its pieces to the class's cursor once
// and its rows share the range out by a prefix sum (a row has fewer than 2^19 pieces: a wave's sum fits 32 bits).  The order inside
// a class is whatever the atomics give: the counts do not depend on it.
__global__ __launch_bounds__(256) void gz_clf_sort_kernel(GzClfArgs A, unsigned long long* __restrict__ cursor)
{
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = r < A.n_rows;
    const int32_t c = live ? A.labels[r] : -1;
    int64_t p0 = 0, n_pc = 0, at = -1;
    if (live) {
        p0 = A.one_each ? r : A.piece_off[r];
        n_pc = A.one_each ? 1 : A.piece_off[r + 1] - p0;
    }
    for (int k = 0; k < A.n_classes; ++k) {                                          // (wave-uniform: every lane stays for the scan)
        int total;
        const int before = wave_excl_sum(c == k ? (int)n_pc : 0, lane, total);
        unsigned long long base = 0ull;
        if (lane == 0 && total) base = atomicAdd(cursor + k, (unsigned long long)total);
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)base, 0, WAVE), hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), 0, WAVE);
        if (c == k) at = A.cls_start[k] + (int64_t)((uint64_t)hi << 32 | lo) + before;
    }
    if (at < 0) return;                                                              // (no row, or a label the rows pass refused)
    for (int64_t j = 0; j < n_pc; ++j) {
        if (!GZ_CHK(911, at + j, A.n_pieces) || at + j >= A.n_pieces) break;
        A.sorted[at + j] = p0 + j;
    }
}

// FIT: workgroup blockIdx.x takes the run of class c's pieces sorted[cls_start[c] + (blockIdx.x - wg_start[c]) run ..), a wave a piece
template <bool LDS>
__global__ __launch_bounds__(WAVE * CLF_WAVES) void gz_clf_fit_kernel(GzClfArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t clf_lds[];                // LDS: the workgroup's histogram, uint32 [B]
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    int c = 0;
    while (c + 1 < A.n_classes && (int64_t)blockIdx.x >= A.wg_start[c + 1]) ++c;
    const int64_t lo = A.cls_start[c] + ((int64_t)blockIdx.x - A.wg_start[c]) * A.run;
    const int64_t hi = lo + A.run < A.cls_start[c + 1] ? lo + A.run : A.cls_start[c + 1];
    const uint32_t B = 1u << A.bits, bmask = B - 1u;
    const uint64_t C = (uint64_t)A.n_classes, cells = (uint64_t)B * C;
    const int N = A.order;
    (void)cells;                                                                     // (the product build's GZ_CHK does not look at it)
    if (LDS) {
        for (uint32_t b = threadIdx.x; b < B; b += WAVE * CLF_WAVES) clf_lds[b] = 0u;
        __syncthreads();
    }
    for (int64_t q = lo + wave; q < hi; q += CLF_WAVES) {                            // (wave-uniform: q, the piece and its bounds)
        const int64_t p = A.sorted[q];
        if (!GZ_CHK(912, p, A.n_pieces) || p < 0 || p >= A.n_pieces) continue;
        int64_t j, n_pc, m;
        const int64_t r = piece_row(A, p, &j, &n_pc);
        const int64_t a = piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
        const int64_t s0 = j * GZ_PIECE, s1 = s0 + GZ_PIECE < m ? s0 + GZ_PIECE : m;
        const int32_t* const body = A.ids + a;                                       // (never read when m == 0)
        uint32_t prev = j > 0 ? (uint32_t)body[s0 - WAVE + lane] : 0u;
        for (int64_t t = s0; t < s1; t += WAVE) {                                    // (wave-uniform bounds: every lane stays for the shuffles)
            const int64_t i = t + lane;
            const bool live = i < s1;
            const uint32_t cur = live ? (uint32_t)body[i] : 0u;
            const int K = !live ? 0 : (i + 1 < N ? (int)(i + 1) : N);
            uint32_t h1 = 0u, h2 = NG_SEED2, x1 = 0u;
#pragma unroll
            for (int k = 1; k <= GZ_CLF_MAX_ORDER; ++k) {
                if (k > N) break;
                const uint32_t x = k == 1 ? cur : lm_pred(cur, prev, lane, k - 1);
                if (k == 2) x1 = x;
                ng_mix(h1, h2, x);
                const uint32_t bucket = (uint32_t)ng_finish(h1, h2, k) & bmask;
                if (LDS) {
                    if (k <= K) atomicAdd(&clf_lds[bucket], 1u);
                    continue;
                }
                uint32_t add = k <= K ? 1u : 0u;
                if (k <= 2) {                                                        // equal grams of the trip: the first lane of each adds them all
                    uint64_t todo = wballot(k <= K);
                    add = 0u;
                    while (todo) {
                        const int L = __builtin_ctzll(todo);
                        const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)cur, L), l1 = (uint32_t)__builtin_amdgcn_readlane((int)x1, L);
                        const uint64_t same = wballot(k <= K && cur == l0 && (k == 1 || x1 == l1));
                        if (lane == L) add = (uint32_t)__builtin_popcountll(same);
                        todo &= ~same;
                    }
                }
                const uint64_t cell = (uint64_t)bucket * C + (uint64_t)c;
                if (add && GZ_CHK(913, cell, cells)) atomicAdd(A.count + cell, add);
            }
            prev = cur;
        }
    }
    if (!LDS) return;
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < B; b += WAVE * CLF_WAVES) {
        const uint32_t v = clf_lds[b];
        const uint64_t cell = (uint64_t)b * C + (uint64_t)c;
        if (v && GZ_CHK(915, cell, cells)) atomicAdd(A.count + cell, v);
    }
}

// DERIVE: a thread a cell of [B][C].  From the counts: w and its copy at [B][CP]; without counts (the caller's weights): the copy alone
__global__ __launch_bounds__(256) void gz_clf_derive_kernel(GzClfArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, C = (uint64_t)A.n_classes;
    if (i >= C << A.bits) return;
    const uint64_t b = i / C, c = i - b * C;
    int32_t w;
    if (A.count) {
        w = (int32_t)__double2ll_rn(16777216.0 * (log2(A.tb[c]) - log2((double)A.count[i] + A.smoothing)));
        A.w[i] = w;
    } else w = A.w[i];
    if (A.wpad != A.w) A.wpad[b * (uint64_t)A.cp + c] = w;
}

// the CP weights of `bucket` added to the lane's sums; tab: [B][CP] in LDS or in memory
template <int CP>
__device__ __forceinline__ void clf_gather(const int32_t* __restrict__ tab, uint32_t bucket, int64_t (&acc)[CP])
{
    const int32_t* const row = tab + (size_t)bucket * CP;
    if (CP == 1) acc[0] += row[0];
    else if (CP == 2) {
        const int2 v = *reinterpret_cast<const int2*>(row);
        acc[0] += v.x; acc[1] += v.y;
    } else {
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) {
            const int4 v = reinterpret_cast<const int4*>(row)[q];
            acc[4 * q] += v.x; acc[4 * q + 1] += v.y; acc[4 * q + 2] += v.z; acc[4 * q + 3] += v.w;
        }
    }
}

// SCORE: the wave's pieces are blockIdx.x CLF_WAVES + wave, + gridDim.x CLF_WAVES, ... (LDS: a persistent grid; otherwise one each)
template <int CP, bool LDS>
__global__ __launch_bounds__(WAVE * CLF_WAVES) void gz_clf_score_kernel(GzClfArgs A)
{
    extern __shared__ __attribute__((aligned(16))) int32_t clf_tab[];                 // LDS: the weights, int32 [B][CP]
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const uint32_t B = 1u << A.bits, bmask = B - 1u;
    const int N = A.order, C = A.n_classes;
    if (LDS) {                                                                       // the whole table: 16 bytes a lane, B CP / 4 >= 64 of them
        const int4* const src = reinterpret_cast<const int4*>(A.wpad);
        int4* const dst = reinterpret_cast<int4*>(clf_tab);
        for (uint32_t i = threadIdx.x; i < B / 4 * CP; i += WAVE * CLF_WAVES) dst[i] = src[i];
        __syncthreads();
    }
    for (int64_t p = (int64_t)blockIdx.x * CLF_WAVES + wave; p < A.n_pieces; p += (int64_t)gridDim.x * CLF_WAVES) {
        int64_t j, n_pc, m;
        const int64_t r = piece_row(A, p, &j, &n_pc);
        const int64_t a = piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
        const int64_t s0 = j * GZ_PIECE, s1 = s0 + GZ_PIECE < m ? s0 + GZ_PIECE : m;
        const int32_t* const body = A.ids + a;                                       // (never read when m == 0)
        uint32_t prev = j > 0 ? (uint32_t)body[s0 - WAVE + lane] : 0u;
        int64_t acc[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) acc[c] = 0;
        for (int64_t t = s0; t < s1; t += WAVE) {                                    // (wave-uniform bounds: every lane stays for the shuffles)
            const int64_t i = t + lane;
            const bool live = i < s1;
            const uint32_t cur = live ? (uint32_t)body[i] : 0u;
            const int K = !live ? 0 : (i + 1 < N ? (int)(i + 1) : N);
            uint32_t h1 = 0u, h2 = NG_SEED2;
#pragma unroll
            for (int k = 1; k <= GZ_CLF_MAX_ORDER; ++k) {
                if (k > N) break;
                ng_mix(h1, h2, k == 1 ? cur : lm_pred(cur, prev, lane, k - 1));
                const uint32_t bucket = (uint32_t)ng_finish(h1, h2, k) & bmask;
                if (k > K || !GZ_CHK(914, bucket, B)) continue;
                if (LDS) clf_gather<CP>(clf_tab, bucket, acc);
                else clf_gather<CP>(A.wpad, bucket, acc);
            }
            prev = cur;
        }
#pragma unroll
        for (int c = 0; c < CP; ++c) acc[c] = (int64_t)lm_wave_sum64((uint64_t)acc[c]);
        if (lane != 0) continue;
        if (j == 0 && A.n_features) {
            const int64_t f = clf_features(m, N);
            A.n_features[r] = f > 0x7FFFFFFF ? 0x7FFFFFFF : (int32_t)f;
        }
        if (n_pc == 1) {
            int32_t best = m > 0 ? 0 : -1;
            int64_t least = acc[0];
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                if (c >= C) break;
                if (A.bits_fx) A.bits_fx[(int64_t)c * A.n_rows + r] = acc[c];
                if (m > 0 && acc[c] < least) { least = acc[c]; best = c; }
            }
            if (A.best) A.best[r] = best;
        } else if (A.bits_fx) {
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                if (c >= C) break;
                if (acc[c]) atomicAdd(reinterpret_cast<unsigned long long*>(A.bits_fx + ((int64_t)c * A.n_rows + r)), (unsigned long long)acc[c]);
            }
        }
    }
}

// BEST of every row from the complete sums (launched where some row has several pieces): a thread a row
__global__ __launch_bounds__(256) void gz_clf_best_kernel(GzClfArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rows) return;
    int64_t m;
    piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
    int32_t best = -1;
    if (m > 0) {
        long long least = A.bits_fx[r];
        best = 0;
        for (int c = 1; c < A.n_classes; ++c) {
            const long long v = A.bits_fx[(int64_t)c * A.n_rows + r];
            if (v < least) { least = v; best = c; }
        }
    }
    A.best[r] = best;
}
