// gz_topk.inc -- BM25 top-k (gz_bm25_topk[_device]): the k best documents of every score row, selected where the rows lie (HBM),
// included by gz_kernels.hip after gz_bm25.inc.
//
// Order: higher scores first, +0.0 and -0.0 tie, every NaN below every number (-inf included), ties to the lower document index.
// A score's key is a u64 whose ASCENDING order is that order: NaN -> ~0; else -0.0 -> +0.0, the usual sign flip of ascending
// doubles (negative: all bits inverted, else the sign bit set), inverted.  (key, position) is unique, so the top k are the k
// smallest pairs.
//
// gz_topk_kernel<FIRST>: a selection level.  Grid (tiles, rows); a workgroup owns up to GZ_TOPK_TILE_MAX consecutive elements of
// one row, 16 per thread in registers (element p = j * 256 + thread, loads coalesced per j), and keeps the kc = min(k, tile)
// smallest:
//   radix select, MSB first, 8 bits per digit: an LDS histogram of the digit over the elements that still match the prefix (a
//   wave adds its two commonest digits once each -- most documents of a BM25 row share the score 0.0 -- the rest with LDS
//   atomics), a block scan finds the bucket that holds the kc-th element.  Stops after the digit whose whole bucket is taken,
//   else after 8 digits with the exact threshold key.
//   compaction in element order: per slice j a ballot of "below the threshold" and "equal to it" per wave, the waves' counts
//   through LDS; an equal element is taken while fewer than the rank still needed came before it.  No atomics decide an order.
// FIRST reads score rows (element = document); the next levels read the (key, index) candidates of the level before, laid out per
// row as tile after tile in element order, padding (~0, ~0u) only behind the last real candidate: element order is index order,
// so the same compaction keeps ties to the lower index.  A level with one tile per row is the last: it sorts its k winners by
// (key, index) with a bitonic sort in LDS and writes the ids and the scores' original bits (read back from the row).
// Levels after the first use tiles of GZ_TOPK_TILE_MAX >= 4 k: each cuts a row's candidates at least four-fold.
//
// Vector stores and LDS atomics only.

namespace {

constexpr int TK_E = GZ_TOPK_TILE_MAX / 256;           // elements per thread

__device__ __forceinline__ unsigned long long tk_key(double v)
{
    if (v != v) return ~0ull;
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    if (b == 0x8000000000000000ull) b = 0ull;
    const unsigned long long asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return ~asc;
}

// hist[dg] += 1 for every lane with part set
__device__ __forceinline__ void tk_hist_add(uint32_t* hist, bool part, uint32_t dg, int lane)
{
    unsigned long long pend = __ballot(part);
    for (int r = 0; r < 2 && pend; ++r) {
        const int leader = __ffsll((long long)pend) - 1;
        const uint32_t v = (uint32_t)__shfl((int)dg, leader, WAVE);
        const unsigned long long m = __ballot(part && dg == v);
        if (lane == leader) atomicAdd(&hist[v], (uint32_t)__popcll(m));
        pend &= ~m;
        if (dg == v) part = false;
    }
    if (part) atomicAdd(&hist[dg], 1u);
}

__device__ __forceinline__ bool tk_less(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib)
{
    return ka < kb || (ka == kb && ia < ib);
}
}  // namespace

// in_key / in_idx: [rows, m_in] candidates of the level before (FIRST: the score rows, m_in = n_docs); out_*: [rows, m_out] with
// m_out = tiles * min(k, tile) (null on the last level)
template <bool FIRST>
__global__ __launch_bounds__(256) void gz_topk_kernel(GzTopk T, const unsigned long long* in_key, const uint32_t* in_idx, int64_t m_in,
                                                      int tile, unsigned long long* out_key, uint32_t* out_idx, int64_t m_out)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t sel[3];                      // the digit's bucket, elements below it, elements in it
    __shared__ uint2 cnt[TK_E][4];                   // per slice and wave: (below, equal)
    __shared__ unsigned long long sk[GZ_TOPK_SORT];
    __shared__ uint32_t si[GZ_TOPK_SORT];
    const int t = threadIdx.x, lane = lane_id(), wv = t / WAVE;
    const int64_t row = blockIdx.y, p0 = (int64_t)blockIdx.x * tile;
    const int len = (int)(m_in - p0 < tile ? m_in - p0 : tile);
    const uint32_t kc = (uint32_t)(T.k < tile ? T.k : tile);
    const bool last = gridDim.x == 1;

    unsigned long long key[TK_E];
    uint32_t idx[TK_E];
#pragma unroll
    for (int j = 0; j < TK_E; ++j) {
        const int p = j * 256 + t;
        key[j] = ~0ull;
        idx[j] = ~0u;
        if (p < len) {
            if (FIRST) {
                key[j] = tk_key(T.scores[row * T.n_docs + p0 + p]);
                idx[j] = (uint32_t)(p0 + p);
            } else {
                key[j] = in_key[row * m_in + p0 + p];
                idx[j] = in_idx[row * m_in + p0 + p];
            }
        }
    }

    // ---- radix select: afterwards every element with (key & mask) < prefix is taken, and the first kr with (key & mask) == prefix
    unsigned long long prefix = 0ull, mask = 0ull;
    uint32_t kr = kc;                                // (len <= kc: mask 0, every element equal, all taken)
    if ((uint32_t)len > kc) {
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[t] = 0u;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < TK_E; ++j) {
                const bool part = j * 256 + t < len && (key[j] & mask) == prefix;
                tk_hist_add(hist, part, (uint32_t)(key[j] >> shift) & 255u, lane);
            }
            __syncthreads();
            const uint32_t h = hist[t];
            uint32_t all;
            const uint32_t below = bm_block_scan(h, all, wsum);
            if (below < kr && kr <= below + h) { sel[0] = (uint32_t)t; sel[1] = below; sel[2] = h; }
            __syncthreads();
            const uint32_t b = sel[0], hb = sel[2];
            kr -= sel[1];
            prefix |= (unsigned long long)b << shift;
            mask |= 255ull << shift;
            __syncthreads();                         // (sel and hist are written again by the next digit)
            if (hb == kr) break;                     // the whole bucket is taken
        }
    }

    // ---- compaction in element order
#pragma unroll
    for (int j = 0; j < TK_E; ++j) {
        const bool ok = j * 256 + t < len;
        const unsigned long long km = key[j] & mask;
        const unsigned long long bl = __ballot(ok && km < prefix), be = __ballot(ok && km == prefix);
        if (lane == 0) cnt[j][wv] = make_uint2((uint32_t)__popcll(bl), (uint32_t)__popcll(be));
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t nl = 0u, ne = 0u;                       // below / equal elements of the slices before j
    const int64_t ob = row * m_out + (int64_t)blockIdx.x * kc;
#pragma unroll
    for (int j = 0; j < TK_E; ++j) {
        uint32_t wl = 0u, we = 0u, sl = 0u, se = 0u;
        for (int w = 0; w < 4; ++w) {
            const uint2 c2 = cnt[j][w];
            if (w < wv) { wl += c2.x; we += c2.y; }
            sl += c2.x; se += c2.y;
        }
        const bool ok = j * 256 + t < len;
        const unsigned long long km = key[j] & mask;
        const bool lo = ok && km < prefix, eq = ok && km == prefix;
        const unsigned long long bl = __ballot(lo), be = __ballot(eq);
        const uint32_t rl = nl + wl + (uint32_t)__popcll(bl & lt), re = ne + we + (uint32_t)__popcll(be & lt);
        if (lo || (eq && re < kr)) {
            const uint32_t slot = rl + (re < kr ? re : kr);
            if (last) { sk[slot] = key[j]; si[slot] = idx[j]; }
            else { out_key[ob + slot] = key[j]; out_idx[ob + slot] = idx[j]; }
        }
        nl += sl;
        ne += se;
    }
    const uint32_t taken = (uint32_t)len < kc ? (uint32_t)len : kc;
    if (!last) {
        for (uint32_t s = taken + t; s < kc; s += 256) { out_key[ob + s] = ~0ull; out_idx[ob + s] = ~0u; }
        return;
    }

    // ---- last level: sort the winners by (key, index), write ids and scores
    uint32_t P = 2;
    while (P < taken) P <<= 1;
    for (uint32_t s = taken + t; s < P; s += 256) { sk[s] = ~0ull; si[s] = ~0u; }
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = t; i < P / 2; i += 256) {
                const uint32_t a = 2 * i - (i & (stride - 1)), c = a + stride;
                const bool up = (a & size) == 0;
                const unsigned long long ka = sk[a], kb = sk[c];
                const uint32_t ia = si[a], ib = si[c];
                if (tk_less(kb, ib, ka, ia) == up) { sk[a] = kb; si[a] = ib; sk[c] = ka; si[c] = ia; }
            }
        }
    __syncthreads();
    for (uint32_t r = t; r < kc; r += 256) {
        const uint32_t id = si[r];                  // (a real document: every row has >= k of them, padding sorts behind)
        T.doc_out[row * T.k + r] = (int64_t)id;
        T.score_out[row * T.k + r] = id < T.n_docs ? T.scores[row * T.n_docs + id] : __longlong_as_double(-1ll);
    }
}

void gz_launch_topk(const GzTopk& T, hipStream_t s)
{
    if (T.rows <= 0 || T.n_docs <= 0 || T.k <= 0) return;
    const unsigned rows = (unsigned)T.rows;
    int64_t m = T.n_docs, tile = T.tile, tiles = (m + tile - 1) / tile;
    hipLaunchKernelGGL(gz_topk_kernel<true>, dim3((unsigned)tiles, rows), dim3(256), 0, s, T, nullptr, nullptr, m, (int)tile,
                       tiles > 1 ? T.ckey[0] : nullptr, tiles > 1 ? T.cidx[0] : nullptr, gz_topk_level(m, tile, T.k));
    for (int b = 0; tiles > 1; b ^= 1) {
        m = gz_topk_level(m, tile, T.k);
        tile = GZ_TOPK_TILE_MAX;
        tiles = (m + tile - 1) / tile;
        hipLaunchKernelGGL(gz_topk_kernel<false>, dim3((unsigned)tiles, rows), dim3(256), 0, s, T, (const unsigned long long*)T.ckey[b],
                           (const uint32_t*)T.cidx[b], m, (int)tile, tiles > 1 ? T.ckey[b ^ 1] : nullptr, tiles > 1 ? T.cidx[b ^ 1] : nullptr,
                           gz_topk_level(m, tile, T.k));
    }
}
