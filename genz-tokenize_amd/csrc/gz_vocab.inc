// gz_vocab.inc -- BM25 vocabulary queries (gz_bm25_similar, gz_bm25_prefix, gz_bm25_term_bytes): query words against every live
// term of the index, included by gz_kernels.hip after gz_topk.inc.
//
// The terms are addressed by their canonical ids (bm25_number: new id n is table term order[n], nlen[n] bytes at tstart[order[n]]),
// so every kernel here works on an index in any state and reads it only.
//
//   gz_bm25_edit_kernel     Levenshtein distance (unit costs, code points) of VC_G query words to 256 terms per workgroup, by the
//                           bit-parallel recurrence of Myers / Hyyro with the query word as the pattern: one uint64_t per state vector,
//                           hence at most GZ_VOCAB_EDIT_MAX = 64 code points a word.  Per word an open-addressing table (code point ->
//                           the 64-bit mask of its places in the word) is built in LDS; a lane owns a term, decodes its UTF-8 once and
//                           advances the VC_G words' states (Pv, Mv, the score at the word's last place) side by side.  A term whose
//                           byte length proves more than max_edits insertions or deletions against every word of the group is
//                           never read (it has between ceil(bytes / 4) and bytes code points); the distance is exact otherwise.
//   gz_bm25_prefix_kernel   a lane per term, a word per blockIdx.y: the term's first bytes against the word's
//   both write one float64 key per (word, term) in canonical column order -- -(distance * 2^32) + df (exact: distance <= 128,
//   df < 2^31), the prefix form df alone, NaN where the term does not match -- and add the matches of a wave to the word's count
//   (a ballot and one atomic add per wave: a plain sum).  gz_launch_topk over the key rows is then the order (distance, -df, id).
//   gz_bm25_vc_unpack_kernel  the selected keys back into distance and df; id -1, distance -1, df 0 from the word's count on
//   gz_bm25_vc_len_kernel / gz_bm25_vc_gather_kernel   byte lengths and bytes of listed terms (id -1: none), gz_bm25_cp_gather_kernel's
//                           copy: short terms by their lane, longer ones by the wave
//
// Vector stores, LDS atomics and vector atomics only.

namespace {

constexpr int VC_G = 8;                                // query words per workgroup of the distance kernel
constexpr int VC_SLOTS = 128;                          // slots of a word's code point table (at most 64 are used)
static_assert(GZ_VOCAB_EDIT_MAX == 64, "one uint64_t per state vector");

__device__ __forceinline__ uint32_t vc_hash(uint32_t cp) { return (cp * 0x9E3779B1u) >> 25; }         // 7 bits: a slot

}  // namespace

__global__ __launch_bounds__(256) void gz_bm25_edit_kernel(GzBm25Vocab V)
{
    __shared__ uint32_t hk[VC_G * VC_SLOTS];                 // code point + 1 (0: empty)
    __shared__ unsigned long long hm[VC_G * VC_SLOTS];       // bit j: the word's j-th code point is this one
    __shared__ uint32_t wm[VC_G];                            // code points of the word (0 behind the chunk's last word)
    const int t = threadIdx.x, lane = lane_id();
    const int64_t r0 = (int64_t)blockIdx.y * VC_G;
    const int g = (int)(V.rows - r0 < VC_G ? V.rows - r0 : VC_G);
    for (int i = t; i < VC_G * VC_SLOTS; i += 256) { hk[i] = 0u; hm[i] = 0ull; }
    if (t < VC_G) {
        const uint32_t m = t < g ? V.cpoff[r0 + t + 1] - V.cpoff[r0 + t] : 0u;
        wm[t] = m < (uint32_t)GZ_VOCAB_EDIT_MAX ? m : (uint32_t)GZ_VOCAB_EDIT_MAX;        // (the host refuses longer words)
    }
    __syncthreads();
    for (int i = t; i < VC_G * GZ_VOCAB_EDIT_MAX; i += 256) {
        const int w = i / GZ_VOCAB_EDIT_MAX, j = i % GZ_VOCAB_EDIT_MAX;
        if (w < g && (uint32_t)j < wm[w]) {
            const uint32_t cp = V.cps[V.cpoff[r0 + w] + (uint32_t)j];
            uint32_t s = vc_hash(cp);
            for (;;) {                                       // (more slots than code points: an empty one is always met)
                const uint32_t prev = atomicCAS(&hk[w * VC_SLOTS + s], 0u, cp + 1u);
                if (prev == 0u || prev == cp + 1u) break;
                s = (s + 1u) & (uint32_t)(VC_SLOTS - 1);
            }
            atomicOr(&hm[w * VC_SLOTS + s], 1ull << j);
        }
    }
    __syncthreads();

    const int64_t n = (int64_t)blockIdx.x * 256 + t;
    const bool have = n < V.n_new;
    const uint8_t* p = V.tb;
    uint32_t len = 0u, df = 0u;
    if (have) {
        const uint32_t o = V.order[n];
        p = V.tb + V.tstart[o];
        len = V.nlen[n];
        df = V.df[o];
    }
    // the byte length against every word of the group: cpmin <= code points <= len
    const int64_t cpmin = ((int64_t)len + 3) / 4, E = V.max_edits;
    bool any = false;
    unsigned long long Pv[VC_G], Mv[VC_G], top[VC_G];
    int sc[VC_G];
#pragma unroll
    for (int w = 0; w < VC_G; ++w) {
        const int64_t m = wm[w];
        any = any || (w < g && cpmin <= m + E && (int64_t)len + E >= m);
        Pv[w] = ~0ull; Mv[w] = 0ull; sc[w] = (int)m;
        top[w] = m > 0 ? 1ull << (m - 1) : 0ull;
    }
    any = any && have;
    uint32_t ncp = 0u;
    if (any) {                                               // (then len <= 4 * (64 + 64) bytes: a bounded walk)
        auto at = [&](int64_t i) -> uint32_t { return p[i]; };
        for (int64_t i = 0; i < (int64_t)len;) {
            int l;
            const uint32_t cp = decode_cp(at, i, (int64_t)len, l);
            i += l > 0 ? l : 1;
            ++ncp;
            const uint32_t h0 = vc_hash(cp);
#pragma unroll
            for (int w = 0; w < VC_G; ++w) {
                unsigned long long Eq = 0ull;
                uint32_t s = h0;
                for (;;) {
                    const uint32_t k = hk[w * VC_SLOTS + s];
                    if (k == cp + 1u) { Eq = hm[w * VC_SLOTS + s]; break; }
                    if (k == 0u) break;
                    s = (s + 1u) & (uint32_t)(VC_SLOTS - 1);
                }
                const unsigned long long Xv = Eq | Mv[w];
                const unsigned long long Xh = (((Eq & Pv[w]) + Pv[w]) ^ Pv[w]) | Eq;
                unsigned long long Ph = Mv[w] | ~(Xh | Pv[w]);
                unsigned long long Mh = Pv[w] & Xh;
                sc[w] += (Ph & top[w]) ? 1 : 0;
                sc[w] -= (Mh & top[w]) ? 1 : 0;
                Ph = (Ph << 1) | 1ull;                       // (the distance of whole strings: row 0 grows by one per column)
                Mh <<= 1;
                Pv[w] = Mh | ~(Xv | Ph);
                Mv[w] = Ph & Xv;
            }
        }
    }
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
    for (int w = 0; w < VC_G; ++w) {
        if (w >= g) break;                                   // (uniform)
        const int64_t dist = wm[w] ? (int64_t)sc[w] : (int64_t)ncp;
        const bool match = any && dist <= E;
        if (have) V.keys[(r0 + w) * V.n_new + n] = match ? (double)df - (double)dist * 4294967296.0 : nan;
        const unsigned long long b = wballot(match);
        if (b && lane == 0) atomicAdd(&V.cnt[r0 + w], (uint32_t)__popcll(b));
    }
}

__global__ __launch_bounds__(256) void gz_bm25_prefix_kernel(GzBm25Vocab V)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    const int64_t ws = V.woff[r], wl = V.woff[r + 1] - ws;
    bool match = false;
    if (n < V.n_new) {
        const uint32_t o = V.order[n];
        if ((int64_t)V.nlen[n] >= wl) {
            const uint8_t* p = V.tb + V.tstart[o];
            const uint8_t* q = V.wbytes + ws;
            int64_t i = 0;
            while (i < wl && p[i] == q[i]) ++i;
            match = i == wl;
        }
        V.keys[r * V.n_new + n] = match ? (double)V.df[o] : __longlong_as_double(0x7FF8000000000000ll);
    }
    const unsigned long long b = wballot(match);
    if (b && lane_id() == 0) atomicAdd(&V.cnt[r], (uint32_t)__popcll(b));
}

// the selection's (id, key) of every row -> ids, distances, dfs; the padding from the row's count on
__global__ __launch_bounds__(256) void gz_bm25_vc_unpack_kernel(GzBm25Vocab V)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= V.rows * V.k) return;
    const int64_t r = i / V.k, j = i - r * V.k;
    const int64_t c = (int64_t)V.cnt[r];
    if (j == 0) V.cnt_out[r] = c;
    int64_t id = -1;
    int32_t dist = -1, df = 0;
    if (j < c) {
        id = V.sel_id[i];
        const double key = V.sel_key[i];
        if (V.prefix || key > 0.0) { dist = 0; df = (int32_t)key; }
        else {                                               // -key = dist * 2^32 - df, 1 <= df < 2^31
            const int64_t nk = (int64_t)(-key);
            dist = (int32_t)(nk >> 32) + 1;
            df = (int32_t)(((int64_t)dist << 32) - nk);
        }
    }
    V.ids_out[i] = id;
    if (V.dist_out) V.dist_out[i] = dist;
    V.df_out[i] = df;
}

__global__ __launch_bounds__(256) void gz_bm25_vc_len_kernel(GzBm25Vocab V)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= V.n_ids) return;
    const int64_t id = V.ids[i];
    V.len_out[i] = id >= 0 && id < V.n_new ? V.nlen[id] : 0u;
}

__global__ __launch_bounds__(256) void gz_bm25_vc_gather_kernel(GzBm25Vocab V)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    int64_t src = 0, dst = 0;
    uint32_t len = 0u;
    if (i < V.n_ids) {
        const int64_t id = V.ids[i];
        if (id >= 0 && id < V.n_new) {
            src = V.tstart[V.order[id]];
            dst = V.boff[i];
            const int64_t room = V.boff[i + 1] - dst;       // (== nlen[id]: the offsets are the scan of gz_bm25_vc_len_kernel's lengths)
            len = V.nlen[id];
            if ((int64_t)len > room) len = room > 0 ? (uint32_t)room : 0u;
        }
    }
    if (len <= BM_CP_SHORT)
        for (uint32_t b = 0; b < len; ++b) V.bytes[dst + b] = V.tb[src + b];
    uint64_t m = wballot(len > BM_CP_SHORT);
    while (m) {                                              // (uniform)
        const int k = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int64_t s = __shfl(src, k, WAVE), d = __shfl(dst, k, WAVE);
        const uint32_t l = (uint32_t)__shfl((int)len, k, WAVE);
        for (uint32_t b = (uint32_t)lane; b < l; b += WAVE) V.bytes[d + b] = V.tb[s + b];
    }
}

void gz_launch_bm25_vocab(int step, const GzBm25Vocab& V, hipStream_t s)
{
    switch (step) {
    case GZ_BM25_VC_EDIT:
        if (V.rows > 0 && V.n_new > 0)
            hipLaunchKernelGGL(gz_bm25_edit_kernel, dim3(bm_grid(V.n_new, 256), bm_grid(V.rows, VC_G)), dim3(256), 0, s, V);
        break;
    case GZ_BM25_VC_PREFIX:
        if (V.rows > 0 && V.n_new > 0)
            hipLaunchKernelGGL(gz_bm25_prefix_kernel, dim3(bm_grid(V.n_new, 256), (unsigned)V.rows), dim3(256), 0, s, V);
        break;
    case GZ_BM25_VC_UNPACK:
        if (V.rows > 0 && V.k > 0) hipLaunchKernelGGL(gz_bm25_vc_unpack_kernel, dim3(bm_grid(V.rows * V.k, 256)), dim3(256), 0, s, V);
        break;
    case GZ_BM25_VC_LEN: if (V.n_ids > 0) hipLaunchKernelGGL(gz_bm25_vc_len_kernel, dim3(bm_grid(V.n_ids, 256)), dim3(256), 0, s, V); break;
    case GZ_BM25_VC_GATHER: if (V.n_ids > 0) hipLaunchKernelGGL(gz_bm25_vc_gather_kernel, dim3(bm_grid(V.n_ids, 256)), dim3(256), 0, s, V); break;
    default: break;
    }
}
