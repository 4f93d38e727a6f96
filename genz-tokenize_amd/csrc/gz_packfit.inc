// gz_packfit.inc -- best-fit packing of short documents into rows of max_len (included by gz_kernels.hip behind gz_packrows.inc,
// whose len kernel and fill body it shares).  The rule and the host plan are in gz_packfit.h.
//
// With L = max_len <= GZ_PACK_FIT_MAX_LEN and len as in gz_packrows.inc, the documents are placed in the order (len descending,
// index ascending).  What a document needs to place itself is its RANK among the documents of its length, by index; everything
// sequential happens on the host over the length histogram (at most L bins).  Passes, all on one stream:
//   len    gz_pack_len_kernel (gz_packrows.inc).
//   rank   PF_T documents per workgroup, PF_WD consecutive ones per wave, 64 per round.  A round matches equal lengths inside the
//          wave by ballots over the length's bits: a document's rank within the wave's run is what the wave's own table in LDS
//          holds for its length plus the equal ones on lower lanes; the lowest lane of every length adds the round's count.  One
//          wave owns one table, so nothing depends on the order in which the waves run.  Then, per length, the four waves' counts
//          become their exclusive prefix (a document's rank in the TILE) and their sum goes to tab[tile][l].
//   cols   per length, the exclusive scan of tab[.][l] over the tiles, in place (16 waves take a sixteenth of the tiles each, sum,
//          exchange, then write), and the total h[l].  A document's rank is rk[d] + tab[d / PF_T][len].
//   (host) h comes down, gz_packfit_plan runs, the events and the final segments go up.  R is known here.
//   rows   a thread per row: row_off from the final segments (a closed form per segment).
//   place  a thread per document: its event by a binary search over the events of its length, then doc_row, doc_col and its place
//          in row_docs.
//   segs   len64[p] = doc_len[row_docs[p]], then the 64-bit scan -> seg_off.
//   fill   gz_pack_fill_kernel<U, true> (gz_packrows.inc): the same cells over the PACKED slots, slot p is document row_docs[p].
// WORKSPACE: rk 4 bytes a document; tab 4 * (L + 1) bytes a tile of PF_T documents, i.e. (L + 1) / 256 bytes a document (0.5 at
// L = 128, 16 at L = 4096), plus 4 * (L + 1) for h; the events and segments, 32 and 16 bytes each.
// Nothing here hands data from one workgroup to another inside a kernel: every dependency is a kernel boundary.

constexpr int PF_T = GZ_FIT_TILE;              // documents per tile of the rank pass
constexpr int PF_WD = PF_T / 4;                // consecutive documents per wave (4 waves a workgroup)
static_assert(PF_WD % WAVE == 0 && PF_WD <= 0xFFFF, "a wave's count of one length fits its 16-bit table entry");

__global__ __launch_bounds__(256) void gz_packfit_rank_kernel(const int32_t* __restrict__ doc_len, int32_t n, int32_t L, int32_t nbits,
                                                              int32_t* __restrict__ tab, int32_t* __restrict__ rk)
{
    extern __shared__ uint16_t pf_cnt[];                                   // [4][L + 1]: documents of length l the wave has seen
    const int W = L + 1, lane = lane_id(), wv = threadIdx.x / WAVE;
    for (int i = threadIdx.x; i < 4 * W; i += 256) pf_cnt[i] = 0;
    __syncthreads();
    uint16_t* const mine = pf_cnt + wv * W;
    const int64_t d0 = (int64_t)blockIdx.x * PF_T + wv * PF_WD + lane;
    int32_t ln[PF_WD / WAVE], loc[PF_WD / WAVE];
#pragma unroll
    for (int r = 0; r < PF_WD / WAVE; ++r) {
        const int64_t d = d0 + r * WAVE;
        const bool valid = d < n;
        int32_t l = valid ? doc_len[d] : 0;
        l = l < 0 ? 0 : l > L ? L : l;                                     // (the len kernel's range; an index into the table whatever it read)
        uint64_t peers = wballot(valid);
        for (int b = 0; b < nbits; ++b) {
            const bool bit = (l >> b) & 1;
            const uint64_t m = wballot(bit);
            peers &= bit ? m : ~m;
        }
        const int lower = below(peers);
        const int32_t seen = valid ? mine[l] : 0;                          // every lane of the round reads before its leaders write
        if (valid && lower == 0) mine[l] = (uint16_t)(seen + __popcll(peers));
        ln[r] = l; loc[r] = seen + lower;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < W; l += 256) {
        const int32_t c0 = pf_cnt[l], c1 = pf_cnt[W + l], c2 = pf_cnt[2 * W + l], c3 = pf_cnt[3 * W + l];
        pf_cnt[l] = 0; pf_cnt[W + l] = (uint16_t)c0; pf_cnt[2 * W + l] = (uint16_t)(c0 + c1); pf_cnt[3 * W + l] = (uint16_t)(c0 + c1 + c2);
        tab[(int64_t)blockIdx.x * W + l] = c0 + c1 + c2 + c3;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PF_WD / WAVE; ++r) {
        const int64_t d = d0 + r * WAVE;
        if (d < n) rk[d] = loc[r] + mine[ln[r]];
    }
}

__global__ __launch_bounds__(1024) void gz_packfit_cols_kernel(int32_t* __restrict__ tab, int32_t tiles, int32_t W, int32_t* __restrict__ hist)
{
    __shared__ int32_t part[16][WAVE];
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const int32_t l = (int32_t)blockIdx.x * WAVE + lane;
    const int32_t each = (tiles + 15) / 16, t0 = wv * each < tiles ? wv * each : tiles, t1 = tiles - t0 > each ? t0 + each : tiles;
    int32_t s = 0;
    if (l < W)
        for (int32_t t = t0; t < t1; ++t) s += tab[(int64_t)t * W + l];
    part[wv][lane] = s;
    __syncthreads();
    int32_t pre = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int32_t w = part[k][lane]; if (k < wv) pre += w; all += w; }
    if (l >= W) return;
    for (int32_t t = t0; t < t1; ++t) {
        const int32_t v = tab[(int64_t)t * W + l];
        tab[(int64_t)t * W + l] = pre;
        pre += v;
    }
    if (wv == 0) hist[l] = all;
}

// a thread per row i <= R: row_off[i] from the last segment that starts at or before i (seg[n_seg - 1] = {R, 0, N} closes the list)
__global__ __launch_bounds__(256) void gz_packfit_rows_kernel(const GzFitSeg* __restrict__ seg, int32_t n_seg, int64_t R, int64_t* __restrict__ pack_off)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > R) return;
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].row <= i) lo = mid; else hi = mid - 1;
    }
    const GzFitSeg g = seg[lo];
    pack_off[i] = g.base + (i - g.row) * g.docs;
}

__global__ __launch_bounds__(256) void gz_packfit_place_kernel(const int32_t* __restrict__ doc_len, const int32_t* __restrict__ rk,
                                                               const int32_t* __restrict__ tab, int32_t n, int32_t L, int64_t R,
                                                               const GzFitEvent* __restrict__ ev, const int32_t* __restrict__ ev_off,
                                                               const int64_t* __restrict__ pack_off, int32_t* __restrict__ doc_row,
                                                               int32_t* __restrict__ doc_col, int32_t* __restrict__ row_docs)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n) return;
    const int32_t l = doc_len[d];
    if (l < 2 || l > L) return;                                            // (never: the len kernel's range)
    const int32_t j = rk[d] + tab[(d / PF_T) * (L + 1) + l];
    int32_t lo = ev_off[l + 1], hi = ev_off[l] - 1;                        // the last event of this length that starts at or before rank j
    if (hi < lo) return;                                                   // (never: a length that occurs has an event)
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (ev[mid].start <= j) lo = mid; else hi = mid - 1;
    }
    const GzFitEvent e = ev[lo];
    const int32_t q = j - e.start, in = q / e.k, slot = q - in * e.k, row = e.row + in;
    if (q < 0 || row >= R) return;                                         // (never: the plan covers every rank)
    const int64_t at = pack_off[row] + e.before + slot;
    doc_row[d] = row;
    doc_col[d] = e.col0 + slot * l;
    if (at < n) row_docs[at] = (int32_t)d;
}

__global__ __launch_bounds__(256) void gz_packfit_seglen_kernel(const int32_t* __restrict__ doc_len, const int32_t* __restrict__ row_docs, int32_t n,
                                                                int64_t* __restrict__ len64)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) len64[p] = doc_len[row_docs[p]];
}
