// gz_packrows.inc -- short documents packed back to back into rows of max_len (included by gz_kernels.hip).
// (Not gz_pack.c, which packs Python strings on the host.)
//
// With L = max_len and body = the row without its frame (T tokens), document r is seg_r = [bos] + body[:min(T, L-2)] + [eos],
// len_r = min(T, L-2) + 2 in [2, L]: the reference's own row without its padding (tokenize.py:141-146).  Next-fit, order kept:
// a document that does not fit behind the ones before it opens the next row.  seg_off = the exclusive scan of len;
//
//   nxt(i) = the largest j <= N with seg_off[j] - seg_off[i] <= L        (the first document that no longer fits behind i;
//                                                                          nxt(i) - i <= L / 2 because every len >= 2)
//
// and the row heads are the orbit of document 0 under nxt: a sequential chain, where row k+1 starts depends on where row k did.
// Passes (all on one stream):
//   len    a thread per document: len, then the 64-bit scan that decode and the window pass use -> seg_off.
//   tile   PK_B documents per workgroup.  Pointer doubling in LDS gives for EVERY document i of the tile, as if it were a head,
//          exit(i) = the first orbit element at or beyond the tile's end and cnt(i) = the orbit elements of i inside the tile.
//          (nxt itself, a binary search in seg_off, is kept for the mark pass.)
//   hop    PK_G tiles form a group.  A chain can enter a group only in its first K = min(L / 2, group) documents; for each of those a
//          thread follows exit() to the group's end: PK_G dependent loads, all entries of all groups at once.
//   down   a thread per group follows the hops from document 0 to its group (one lookup per group before it, in LDS when the
//          hop table fits there), then exit() through
//          its own tiles: every tile's true entry (or none: a row longer than a tile skips it) and the number of heads before it.
//   mark   per tile, from its entry: the doubling tables of all levels stay in LDS, thread d takes the d-th successor of the
//          entry in <= 10 lookups -> row_off[base + d]; every document finds its head among them -> doc_row.
//   col    doc_col = seg_off[r] - seg_off[row_off[doc_row[r]]]  (the head may lie in an earlier tile); a call that also fills
//          leaves this to the fill, which needs the same three loads.
//   fill   divided over DOCUMENTS' cells, which lie back to back in the output: a workgroup owns the cells from its first
//          document's first cell to its last document's row tail, in units of U cells (16-byte stores where L % 4 == 0).  Ids,
//          frame, tail, mask, segment and position leave together; every cell of [R, L] is written once, nothing is cleared.
//          It takes R from device memory and checks the caller's capacity itself, so it is enqueued right behind the maps:
//          the host learns R (and reports a capacity error) once, after everything.
// Nothing here hands data from one workgroup to another inside a kernel: every dependency is a kernel boundary.

constexpr int PK_B = GZ_PACK_TILE;             // documents per tile = threads per workgroup of the tile and mark kernels
constexpr int PK_LV = 10;                      // 2^PK_LV = PK_B
constexpr int PK_G = GZ_PACK_GROUP;            // tiles per group
constexpr int PK_GB = PK_B * PK_G;             // documents per group
constexpr int PK_FD = 256;                     // documents per workgroup of the fill
constexpr int PK_AL = 32;                      // the fill's workgroups meet on multiples of PK_AL cells: every wave stores whole 128-byte lines
constexpr int PK_STAGE = 8192;                 // hop entries the down kernel keeps in LDS (64 KB)
static_assert((1 << PK_LV) == PK_B, "doubling levels");

__global__ __launch_bounds__(256) void gz_pack_len_kernel(const int64_t* __restrict__ row_off, int32_t n, int32_t room, int32_t skip,
                                                          int64_t* __restrict__ len64, int32_t* __restrict__ doc_len)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int64_t T = row_off[r + 1] - row_off[r] - skip;                       // absolute offsets from the ids base pointer
    T = T < 0 ? 0 : T > room ? room : T;
    len64[r] = T + 2;
    if (doc_len) doc_len[r] = (int32_t)T + 2;
}

// the first document that does not fit into the row document i opens (n when all the rest fits)
__device__ __forceinline__ int32_t pack_nxt(const int64_t* __restrict__ seg, int32_t i, int32_t n, int32_t L)
{
    const int64_t lim = seg[i] + L;
    int32_t lo = i + 1, hi = n - i > L / 2 ? i + L / 2 : n;              // seg[i + 1] <= lim always: len <= L
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (seg[mid] <= lim) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(PK_B) void gz_pack_tile_kernel(const int64_t* __restrict__ seg, int32_t n, int32_t L, int2* __restrict__ jc,
                                                            int32_t* __restrict__ nxt)
{
    __shared__ int32_t q[PK_B], ex[PK_B], cn[PK_B];                        // where i stands now (PK_B: it has left the tile), its exit, heads so far
    const int i = threadIdx.x;
    const int32_t tS = (int32_t)blockIdx.x * PK_B, tE = n - tS > PK_B ? tS + PK_B : n, g = tS + i;
    int32_t myq = PK_B, myex = n, myc = 0;
    if (g < n) {
        const int32_t n0 = pack_nxt(seg, g, n, L);
        nxt[g] = n0;                                                       // (the mark pass takes it from here)
        myc = 1;
        if (n0 < tE) myq = n0 - tS; else myex = n0;
    }
    q[i] = myq; ex[i] = myex; cn[i] = myc;
    __syncthreads();
    for (int k = 0; k < PK_LV; ++k) {                                      // after round k every pointer has taken 2^(k+1) steps or left
        int32_t a = myq, e2 = myex, c2 = 0;
        if (myq < PK_B) { a = q[myq]; e2 = ex[myq]; c2 = cn[myq]; }
        const int more = __syncthreads_or(a < PK_B);                       // (the barrier between this round's reads and its writes)
        myq = a; myex = e2; myc += c2;
        q[i] = myq; ex[i] = myex; cn[i] = myc;
        __syncthreads();
        if (!more) break;
    }
    if (g < n) jc[g] = make_int2(myex, myc);
}

__global__ __launch_bounds__(256) void gz_pack_hop_kernel(const int2* __restrict__ jc, int32_t n, int32_t K, int32_t blocks_per_group,
                                                          int2* __restrict__ jc2)
{
    const int32_t s = (int32_t)(blockIdx.x / blocks_per_group), o = (int32_t)(blockIdx.x % blocks_per_group) * 256 + threadIdx.x;
    const int32_t gS = s * PK_GB, gE = n - gS > PK_GB ? gS + PK_GB : n;
    if (o >= K || o >= gE - gS) return;
    int32_t e = gS + o, c = 0;
    while (e < gE) { const int2 v = jc[e]; c += v.y; e = v.x; }
    jc2[(int64_t)s * K + o] = make_int2(e, c);
}

__global__ __launch_bounds__(256) void gz_pack_down_kernel(const int2* __restrict__ jc, const int2* __restrict__ jc2, int32_t n, int32_t K,
                                                           int32_t n_tiles, int2* __restrict__ tile, int64_t* __restrict__ pack_off,
                                                           int64_t* __restrict__ total)
{
    __shared__ int2 hops[PK_STAGE];                                        // the hop table, when it fits: the walk below is one lookup after the other
    const int32_t n_groups = (n_tiles + PK_G - 1) / PK_G, s = (int32_t)blockIdx.x * 256 + threadIdx.x;
    const bool staged = (int64_t)n_groups * K <= PK_STAGE;
    if (staged) {
        for (int32_t k = threadIdx.x; k < n_groups * K; k += 256) hops[k] = jc2[k];
        __syncthreads();
    }
    if (s >= n_groups) return;
    const int32_t gS = s * PK_GB;
    int32_t e = 0, base = 0;                                               // the chain's element at or beyond gS, the heads before it
    while (e < gS) {                                                       // (an entry from outside lies in its group's first K documents)
        const int32_t s2 = e / PK_GB;
        const int64_t at = (int64_t)s2 * K + (e - s2 * PK_GB);
        const int2 v = staged ? hops[at] : jc2[at];
        base += v.y; e = v.x;
    }
    const int32_t t1 = (s + 1) * PK_G < n_tiles ? (s + 1) * PK_G : n_tiles;
    for (int32_t t = s * PK_G; t < t1; ++t) {
        const int32_t tE = n - t * PK_B > PK_B ? (t + 1) * PK_B : n;
        if (e < tE) {
            tile[t] = make_int2(e, base);
            const int2 v = jc[e];
            base += v.y; e = v.x;
        } else tile[t] = make_int2(-1, base);                              // the chain passes over this tile
    }
    if (s == n_groups - 1) { *total = base; pack_off[base] = n; }
}

__global__ __launch_bounds__(PK_B) void gz_pack_mark_kernel(const int32_t* __restrict__ nxt, int32_t n, const int2* __restrict__ tile,
                                                            int64_t* __restrict__ pack_off, int32_t* __restrict__ doc_row)
{
    __shared__ uint16_t up[PK_LV][PK_B];                                   // up[k][i]: 2^k steps from i, PK_B once outside the tile
    __shared__ uint16_t heads[PK_B];
    const int i = threadIdx.x;
    const int32_t tS = (int32_t)blockIdx.x * PK_B, tE = n - tS > PK_B ? tS + PK_B : n, g = tS + i;
    const int2 tb = tile[blockIdx.x];
    const int32_t entry = tb.x, base = tb.y;
    if (entry < 0) {                                                       // (the whole workgroup) no head here: all in the row before
        if (g < n) doc_row[g] = base - 1;
        return;
    }
    uint16_t u = PK_B;
    if (g < n) {
        const int32_t n0 = nxt[g];
        if (n0 < tE) u = (uint16_t)(n0 - tS);
    }
    up[0][i] = u;
    __syncthreads();
    for (int k = 1; k < PK_LV; ++k) {
        const uint16_t a = up[k - 1][i];
        up[k][i] = a < PK_B ? up[k - 1][a] : (uint16_t)PK_B;
        __syncthreads();
    }
    // thread d: the d-th successor of the entry (d < PK_B = 2^PK_LV); successors grow, so the ones inside the tile are a prefix
    uint16_t a = (uint16_t)(entry - tS);
#pragma unroll
    for (int k = 0; k < PK_LV; ++k)
        if (((i >> k) & 1) && a < PK_B) a = up[k][a];
    const bool is_head = a < PK_B;
    heads[i] = is_head ? a : (uint16_t)0xFFFF;
    if (is_head) pack_off[(int64_t)base + i] = (int64_t)tS + a;
    const int cnt = __syncthreads_count(is_head);
    if (g < n) {
        int lo = 0, hi = cnt;                                              // heads at or before i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)heads[mid] <= i) lo = mid + 1; else hi = mid;
        }
        doc_row[g] = base + lo - 1;                                        // (none: the last row of an earlier tile)
    }
}

__global__ __launch_bounds__(256) void gz_pack_col_kernel(const int64_t* __restrict__ seg, const int64_t* __restrict__ pack_off,
                                                          const int32_t* __restrict__ doc_row, int32_t n, int32_t* __restrict__ doc_col)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    doc_col[r] = (int32_t)(seg[r] - seg[pack_off[doc_row[r]]]);
}

// U cells per thread and store: 4 (rows and base pointers 16-byte aligned) or 1 (any L)
// FIT (best-fit order, gz_packfit.inc): the same cells over the PACKED slots -- slot d is document A.row_docs[d], the maps are
// complete, and the host knows R = A.fit_rows and has checked the capacity before the launch.
template <int U, bool FIT = false>
__global__ __launch_bounds__(PK_FD) void gz_pack_fill_kernel(GzPackArgs A)
{
    // documents d0 .. d0 + PK_FD + PK_AL / 2 - 1: a cell less than PK_AL behind document d0 + PK_FD's first can belong to PK_AL / 2
    // documents further (the shortest has 2 cells); one more entry so that "the next document's first cell" always exists
    constexpr int ND = PK_FD + PK_AL / 2 + 1;
    __shared__ int64_t P[ND], src[ND];                                     // the document's first cell in the flat output, its body in ids
    __shared__ int32_t ln[ND], sg[ND];                                     // its len, its index within its row
    int64_t n_pack;
    if constexpr (FIT) n_pack = A.fit_rows;
    else {
        n_pack = *A.total;                                                 // (from the maps' pass on this stream: the host has not seen it yet)
        if (n_pack > A.capacity) return;                                   // the caller's arrays are too small: nothing is written, the host reports it
    }
    const int64_t d0 = (int64_t)blockIdx.x * PK_FD, L = A.max_len, end = n_pack * L;
    for (int k = threadIdx.x; k < ND; k += PK_FD) {
        const int64_t d = d0 + k;
        int64_t p = end, s = 0;
        int32_t l = 0, q = 0;
        if constexpr (FIT) {
            if (d < A.n_rows) {
                const int32_t doc = A.row_docs[d], row = A.doc_row[doc];
                p = row * L + A.doc_col[doc];
                l = A.doc_len[doc];
                s = A.row_off[doc] + A.skip_front;
                q = (int32_t)(d - A.pack_off[row]);
            }
        } else if (d < A.n_rows) {
            const int32_t row = A.doc_row[d];
            const int64_t head = A.pack_off[row], at = A.seg_off[d];
            const int32_t col = (int32_t)(at - A.seg_off[head]);
            if (k < PK_FD) A.doc_col[d] = col;                             // (the col pass, which a call that fills leaves to this one)
            p = row * L + col;
            l = (int32_t)(A.seg_off[d + 1] - at);
            s = A.row_off[d] + A.skip_front;
            q = (int32_t)(d - head);
        }
        P[k] = p; src[k] = s; ln[k] = l; sg[k] = q;
    }
    __syncthreads();
    // this workgroup's cells: from its first document's first cell to the next workgroup's, both rounded up to PK_AL cells (the
    // cells in between belong to the workgroup before) and cut at the end of the last row, where the last workgroup stops
    const int64_t r0 = (P[0] + PK_AL - 1) / PK_AL * PK_AL, r1 = (P[PK_FD] + PK_AL - 1) / PK_AL * PK_AL;
    const int64_t x0 = r0 < end ? r0 : end, x1 = r1 < end ? r1 : end;                       // (P beyond the last document = end)
    for (int64_t x = x0 + (int64_t)threadIdx.x * U; x < x1; x += (int64_t)PK_FD * U) {
        int lo = 0, hi = ND - 2;                                           // the last document with P <= x (x0 >= P[0])
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (P[mid] <= x) lo = mid; else hi = mid - 1;
        }
        int k = lo;
        int32_t pos[U], len[U], seg[U];
        int64_t at[U];
        int64_t safe = -1;
#pragma unroll
        for (int u = 0; u < U; ++u) {                                      // (a unit may hold cells of up to three documents)
            const int64_t xc = x + u;
            while (xc >= P[k + 1]) ++k;
            pos[u] = (int32_t)(xc - P[k]); len[u] = ln[k]; seg[u] = sg[k];
            at[u] = pos[u] >= 1 && pos[u] < len[u] - 1 ? src[k] + pos[u] - 1 : -1;
            if (safe < 0) safe = at[u];
        }
        int32_t tok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) tok[u] = 0;
        if (safe >= 0) {                                                   // the unit holds body cells: all its loads under ONE branch, each at a body cell
#pragma unroll
            for (int u = 0; u < U; ++u) tok[u] = A.ids[at[u] >= 0 ? at[u] : safe];
        }
        int32_t v[U], m[U], sv[U], pv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool real = pos[u] < len[u];                             // (beyond the row's last document: the tail)
            v[u] = !real ? A.pad_id : pos[u] == 0 ? A.bos_id : pos[u] == len[u] - 1 ? A.eos_id : tok[u];
            m[u] = v[u] != A.pad_id ? 1 : 0;
            sv[u] = real ? seg[u] + 1 : 0;
            pv[u] = real ? pos[u] : 0;
        }
        if constexpr (U == 4) {
            nt_store4(A.out_ids + x, v[0], v[1], v[2], v[3]);
            if (A.out_mask) nt_store4(A.out_mask + x, m[0], m[1], m[2], m[3]);
            if (A.out_seg) nt_store4(A.out_seg + x, sv[0], sv[1], sv[2], sv[3]);
            if (A.out_pos) nt_store4(A.out_pos + x, pv[0], pv[1], pv[2], pv[3]);
        } else {
            A.out_ids[x] = v[0];
            if (A.out_mask) A.out_mask[x] = m[0];
            if (A.out_seg) A.out_seg[x] = sv[0];
            if (A.out_pos) A.out_pos[x] = pv[0];
        }
    }
}
