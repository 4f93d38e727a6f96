// gz_align.inc -- word spans, word ids and aligned token labels for token classification (included by gz_kernels.hip after
// gz_pipeline.inc, whose is_ws1 / is_ws2 / is_ws3 are the word rule: nothing of it is restated here).
//
// Words of a document: the matches of "\S+\n?" with Unicode whitespace as str.isspace (tokenize.py:106); a document boundary
// ends a word.  A byte is WHITE when it lies inside a whitespace code point (the three byte patterns), bytes outside the
// packed text read as spaces.  With ds(p) = "a document starts at byte p, or p is the end of the text":
//   a word STARTS at p        p is not white and (p - 1 is white or ds(p))
//   a word's LAST byte is q   q is not white and (q + 1 is white or ds(q + 1))
// Both come from the same two predicates, so starts and last bytes pair up one to one whatever the bytes are; for structurally valid
// UTF-8 the words are the encoder's.  The glued line feed is white: it is never inside a span.
//
// Spans, no carry between tiles.  A granule is 16 bytes of the packed text (one lane), a block 256 granules.
//   gz_span_scan_kernel   every granule: start bits, last-byte bits, lead bits (bytes that are not 10xxxxxx); the block's exclusive
//                         scan of (starts, leads), packed 16 + 16 bits -> gran[g]; the block's totals -> blk_s, blk_l
//   (scan64 twice)        -> base_s, base_l: starts and leads before every block; base_s[nblk] = W
//   gz_span_doc_kernel    one thread a document (and one for the end): the scan AT its first byte -> word_off[d], lead0[d]; and
//                         blk_doc[b] = d for the blocks whose first byte lies in document d
//   gz_span_write_kernel  every granule with an event: the document of its first event by binary search in text_off between
//                         blk_doc of its block and of the next one, then along;
//                         a start at p is word s(p) and writes span[s(p)][0]; a last byte at q is word s(q + 1) - 1 and writes
//                         span[..][1] -- the same index from either side, so a word across three tiles needs no special path.
//   code point index = leads since the document's first byte.
//
// Align.  tok_off = the exclusive scan of the piece counts (32 bits, wrapping: see below), so C_j = tok_off[w0 + j] - tok_off[w0].
// Rows of up to 1 024 cells: a block takes several rows, marks in an LDS bitmap the cell where each word of a row starts (one
// contiguous load of tok_off a word) and every cell counts the bits up to its own.  Longer rows: one thread a cell, the word of body
// token t by binary search in tok_off over [w0, min(w1 - 1, w0 + t)] (a word has at least one piece, so word j holds no token before
// j).  Every cell is written once.
//
// Span labels.  owner[w] = smallest mark index overlapping word w (atomicMin over the words a mark covers, found by two binary
// searches in the document's sorted spans), then one pass a word, then the first word of every document (no word before it).

namespace {

constexpr int AL_BLK = 4096;                  // bytes per block of the span kernels: 256 lanes x 16
constexpr uint32_t AL_NONE = 0xFFFFFFFFu;     // a word no mark overlaps

struct AlGran { uint32_t st, el, lead; };

// granule g of the packed text tb[0 .. B): bit i of st / el / lead speaks of byte 16 g + i.  Reads nothing outside [0, B).
__device__ __forceinline__ AlGran al_classify(const uint8_t* __restrict__ tb, int64_t B, const uint32_t* __restrict__ brk, int64_t g)
{
    typedef unsigned __attribute__((ext_vector_type(4), aligned(1))) v4u_u;
    typedef unsigned __attribute__((aligned(1))) u32_u;
    const int64_t p0 = g * 16;
    uint32_t w[6];                                                       // bytes p0 - 4 .. p0 + 19, byte k of the window = byte p0 - 4 + k
    if (p0 >= 4 && p0 + 20 <= B) {
        w[0] = *reinterpret_cast<const u32_u*>(tb + p0 - 4);
        const auto v = *reinterpret_cast<const v4u_u*>(tb + p0);
        w[1] = v.x; w[2] = v.y; w[3] = v.z; w[4] = v.w;
        w[5] = *reinterpret_cast<const u32_u*>(tb + p0 + 16);
    } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            uint32_t x = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = p0 - 4 + 4 * q + k;
                x |= ((i >= 0 && i < B) ? (uint32_t)tb[i] : 0x20u) << (8 * k);
            }
            w[q] = x;
        }
    }
    auto byte = [&](int k) -> uint32_t { return (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu; };
    uint32_t ws = 0, lead = 0;
#pragma unroll
    for (int k = 0; k < 24; ++k) ws |= (uint32_t)is_ws1(byte(k)) << k;
#pragma unroll
    for (int i = 0; i < 16; ++i) lead |= (uint32_t)((byte(i + 4) & 0xC0u) != 0x80u) << i;
    if ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5]) & 0x80808080u) {      // multi-byte whitespace: C2 xx, E1 / E2 / E3 xx xx
#pragma unroll
        for (int k = 0; k < 22; ++k) {
            const uint32_t b = byte(k);
            if (b == 0xC2u || (b >= 0xE1u && b <= 0xE3u)) {
                if (is_ws2(b, byte(k + 1))) ws |= 3u << k;
                if (is_ws3(b, byte(k + 1), byte(k + 2))) ws |= 7u << k;
            }
        }
    }
    // ds: bit i = a document starts at p0 + i, or p0 + i is the end of the text (i = 0 .. 16)
    const uint32_t* const bw = brk + (p0 >> 5);
    const uint64_t bb = (uint64_t)bw[0] | ((uint64_t)bw[1] << 32);
    uint32_t ds = (uint32_t)(bb >> (p0 & 31)) & 0x1FFFFu;
    if (p0 == 0) ds |= 1u;
    const int64_t left = B - p0;                                          // > 0
    if (left <= 16) ds |= 1u << (int)left;
    const uint32_t inb = left >= 16 ? 0xFFFFu : (1u << (int)left) - 1u;
    const uint32_t nw = (~ws >> 4) & inb, pw = (ws >> 3) & 0xFFFFu, xw = (ws >> 5) & 0xFFFFu;
    AlGran c;
    c.st = nw & (pw | ds) & 0xFFFFu;
    c.el = nw & (xw | (ds >> 1)) & 0xFFFFu;
    c.lead = lead & inb;
    return c;
}

}  // namespace

__global__ __launch_bounds__(256) void gz_span_scan_kernel(GzSpanArgs A)
{
    __shared__ uint32_t wsum[4];
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t v = 0;
    if (g * 16 < A.B) {
        const AlGran c = al_classify(A.text + A.text_off[0], A.B, A.brk, g);
        v = (uint32_t)__popc(c.st) | ((uint32_t)__popc(c.lead) << 16);           // (a block holds at most 2 048 starts and 4 096 leads)
    }
    int tot;
    const int ex = wave_excl_sum((int)v, lane, tot);
    if (lane == 0) wsum[wv] = (uint32_t)tot;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t s = wsum[k]; if (k < wv) pre += s; all += s; }
    A.gran[g] = (uint32_t)ex + pre;
    if (threadIdx.x == 0) { A.blk_s[blockIdx.x] = (int64_t)(all & 0xFFFFu); A.blk_l[blockIdx.x] = (int64_t)(all >> 16); }
}

__global__ __launch_bounds__(256) void gz_span_doc_kernel(GzSpanArgs A)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d > A.n_docs) return;
    const int64_t off0 = A.text_off[0];
    int64_t p = A.text_off[d] - off0;
    if (p < 0) p = 0;
    if (d < A.n_docs && A.text_off[d + 1] - A.text_off[d] >= ((int64_t)1 << 31)) atomicOr(A.too_long, 1u);
    const int64_t nblk = (A.B + AL_BLK - 1) / AL_BLK;
    int64_t s, l;
    if (p >= A.B) { s = A.base_s[nblk]; l = A.base_l[nblk]; }
    else {
        const int64_t g = p >> 4;
        const uint32_t u = A.gran[g], m = (1u << (int)(p & 15)) - 1u;
        const AlGran c = al_classify(A.text + off0, A.B, A.brk, g);
        s = A.base_s[g >> 8] + (int64_t)(u & 0xFFFFu) + __popc(c.st & m);
        l = A.base_l[g >> 8] + (int64_t)(u >> 16) + __popc(c.lead & m);
    }
    A.word_off[d] = s;
    A.lead0[d] = l;
    // the document of every block's first byte, for the write pass's search (a document shorter than a block owns one block or none)
    if (d == A.n_docs) { A.blk_doc[nblk] = A.n_docs - 1; return; }
    const int64_t e = A.text_off[d + 1] - off0;
    for (int64_t b = (p + AL_BLK - 1) / AL_BLK; b < nblk && b * AL_BLK < e; ++b) A.blk_doc[b] = d;
}

__global__ __launch_bounds__(256) void gz_span_write_kernel(GzSpanArgs A)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, p0 = g * 16;
    if (p0 >= A.B) return;
    const int64_t off0 = A.text_off[0];
    const AlGran c = al_classify(A.text + off0, A.B, A.brk, g);
    uint32_t ev = c.st | c.el;
    if (!ev) return;
    const uint32_t u = A.gran[g];
    const int64_t bs = A.base_s[g >> 8] + (int64_t)(u & 0xFFFFu), bl = A.base_l[g >> 8] + (int64_t)(u >> 16);
    // the document of the first event: the last d with text_off[d] - off0 <= p (behind any empty documents that start there)
    int64_t lo = A.blk_doc[g >> 8], hi = A.blk_doc[(g >> 8) + 1];             // between the documents of this block's and the next one's first byte
    lo = lo < 0 ? 0 : lo > A.n_docs - 1 ? A.n_docs - 1 : lo;                  // (offsets the device form could not read: inside the array all the same)
    hi = hi < lo ? lo : hi > A.n_docs - 1 ? A.n_docs - 1 : hi;
    {
        const int64_t p = p0 + __ffs(ev) - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (A.text_off[mid] - off0 <= p) lo = mid; else hi = mid - 1;
        }
    }
    int64_t d = lo, dstart = A.text_off[d] - off0, dnext = A.text_off[d + 1] - off0;
    for (; ev; ev &= ev - 1) {
        const int i = __ffs(ev) - 1;
        const int64_t p = p0 + i;
        while (dnext <= p && d + 1 < A.n_docs) { ++d; dstart = dnext; dnext = A.text_off[d + 1] - off0; }
        const uint32_t m = (1u << i) - 1u, is_st = (c.st >> i) & 1u, is_ld = (c.lead >> i) & 1u;
        const int64_t sb = bs + __popc(c.st & m), lb = bl + __popc(c.lead & m);
        if (is_st) {
            const int64_t v = A.unit ? p - dstart : lb - A.lead0[d];
            if ((uint64_t)sb < (uint64_t)A.n_words) A.span[2 * sb] = (int32_t)v;
        }
        if ((c.el >> i) & 1u) {
            const int64_t wi = sb + is_st - 1;
            const int64_t v = A.unit ? p + 1 - dstart : lb + is_ld - A.lead0[d];
            if ((uint64_t)wi < (uint64_t)A.n_words) A.span[2 * wi + 1] = (int32_t)v;
        }
    }
}

// ---- align -----------------------------------------------------------------------------------------------------------
// tok_off: the exclusive scan of the piece counts in 32 bits, wrapping.  Only differences inside one document are ever taken, and a
// document holds fewer than 2^31 tokens (one a byte at the most), so they are exact.  The scan is gz_scan32x_* of gz_kernels.hip; its
// first step is restated here because the counts start at counts[word_off[0]], an index only the device knows.
__global__ __launch_bounds__(1024) void gz_align_scan_local_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ word_off, int64_t n,
                                                                   uint32_t* __restrict__ out /* n+1 */)
{
    __shared__ uint32_t wsum[16];
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const int32_t* const in = counts + word_off[0];
    const int64_t b0 = (int64_t)blockIdx.x * SC32, i = b0 + 4 * (int64_t)threadIdx.x;
    uint32_t a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = i + k < n ? (uint32_t)in[i + k] : 0u;
    uint32_t x = a[0] + a[1] + a[2] + a[3];
    const uint32_t mine = x;
#pragma unroll
    for (int dlt = 1; dlt < WAVE; dlt <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, dlt, WAVE);
        if (lane >= dlt) x += y;
    }
    if (lane == WAVE - 1) wsum[wv] = x;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const uint32_t w = wsum[k]; if (k < wv) pre += w; all += w; }
    uint32_t e = pre + x - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i + k <= n && i + k != b0) out[i + k] = e;           // (slot b0 belongs to the block before: its total; block 0: zero)
        e += a[k];
    }
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) out[0] = 0;
        if (b0 + SC32 <= n) out[b0 + SC32] = all;
    }
}

namespace {
// a row's document and chunk: w0, w1 = its words (inside [0, n_words]: offsets the device form could not read stay inside the arrays),
// s = its start, n = its chunk length
struct AlRow { int64_t w0, w1, s; int n; };
__device__ __forceinline__ AlRow al_row(const GzAlignArgs& A, int64_t r, int64_t wbase)
{
    AlRow R;
    const int64_t d = A.row_doc ? (int64_t)A.row_doc[r] : r;
    R.s = A.row_start ? (int64_t)A.row_start[r] : 0;
    if (R.s < 0) R.s = 0;
    R.w0 = R.w1 = 0;
    if (d >= 0 && d < A.n_docs) { R.w0 = A.word_off[d] - wbase; R.w1 = A.word_off[d + 1] - wbase; }
    if (R.w0 < 0) R.w0 = 0;
    if (R.w0 > A.n_words) R.w0 = A.n_words;
    if (R.w1 > A.n_words) R.w1 = A.n_words;
    if (R.w1 < R.w0) R.w1 = R.w0;
    const int64_t left = (int64_t)(A.tok_off[R.w1] - A.tok_off[R.w0]) - R.s, room = (int64_t)A.max_len - 2;
    R.n = left <= 0 ? 0 : left < room ? (int)left : (int)room;
    return R;
}
// the last word of [w0, w1) that starts at or before body token tt of its document (w0 < w1, tt < T)
__device__ __forceinline__ int64_t al_word_of(const uint32_t* __restrict__ tok_off, int64_t w0, int64_t w1, uint32_t tt)
{
    const uint32_t t0 = tok_off[w0];
    int64_t lo = w0, hi = w0 + (int64_t)tt < w1 - 1 ? w0 + (int64_t)tt : w1 - 1;      // (a word has a piece at least: word j holds no token before j)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (tok_off[mid] - t0 <= tt) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int32_t al_label(const GzAlignArgs& A, int32_t v, bool first)
{
    if (first || A.continuation == 1) return v;
    if (A.continuation == 2) return (v >= 0 && v < A.n_map) ? A.cont_map[v] : v;
    return A.ignore_index;
}
}  // namespace

// Any max_len: one thread a cell, the word of its token by binary search.
__global__ __launch_bounds__(256) void gz_align_rows_kernel(GzAlignArgs A)
{
    const int64_t L = A.max_len, cells = A.n_rows * L, stride = (int64_t)gridDim.x * 256;
    const int64_t wbase = A.word_off[0];
    for (int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x; cell < cells; cell += stride) {
        const int64_t r = cell / L;
        const int k = (int)(cell - r * L);
        const AlRow R = al_row(A, r, wbase);
        if (k == 0 && A.n_real) A.n_real[r] = R.n + 2;
        int32_t wid = -1, lab = A.ignore_index;
        if (k >= 1 && k <= R.n) {
            const uint32_t tt = (uint32_t)(R.s + k - 1);
            const int64_t j = al_word_of(A.tok_off, R.w0, R.w1, tt);
            wid = (int32_t)(j - R.w0);
            if (A.labels) lab = al_label(A, A.word_labels[wbase + j], A.tok_off[j] - A.tok_off[R.w0] == tt);
        }
        if (A.word_ids) A.word_ids[cell] = wid;
        if (A.labels) A.labels[cell] = lab;
    }
}

// max_len <= AL_LMAX: a block takes A.rows_per_block rows.  One thread a row finds the row's first word j0 (no search where start is 0);
// one thread a (row, slot) loads tok_off[j0 + slot] -- contiguous -- and sets the bit of the cell where that word starts in the row's
// bitmap in LDS; one thread a cell then counts the bits up to its own: its word is j0 + that count (less one where the row begins at a
// word's start), and its own bit says "first piece".  One dependent load a cell in place of a search.
constexpr int AL_LMAX = 1024, AL_RMAX = 64, AL_BITS = 256;            // rows_per_block * ceil(max_len / 32) <= AL_BITS
template <int U>
__global__ __launch_bounds__(256) void gz_align_rows_lds_kernel(GzAlignArgs A)
{
    __shared__ uint32_t bits[AL_BITS];
    __shared__ int64_t sh_j0[AL_RMAX], sh_w0[AL_RMAX], sh_w1[AL_RMAX];
    __shared__ uint32_t sh_base[AL_RMAX];
    __shared__ int sh_n[AL_RMAX];
    const int L = A.max_len, RB = A.rows_per_block, wpr = (L + 31) >> 5, tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * RB, wbase = A.word_off[0];
    for (int i = tid; i < RB * wpr; i += 256) bits[i] = 0u;
    if (tid < RB) {
        const int64_t r = r0 + tid;
        int n = -1;
        if (r < A.n_rows) {
            const AlRow R = al_row(A, r, wbase);
            n = R.n;
            if (A.n_real) A.n_real[r] = n + 2;
            sh_w0[tid] = R.w0; sh_w1[tid] = R.w1;
            sh_base[tid] = A.tok_off[R.w0] + (uint32_t)R.s;
            sh_j0[tid] = n > 0 && R.s > 0 ? al_word_of(A.tok_off, R.w0, R.w1, (uint32_t)R.s) : R.w0;
        }
        sh_n[tid] = n;
    }
    __syncthreads();
    const int total = RB * L;
    for (int i = tid; i < total; i += 256) {                                // slot: the words j0 .. j0 + n start at or behind the row's first cell
        const int row = i / L, slot = i - row * L, n = sh_n[row];
        const int64_t j = sh_j0[row] + slot;
        if (slot <= n && n > 0 && j < sh_w1[row]) {
            const int32_t rel = (int32_t)(A.tok_off[j] - sh_base[row]);
            if (rel >= 0 && rel < n) atomicOr(&bits[row * wpr + (rel >> 5)], 1u << (rel & 31));
        }
    }
    __syncthreads();
    // U cells a lane and store: 4 (rows and base pointers 16-byte aligned: one streaming 16-byte store an array) or 1 (any max_len)
    const int Q = L / U, units = RB * Q;
    for (int i = tid; i < units; i += 256) {
        const int row = i / Q, k0 = (i - row * Q) * U, n = sh_n[row];
        if (n < 0) continue;                                                // (past the last row)
        const uint32_t* const b = bits + row * wpr;
        int32_t wid[U], lab[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u;
            wid[u] = -1; lab[u] = A.ignore_index;
            if (k >= 1 && k <= n) {
                const int p = k - 1;
                int cnt = __popc(b[p >> 5] & (0xFFFFFFFFu >> (31 - (p & 31))));
                for (int q = 0; q < (p >> 5); ++q) cnt += __popc(b[q]);
                const int64_t j = sh_j0[row] + cnt - (int)(b[0] & 1u);
                wid[u] = (int32_t)(j - sh_w0[row]);
                if (A.labels) lab[u] = al_label(A, A.word_labels[wbase + j], (b[p >> 5] >> (p & 31)) & 1u);
            }
        }
        const int64_t cell = (r0 + row) * (int64_t)L + k0;
        if constexpr (U == 4) {
            if (A.word_ids) nt_store4(A.word_ids + cell, wid[0], wid[1], wid[2], wid[3]);
            if (A.labels) nt_store4(A.labels + cell, lab[0], lab[1], lab[2], lab[3]);
        } else {
            if (A.word_ids) A.word_ids[cell] = wid[0];
            if (A.labels) A.labels[cell] = lab[0];
        }
    }
}

// ---- span labels -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gz_spanlab_mark_kernel(GzSpanLabArgs A)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= A.n_marks) return;
    const int64_t mo0 = A.mark_off[0], wbase = A.word_off[0];
    int64_t lo = 0, hi = A.n_docs - 1;                                        // the last d with mark_off[d] - mo0 <= m
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (A.mark_off[mid] - mo0 <= m) lo = mid; else hi = mid - 1;
    }
    int64_t w0 = A.word_off[lo] - wbase, w1 = A.word_off[lo + 1] - wbase;
    if (w0 < 0) w0 = 0;                                                       // (as in gz_align_rows_kernel)
    if (w1 > A.n_words) w1 = A.n_words;
    const int32_t* const mk = A.marks + 3 * (mo0 + m);
    const int32_t b = mk[0], e = mk[1];
    const int32_t* const sp = A.span + 2 * wbase;
    int64_t f = w1, l = w0;
    if (e > b && w1 > w0) {
        int64_t a = w0, z = w1;                                               // f: the first word with end > b
        while (a < z) { const int64_t mid = (a + z) >> 1; if (sp[2 * mid + 1] > b) z = mid; else a = mid + 1; }
        f = a;
        a = w0; z = w1;                                                       // l: the first word with begin >= e
        while (a < z) { const int64_t mid = (a + z) >> 1; if (sp[2 * mid] >= e) z = mid; else a = mid + 1; }
        l = a;
    }
    const bool any = f < l;
    if (A.mark_words) { A.mark_words[2 * m] = any ? (int32_t)(f - w0) : -1; A.mark_words[2 * m + 1] = any ? (int32_t)(l - w0) : -1; }
    if (any && A.owner) for (int64_t j = f; j < l; ++j) atomicMin(&A.owner[j], (uint32_t)m);
}

__global__ __launch_bounds__(256) void gz_spanlab_word_kernel(GzSpanLabArgs A)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    const uint32_t o = A.owner[w];
    int32_t v;
    if (o == AL_NONE) v = A.scheme ? 0 : A.outside;
    else {
        const int32_t lab = A.marks[3 * (A.mark_off[0] + (int64_t)o) + 2];
        if (!A.scheme) v = lab;
        else v = (w == 0 || A.owner[w - 1] != o) ? 2 * lab + 1 : 2 * lab + 2;
    }
    A.word_labels[A.word_off[0] + w] = v;
}

// BIO: the first word of a document has no word before it
__global__ __launch_bounds__(256) void gz_spanlab_first_kernel(GzSpanLabArgs A)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= A.n_docs) return;
    const int64_t wbase = A.word_off[0], w0 = A.word_off[d] - wbase, w1 = A.word_off[d + 1] - wbase;
    if (w0 < 0 || w0 >= w1 || w0 >= A.n_words) return;
    const uint32_t o = A.owner[w0];
    if (o != AL_NONE) A.word_labels[wbase + w0] = 2 * A.marks[3 * (A.mark_off[0] + (int64_t)o) + 2] + 1;
}
