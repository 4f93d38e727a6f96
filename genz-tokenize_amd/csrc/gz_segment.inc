// gz_segment.inc -- Vietnamese word segmentation by lexicon: minimum-cost segmentation of every document's tokens into lexicon words
// (included by gz_kernels.hip behind gz_bm25.inc, whose word front -- count, scan, words -- makes the whitespace pieces this file
// starts from; nothing of the splitter is restated here).
//
// THE RULE (include/genz_tokenize.h, "segment").  TOKENS: a whitespace piece, or with split_punct every ASCII punctuation character but
// '_' of its leading and of its trailing run, and the core between them.  CANDIDATES: k = 1..K consecutive tokens of one document
// joined by '_', case-folded by gz_seg_fold, that equal a lexicon entry byte for byte; the cost is the entry's; a single token that is
// no entry costs unk_cost.  CHOICE: best[0] = 0, best[i] = min over k of best[i - k] + cost(i - k, i), the largest k among equal
// minima; the back-trace from the document's end glues the tokens of a word.
//
// gz_seg_piece_kernel<WRITE>   a lane a piece: the piece's tokens counted, and after the scan of the counts written (first byte, bytes,
//                              document)
// gz_seg_docs_kernel           a lane a document: its output bytes = its tokens' bytes + a separator between two, its n_tokens
// gz_seg_cand_kernel<LDS>      a lane a token START i, a trip GZ_SEG_TILE starts a workgroup.  The trip's token records (with the K - 1
//                              behind it) and the bytes they cover come through LDS once; a span longer than GZ_SEG_LDS_TEXT is read
//                              from memory instead.  ONE 64-bit hash is extended token by token for k = 1..K and finished after each;
//                              it stops at the document's end and where the key outgrows the longest entry.  LDS: the lexicon's bit
//                              filter over the hashes (2^20 bits, 128 KB) is copied into LDS once by every workgroup of a persistent
//                              grid, and a key whose bit is clear is answered there.  A survivor probes the open-addressing table
//                              (hash, cost, bytes) and compares its bytes with the entry's.  The hash decides where to look, never
//                              whether two keys are equal.  -> cand[i][k - 1], reach[i]
// gz_seg_mark_kernel           a lane a token b: the boundary before it is CLOSED when b starts its document or no multi-token
//                              candidate covers it (i + reach[i] <= b for the K - 1 starts before it).  No optimal segmentation
//                              crosses a closed boundary, so the recurrence, ties included, restarts there.  The closed tokens are
//                              compacted by ballot and prefix, one atomicAdd a wave (their order in the list is never read)
// gz_seg_walk_kernel           a lane a STRETCH (closed token to the next): the K-wide ring of best values stays in registers as
//                              int64 relative to the stretch start -- a stretch of n tokens sums at most n (2^24 - 1) < 2^56, so
//                              nothing is renormalised -- one byte of chosen k a token goes to memory, and the lane's back-trace
//                              writes join.  Words, known words and cost meet per document by 64-bit integer atomicAdd.
// gz_seg_emit_kernel           GZ_SEG_EMIT_LANES lanes a token copy its bytes to out_off[d] + the document's token bytes before it +
//                              the tokens before it, and '_' or ' ' behind it from join; nothing behind a document's last token
// Vector stores and integer vector atomics only; no result depends on the order in which the atomics land (sums, a maximum, and a
// list whose order is not read).
// Bounds: a token index is below n_tokens before anything of it is read; a record index of a trip is below GZ_SEG_TILE + K - 1; a
// token's bytes lie inside its piece, a piece inside its document, a document inside [lo, hi] (bm_doc_len); an LDS text index is below
// the staged span by the same containment; a table slot is masked; an entry's bytes are read only after its length equalled the
// key's; an output position is below out_off[d + 1] <= capacity (the host checked the total before the launch).

namespace {
constexpr int SEG_THREADS = GZ_SEG_TILE;                              // 16 waves: with the filter in LDS a compute unit holds one workgroup
constexpr int SEG_RECS = GZ_SEG_TILE + GZ_SEG_MAX_SYLLABLES;          // token records of a trip (its starts and the K - 1 tokens behind them)
constexpr uint32_t SEG_FILTER_WORDS = 1u << (GZ_SEG_FILTER_BITS - 5);
constexpr size_t SEG_LDS_BYTES = (size_t)3 * SEG_RECS * 4 + 16 + GZ_SEG_LDS_TEXT;     // records, span, text: what a trip keeps in LDS beside the filter
static_assert(SEG_LDS_BYTES + (size_t)SEG_FILTER_WORDS * 4 <= (160u << 10), "the candidate kernel's LDS passes a compute unit's 160 KB");

// the tokens of piece [s, e): its leading punctuation run, and the trailing one when a core is left
__device__ __forceinline__ void seg_piece_runs(const uint8_t* tb, int64_t s, int64_t e, bool split, uint32_t& lead, uint32_t& trail, bool& core)
{
    lead = trail = 0u;
    core = true;
    if (!split) return;
    const int64_t n = e - s;
    while ((int64_t)lead < n && gz_seg_punct(tb[s + lead])) ++lead;
    if ((int64_t)lead == n) { core = false; return; }
    while (gz_seg_punct(tb[e - 1 - trail])) ++trail;                   // (stops at the core's last byte at the latest)
}

// the folded bytes of the key of tokens j0 .. j0 + k - 1 (records in LDS) against entry bytes eb[0 .. n)
template <class Src>
__device__ __forceinline__ bool seg_equal(const Src src, const uint32_t* rs, const uint32_t* rl, int j0, int k, bool fold, const uint8_t* eb)
{
    uint32_t p1 = 0u, p2 = 0u, at = 0u;
    for (int q = 0; q < k; ++q) {
        if (q) { if (eb[at++] != 0x5Fu) return false; p2 = p1; p1 = 0x5Fu; }
        const uint32_t s = rs[j0 + q], L = rl[j0 + q];
        for (uint32_t b = 0; b < L; ++b) {
            const uint32_t c = src[s + b], f = fold ? gz_seg_fold(p2, p1, c) : c;
            if (eb[at++] != f) return false;
            p2 = p1; p1 = c;
        }
    }
    return true;
}

// the cost of the entry whose bytes are the key's, or GZ_SEG_NONE
template <class Src>
__device__ __forceinline__ uint32_t seg_probe(const GzSegArgs& A, const Src src, const uint32_t* rs, const uint32_t* rl, int j0, int k, unsigned long long hk,
                                              uint32_t nbytes)
{
    const unsigned long long key = hk | (1ull << 63);
    unsigned long long slot = gz_seg_slot(hk) & A.tmask;
    for (unsigned long long n = 0; n <= A.tmask; ++n, slot = (slot + 1ull) & A.tmask) {
        const GzSegSlot e = A.tab[slot];
        if (e.key == 0ull) return GZ_SEG_NONE;
        if (e.key == key && e.len == nbytes && seg_equal(src, rs, rl, j0, k, A.fold_case != 0, A.ebytes + e.off)) return e.cost;
    }
    return GZ_SEG_NONE;
}

// token start j0 of the trip (token t): its K candidates and its reach
template <bool LDS, class Src>
__device__ __forceinline__ void seg_start(const GzSegArgs& A, const Src src, const uint32_t* rs, const uint32_t* rl, const uint32_t* rd, const uint32_t* filter,
                                          int j0, int64_t t)
{
    const uint32_t doc = rd[j0];
    const bool fold = A.fold_case != 0;
    unsigned long long h = GZ_SEG_HASH_SEED;
    uint32_t nbytes = 0u, p1 = 0u, p2 = 0u, reach = 1u;
    uint32_t* const out = A.cand + (size_t)t * (size_t)A.K;
    int k = 1;
    for (; k <= A.K; ++k) {
        const int j = j0 + k - 1;
        if (rd[j] != doc) break;                                      // (the document's end; a record behind the last token has no document)
        const uint32_t s = rs[j], L = rl[j];
        if ((unsigned long long)nbytes + L + (k > 1 ? 1u : 0u) > A.max_len) break;     // (no entry is that long: nor is any longer key)
        if (k > 1) { h = gz_seg_hash_byte(h, 0x5Fu); ++nbytes; p2 = p1; p1 = 0x5Fu; }
        for (uint32_t b = 0; b < L; ++b) {
            const uint32_t c = src[s + b];
            h = gz_seg_hash_byte(h, fold ? gz_seg_fold(p2, p1, c) : c);
            p2 = p1; p1 = c;
        }
        nbytes += L;
        const unsigned long long hk = gz_seg_hash_fin(h, nbytes) & A.hmask;
        uint32_t cost = GZ_SEG_NONE;
        const uint32_t bit = (uint32_t)hk & ((1u << GZ_SEG_FILTER_BITS) - 1u);
        if (!LDS || ((filter[bit >> 5] >> (bit & 31u)) & 1u)) cost = seg_probe(A, src, rs, rl, j0, k, hk, nbytes);
        out[k - 1] = cost;
        if (cost != GZ_SEG_NONE && k > 1) reach = (uint32_t)k;
    }
    for (; k <= A.K; ++k) out[k - 1] = GZ_SEG_NONE;
    A.reach[t] = (uint8_t)reach;
}

// text read through LDS: byte p of the text (relative to lo) sits at buf[p - first]
struct SegLdsText {
    const uint8_t* buf; uint32_t first;
    __device__ __forceinline__ uint32_t operator[](uint32_t p) const { return buf[p - first]; }
};
struct SegMemText {
    const uint8_t* base;
    __device__ __forceinline__ uint32_t operator[](uint32_t p) const { return base[p]; }
};
}  // namespace

template <bool WRITE>
__global__ __launch_bounds__(256) void gz_seg_piece_kernel(GzSegArgs A)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.n_pieces) return;
    const int64_t s = A.wstart[p], e = A.wend[p];
    if (s < A.lo || e <= s || e > A.hi) {                             // (the word front never gives such a piece)
        if (!WRITE) A.ptc[p] = 0u;
        return;
    }
    uint32_t lead, trail;
    bool core;
    seg_piece_runs(A.tb, s, e, A.split_punct != 0, lead, trail, core);
    const uint32_t n = lead + trail + (core ? 1u : 0u);
    if (!WRITE) { A.ptc[p] = n; return; }
    const uint32_t t0 = A.ptoff[p], doc = A.wdoc[p], rel = (uint32_t)(s - A.lo), len = (uint32_t)(e - s);
    if (!GZ_CHK(921, (uint64_t)t0 + n, (uint64_t)A.n_tokens + 1) || (int64_t)t0 + n > A.n_tokens) return;
    uint32_t t = t0;
    for (uint32_t i = 0; i < lead; ++i, ++t) { A.tstart[t] = rel + i; A.tlen[t] = 1u; A.tdoc[t] = doc; }
    if (core) { A.tstart[t] = rel + lead; A.tlen[t] = len - lead - trail; A.tdoc[t] = doc; ++t; }
    for (uint32_t i = 0; i < trail; ++i, ++t) { A.tstart[t] = rel + len - trail + i; A.tlen[t] = 1u; A.tdoc[t] = doc; }
}

__global__ __launch_bounds__(256) void gz_seg_docs_kernel(GzSegArgs A)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= A.n_docs) return;
    const uint32_t t0 = A.ptoff[A.woff[d]], t1 = A.ptoff[A.woff[d + 1]], n = t1 - t0;
    A.doclen[d] = (int64_t)(A.tlsum[t1] - A.tlsum[t0]) + (n ? (int64_t)n - 1 : 0);
    if (A.stats) {
        A.stats[4 * d] = n;
        A.stats[4 * d + 1] = A.stats[4 * d + 2] = A.stats[4 * d + 3] = 0ull;
    }
}

template <bool LDS>
__global__ __launch_bounds__(SEG_THREADS) void gz_seg_cand_kernel(GzSegArgs A, int64_t n_trips)
{
    // LDS, all of it dynamic (a static word beside it would count against the 160 KB the attribute asks for): [the filter] the records'
    // starts, bytes and documents; the trip's span; the text
    extern __shared__ __attribute__((aligned(16))) uint32_t seg_lds[];
    uint32_t* const filter = seg_lds;
    uint32_t* const rs = seg_lds + (LDS ? SEG_FILTER_WORDS : 0u);
    uint32_t* const rl = rs + SEG_RECS;
    uint32_t* const rd = rl + SEG_RECS;
    uint32_t* const span = rd + SEG_RECS;
    uint8_t* const text = reinterpret_cast<uint8_t*>(span + 4);
    if (LDS) {                                                        // the whole filter: 16 bytes a lane
        const int4* const src = reinterpret_cast<const int4*>(A.filter);
        int4* const dst = reinterpret_cast<int4*>(filter);
        for (uint32_t i = threadIdx.x; i < SEG_FILTER_WORDS / 4; i += SEG_THREADS) dst[i] = src[i];
    }
    const int nrec = GZ_SEG_TILE + A.K - 1;
    for (int64_t trip = blockIdx.x; trip < n_trips; trip += gridDim.x) {
        const int64_t base = trip * GZ_SEG_TILE;
        __syncthreads();                                              // (the trip before is done with the records and the text; the filter is there)
        for (int j = threadIdx.x; j < nrec; j += SEG_THREADS) {
            const int64_t t = base + j;
            const bool live = t < A.n_tokens;
            rs[j] = live ? A.tstart[t] : 0u; rl[j] = live ? A.tlen[t] : 0u; rd[j] = live ? A.tdoc[t] : 0xFFFFFFFFu;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int64_t left = A.n_tokens - base;
            const int last = (int)(left < nrec ? left : nrec) - 1;    // (>= 0: a trip has a token)
            span[0] = rs[0]; span[1] = rs[last] + rl[last] - rs[0];
        }
        __syncthreads();
        const uint32_t first = span[0], bytes = span[1];
        const bool staged = bytes <= (uint32_t)GZ_SEG_LDS_TEXT;
        const uint8_t* const mem = A.tb + A.lo;
        if (staged) {
            for (uint32_t i = threadIdx.x; i < bytes; i += SEG_THREADS) text[i] = mem[first + i];
            __syncthreads();
        }
        const int64_t t = base + threadIdx.x;
        if (t >= A.n_tokens) continue;                                // (block-uniform barriers only: the loop's own, at its top)
        if (staged) seg_start<LDS>(A, SegLdsText{text, first}, rs, rl, rd, filter, (int)threadIdx.x, t);
        else seg_start<LDS>(A, SegMemText{mem}, rs, rl, rd, filter, (int)threadIdx.x, t);
    }
}

__global__ __launch_bounds__(256) void gz_seg_mark_kernel(GzSegArgs A)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool closed = false;
    if (b < A.n_tokens) {
        closed = b == 0 || A.tdoc[b - 1] != A.tdoc[b];
        if (!closed) {
            closed = true;
            for (int64_t i = b - 1; i >= 0 && i > b - A.K; --i)
                if (i + (int64_t)A.reach[i] > b) { closed = false; break; }
        }
        A.closed[b] = closed ? 1 : 0;
    }
    const uint64_t m = wballot(closed);
    if (!m) return;
    uint32_t at = 0u;
    if (lane_id() == 0) at = atomicAdd(A.ctl + GZ_SEG_CTL_STRETCHES, (uint32_t)__popcll(m));
    at = (uint32_t)__shfl((int)at, 0, WAVE) + (uint32_t)below(m);
    if (closed && GZ_CHK(922, at, A.n_tokens)) A.starts[at] = (uint32_t)b;
}

__global__ __launch_bounds__(256) void gz_seg_walk_kernel(GzSegArgs A)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = q < (int64_t)A.ctl[GZ_SEG_CTL_STRETCHES];
    int64_t len = 0;
    if (live) {
        const int64_t s = A.starts[q];
        const int K = A.K;
        int64_t best[GZ_SEG_MAX_SYLLABLES];                           // best[m] = the best cost of the stretch's first j - 1 - m tokens
#pragma unroll
        for (int m = 0; m < GZ_SEG_MAX_SYLLABLES; ++m) best[m] = 0;
        int64_t j = 1;
        for (;; ++j) {
            const int64_t t = s + j - 1;
            int64_t least = INT64_MAX;
            uint32_t pick = 0u;
#pragma unroll
            for (int k = 1; k <= GZ_SEG_MAX_SYLLABLES; ++k) {
                if (k > K || k > j) break;
                uint32_t c = A.cand[(size_t)(t - k + 1) * (size_t)K + (size_t)(k - 1)];
                const bool known = c != GZ_SEG_NONE;
                if (k == 1 && !known) c = A.unk_cost;
                if (c == GZ_SEG_NONE) continue;
                const int64_t v = best[k - 1] + (int64_t)c;
                if (v <= least) { least = v; pick = (uint32_t)k | (known ? 0x80u : 0u); }     // (equal minima: the largest k)
            }
            A.choice[t] = (uint8_t)pick;
#pragma unroll
            for (int m = GZ_SEG_MAX_SYLLABLES - 1; m > 0; --m) best[m] = best[m - 1];
            best[0] = least;
            if (t + 1 >= A.n_tokens || A.closed[t + 1]) break;
        }
        len = j;
        unsigned long long words = 0ull, known = 0ull;
        for (int64_t pos = s + len; pos > s;) {
            const uint32_t ch = A.choice[pos - 1];
            int64_t k = ch & 0x7Fu;
            if (k < 1 || k > pos - s) k = 1;                          // (never: the walk above wrote a k inside the stretch)
            for (int64_t i = pos - k; i < pos - 1; ++i) A.join[i] = 1;
            A.join[pos - 1] = 0;
            ++words; known += ch >> 7;
            pos -= k;
        }
        unsigned long long* const st = A.stats + 4 * (size_t)A.tdoc[s];
        atomicAdd(st + 1, words);
        if (known) atomicAdd(st + 2, known);
        atomicAdd(st + 3, (unsigned long long)best[0]);
    }
    // the stretch lengths of the call, for whoever measures: a wave adds its counts once
    const uint64_t m1 = wballot(live && len == 1), m8 = wballot(live && len > 1 && len <= 8), mx = wballot(live && len > 8);
    uint32_t longest = (uint32_t)(len > 0xFFFFFFFFll ? 0xFFFFFFFFll : len);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)longest, d, WAVE);
        longest = y > longest ? y : longest;
    }
    if (lane_id() != 0) return;
    if (m1) atomicAdd(A.ctl + GZ_SEG_CTL_LEN1, (uint32_t)__popcll(m1));
    if (m8) atomicAdd(A.ctl + GZ_SEG_CTL_LEN8, (uint32_t)__popcll(m8));
    if (mx) atomicAdd(A.ctl + GZ_SEG_CTL_LONGER, (uint32_t)__popcll(mx));
    if (longest) atomicMax(A.ctl + GZ_SEG_CTL_LONGEST, longest);
}

__global__ __launch_bounds__(256) void gz_seg_emit_kernel(GzSegArgs A)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, t = g / GZ_SEG_EMIT_LANES;
    const uint32_t sub = (uint32_t)(g % GZ_SEG_EMIT_LANES);
    if (t >= A.n_tokens) return;
    const uint32_t d = A.tdoc[t];
    if (!GZ_CHK(923, d, A.n_docs) || (int64_t)d >= A.n_docs) return;
    const uint32_t t0 = A.ptoff[A.woff[d]], t1 = A.ptoff[A.woff[d + 1]], len = A.tlen[t];
    const int64_t pos = A.out_off[d] + (int64_t)(A.tlsum[t] - A.tlsum[t0]) + (t - (int64_t)t0);
    const bool last = t + 1 >= (int64_t)t1;
    if (pos < A.out_off[d] || pos + len + (last ? 0 : 1) > A.out_off[d + 1]) return;      // (never: the offsets are these sums)
    const uint8_t* const src = A.tb + A.lo + A.tstart[t];
    for (uint32_t i = sub; i < len; i += GZ_SEG_EMIT_LANES) A.out[pos + i] = src[i];
    if (sub != 0) return;
    if (!last) A.out[pos + len] = A.join[t] ? 0x5Fu : 0x20u;
    if (A.tok_off) A.tok_off[t] = A.lo + (int64_t)A.tstart[t];
}
