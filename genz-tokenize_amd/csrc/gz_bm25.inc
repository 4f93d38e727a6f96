// gz_bm25.inc -- BM25 / BM25Plus index and scoring (genz_tokenize/ranking.py of the reference), included by gz_kernels.hip.
//
// Index build over packed UTF-8 + int64 offsets in HBM (the reference's __init__, ranking.py:6-27):
//   gz_bm25_count_kernel    one wave per document, 64-byte tiles (a lane per byte): str.split() word boundaries -- a word is a
//                           maximal run of bytes that belong to no whitespace character (the 29 code points of str.isspace(),
//                           is_ws1/2/3 of gz_pipeline.inc; no '\n' glued to a word) -> words per document = fieldLens
//   gz_bm25_scan_*          exclusive scan (u32) over many workgroups: reduce, scan of the block sums, down-sweep
//   gz_bm25_words_kernel    the same walk again: start / end byte of every word, compacted by ballot + the scanned counts
//   gz_bm25_hash_kernel     64-bit hash of each word's bytes (truncated by the switch bm25_hash_bits: forced collisions)
//   gz_bm25_dedup_*         exact de-duplication in rounds: every word of the round inserts its hash into an open-addressing
//                           table and takes part in an atomicMax(~word) (the smallest word index wins); after the kernel boundary
//                           each word compares its BYTES with the winner of its slot -- equal: that is its representative, else it
//                           goes to the next round (a true hash collision becomes two terms).  No lane ever waits for another.
//   gz_bm25_first / _term   term id = number of representatives before the word's representative (first-occurrence order)
//   gz_bm25_pair_*          (document, term) pairs in a second table: count, first occurrence in the document; then df[term] (16
//                           counters per term, summed by gz_bm25_df_kernel),
//                           a 256-bit term signature per document and the doc-major (term, count) entries
//   gz_bm25_known_kernel    an append (gz_bm25_append): the batch's words against the live term table; the unknown ones go through
//                           the de-duplication as a list, and every kernel above numbers the batch from the bases in GzBm25Args
//   gz_bm25_rehash_kernel   the term table or the pair table into a larger one, slot by slot (the keys carry the index's own hash mask)
//   gz_bm25_rm_*            a removal (gz_bm25_remove): mark the documents, scan the marks (new id = old id - removed before it) and
//                           the kept documents' entry counts, then compact fieldLens, signatures and entries OUT OF PLACE into staged
//                           buffers, fill a fresh pair table from the compacted entries and take the removed documents' entries off
//                           a staged copy of df.  The live index is only read.  (gz_bm25_rm_seq_kernel: a positional index's words)
//   gz_bm25_cp_*            the canonical numbering of the live terms (gz_bm25_compact, gz_bm25_terms): first[term] = its smallest
//                           entry index, the entries that are their term's first flagged and scanned -> new id = a fresh build's; the
//                           terms' lengths scanned in new-id order, their bytes gathered into an arena; then (a compaction) entries,
//                           pair table and signatures again under the new ids and, gz_bm25_rekey_kernel, the term table without its
//                           dead terms -- all OUT OF PLACE, the live index is only read  (gz_bm25_cp_seq_kernel: a positional
//                           index's words under the new ids)
//   gz_bm25_lookup_kernel   query words (packed) -> term id (-1: absent) and df, bytes compared in full
//   gz_bm25_score_kernel    scores[Q, N] float64 in the reference's order of operations (ranking.py:33-45, :52-63)
// (gz_search.inc: the term-major postings and the search over them)
//
// Vector stores and vector atomics only.  Results never depend on the order in which atomics land: counts and df are sums,
// representatives and first occurrences are minima, signatures are ORs, term ids come out of a scan; of the decrements that
// take a term's df to 0 exactly one sees the 1, whatever their order.  In the compaction: first[] is a minimum; flags, new ids,
// orders and offsets are plain stores of values that scans of those give; every arena byte, entry and signature word has one
// writer (signatures are ORed in registers); table slots are claimed by CAS, and which of several equal keys sits first along a
// probe sequence is the one thing that varies -- no answer reads it (a lookup compares bytes, pair keys are unique).
// The postings of a search (gz_search.inc) are filled through per-term atomic cursors: the order of the documents inside a term's
// list varies from run to run, and no answer reads it either -- a list only ever becomes bits of a per-query bitmap (an OR), and
// counts, candidates (in ascending document id), scores and ranks are functions of the bits.

namespace {

constexpr int BM_WPB = 4;                    // waves (documents) per workgroup of the walking kernels
constexpr int BM_SCAN_BLOCK = 4096;          // elements per workgroup of the scan (16 rounds of 256)
constexpr int BM_SC_LDS = 4096;              // (term, count) entries a scoring workgroup stages in LDS (32 KB)
constexpr int BM_QW_LDS = 512;               // query words a scoring workgroup stages in LDS at a time (8 KB)
constexpr uint32_t BM_CP_SHORT = 16;         // bytes of a term that its own lane copies (gz_bm25_cp_gather_kernel); longer: the wave
struct BmQword { int32_t t; uint32_t bit; double idf; };

__device__ __forceinline__ unsigned long long bm_mix64(unsigned long long x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// FNV-1a over the bytes, then a finaliser (truncation to the low bits must still spread the words)
__device__ __forceinline__ unsigned long long bm_hash(const uint8_t* p, int64_t n)
{
    unsigned long long h = 0xCBF29CE484222325ull;
    for (int64_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001B3ull; }
    return bm_mix64(h ^ (unsigned long long)n);
}
// table key of a hash: never 0 (the empty slot)
__device__ __forceinline__ unsigned long long bm_key(unsigned long long h, unsigned long long mask) { return (h & mask) | (1ull << 63); }
__device__ __forceinline__ uint32_t bm_sig_bit(uint32_t term) { return (uint32_t)(bm_mix64((unsigned long long)term + 0x9E3779B97F4A7C15ull) & 255u); }
// The NaN the reference's host arithmetic gives (x86 SSE, ranking.py evaluated left to right): when r = a op b is a NaN, it is the
// first NaN operand, quieted, else -- an invalid operation such as 0 / 0 -- the x86 default NaN, whose sign bit is SET.  (The GPU's
// own NaNs are positive: without this, a score of all-empty documents or k1 = 0 would differ from the reference in its sign bit.)
__device__ __forceinline__ double bm_nan(double r, double a, double b)
{
    if (r == r) return r;
    const unsigned long long q = 0x0008000000000000ull;
    const unsigned long long u = a != a ? (unsigned long long)__double_as_longlong(a) | q
                               : b != b ? (unsigned long long)__double_as_longlong(b) | q : 0xFFF8000000000000ull;
    return __longlong_as_double((long long)u);
}
// The scoring arithmetic, shared by gz_bm25_score_kernel and gz_bm25_sr_score_kernel (gz_search.inc) so that both give the same
// bits.  A document's factors: K = k1 * ((1 - b) + b * (dl / avg)) and t0, the term for f = 0.
__device__ __forceinline__ void bm_doc_factors(const GzBm25Score& S, double dl, double& K, double& t0)
{
#pragma clang fp contract(off)
    const double x = bm_nan(dl / S.avg, dl, S.avg);
    const double y = bm_nan(S.b * x, S.b, x);
    const double z = bm_nan(S.omb + y, S.omb, y);
    K = bm_nan(S.k1 * z, S.k1, z);
    const double n0 = bm_nan(0.0 * S.kp1, 0.0, S.kp1), d0K = bm_nan(0.0 + K, 0.0, K);
    t0 = bm_nan(n0 / d0K, n0, d0K);
}
// one query word: score + idf * t (BM25Plus: idf * (t + delta)) for the word's count f in the document
__device__ __forceinline__ double bm_word_score(const GzBm25Score& S, double score, uint32_t f, double K, double t0, double idf)
{
#pragma clang fp contract(off)
    double tf = t0;
    if (f != 0) {
        const double fd = (double)f;
        const double num = bm_nan(fd * S.kp1, fd, S.kp1), den = bm_nan(fd + K, fd, K);
        tf = bm_nan(num / den, num, den);
    }
    const double v = S.plus ? bm_nan(tf + S.delta, tf, S.delta) : tf;
    const double a = bm_nan(idf * v, idf, v);
    return bm_nan(score + a, score, a);
}
__device__ __forceinline__ bool bm_equal(const uint8_t* a, const uint8_t* b, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) if (a[i] != b[i]) return false;
    return true;
}

// Words of one document by one wave.  p = its first byte, len its bytes, abs0 its absolute offset.  WRITE: word k of the
// document gets wstart / wend (absolute byte offsets) and wdoc at index w0 + k.  Returns the number of words (every lane).
template <bool WRITE>
__device__ uint32_t bm_doc_words(const uint8_t* p, int64_t len, int64_t abs0, uint32_t w0, int64_t* wstart, int64_t* wend, uint32_t* wdoc,
                                 uint32_t doc)
{
    const int lane = lane_id();
    uint64_t spill = 0, prev = 0;            // whitespace bytes of a character that began in the tile before; its last byte was a word byte
    uint32_t ns = 0, ne = 0;
    for (int64_t t = 0; t < len; t += WAVE) {
        const int64_t i = t + lane;
        const bool valid = i < len;
        const uint32_t b0 = valid ? p[i] : 0u, b1 = i + 1 < len ? p[i + 1] : 0u, b2 = i + 2 < len ? p[i + 2] : 0u;
        const uint64_t vm = wballot(valid);
        const uint64_t l1 = wballot(valid && is_ws1(b0));
        const uint64_t l2 = wballot(valid && is_ws2(b0, b1));
        const uint64_t l3 = wballot(valid && is_ws3(b0, b1, b2));
        const uint64_t ws = l1 | l2 | (l2 << 1) | l3 | (l3 << 1) | (l3 << 2) | spill;
        spill = (l2 >> 63) | (l3 >> 62) | (l3 >> 63);
        const uint64_t word = vm & ~ws;
        const uint64_t before = (word << 1) | prev;       // bit k: byte k - 1 is a word byte
        const uint64_t st = word & ~before;
        const uint64_t en = ~word & before;               // (the first byte past the document ends its last word too)
        prev = word >> 63;
        if (WRITE) {
            if ((st >> lane) & 1ull) {
                const uint32_t k = w0 + ns + (uint32_t)__popcll(st & lt_mask(lane));
                wstart[k] = abs0 + i;
                wdoc[k] = doc;
            }
            if ((en >> lane) & 1ull) wend[w0 + ne + (uint32_t)__popcll(en & lt_mask(lane))] = abs0 + i;
        }
        ns += (uint32_t)__popcll(st);
        ne += (uint32_t)__popcll(en);
    }
    if (prev) {                                           // the last word runs to the end of the document
        if (WRITE && lane == 0) wend[w0 + ne] = abs0 + len;
    }
    return ns;
}

// a document's bytes, or none when its offsets are not inside the text the caller announced (flag raised)
__device__ __forceinline__ int64_t bm_doc_len(const GzBm25Args& A, int64_t d, int64_t& o, bool raise)
{
    o = A.off[d] + A.obase;
    const int64_t e = A.off[d + 1] + A.obase;
    if (o < A.lo || e < o || e > A.hi) {
        if (raise && lane_id() == 0) atomicOr(&A.ctl[1], 1u);
        return 0;
    }
    return e - o;
}

}  // namespace

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_count_kernel(GzBm25Args A)
{
    const int64_t d = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= A.n_docs) return;
    int64_t o;
    const int64_t len = bm_doc_len(A, d, o, true);
    const uint32_t n = bm_doc_words<false>(A.tb + o, len, o, 0, nullptr, nullptr, nullptr, 0);
    if (lane_id() == 0) A.wcnt[d] = n;
}

__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_words_kernel(GzBm25Args A)
{
    const int64_t d = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= A.n_docs) return;
    int64_t o;
    const int64_t len = bm_doc_len(A, d, o, false);
    (void)bm_doc_words<true>(A.tb + o, len, o, A.woff[d], A.wstart, A.wend, A.wdoc, A.doc_base + (uint32_t)d);
}

// ---- exclusive scan of u32 values: out[i] = in[0] + ... + in[i - 1], out[n] = total (the total must fit 32 bits) ----------
namespace {
// block-wide exclusive scan of one value per thread (256 threads); `all` = the block's total
__device__ __forceinline__ uint32_t bm_block_scan(uint32_t v, uint32_t& all, uint32_t* wt)
{
    const int lane = lane_id(), wv = (int)(threadIdx.x / WAVE);
    int tot;
    const uint32_t ex = (uint32_t)wave_excl_sum((int)v, lane, tot);
    if (lane == 0) wt[wv] = (uint32_t)tot;
    __syncthreads();
    uint32_t pre = 0;
    all = 0;
    for (int k = 0; k < 4; ++k) { const uint32_t x = wt[k]; if (k < wv) pre += x; all += x; }
    __syncthreads();
    return pre + ex;
}
}  // namespace

__global__ __launch_bounds__(256) void gz_bm25_scan_a_kernel(const uint32_t* in, int64_t n, uint32_t* bsum)
{
    __shared__ uint32_t wt[4];
    uint32_t s = 0;
    for (int r = 0; r < BM_SCAN_BLOCK / 256; ++r) {
        const int64_t i = (int64_t)blockIdx.x * BM_SCAN_BLOCK + r * 256 + threadIdx.x;
        if (i < n) s += in[i];
    }
    uint32_t all;
    (void)bm_block_scan(s, all, wt);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void gz_bm25_scan_b_kernel(uint32_t* bsum, int64_t nb, uint32_t* total)
{
    __shared__ uint32_t wt[4];
    uint32_t carry = 0;
    for (int64_t r = 0; r < nb; r += 256) {
        const int64_t i = r + threadIdx.x;
        const uint32_t v = i < nb ? bsum[i] : 0u;
        uint32_t all;
        const uint32_t ex = bm_block_scan(v, all, wt);
        if (i < nb) bsum[i] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void gz_bm25_scan_c_kernel(const uint32_t* in, int64_t n, const uint32_t* bsum, uint32_t* out)
{
    __shared__ uint32_t wt[4];
    uint32_t carry = bsum[blockIdx.x];
    for (int r = 0; r < BM_SCAN_BLOCK / 256; ++r) {
        const int64_t i = (int64_t)blockIdx.x * BM_SCAN_BLOCK + r * 256 + threadIdx.x;
        const uint32_t v = i < n ? in[i] : 0u;
        uint32_t all;
        const uint32_t ex = bm_block_scan(v, all, wt);
        if (i < n) out[i] = carry + ex;
        carry += all;
    }
}

// ---- per word -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gz_bm25_hash_kernel(GzBm25Args A)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    const int64_t s = A.wstart[w];
    A.whash[w] = bm_key(bm_hash(A.tb + s, A.wend[w] - s), A.hmask);
}

// one round of the de-duplication: the words list[0 .. n) (list == nullptr: every word) insert their keys
__global__ __launch_bounds__(256) void gz_bm25_dedup_ins_kernel(GzBm25Args A, const uint32_t* list, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = list ? list[i] : (uint32_t)i;
    const unsigned long long key = A.whash[w];
    unsigned long long s = bm_mix64(key) & A.dmask;
    // Frequent words put up to millions of words on one slot: a plain load first, and an atomic only where it can still change
    // something (a key, once set, never changes; the slot's value only grows -- a stale load just costs the atomic).
    for (;;) {                                            // (a probe, not a wait: the table has more slots than keys)
        unsigned long long old = __hip_atomic_load(&A.dtab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0ull) old = atomicCAS(&A.dtab[s].key, 0ull, key);
        if (old == 0ull || old == key) break;
        s = (s + 1) & A.dmask;
    }
    if (__hip_atomic_load(&A.dtab[s].a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ~w) atomicMax(&A.dtab[s].a, ~w);
    A.wslot[w] = (uint32_t)s;
}

// ... and, after the kernel boundary, compare bytes with the slot's winner; the words that differ form the next round
__global__ __launch_bounds__(256) void gz_bm25_dedup_res_kernel(GzBm25Args A, const uint32_t* list, int64_t n, uint32_t* next)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = list ? list[i] : (uint32_t)i;
    const uint32_t r = ~A.dtab[A.wslot[w]].a;
    bool same = r == w;
    if (!same) {
        const int64_t sw = A.wstart[w], sr = A.wstart[r], lw = A.wend[w] - sw;
        same = lw == A.wend[r] - sr && bm_equal(A.tb + sw, A.tb + sr, lw);
    }
    if (same) A.rep[w] = r;
    else next[atomicAdd(&A.ctl[0], 1u)] = w;
}

__global__ __launch_bounds__(256) void gz_bm25_first_kernel(GzBm25Args A)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    A.flag[w] = A.rep[w] == (uint32_t)w ? 1u : 0u;
}

// term ids (scan of the representative flags); representatives describe their term and enter the lookup table
__global__ __launch_bounds__(256) void gz_bm25_term_kernel(GzBm25Args A)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    const uint32_t r = A.rep[w];
    if (r == GZ_BM25_KNOWN_WORD) return;                  // (an append: gz_bm25_known_kernel wrote its term)
    const uint32_t t = A.term_base + A.scan[r];
    A.term[w] = t;
    if (r != (uint32_t)w) return;
    A.tstart[t] = A.wstart[w];
    A.tlen[t] = (uint32_t)(A.wend[w] - A.wstart[w]);
    const unsigned long long key = A.whash[w];
    unsigned long long s = bm_mix64(key) & A.tmask;
    while (atomicCAS(&A.ttab[s].key, 0ull, key) != 0ull) s = (s + 1) & A.tmask;       // every term its own slot
    A.ttab[s].a = t;
}

// (document, term) pairs: count and first occurrence (smallest word index) in the document
__global__ __launch_bounds__(256) void gz_bm25_pair_ins_kernel(GzBm25Args A)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    const unsigned long long key = (((unsigned long long)A.wdoc[w] << 32) | A.term[w]) + 1ull;
    unsigned long long s = bm_mix64(key) & A.pmask;
    for (;;) {
        const unsigned long long old = atomicCAS(&A.ptab[s].key, 0ull, key);
        if (old == 0ull || old == key) break;
        s = (s + 1) & A.pmask;
    }
    atomicAdd(&A.ptab[s].a, 1u);
    atomicMax(&A.ptab[s].b, ~(uint32_t)w);
    A.wslot[w] = (uint32_t)s;
}

__global__ __launch_bounds__(256) void gz_bm25_pair_first_kernel(GzBm25Args A)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    const bool first = ~A.ptab[A.wslot[w]].b == (uint32_t)w;
    A.flag[w] = first ? 1u : 0u;
    if (!first) return;
    const uint32_t t = A.term[w], bit = bm_sig_bit(t);
    const uint32_t had = atomicAdd(&A.dfs[(int64_t)(A.wdoc[w] & (GZ_BM25_DF_SHARDS - 1)) * A.n_terms + t], 1u);     // (16 counters per term: frequent terms)
    // an append (one counter per term, df itself): a term older than the batch whose df was 0 -- every document that had it was
    // removed -- is live again; exactly one increment starts from 0
    if (had == 0u && t < A.term_base) atomicAdd(&A.ctl[2], 1u);
    atomicOr(&A.sig[(int64_t)A.wdoc[w] * 4 + (bit >> 6)], 1ull << (bit & 63u));
}

__global__ __launch_bounds__(256) void gz_bm25_ent_kernel(GzBm25Args A)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w < A.n_words && A.flag[w]) A.ent[A.scan[w]] = make_uint2(A.term[w], A.ptab[A.wslot[w]].a);
    if (w <= A.n_docs) A.eoff[w] = A.ent_base + A.scan[A.woff[w]];      // (the launch covers max(words, documents + 1) threads)
}

__global__ __launch_bounds__(256) void gz_bm25_df_kernel(GzBm25Args A)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= A.n_terms) return;
    uint32_t n = 0;
    for (int k = 0; k < GZ_BM25_DF_SHARDS; ++k) n += A.dfs[k * A.n_terms + t];
    A.df[t] = n;
}

// ---- append ---------------------------------------------------------------------------------------------------------------
// The batch's words against the live term table (gz_bm25_lookup_kernel's probe, the bytes compared in full): a word that is a term
// already takes its id and stays out of the de-duplication; the others form the first round's list (any order: a round's outcome is
// a minimum over word indices).
__global__ __launch_bounds__(256) void gz_bm25_known_kernel(GzBm25Args A, uint32_t* next)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.n_words) return;
    const int64_t s = A.wstart[w], n = A.wend[w] - s;
    const unsigned long long key = A.whash[w];
    unsigned long long slot = bm_mix64(key) & A.tmask;
    for (;;) {
        const unsigned long long k = A.ttab[slot].key;
        if (k == 0ull) break;
        if (k == key) {
            const uint32_t t = A.ttab[slot].a;
            if ((int64_t)A.tlen[t] == n && bm_equal(A.tb + A.tstart[t], A.tb + s, n)) {
                A.term[w] = t;
                A.rep[w] = GZ_BM25_KNOWN_WORD;
                return;
            }
        }
        slot = (slot + 1) & A.tmask;
    }
    next[atomicAdd(&A.ctl[0], 1u)] = (uint32_t)w;
}

// a table moves into a larger one: keys are unique in `from`, so every one claims its own slot; a and b travel with it
__global__ __launch_bounds__(256) void gz_bm25_rehash_kernel(const GzBm25Slot* from, int64_t n_slots, GzBm25Slot* to, unsigned long long mask)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_slots) return;
    const GzBm25Slot o = from[i];
    if (o.key == 0ull) return;
    unsigned long long s = bm_mix64(o.key) & mask;
    while (atomicCAS(&to[s].key, 0ull, o.key) != 0ull) s = (s + 1) & mask;
    to[s].a = o.a;
    to[s].b = o.b;
}

// ---- remove ---------------------------------------------------------------------------------------------------------------
// Every kernel here reads the live index and writes workspace or staged buffers only (gz_bm25_remove swaps them in afterwards).
// gone[] is cleared by the caller.  An id listed twice stores the same 1 twice: the scan counts the document once.
__global__ __launch_bounds__(256) void gz_bm25_rm_mark_kernel(GzBm25Rm R)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R.n_ids) return;
    const int64_t id = R.ids[i];
    if (id < 0 || id >= R.n_docs) atomicOr(&R.ctl[1], 1u);
    else R.gone[id] = 1u;
}

// entries each document keeps (none when it goes)
__global__ __launch_bounds__(256) void gz_bm25_rm_count_kernel(GzBm25Rm R)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= R.n_docs) return;
    R.kcnt[d] = R.gone[d] ? 0u : R.eoff[d + 1] - R.eoff[d];
    if (R.kdl) R.kdl[d] = R.gone[d] ? 0u : R.dl[d];          // (a positional index: the words it keeps)
}

// per kept document: fieldLen, signature and first entry under its new id; thread n_docs closes the new eoff
__global__ __launch_bounds__(256) void gz_bm25_rm_docs_kernel(GzBm25Rm R)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d > R.n_docs) return;
    const int64_t nd = d - (int64_t)R.before[d];
    if (d == R.n_docs) { R.eoff2[nd] = R.neoff[d]; return; }
    if (R.gone[d]) return;
    R.dl2[nd] = R.dl[d];
    for (int k = 0; k < 4; ++k) R.sig2[nd * 4 + k] = R.sig[d * 4 + k];
    R.eoff2[nd] = R.neoff[d];
}

// A wave per document (one may hold 100 000 entries).  Kept: its entries move to their new place and enter the fresh pair table
// under the new document id (keys are unique, every one claims its own slot; only `a` is read after a build or an append).
// Removed: each entry takes 1 off the staged df of its term; the decrement that sees 1 makes the term a dead one.
__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_rm_ent_kernel(GzBm25Rm R)
{
    const int64_t d = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= R.n_docs) return;
    const int lane = lane_id();
    const uint32_t e0 = R.eoff[d], e1 = R.eoff[d + 1];
    if (R.gone[d]) {
        for (uint32_t e = e0 + (uint32_t)lane; e < e1; e += WAVE)
            if (atomicSub(&R.df2[R.ent[e].x], 1u) == 1u) atomicAdd(&R.ctl[2], 1u);
        if (lane == 0) atomicAdd((unsigned long long*)(R.ctl + 4), (unsigned long long)R.dl[d]);
        return;
    }
    const unsigned long long pkey = (unsigned long long)(d - (int64_t)R.before[d]) << 32;
    const uint32_t o = R.neoff[d];
    for (uint32_t e = e0 + (uint32_t)lane; e < e1; e += WAVE) {
        const uint2 en = R.ent[e];
        R.ent2[o + (e - e0)] = en;
        const unsigned long long key = (pkey | en.x) + 1ull;
        unsigned long long s = bm_mix64(key) & R.pmask2;
        while (atomicCAS(&R.ptab2[s].key, 0ull, key) != 0ull) s = (s + 1) & R.pmask2;     // (a probe: more slots than keys)
        R.ptab2[s].a = en.y;
    }
}

// A positional index: a wave per document (one may hold 100 000 words), the kept documents' words to their new places.  The old
// range must lie inside the n_words words of seq (else the flag: dl and seq contradict each other); the new one is as long, and
// the scan of the kept lengths ends where seq2 does.
__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_rm_seq_kernel(GzBm25Rm R)
{
    const int64_t d = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= R.n_docs || R.gone[d]) return;
    const uint32_t w0 = R.woff[d], w1 = R.woff[d + 1], o = R.nwoff[d];
    if (w1 < w0 || (int64_t)w1 > R.n_words || R.nwoff[d + 1] - o != w1 - w0) {
        if (lane_id() == 0) atomicOr(&R.ctl[1], 1u);
        return;
    }
    for (uint32_t i = w0 + (uint32_t)lane_id(); i < w1; i += WAVE) R.seq2[o + (i - w0)] = R.seq[i];
}

// ---- compact / vocabulary ---------------------------------------------------------------------------------------------------
// The canonical numbering.  Entries are doc-major and in first-occurrence order inside a document (a removal keeps both), so the
// entry with the smallest index among a term's entries is where a fresh build of the current documents meets the term first:
// numbering the terms by that entry is that build's numbering.  Every kernel here reads the live index and writes workspace or
// staged buffers only.  first[] is set to all ones by the caller.
__global__ __launch_bounds__(256) void gz_bm25_cp_first_kernel(GzBm25Cp C)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= C.n_ent) return;
    const uint32_t t = C.ent[e].x;
    if ((int64_t)t >= C.n_terms) { atomicOr(&C.ctl[1], 1u); return; }
    // a minimum: whatever the order of the atomics (a frequent term has millions of entries: a load first, the atomic only where
    // it can still lower the value -- a stale load just costs the atomic)
    if (__hip_atomic_load(&C.first[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)e) atomicMin(&C.first[t], (uint32_t)e);
}

__global__ __launch_bounds__(256) void gz_bm25_cp_flag_kernel(GzBm25Cp C)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= C.n_ent) return;
    const uint32_t t = C.ent[e].x;
    C.flag[e] = (int64_t)t < C.n_terms && C.first[t] == (uint32_t)e ? 1u : 0u;
}

// new id = flags before the term's first entry; the new order's view of the old terms (order, nlen)
__global__ __launch_bounds__(256) void gz_bm25_cp_newid_kernel(GzBm25Cp C)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= C.n_terms) return;
    const uint32_t f = C.first[t];
    const bool live = f != 0xFFFFFFFFu;
    if (live != (C.df[t] != 0u)) atomicOr(&C.ctl[1], 1u);
    if (!live) { C.newid[t] = 0xFFFFFFFFu; return; }
    const uint32_t n = C.scan[f];                             // (< flags raised <= n_terms: order and nlen hold n_terms + 1)
    C.newid[t] = n;
    C.order[n] = (uint32_t)t;
    C.nlen[n] = C.tlen[t];
}

// The live terms' bytes into the arena, and their rows under the new ids.  A lane per term, 64 consecutive new ids per wave (their
// bytes are neighbours in the arena): a term of at most BM_CP_SHORT bytes -- nearly all -- is copied by its lane; the longer ones
// are then taken one after the other by the whole wave, 64 bytes a step (an 80 000-byte term: 1 250 steps of a wave, and the
// other waves go on).  Every byte of the arena has exactly one writer.
__global__ __launch_bounds__(256) void gz_bm25_cp_gather_kernel(GzBm25Cp C)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    int64_t src = 0;
    uint32_t len = 0, dst = 0;
    if (n < C.n_new) {
        const uint32_t o = C.order[n];
        src = C.tstart[o]; len = C.nlen[n]; dst = C.toff[n];
        C.tstart2[n] = (int64_t)dst;
        if (C.tlen2) C.tlen2[n] = len;
        C.df2[n] = C.df[o];
    } else if (n == C.n_new && C.close) C.tstart2[n] = (int64_t)C.toff[n];
    if (!C.arena) return;                                     // (uniform)
    if (len <= BM_CP_SHORT)
        for (uint32_t i = 0; i < len; ++i) C.arena[(int64_t)dst + i] = C.tb[src + i];
    uint64_t m = wballot(len > BM_CP_SHORT);
    while (m) {                                               // (uniform)
        const int k = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int64_t s = __shfl(src, k, WAVE), d = (int64_t)(uint32_t)__shfl((int)dst, k, WAVE);
        const uint32_t l = (uint32_t)__shfl((int)len, k, WAVE);
        for (uint32_t i = (uint32_t)lane; i < l; i += WAVE) C.arena[d + i] = C.tb[s + i];
    }
}

// the term table into a fresh one under the new ids; the keys carry the index's hash mask already (no byte is hashed).  Terms that
// share a (truncated) key keep a slot each; their order along the probe sequence depends on who lands first, what a lookup
// answers does not (it compares the bytes).
__global__ __launch_bounds__(256) void gz_bm25_rekey_kernel(const GzBm25Slot* from, int64_t n_slots, const uint32_t* newid, GzBm25Slot* to,
                                                            unsigned long long mask)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_slots) return;
    const GzBm25Slot o = from[i];
    if (o.key == 0ull) return;
    const uint32_t t = newid[o.a];
    if (t == 0xFFFFFFFFu) return;                             // a dead term leaves the table
    unsigned long long s = bm_mix64(o.key) & mask;
    while (atomicCAS(&to[s].key, 0ull, o.key) != 0ull) s = (s + 1) & mask;          // (a probe: more slots than keys)
    to[s].a = t;
}

// A wave per document, as gz_bm25_rm_ent_kernel: its entries under the new ids at their old places, the pairs into the fresh pair
// table (unique keys, every one claims its own slot), and the document's signature again from the new ids -- ORed in registers
// and across the wave, then stored: no atomic touches it.
__global__ __launch_bounds__(WAVE * BM_WPB) void gz_bm25_cp_ent_kernel(GzBm25Cp C)
{
    const int64_t d = (int64_t)blockIdx.x * BM_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= C.n_docs) return;
    const int lane = lane_id();
    const uint32_t e0 = C.eoff[d], e1 = C.eoff[d + 1];
    const unsigned long long pkey = (unsigned long long)d << 32;
    unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t e = e0 + (uint32_t)lane; e < e1; e += WAVE) {
        const uint2 en = C.ent[e];
        const uint32_t t = (int64_t)en.x < C.n_terms ? C.newid[en.x] : 0xFFFFFFFFu;
        if (t == 0xFFFFFFFFu) { atomicOr(&C.ctl[1], 1u); continue; }
        C.ent2[e] = make_uint2(t, en.y);
        const uint32_t bit = bm_sig_bit(t), w = bit >> 6;
        const unsigned long long b = 1ull << (bit & 63u);
        s0 |= w == 0u ? b : 0ull; s1 |= w == 1u ? b : 0ull; s2 |= w == 2u ? b : 0ull; s3 |= w == 3u ? b : 0ull;
        const unsigned long long key = (pkey | t) + 1ull;
        unsigned long long s = bm_mix64(key) & C.pmask2;
        while (atomicCAS(&C.ptab2[s].key, 0ull, key) != 0ull) s = (s + 1) & C.pmask2;     // (a probe: more slots than keys)
        C.ptab2[s].a = en.y;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        s0 |= __shfl_xor(s0, o, WAVE); s1 |= __shfl_xor(s1, o, WAVE); s2 |= __shfl_xor(s2, o, WAVE); s3 |= __shfl_xor(s3, o, WAVE);
    }
    if (lane < 4) C.sig2[d * 4 + lane] = lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? s2 : s3;
}

// A positional index: every word's term id under the new numbering.  A word whose term has no new id contradicts the index.
__global__ __launch_bounds__(256) void gz_bm25_cp_seq_kernel(GzBm25Cp C)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C.n_words) return;
    const uint32_t o = C.seq[i];
    const uint32_t t = (int64_t)o < C.n_terms ? C.newid[o] : 0xFFFFFFFFu;
    if (t == 0xFFFFFFFFu) { atomicOr(&C.ctl[1], 1u); return; }
    C.seq2[i] = t;
}

// ---- lookup ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gz_bm25_lookup_kernel(GzBm25Look L)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.n) return;
    const int64_t s = L.qoff[i], n = L.qoff[i + 1] - s;
    const unsigned long long key = bm_key(bm_hash(L.qtext + s, n), L.hmask);
    unsigned long long slot = bm_mix64(key) & L.tmask;
    int32_t found = -1;
    for (;;) {
        const unsigned long long k = L.ttab[slot].key;
        if (k == 0ull) break;
        if (k == key) {
            const uint32_t t = L.ttab[slot].a;
            if ((int64_t)L.tlen[t] == n && bm_equal(L.tb + L.tstart[t], L.qtext + s, n)) { found = (int32_t)t; break; }
        }
        slot = (slot + 1) & L.tmask;
    }
    const uint32_t df = found >= 0 ? L.df[found] : 0u;
    if (df == 0u) found = -1;                                 // (a term whose last document was removed: in the table, in no document)
    L.term_out[i] = found;
    L.df_out[i] = (int32_t)df;
}

// ---- scoring: one thread per document, every query of the batch --------------------------------------------------------------
// score = 0; for each query word in order: score = score + idf * t   (BM25Plus: idf * (t + delta)), with
//   t = (f * (k1 + 1)) / (f + k1 * ((1 - b) + b * (dl / avg)))
// in IEEE double, no contraction (a + b * c must not become an FMA), NaNs as the host makes them (bm_nan).  The document's factor
// K = k1 * (...) is hoisted, and so is t for f = 0: t0 = (0 * (k1 + 1)) / (0 + K) -- the same operations on the same operands, so
// the same bits, nan / inf / -0.0 included.
// f comes from the document's (term, count) entries in LDS (the workgroup's 256 documents, when they fit), else from the pair
// table; a 256-bit signature per document skips the search for most absent words.  The queries' words pass through LDS in chunks
// (one broadcast read per word instead of a scalar and a vector load from memory, each waited for).
__global__ __launch_bounds__(256) void gz_bm25_score_kernel(GzBm25Score S)
{
#pragma clang fp contract(off)
    __shared__ uint2 L[BM_SC_LDS];
    __shared__ BmQword QW[BM_QW_LDS];
    const int64_t d0 = (int64_t)blockIdx.x * 256, d = d0 + threadIdx.x;
    const bool active = d < S.n_docs;
    const int64_t dn = d0 + 256 < S.n_docs ? d0 + 256 : S.n_docs;
    const uint32_t e0 = S.eoff[d0], e1 = S.eoff[dn];
    const bool staged = e1 - e0 <= (uint32_t)BM_SC_LDS;
    if (staged)
        for (uint32_t k = threadIdx.x; k < e1 - e0; k += 256) L[k] = S.ent[e0 + k];
    const int64_t dc = active ? d : d0;                       // (inactive lanes compute for a real document and write nothing)
    const uint32_t eb = S.eoff[dc] - e0, ne = S.eoff[dc + 1] - S.eoff[dc];
    double K, t0;
    bm_doc_factors(S, (double)S.dl[dc], K, t0);
    const unsigned long long sg[4] = {S.sig[dc * 4], S.sig[dc * 4 + 1], S.sig[dc * 4 + 2], S.sig[dc * 4 + 3]};
    const unsigned long long pkey = (unsigned long long)dc << 32;
    // the batch's words, BM_QW_LDS at a time, staged in LDS (term, signature bit, idf); queries end where their offsets say
    const int64_t jb = S.qoff[0], je = S.qoff[S.n_q];
    int64_t q = 0, qend = S.qoff[1];
    double score = 0.0;
    for (int64_t c0 = jb; c0 < je; c0 += BM_QW_LDS) {
        const int64_t cn = je - c0 < BM_QW_LDS ? je - c0 : BM_QW_LDS;
        __syncthreads();
        for (int64_t k = threadIdx.x; k < cn; k += 256) {
            const int32_t t = S.qterm[c0 + k];
            QW[k] = BmQword{t, t >= 0 ? bm_sig_bit((uint32_t)t) : 0u, S.qidf[c0 + k]};
        }
        __syncthreads();
        for (int64_t k = 0; k < cn; ++k) {
            while (c0 + k == qend) {                          // (uniform) query q is complete
                if (active) S.out[q * S.n_docs + d] = score;
                score = 0.0;
                ++q;
                qend = S.qoff[q + 1];
            }
            const BmQword qw = QW[k];
            uint32_t f = 0;
            if (qw.t >= 0) {
                const uint32_t bit = qw.bit;
                const unsigned long long word = bit < 64 ? sg[0] : bit < 128 ? sg[1] : bit < 192 ? sg[2] : sg[3];
                if ((word >> (bit & 63u)) & 1ull) {
                    if (staged) {
                        for (uint32_t e = 0; e < ne; ++e) {
                            const uint2 en = L[eb + e];
                            if (en.x == (uint32_t)qw.t) { f = en.y; break; }
                        }
                    } else {
                        const unsigned long long key = (pkey | (uint32_t)qw.t) + 1ull;
                        unsigned long long sl = bm_mix64(key) & S.pmask;
                        for (;;) {
                            const unsigned long long kk = S.ptab[sl].key;
                            if (kk == key) { f = S.ptab[sl].a; break; }
                            if (kk == 0ull) break;
                            sl = (sl + 1) & S.pmask;
                        }
                    }
                }
            }
            score = bm_word_score(S, score, f, K, t0, qw.idf);
        }
    }
    for (; q < S.n_q; ++q) {                                  // the last query, and empty queries at the end
        if (active) S.out[q * S.n_docs + d] = score;
        score = 0.0;
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
namespace {
unsigned bm_grid(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
}

void gz_launch_bm25(int step, const GzBm25Args& A, const uint32_t* list, int64_t n, uint32_t* next, hipStream_t s)
{
    switch (step) {
    case GZ_BM25_COUNT: if (A.n_docs > 0) hipLaunchKernelGGL(gz_bm25_count_kernel, dim3(bm_grid(A.n_docs, BM_WPB)), dim3(WAVE * BM_WPB), 0, s, A); break;
    case GZ_BM25_WORDS: if (A.n_docs > 0) hipLaunchKernelGGL(gz_bm25_words_kernel, dim3(bm_grid(A.n_docs, BM_WPB)), dim3(WAVE * BM_WPB), 0, s, A); break;
    case GZ_BM25_HASH: if (A.n_words > 0) hipLaunchKernelGGL(gz_bm25_hash_kernel, dim3(bm_grid(A.n_words, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_DEDUP_INS: if (n > 0) hipLaunchKernelGGL(gz_bm25_dedup_ins_kernel, dim3(bm_grid(n, 256)), dim3(256), 0, s, A, list, n); break;
    case GZ_BM25_DEDUP_RES: if (n > 0) hipLaunchKernelGGL(gz_bm25_dedup_res_kernel, dim3(bm_grid(n, 256)), dim3(256), 0, s, A, list, n, next); break;
    case GZ_BM25_FIRST: if (A.n_words > 0) hipLaunchKernelGGL(gz_bm25_first_kernel, dim3(bm_grid(A.n_words, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_TERM: if (A.n_words > 0) hipLaunchKernelGGL(gz_bm25_term_kernel, dim3(bm_grid(A.n_words, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_PAIR_INS: if (A.n_words > 0) hipLaunchKernelGGL(gz_bm25_pair_ins_kernel, dim3(bm_grid(A.n_words, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_PAIR_FIRST: if (A.n_words > 0) hipLaunchKernelGGL(gz_bm25_pair_first_kernel, dim3(bm_grid(A.n_words, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_DF: if (A.n_terms > 0) hipLaunchKernelGGL(gz_bm25_df_kernel, dim3(bm_grid(A.n_terms, 256)), dim3(256), 0, s, A); break;
    case GZ_BM25_ENT: {
        const int64_t m = A.n_words > A.n_docs + 1 ? A.n_words : A.n_docs + 1;
        hipLaunchKernelGGL(gz_bm25_ent_kernel, dim3(bm_grid(m, 256)), dim3(256), 0, s, A);
        break;
    }
    case GZ_BM25_KNOWN: if (A.n_words > 0) hipLaunchKernelGGL(gz_bm25_known_kernel, dim3(bm_grid(A.n_words, 256)), dim3(256), 0, s, A, next); break;
    default: break;
    }
}

void gz_launch_bm25_rehash(const GzBm25Slot* from, int64_t n_slots, GzBm25Slot* to, unsigned long long mask, hipStream_t s)
{
    if (n_slots > 0) hipLaunchKernelGGL(gz_bm25_rehash_kernel, dim3(bm_grid(n_slots, 256)), dim3(256), 0, s, from, n_slots, to, mask);
}

void gz_launch_bm25_remove(int step, const GzBm25Rm& R, hipStream_t s)
{
    switch (step) {
    case GZ_BM25_RM_MARK: if (R.n_ids > 0) hipLaunchKernelGGL(gz_bm25_rm_mark_kernel, dim3(bm_grid(R.n_ids, 256)), dim3(256), 0, s, R); break;
    case GZ_BM25_RM_COUNT: if (R.n_docs > 0) hipLaunchKernelGGL(gz_bm25_rm_count_kernel, dim3(bm_grid(R.n_docs, 256)), dim3(256), 0, s, R); break;
    case GZ_BM25_RM_DOCS: hipLaunchKernelGGL(gz_bm25_rm_docs_kernel, dim3(bm_grid(R.n_docs + 1, 256)), dim3(256), 0, s, R); break;
    case GZ_BM25_RM_ENT: if (R.n_docs > 0) hipLaunchKernelGGL(gz_bm25_rm_ent_kernel, dim3(bm_grid(R.n_docs, BM_WPB)), dim3(WAVE * BM_WPB), 0, s, R); break;
    case GZ_BM25_RM_SEQ: if (R.n_docs > 0) hipLaunchKernelGGL(gz_bm25_rm_seq_kernel, dim3(bm_grid(R.n_docs, BM_WPB)), dim3(WAVE * BM_WPB), 0, s, R); break;
    default: break;
    }
}

void gz_launch_bm25_compact(int step, const GzBm25Cp& C, hipStream_t s)
{
    switch (step) {
    case GZ_BM25_CP_FIRST: if (C.n_ent > 0) hipLaunchKernelGGL(gz_bm25_cp_first_kernel, dim3(bm_grid(C.n_ent, 256)), dim3(256), 0, s, C); break;
    case GZ_BM25_CP_FLAG: if (C.n_ent > 0) hipLaunchKernelGGL(gz_bm25_cp_flag_kernel, dim3(bm_grid(C.n_ent, 256)), dim3(256), 0, s, C); break;
    case GZ_BM25_CP_NEWID: if (C.n_terms > 0) hipLaunchKernelGGL(gz_bm25_cp_newid_kernel, dim3(bm_grid(C.n_terms, 256)), dim3(256), 0, s, C); break;
    case GZ_BM25_CP_GATHER: hipLaunchKernelGGL(gz_bm25_cp_gather_kernel, dim3(bm_grid(C.n_new + 1, 256)), dim3(256), 0, s, C); break;
    case GZ_BM25_CP_ENT: if (C.n_docs > 0) hipLaunchKernelGGL(gz_bm25_cp_ent_kernel, dim3(bm_grid(C.n_docs, BM_WPB)), dim3(WAVE * BM_WPB), 0, s, C); break;
    case GZ_BM25_CP_SEQ: if (C.n_words > 0) hipLaunchKernelGGL(gz_bm25_cp_seq_kernel, dim3(bm_grid(C.n_words, 256)), dim3(256), 0, s, C); break;
    default: break;
    }
}

void gz_launch_bm25_rekey(const GzBm25Slot* from, int64_t n_slots, const uint32_t* newid, GzBm25Slot* to, unsigned long long mask, hipStream_t s)
{
    if (n_slots > 0) hipLaunchKernelGGL(gz_bm25_rekey_kernel, dim3(bm_grid(n_slots, 256)), dim3(256), 0, s, from, n_slots, newid, to, mask);
}

void gz_launch_bm25_scan(const uint32_t* in, int64_t n, uint32_t* out, uint32_t* bsum, hipStream_t s)
{
    const int64_t nb = n > 0 ? (n + BM_SCAN_BLOCK - 1) / BM_SCAN_BLOCK : 0;
    if (nb > 0) hipLaunchKernelGGL(gz_bm25_scan_a_kernel, dim3((unsigned)nb), dim3(256), 0, s, in, n, bsum);
    hipLaunchKernelGGL(gz_bm25_scan_b_kernel, dim3(1), dim3(256), 0, s, bsum, nb, out + n);
    if (nb > 0) hipLaunchKernelGGL(gz_bm25_scan_c_kernel, dim3((unsigned)nb), dim3(256), 0, s, in, n, (const uint32_t*)bsum, out);
}

void gz_launch_bm25_lookup(const GzBm25Look& L, hipStream_t s)
{
    if (L.n > 0) hipLaunchKernelGGL(gz_bm25_lookup_kernel, dim3(bm_grid(L.n, 256)), dim3(256), 0, s, L);
}

void gz_launch_bm25_score(const GzBm25Score& S, hipStream_t s)
{
    if (S.n_docs > 0 && S.n_q > 0) hipLaunchKernelGGL(gz_bm25_score_kernel, dim3(bm_grid(S.n_docs, 256)), dim3(256), 0, s, S);
}
