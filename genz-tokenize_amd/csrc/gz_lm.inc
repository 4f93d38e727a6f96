// gz_lm.inc -- a token n-gram language model resident in HBM and the perplexity of ragged rows under it: the counts of every order
// 1..N in ONE table, and a backoff walk per token position (included by gz_kernels.hip behind gz_pieces.inc, whose body rule and
// piece walk it uses, and gz_ngram.inc, whose two hash streams it extends).
//
// THE RULE (include/genz_tokenize.h, "token n-gram language model and perplexity"): Stupid Backoff (Brants et al., 2007).  The body
// of a row is the row without its skips.  For k = 1..N, c(g) is the number of occurrences of the k-gram g in the training bodies (a
// k-gram never crosses a row; a body shorter than k has none) and T the number of training body tokens.  For a query body q of m ids
// and position i: K = min(i + 1, N); j = the largest k in 0..K with c(q[i-k+1 .. i]) > 0 (counts are monotone: j is the first k at
// which walking upward from k = 1 misses, minus one); num = c(q[i-j+1 .. i]), den = c(q[i-j+1 .. i-1]) (T when j = 1); j = 0: num = 1,
// den = T; back = K - j; cost = log2(den) - log2(num) + back * lam in float64, lam = -log2(alpha); fx = rint(cost * 2^24).  Per row:
// n_tokens = m, bits_fx = the sum of fx (an integer: no order of addition changes it), n_order[j] = positions with that j; per
// token, optionally, j, num and den.  A hash decides where to look, never whether two n-grams are equal: every tag match is followed
// by a comparison of the order and the k ids.
//
// THE HASH extends BACKWARDS, a step an order: H_1 = mix(seed, q[e]), H_k = mix(H_{k-1}, q[e-k+1]) -- gz_ngram.inc's two
// MurmurHash3_x86_32 streams, seeds 0 and 0x9E3779B9 -- so the N grams that end at a position share one chain: N steps a position,
// not N (N + 1) / 2, and a query that stops walking stops hashing.  The k-gram's h = fmix32(H_k ^ 4 k) of both streams, 64 bits, cut
// to its low lm_hash_bits bits when that switch is set; start slot = h & (slots - 1); tag = (h >> 32) with its low 3 bits replaced
// by k - 1.
//
// THE TABLE.  One open-addressing table, linear probing, all orders, 16 bytes a slot: a 64-bit key word tag << 32 | (end + 1) -- end
// = the global index of the gram's LAST id in the model's own copy of the training ids; 0 = free -- and a 32-bit count behind it.
// Slots: the smallest power of two that is at least twice the gram positions of all orders, so every probe ends at a free slot.
// INSERT: a free slot is claimed by 64-bit atomicCAS; on a taken slot whose tag (and so order) agrees, the k ids at the occupant's
// end are compared with the inserter's -- equal: atomicAdd on the count and done; otherwise the next slot.  A slot, once taken,
// holds ONE gram for good, so every occurrence of a gram ends in the same slot and its count is the number of its occurrences,
// whatever the order of the inserts.  Successful claims per order are the distinct grams.
//
// THE WALK.  Pieces of GZ_PIECE = 4096 END positions (gz_pieces.inc at width 1: every body token is a position), a wave a piece; a
// trip is 64 positions and lane l owns end position t + l.  Its up to N - 1 predecessor ids come from the lanes below it by wave
// shuffles, for the first lanes from the previous trip's ids, which the wave carries in a register; a piece that is not its row's
// first loads the 64 ids before its start (s0 >= 4096: never before the body's start).  No LDS.
// BUILD: for k = 1..K one hash step, then one insert.  With `combine` the equal unigrams and bigrams of a trip are added once: a
// ballot-match loop over the lanes' ids (the ids themselves, not their hash), the leader adding the population count.
// SCORE: k = 1 upward, one probe each, until the first miss or K; the loop ends for the wave when no lane walks.  den of order k is
// the count the lane BELOW found at order k - 1 (the (k-1)-gram that ends at i - 1): one shuffle an order, lane 0 from the
// previous trip's lane 63, carried wave-uniform; a piece that is not its row's first walks position s0 - 1 once more for that carry.
// So j, num and den come out of the walk with no probe beyond the miss, and an unseen token costs one probe.  Per trip the order
// histogram is a ballot and a population count an order; fx is summed a lane and reduced once a piece.  A row of one piece stores
// its sums plainly; the pieces of a longer row meet by integer atomicAdd in rows the launcher preset.  Every body token belongs to
// exactly one piece, which stores its per-token cells; the row's first piece stores the frame cells' zeros.
// Bounds: a gram of order k at end i is touched only when k <= K <= i + 1, so body[i - k + 1 .. i] lies inside the body; a slot's
// end was inserted under the same rule with the same k, so ref_ids[end - k + 1 .. end] lies inside a training body.

// the id d places before the lane's own (0 <= d < 64): from the trip's ids, for the first d lanes from the previous trip's
__device__ __forceinline__ uint32_t lm_pred(uint32_t cur, uint32_t prev, int lane, int d)
{
    const int src = (lane - d) & (WAVE - 1);
    const uint32_t x = (uint32_t)__shfl((int)cur, src, WAVE), y = (uint32_t)__shfl((int)prev, src, WAVE);
    return lane >= d ? x : y;
}

// x_end[-d] == y_end[-d] for d in 0..k-1
__device__ __forceinline__ bool lm_equal_back(const int32_t* __restrict__ x_end, const int32_t* __restrict__ y_end, int k)
{
    for (int d = 0; d < k; ++d) if (x_end[-d] != y_end[-d]) return false;
    return true;
}

__device__ __forceinline__ uint32_t lm_tag(uint64_t h, int k) { return ((uint32_t)(h >> 32) & ~7u) | (uint32_t)(k - 1); }

__device__ __forceinline__ uint64_t lm_wave_sum64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, WAVE);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

// Add `add` occurrences of the k-gram that ends at `end` of the model's id copy; 1 when this thread claimed a free slot.
__device__ __forceinline__ int lm_insert(const GzLmArgs& A, uint64_t h, int k, uint64_t end, uint32_t add)
{
    const uint32_t tag = lm_tag(h, k);
    const unsigned long long mine = (unsigned long long)tag << 32 | (unsigned long long)(end + 1);
    for (uint64_t s = h & A.mask;; s = (s + 1) & A.mask) {                            // (ends: the table is at most half full)
        unsigned long long* const slot = A.table + 2 * s;
        unsigned long long seen = __atomic_load_n(slot, __ATOMIC_RELAXED);            // (a taken slot stays as it is: no CAS on it)
        if (seen == 0ull) seen = atomicCAS(slot, 0ull, mine);
        const bool claimed = seen == 0ull;
        if (!claimed) {
            if ((uint32_t)(seen >> 32) != tag) continue;
            const uint64_t at = (uint64_t)(uint32_t)seen - 1u;
            if (!GZ_CHK(901, at, A.ref_n_ids) || !GZ_CHK(902, (uint64_t)(k - 1), at + 1)) continue;
            if (!lm_equal_back(A.ref_ids + at, A.ref_ids + end, k)) continue;
        }
        atomicAdd(reinterpret_cast<uint32_t*>(slot + 1), add);
        return claimed ? 1 : 0;
    }
}

// c(g) of the k-gram whose last id is *g_end, 0 when the model does not hold it
__device__ __forceinline__ uint32_t lm_probe(const GzLmArgs& A, uint64_t h, int k, const int32_t* __restrict__ g_end)
{
    const uint32_t tag = lm_tag(h, k);
    const ulonglong2* const table = reinterpret_cast<const ulonglong2*>(A.table);
    for (uint64_t s = h & A.mask;; s = (s + 1) & A.mask) {                            // (ends: the table is at most half full)
        const ulonglong2 v = table[s];                                               // key and count: one 16-byte load
        if (v.x == 0ull) return 0u;
        if ((uint32_t)(v.x >> 32) != tag) continue;
        const uint64_t at = (uint64_t)(uint32_t)v.x - 1u;
        if (!GZ_CHK(903, at, A.ref_n_ids) || !GZ_CHK(904, (uint64_t)(k - 1), at + 1)) continue;
        if (lm_equal_back(A.ref_ids + at, g_end, k)) return (uint32_t)v.y;
    }
}

// gram positions of every order, a thread a row: stats[k - 1] += max(0, m - k + 1)
__global__ __launch_bounds__(256) void gz_lm_count_kernel(const int64_t* __restrict__ row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                                                          int32_t order, unsigned long long* __restrict__ stats)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t m = 0;
    if (r < n_rows) piece_body(row_off, r, skip_front, skip_back, &m);
    if (m >= ((int64_t)1 << 31)) m = 0;                                              // (the piece count refuses the call)
    for (int k = 1; k <= order; ++k) {                                               // (every lane stays for the shuffles)
        const int64_t g = m >= k ? m - k + 1 : 0;
        const int lo = wave_sum((int)(g & 0xFFFF)), hi = wave_sum((int)(g >> 16));
        if (lane_id() == 0 && (lo | hi)) atomicAdd(stats + (k - 1), (unsigned long long)lo + ((unsigned long long)hi << 16));
    }
}

// BUILD: A.ids / A.row_off are the caller's rows (absolute offsets); a gram's end counts from A.off0 into the model's copy A.ref_ids
template <bool COMBINE>
__global__ __launch_bounds__(WAVE * 4) void gz_lm_build_kernel(GzLmArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t j, n_pc, m;
    const int64_t r = piece_row(A, p, &j, &n_pc);
    const int64_t a = piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
    const int64_t s0 = j * GZ_PIECE, s1 = s0 + GZ_PIECE < m ? s0 + GZ_PIECE : m;
    const int32_t* const body = A.ids + a;                                           // (never read when m == 0)
    const int N = A.order;
    uint32_t prev = j > 0 ? (uint32_t)body[s0 - WAVE + lane] : 0u;
    int claimed[GZ_LM_MAX_ORDER] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t t = s0; t < s1; t += WAVE) {                                        // (wave-uniform bounds: every lane stays for the shuffles)
        const int64_t i = t + lane;
        const bool live = i < s1;
        const uint32_t cur = live ? (uint32_t)body[i] : 0u;
        const int K = !live ? 0 : (i + 1 < N ? (int)(i + 1) : N);
        const uint64_t end = (uint64_t)(a - A.off0 + i);
        uint32_t h1 = 0u, h2 = NG_SEED2, x1 = 0u;
#pragma unroll
        for (int k = 1; k <= GZ_LM_MAX_ORDER; ++k) {
            if (k > N) break;
            const uint32_t x = k == 1 ? cur : lm_pred(cur, prev, lane, k - 1);
            if (k == 2) x1 = x;
            ng_mix(h1, h2, x);
            const uint64_t h = ng_finish(h1, h2, k) & A.hmask;
            if (COMBINE && k <= 2) {                                                 // equal grams of the trip: the first lane of each adds them all
                uint64_t todo = wballot(k <= K);
                uint32_t add = 0u;
                while (todo) {
                    const int L = __builtin_ctzll(todo);
                    const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)cur, L), l1 = (uint32_t)__builtin_amdgcn_readlane((int)x1, L);
                    const uint64_t same = wballot(k <= K && cur == l0 && (k == 1 || x1 == l1));
                    if (lane == L) add = (uint32_t)__builtin_popcountll(same);
                    todo &= ~same;
                }
                if (add) claimed[k - 1] += lm_insert(A, h, k, end, add);
            } else if (k <= K) claimed[k - 1] += lm_insert(A, h, k, end, 1u);
        }
        prev = cur;
    }
#pragma unroll
    for (int k = 0; k < GZ_LM_MAX_ORDER; ++k) {
        if (k >= N) break;
        const int c = wave_sum(claimed[k]);
        if (lane == 0 && c) atomicAdd(A.stats + k, (unsigned long long)c);
    }
}

// The walk of one trip: lane's end position holds `cur`, K = the longest gram it may use (0: the lane does not walk); g_end = the
// address of its own id.  carry[k - 1] = c of the k-gram that ends one position before the trip (wave-uniform), replaced by this
// trip's lane 63's.  *jj, *num, *den as the rule names them.
__device__ __forceinline__ void lm_walk(const GzLmArgs& A, uint32_t cur, uint32_t prev, int lane, int K, const int32_t* __restrict__ g_end,
                                        uint32_t (&carry)[GZ_LM_MAX_ORDER], int* jj, uint32_t* num, uint32_t* den)
{
    const int N = A.order;
    uint32_t next[GZ_LM_MAX_ORDER] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t h1 = 0u, h2 = NG_SEED2, below = A.T;                                     // below: c of the (k-1)-gram that ends at i - 1; T for k = 1
    bool alive = K >= 1;
    *jj = 0; *num = 1u; *den = A.T;
#pragma unroll
    for (int k = 1; k <= GZ_LM_MAX_ORDER; ++k) {
        if (k > N || !wballot(alive)) break;                                         // (wave-uniform: every lane stays for the shuffles)
        const uint32_t x = k == 1 ? cur : lm_pred(cur, prev, lane, k - 1);
        ng_mix(h1, h2, x);
        uint32_t c = 0u;
        if (alive && k <= K) c = lm_probe(A, ng_finish(h1, h2, k) & A.hmask, k, g_end);
        alive = c != 0u;
        if (c) { *jj = k; *num = c; *den = below; }
        const uint32_t up = (uint32_t)__shfl_up((int)c, 1, WAVE);
        below = lane == 0 ? carry[k - 1] : up;
        next[k - 1] = (uint32_t)__builtin_amdgcn_readlane((int)c, WAVE - 1);
    }
#pragma unroll
    for (int k = 0; k < GZ_LM_MAX_ORDER; ++k) carry[k] = next[k];
}

// SCORE: A.ids / A.row_off are the caller's rows (absolute offsets); the table and A.ref_ids are the model's
__global__ __launch_bounds__(WAVE * 4) void gz_lm_score_kernel(GzLmArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t j, n_pc, m;
    const int64_t r = piece_row(A, p, &j, &n_pc);
    const int64_t a = piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
    const int64_t s0 = j * GZ_PIECE, s1 = s0 + GZ_PIECE < m ? s0 + GZ_PIECE : m;
    const int32_t* const body = A.ids + a;                                           // (never read when m == 0)
    const int N = A.order;
    if (j == 0) {
        if (lane == 0 && A.n_tokens) A.n_tokens[r] = (int32_t)m;
        const int64_t lo = A.row_off[r], hi = A.row_off[r + 1];                      // the frame cells: in no body
        if (hi > lo && ((lane == 0 && A.skip_front) || (lane == 1 && A.skip_back))) {
            const int64_t cell = lane == 0 ? lo : hi - 1;
            if (A.token_order) A.token_order[cell] = 0;
            if (A.token_num) A.token_num[cell] = 0u;
            if (A.token_den) A.token_den[cell] = 0u;
        }
    }
    uint32_t carry[GZ_LM_MAX_ORDER] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t prev = 0u;
    int jj;
    uint32_t num, den;
    if (j > 0) {                                                                     // position s0 - 1 once more, lane 63 alone, orders 1..N-1: the carries
        prev = (uint32_t)body[s0 - WAVE + lane];
        if (N > 1) lm_walk(A, prev, 0u, lane, lane == WAVE - 1 ? N - 1 : 0, body + (s0 - WAVE + lane), carry, &jj, &num, &den);
    }
    uint64_t bits = 0ull;
    int hist[GZ_LM_MAX_ORDER + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t t = s0; t < s1; t += WAVE) {                                        // (wave-uniform bounds: every lane stays for the shuffles and ballots)
        const int64_t i = t + lane;
        const bool live = i < s1;
        const uint32_t cur = live ? (uint32_t)body[i] : 0u;
        const int K = !live ? 0 : (i + 1 < N ? (int)(i + 1) : N);
        lm_walk(A, cur, prev, lane, K, body + i, carry, &jj, &num, &den);
        if (live) {
            const double cost = log2((double)den) - log2((double)num) + (double)(K - jj) * A.lam;
            bits += (uint64_t)__double2ll_rn(cost * 16777216.0);
            if (A.token_order) A.token_order[a + i] = (uint8_t)jj;
            if (A.token_num) A.token_num[a + i] = num;
            if (A.token_den) A.token_den[a + i] = den;
        }
#pragma unroll
        for (int k = 0; k <= GZ_LM_MAX_ORDER; ++k) {
            if (k > N) break;
            hist[k] += __builtin_popcountll(wballot(live && jj == k));
        }
        prev = cur;
    }
    bits = lm_wave_sum64(bits);
    if (lane != 0) return;
    if (n_pc == 1) {
        if (A.bits_fx) A.bits_fx[r] = bits;
    } else if (A.bits_fx && bits) atomicAdd(A.bits_fx + r, (unsigned long long)bits);
    if (!A.n_order) return;
#pragma unroll
    for (int k = 0; k <= GZ_LM_MAX_ORDER; ++k) {
        if (k > N) break;
        if (n_pc == 1) A.n_order[(int64_t)k * A.n_rows + r] = hist[k];
        else if (hist[k]) atomicAdd(A.n_order + (int64_t)k * A.n_rows + r, hist[k]);
    }
}
