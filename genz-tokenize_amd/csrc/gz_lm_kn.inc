// gz_lm_kn.inc -- interpolated modified Kneser-Ney (Chen & Goodman 1998; Heafield et al. 2013) over the n-gram model of gz_lm.inc: two
// derivation passes over the table's slots into a sidecar, and a scoring walk that carries a context's statistics from lane to lane
// (included by gz_kernels.hip behind gz_lm.inc, whose hash chain, tag, id comparison, predecessor shuffles and piece walk it uses).
//
// THE RULE (include/genz_tokenize.h, "modified Kneser-Ney perplexity", verbatim).  The model is a gz_ngram_lm of order N with c(g) and
// the distinct grams of each order as they are.
// ADJUSTED COUNTS.  For a distinct k-gram g: L(g) = the number of distinct (k+1)-grams of the model whose last k ids are g (its distinct
// left neighbours; L = 0 for k = N).  a(g) = c(g) if k = N, else max(L(g), 1): a gram seen only at the starts of bodies has no left
// neighbour and counts as one type, so every gram the model holds has a >= 1.
// CONTEXT STATISTICS.  For a context x (a (k-1)-gram; the empty gram for k = 1), over the distinct k-grams x.w of the model:
// A(x) = the sum of a(x.w); F_j(x) = the number of them with min(a, 3) = j, j = 1, 2, 3.  The empty context's four numbers are global.
// V = the number of distinct unigrams.
// DISCOUNTS.  Per order k, n_j(k) = the number of distinct k-grams with a = j, j = 1..4.  Y = n1 / (n1 + 2 n2); D_k1 = 1 - 2 Y n2 / n1,
// D_k2 = 2 - 3 Y n3 / n2, D_k3 = 3 - 4 Y n4 / n3.  The fallback (0.5, 1, 1.5) holds for an order when any of n1..n4 is 0 or some D_kj is
// not in (0, j) (KenLM's --discount_fallback).  Computed on the host in float64 from the 4 N integers (gz_rowrules.h, lm_kn_discounts); a
// caller may pass its own [N, 3], each in (0, j].
// SCORE.  For a query body q, position i, K = min(i + 1, N): p_0 = 1 / (V + 1).  For k = 1..K let x = q[i-k+1 .. i-1] and g = x.q[i].
// If k > 1 and the model does not hold x, or if A(x) = 0 (x occurs only at body ends), stop: the result is p_{k-1}.  Else
// p_k = ( max(a(g) - D_k,min(a(g),3), 0) + (D_k1 F_1(x) + D_k2 F_2(x) + D_k3 F_3(x)) p_{k-1} ) / A(x), with a(g) = 0 and no discount when g
// is unseen: the walk goes on through seen contexts after the token's own gram has missed.  j = the largest k with g seen.
// cost = -log2(p) in float64; fx = rint(min(cost, 120) 2^24).  Per row n_tokens, bits_fx (the uint64 sum of fx), n_order [N + 1, rows]; per
// token, optionally, token_order uint8 and token_bits_fx uint32.
//
// THE SIDECAR.  Two arrays parallel to the table's slots, owned by the model, 20 bytes a slot: left[s] = L of the slot's gram (uint32), and
// rec[s] = {A, F1, F2, F3} of the slot's gram AS A CONTEXT (four uint32, one 16-byte load).  The empty context's record and the counts of
// counts n_j(k) are 4 + 4 N cells the host reads back.  The table's slots and the id copy are read, never written.
// PASS 1, left neighbours, a lane a slot: a taken slot of order k >= 2 with end e hashes the (k-1)-gram that ends at e -- k - 1 steps of
// the chain the gram itself was inserted under -- probes for it and adds 1 to its L.  The suffix is in the table (counts are monotone).
// PASS 2, context statistics, a launch of its own since L must be complete, a lane a slot: a from c or L; the (k-1)-gram that ends at
// e - 1 (a fresh chain) gets a added to its A and 1 to its F_min(a,3).  The unigrams' go to the global cells, summed in the wave first
// (every unigram has the one empty context: V atomics on four cells otherwise).  Counts of counts: the lanes with a <= 4 name a cell
// 4 (k - 1) + a - 1; a ballot-match loop adds each distinct cell of the wave once.  No combining of equal contexts in the wave: a wave's
// 64 slots are hash neighbours, so equal targets are rare.
// THE WALK has gz_lm_score_kernel's shape: a wave a piece of 4096 end positions, a trip of 64, lane l owns end t + l.  Per order k one
// probe of the lane's own gram while every lower order was found; the probe returns the SLOT, from which a (the count for k = N, left
// for k < N) and, for k < N, the record are loaded.  The context of order k + 1 at position i is the k-gram that ends at i - 1: the lane
// BELOW's own gram, so its found flag and record come up by five shuffles an order; lane 0 takes them from the previous trip's lane 63,
// carried wave-uniform per order, and a piece that is not its row's first walks position s0 - 1 once more, lane 63 alone, for that
// carry.  The recursion step is done in the lane in float64.  The wave leaves the loop when no lane walks and no lane's context is found.
// No LDS.
// Bounds: as gz_lm.inc's; a sidecar index is a slot index the probe loop returned (below slots), or nothing is touched.

constexpr uint64_t LM_NONE = ~0ull;

// the slot of the k-gram whose last id is *g_end and its count, LM_NONE when the model does not hold it
__device__ __forceinline__ uint64_t lm_find(const GzLmArgs& A, uint64_t h, int k, const int32_t* __restrict__ g_end, uint32_t* count)
{
    const uint32_t tag = lm_tag(h, k);
    const ulonglong2* const table = reinterpret_cast<const ulonglong2*>(A.table);
    for (uint64_t s = h & A.mask;; s = (s + 1) & A.mask) {                            // (ends: the table is at most half full)
        const ulonglong2 v = table[s];
        if (v.x == 0ull) return LM_NONE;
        if ((uint32_t)(v.x >> 32) != tag) continue;
        const uint64_t at = (uint64_t)(uint32_t)v.x - 1u;
        if (!GZ_CHK(905, at, A.ref_n_ids) || !GZ_CHK(906, (uint64_t)(k - 1), at + 1)) continue;
        if (lm_equal_back(A.ref_ids + at, g_end, k)) { *count = (uint32_t)v.y; return s; }
    }
}

// the slot of the n-gram (n >= 1) whose last id is *g_end, hashed from its end; LM_NONE when the model does not hold it
__device__ __forceinline__ uint64_t lm_find_serial(const GzLmArgs& A, int n, const int32_t* __restrict__ g_end)
{
    uint32_t h1 = 0u, h2 = NG_SEED2, c;
    for (int d = 0; d < n; ++d) ng_mix(h1, h2, (uint32_t)g_end[-d]);
    return lm_find(A, ng_finish(h1, h2, n) & A.hmask, n, g_end, &c);
}

// the order (0: a free slot, or one past the table) and the end of slot s's gram; the count behind it
__device__ __forceinline__ int lm_slot_gram(const GzLmKnArgs& K, uint64_t s, uint64_t* end, uint32_t* count)
{
    if (s >= K.slots) return 0;
    const ulonglong2 v = reinterpret_cast<const ulonglong2*>(K.M.table)[s];
    if (v.x == 0ull) return 0;
    const int k = (int)((uint32_t)(v.x >> 32) & 7u) + 1;
    *end = (uint64_t)(uint32_t)v.x - 1u;
    *count = (uint32_t)v.y;
    if (!GZ_CHK(907, *end, K.M.ref_n_ids) || !GZ_CHK(908, (uint64_t)(k - 1), *end + 1)) return 0;
    return k;
}

// PASS 1: L of every gram, a lane a slot
__global__ __launch_bounds__(256) void gz_lm_kn_left_kernel(GzLmKnArgs K)
{
    uint64_t e;
    uint32_t c;
    const int k = lm_slot_gram(K, (uint64_t)blockIdx.x * 256 + threadIdx.x, &e, &c);
    if (k < 2) return;
    const uint64_t at = lm_find_serial(K.M, k - 1, K.M.ref_ids + e);                  // the suffix: the (k-1)-gram that ends at e
    if (at == LM_NONE) { (void)GZ_CHK(909, at, K.slots); return; }                    // (never: counts are monotone)
    atomicAdd(K.left + at, 1u);
}

// PASS 2: {A, F1, F2, F3} of every context and the counts of counts, a lane a slot (every lane stays for the ballots)
__global__ __launch_bounds__(256) void gz_lm_kn_context_kernel(GzLmKnArgs K)
{
    const int lane = lane_id(), N = K.M.order;
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t e = 0;
    uint32_t a = 0u;
    const int k = lm_slot_gram(K, s, &e, &a);
    if (k >= 1 && k < N) { const uint32_t L = K.left[s]; a = L > 1u ? L : 1u; }
    const uint32_t j = a < 3u ? a : 3u;
    if (k >= 2) {
        const uint64_t at = lm_find_serial(K.M, k - 1, K.M.ref_ids + e - 1);          // the context: the (k-1)-gram that ends at e - 1
        if (at == LM_NONE) (void)GZ_CHK(910, at, K.slots);                            // (never: counts are monotone)
        else { atomicAdd(K.rec + 4 * at, a); atomicAdd(K.rec + 4 * at + j, 1u); }
    }
    const bool uni = k == 1;                                                         // the empty context's record: summed in the wave
    if (wballot(uni)) {
        const uint64_t sum = lm_wave_sum64(uni ? (uint64_t)a : 0ull);
#pragma unroll
        for (uint32_t f = 1; f <= 3; ++f) {
            const int n = __builtin_popcountll(wballot(uni && j == f));
            if (lane == 0 && n) atomicAdd(K.cells + f, (unsigned long long)n);
        }
        if (lane == 0) atomicAdd(K.cells, (unsigned long long)sum);
    }
    const int cell = k >= 1 && a <= 4u ? 4 * (k - 1) + (int)a - 1 : -1;               // counts of counts: each distinct cell of the wave once
    uint64_t todo = wballot(cell >= 0);
    while (todo) {
        const int first = __builtin_ctzll(todo);
        const uint64_t same = wballot(cell == __builtin_amdgcn_readlane(cell, first));
        if (lane == first) atomicAdd(K.cells + 4 + cell, (unsigned long long)__builtin_popcountll(same));
        todo &= ~same;
    }
}

// what the walk hands from the previous trip's lane 63 to lane 0: per order k, at [k - 1], whether the k-gram that ends one position
// before the trip is held (bit k - 1 of found) and its record as a context.  Wave-uniform.
struct LmKnCarry { uint32_t found, A[GZ_LM_MAX_ORDER], F1[GZ_LM_MAX_ORDER], F2[GZ_LM_MAX_ORDER], F3[GZ_LM_MAX_ORDER]; };

__device__ __forceinline__ uint32_t lm_from_below(uint32_t v, uint32_t lane0, int lane)
{
    const uint32_t up = (uint32_t)__shfl_up((int)v, 1, WAVE);
    return lane == 0 ? lane0 : up;
}

// The walk of one trip: lane's end position holds `cur`, K = the longest gram it may use (0: the lane does not walk); g_end = the
// address of its own id.  *jj and *pp as the rule names j and p.
__device__ __forceinline__ void lm_kn_walk(const GzLmKnArgs& Kn, uint32_t cur, uint32_t prev, int lane, int K, const int32_t* __restrict__ g_end,
                                           LmKnCarry& carry, int* jj, double* pp)
{
    const GzLmArgs& A = Kn.M;
    const int N = A.order;
    LmKnCarry next = {};
    uint32_t h1 = 0u, h2 = NG_SEED2;
    bool alive = K >= 1, going = K >= 1;                                             // alive: every lower order of the own gram was found; going: no stop yet
    uint32_t cf = 1u, cA = Kn.A0, c1 = Kn.F0[0], c2 = Kn.F0[1], c3 = Kn.F0[2];        // the context of order k: held?, its record (k = 1: the empty one)
    double p = Kn.p0;
    *jj = 0;
#pragma unroll
    for (int k = 1; k <= GZ_LM_MAX_ORDER; ++k) {
        if (k > N || !wballot((alive || (going && cf)) && k <= K)) break;            // (wave-uniform: every lane stays for the shuffles)
        const uint32_t x = k == 1 ? cur : lm_pred(cur, prev, lane, k - 1);
        ng_mix(h1, h2, x);
        uint32_t a = 0u, found = 0u, rA = 0u, r1 = 0u, r2 = 0u, r3 = 0u;             // the own gram of order k: a (0: unseen), and its record as a context
        if (alive && k <= K) {
            uint32_t c = 0u;
            const uint64_t s = lm_find(A, ng_finish(h1, h2, k) & A.hmask, k, g_end, &c);
            if (s != LM_NONE) {
                found = 1u;
                if (k == N) a = c;
                else {
                    const uint32_t L = Kn.left[s];
                    const uint4 r = reinterpret_cast<const uint4*>(Kn.rec)[s];
                    a = L > 1u ? L : 1u; rA = r.x; r1 = r.y; r2 = r.z; r3 = r.w;
                }
            }
        }
        alive = found != 0u;
        if (found) *jj = k;
        going = going && k <= K && cf && cA != 0u;
        if (going) {
            const double* const D = Kn.D[k - 1];
            const double gamma = D[0] * (double)c1 + D[1] * (double)c2 + D[2] * (double)c3;
            const double d = a == 1u ? D[0] : (a == 2u ? D[1] : D[2]);
            const double num = a ? fmax((double)a - d, 0.0) : 0.0;
            p = (num + gamma * p) / (double)cA;
        }
        cf = lm_from_below(found, (carry.found >> (k - 1)) & 1u, lane);              // the context of order k + 1: the lane below's gram of order k
        cA = lm_from_below(rA, carry.A[k - 1], lane);
        c1 = lm_from_below(r1, carry.F1[k - 1], lane);
        c2 = lm_from_below(r2, carry.F2[k - 1], lane);
        c3 = lm_from_below(r3, carry.F3[k - 1], lane);
        next.found |= (uint32_t)__builtin_amdgcn_readlane((int)found, WAVE - 1) << (k - 1);
        next.A[k - 1] = (uint32_t)__builtin_amdgcn_readlane((int)rA, WAVE - 1);
        next.F1[k - 1] = (uint32_t)__builtin_amdgcn_readlane((int)r1, WAVE - 1);
        next.F2[k - 1] = (uint32_t)__builtin_amdgcn_readlane((int)r2, WAVE - 1);
        next.F3[k - 1] = (uint32_t)__builtin_amdgcn_readlane((int)r3, WAVE - 1);
    }
    carry = next;
    *pp = p;
}

// SCORE: Kn.M.ids / row_off are the caller's rows (absolute offsets); the table, the sidecar and Kn.M.ref_ids are the model's
__global__ __launch_bounds__(WAVE * 4) void gz_lm_kn_score_kernel(GzLmKnArgs Kn)
{
    const GzLmArgs& A = Kn.M;
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
            if (Kn.token_bits_fx) Kn.token_bits_fx[cell] = 0u;
        }
    }
    LmKnCarry carry = {};
    uint32_t prev = 0u;
    int jj;
    double pr;
    if (j > 0) {                                                                     // position s0 - 1 once more, lane 63 alone, orders 1..N-1: the carries
        prev = (uint32_t)body[s0 - WAVE + lane];
        if (N > 1) lm_kn_walk(Kn, prev, 0u, lane, lane == WAVE - 1 ? N - 1 : 0, body + (s0 - WAVE + lane), carry, &jj, &pr);
    }
    uint64_t bits = 0ull;
    int hist[GZ_LM_MAX_ORDER + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t t = s0; t < s1; t += WAVE) {                                        // (wave-uniform bounds: every lane stays for the shuffles and ballots)
        const int64_t i = t + lane;
        const bool live = i < s1;
        const uint32_t cur = live ? (uint32_t)body[i] : 0u;
        const int K = !live ? 0 : (i + 1 < N ? (int)(i + 1) : N);
        lm_kn_walk(Kn, cur, prev, lane, K, body + i, carry, &jj, &pr);
        if (live) {
            const double cost = fmin(fmax(-log2(pr), 0.0), 120.0);                   // (p <= 1 but for its roundings)
            const uint32_t fx = (uint32_t)__double2ll_rn(cost * 16777216.0);
            bits += fx;
            if (A.token_order) A.token_order[a + i] = (uint8_t)jj;
            if (Kn.token_bits_fx) Kn.token_bits_fx[a + i] = fx;
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
