// gz_repeat.inc -- n-gram repetition INSIDE a document: per row and width, how many n-grams there are, how many different ones, how
// many positions hold an n-gram that occurs twice or more, how many tokens lie inside such an n-gram, and the most frequent n-gram
// (included by gz_kernels.hip behind gz_pieces.inc, whose body rule, n-gram rule and piece walk it uses, and gz_ngram.inc, whose
// hash, comparison and coverage by ballots and shifts it shares).
//
// The rule (include/genz_tokenize.h, "repeats: n-gram repetition inside a document"): the body q of a row is the row without its
// skips, m ids; for width n its n-grams are the G = max(0, m - n + 1) runs q[i:i+n]; c(g) = the positions whose n-gram is g
// (occurrences may overlap), first(g) the smallest of them.  n_grams = G; n_distinct = different n-grams; n_repeated = positions i
// with c(q[i:i+n]) >= 2; n_covered = body tokens t with some repeated i, i <= t < i + n; top_count = max c(g) (0 when G == 0);
// top_pos = first(g) of the n-gram with the largest count, among equal counts the smallest first (-1 when G == 0); covered: bit k of
// the uint16 of a token = covered at widths[k].  A row's outputs depend on its own body and the widths alone.  A hash decides where
// to look, never whether two n-grams are equal, nor whether they stand in the same row.
//
// THE TABLE.  One table a call, cleared per width: open addressing, linear probing, slots = the smallest power of two that is at
// least twice the call's n-gram positions at the SMALLEST width (no width has more), so it is never more than half full and every
// probe ends.  A slot is 8 bytes, tag << 32 | (position + 1), position = the index of the n-gram's first id in the caller's flat ids
// relative to row_off[0], 0 = free; and 4 bytes in a parallel array, the occurrence count.  The key of a slot is (row, n-gram).
// THE HASH.  ng_trip_hash of the n ids, then the row mixed in: h ^= rp_row_mix(r), the finalizer of splitmix64 over
// r + 0x9E3779B97F4A7C15; h &= hmask (the switch repeat_hash_bits; all ones in the product); tag = h >> 32; start slot = h & (slots - 1).
// INSERT: 64-bit atomicCAS on a free slot; on a taken slot whose tag agrees the occupant is the same key only if its position lies
// inside this row's n-gram positions [lo, lo + G) AND the n ids there equal the inserter's: then the slot is lowered to the smaller
// position by the 64-bit atomicMin (equal tags: the packed order is the position order); otherwise the next slot.  Then
// atomicAdd(count[slot], 1) on the slot the occurrence ended in.  A slot, once taken, holds one key for good, so every occurrence of a
// key ends in the same slot, whatever the order: the slot ends at first(g) and the count at c(g).
// QUERY: every position probes and reads (first, c).  repeated = c >= 2; distinct += first == own position; the row's top key
// c << 32 | (0xFFFFFFFF - first_in_body) is a maximum: more occurrences win, then the smaller first position.  Coverage comes from
// ballot(repeated) exactly as gz_ngram_query_kernel derives it from its hits.
//
// PIECES (gz_pieces.inc) are those of the SMALLEST width for every width (one count pass): piece j of a row takes positions [4096 j, 4096 (j + 1))
// below G and owns the tokens of that range; the row's last piece owns the tokens up to m.  At a larger width a piece's last
// positions, or all of them, may lie at or beyond G: they are tail tokens, covered through the carry.  A piece that is not its row's
// first evaluates the n - 1 positions before its start once more, for the carry only.  Every body token belongs to exactly one
// piece at every width, which is why bit k of `covered` needs no atomic: width 0 stores the uint16, later widths OR into it, and the
// widths run in stream order.  A row of one piece stores its counts and its top plainly; the pieces of a longer row meet by 32-bit
// atomicAdd in rows the launcher preset and by the 64-bit atomicMax in a preset cell, which a last pass unpacks: integer operations
// that do not depend on order.
// Bounds: a position i is inserted and probed only when i < G, so q[i .. i + n) lies inside the body; a slot's position was inserted
// under the same rule and is compared only when it lies in [lo, lo + G) of the SAME row.  Look-back trips start at s0 - 64 >= 4032.

__device__ __forceinline__ uint64_t rp_row_mix(int64_t r)
{
    uint64_t x = (uint64_t)r + 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, WAVE);
        const uint64_t y = (uint64_t)hi << 32 | lo;
        v = y > v ? y : v;
    }
    return v;
}

// One occurrence of the n-gram at position pos (relative to off0) of a row whose n-gram positions are [lo, lo + n_g).
__device__ __forceinline__ void rp_insert(const GzRepeatArgs& A, uint64_t h, uint32_t pos, uint32_t lo, uint32_t n_g)
{
    const int32_t* const base = A.ids + A.off0;
    const uint32_t tag = (uint32_t)(h >> 32);
    const unsigned long long mine = (unsigned long long)tag << 32 | (unsigned long long)(pos + 1u);
    uint64_t s = h & A.mask;
    for (;; s = (s + 1) & A.mask) {                                                   // (ends: the table is at most half full)
        const unsigned long long seen = atomicCAS(A.table + s, 0ull, mine);
        if (seen == 0ull) break;
        if ((uint32_t)(seen >> 32) != tag) continue;
        const uint32_t q = (uint32_t)seen - 1u;
        if (q - lo < n_g && ng_equal(base + q, base + pos, A.n)) {                    // (unsigned: q < lo wraps beyond n_g < 2^31)
            atomicMin(A.table + s, mine);
            break;
        }
    }
    atomicAdd(A.count + s, 1u);
}

// (first position + 1, occurrences) of the n-gram at position pos of that row; every probed position was inserted
__device__ __forceinline__ uint32_t rp_probe(const GzRepeatArgs& A, uint64_t h, uint32_t pos, uint32_t lo, uint32_t n_g, uint32_t* c)
{
    const int32_t* const base = A.ids + A.off0;
    const uint32_t tag = (uint32_t)(h >> 32);
    for (uint64_t s = h & A.mask;; s = (s + 1) & A.mask) {                            // (ends: the table is at most half full)
        const unsigned long long v = A.table[s];
        if (v == 0ull) { *c = 0u; return 0u; }                                        // (never: pos was inserted)
        if ((uint32_t)(v >> 32) != tag) continue;
        const uint32_t q = (uint32_t)v - 1u;
        if (q - lo < n_g && ng_equal(base + q, base + pos, A.n)) { *c = A.count[s]; return (uint32_t)v; }
    }
}

// the piece of wave p at width A.n: *r its row, *a its body's first id (absolute), *m the body's ids, *n_g its n-grams, [*s0, *s1)
// the positions the piece takes (empty when *s1 <= *s0), *tok_end the end of the tokens it owns
__device__ __forceinline__ void rp_piece(const GzRepeatArgs& A, int64_t p, int64_t* r, int64_t* a, int64_t* m, int64_t* n_g, int64_t* s0,
                                         int64_t* s1, int64_t* tok_end, int64_t* j, int64_t* n_pc)
{
    *r = piece_row(A, p, j, n_pc);
    *a = piece_body(A.row_off, *r, A.skip_front, A.skip_back, m);
    *n_g = piece_grams(*m, A.n);
    *s0 = *j * GZ_PIECE;
    *s1 = *s0 + GZ_PIECE < *n_g ? *s0 + GZ_PIECE : *n_g;
    *tok_end = *j == *n_pc - 1 ? *m : *s0 + GZ_PIECE;                            // the last piece owns the tail, which starts no n-gram
}

__global__ __launch_bounds__(WAVE * 4) void gz_repeat_insert_kernel(GzRepeatArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t r, a, m, n_g, s0, s1, tok_end, j, n_pc;
    rp_piece(A, p, &r, &a, &m, &n_g, &s0, &s1, &tok_end, &j, &n_pc);
    const int32_t* const body = A.ids + a;                                           // (never read when m == 0)
    const uint64_t rmix = rp_row_mix(r);
    const uint32_t lo = (uint32_t)(a - A.off0);
    for (int64_t t = s0; t < s1; t += WAVE) {                                        // (wave-uniform bounds: every lane stays for the shuffles)
        const uint64_t h = (ng_trip_hash(body, m, t, lane, A.n) ^ rmix) & A.hmask;
        if (t + lane < s1) rp_insert(A, h, lo + (uint32_t)(t + lane), lo, (uint32_t)n_g);
    }
}

__global__ __launch_bounds__(WAVE * 4) void gz_repeat_query_kernel(GzRepeatArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t r, a, m, n_g, s0, s1, tok_end, j, n_pc;
    rp_piece(A, p, &r, &a, &m, &n_g, &s0, &s1, &tok_end, &j, &n_pc);
    const int32_t* const body = A.ids + a;                                           // (never read when m == 0)
    const uint64_t rmix = rp_row_mix(r);
    const uint32_t lo = (uint32_t)(a - A.off0);
    const uint16_t bit = (uint16_t)(1u << A.k);
    if (j == 0) {
        if (lane == 0 && A.n_grams) A.n_grams[r] = (int32_t)n_g;
        if (A.covered && A.k == 0) {                                                 // the frame cells: in no body, never covered
            const int64_t b = A.row_off[r], e = A.row_off[r + 1];
            if (lane == 0 && A.skip_front && e > b) A.covered[b] = 0;
            if (lane == 1 && A.skip_back && e > b) A.covered[e - 1] = 0;
        }
    }
    uint64_t prev = 0ull;                                                            // repeated bits of the 64 positions before the trip
    if (j > 0 && A.n > 1) {                                                          // the n - 1 positions before the piece: the carry only
        const int64_t t = s0 - WAVE;
        const uint64_t h = (ng_trip_hash(body, m, t, lane, A.n) ^ rmix) & A.hmask;
        uint32_t c = 0u;
        if (lane >= WAVE - (A.n - 1) && t + lane < n_g) rp_probe(A, h, lo + (uint32_t)(t + lane), lo, (uint32_t)n_g, &c);
        prev = wballot(c >= 2u);
    }
    int n_rep = 0, n_cov = 0, n_dis = 0;
    uint64_t top = 0ull;
    for (int64_t t = s0; t < tok_end; t += WAVE) {                                   // (wave-uniform bounds: every lane stays for the shuffles and ballots)
        const uint64_t h = (ng_trip_hash(body, m, t, lane, A.n) ^ rmix) & A.hmask;
        const int64_t i = t + lane;
        uint32_t c = 0u;
        if (i < s1) {
            const uint32_t own = lo + (uint32_t)i, v = rp_probe(A, h, own, lo, (uint32_t)n_g, &c);
            if (v != 0u) {                                                           // (always)
                const uint32_t first = v - 1u;
                n_dis += first == own ? 1 : 0;
                const uint64_t key = (uint64_t)c << 32 | (uint64_t)(0xFFFFFFFFu - (first - lo));
                top = key > top ? key : top;
            }
        }
        const uint64_t reps = wballot(c >= 2u);
        // token i is covered when a position in (i - n, i] is repeated: position i at bit 63, the earlier ones below it
        const uint64_t w = (reps << (63 - lane)) | (lane < 63 ? prev >> (lane + 1) : 0ull);
        const bool cov = i < tok_end && (w >> (64 - A.n)) != 0ull;
        n_rep += __builtin_popcountll(reps);
        n_cov += __builtin_popcountll(wballot(cov));
        if (A.covered && i < tok_end) {
            if (A.k == 0) A.covered[a + i] = cov ? bit : (uint16_t)0;
            else if (cov) A.covered[a + i] |= bit;
        }
        prev = reps;
    }
    n_dis = wave_sum(n_dis);
    top = wave_max_u64(top);
    if (lane != 0) return;
    if (n_pc == 1) {
        if (A.n_distinct) A.n_distinct[r] = n_dis;
        if (A.n_repeated) A.n_repeated[r] = n_rep;
        if (A.n_covered) A.n_covered[r] = n_cov;
        if (A.top_count) A.top_count[r] = (int32_t)(top >> 32);
        if (A.top_pos) A.top_pos[r] = top ? (int32_t)(0xFFFFFFFFu - (uint32_t)top) : -1;
    } else {
        if (A.n_distinct && n_dis) atomicAdd(A.n_distinct + r, n_dis);
        if (A.n_repeated && n_rep) atomicAdd(A.n_repeated + r, n_rep);
        if (A.n_covered && n_cov) atomicAdd(A.n_covered + r, n_cov);
        if (A.top && top) atomicMax(A.top + r, (unsigned long long)top);
    }
}

// top_count / top_pos of the rows of several pieces from their cell of A.top, a thread a row
__global__ __launch_bounds__(256) void gz_repeat_top_kernel(GzRepeatArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rows || A.piece_off[r + 1] - A.piece_off[r] == 1) return;
    const unsigned long long top = A.top[r];
    if (A.top_count) A.top_count[r] = (int32_t)(top >> 32);
    if (A.top_pos) A.top_pos[r] = top ? (int32_t)(0xFFFFFFFFu - (uint32_t)top) : -1;
}
