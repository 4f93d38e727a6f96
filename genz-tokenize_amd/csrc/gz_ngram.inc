// gz_ngram.inc -- exact token n-gram overlap of ragged rows against a held-out set: an index of n-grams resident in HBM, and the
// membership probe + token coverage of query rows (included by gz_kernels.hip behind gz_pieces.inc, whose body rule, position rule
// and piece walk it uses, and gz_minhash.inc, whose rotl and fmix32 it shares).
//
// The rule (include/genz_tokenize.h, "token n-gram overlap against a held-out set"): the body of a row is the row without its skips;
// its n-grams are the max(0, m - n + 1) runs of n ids (a body shorter than n has NONE: a shorter run is no evidence of leakage); S is
// the set of the reference bodies' n-grams and first(g) the smallest reference row that holds g.  Per query row: n_hits = positions
// whose n-gram is in S, n_covered = body tokens that lie inside some such n-gram, first_hit the smallest such position, first_ref =
// first of its n-gram.  A hash decides where to look, never whether two n-grams are equal: every tag match is followed by a
// comparison of the n ids.
//
// THE HASH.  One evaluation per position over the n ids, taken from the neighbouring lanes as the signature kernel takes them: two
// MurmurHash3_x86_32 streams over the same ids (they share the two multiplies per id that scramble the id; the stream step itself is
// a rotate, a shift-add and an add), seed 0 and seed 0x9E3779B9, each finished with ^ 4 n and fmix32:
//     h = (uint64) H_0(g) << 32 | H_0x9E3779B9(g);   h &= hmask (the switch ngram_hash_bits; all ones in the product)
//     tag = h >> 32;   start slot = h & (slots - 1)
// H of MinHash alone (32 bits) is too narrow for slot AND tag once a table passes 2^16 slots.
//
// THE TABLE.  One open-addressing table, linear probing, 8 bytes a slot: tag << 32 | (position + 1), position = the global index of
// the n-gram's first id in the index's own copy of the reference ids; 0 = free.  Slots: the smallest power of two that is at least
// twice the reference positions, so the table is never more than half full and every probe ends at a free slot.  INSERT: 64-bit
// atomicCAS on the free slot; on a taken slot whose tag agrees, the n ids at the occupant's position are compared with the
// inserter's own -- equal: the slot is lowered to the inserter's position with the 64-bit atomicMin (equal tags: the packed order is
// the position order) and the insert is done; otherwise the next slot.  A slot, once taken, holds occurrences of ONE n-gram for
// good (only equal n-grams ever lower it), so every occurrence of an n-gram ends in the same slot -- the first taken slot of its
// probe sequence that holds it -- and that slot ends at the n-gram's smallest position, whatever the order of the inserts.
// first(g) = the row of that position: a binary search in the index's offsets.  Distinct n-grams = successful claims.
//
// BUILD AND QUERY walk the rows as gz_minhash_sig_kernel does: PIECES of GZ_PIECE = 4096 n-gram positions, a wave a piece
// whatever row it comes from (gz_pieces.inc: count pass, piece_row, piece_body, piece_grams); a trip is 64 positions: two
// coalesced loads, one hash a lane, one probe a lane.  QUERY: hits = ballot(hit); lane l then owns TOKEN t + l of the trip, which is
// covered when one of the positions t + l - n + 1 .. t + l hit: the trip's hit bits shifted so that position t + l stands at bit 63,
// ORed with the carried hit bits of the previous 64 positions shifted in below them, and the top n bits tested -- shifts and ORs,
// no LDS.  A piece that is not its row's first evaluates the n - 1 positions before its start once more (for the carry only: they
// are the previous piece's hits); a row's last piece goes on over the body's tail of n - 1 tokens, which start no n-gram.  Every
// body token belongs to exactly one piece, which stores its `covered` byte; the row's first piece stores the frame cells' zeros.
// A row of one piece stores its counts plainly; the pieces of a longer row meet by 32-bit atomicAdd (n_hits, n_covered) and
// atomicMin (first_hit as unsigned: the launcher's 0xFFFFFFFF = -1 stays when nothing hit) in rows the launcher preset: integer
// operations that do not depend on order.  A last pass, a thread a row, hashes the n ids at first_hit again, finds their slot and
// resolves first_ref.
// Bounds: a position i is probed only when i < n_g = m - n + 1, so body[i .. i + n) lies inside the body; a slot's position was
// inserted under the same rule, so ref_ids[q .. q + n) lies inside a reference body.  Look-back trips start at s0 - 64 >= 4032.
// Workspace of a call, build or query: 16 bytes a row (piece counts and their scan; the position total is one word behind them).
// The index: 4 bytes a reference id (the copy), 8 bytes a reference row (offsets), 8 bytes a slot: 16 to 32 bytes a position.

__device__ __forceinline__ void ng_mix(uint32_t& h1, uint32_t& h2, uint32_t id)
{
    uint32_t k = id * 0xCC9E2D51u;
    k = mh_rotl(k, 15) * 0x1B873593u;
    h1 = mh_rotl(h1 ^ k, 13) * 5u + 0xE6546B64u;
    h2 = mh_rotl(h2 ^ k, 13) * 5u + 0xE6546B64u;
}
__device__ __forceinline__ uint64_t ng_finish(uint32_t h1, uint32_t h2, int n)
{
    return (uint64_t)mh_fmix32(h1 ^ (uint32_t)(4 * n)) << 32 | (uint64_t)mh_fmix32(h2 ^ (uint32_t)(4 * n));
}
constexpr uint32_t NG_SEED2 = 0x9E3779B9u;

// the hash of g[0 .. n), one thread (the resolve pass)
__device__ __forceinline__ uint64_t ng_hash_serial(const int32_t* __restrict__ g, int n)
{
    uint32_t h1 = 0u, h2 = NG_SEED2;
    for (int i = 0; i < n; ++i) ng_mix(h1, h2, (uint32_t)g[i]);
    return ng_finish(h1, h2, n);
}

// The hash of the n-gram at body position t + lane, for every lane of the wave at once (call it with all lanes active): lane l
// loads id t + l and, for the n - 1 ids beyond the trip, id t + 64 + l; the ids of a lane's own run come from its neighbours by wave
// shuffles.  Lanes whose run leaves the body get a hash of zero-filled ids, which nobody uses.  m: ids of the body; t >= 0.
__device__ __forceinline__ uint64_t ng_trip_hash(const int32_t* __restrict__ body, int64_t m, int64_t t, int lane, int n)
{
    const int64_t q0 = t + lane, q1 = t + WAVE + lane;
    const uint32_t id0 = q0 < m ? (uint32_t)body[q0] : 0u;
    const uint32_t id1 = (lane < n - 1 && q1 < m) ? (uint32_t)body[q1] : 0u;
    uint32_t h1 = 0u, h2 = NG_SEED2;
    for (int i = 0; i < n; ++i) {
        const int src = lane + i;
        const uint32_t x = (uint32_t)__shfl((int)id0, src & (WAVE - 1), WAVE), y = (uint32_t)__shfl((int)id1, src & (WAVE - 1), WAVE);
        ng_mix(h1, h2, src < WAVE ? x : y);
    }
    return ng_finish(h1, h2, n);
}

__device__ __forceinline__ bool ng_equal(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int n)
{
    for (int i = 0; i < n; ++i) if (x[i] != y[i]) return false;
    return true;
}

// Insert the n-gram at position pos of the index's id copy; 1 when this thread claimed a free slot (a new distinct n-gram).
__device__ __forceinline__ int ng_insert(const GzNgramArgs& A, uint64_t h, uint64_t pos)
{
    const uint32_t tag = (uint32_t)(h >> 32);
    const unsigned long long mine = (unsigned long long)tag << 32 | (unsigned long long)(pos + 1);
    for (uint64_t s = h & A.mask;; s = (s + 1) & A.mask) {                            // (ends: the table is at most half full)
        const unsigned long long seen = atomicCAS(A.table + s, 0ull, mine);
        if (seen == 0ull) return 1;
        if ((uint32_t)(seen >> 32) == tag && ng_equal(A.ref_ids + ((uint32_t)seen - 1u), A.ref_ids + pos, A.n)) {
            atomicMin(A.table + s, mine);
            return 0;
        }
    }
}

// position + 1 of the smallest occurrence of g[0 .. n) in the reference, 0 when S does not hold it
__device__ __forceinline__ uint32_t ng_probe(const GzNgramArgs& A, uint64_t h, const int32_t* __restrict__ g)
{
    const uint32_t tag = (uint32_t)(h >> 32);
    for (uint64_t s = h & A.mask;; s = (s + 1) & A.mask) {                            // (ends: the table is at most half full)
        const unsigned long long v = A.table[s];
        if (v == 0ull) return 0u;
        if ((uint32_t)(v >> 32) == tag && ng_equal(A.ref_ids + ((uint32_t)v - 1u), g, A.n)) return (uint32_t)v;
    }
}

// BUILD: A.ids / A.row_off are the index's own copy and its rebased offsets (A.ref_ids == A.ids)
__global__ __launch_bounds__(WAVE * 4) void gz_ngram_insert_kernel(GzNgramArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t j, n_pc, m;
    const int64_t r = piece_row(A, p, &j, &n_pc);
    const int64_t a = piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
    const int64_t n_g = piece_grams(m, A.n);
    const int64_t s0 = j * GZ_PIECE, s1 = s0 + GZ_PIECE < n_g ? s0 + GZ_PIECE : n_g;
    const int32_t* const body = A.ids + a;                                           // (never read when m == 0)
    int claimed = 0;
    for (int64_t t = s0; t < s1; t += WAVE) {                                        // (wave-uniform bounds: every lane stays for the shuffles)
        const uint64_t h = ng_trip_hash(body, m, t, lane, A.n) & A.hmask;
        if (t + lane < s1) claimed += ng_insert(A, h, (uint64_t)(a + t + lane));
    }
    claimed = wave_sum(claimed);
    if (lane == 0 && claimed) atomicAdd(A.n_distinct, (unsigned long long)claimed);
}

// QUERY: A.ids / A.row_off are the caller's rows (absolute offsets); the table, A.ref_ids and A.ref_off are the index's
__global__ __launch_bounds__(WAVE * 4) void gz_ngram_query_kernel(GzNgramArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t j, n_pc, m;
    const int64_t r = piece_row(A, p, &j, &n_pc);
    const int64_t a = piece_body(A.row_off, r, A.skip_front, A.skip_back, &m);
    const int64_t n_g = piece_grams(m, A.n);
    const int64_t s0 = j * GZ_PIECE, s1 = s0 + GZ_PIECE < n_g ? s0 + GZ_PIECE : n_g;
    const int64_t tok_end = j == n_pc - 1 ? m : s1;                                   // the last piece owns the tail, which starts no n-gram
    const int32_t* const body = A.ids + a;                                           // (never read when m == 0)
    if (j == 0) {
        if (lane == 0 && A.n_grams) A.n_grams[r] = (int32_t)n_g;
        if (A.covered) {                                                             // the frame cells: in no body, never covered
            const int64_t lo = A.row_off[r], hi = A.row_off[r + 1];
            if (lane == 0 && A.skip_front && hi > lo) A.covered[lo] = 0;
            if (lane == 1 && A.skip_back && hi > lo) A.covered[hi - 1] = 0;
        }
    }
    uint64_t prev = 0ull;                                                            // hit bits of the 64 positions before the trip
    if (j > 0 && A.n > 1) {                                                          // the n - 1 positions before the piece: the carry only
        const int64_t t = s0 - WAVE;
        const uint64_t h = ng_trip_hash(body, m, t, lane, A.n) & A.hmask;
        prev = wballot(lane >= WAVE - (A.n - 1) && ng_probe(A, h, body + t + lane) != 0u);
    }
    int n_hits = 0, n_cov = 0;
    int64_t first = -1;
    for (int64_t t = s0; t < tok_end; t += WAVE) {                                   // (wave-uniform bounds: every lane stays for the shuffles and ballots)
        const uint64_t h = ng_trip_hash(body, m, t, lane, A.n) & A.hmask;
        const int64_t i = t + lane;
        const uint64_t hits = wballot(i < s1 && ng_probe(A, h, body + i) != 0u);
        // token i is covered when a position in (i - n, i] hit: position i at bit 63, the earlier ones below it
        const uint64_t w = (hits << (63 - lane)) | (lane < 63 ? prev >> (lane + 1) : 0ull);
        const bool cov = i < tok_end && (w >> (64 - A.n)) != 0ull;
        const uint64_t covered = wballot(cov);
        n_hits += __builtin_popcountll(hits);
        n_cov += __builtin_popcountll(covered);
        if (first < 0 && hits) first = t + __builtin_ctzll(hits);
        if (A.covered && i < tok_end) A.covered[a + i] = cov ? 1 : 0;
        prev = hits;
    }
    if (lane != 0) return;
    if (n_pc == 1) {
        if (A.n_hits) A.n_hits[r] = n_hits;
        if (A.n_covered) A.n_covered[r] = n_cov;
        if (A.first_hit) A.first_hit[r] = (int32_t)first;
    } else {
        if (A.n_hits && n_hits) atomicAdd(A.n_hits + r, n_hits);
        if (A.n_covered && n_cov) atomicAdd(A.n_covered + r, n_cov);
        if (A.first_hit && first >= 0) atomicMin(reinterpret_cast<uint32_t*>(A.first_hit) + r, (uint32_t)first);
    }
}

// first_ref[r] from first_hit[r], a thread a row: the slot of the n-gram there holds its smallest reference position, whose row is
// the last r' with ref_off[r'] <= position (rows of no ids share their offset with the row behind them: the last one holds it)
__global__ __launch_bounds__(256) void gz_ngram_resolve_kernel(GzNgramArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rows) return;
    const int32_t fh = A.first_hit[r];
    int32_t ref = -1;
    if (fh >= 0) {
        int64_t m;
        const int32_t* const g = A.ids + piece_body(A.row_off, r, A.skip_front, A.skip_back, &m) + fh;
        const uint32_t v = ng_probe(A, ng_hash_serial(g, A.n) & A.hmask, g);
        if (v != 0u) {                                                               // (always: first_hit is a position that hit)
            const int64_t q = (int64_t)(v - 1u);
            int64_t lo = 0, hi = A.ref_rows - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (A.ref_off[mid] <= q) lo = mid; else hi = mid - 1;
            }
            ref = (int32_t)lo;
        }
    }
    A.first_ref[r] = ref;
}
