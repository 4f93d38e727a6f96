// gz_substr.inc -- exact duplicate substrings ACROSS the rows of a call (the ExactSubstr half of Lee et al. 2021, at threshold n), and
// the cut of marked ids out of ragged rows (included by gz_kernels.hip behind gz_pieces.inc, whose body rule, n-gram rule and piece
// walk it uses, and gz_ngram.inc, whose two hash streams it shares).
//
// The rule (include/genz_tokenize.h, "duplicate substrings across documents"): the body of a row is the row without its skips; its
// n-gram positions are the max(0, m - n + 1) runs body[i .. i + n), 1 <= n <= 256, ordered by (row, i) -- the order they stand in
// ids.  later(r, i): the same n ids stand at a smaller position, in an earlier row or earlier in row r.  Per row: n_grams, n_later =
// positions with later, n_dup = body tokens t with some later i, i <= t < i + n, first_dup = the smallest later i (-1: none),
// first_src = the row of the smallest position of the whole call that holds the n-gram at first_dup; dup = one byte an id.  A token
// lies inside a repeated substring of n ids or more exactly when it lies inside a repeated n-gram window: one table over the call's
// own positions gives ExactSubstr's answer without a suffix array.  A hash decides where to look, never whether two n-grams are
// equal: every tag match is followed by a comparison of the n ids.
//
// THE HASH.  ng_trip_hash takes a lane's run from its neighbours' registers and ends at n = 32.  Here a trip STAGES its 64 + n - 1 ids
// (at most 319) in the wave's own 1280 bytes of LDS with coalesced loads (ids beyond the body are zero) and lane l hashes
// stage[l .. l + n): consecutive lanes read consecutive words, so no two lanes meet in a bank.  The streams are gz_ngram.inc's: two
// MurmurHash3_x86_32 streams, seeds 0 and 0x9E3779B9, ^ 4 n, fmix32; h &= hmask (the switch substr_hash_bits); tag = h >> 32; start
// slot = h & (slots - 1).  A wave's LDS traffic is its own: the four waves of a workgroup never wait for each other.
//
// INSERT (gz_substr_insert_kernel).  One open-addressing table, linear probing, 8 bytes a slot: tag << 32 | (position + 1), position
// = the index of the n-gram's first id counted from row_off[0]; 0 = free; slots = gz_substr_slots(positions).  The protocol is
// gz_ngram.inc's: 64-bit atomicCAS on a free slot; on a taken slot whose tag agrees the n ids at the occupant's position (global
// memory) are compared with the inserter's (LDS) -- equal: the slot is lowered by the 64-bit atomicMin and the insert is done;
// otherwise the next slot.  A slot, once taken, holds occurrences of ONE n-gram for good, so every occurrence of an n-gram ends in
// the same slot, and that slot ends at the n-gram's smallest position whatever the order of the inserts.  Each position also stores
// the index of the slot it ended in: slot_of[position], 4 bytes.
// MARK (gz_substr_mark_kernel).  No second hash, no second comparison: later(position) = table[slot_of[position]] holds another
// position.  Coverage at n up to 256 does not fit the 64-bit shifted ballot of gz_ngram_query_kernel: the wave carries the LAST later
// position it has seen.  In a trip lane l owns token t + l and takes the highest set bit of ballot(later) at or below l, else the
// carry; the token is dup when that position >= token - n + 1.  A piece that is not its row's first looks back over the n - 1
// positions before its start for the carry only (trips of 64 from the nearest back; the first with a later position ends the walk).
// A row's last piece goes on over the body's tail of n - 1 tokens.  Every body token belongs to exactly one piece, which stores its
// dup byte; the row's first piece stores the frame cells' zeros.  A row of one piece stores its counts plainly; the pieces of a longer
// row meet by 32-bit atomicAdd (n_later, n_dup) and atomicMin (first_dup as unsigned) in rows the launcher preset.
// RESOLVE (gz_substr_resolve_kernel), a thread a row: first_src = the last row r' <= r with row_off[r'] <= the position in the slot of
// first_dup's n-gram.
// Bounds: a position i is inserted and marked only when i < n_g = m - n + 1, so body[i .. i + n) lies inside the body and every
// slot_of word that is read was written; a slot's position was inserted under the same rule.  Look-back trips start at
// s0 - 64 k >= 4096 - 320.  Every index that comes out of memory is checked in the diagnostic build (GZ_CHK 801..806).
//
// CUT (gz_cut_count_kernel, gz_cut_write_kernel): output row r = the ids of row r whose drop byte is 0, in order.  Pieces of 4096 ids
// of the WHOLE row (the piece count at width 1 without skips), a wave a piece.  Count: kept ids of a piece -> piece_kept[p].  ONE
// 64-bit scan over the pieces -> piece_base.  Pieces stand in row order, so piece_base[first piece of r] is out_row_off[r] and the
// kept ids of a row's earlier pieces are a difference of two scan words: no atomic ticket, nothing that depends on scheduling, and no
// second scan over the rows.  Write: a trip's kept ids go to base + (kept ids below the lane: a ballot and v_mbcnt) and the base is
// carried over the trips.  GZ_CHK 811..812.

constexpr int SS_STAGE = WAVE + GZ_SUBSTR_MAX_N;                                      // words of LDS a wave stages a trip in: 64 + n - 1 <= 319

// the trip at body position t into the wave's stage: ids t .. t + 64 + n - 2, zero beyond the body (all lanes; m ids in the body)
__device__ __forceinline__ void ss_stage(int32_t* __restrict__ w, const int32_t* __restrict__ body, int64_t m, int64_t t, int lane, int n)
{
    __builtin_amdgcn_wave_barrier();                                                 // (the last trip's reads are behind us)
    for (int k = lane; k < WAVE + n - 1; k += WAVE) w[k] = t + k < m ? body[t + k] : 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the hash of g[0 .. n), g in LDS: the streams of ng_hash_serial
__device__ __forceinline__ uint64_t ss_hash(const int32_t* g, int n)
{
    uint32_t h1 = 0u, h2 = NG_SEED2;
    for (int i = 0; i < n; ++i) ng_mix(h1, h2, (uint32_t)g[i]);
    return ng_finish(h1, h2, n);
}

// x in global memory, y in LDS
__device__ __forceinline__ bool ss_equal(const int32_t* __restrict__ x, const int32_t* y, int n)
{
    for (int i = 0; i < n; ++i) if (x[i] != y[i]) return false;
    return true;
}

// Insert the n-gram at position pos (from off0), whose ids stand at g in LDS; the slot it ended in.  (One exit, behind the loop, as in
// rp_insert: with a return from inside the comparison's branch the compiler lost the slot on that path.)
__device__ __forceinline__ uint32_t ss_insert(const GzSubstrArgs& A, uint64_t h, uint32_t pos, const int32_t* g)
{
    const int32_t* const base = A.ids + A.off0;
    const uint32_t tag = (uint32_t)(h >> 32);
    const unsigned long long mine = (unsigned long long)tag << 32 | (unsigned long long)(pos + 1u);
    uint64_t s = h & A.mask;
    for (;; s = (s + 1) & A.mask) {                                                   // (ends: a free slot or the n-gram's own; the table is never full)
        const unsigned long long seen = atomicCAS(A.table + s, 0ull, mine);
        if (seen == 0ull) break;
        if ((uint32_t)(seen >> 32) != tag) continue;
        const uint32_t q = (uint32_t)seen - 1u;
        if (!GZ_CHK(801, (uint64_t)q + (uint64_t)A.n, A.n_ids + 1)) continue;
        if (ss_equal(base + q, g, A.n)) {
            atomicMin(A.table + s, mine);
            break;
        }
    }
    return (uint32_t)s;
}

// the piece of wave p: *r its row, *a its body's first id (absolute), *m the body's ids, *n_g its n-grams, [*s0, *s1) the positions
// the piece takes (empty when *s1 <= *s0), *tok_end the end of the tokens it owns
__device__ __forceinline__ void ss_piece(const GzSubstrArgs& A, int64_t p, int64_t* r, int64_t* a, int64_t* m, int64_t* n_g, int64_t* s0, int64_t* s1,
                                         int64_t* tok_end, int64_t* j, int64_t* n_pc)
{
    *r = piece_row(A, p, j, n_pc);
    *a = piece_body(A.row_off, *r, A.skip_front, A.skip_back, m);
    *n_g = piece_grams(*m, A.n);
    *s0 = *j * GZ_PIECE;
    *s1 = *s0 + GZ_PIECE < *n_g ? *s0 + GZ_PIECE : *n_g;
    *tok_end = *j == *n_pc - 1 ? *m : *s0 + GZ_PIECE;                                 // the last piece owns the tail, which starts no n-gram
}

__global__ __launch_bounds__(WAVE * 4) void gz_substr_insert_kernel(GzSubstrArgs A)
{
    __shared__ int32_t stage[4][SS_STAGE];
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int32_t* const w = stage[threadIdx.x / WAVE];
    int64_t r, a, m, n_g, s0, s1, tok_end, j, n_pc;
    ss_piece(A, p, &r, &a, &m, &n_g, &s0, &s1, &tok_end, &j, &n_pc);
    const int32_t* const body = A.ids + a;                                           // (never read when m == 0)
    const uint32_t lo = (uint32_t)(a - A.off0);
    for (int64_t t = s0; t < s1; t += WAVE) {                                        // (wave-uniform bounds: every lane stages)
        ss_stage(w, body, m, t, lane, A.n);
        if (t + lane < s1) {
            const uint32_t pos = lo + (uint32_t)(t + lane);
            const uint32_t s = ss_insert(A, ss_hash(w + lane, A.n) & A.hmask, pos, w + lane);
            if (GZ_CHK(802, pos, A.n_ids)) A.slot_of[pos] = s;
        }
    }
}

// later(position): the slot its n-gram ended in holds a smaller position (every marked position was inserted)
__device__ __forceinline__ bool ss_later(const GzSubstrArgs& A, uint32_t pos)
{
    if (!GZ_CHK(803, pos, A.n_ids)) return false;
    const uint32_t s = A.slot_of[pos];
    if (!GZ_CHK(804, s, A.mask + 1)) return false;
    return (uint32_t)A.table[s & A.mask] != pos + 1u;                                // (masked: a slot word comes out of memory)
}

__global__ __launch_bounds__(WAVE * 4) void gz_substr_mark_kernel(GzSubstrArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t r, a, m, n_g, s0, s1, tok_end, j, n_pc;
    ss_piece(A, p, &r, &a, &m, &n_g, &s0, &s1, &tok_end, &j, &n_pc);
    const uint32_t lo = (uint32_t)(a - A.off0);
    if (j == 0) {
        if (lane == 0 && A.n_grams) A.n_grams[r] = (int32_t)n_g;
        if (A.dup) {                                                                 // the frame cells: in no body, never dup
            const int64_t b = A.row_off[r], e = A.row_off[r + 1];
            if (lane == 0 && A.skip_front && e > b) A.dup[b] = 0;
            if (lane == 1 && A.skip_back && e > b) A.dup[e - 1] = 0;
        }
    }
    int64_t last = -1;                                                               // the last later position seen, -1: none yet
    if (j > 0)                                                                       // the n - 1 positions before the piece: the carry only
        for (int64_t t = s0 - WAVE; t > s0 - WAVE - (A.n - 1); t -= WAVE) {          // (wave-uniform; from the nearest trip back)
            const int64_t i = t + lane;
            const uint64_t L = wballot(i >= s0 - (A.n - 1) && ss_later(A, lo + (uint32_t)i));
            if (L) { last = t + 63 - __builtin_clzll(L); break; }
        }
    int n_lat = 0, n_dp = 0;
    int64_t first = -1;
    for (int64_t t = s0; t < tok_end; t += WAVE) {                                   // (wave-uniform bounds: every lane stays for the ballots)
        const int64_t i = t + lane;
        const uint64_t L = wballot(i < s1 && ss_later(A, lo + (uint32_t)i));
        // token i is dup when the nearest later position at or before it lies in (i - n, i]
        const uint64_t at = L & (lane == WAVE - 1 ? ~0ull : (2ull << lane) - 1ull);
        const int64_t q = at ? t + 63 - __builtin_clzll(at) : last;
        const bool d = i < tok_end && q >= 0 && q + A.n > i;
        n_lat += __builtin_popcountll(L);
        n_dp += __builtin_popcountll(wballot(d));
        if (first < 0 && L) first = t + __builtin_ctzll(L);
        if (A.dup && i < tok_end && GZ_CHK(805, (uint64_t)(a - A.off0 + i), A.n_ids)) A.dup[a + i] = d ? 1 : 0;
        if (L) last = t + 63 - __builtin_clzll(L);
    }
    if (lane != 0) return;
    if (n_pc == 1) {
        if (A.n_later) A.n_later[r] = n_lat;
        if (A.n_dup) A.n_dup[r] = n_dp;
        if (A.first_dup) A.first_dup[r] = (int32_t)first;
    } else {
        if (A.n_later && n_lat) atomicAdd(A.n_later + r, n_lat);
        if (A.n_dup && n_dp) atomicAdd(A.n_dup + r, n_dp);
        if (A.first_dup && first >= 0) atomicMin(reinterpret_cast<uint32_t*>(A.first_dup) + r, (uint32_t)first);
    }
}

// first_src[r] from first_dup[r], a thread a row: the slot of the n-gram there holds its smallest position of the call, whose row is the
// last r' <= r with row_off[r'] <= position (rows of no ids share their offset with the row behind them: the last one holds it)
__global__ __launch_bounds__(256) void gz_substr_resolve_kernel(GzSubstrArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rows) return;
    const int32_t fd = A.first_dup[r];
    int32_t src = -1;
    if (fd >= 0) {
        int64_t m;
        const uint64_t pos = (uint64_t)(piece_body(A.row_off, r, A.skip_front, A.skip_back, &m) - A.off0 + fd);
        if (GZ_CHK(806, pos, A.n_ids)) {
            const uint32_t s = A.slot_of[pos];
            const int64_t q = A.off0 + (int64_t)((uint32_t)A.table[s & A.mask] - 1u);
            int64_t lo = 0, hi = r;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (A.row_off[mid] <= q) lo = mid; else hi = mid - 1;
            }
            src = (int32_t)lo;
        }
    }
    A.first_src[r] = src;
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------
// the piece of wave p over WHOLE rows: its row, and the ids [*b, *e) (absolute) it takes
__device__ __forceinline__ int64_t cut_piece(const GzCutArgs& A, int64_t p, int64_t* b, int64_t* e, int64_t* j)
{
    int64_t n_pc;
    const int64_t r = piece_row(A, p, j, &n_pc);
    const int64_t lo = A.row_off[r], hi = A.row_off[r + 1];
    *b = lo + *j * GZ_PIECE;
    *e = *b + GZ_PIECE < hi ? *b + GZ_PIECE : hi;
    return r;
}

__global__ __launch_bounds__(WAVE * 4) void gz_cut_count_kernel(GzCutArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t b, e, j;
    cut_piece(A, p, &b, &e, &j);
    int kept = 0;
    for (int64_t i = b + lane; i < e; i += WAVE) kept += A.drop[i] == 0 ? 1 : 0;
    kept = wave_sum(kept);
    if (lane == 0) A.piece_kept[p] = kept;
}

__global__ __launch_bounds__(WAVE * 4) void gz_cut_write_kernel(GzCutArgs A)
{
    const int lane = lane_id();
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;                  // the wave's piece
    if (p >= A.n_pieces) return;
    int64_t b, e, j;
    const int64_t r = cut_piece(A, p, &b, &e, &j);
    int64_t base = A.piece_base[p];                                                  // kept ids of every piece before this one: rows stand back to back
    if (lane == 0) {
        if (j == 0) {
            A.out_row_off[r] = base;
            if (A.n_kept) A.n_kept[r] = (int32_t)(A.piece_base[A.one_each ? r + 1 : A.piece_off[r + 1]] - base);
        }
        if (p == A.n_pieces - 1) A.out_row_off[A.n_rows] = A.piece_base[A.n_pieces];  // (the last piece is the last row's)
    }
    if (!A.out_ids) return;
    for (int64_t t = b; t < e; t += WAVE) {                                          // (wave-uniform bounds: every lane stays for the ballot)
        const int64_t i = t + lane;
        const bool keep = i < e && A.drop[i] == 0;
        const uint64_t K = wballot(keep);
        const int64_t at = base + below(K);
        if (keep && GZ_CHK(811, at, A.n_ids)) A.out_ids[at] = A.ids[i];
        base += __builtin_popcountll(K);
    }
    (void)GZ_CHK(812, base, A.n_ids + 1);
}
