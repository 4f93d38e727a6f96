// gz_pieces.inc -- how a ragged row's body is divided over waves: the one decision MinHash signatures (gz_minhash.inc), the n-gram
// overlap index (gz_ngram.inc) and n-gram repeats (gz_repeat.inc) share (included by gz_kernels.hip in front of the three).
//
// The BODY of a row is the row without its skips.  Its POSITIONS are what a lane evaluates: the shingles of a signature (runs of w
// ids; ONE run, the whole body, when it is shorter: a non-empty body always has a position) or the n-grams of an index, a query or a
// repeat count (runs of n ids; a body shorter than n has NONE).  Work is divided over PIECES of GZ_PIECE = 4096 positions, never over
// rows: a row has max(1, ceil(positions / 4096)) pieces -- every row has one, so that it is visited and its outputs are written --
// and a wave owns one piece, whatever row it comes from.
//
// COUNT (gz_piece_count_kernel<RULE, ROWS>, compiled once per position rule): n_pieces[r]; optionally the offsets rebased to
// row_off[0] (the index's own copy); optionally the rows' position total, a wave's sum in one 64-bit atomicAdd; and the flag of a
// body of 2^31 ids or more, which no piece kernel is launched over.  ROWS: a thread takes one row where no total is asked for.
// Where one is, it takes GZ_PIECE_TOTAL_ROWS rows, 256 apart (the loads stay coalesced): the waves' atomics all land on ONE
// address, where they queue, and with a row a thread the index build over 1 M rows took 10.92 to 11.11 ms against the 10.79 to
// 10.83 ms of a second scan (profiles/pieces_ab.json, "a_row_a_thread_with_total").  The launcher clears total and flag, and scans n_pieces into
// piece_off with the 64-bit scan every ragged pass uses.  The host waits once for piece_off[n_rows], the total and the flag
// (gz_rows_api.inc, pieces_count_locked).
// WALK (piece_row): the row of piece p is the last r with piece_off[r] <= p -- a binary search, skipped when every row has one piece
// (the launchers set one_each: piece p is row p and piece_off is not read).

constexpr int GZ_PIECE = 4096;                                                        // positions a wave takes: 64 trips of 64
constexpr int GZ_PIECE_TOTAL_ROWS = 8;                                                // rows a thread of the count kernel takes where the position total is wanted

// the body of row r: where it starts in ids and how many ids it holds (0 for a row shorter than its skips)
__device__ __forceinline__ int64_t piece_body(const int64_t* __restrict__ row_off, int64_t r, int32_t skip_front, int32_t skip_back, int64_t* n)
{
    const int64_t a = row_off[r] + skip_front, b = row_off[r + 1] - skip_back;
    *n = b > a ? b - a : 0;
    return a;
}
// the two position rules: of a body of n ids at width w
__device__ __forceinline__ int64_t piece_shingles(int64_t n, int32_t w) { return n >= w ? n - w + 1 : (n > 0 ? 1 : 0); }
__device__ __forceinline__ int64_t piece_grams(int64_t n, int32_t w) { return n >= w ? n - w + 1 : 0; }

// rebased may be null and has n_rows + 1 cells; n_pos is null with ROWS == 1 (then nobody asked for the total)
template <int RULE, int ROWS>
__global__ __launch_bounds__(256) void gz_piece_count_kernel(const int64_t* __restrict__ row_off, int64_t n_rows, int32_t skip_front,
                                                             int32_t skip_back, int32_t w, int64_t* __restrict__ n_pieces,
                                                             int64_t* __restrict__ rebased, unsigned long long* __restrict__ n_pos,
                                                             uint32_t* __restrict__ too_long)
{
    int64_t sum = 0;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int64_t r = ((int64_t)blockIdx.x * ROWS + k) * 256 + threadIdx.x;
        if (r >= n_rows) break;
        int64_t m;
        piece_body(row_off, r, skip_front, skip_back, &m);
        if (m >= ((int64_t)1 << 31)) atomicOr(too_long, 1u);
        const int64_t g = RULE == GZ_PIECES_SHINGLES ? piece_shingles(m, w) : piece_grams(m, w);
        n_pieces[r] = g <= GZ_PIECE ? 1 : (g + GZ_PIECE - 1) / GZ_PIECE;
        if (rebased) {
            const int64_t base = row_off[0];
            rebased[r] = row_off[r] - base;
            if (r == n_rows - 1) rebased[n_rows] = row_off[n_rows] - base;
        }
        sum += g;
    }
    if (ROWS == 1) return;
    // (every lane stays for the shuffles; 64 x 8 bodies below 2^31 fit 40 bits: the halves are summed apart)
    const int lo = wave_sum((int)(sum & 0xFFFF)), hi = wave_sum((int)(sum >> 16));
    if (lane_id() == 0 && (lo | hi)) atomicAdd(n_pos, (unsigned long long)lo + ((unsigned long long)hi << 16));
}

// the wave's piece p: its row (the last row with piece_off[r] <= p; every row has a piece), which of the row's pieces it is (*j) and
// how many the row has (*n_pc).  Args: GzMinhashArgs, GzNgramArgs or GzRepeatArgs -- their one_each, n_rows and piece_off.
template <class Args>
__device__ __forceinline__ int64_t piece_row(const Args& A, int64_t p, int64_t* j, int64_t* n_pc)
{
    if (A.one_each) { *j = 0; *n_pc = 1; return p; }
    int64_t lo = 0, hi = p < A.n_rows - 1 ? p : A.n_rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (A.piece_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    *j = p - A.piece_off[lo];
    *n_pc = A.piece_off[lo + 1] - A.piece_off[lo];
    return lo;
}
