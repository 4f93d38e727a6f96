// gz_window.inc -- overlapping max_len windows over ragged token rows (included by gz_kernels.hip).
//
// The reference cuts a document longer than max_len to token[:max_len-1] + [eos] (tokenize.py:141-146) and drops the rest.  Here
// the rest follows in further rows of the same shape.  With L = max_len, s = stride, room = L - 2, step = room - s (>= 1) and
// body = the row without its frame (T tokens):
//
//   n_win = 1 if T <= room else 1 + ceil((T - room) / step)
//   window j: start = j * step, chunk = body[start : min(start + room, T)]
//   row = [bos] + chunk + [eos] + [pad] * (room - len(chunk)),   n_real = len(chunk) + 2,   mask = (row != pad)  (tokenize.py:148-152)
//
// Window 0 is the reference's own row; the last window is shorter, not shifted back.
//
// Two passes.  Count: one thread per row, n_win[r], then the 64-bit exclusive scan that decode and the pre-pass use -> win_off.
// Fill: work is divided over WINDOWS, never over documents -- a wave owns 64 consecutive windows, whatever rows they come from.
// Each lane first finds the row of one window (binary search in win_off: every row has a window, so win_off is strictly
// increasing) and keeps that window's source position and chunk length; the wave then walks the 64 * L cells of its windows as one
// flat range, 16 bytes a lane where the rows are 16-byte aligned (L % 4 == 0), and takes each cell's window from the lane that
// looked it up (a wave shuffle).  Chunk, frame, padding and mask leave together: every cell is written once, nothing is cleared
// beforehand.  Write-bound: 8 W L bytes out (+ 12 a window), about 4 T room / step bytes in per document, whose source position
// has no alignment beyond 4 bytes (dword loads).  Cell indices are 64-bit throughout (W * L may exceed 2^31).

__global__ __launch_bounds__(256) void gz_window_count_kernel(const int64_t* __restrict__ row_off, int64_t n_rows, int32_t room, int32_t step,
                                                              int32_t skip, int64_t* __restrict__ n_win)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t T = row_off[r + 1] - row_off[r] - skip;                 // absolute offsets from the ids base pointer (as gz_decode_kernel)
    n_win[r] = T <= room ? 1 : 1 + (T - room + step - 1) / step;
}

// U cells per lane and store: 4 (rows and base pointers 16-byte aligned) or 1 (any L)
template <int U>
__global__ __launch_bounds__(WAVE * 4) void gz_window_fill_kernel(GzWinArgs A)
{
    const int lane = lane_id();
    const int64_t w0 = ((int64_t)blockIdx.x * 4 + threadIdx.x / WAVE) * WAVE;       // the wave's first window
    if (w0 >= A.n_win) return;
    const int nw = A.n_win - w0 < WAVE ? (int)(A.n_win - w0) : WAVE;
    // lane = window w0 + lane: its row d (the last one with win_off[d] <= w; d <= w), where its chunk starts in ids, how long it is
    int64_t src = 0;
    int clen = 0;
    if (lane < nw) {
        const int64_t w = w0 + lane;
        int64_t lo = 0, hi = w < A.n_rows - 1 ? w : A.n_rows - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (A.win_off[mid] <= w) lo = mid; else hi = mid - 1;
        }
        const int64_t a = A.row_off[lo], b = A.row_off[lo + 1];
        const int64_t start = (w - A.win_off[lo]) * A.step;
        const int64_t left = b - a - A.skip_front - A.skip_back - start;             // > stride for every window but a lone empty one
        clen = left < A.room ? (left > 0 ? (int)left : 0) : A.room;
        src = a + A.skip_front + start;
        if (A.win_doc) A.win_doc[w] = (int32_t)lo;
        if (A.win_start) A.win_start[w] = (int32_t)start;
        if (A.win_n_real) A.win_n_real[w] = clen + 2;
    }
    // the wave's nw * L cells as one range of units of U cells; unit t = (window t / Q, column U * (t % Q)), carried along instead of divided
    const int Q = A.max_len / U;
    const int64_t n_units = (int64_t)nw * Q;
    const int dj = WAVE / Q, dc = WAVE % Q;
    int j = lane / Q, col = lane % Q;
    for (int64_t base = 0; base < n_units; base += WAVE) {                           // (every lane stays in the loop: the shuffles read all of them)
        const int64_t s_j = __shfl(src, j & (WAVE - 1), WAVE);
        const int c_j = __shfl(clen, j & (WAVE - 1), WAVE);
        if (base + lane < n_units) {
            const int k0 = col * U;
            int32_t tok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) tok[u] = 0;
            if (c_j > 0 && k0 <= c_j) {                                              // the unit holds chunk cells: all its loads under ONE branch, inside the chunk
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    int kk = k0 + u - 1;
                    kk = kk < 0 ? 0 : kk;
                    kk = kk < c_j ? kk : c_j - 1;
                    tok[u] = A.ids[s_j + kk];
                }
            }
            int32_t v[U], m[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u;
                v[u] = k == 0 ? A.bos_id : k <= c_j ? tok[u] : k == c_j + 1 ? A.eos_id : A.pad_id;
                m[u] = v[u] != A.pad_id ? 1 : 0;
            }
            const int64_t cell = (w0 + j) * (int64_t)A.max_len + k0;
            if constexpr (U == 4) {
                nt_store4(A.out_ids + cell, v[0], v[1], v[2], v[3]);
                if (A.out_mask) nt_store4(A.out_mask + cell, m[0], m[1], m[2], m[3]);
            } else {
                A.out_ids[cell] = v[0];
                if (A.out_mask) A.out_mask[cell] = m[0];
            }
        }
        col += dc; j += dj;
        if (col >= Q) { col -= Q; ++j; }
    }
}
