// gz_pairwin.inc -- question-context windows with answer positions over ragged token rows (included by gz_kernels.hip).
//
// gz_window.inc keeps a long document whole but has no question in front; the reference's pair row (tokenize.py:141-146,
// `<s> question </s></s> context </s>`) has one but cuts the context at max_len.  Here the question stands in front of EVERY window
// of its context.  With L = max_len, s = stride, mq = max_query_len, Q = the question body (Tq tokens), body = the context body
// (T tokens):
//
//   q      = min(Tq, mq)                    (the question keeps its FIRST q tokens)
//   room   = L - 4 - q   (>= s + 1)         step = room - s  (>= 1)
//   n_win  = 1 if T <= room else 1 + ceil((T - room) / step)
//   window j: start = j * step, chunk = body[start : min(start + room, T)], n = len(chunk)
//   row    = [bos] + Q[:q] + [eos, eos] + chunk + [eos] + [pad] * (room - n)      n_real = q + 4 + n
//   mask   = (row != pad)                                    (tokenize.py:148-152, as everywhere)
//   type   = 0 on columns < q + 2, 1 on columns q + 2 .. n_real - 1, the pad id behind them
//   ctx_col = q + 3                                          (column of chunk[0])
//
// The last window is shorter, not shifted back.  An answer [a0, a1) of the body (present iff 0 <= a0 < a1 <= T) is held by window j iff
// start <= a0 and a1 <= start + n: start_pos = ctx_col + a0 - start, end_pos = ctx_col + a1 - 1 - start, has_answer = 1; otherwise
// start_pos = end_pos = 0 (the bos column) and has_answer = 0.
//
// Two passes, as gz_window.inc and for its reasons.  Count: one thread per pair, n_win[r] and q[r] (room depends on the pair here),
// then the 64-bit exclusive scan -> win_off.  Fill: work is divided over WINDOWS, never over pairs -- a wave owns 64 consecutive
// windows.  Each lane finds the pair of one window (binary search in win_off: every pair has a window, so win_off is strictly
// increasing), keeps that window's question source, chunk source, q and n, and writes the per-window outputs; the wave then walks the
// 64 * L cells of its windows as one flat range, 16 bytes a lane where the rows are 16-byte aligned (L % 4 == 0), and takes each
// cell's window from the lane that looked it up (wave shuffles).  ids, mask and type leave together: every cell is written once,
// nothing is cleared beforehand.  Write-bound: 12 W L bytes out (+ 28 a window), 4 (q + n) bytes in per window from two sources, each
// with offsets of its own and no alignment beyond 4 bytes.  Cell indices are 64-bit throughout.
//
// A q_row entry outside [0, n_q) is an empty question (the host form refuses it; the device form cannot read it beforehand): no
// address is formed from it.

// the question of pair r: its row in the question set, or -1 for none
__device__ __forceinline__ int64_t pw_question(const GzPairWinArgs& A, int64_t r)
{
    const int64_t qi = A.q_row ? (int64_t)A.q_row[r] : r;
    return qi >= 0 && qi < A.n_q ? qi : -1;
}

__global__ __launch_bounds__(256) void gz_pairwin_count_kernel(GzPairWinArgs A, int64_t* __restrict__ n_win)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rows) return;
    const int32_t skip = A.skip_front + A.skip_back;
    const int64_t qi = pw_question(A, r);
    int64_t Tq = qi >= 0 ? A.q_off[qi + 1] - A.q_off[qi] - skip : 0;                // absolute offsets from the ids base pointers
    Tq = Tq < 0 ? 0 : Tq;
    const int32_t q = Tq < A.max_q ? (int32_t)Tq : A.max_q;
    const int64_t room = A.max_len - 4 - q, step = room - A.stride;
    const int64_t T = A.c_off[r + 1] - A.c_off[r] - skip;
    n_win[r] = T <= room ? 1 : 1 + (T - room + step - 1) / step;
    A.pair_q[r] = q;
}

// U cells per lane and store: 4 (rows and base pointers 16-byte aligned) or 1 (any L)
template <int U>
__global__ __launch_bounds__(WAVE * 4) void gz_pairwin_fill_kernel(GzPairWinArgs A)
{
    const int lane = lane_id();
    const int64_t w0 = ((int64_t)blockIdx.x * 4 + threadIdx.x / WAVE) * WAVE;       // the wave's first window
    if (w0 >= A.n_win) return;
    const int nw = A.n_win - w0 < WAVE ? (int)(A.n_win - w0) : WAVE;
    // lane = window w0 + lane: its pair d (the last one with win_off[d] <= w; d <= w), where its question and its chunk start, q and n
    int64_t qsrc = 0, csrc = 0;
    int q = 0, n = 0;
    if (lane < nw) {
        const int64_t w = w0 + lane;
        int64_t lo = 0, hi = w < A.n_rows - 1 ? w : A.n_rows - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (A.win_off[mid] <= w) lo = mid; else hi = mid - 1;
        }
        q = A.pair_q[lo];
        const int64_t qi = pw_question(A, lo);
        if (q > 0) qsrc = A.q_off[qi] + A.skip_front;                                // (q > 0 only where the question exists)
        const int64_t room = A.max_len - 4 - q, step = room - A.stride;
        const int64_t a = A.c_off[lo], b = A.c_off[lo + 1];
        const int64_t start = (w - A.win_off[lo]) * step;
        int64_t T = b - a - A.skip_front - A.skip_back;
        T = T < 0 ? 0 : T;
        const int64_t left = T - start;                                              // > stride for every window but a lone empty one
        n = left < room ? (left > 0 ? (int)left : 0) : (int)room;
        csrc = a + A.skip_front + start;
        if (A.win_pair) A.win_pair[w] = (int32_t)lo;
        if (A.win_start) A.win_start[w] = (int32_t)start;
        if (A.win_n_real) A.win_n_real[w] = q + 4 + n;
        if (A.win_q_len) A.win_q_len[w] = q;
        if (A.ans) {
            const int64_t a0 = A.ans[2 * lo], a1 = A.ans[2 * lo + 1];
            const bool held = 0 <= a0 && a0 < a1 && a1 <= T && start <= a0 && a1 <= start + n;
            if (A.start_pos) A.start_pos[w] = held ? (int32_t)(q + 3 + a0 - start) : 0;
            if (A.end_pos) A.end_pos[w] = held ? (int32_t)(q + 3 + a1 - 1 - start) : 0;
            if (A.has_answer) A.has_answer[w] = held ? 1 : 0;
        }
    }
    const int64_t qn = (int64_t)(((uint64_t)(uint32_t)q << 32) | (uint32_t)n);      // one shuffle for both
    // the wave's nw * L cells as one range of units of U cells; unit t = (window t / Q, column U * (t % Q)), carried along instead of divided
    const int Q = A.max_len / U;
    const int64_t n_units = (int64_t)nw * Q;
    const int dj = WAVE / Q, dc = WAVE % Q;
    int j = lane / Q, col = lane % Q;
    for (int64_t base = 0; base < n_units; base += WAVE) {                           // (every lane stays in the loop: the shuffles read all of them)
        const int64_t qs_j = __shfl(qsrc, j & (WAVE - 1), WAVE);
        const int64_t cs_j = __shfl(csrc, j & (WAVE - 1), WAVE);
        const int64_t qn_j = __shfl(qn, j & (WAVE - 1), WAVE);
        const int q_j = (int)(qn_j >> 32), n_j = (int)(uint32_t)qn_j;
        if (base + lane < n_units) {
            const int k0 = col * U;
            const int c0 = q_j + 3;                                                  // ctx_col
            int32_t tok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) tok[u] = 0;
            if ((q_j > 0 || n_j > 0) && k0 < c0 + n_j) {                             // the unit may hold source cells: all its loads under ONE branch, inside a source
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u;
                    const bool from_q = n_j == 0 || (q_j > 0 && k <= q_j + 1);
                    int kk = from_q ? k - 1 : k - c0;
                    const int top = from_q ? q_j - 1 : n_j - 1;
                    kk = kk < 0 ? 0 : kk;
                    kk = kk < top ? kk : top;
                    const int32_t* const p = from_q ? A.q_ids + qs_j : A.c_ids + cs_j;
                    tok[u] = p[kk];
                }
            }
            int32_t v[U], m[U], ty[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u;
                v[u] = k == 0 ? A.bos_id : k <= q_j ? tok[u] : k < c0 ? A.eos_id : k < c0 + n_j ? tok[u] : k == c0 + n_j ? A.eos_id : A.pad_id;
                m[u] = v[u] != A.pad_id ? 1 : 0;
                ty[u] = k < q_j + 2 ? 0 : k <= c0 + n_j ? 1 : A.pad_id;
            }
            const int64_t cell = (w0 + j) * (int64_t)A.max_len + k0;
            if constexpr (U == 4) {
                nt_store4(A.out_ids + cell, v[0], v[1], v[2], v[3]);
                if (A.out_mask) nt_store4(A.out_mask + cell, m[0], m[1], m[2], m[3]);
                if (A.out_type) nt_store4(A.out_type + cell, ty[0], ty[1], ty[2], ty[3]);
            } else {
                A.out_ids[cell] = v[0];
                if (A.out_mask) A.out_mask[cell] = m[0];
                if (A.out_type) A.out_type[cell] = ty[0];
            }
        }
        col += dc; j += dj;
        if (col >= Q) { col -= Q; ++j; }
    }
}

// ---- gz_span_tokens: the word ranges of span labels as body-token ranges ------------------------------------------------------------
// counts as 64-bit words from 0 (the input of the scan); word_off absolute
__global__ __launch_bounds__(256) void gz_spantok_widen_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ word_off, int64_t n_words,
                                                               int64_t* __restrict__ cnt64)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    cnt64[i] = counts[word_off[0] + i];
}

// a thread per span: its document (the last d with mark_off[d] <= the span's absolute index), then the tokens before its two words
__global__ __launch_bounds__(256) void gz_spantok_kernel(GzSpanTokArgs A)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= A.n_marks) return;
    const int32_t f = A.mark_words[2 * m], l = A.mark_words[2 * m + 1];
    int32_t t0 = -1, t1 = -1;
    if (f >= 0 && l >= 0) {
        const int64_t ma = m + A.mark_off[0];
        int64_t lo = 0, hi = A.n_docs - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (A.mark_off[mid] <= ma) lo = mid; else hi = mid - 1;
        }
        int64_t wb = A.word_off[lo] - A.word_off[0], we = A.word_off[lo + 1] - A.word_off[0];
        wb = wb < 0 ? 0 : wb > A.n_words ? A.n_words : wb;                           // (a promise the device form cannot check: clamped into the scan)
        we = we < wb ? wb : we > A.n_words ? A.n_words : we;
        const int64_t wf = wb + f < we ? wb + f : we, wl = wb + l < we ? wb + l : we;
        t0 = (int32_t)(A.tok_off[wf] - A.tok_off[wb]);
        t1 = (int32_t)(A.tok_off[wl] - A.tok_off[wb]);
    }
    A.out[2 * m] = t0;
    A.out[2 * m + 1] = t1;
}
