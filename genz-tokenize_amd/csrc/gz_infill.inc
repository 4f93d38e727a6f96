// gz_infill.inc -- span-corruption inputs and targets over dense [R, L] rows for encoder-decoder models (included by gz_kernels.hip).
//
// The rule (include/genz_tokenize.h, "span-corruption inputs and targets"): PROTECTED, CONTINUATION, start, head, g and D are the
// mask rule's (gz_mask.inc).  n(r, c) = starts of the row at columns <= c.  A span begins at a start s when D(g(s)).x0 < t_start and
// is len(s) = 1 + #{k < n_len - 1 : D(g(s)).x1 >= len_t[k]} words long; reach(s) = n(s) + len(s) there and 0 elsewhere, far(c) the
// running maximum of reach over the row's columns <= c; a cell is chosen when it is unprotected and far(c) > n(c) (far(head(c)) ==
// far(c): no start lies between a cell and its head).  A run is a maximal stretch of chosen columns.  The encoder row E keeps every
// non-pad cell that is not chosen and puts ONE mask_id where a run begins; the target T is, run by run, mask_id and the run's ids,
// closed by one eos.  labels = T[:dec_width], decoder_input_ids = ([bos] + T[:-1])[:dec_width].
//
// One launch, the shape of gz_mask_kernel: a wave owns rows_per_wave consecutive rows and walks their cells as one flat range, 64
// cells a trip, one cell a lane (the stores are scatters, so there is no 16-byte form); the continuation bitmap is staged in LDS
// under the same size rule.  Per trip a lane knows the first lane of its own row in the trip (lane - column, or 0 when the row began
// in an earlier trip: then the carries are its row's), and under that lane mask
//   n      = popcount(start ballot, at or below the lane) + carry
//   far    = six shuffle steps of a running maximum that stop at the row's first lane, then max with the carry
//   enc position = popcount(kept ballot, below the lane) + carry
//   dec position = popcount(chosen ballot, below) + popcount(run-first ballot, at or below) + carries
// The draw runs for starts only.  Stores are monotone scatters inside the row: neighbouring kept lanes hit neighbouring addresses.
// Carries (wave-uniform, read from lane 63): n, far, kept, chosen and run counts, "the cell before is chosen", "the cell before is an
// unprotected continuation".  None needs clearing: a lane reads them only when its row began before the trip, and the two bits only
// when its column is not 0.  A row that ends in the trip is closed by the whole wave: the eos of T, the three counts, then the pad /
// 0 / ignore_index tails; a store at or beyond dec_width is dropped.  Every output cell is written exactly once, every row belongs
// to one wave: no atomics, nothing to zero beforehand.  A trip that holds padding alone (wave-uniform: one ballot) skips all of
// that -- nothing in it starts, is kept or is chosen, so its lanes hand the carries on (0 in a row that began inside it) --; the rows
// that end in it are closed as everywhere.
// Traffic per cell: 4 bytes in; 8 out over E and its tail, 8 * dec_width / row_len out over T and its tail; one LDS read; 10 Philox
// rounds a start.  Cell indices and g are 64-bit; positions inside a row are 32-bit unsigned (len(T) <= row_len + 2).

template <bool LDS>
__global__ __launch_bounds__(WAVE * 4) void gz_infill_kernel(GzInfillArgs A)
{
    extern __shared__ uint32_t infill_cont_lds[];                                    // (n_ids + 31) / 32 words when LDS
    if constexpr (LDS) {                                                             // (before any wave leaves: the barrier is the workgroup's)
        const int words = (A.n_ids + 31) >> 5;
        for (int i = threadIdx.x; i < words; i += WAVE * 4) infill_cont_lds[i] = A.cont_bits[i];
        __syncthreads();
    }
    const int lane = lane_id();
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + threadIdx.x / WAVE) * A.rows_per_wave;      // the wave's first row
    if (r0 >= A.n_rows) return;
    const int nr = A.n_rows - r0 < A.rows_per_wave ? (int)(A.n_rows - r0) : A.rows_per_wave;
    const int L = A.row_len;
    const uint32_t W = (uint32_t)A.dec_width;
    const int64_t n_cells = (int64_t)nr * L;
    const int dj = WAVE / L, dc = WAVE % L;
    int j = lane / L, col = lane % L;                                                // the lane's cell = (row r0 + j, column col), carried along instead of divided
    // (wave-uniform) the state of the row that is open at the end of a trip, as lane 63 saw it
    bool carry_nc = false, carry_ch = false;
    uint32_t carry_n = 0u, carry_far = 0u, carry_kept = 0u, carry_cho = 0u, carry_runs = 0u;
    for (int64_t base = 0; base < n_cells; base += WAVE) {                           // (every lane stays in the loop: ballots and shuffles read all of them)
        const bool in = base + lane < n_cells;
        const int64_t row = r0 + j;                                                  // < n_rows when `in`
        const int32_t tok = in ? A.ids[row * L + col] : A.pad_id;
        // the lanes of my row in this trip: lo .. ; `open`: the row began in an earlier trip and the carries are its
        const int lo = lane > col ? lane - col : 0;
        const bool open = col > lane;
        uint32_t n = open ? carry_n : 0u, far = open ? carry_far : 0u;               // what a trip of padding alone hands on: nothing in it starts,
        uint32_t kept_le = open ? carry_kept : 0u, cho_le = open ? carry_cho : 0u, runs = open ? carry_runs : 0u;      // is kept or is chosen
        uint64_t m_nc = 0ull, m_ch = 0ull;
        if (wballot(in && tok != A.pad_id)) {                                        // (wave-uniform; a third of a window batch's trips and more are padding)
            const bool prot = !in || tok == A.pad_id || tok == A.bos_id || tok == A.eos_id || tok == A.mask_id;
            bool nc = false;                                                             // unprotected continuation
            if (A.whole_word && !prot && tok >= 0 && tok < A.n_ids) {                    // (outside the snapshot: no continuation; no unk fallback)
                uint32_t w;
                if constexpr (LDS) w = infill_cont_lds[tok >> 5]; else w = A.cont_bits[tok >> 5];
                nc = ((w >> (tok & 31)) & 1u) != 0u;
            }
            m_nc = wballot(nc);
            const bool nc_before = lane > 0 ? ((m_nc >> (lane - 1)) & 1ull) != 0ull : carry_nc;
            const bool start = !prot && !(col != 0 && nc_before);
            const uint64_t seg_lt = lt_mask(lane) & ~lt_mask(lo), seg_le = seg_lt | (1ull << lane);
            const uint64_t m_start = wballot(start);
            n += (uint32_t)__builtin_popcountll(m_start & seg_le);
            uint32_t reach = 0u;
            if (start) {                                                                 // the draw: starts only, nothing else reads it
                const Philox3 d = mask_draw((uint64_t)(A.row_base + row) * (uint64_t)L + (uint64_t)col, A.key0, A.key1);
                if ((uint64_t)d.x0 < A.t_start) {
                    uint32_t len = 1u;
#pragma unroll
                    for (int k = 0; k < 15; ++k) len += (uint64_t)d.x1 >= A.len_t[k] ? 1u : 0u;     // (words behind n_len - 1 hold 2^32: never)
                    reach = n + len;
                }
            }
            uint32_t fr = reach;                                                         // running maximum, segmented by row
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const uint32_t t = __shfl_up(fr, (unsigned)d, WAVE);
                if (lane - d >= lo && t > fr) fr = t;
            }
            if (fr > far) far = fr;                                                      // (far came in as the carry of an open row)
            const bool ch = !prot && far > n;
            m_ch = wballot(ch);
            const bool ch_before = lane > 0 ? ((m_ch >> (lane - 1)) & 1ull) != 0ull : carry_ch;
            const bool first = ch && !(col != 0 && ch_before);                           // the first cell of a run
            const bool kept = in && (ch ? first : tok != A.pad_id);
            const uint64_t m_first = wballot(first), m_kept = wballot(kept);
            const uint32_t epos = (uint32_t)__builtin_popcountll(m_kept & seg_lt) + kept_le;
            runs += (uint32_t)__builtin_popcountll(m_first & seg_le);                    // at or below
            const uint32_t cho = (uint32_t)__builtin_popcountll(m_ch & seg_lt) + cho_le; // below
            const uint32_t dpos = cho + runs;                                            // where a chosen cell's id stands in T; its run's mask_id at dpos - 1 when first
            if (kept) {
                nt_store1(A.out_ids + row * L + epos, first ? A.mask_id : tok);
                if (A.out_mask) nt_store1(A.out_mask + row * L + epos, 1);
            }
            if (ch) {
                int32_t* lab = A.labels + row * (int64_t)W;
                if (first && dpos - 1u < W) nt_store1(lab + (dpos - 1u), A.mask_id);
                if (dpos < W) nt_store1(lab + dpos, tok);
                if (A.dec_ids) {                                                         // T shifted right by one behind bos
                    int32_t* dec = A.dec_ids + row * (int64_t)W;
                    if (first && dpos < W) nt_store1(dec + dpos, A.mask_id);
                    if (dpos + 1u < W) nt_store1(dec + (dpos + 1u), tok);
                }
            }
            kept_le = epos + (kept ? 1u : 0u); cho_le = cho + (ch ? 1u : 0u);           // at or below
        }
        if (in && col == 0 && A.dec_ids) nt_store1(A.dec_ids + row * (int64_t)W, A.bos_id);
        // rows that end in this trip: the wave closes them one after the other
        uint64_t m_end = wballot(in && col == L - 1);
        while (m_end) {
            const int src = __builtin_ctzll(m_end);
            m_end &= m_end - 1ull;
            const int64_t rr = r0 + __builtin_amdgcn_readlane(j, src);
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)kept_le, src), c = (uint32_t)__builtin_amdgcn_readlane((int)cho_le, src),
                           s = (uint32_t)__builtin_amdgcn_readlane((int)runs, src);
            const uint32_t t = c + s;                                                // T without its eos: at most L + 1
            int32_t* lab = A.labels + rr * (int64_t)W;
            if (lane == 0) {
                if (t < W) nt_store1(lab + t, A.eos_id);
                if (A.enc_len) A.enc_len[rr] = (int32_t)e;
                if (A.dec_len) A.dec_len[rr] = (int32_t)(t + 1u);
                if (A.n_spans) A.n_spans[rr] = (int32_t)s;
            }
            for (uint32_t i = e + (uint32_t)lane; i < (uint32_t)L; i += WAVE) {
                nt_store1(A.out_ids + rr * L + i, A.pad_id);
                if (A.out_mask) nt_store1(A.out_mask + rr * L + i, 0);
            }
            for (uint64_t i = (uint64_t)t + 1u + (uint64_t)lane; i < W; i += WAVE) {
                nt_store1(lab + i, A.ignore_index);
                if (A.dec_ids) nt_store1(A.dec_ids + rr * (int64_t)W + i, A.pad_id);
            }
        }
        carry_nc = (m_nc >> (WAVE - 1)) != 0ull;
        carry_ch = (m_ch >> (WAVE - 1)) != 0ull;
        carry_n = (uint32_t)__builtin_amdgcn_readlane((int)n, WAVE - 1);
        carry_far = (uint32_t)__builtin_amdgcn_readlane((int)far, WAVE - 1);
        carry_kept = (uint32_t)__builtin_amdgcn_readlane((int)kept_le, WAVE - 1);
        carry_cho = (uint32_t)__builtin_amdgcn_readlane((int)cho_le, WAVE - 1);
        carry_runs = (uint32_t)__builtin_amdgcn_readlane((int)runs, WAVE - 1);
        col += dc; j += dj;
        if (col >= L) { col -= L; ++j; }
    }
}
