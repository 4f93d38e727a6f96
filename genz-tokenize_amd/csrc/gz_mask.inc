// gz_mask.inc -- masked-LM inputs and labels over dense [R, L] rows, whole-word (included by gz_kernels.hip).
//
// The rule (include/genz_tokenize.h, "masked-LM inputs and labels"): a cell is PROTECTED when its id is pad, bos, eos or mask_id; an
// unprotected cell is a word START when it is the row's first cell or the cell before it is protected or is no continuation token
// (a token of the decoder snapshot whose word ends in "@@": one bit an id, made with the snapshot from GZ_DEC_ENDS_ATAT); its HEAD
// is the nearest start at or before it (the cell itself without whole_word).  With D(g) = Philox4x32-10 of the cell's global index g = (row_base + r) * L + c under the seed,
// a cell is chosen when D(g(head)).x0 < t_sel, and a chosen cell becomes mask_id (D(g).x1 < t1), a random id (x1 < t2: rand_lo +
// mulhi(x2, rand_hi - rand_lo)) or stays.  The draw is a function of (seed, g) alone: no state, no dependence on the launch shape.
//
// One launch.  Work is divided over CELLS: a wave owns rows_per_wave consecutive rows and walks their cells as one flat range, 64
// units of U cells a trip -- 16 bytes a lane where the rows are 16-byte aligned (L % 4 == 0), one cell a lane otherwise; a unit never
// straddles a row.  A lane looks up the continuation bit of each of its ids and draws D for each unprotected cell -- padding costs
// neither.  The bitmap (6 KB for the bundled vocabulary) is staged in LDS by every workgroup while it fits GZ_MASK_LDS_MAX_BYTES, so
// the lookup is an LDS read (ds_read_b32: the LDS form is a template parameter, not a pointer select) instead of a dependent gather
// from the 775 KB of decoder entries in L2; beyond that size, or with the switch mask_lds = 0, it is a gather from the bitmap in memory.
// Heads: inside a lane the U cells are walked in order; across lanes ONE
// ballot says which lanes hold a start and one says whether each lane's LAST start is chosen, so a cell without a start in its own
// lane reads its head's bit out of the second mask at the highest set bit of the first below it -- no shuffle; a word that began in
// an earlier trip takes the carried bit (the ballot-per-trip, carry-across-trips pattern of gz_near.inc).  The carry needs no
// clearing: column 0 and the cell behind a protected cell are starts by definition, so only cells of the carried word ever read it.
// n_chosen: popcounts of the chosen ballots under each row's lane mask, kept in a scalar while the row is open and stored once --
// every row belongs to one wave, so there are no atomics and nothing to zero beforehand.
// Traffic per cell: 4 bytes in, 8 out (non-temporal: written once), one LDS read; the bitmap once a workgroup (about 16 K cells)
// from L2; 10 Philox rounds = 20 32x32->64 multiplies.  Cell indices and g are 64-bit throughout.

// U cells per lane, load and store: 4 (rows and base pointers 16-byte aligned) or 1 (any L); LDS: the continuation bitmap is staged in LDS
template <int U, bool LDS>
__global__ __launch_bounds__(WAVE * 4) void gz_mask_kernel(GzMaskArgs A)
{
    extern __shared__ uint32_t mask_cont_lds[];                                      // (n_ids + 31) / 32 words when LDS
    if constexpr (LDS) {                                                             // (before any wave leaves: the barrier is the workgroup's)
        const int words = (A.n_ids + 31) >> 5;
        for (int i = threadIdx.x; i < words; i += WAVE * 4) mask_cont_lds[i] = A.cont_bits[i];
        __syncthreads();
    }
    const int lane = lane_id();
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + threadIdx.x / WAVE) * A.rows_per_wave;      // the wave's first row
    if (r0 >= A.n_rows) return;
    const int nr = A.n_rows - r0 < A.rows_per_wave ? (int)(A.n_rows - r0) : A.rows_per_wave;
    // the wave's nr * L cells as one range of units of U cells; unit t = (row t / Q, column U * (t % Q)), carried along instead of divided
    const int Q = A.row_len / U;
    const int64_t n_units = (int64_t)nr * Q;
    const int dj = WAVE / Q, dc = WAVE % Q;
    int j = lane / Q, col = lane % Q;
    bool carry_nc = false, carry_ch = false;          // (wave-uniform) the cell before this trip is an unprotected continuation; its word is chosen
    int open_row = -1, open_cnt = 0;                  // (wave-uniform) the row whose count is still growing
    for (int64_t base = 0; base < n_units; base += WAVE) {                           // (every lane stays in the loop: the ballots read all of them)
        const bool in = base + lane < n_units;
        const int k0 = col * U;
        const int64_t cell = (r0 + j) * (int64_t)A.row_len + k0;                     // within this call's arrays; < n_rows * row_len when `in`
        int32_t tok[U];
        if (in) {
            if constexpr (U == 4) {
                typedef int __attribute__((ext_vector_type(4))) v4i;
                const v4i v = *reinterpret_cast<const v4i*>(A.ids + cell);
                tok[0] = v.x; tok[1] = v.y; tok[2] = v.z; tok[3] = v.w;
            } else tok[0] = A.ids[cell];
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) tok[u] = A.pad_id;
        }
        bool prot[U], nc[U];                                                         // protected; unprotected continuation
#pragma unroll
        for (int u = 0; u < U; ++u) {
            prot[u] = !in || tok[u] == A.pad_id || tok[u] == A.bos_id || tok[u] == A.eos_id || tok[u] == A.mask_id;
            nc[u] = false;
        }
        if (A.whole_word) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!prot[u] && tok[u] >= 0 && tok[u] < A.n_ids) {                   // (outside the snapshot: no continuation; no unk fallback)
                    uint32_t w;
                    if constexpr (LDS) w = mask_cont_lds[tok[u] >> 5]; else w = A.cont_bits[tok[u] >> 5];
                    nc[u] = ((w >> (tok[u] & 31)) & 1u) != 0u;
                }
            }
        }
        // the draws: every unprotected cell (a start needs x0, a chosen cell x1 and x2)
        const uint64_t g0 = (uint64_t)(A.row_base + r0 + j) * (uint64_t)A.row_len + (uint64_t)k0;
        Philox3 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            d[u] = Philox3{0u, 0u, 0u};
            if (!prot[u]) d[u] = mask_draw(g0 + (uint64_t)u, A.key0, A.key1);
        }
        // starts, and each start's own decision
        const uint64_t nc_last = wballot(nc[U - 1]);
        const bool nc_before = lane > 0 ? ((nc_last >> (lane - 1)) & 1ull) != 0ull : carry_nc;
        bool start[U], sel[U];
        bool any_start = false, last_sel = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool prev_nc = u == 0 ? (k0 != 0 && nc_before) : nc[u > 0 ? u - 1 : 0];
            start[u] = !prot[u] && !prev_nc;
            sel[u] = start[u] && (uint64_t)d[u].x0 < A.t_sel;
            if (start[u]) { any_start = true; last_sel = sel[u]; }
        }
        // heads: the nearest start at or below -- in the lane, else the last start of the highest lane below that has one, else the carry
        const uint64_t m_any = wballot(any_start), m_sel = wballot(last_sel);
        const uint64_t below_me = m_any & lt_mask(lane);
        bool cur = below_me ? ((m_sel >> (63 - __builtin_clzll(below_me))) & 1ull) != 0ull : carry_ch;
        bool ch[U];
        int32_t out[U], lab[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (start[u]) cur = sel[u];
            ch[u] = !prot[u] && cur;
            out[u] = tok[u];
            lab[u] = A.ignore_index;
            if (ch[u]) {
                lab[u] = tok[u];
                const uint64_t a = d[u].x1;
                if (a < A.t1) out[u] = A.mask_id;
                else if (a < A.t2) out[u] = (int32_t)((uint32_t)A.rand_lo + __umulhi(d[u].x2, A.rand_span));
            }
        }
        if (in) {
            if constexpr (U == 4) {
                nt_store4(A.out_ids + cell, out[0], out[1], out[2], out[3]);
                nt_store4(A.labels + cell, lab[0], lab[1], lab[2], lab[3]);
            } else {
                nt_store1(A.out_ids + cell, out[0]);
                nt_store1(A.labels + cell, lab[0]);
            }
        }
        if (A.n_chosen) {                                                            // rows of this trip: first .. last, at most 1 + 64 / Q
            uint64_t m_ch[U];
#pragma unroll
            for (int u = 0; u < U; ++u) m_ch[u] = wballot(ch[u]);
            const int n_act = n_units - base < WAVE ? (int)(n_units - base) : WAVE;
            const int j_first = __builtin_amdgcn_readfirstlane(j), j_last = __builtin_amdgcn_readlane(j, n_act - 1);
            for (int jj = j_first; jj <= j_last; ++jj) {
                const uint64_t m_row = wballot(in && j == jj);
                int cnt = 0;
#pragma unroll
                for (int u = 0; u < U; ++u) cnt += __builtin_popcountll(m_ch[u] & m_row);
                if (jj != open_row) {
                    if (open_row >= 0 && lane == 0) A.n_chosen[r0 + open_row] = open_cnt;
                    open_row = jj; open_cnt = 0;
                }
                open_cnt += cnt;
            }
        }
        carry_nc = (nc_last >> (WAVE - 1)) != 0ull;
        if (m_any) carry_ch = ((m_sel >> (63 - __builtin_clzll(m_any))) & 1ull) != 0ull;
        col += dc; j += dj;
        if (col >= Q) { col -= Q; ++j; }
    }
    if (A.n_chosen && open_row >= 0 && lane == 0) A.n_chosen[r0 + open_row] = open_cnt;
}
