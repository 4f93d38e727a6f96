// BPE-dropout (Provilkov et al., 2020): the merge stage of a dropout call (included by gz_kernels.hip after gz_hot.inc, same
// translation unit).  A dropout call runs the pipeline as a call without the whole-word tables does -- classification, scans, word
// kernel, pre-pass, row kernels: unchanged -- and only the kernels that run the merge loop are these instead of gz_miss2_kernel /
// gz_miss_wide_kernel / gz_long_kernel.  They honour the same contracts: the sorted miss list mq and the wide list wlist in, word
// records in near and far form out, a word that ends as one piece gets the piece's id as its record, token places as the pre-pass
// reserved them (by symbol count: a dropout result never has more pieces than symbols).
//
// The rule (include/genz_tokenize.h "BPE-dropout", tests/dropout_oracle.py).  Only the merge loop of one word changes; its draws are
// a pure function of (seed, D, j, t, i): D the global document index (doc0 + d), j the word's index within its document, t the merge
// iteration, i the position in the word's current symbol list.
//   key(seed, D, j) = Philox4x32-10(counter (D lo, D hi, j, 0), key (seed lo, seed hi)) words 0, 1
//   u(key, t, i)    = Philox4x32-10(counter (t, i >> 2, 0, 0), key) word i & 3          -- one call serves four neighbouring positions
//   iteration t: the pairs (s[i], s[i+1]) with u(key, t, i) >= thr that the merge table holds are live; none: the word is finished;
//   else the smallest rank among them is merged at every live position that holds it, left to right, never overlapping (a dropped
//   occurrence of that pair stays as it is).  An iteration merges at least once: at most n - 1 iterations, no spins, no retries.
//
//   gz_dmiss_kernel   words of <= 16 symbols, ONE LANE PER WORD, 64 words of a sorted chunk side by side: symbols in registers with
//                     a copy in the lane's LDS row, the pair table's displacement array in LDS, one Philox call per four positions
//                     and iteration, the word key once per word
//   gz_dwide_kernel   longer words, one wave per word (wave_merge_drop: the candidate ballot is masked with the keep bits before
//                     the minimum and before the pick; the greedy l == r pick runs over the surviving matches, with its carry across
//                     the 64-position tiles)
//   a word's document: a binary search of its global word index in docw0 (the launcher puts gz_docw0_kernel on the main stream)

namespace {

struct Philox4 { uint32_t x0, x1, x2, x3; };

// Philox4x32-10 (Salmon et al., SC'11), all four output words
__device__ __forceinline__ Philox4 philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

// u(key, t, i) for one position (the lane-per-symbol forms: a lane holds one position)
__device__ __forceinline__ uint32_t drop_u(uint32_t k0, uint32_t k1, uint32_t t, uint32_t i)
{
    const Philox4 x = philox4(t, i >> 2, 0u, 0u, k0, k1);
    const uint32_t q = i & 3u;
    return q == 0u ? x.x0 : q == 1u ? x.x1 : q == 2u ? x.x2 : x.x3;
}

// the key of word `widx` (global index within the text of X): its document by a search in docw0[0 .. n_docs) -- the LAST document
// whose first word is <= widx (empty documents share their successor's first word) -- and its index within that document
__device__ __forceinline__ void drop_word_key(const GzTextBufs& X, int64_t n_docs, const GzDrop& R, uint32_t widx, uint32_t& k0, uint32_t& k1)
{
    typedef const uint32_t __attribute__((address_space(1)))* g32_t;
    const g32_t dw = (g32_t)X.docw0;
    int64_t lo = 0, hi = n_docs;                                  // first d in [0, n_docs) with docw0[d] > widx (n_docs: none)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (dw[mid] > widx) hi = mid; else lo = mid + 1;
    }
    const int64_t d = lo > 0 ? lo - 1 : 0;                        // (docw0[0] == 0 <= widx: lo >= 1)
    const uint32_t j = widx - dw[d];
    const uint64_t D = (uint64_t)R.doc0 + (uint64_t)d;
    const Philox4 x = philox4((uint32_t)D, (uint32_t)(D >> 32), j, 0u, (uint32_t)R.seed, (uint32_t)(R.seed >> 32));
    k0 = x.x0; k1 = x.x1;
}

// wave_merge (gz_kernels.hip) under dropout: S[0 .. n) in LDS or global scratch, one lane per position, tiles of 64 positions
__device__ __noinline__ int wave_merge_drop(const GzDeviceTables* Tp, uint32_t* S, int n, int lane, bool global_scratch, uint32_t k0, uint32_t k1,
                                            uint64_t thr)
{
    const GzDeviceTables& T = *Tp;
    uint32_t t = 0;
    while (n > 1) {
        uint32_t best = GZ_RANK_NONE;
        for (int i = lane; i < n - 1; i += WAVE) {
            if ((uint64_t)drop_u(k0, k1, t, (uint32_t)i) >= thr) {       // a dropped position is no candidate: neither for the minimum ...
                const uint32_t r = probe_rank(T, S[i], S[i + 1]);
                best = r < best ? r : best;
            }
        }
        best = wave_min_u32(best);
        if (best == GZ_RANK_NONE) break;                           // nothing survived: the word is finished
        const GzMergeInfo mi = T.merges[best];
        int out = 0;
        bool skip0 = false;                                        // S[base] is the `second` of a pair merged in the tile before
        for (int base = 0; base < n; base += WAVE) {
            const int i = base + lane;
            const uint32_t s = i < n ? S[i] : GZ_NO_SYMBOL;
            const uint32_t s1 = i + 1 < n ? S[i + 1] : GZ_NO_SYMBOL;
            const uint64_t valid = wballot(i < n);
            bool cand = i + 1 < n && s == mi.left && s1 == mi.right;
            if (cand) cand = (uint64_t)drop_u(k0, k1, t, (uint32_t)i) >= thr;      // ... nor for the pick
            uint64_t m = wballot(cand);
            if (skip0) m &= ~1ull;
            uint64_t pick = m;
            if (mi.left == mi.right) {                             // overlapping candidates: greedy left to right over the survivors
                pick = 0;
                uint64_t rem = m;
                while (rem) {
                    const uint64_t low = rem & (0 - rem);
                    pick |= low;
                    rem &= ~(low | (low << 1));
                }
            }
            const uint64_t keep = valid & ~((pick << 1) | (skip0 ? 1ull : 0ull));
            skip0 = (pick >> 63) & 1ull;
            const uint32_t val = ((pick >> lane) & 1ull) ? mi.merged : s;
            const int dest = out + below(keep);
            if ((keep >> lane) & 1ull) S[dest] = val;
            out += __popcll(keep);
        }
        n = out;
        ++t;
        if (global_scratch) __threadfence();
    }
    return n;
}

// long_word (gz_kernels.hip) under dropout: bytes g[0 .. nbytes) of ONE word, an optional glued line feed; the symbols go to the LDS
// scratch when they fit, else to arena_slot (never null here)
__device__ __noinline__ int long_word_drop(const GzDeviceTables* Tp, uint32_t* lds_scratch, int lds_cap, const uint8_t* g, int64_t nbytes, bool glue,
                                           uint32_t* arena_slot, Emit E, int lane, uint32_t k0, uint32_t k1, uint64_t thr)
{
    const GzDeviceTables& T = *Tp;
    auto at = [&](int64_t i) -> uint32_t { return g[i]; };
    int leads = 0;
    for (int64_t i = lane; i < nbytes; i += WAVE) leads += (g[i] & 0xC0) != 0x80;
    const int64_t nsym64 = (int64_t)wave_sum(leads) + (glue ? 1 : 0);
    uint32_t* S = lds_scratch;
    bool global_scratch = false;
    if (nsym64 > lds_cap) { S = arena_slot; global_scratch = true; }
    int n = (int)nsym64;
    int symbase = 0;
    for (int64_t base = 0; base < nbytes; base += WAVE) {
        const int64_t i = base + lane;
        const bool lead = i < nbytes && (g[i] & 0xC0) != 0x80;
        const uint64_t m = wballot(lead);
        if (lead) {
            int len;
            const uint32_t cp = decode_cp(at, i, nbytes, len);
            const int idx = symbase + below(m);
            S[idx] = initial_symbol(T, cp, !glue && idx == n - 1);
        }
        symbase += __popcll(m);
    }
    if (glue && lane == 0) S[n - 1] = initial_symbol(T, 0x0Au, true);
    if (global_scratch) __threadfence();
    if (n > 1) n = wave_merge_drop(Tp, S, n, lane, global_scratch, k0, k1, thr);
    for (int base = 0; base < n; base += WAVE) {
        const int i = base + lane;
        if (i < n) {
            if (E.symout) { if (E.ntok + i < E.limit) E.symout[E.ntok + i] = (int32_t)S[i]; }
            else emit_at(E, E.ntok + i, token_id(T, S[i], i == n - 1));
        }
    }
    return E.ntok + n;
}

constexpr int DM_WPB = 8;                     // waves per workgroup of gz_dmiss_kernel: 34 KB of rows + the displacement array, two workgroups per CU
constexpr int DM_N = M2_N;                    // symbols per word at most (longer: gz_dwide_kernel)

}  // namespace

// LD: the pair table's displacement array is staged in LDS (else read from memory).  ONE instance takes every chunk of the sorted
// list (the plain merge kernel's split into a 16- and an 8-symbol instance is a register-budget matter of that kernel).
template <bool LD>
__global__ __launch_bounds__(WAVE * DM_WPB) void gz_dmiss_kernel(const GzDeviceTables* __restrict__ Tp, GzTextBufs X, int64_t n_docs, GzDrop R)
{
    constexpr int NS = DM_N, STRIDE = NS + 1;
    extern __shared__ __attribute__((aligned(16))) uint8_t dm_dyn[];      // [DM_WPB] Miss2Wave, the displacement array
    typedef const uint32_t __attribute__((address_space(1)))* g32_t;
    typedef uint32_t __attribute__((address_space(3)))* l32_t;
    Miss2Wave* wl = reinterpret_cast<Miss2Wave*>(dm_dyn);
    uint16_t* ldisp = LD ? reinterpret_cast<uint16_t*>(dm_dyn + DM_WPB * sizeof(Miss2Wave)) : nullptr;
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const GzDeviceTables T = *Tp;
    const uint32_t M = X.blkmiss[X.nblk];
    const uint32_t ntile = (M + M2_TILE - 1u) / M2_TILE, nchunk = ntile * (M2_TILE / WAVE);
    if (blockIdx.x * (uint32_t)DM_WPB >= nchunk) return;          // (the whole workgroup: nothing to do)
    if (LD) stage_disp(ldisp, T.pair_ph);
    __syncthreads();
    const l32_t Sl = (l32_t)(wl[wv].s + lane * STRIDE);           // this lane's 17 dwords
    const uint32_t nl_final = T.bmp[0x0A].final_;                 // symbol of "\n</w>" (a glued line feed)
    const uint64_t thr = R.thr;
    // position p of the walk: chunk p / ntile of tile p % ntile -- every tile's longest chunk first (a tile is sorted longest first)
    for (uint32_t p = blockIdx.x * (uint32_t)DM_WPB + (uint32_t)wv; p < nchunk; p += gridDim.x * (uint32_t)DM_WPB) {
        const uint32_t kk = p / ntile, tile = p - kk * ntile;
        const uint32_t total = X.tcnt[tile] & 0xFFFFu;            // records of the tile
        if (kk * WAVE >= total) continue;                         // (wave-uniform)
        bool in = kk * WAVE + (uint32_t)lane < total;
        if (in && !GZ_CHK(701, (size_t)tile * M2_TILE + kk * WAVE + lane, X.wmax)) in = false;
        uint4 mr = in ? X.mq[(size_t)tile * M2_TILE + kk * WAVE + lane] : make_uint4(0u, 0u, 0u, 0u);
        if (in && !(GZ_CHK(702, mr.x, X.wmax) && GZ_CHK(703, mr.y, X.B) && GZ_CHK(704, mr.w, 2 * (X.B + 32)) && GZ_CHK(705, (uint64_t)(mr.z & 0x7FFFu) + mr.y, X.B + 1))) {
            in = false; mr = make_uint4(0u, 0u, 0u, 0u);
        }
        const uint32_t widx = mr.x, start = mr.y, rec = mr.z, tbase = mr.w;     // tbase: the word's place in the compact token area
        const int nb = in ? (int)(rec & 0x7FFFu) : 0;
        const bool glue = (rec & 0x8000u) != 0;
        // ---- the word's key: its document (a search in docw0) and its index there
        uint32_t key0 = 0, key1 = 0;
        if (in) drop_word_key(X, n_docs, R, widx, key0, key1);
        // ---- the word's bytes -> this lane's LDS row (at most 64: the pre-pass sent longer words away)
        {
            const int nch = (nb + 15) >> 4;
#pragma unroll
            for (int c = 0; c < NS / 4; ++c) {
                if (wballot(c < nch) == 0) break;
                if (c < nch) {
                    uint32_t w[4];
                    load16(X.tb, (int64_t)start + 16 * c, X.B, w);
                    Sl[4 * c] = w[0]; Sl[4 * c + 1] = w[1]; Sl[4 * c + 2] = w[2]; Sl[4 * c + 3] = w[3];
                }
            }
        }
        // ---- code points -> initial symbols (tuple(token), word[-1] + "</w>": tokenize.py:63-64), as gz_miss2_kernel makes them
        uint32_t sym[NS];
        int n = 0;
        bool over = false, stray = false;
        {
            int q = 0;
            const int jdec = wave_max_i32(nb);                      // (a symbol has at least one byte)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                sym[j] = GZ_NO_SYMBOL;
                if (j >= jdec) continue;                             // (wave-uniform)
                const bool act = q < nb;
                const uint32_t pa = act ? (uint32_t)q : 0u;         // (two ALIGNED dwords of the row: q < nb <= 4 NS, so q / 4 + 1 <= NS)
                const uint32_t f = __builtin_amdgcn_alignbyte(Sl[(pa >> 2) + 1u], Sl[pa >> 2], pa & 3u);
                const uint32_t c0b = f & 0xFFu;
                int want = c0b < 0x80u ? 1 : c0b < 0xE0u ? 2 : c0b < 0xF0u ? 3 : 4;
                if (q + want > nb) want = nb - q;                    // structural decode, never past the end of the word
                uint32_t cp = c0b;
                if (c0b >= 0x80u) {
                    cp = want == 2 ? (c0b & 0x1Fu) : want == 3 ? (c0b & 0x0Fu) : want == 4 ? (c0b & 0x07u) : (c0b & 0x3Fu);
                    if (want > 1) cp = (cp << 6) | ((f >> 8) & 0x3Fu);
                    if (want > 2) cp = (cp << 6) | ((f >> 16) & 0x3Fu);
                    if (want > 3) cp = (cp << 6) | ((f >> 24) & 0x3Fu);
                }
                // (a code point that starts at a continuation byte -- bytes that are not UTF-8 -- decodes to more symbols than the
                //  pre-pass reserved token places for: the wave-cooperative path below, tokens at the word's own byte offset)
                stray |= act && (c0b & 0xC0u) == 0x80u;
                if (act) {
                    const bool last = !glue && q + want >= nb;
                    if (cp < 0x10000u) sym[j] = ((g32_t)T.bmp)[2u * cp + (last ? 1u : 0u)];   // (entries of unknown code points hold GZ_SYM_UNKNOWN | cp)
                    else sym[j] = initial_symbol(T, cp, last);
                    q += want;
                    n = j + 1;
                }
            }
            if (q < nb) over = true;                                 // more than 16 code points
            over |= stray;
            if (glue) { if (n < NS) n += 1; else over = true; }
        }
        if (over) n = 0;
        // a glued "\n" is the last symbol; symbols -> the LDS row (over the bytes)
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            if (glue && j == n - 1) sym[j] = nl_final;
            if (wballot(j < n) == 0) break;
            if (j < n) Sl[j] = sym[j];
        }
        // ---- merge iterations: iteration t of every live lane is the loop's own count (a lane that merges nothing is finished)
        bool live = n > 1;
        for (uint32_t t = 0;; ++t) {
            const int jmax = wave_max_i32(live ? n : 0) - 1;         // pairs 0 .. jmax-1 exist somewhere in the wave
            if (jmax < 1) break;
            // the keep bits of this iteration: ONE Philox call per four positions
            uint32_t keepm = 0;
#pragma unroll
            for (int g = 0; g < (NS - 1 + 3) / 4; ++g) {
                if (4 * g >= jmax) continue;                         // (wave-uniform)
                if (live && 4 * g < n - 1) {
                    const Philox4 x = philox4(t, (uint32_t)g, 0u, 0u, key0, key1);
                    keepm |= ((uint64_t)x.x0 >= thr ? 1u : 0u) << (4 * g);
                    keepm |= ((uint64_t)x.x1 >= thr ? 2u : 0u) << (4 * g);
                    keepm |= ((uint64_t)x.x2 >= thr ? 4u : 0u) << (4 * g);
                    keepm |= ((uint64_t)x.x3 >= thr ? 8u : 0u) << (4 * g);
                }
            }
            // the surviving pairs the table holds, and the smallest rank among them (ranks are unique: every position of that rank
            // holds the same pair and merges to the same symbol)
            uint32_t rk[NS - 1];
            uint32_t best = GZ_RANK_NONE, merged = 0;
#pragma unroll
            for (int j = 0; j < NS - 1; ++j) {
                rk[j] = GZ_RANK_NONE;
                if (j >= jmax) continue;                             // (wave-uniform)
                if (live && j + 1 < n && ((keepm >> j) & 1u)) {
                    uint32_t mj = 0;
                    rk[j] = probe_pair(T, sym[j], sym[j + 1], mj, ldisp);
                    if (rk[j] < best) { best = rk[j]; merged = mj; }
                }
            }
            live = live && best != GZ_RANK_NONE;                     // nothing survived: the word is finished
            if (wballot(live) == 0) break;
            // every surviving occurrence, left to right, non-overlapping, compacted into the LDS row
            {
                int out = 0;
                bool skip = false;
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    if (j > jmax) continue;                          // (wave-uniform: n <= jmax + 1)
                    const bool here = live && j < n && !skip;
                    const bool hit = here && j + 1 < n && rk[j < NS - 1 ? j : NS - 2] == best && j < NS - 1;
                    if (here) { Sl[out] = hit ? merged : sym[j]; ++out; }
                    skip = hit;
                }
                if (live) n = out;
            }
            live = live && n > 1;
            {
                const int jr = wave_max_i32(live ? n : 0);           // read back what the next iteration looks at
#pragma unroll
                for (int j = 0; j < NS; ++j) { if (j >= jr) break; sym[j] = Sl[j]; }
            }
        }
        // ---- ids of the pieces (encoder.get(piece, unk), tokenize.py:120-121) and the word's record, as gz_miss2_kernel leaves them
        const bool rv = in && !over;
        if (wballot(rv)) {
            typedef const int32_t __attribute__((address_space(1)))* gi32_t;
            const int nmax = wave_max_i32(rv ? n : 0);
            int32_t id0 = 0;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (j >= nmax) break;                                // (wave-uniform)
                if (rv && j < n) {
                    const uint32_t s = Sl[j];
                    const int32_t id = (s & GZ_SYM_UNKNOWN) ? T.unk_id : ((gi32_t)T.sym_ids)[2u * s + (j == n - 1 ? 1u : 0u)];
                    if (n > 1 && GZ_CHK(706, (uint64_t)tbase + j, 2 * (X.B + 32))) X.mtok[tbase + j] = id;
                    if (j == 0) id0 = id;
                }
            }
            if (rv) {
                const uint32_t place = tbase - ((uint32_t)X.B + 32u);
                if (n == 1) X.wtok[widx] = (uint32_t)id0;            // ONE piece: its id is the word's record
                else if (place < X.near_lim) X.wtok[widx] = W_MISS | W_NEAR | ((uint32_t)(n - 1) << 25) | place;
                else { X.wtok[widx] = W_MISS | (uint32_t)n; X.waux[widx] = tbase; }
            }
        }
        // a word the pre-pass counted at <= 16 symbols that decodes to more (bytes that are not UTF-8): wave-cooperative, here and now
        uint64_t ob = wballot(in && over);
        while (ob) {
            const int src = __ffsll((unsigned long long)ob) - 1;
            ob &= ob - 1;
            const uint32_t lw = (uint32_t)__shfl((int)widx, src, WAVE), lstart = (uint32_t)__shfl((int)start, src, WAVE);
            const uint32_t lrec = (uint32_t)__shfl((int)rec, src, WAVE);
            const uint32_t lk0 = (uint32_t)__shfl((int)key0, src, WAVE), lk1 = (uint32_t)__shfl((int)key1, src, WAVE);
            Emit E;
            E.ids = X.mtok + lstart; E.mask = nullptr; E.symout = nullptr; E.pad_hit = nullptr;
            E.limit = 0x7FFFFFFF; E.stop = 0x7FFFFFFF; E.ntok = 0; E.pad_id = 0x7FFFFFFF;
            const int nt = long_word_drop(Tp, wl[wv].s, WAVE * STRIDE, X.tb + lstart, (int64_t)(lrec & 0x7FFFu), (lrec & 0x8000u) != 0,
                                          reinterpret_cast<uint32_t*>(X.mtok + lstart), E, lane, lk0, lk1, thr);
            if (lane == 0) { X.wtok[lw] = W_MISS | (uint32_t)nt; X.waux[lw] = lstart; }
        }
    }
}

// words of more than 16 symbols (the list gz_mpre_kernel made): one wave per word, whatever its length -- up to PLONG symbols in LDS,
// beyond that in the word's own place of the token area (a word has at least as many bytes as symbols)
__global__ __launch_bounds__(WAVE * PWPB) void gz_dwide_kernel(const GzDeviceTables* __restrict__ Tp, GzTextBufs X, int64_t n_docs, GzDrop R)
{
    __shared__ uint32_t lsym[PWPB][PLONG];
    const int lane = lane_id();
    const uint32_t n = X.wlist[0];
    for (uint32_t i = blockIdx.x * PWPB + threadIdx.x / WAVE; i < n; i += gridDim.x * PWPB) {
        if (!GZ_CHK(711, (uint64_t)1 + i, X.wmax + 7)) continue;
        const uint32_t lw = X.wlist[1 + i];
        if (!GZ_CHK(712, lw, X.wmax)) continue;
        const uint32_t lrec = X.wtok[lw];
        if ((lrec & (W_MISS | W_PEND | W_LONG)) != (W_MISS | W_PEND | W_LONG)) continue;
        const uint32_t lstart = X.waux[lw];
        if (!GZ_CHK(713, lstart, X.B)) continue;
        int64_t lnb = lrec & 0x7FFFu;
        if (lnb == 0x7FFF)                                         // length did not fit 15 bits: find the end again
            lnb = scan_word_end(X, (int64_t)lstart + 1) - lstart;
        if (!GZ_CHK(714, (uint64_t)lstart + (uint64_t)lnb, X.B + 1)) continue;
        uint32_t k0, k1;
        drop_word_key(X, n_docs, R, lw, k0, k1);
        Emit E;
        E.ids = X.mtok + lstart; E.mask = nullptr; E.symout = nullptr; E.pad_hit = nullptr;
        E.limit = 0x7FFFFFFF; E.stop = 0x7FFFFFFF; E.ntok = 0; E.pad_id = 0x7FFFFFFF;
        const int nt = long_word_drop(Tp, lsym[threadIdx.x / WAVE], PLONG, X.tb + lstart, lnb, (lrec & 0x8000u) != 0,
                                      reinterpret_cast<uint32_t*>(X.mtok + lstart), E, lane, k0, k1, R.thr);
        if (lane == 0) X.wtok[lw] = W_MISS | (uint32_t)nt;        // (far record: waux holds the word's byte offset since the pre-pass)
    }
}

// Tokenize.bpe_dropout(token): the whole input is ONE word; the caller names its document and its index there
__global__ __launch_bounds__(WAVE) void gz_bpe_word_drop_kernel(const GzDeviceTables* __restrict__ Tp, const uint8_t* word, int64_t nbytes, uint32_t* arena,
                                                                 int32_t* out, int32_t cap, int32_t* n_out, GzDrop R, uint32_t word_index)
{
    __shared__ uint32_t lsym[1024];
    const int lane = lane_id();
    const uint64_t D = (uint64_t)R.doc0;
    const Philox4 x = philox4((uint32_t)D, (uint32_t)(D >> 32), word_index, 0u, (uint32_t)R.seed, (uint32_t)(R.seed >> 32));
    Emit E;
    E.ids = nullptr; E.mask = nullptr; E.pad_hit = nullptr; E.symout = out; E.limit = cap; E.stop = 0x7FFFFFFF; E.ntok = 0; E.pad_id = Tp->pad_id;
    const int nt = long_word_drop(Tp, lsym, 1024, word, nbytes, false, arena, E, lane, x.x0, x.x1, R.thr);
    if (lane == 0) *n_out = nt;
}

// -----------------------------------------------------------------------------------------------------------------
void gz_launch_drop_miss(const GzOptions& O, const GzDeviceTables* T, const GzDeviceTables& Th, const GzTextBufs& X, int64_t n_docs, const GzDrop& R, hipStream_t s)
{
    const int64_t gmax = X.wmax / WAVE + 1;                         // chunks of 64 misses at most (every word)
    const bool ld = Th.pair_ph.nbuckets <= GZ_PH_LDS_BUCKETS;
    static const bool attr = [] {                                  // (more than 64 KB of dynamic LDS needs the attribute)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gz_dmiss_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gz_dmiss_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
        return true;
    }();
    (void)attr;
    const size_t lds = DM_WPB * sizeof(Miss2Wave) + (ld ? (size_t)Th.pair_ph.nbuckets * 2 : 0);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((160u << 10) / (lds + 512), 32 / DM_WPB));
    int64_t grid = O.hot_miss_wgs > 0 ? O.hot_miss_wgs : 256 * per_cu;
    const int64_t need = (gmax + DM_WPB - 1) / DM_WPB;
    if (grid > need) grid = need;
    if (ld) hipLaunchKernelGGL(gz_dmiss_kernel<true>, dim3((unsigned)grid), dim3(WAVE * DM_WPB), lds, s, T, X, n_docs, R);
    else hipLaunchKernelGGL(gz_dmiss_kernel<false>, dim3((unsigned)grid), dim3(WAVE * DM_WPB), lds, s, T, X, n_docs, R);
}

void gz_launch_drop_wide(const GzDeviceTables* T, const GzTextBufs& X, int64_t n_docs, const GzDrop& R, hipStream_t s)
{
    const unsigned nb = (unsigned)((X.nblk + PWPB - 1) / PWPB);
    hipLaunchKernelGGL(gz_dwide_kernel, dim3(nb < 1024u ? nb : 1024u), dim3(WAVE * PWPB), 0, s, T, X, n_docs, R);     // (grid-stride over the list)
}

void gz_launch_bpe_word_drop(const GzDeviceTables* T, const uint8_t* word, int64_t nbytes, uint32_t* arena, int32_t* out, int32_t cap, int32_t* n_out,
                             const GzDrop& R, uint32_t word_index, hipStream_t s)
{
    hipLaunchKernelGGL(gz_bpe_word_drop_kernel, dim3(1), dim3(WAVE), 0, s, T, word, nbytes, arena, out, cap, n_out, R, word_index);
}
