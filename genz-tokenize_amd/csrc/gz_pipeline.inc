// The multi-kernel form of the hot path (included by gz_kernels.hip, shares its device helpers).  One launch of the
// pipeline = these kernels on one stream, per text (A, and B in pair mode); gz_launch_pipeline_text at the end of the file:
//
//   gz_brk_kernel        document starts -> 1 bit per byte                                   (N threads)
//   gz_classify_kernel   K1: coalesced 16-B loads, SWAR byte classes, the Unicode "\S+\n?" split as two bitmaps
//                        (word starts / word ends, 1 bit per byte each) + word count per 4-KiB block
//   gz_scan32[m]_kernel  exclusive scan of the block counts -> global index of every block's first word
//   gz_docw0_kernel      index of each document's first word (rank query on the start bitmap)
//   gz_words2_kernel     K2 (gz_hot.inc): one lane per word, whole-word table probe (perfect hash: one line per probe)
//                        -> wtok[word] = id; everything else is a "miss": a pending record on the block's compact list
//   gz_scan32[m]_kernel  exclusive scan of the per-block miss counts (+ which block holds miss 64 g)
//   gz_mpre_kernel       K2b (gz_hot.inc): one lane per miss: long-key whole-word table, symbol count, the misses of every
//                        3 072 sorted by symbol count, their places in the compact token area
//   gz_miss2_kernel      K2b (gz_hot.inc): bpe() (tokenize.py:62-101), one lane per word, 64 words of one length per wave
//   gz_miss_wide_kernel, gz_long_kernel   words of 17..64 symbols (32 / 64 lanes per word) and longer ones (wave-cooperative,
//                        chunked), on a side stream beside gz_miss2_kernel
//   gz_rows1_kernel      K3: rounds of documents; word records by LDS-DMA, positions, rows composed in LDS and written once
//                        with 16-byte stores: bos/eos framing, truncation, padding, attention mask (tokenize.py:126-152)
//   gz_rowsr_kernel      K3 without padding (max_len None, padding False), single texts: the same walk twice -- the rows' lengths, then
//                        (after gz_rowlen / the 64-bit scan) the rows written once at their places
//   (gz_rows_kernel / gz_assemble_kernel: pair mode, the other ragged layouts, max_len not a multiple of 4)
//   gz_compact_kernel / gz_expand_kernel   dense rows <-> an exchange block's entries (multi-GPU runs, the CSR host path)
//
// merge_rows / merge_passes (lane per symbol) serve gz_small_kernel and the wide-word kernel; every kernel probes the same
// perfectly hashed tables (gz_common.h).

namespace {

#if defined(GZ_DIAG) || defined(GZ_ABLATE)
constexpr bool GZ_DIAG_ON = true;             // timing switches (`ablate`, `rows_dbg`: results are WRONG when set) exist in diagnostic builds only
#else
constexpr bool GZ_DIAG_ON = false;
#endif
constexpr int PBLK = 4096;                    // bytes per scan block (4 tiles)
#ifndef GZ_PWPB
#define GZ_PWPB 4
#endif
constexpr int PWPB = GZ_PWPB;                 // waves per workgroup in the pipeline kernels
constexpr uint32_t W_MISS = 0x80000000u;      // wtok: [miss:1][pending:1][long:1][id | token count | glue<<15 | bytes]
constexpr uint32_t W_PEND = 0x40000000u;      // miss not merged yet: low 15 bits = bytes (0x7FFF: more), bit 15 = glued '\n'
constexpr uint32_t W_LONG = 0x20000000u;      // pending miss of more than 16 symbols: gz_miss_wide_kernel (32 / 64 lanes per word)
constexpr uint32_t W_HUGE = 0x10000000u;      // ... of more than 64 symbols: gz_long_kernel (wave-cooperative, chunked)
// A merged word's FINAL record (pending clear) has two forms:
//   far   W_MISS | token count (28 bits); the tokens are at mtok[waux[word]]
//   near  W_MISS | W_NEAR | (count - 1) << 25 | place: <= 16 tokens at mtok[B + 32 + place], place < X.near_lim <= 2^25 -- the
//         one-lane-per-word merge kernel's words (its compact token area starts at B + 32).  Everything a consumer needs is in
//         the record: no second, scattered load (waux) per merged word.
constexpr uint32_t W_NEAR = 0x20000000u;
constexpr uint32_t W_NEAR_MAX = 1u << 25;
__device__ __forceinline__ const int32_t* miss_pieces(const GzTextBufs& X, uint32_t rec, uint32_t w)
{
#ifdef GZ_DIAG
    // (diagnostic build: the record is final -- a pending one here means a merge kernel has not run or not finished -- and
    // its pieces lie inside the token array; else the word reads as ONE token from the start of the array)
    const uint64_t place = (rec & W_NEAR) ? (uint64_t)X.B + 32u + (rec & (W_NEAR_MAX - 1u)) : (uint64_t)X.waux[w];
    const uint64_t cnt = (rec & W_NEAR) ? ((rec >> 25) & 15u) + 1u : (rec & 0x0FFFFFFFu);
    if (!(GZ_CHK(501, (rec & W_PEND) ? 1 : 0, 1) && GZ_CHK(502, place + cnt, 2 * (X.B + 32) + 1))) return X.mtok;
#endif
    return X.mtok + ((rec & W_NEAR) ? (uint32_t)X.B + 32u + (rec & (W_NEAR_MAX - 1u)) : X.waux[w]);
}
__device__ __forceinline__ int miss_count(uint32_t rec)
{
#ifdef GZ_DIAG
    if (!GZ_CHK(503, (rec & W_PEND) ? 1 : 0, 1)) return 1;
#endif
    return (rec & W_NEAR) ? (int)((rec >> 25) & 15u) + 1 : (int)(rec & 0x0FFFFFFFu);
}
constexpr int PLONG = 256;                    // symbols the LDS long-word scratch holds

__device__ __forceinline__ bool is_ws1(uint32_t b) { return b == 0x20u || (b >= 0x09u && b <= 0x0Du) || (b >= 0x1Cu && b <= 0x1Fu); }
__device__ __forceinline__ bool is_ws2(uint32_t b, uint32_t n1) { return b == 0xC2u && (n1 == 0x85u || n1 == 0xA0u); }
__device__ __forceinline__ bool is_ws3(uint32_t b, uint32_t n1, uint32_t n2)
{
    return (b == 0xE2u && ((n1 == 0x80u && ((n2 >= 0x80u && n2 <= 0x8Au) || n2 == 0xA8u || n2 == 0xA9u || n2 == 0xAFu)) ||
                           (n1 == 0x81u && n2 == 0x9Fu))) ||
           (b == 0xE1u && n1 == 0x9Au && n2 == 0x80u) || (b == 0xE3u && n1 == 0x80u && n2 == 0x80u);
}

// 16 bytes at tb[p .. p+16) with bytes at or past B read as spaces.  Near the end of the text the load is moved back
// to B-16 and the bytes are shifted into place, so nothing at or past B is ever touched and there is no byte loop
// (a text of fewer than 16 bytes is staged behind 16 bytes of lead-in by gz_api.cpp, so tb + B - 16 is always readable).
__device__ __forceinline__ void load16(const uint8_t* tb, int64_t p, int64_t B, uint32_t r[4])
{
    typedef unsigned __attribute__((ext_vector_type(4), aligned(1))) v4u_u;
    constexpr uint64_t SP = 0x2020202020202020ull;
    const int64_t nv = B - p;
    if (nv >= 16) {
        const auto v = __builtin_nontemporal_load(reinterpret_cast<const v4u_u*>(tb + p));
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else if (nv > 0) {
        const auto v = __builtin_nontemporal_load(reinterpret_cast<const v4u_u*>(tb + B - 16));
        const uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
        const int s = 16 - (int)nv;                             // 1..15 bytes to drop from the front
        uint64_t rlo, rhi;
        if (s < 8) { const int sh = 8 * s; rlo = (lo >> sh) | (hi << (64 - sh)); rhi = (hi >> sh) | (SP << (64 - sh)); }
        else { const int sh = 8 * (s - 8); rlo = sh ? (hi >> sh) | (SP << (64 - sh)) : hi; rhi = SP; }
        r[0] = (uint32_t)rlo; r[1] = (uint32_t)(rlo >> 32); r[2] = (uint32_t)rhi; r[3] = (uint32_t)(rhi >> 32);
    } else r[0] = r[1] = r[2] = r[3] = 0x20202020u;
}

__device__ __forceinline__ uint32_t load4_tail(const uint8_t* tb, int64_t p, int64_t B)
{
    typedef unsigned __attribute__((aligned(1))) u32_u;
    const int64_t nv = B - p;
    if (nv >= 4) return *reinterpret_cast<const u32_u*>(tb + p);
    if (nv <= 0) return 0x20202020u;
    const int s = 4 - (int)nv;                                  // 1..3
    return (*reinterpret_cast<const u32_u*>(tb + B - 4) >> (8 * s)) | (0x20202020u << (32 - 8 * s));
}

// classify() for a stream of consecutive tiles: the whitespace state enters lane 0 through prevbit/carry and
// leaves through them (taken from lane 63).
__device__ __forceinline__ void classify_stream(const uint32_t w[4], uint32_t w4, int lane, uint32_t& prevbit_io,
                                                uint32_t& carry_io, uint32_t brk16, uint32_t& start16, uint32_t& end16)
{
    uint32_t leadm[4], wsm[4];
    uint32_t rare = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t x = w[i], nx = i < 3 ? w[i + 1] : w4;
        const uint32_t y = (x >> 8) | (nx << 24);
        const uint32_t hi = x & 0x80808080u, x7o = x | 0x80808080u;
        leadm[i] = ~(x & ~(x << 1)) & 0x80808080u;
        wsm[i] = ((swar_ge7(x7o, 0x09u) & ~swar_ge7(x7o, 0x0Eu)) | (swar_ge7(x7o, 0x1Cu) & ~swar_ge7(x7o, 0x21u))) & ~hi;
        // Multi-byte whitespace is rare; its lead bytes are C2, E2, E3, or E1 followed by 9A.  (E1 alone is everywhere
        // in Vietnamese text.)  Only a wave that sees a CANDIDATE does the full test below; the filter is deliberately
        // coarse (false positives only cost the slow path): a byte >= E2, a byte C2, or a byte 9A among this dword's
        // bytes 1..3 and the next dword's first (a 9A in byte 0 belongs to the dword, lane or tile before).
        {
            const uint32_t tc = x ^ 0xC2C2C2C2u, t9 = y ^ 0x9A9A9A9Au;                            // "has a zero byte" (no false negatives)
            rare |= (hi & swar_ge7(x7o, 0x62u)) | ((tc - 0x01010101u) & ~tc & 0x80808080u) | ((t9 - 0x01010101u) & ~t9 & 0x80808080u);
        }
    }
    const uint32_t lead = swar_bits(leadm[0], leadm[1], leadm[2], leadm[3]);
    uint32_t ws = swar_bits(wsm[0], wsm[1], wsm[2], wsm[3]);
    uint32_t ws23 = 0, ws3 = 0;
    if (wballot(rare != 0)) {
        uint32_t ws23m[4], c3m[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = w[i], nx = i < 3 ? w[i + 1] : w4;
            const uint32_t y = (x >> 8) | (nx << 24);
            const uint32_t hi = x & 0x80808080u, x7o = x | 0x80808080u;
            const uint32_t a2 = swar_eq(x, 0xC2u) & (swar_eq(y, 0x85u) | swar_eq(y, 0xA0u));
            const uint32_t eE = swar_ge7(x7o, 0x61u) & ~swar_ge7(x7o, 0x64u) & hi;
            const uint32_t b0 = (x << 7) & 0x80808080u, b1 = (x << 6) & 0x80808080u;
            const uint32_t y80 = swar_eq(y, 0x80u);
            c3m[i] = eE & ((b0 & ~b1 & swar_eq(y, 0x9Au)) | (~b0 & b1 & (y80 | swar_eq(y, 0x81u))) | (b0 & b1 & y80));
            ws23m[i] = a2;
        }
        ws23 = swar_bits(ws23m[0], ws23m[1], ws23m[2], ws23m[3]);
        ws |= ws23;
        uint32_t c = swar_bits(c3m[0], c3m[1], c3m[2], c3m[3]);
        for (; c; c &= c - 1) {
            const int j = __ffs(c) - 1;
            auto byte = [&](int k) -> uint32_t {
                const uint32_t ww = k < 4 ? w[0] : k < 8 ? w[1] : k < 12 ? w[2] : k < 16 ? w[3] : w4;
                return (ww >> ((k & 3) * 8)) & 0xFFu;
            };
            ws3 |= (uint32_t)is_ws3(byte(j), byte(j + 1), byte(j + 2)) << j;
        }
        ws |= ws3;
        ws23 |= ws3;
    }
    const uint32_t full = ws | (ws23 << 1) | (ws3 << 2);
    uint32_t carry = (uint32_t)__shfl_up((int)(full >> 16), 1, WAVE);
    uint32_t prevbit = (uint32_t)__shfl_up((int)((full >> 15) & 1u), 1, WAVE);
    if (lane == 0) { carry = carry_io; prevbit = prevbit_io; }
    const uint32_t fullc = (full | carry) & 0xFFFFu;
    const uint32_t prev_ws = ((fullc << 1) | prevbit) & 0xFFFFu;
    start16 = lead & ~ws & (prev_ws | brk16) & 0xFFFFu;
    end16 = (ws | brk16) & ~prev_ws & 0xFFFFu;
    carry_io = (uint32_t)__shfl((int)(full >> 16), WAVE - 1, WAVE);
    prevbit_io = (uint32_t)__shfl((int)((fullc >> 15) & 1u), WAVE - 1, WAVE);
}

}  // namespace

// -----------------------------------------------------------------------------------------------------------------
__global__ void gz_brk_kernel(const int64_t* off, int64_t n_docs, uint32_t* brk32)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (d >= n_docs) return;
    const int64_t p = off[d] - off[0];
    if (p > 0) atomicOr(&brk32[p >> 5], 1u << (p & 31));
}

// -----------------------------------------------------------------------------------------------------------------
// Two forms per tile, chosen by the wave (both exact for structurally valid UTF-8):
//   fast     the tile holds no control character other than the space, no byte that could lead a multi-byte whitespace
//            character (C2, E2 and above; 9A, the second byte of U+1680, also as the first byte BEHIND a tile that ends in E1)
//            and nothing carried in from the tile before: then the whitespace of the tile is exactly its bytes below 0x21, a
//            word starts at every other byte that follows one (or a document start) -- a third of the instructions of the
//            general form, and what running text takes nearly always;
//   general  classify_stream(): every Unicode whitespace code point, "\n" and friends included.
__global__ __launch_bounds__(WAVE * PWPB) void gz_classify_kernel(GzTextBufs X)
{
    typedef unsigned __attribute__((ext_vector_type(4), aligned(1))) v4u_u;
    constexpr uint32_t H = 0x80808080u;
    const int lane = lane_id();
    const int64_t blk = (int64_t)blockIdx.x * PWPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));     // (scalar)
    if (blk >= X.nblk) return;
    const uint8_t* tb = X.tb;
    const int64_t B = X.B, p0 = blk * PBLK;
    // whitespace state entering the block: look back up to 3 bytes
    uint32_t prevbit = 1, carry = 0;
    if (p0 > 0) {
        auto at = [&](int64_t i) -> uint32_t { return (i >= 0 && i < B) ? tb[i] : 0x20u; };
        const uint32_t b1 = at(p0 - 1), b2 = at(p0 - 2), b3 = at(p0 - 3), c0 = at(p0), c1 = at(p0 + 1);
        const bool l1_2 = is_ws2(b1, c0), l1_3 = is_ws3(b1, c0, c1), l2_3 = is_ws3(b2, b1, c0);
        prevbit = (is_ws1(b1) || l1_2 || l1_3 || is_ws2(b2, b1) || l2_3 || is_ws3(b3, b2, b1)) ? 1u : 0u;
        carry = ((l1_2 || l1_3 || l2_3) ? 1u : 0u) | (l1_3 ? 2u : 0u);
    }
    int count = 0;
    // one tile: its 16 bytes per lane (w) and its document-start bits (brk16) -> start / end bits, the running word count
    // (nx0: the first byte behind the tile, wave-uniform; a space behind the text)
    auto tile = [&](int t, const uint32_t (&w)[4], uint32_t brk16, uint32_t nx0) {
        const int64_t pos = p0 + (int64_t)t * TILE;
        // bytes below 0x21 (ASCII), and what would send the tile to the general form
        uint32_t lt[4], odd = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = w[i], x7o = x | H;
            lt[i] = ~(x7o - 0x21212121u) & ~x & H;                               // low 7 bits < 0x21, bit 7 clear
            const uint32_t tc = x ^ 0xC2C2C2C2u, t9 = x ^ 0x9A9A9A9Au;            // "has a zero byte" tests (no false negatives)
            odd |= (lt[i] & ~(x << 2))                                            // a control character (below 0x20: bit 5 clear)
                 | (x & (x7o - 0x62626262u) & H)                                  // a byte >= 0xE2
                 | ((tc - 0x01010101u) & ~tc & H) | ((t9 - 0x01010101u) & ~t9 & H);
        }
        // E1 in the tile's last byte with 9A behind it (U+1680 = E1 9A 80 cut 1|2 by the tile edge): the 9A is the next tile's, so
        // nothing above sees it -- and the general form must run HERE, for the end bit at the E1 and the carry into the next tile
        if (lane == WAVE - 1 && (w[3] >> 24) == 0xE1u && nx0 == 0x9Au) odd |= H;
        uint32_t st16, en16;
        uint32_t has_nl = 0;                               // (wave-uniform) the tile may hold a line feed: only the general form can see one
        if (carry == 0 && wballot(odd != 0) == 0) {
            const uint32_t ws = swar_bits(lt[0], lt[1], lt[2], lt[3]);
            uint32_t pb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(ws >> 15), 0x138, 0xF, 0xF, false);    // wave_shr:1: bit 15 of the lane before
            if (lane == 0) pb = prevbit;
            const uint32_t prev_ws = ((ws << 1) | pb) & 0xFFFFu;
            st16 = ~ws & (prev_ws | brk16) & 0xFFFFu;
            en16 = (ws | brk16) & ~prev_ws & 0xFFFFu;
            prevbit = (uint32_t)__builtin_amdgcn_readlane((int)(ws >> 15), WAVE - 1);
        } else {
            uint32_t w4 = (uint32_t)__shfl_down((int)w[0], 1, WAVE);
            if (lane == WAVE - 1) w4 = load4_tail(tb, pos + TILE, B);
            classify_stream(w, w4, lane, prevbit, carry, brk16, st16, en16);
            has_nl = 0x8000u;
        }
        X.st[(pos >> 4) + lane] = (uint16_t)st16;
        X.en[(pos >> 4) + lane] = (uint16_t)en16;
        // word starts of the block before this tile (gz_docw0_kernel) | "may hold a line feed" << 15 (the word kernel's glue test)
        if (lane == 0) X.tilecnt[4 * blk + t] = (uint16_t)((uint32_t)count | has_nl);
        int tot;
        (void)wave_excl_sum(__popc(st16), lane, tot);
        count += tot;
    };
    if (p0 + PBLK + 16 <= B) {
        // a block inside the text (all but the last one or two): its four tiles are requested at once -- a wave that asks for one
        // kilobyte, waits, and asks for the next keeps too few bytes in flight to fill the memory pipe
        uint32_t w[PBLK / TILE][4], brk16[PBLK / TILE];
#pragma unroll
        for (int t = 0; t < PBLK / TILE; ++t) {
            const auto v = __builtin_nontemporal_load(reinterpret_cast<const v4u_u*>(tb + p0 + t * TILE + 16 * lane));
            w[t][0] = v.x; w[t][1] = v.y; w[t][2] = v.z; w[t][3] = v.w;
            brk16[t] = X.brk[((p0 + t * TILE) >> 4) + lane];
        }
        const uint32_t nxb = tb[p0 + PBLK];                   // (inside the text: p0 + PBLK + 16 <= B)
#pragma unroll
        for (int t = 0; t < PBLK / TILE; ++t)
            tile(t, w[t], brk16[t], t + 1 < PBLK / TILE ? (uint32_t)__builtin_amdgcn_readfirstlane((int)w[t + 1 < PBLK / TILE ? t + 1 : t][0]) & 0xFFu : nxb);
    } else {
        for (int t = 0; t < PBLK / TILE; ++t) {
            const int64_t pos = p0 + (int64_t)t * TILE;
            if (pos > B) break;                               // position B itself can still hold a word end
            uint32_t w[4];
            load16(tb, pos + 16 * lane, B, w);
            tile(t, w, X.brk[(pos >> 4) + lane], pos + TILE < B ? (uint32_t)tb[pos + TILE] : 0x20u);
        }
    }
    if (lane == 0) X.blkcnt[blk] = (uint32_t)count;
}

namespace {
// one 8-byte word of a chained scan: {status:2, call number:30, value:32}
constexpr uint64_t LB_AGG = 1ull << 62, LB_PREFIX = 2ull << 62;
__device__ __forceinline__ unsigned long long lb_pack(uint64_t status, uint32_t epoch, uint32_t value)
{
    return status | ((uint64_t)(epoch & 0x3FFFFFFFu) << 32) | value;
}
}  // namespace

// single-workgroup exclusive scan, in place; v[n] receives the total.  4 elements (one 16-byte load) per thread and
// trip, ONE barrier per trip: the wave sums go through a double-buffered LDS array and every thread keeps the running
// carry itself.  (16 elements per thread was measured slower: the per-thread runs stop being coalesced.)
// With `grp` != nullptr the scanned values are the blocks' miss counts and the kernel also writes, for every group of
// 64 consecutive misses (global miss index 64 g ...), the block that holds the group's first miss: grp[g].
__global__ __launch_bounds__(1024) void gz_scan32_kernel(uint32_t* v, int64_t n, uint32_t* grp)
{
    auto groups = [&](int64_t b, uint32_t e, uint32_t cnt) {
        for (uint32_t g = (e + 63u) >> 6; (uint64_t)g << 6 < (uint64_t)e + cnt; ++g) grp[g] = (uint32_t)b;
    };
    typedef unsigned __attribute__((ext_vector_type(4))) v4u;
    __shared__ uint32_t wsum[2][16];
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    uint32_t carry = 0;
    int buf = 0;
    for (int64_t base = 0; base < n; base += 4096, buf ^= 1) {
        const int64_t i = base + 4 * (int64_t)threadIdx.x;
        v4u a = {0u, 0u, 0u, 0u};
        if (i + 3 < n) a = *reinterpret_cast<const v4u*>(v + i);              // (the array is 16-byte aligned)
        else { if (i < n) a.x = v[i]; if (i + 1 < n) a.y = v[i + 1]; if (i + 2 < n) a.z = v[i + 2]; }
        const uint32_t mine = a.x + a.y + a.z + a.w;
        int tot;
        const uint32_t excl = (uint32_t)wave_excl_sum((int)mine, lane, tot);
        if (lane == WAVE - 1) wsum[buf][wv] = (uint32_t)tot;
        __syncthreads();
        uint32_t pre = carry, all = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { const uint32_t w = wsum[buf][k]; if (k < wv) pre += w; all += w; }
        carry += all;
        const uint32_t e0 = pre + excl;
        if (i + 3 < n) { v4u o = {e0, e0 + a.x, e0 + a.x + a.y, e0 + a.x + a.y + a.z}; *reinterpret_cast<v4u*>(v + i) = o; }
        else { if (i < n) v[i] = e0; if (i + 1 < n) v[i + 1] = e0 + a.x; if (i + 2 < n) v[i + 2] = e0 + a.x + a.y; }
        if (grp) {                                                   // (elements at or past n were loaded as zero)
            groups(i, e0, a.x); groups(i + 1, e0 + a.x, a.y); groups(i + 2, e0 + a.x + a.y, a.z);
            groups(i + 3, e0 + a.x + a.y + a.z, a.w);
        }
    }
    if (threadIdx.x == 0) v[n] = carry;
}

// The same scan over many workgroups (large batches: 70 000 block counts per 287 MB of text took the single workgroup
// above 17 dependent trips, 21 us): a chained scan with decoupled look-back.  A workgroup takes a
// TICKET (atomic counter, zeroed with X.ctl) = the 1 024-element chunk it scans, so a chunk only ever waits for chunks
// that are already running; it publishes ONE 8-byte word {status, call number, value} with agent-scope relaxed atomics --
// first its own sum, then the running total up to and including itself -- and a successor adds up sums backwards until it
// meets a running total (64 predecessors per wave-wide read).  `epoch` makes words of earlier scans invalid: the array is
// never cleared and is shared by the scans of a call.  Spins are bounded (time-out -> *err_flag).
constexpr int SCH = 1024;                     // elements per workgroup of gz_scan32m_kernel (256 threads x 4)
#ifdef GZ_DIAG
__device__ int gz_diag_spin_limit = 1 << 21;  // diagnostic builds: gz_diag_set(1, n) -- n < 0 forces the time-out (tests/test_gpu_parity.py)
#define GZ_SPIN_LIMIT gz_diag_spin_limit
#else
#define GZ_SPIN_LIMIT (1 << 21)
#endif
__global__ __launch_bounds__(256) void gz_scan32m_kernel(uint32_t* v, int64_t n, uint32_t* grp, unsigned long long* lb, uint32_t* ticket_ctr,
                                                         uint32_t epoch, int32_t* err_flag)
{
    auto groups = [&](int64_t b, uint32_t e, uint32_t cnt) {
        for (uint32_t g = (e + 63u) >> 6; (uint64_t)g << 6 < (uint64_t)e + cnt; ++g) grp[g] = (uint32_t)b;
    };
    typedef unsigned __attribute__((ext_vector_type(4))) v4u;
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t sh_ticket, sh_base;
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    if (threadIdx.x == 0) sh_ticket = atomicAdd(ticket_ctr, 1u);
    __syncthreads();
    const uint32_t ticket = sh_ticket;
    const int64_t i = (int64_t)ticket * SCH + 4 * (int64_t)threadIdx.x;
    v4u a = {0u, 0u, 0u, 0u};
    if (i + 3 < n) a = *reinterpret_cast<const v4u*>(v + i);                  // (the array is 16-byte aligned)
    else { if (i < n) a.x = v[i]; if (i + 1 < n) a.y = v[i + 1]; if (i + 2 < n) a.z = v[i + 2]; }
    const uint32_t mine = a.x + a.y + a.z + a.w;
    int tot;
    const uint32_t excl = (uint32_t)wave_excl_sum((int)mine, lane, tot);
    if (lane == WAVE - 1) wsum[wv] = (uint32_t)tot;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t w = wsum[k]; if (k < wv) pre += w; all += w; }
    if (wv == 0) {
        if (lane == 0)
            __hip_atomic_store(&lb[ticket], lb_pack(ticket == 0 ? LB_PREFIX : LB_AGG, epoch, all), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t running = 0;
        bool ok = GZ_SPIN_LIMIT >= 0;
        int64_t j = (int64_t)ticket - 1;                         // nearest predecessor not summed yet
        int spins = 0;
        while (j >= 0) {
            const int64_t idx = j - lane;
            unsigned long long w = 0;
            if (idx >= 0) w = __hip_atomic_load(&lb[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool cur = idx >= 0 && (uint32_t)((w >> 32) & 0x3FFFFFFFu) == (epoch & 0x3FFFFFFFu);
            const uint32_t status = cur ? (uint32_t)(w >> 62) : 0u;
            const uint64_t inw = wballot(idx >= 0);
            const uint64_t valid = wballot(status != 0u);
            const uint64_t pref = wballot(status == 2u);
            // lanes 0 .. stop are needed: up to the nearest running total, or the whole window
            const int stop = pref ? __ffsll((unsigned long long)pref) - 1 : (int)__popcll(inw) - 1;
            const uint64_t need = stop >= 63 ? ~0ull : ((2ull << stop) - 1ull);
            if ((valid & need) != need) {                         // somebody has not published yet: look again
                if (++spins > GZ_SPIN_LIMIT) { ok = false; break; }
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            running += (uint32_t)wave_sum((int)(lane <= stop ? (uint32_t)w : 0u));
            if (pref) break;
            j -= WAVE;
        }
        if (lane == 0) {
            if (!ok) *err_flag = 1;
            if (ticket != 0) __hip_atomic_store(&lb[ticket], lb_pack(LB_PREFIX, epoch, running + all), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sh_base = running;
        }
    }
    __syncthreads();
    const uint32_t e0 = sh_base + pre + excl;
    if (i + 3 < n) { v4u o = {e0, e0 + a.x, e0 + a.x + a.y, e0 + a.x + a.y + a.z}; *reinterpret_cast<v4u*>(v + i) = o; }
    else { if (i < n) v[i] = e0; if (i + 1 < n) v[i + 1] = e0 + a.x; if (i + 2 < n) v[i + 2] = e0 + a.x + a.y; }
    if (grp) {                                                       // (elements at or past n were loaded as zero)
        groups(i, e0, a.x); groups(i + 1, e0 + a.x, a.y); groups(i + 2, e0 + a.x + a.y, a.z);
        groups(i + 3, e0 + a.x + a.y + a.z, a.w);
    }
    if (i <= n && n < i + 4) v[n] = e0 + (n > i ? a.x : 0u) + (n > i + 1 ? a.y : 0u) + (n > i + 2 ? a.z : 0u);     // the total
}

// index of the first word of every document (and docw0[N] = number of words at or after the last document start):
// scanned block base + the block's starts before the document's tile + a popcount over at most 1 KiB of the bitmap
__global__ void gz_docw0_kernel(GzTextBufs X, int64_t n_docs)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_docs) return;
    const int64_t p = X.off[d] - X.off[0];
    const int64_t blk = p >> 12;
    uint32_t w = X.blkcnt[blk < X.nblk ? blk : X.nblk];      // scanned: base of the block (or the total)
    if (blk < X.nblk) {
        const int64_t tile = p >> 10;
        w += X.tilecnt[tile] & 0x7FFFu;                        // tile == 4 * blk + (tile within the block); bit 15: a flag of the word kernel
        const uint64_t* st64 = reinterpret_cast<const uint64_t*>(X.st);
        const int64_t u0 = tile * (TILE / 64), u1 = p >> 6;    // whole 64-bit words in [u0, u1), then p & 63 bits
        uint32_t acc = 0;
#pragma unroll 8
        for (int j = 0; j < TILE / 64; ++j) {
            const int64_t u = u0 + j;
            const uint64_t bits = st64[u];
            acc += u < u1 ? __popcll(bits) : (u == u1 ? __popcll(bits & ((1ull << (p & 63)) - 1ull)) : 0);
        }
        w += acc;
    }
    (void)GZ_CHK(601, w, X.wmax + 1);
    X.docw0[d] = w;
}

// -----------------------------------------------------------------------------------------------------------------
// K2 helpers (the kernel itself, gz_words2_kernel, is in gz_hot.inc)
// -----------------------------------------------------------------------------------------------------------------
namespace {

struct alignas(16) WordsLds {
    uint32_t endmap[2 * TILE / 32];           // (first: the word kernel's reads of all three arrays then reach them through the instructions' offset fields)
    uint32_t bytes[(TILE + 48) / 4];          // tile + 48 bytes of look-ahead (a 32-byte word may start at the last byte)
    uint16_t wstart[MAXWORDS + 3];
};

// first word end strictly after tile bit `from` (tile-relative); searches LDS for two tiles, then the global bitmap
// (tile-relative: the end of a word that starts in the tile is less than 4 GiB away, positions stay in 32 bits)
__device__ __forceinline__ uint32_t find_end(const WordsLds& L, const GzTextBufs& X, int64_t pos, int from)
{
    // 64 bits of the end bitmap at once: a word shorter than 32 bytes (nearly all) never enters the loop below
    int q = (from + 1) >> 5;                                   // <= TILE / 32, so q + 1 stays inside the two-tile map
    const uint64_t two = ((uint64_t)L.endmap[q + 1] << 32) | L.endmap[q];
    const uint64_t first = two & (~0ull << ((from + 1) & 31));
    if (first) return (uint32_t)(32 * q + __ffsll((unsigned long long)first) - 1);
    uint32_t bits = 0;
    q += 1;
    while (bits == 0 && q < 2 * TILE / 32 - 1) bits = L.endmap[++q];
    if (bits) return (uint32_t)(32 * q + __ffs(bits) - 1);
    const uint32_t* en32 = reinterpret_cast<const uint32_t*>(X.en);
    int64_t u = (pos + 2 * TILE) >> 5;
    const int64_t ulast = X.B >> 5;                           // position B always terminates a word
    for (; u <= ulast; ++u) {
        const uint32_t b = en32[u];
        if (b) return (uint32_t)(32 * u + __ffs(b) - 1 - pos);
    }
    return (uint32_t)(X.B - pos);
}

// is position p (absolute in the text) where a running word ends: whitespace starts here, a document starts here, or
// the text ends (the byte patterns of classify_stream; structurally valid UTF-8)
__device__ __forceinline__ bool word_ends_at(const GzTextBufs& X, int64_t p)
{
    if (p >= X.B) return true;
    if ((X.brk[p >> 4] >> (p & 15)) & 1u) return true;
    const uint32_t f = load4_tail(X.tb, p, X.B);
    const uint32_t b0 = f & 0xFFu, b1 = (f >> 8) & 0xFFu, b2 = (f >> 16) & 0xFFu;
    return is_ws1(b0) || is_ws2(b0, b1) || is_ws3(b0, b1, b2);
}

// end of the word that is still running at position `from` (absolute), byte by byte: very long words only
__device__ __forceinline__ int64_t scan_word_end(const GzTextBufs& X, int64_t from)
{
    int64_t p = from;
    while (!word_ends_at(X, p)) ++p;
    return p;
}

}  // namespace

// -----------------------------------------------------------------------------------------------------------------
// Lane-per-SYMBOL merge passes (gz_small_kernel's misses; words of more than 16 symbols everywhere): a word takes 8, 16, 32
// or 64 lanes, every adjacent pair of the word probes the pair table in the same instruction, the minimum over the word's
// lanes picks the pair to merge (tokenize.py:70-73), every occurrence merges left to right (:75-92), the symbols are
// compacted through LDS.  (The big pipeline's words of <= 16 symbols take gz_miss2_kernel, one lane per WORD: gz_hot.inc.)
// -----------------------------------------------------------------------------------------------------------------
namespace {
struct MissLds {
    uint32_t sym[WAVE];                       // one merge pass: 64 symbols (8 x 8, 4 x 16, 2 x 32 or 1 x 64)
    uint32_t q[3][WAVE];                      // word indices waiting for 16 / 32 / 64 lanes per word
};

// minimum over the LW lanes of a word (LW = 16: one DPP row)
template <int LW>
__device__ __forceinline__ uint32_t seg_min(uint32_t v)
{
    v = row16_min(v);
    if (LW >= 32) { const uint32_t t = (uint32_t)__shfl_xor((int)v, 16, WAVE); v = t < v ? t : v; }
    if (LW >= 64) { const uint32_t t = (uint32_t)__shfl_xor((int)v, 32, WAVE); v = t < v ? t : v; }
    return v;
}

// Merge passes over L.q[QI][0..nq): LW lanes per word, 64/LW words per pass.  Words with more than LW symbols are
// appended to `over` (next size up) or, from the 64-lane passes, handed to gz_long_kernel.
// (W16: X.waux holds 16-bit word starts -- gz_small_kernel's LDS word list)
template <int LW, int QI, bool W16 = false>
__device__ __forceinline__ int merge_passes(const GzDeviceTables& T, MissLds& L, const GzTextBufs& X, int nq, int lane,
                                            int64_t blk, int32_t* long_flag, const uint16_t* ldisp = nullptr)
{
    constexpr int WP = WAVE / LW;                              // words per pass
    constexpr uint64_t SEGMASK = LW == 64 ? ~0ull : ((1ull << LW) - 1ull);
    int nover = 0;
    for (int c0 = 0; c0 < nq; c0 += WP) {
        const int seg = lane / LW, k = lane % LW;
        const int m = c0 + seg;
        const bool mv = m < nq;
        uint32_t widx = mv ? L.q[QI][m] : 0u;
        if (!W16 && mv && !GZ_CHK(401, widx, X.wmax)) widx = 0u;
        uint32_t rec = mv ? X.wtok[widx] : 0u;
        uint32_t start = mv ? (W16 ? (uint32_t)reinterpret_cast<const uint16_t*>(X.waux)[widx] : X.waux[widx]) : 0u;
        if (!W16 && mv && !(GZ_CHK(402, (rec & (W_MISS | W_PEND | W_LONG)) == (W_MISS | W_PEND | W_LONG) ? 0 : 1, 1) && GZ_CHK(403, (uint64_t)start + (rec & 0x7FFFu), X.B + 1))) { rec = 0u; start = 0u; }
        const uint8_t* g = X.tb + start;
        const int nb = (int)(rec & 0x7FFFu);
        const bool glue = (rec & 0x8000u) != 0;
        uint32_t* S = L.sym + LW * seg;
        bool over = mv && nb > 4 * LW;                         // more than 4*LW bytes cannot be <= LW code points
        int ncp = 0;
        uint32_t leadbits[4], bytev[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int b = LW * p + k;
            const bool in = mv && !over && b < nb;
            bytev[p] = 0x80u;
            if (wballot(in)) {
                if (in) bytev[p] = g[b];
                const uint64_t bal = wballot(in && (bytev[p] & 0xC0u) != 0x80u);
                leadbits[p] = (uint32_t)((bal >> (LW * seg)) & SEGMASK);
                if (LW == 64) leadbits[p] = 0;                 // (64-lane form keeps its masks in 64 bits below)
                ncp += LW == 64 ? __popcll(bal) : __popc(leadbits[p]);
            } else leadbits[p] = 0;
        }
        int n = ncp + (glue ? 1 : 0);
        if (mv && n > LW) over = true;
        const bool rv = mv && !over;
        int before = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int b = LW * p + k;
            const bool lead = rv && b < nb && (bytev[p] & 0xC0u) != 0x80u;
            const uint64_t lb = wballot(lead);
            if (lb) {
                if (lead) {
                    auto at = [&](int64_t i) -> uint32_t { return g[i]; };
                    int len;
                    const uint32_t cp = decode_cp(at, b, nb, len);
                    const int idx = before + __popcll((lb >> (LW * seg)) & SEGMASK & lt_mask(k));
                    S[idx] = initial_symbol(T, cp, !glue && idx == ncp - 1);
                }
                before += __popcll((lb >> (LW * seg)) & SEGMASK);
            }
        }
        if (rv && glue && k == 0) S[n - 1] = initial_symbol(T, 0x0Au, true);
        for (;;) {
            const bool vp = rv && k + 1 < n;
            const uint32_t s = (rv && k < n) ? S[k] : GZ_NO_SYMBOL;
            const uint32_t s1 = vp ? S[k + 1] : GZ_NO_SYMBOL;
            uint32_t merged = 0;
            const uint32_t rank = vp ? probe_pair(T, s, s1, merged, ldisp) : GZ_RANK_NONE;
            const uint32_t best = seg_min<LW>(rank);
            const uint64_t M = wballot(best != GZ_RANK_NONE && rank == best);
            if (M == 0) break;
            uint64_t pick = M;
            if (M & (M << 1)) {                                 // overlapping occurrences (first == second): greedy
                pick = 0;
                uint64_t rem = M;
                while (rem) {
                    const uint64_t low = rem & (0 - rem);
                    pick |= low;
                    rem &= ~(low | (low << 1));
                }
            }
            const bool picked = (pick >> lane) & 1ull;
            const bool consumed = lane > 0 && ((pick >> (lane - 1)) & 1ull);
            const bool keep = rv && k < n && !consumed;
            const uint64_t keepseg = (wballot(keep) >> (LW * seg)) & SEGMASK;
            if (keep) S[__popcll(keepseg & lt_mask(k))] = picked ? merged : s;
            n -= __popcll((pick >> (LW * seg)) & SEGMASK);
        }
        if (rv) {
            if (k < n) X.mtok[start + k] = token_id(T, S[k], k == n - 1);
            if (k == 0) X.wtok[widx] = W_MISS | (uint32_t)n;
        }
        // words that need more lanes
        const uint64_t ob = wballot(mv && over && k == 0);
        if (ob) {
            if (LW < 64) {
                if (mv && over && k == 0) L.q[QI + 1 < 3 ? QI + 1 : 2][nover + below(ob)] = widx;
                nover += __popcll(ob);
            } else {
                if (mv && over && k == 0) X.wtok[widx] = rec | W_HUGE;          // left to gz_long_kernel
                if (mv && over && k == 0) {
                    X.blklong[start >> 12] = 3; *long_flag = 1;
                    if (!W16) X.wlist[X.wmax + 6 - (int64_t)atomicAdd(X.ctl, 1u)] = widx;      // (its list: from the end of the array down)
                }
            }
        }
    }
    return nover;
}
// minimum over the LW (8 or 16) lanes of a word: quad swaps, half-row mirror, row mirror
template <int LW>
__device__ __forceinline__ uint32_t rows_min(uint32_t v)
{
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0xB1, 0xF, 0xF, false); v = t < v ? t : v;   // quad_perm [1,0,3,2]
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x4E, 0xF, 0xF, false); v = t < v ? t : v;   // quad_perm [2,3,0,1]
    t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x141, 0xF, 0xF, false); v = t < v ? t : v;  // row_half_mirror
    if (LW == 16) { t = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x140, 0xF, 0xF, false); v = t < v ? t : v; }  // row_mirror
    return v;
}

template <int LW>
__device__ __forceinline__ int merge_rows(const GzDeviceTables& T, MissLds& L, const GzTextBufs& X, int q0, int q1, int lane)
{
    typedef unsigned __attribute__((aligned(1))) u32_u;
    constexpr int WP = WAVE / LW;                               // words per pass
    constexpr int NP = LW == 8 ? 2 : 4;                         // byte rounds: LW bytes per word and round
    constexpr uint32_t RM = (1u << LW) - 1u;
    const int row = lane / LW, k = lane % LW, sh = LW * row;
    int nover = 0;
    for (int c0 = q0; c0 < q1; c0 += WP) {
        const int m = c0 + row;
        const bool mv = m < q1;
        const uint32_t widx = mv ? L.q[0][m] : 0u;
        const uint32_t rec = mv ? L.q[1][m] : 0u;
        const uint32_t start = mv ? L.q[2][m] : 0u;
        const int nb = (int)(rec & 0x7FFFu);
        const bool glue = (rec & 0x8000u) != 0;
        uint32_t* S = L.sym + LW * row;
        bool over = mv && nb > NP * LW;
        const int nb_ok = over ? 0 : nb;
        int ncp = 0;
        uint32_t leadbits[NP], four[NP];
        bool round_on[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            leadbits[p] = 0;
            four[p] = 0x80808080u;
            round_on[p] = p == 0 || wballot(nb_ok > LW * p) != 0;      // wave-uniform: most passes only have p == 0
            if (round_on[p]) {
                const int b = LW * p + k;
                if (b < nb_ok) {
                    // this byte and the three after it (continuation bytes of a code point that starts here); within 3
                    // bytes of the end of the text the load is moved back and shifted, so nothing past B is touched
                    // (texts of fewer than 16 bytes are staged with zeroed slack behind them, see gz_api.cpp)
                    const uint32_t a = start + (uint32_t)b, last = (uint32_t)X.B - 4u;
                    const uint32_t ac = a <= last ? a : last;
                    four[p] = *reinterpret_cast<const u32_u*>(X.tb + ac) >> (8u * (a - ac));
                }
                const uint64_t bal = wballot((four[p] & 0xC0u) != 0x80u);
                leadbits[p] = (uint32_t)(bal >> sh) & RM;
                ncp += __popc(leadbits[p]);
            }
        }
        int n = ncp + (glue ? 1 : 0);
        if (mv && n > LW) over = true;
        const bool rv = mv && !over;
        int before = 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (round_on[p]) {
                const int b = LW * p + k;
                const uint32_t f = four[p], b0 = f & 0xFFu;
                if (rv && (b0 & 0xC0u) != 0x80u) {
                    // structural UTF-8 decode, never past the end of the word
                    int want = b0 < 0x80u ? 1 : b0 < 0xE0u ? 2 : b0 < 0xF0u ? 3 : 4;
                    if (b + want > nb) want = nb - b;
                    uint32_t cp = b0;
                    if (b0 >= 0x80u) {
                        cp = want == 2 ? (b0 & 0x1Fu) : want == 3 ? (b0 & 0x0Fu) : want == 4 ? (b0 & 0x07u) : (b0 & 0x3Fu);
                        if (want > 1) cp = (cp << 6) | ((f >> 8) & 0x3Fu);
                        if (want > 2) cp = (cp << 6) | ((f >> 16) & 0x3Fu);
                        if (want > 3) cp = (cp << 6) | ((f >> 24) & 0x3Fu);
                    }
                    const int idx = before + __popc(leadbits[p] & ((1u << k) - 1u));
                    S[idx] = initial_symbol(T, cp, !glue && idx == ncp - 1);
                }
                before += __popc(leadbits[p]);
            }
        }
        if (rv && glue && k == 0) S[n - 1] = initial_symbol(T, 0x0Au, true);
        for (;;) {
            const bool inw = rv && k + 1 < n;
            const uint32_t sraw = S[k];                           // (unconditional LDS read: no exec juggling)
            const uint32_t s = (rv && k < n) ? sraw : GZ_NO_SYMBOL;
            const uint32_t s1 = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)s, 0x101, 0xF, 0xF, false);   // row_shl:1 = my right neighbour
            const bool vp = inw && !((s | s1) & 0xFFF00000u);     // code points outside every table never merge
            uint32_t merged = 0;
            const uint32_t rank = vp ? probe_pair(T, s, s1, merged) : GZ_RANK_NONE;
            const uint32_t best = rows_min<LW>(rank);
            const uint64_t M = wballot(rank == best) & ~wballot(rank == GZ_RANK_NONE);    // (two plain v_cmp ballots)
            if (M == 0) break;
            uint64_t pick = M;
            if (M & (M << 1)) {                                 // overlapping occurrences (first == second): greedy
                pick = 0;
                uint64_t rem = M;
                while (rem) {
                    const uint64_t low = rem & (0 - rem);
                    pick |= low;
                    rem &= ~(low | (low << 1));
                }
            }
            // the last lane of a row never holds a pair, so "my left neighbour merged" stays inside the row
            const uint32_t prow = (uint32_t)(pick >> sh) & RM;
            const bool picked = (prow >> k) & 1u;
            const bool consumed = ((prow << 1) >> k) & 1u;
            const bool keep = rv && k < n && !consumed;
            const uint32_t krow = (uint32_t)(wballot(keep) >> sh) & RM;
            if (keep) S[__popc(krow & ((1u << k) - 1u))] = picked ? merged : s;
            n -= __popc(prow);
        }
        if (rv) {
            if (k < n) X.mtok[start + k] = token_id(T, S[k], k == n - 1);
            if (k == 0) X.wtok[widx] = W_MISS | (uint32_t)n;
        }
        // words that need more lanes go on one global list for gz_miss_wide_kernel (one atomic per pass)
        const bool ov = mv && over && k == 0;
        const uint64_t ob = wballot(ov);
        if (ob) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(X.wlist, (uint32_t)__popcll(ob));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (ov) { X.wtok[widx] = rec | W_LONG; X.wlist[1 + base + below(ob)] = widx; }
            nover = 1;
        }
    }
    return nover;
}

}  // namespace

// K2b': misses of 17..64 symbols (rare): 32, then 64 lanes per word; the list gz_mpre_kernel made.  Every merge iteration is a
// dependent probe: the displacement array is staged in LDS (when it fits) so that a probe is ONE trip to memory -- the kernel
// runs beside gz_miss2_kernel and the row kernel waits for whichever of the two ends last
__global__ __launch_bounds__(WAVE * PWPB) __attribute__((amdgpu_waves_per_eu(8, 8))) void gz_miss_wide_kernel(const GzDeviceTables* __restrict__ Tp, GzTextBufs X, int32_t* long_flag, int lds_disp)
{
    __shared__ MissLds lds[PWPB];
    extern __shared__ __attribute__((aligned(16))) uint8_t wide_dyn[];           // the pair table's displacement array (lds_disp)
    const int lane = lane_id();
    const uint32_t n = X.wlist[0];                               // words of more than 16 symbols (gz_mpre_kernel's list)
    const uint32_t wave = blockIdx.x * PWPB + threadIdx.x / WAVE, nwaves = gridDim.x * PWPB;
    if (blockIdx.x * PWPB * 2u >= n) return;                     // (the whole workgroup: nothing to do)
    const GzDeviceTables T = *Tp;
    uint16_t* ldisp = nullptr;
    if (lds_disp) {
        ldisp = reinterpret_cast<uint16_t*>(wide_dyn);
        const uint4* src = reinterpret_cast<const uint4*>(T.pair_ph.disp);
        for (uint32_t i = threadIdx.x; i < T.pair_ph.nbuckets / 8u; i += blockDim.x) reinterpret_cast<uint4*>(ldisp)[i] = src[i];
        __syncthreads();
    }
    if (wave * 2u >= n) return;
    MissLds& L = lds[threadIdx.x / WAVE];
    for (uint32_t i = wave * 2u; i < n; i += nwaves * 2u) {      // two words (one 32-lane pass) per trip
        const int nq = (int)min(2u, n - i);
        if (lane < nq) L.q[1][lane] = X.wlist[1 + i + lane];
        const int n64 = merge_passes<32, 1>(T, L, X, nq, lane, 0, long_flag, ldisp);
        if (n64) merge_passes<64, 2>(T, L, X, n64, lane, 0, long_flag, ldisp);
    }
}

// K2c: words of more than 16 symbols (rare): one wave per word, lane per symbol, chunked ballots (wave_merge)
__global__ __launch_bounds__(WAVE * PWPB) void gz_long_kernel(const GzDeviceTables* __restrict__ Tp, GzTextBufs X, const int32_t* long_flag)
{
    __shared__ uint32_t lsym[PWPB][PLONG];
    if (*long_flag == 0) return;                                 // (nearly always: a small grid-stride grid keeps the empty launch short)
    const int lane = lane_id();
    const uint32_t n = X.ctl[0];                                 // words gz_miss_wide_kernel could not fit in 64 lanes
    for (uint32_t i = blockIdx.x * PWPB + threadIdx.x / WAVE; i < n; i += gridDim.x * PWPB) {
        if (!GZ_CHK(411, i, X.wmax + 6)) continue;
        const uint32_t lw = X.wlist[X.wmax + 6 - (int64_t)i];
        if (!GZ_CHK(412, lw, X.wmax)) continue;
        const uint32_t lrec = X.wtok[lw];
        if ((lrec & (W_MISS | W_PEND | W_HUGE)) != (W_MISS | W_PEND | W_HUGE)) continue;
        const uint32_t lstart = X.waux[lw];
        if (!GZ_CHK(413, lstart, X.B)) continue;
        int64_t lnb = lrec & 0x7FFFu;
        if (lnb == 0x7FFF)                                         // length did not fit 15 bits: find the end again
            lnb = scan_word_end(X, (int64_t)lstart + 1) - lstart;
        Emit E;
        E.ids = X.mtok + lstart; E.mask = nullptr; E.symout = nullptr; E.pad_hit = nullptr;
        E.limit = 0x7FFFFFFF; E.stop = 0x7FFFFFFF; E.ntok = 0; E.pad_id = 0x7FFFFFFF;
        const int nt = long_word(Tp, lsym[threadIdx.x / WAVE], PLONG, X.tb + lstart, lnb, (lrec & 0x8000u) != 0,
                                 reinterpret_cast<uint32_t*>(X.mtok + lstart), E, lane);
        if (lane == 0) X.wtok[lw] = W_MISS | (uint32_t)nt;
    }
}

// -----------------------------------------------------------------------------------------------------------------
// K3: assemble rows
// -----------------------------------------------------------------------------------------------------------------
namespace {
struct AsmLds {
    uint32_t dw[GMAX + 1];
    int32_t doc_ntok[GMAX];
    int64_t row_base[GMAX];
    uint8_t pad_hit[GMAX];
};
}  // namespace

__global__ __launch_bounds__(WAVE * PWPB) void gz_assemble_kernel(const GzDeviceTables* __restrict__ Tp, GzAsmArgs A)
{
    __shared__ AsmLds lds[PWPB];
    const GzDeviceTables T = *Tp;
    const int lane = lane_id();
    const int64_t d0 = ((int64_t)blockIdx.x * PWPB + threadIdx.x / WAVE) * A.docs_per_wave;
    if (d0 >= A.n_docs) return;
    AsmLds& L = lds[threadIdx.x / WAVE];
    const int g = (int)(A.n_docs - d0 < A.docs_per_wave ? A.n_docs - d0 : A.docs_per_wave);
    int32_t* out = A.dense ? A.ids : A.raw;
    const int limit = A.dense ? A.max_len - 1 : 0x7FFFFFFF;    // position max_len-1 is eos or padding
    const int stop = A.dense ? A.max_len : 0x7FFFFFFF;
    auto emit = [&](int doc, int pos, int32_t id) {
        if (pos < limit) {
            out[L.row_base[doc] + pos] = id;
            if (id == T.pad_id) L.pad_hit[doc] = 1;
        }
    };
    if (lane < g) {
        const int64_t d = d0 + lane;
        int64_t rb;
        if (A.dense) rb = d * (int64_t)A.max_len;
        else rb = (A.X[0].off[d] - A.X[0].off[0]) + 2 * d + (A.n_texts > 1 ? (A.X[1].off[d] - A.X[1].off[0]) + 2 * d : 0);
        L.row_base[lane] = rb;
        L.pad_hit[lane] = 0;
        L.doc_ntok[lane] = 1;
        if (0 < limit) { out[rb] = T.bos_id; if (T.bos_id == T.pad_id) L.pad_hit[lane] = 1; }       // tokenize.py:134-135
    }
    for (int tx = 0; tx < A.n_texts; ++tx) {
        const GzTextBufs& X = A.X[tx];
        // lane k holds the first word of document k (lane g: one past the group's last word) and the token count
        // document k starts this text with; the walk below reads them with v_readlane (k is wave-uniform)
        const uint32_t dwv = lane <= g ? X.docw0[d0 + lane] : 0xFFFFFFFFu;
        const int ntokv = lane < g ? L.doc_ntok[lane] : 0;
        const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, 0), w1 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, g);
        // the document the chunk's first word belongs to: the last one whose first word is <= that word
        int cur = 0;
        while (cur + 1 < g && (uint32_t)__builtin_amdgcn_readlane((int)dwv, cur + 1) <= w0) ++cur;
        int cur_n = __builtin_amdgcn_readlane(ntokv, cur);      // tokens `cur` holds before the chunk's first lane
        for (uint32_t c = w0; c < w1; c += WAVE) {
            const uint32_t w = c + lane;
            // pass 1 over the documents that start inside this chunk: document and starting count of every lane
            int doc = cur, start = cur_n;
            int kk = cur + 1;
            while (kk < g) {
                const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, kk);
                if (s0 >= c + WAVE) break;
                const bool ge = w >= s0;
                doc = ge ? kk : doc;
                start = ge ? __builtin_amdgcn_readlane(ntokv, kk) : start;
                ++kk;
            }
            const bool valid = w < w1 && start < stop;                           // a full row reads nothing more
            const uint32_t rec = valid ? X.wtok[w] : 0u;
            const bool miss = (rec & W_MISS) != 0;
            const int cnt = valid ? (miss ? miss_count(rec) : 1) : 0;
            int total;
            const int excl = wave_excl_sum(cnt, lane, total);
            // pass 2: tokens of the chunk that precede each lane's document, and the final count of every document
            // that ends inside the chunk
            int segb = 0, seg0 = 0;                                               // seg0: wave-uniform copy for `cur`
            for (int k2 = cur + 1; k2 < kk; ++k2) {
                const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, k2);
                const int e = s0 - c < (uint32_t)WAVE ? __builtin_amdgcn_readlane(excl, (int)(s0 - c)) : total;
                segb = w >= s0 ? e : segb;
                if (lane == 0) L.doc_ntok[cur] = cur_n + (e - seg0);
                cur = k2; cur_n = __builtin_amdgcn_readlane(ntokv, k2); seg0 = e;
            }
            cur_n += total - seg0;
            if (valid) {
                const int pos = start + (excl - segb);
                if (!miss) emit(doc, pos, (int32_t)rec);
                else {
                    const int32_t* src = miss_pieces(X, rec, w);
                    for (int k = 0; k < cnt && pos + k < limit; ++k) emit(doc, pos + k, src[k]);
                }
            }
        }
        if (lane == 0) L.doc_ntok[cur] = cur_n;
        // A eos [eos B eos]   (tokenize.py:134-135, :237-239)
        const int reps = (A.n_texts > 1 && tx == 0) ? 2 : 1;
        if (lane < g) {
            const int p = L.doc_ntok[lane];
            for (int k = 0; k < reps; ++k) emit(lane, p + k, T.eos_id);
            L.doc_ntok[lane] = p + reps;
        }
    }
    if (!A.dense) {
        if (lane < g) A.n_real[d0 + lane] = L.doc_ntok[lane];
        return;
    }
    // __padding (tokenize.py:141-146) + attention mask (:148-152), one row at a time, 16-byte streaming stores
    const int Lm = A.max_len;
    for (int j = 0; j < g; ++j) {
        const int Tn = L.doc_ntok[j];
        const int t = Tn < Lm ? Tn : Lm;
        const bool cut = Tn >= Lm;
        int32_t* ids = A.ids + L.row_base[j];
        int32_t* mask = A.mask + L.row_base[j];
        const int32_t tailv = cut ? T.eos_id : T.pad_id;
        const int first = cut ? Lm - 1 : t;
        const bool slow = L.pad_hit[j] != 0 || (cut && T.eos_id == T.pad_id);
        if ((Lm & 3) == 0) {
            for (int c = lane; c < Lm / 4; c += WAVE) {
                const int i0 = 4 * c;
                if (i0 >= first) nt_store4(ids + i0, tailv, tailv, tailv, tailv);
                else if (i0 + 4 > first) for (int i = first; i < i0 + 4; ++i) ids[i] = tailv;
                if (!slow) nt_store4(mask + i0, i0 < t, i0 + 1 < t, i0 + 2 < t, i0 + 3 < t);
            }
        } else {
            for (int i = lane; i < Lm; i += WAVE) {
                if (i >= first) ids[i] = tailv;
                if (!slow) mask[i] = i < t ? 1 : 0;
            }
        }
        if (slow) {                                                         // a real token equals the pad id
            __threadfence();
            for (int i = lane; i < Lm; i += WAVE) {
                const int32_t v = __builtin_nontemporal_load(ids + i);
                mask[i] = v != T.pad_id ? 1 : 0;
            }
        }
        if (lane == 0) A.n_real[d0 + j] = t;
    }
}

// -----------------------------------------------------------------------------------------------------------------
// K3, dense layouts with max_len a multiple of 4 and at most RB_TOK: the rows of a few documents are put together in
// LDS (bos, the words' tokens, eos: tokenize.py:134-135, :237-239) and leave as WHOLE rows -- input_ids with the
// truncation / padding tail (:141-146) and attention_mask = ids != pad (:148-152) -- in 16-byte streaming stores,
// every output byte written exactly once.  `dps` documents (rows) share the buffer: dps * max_len <= RB_TOK.
// -----------------------------------------------------------------------------------------------------------------
namespace {
constexpr int RB_TOK = 1024;                  // tokens of row buffer per wave (4 KiB)
struct alignas(16) RowsLds {
    int32_t rows[RB_TOK];                     // [dps][max_len]
    int32_t doc_ntok[GMAX];
};
}  // namespace

__global__ __launch_bounds__(WAVE * PWPB) void gz_rows_kernel(const GzDeviceTables* __restrict__ Tp, GzAsmArgs A, int dps, int lq_shift)
{
    typedef int __attribute__((ext_vector_type(4))) v4i;
    __shared__ RowsLds lds[PWPB];
    const GzDeviceTables T = *Tp;
    const int lane = lane_id();
    const int64_t dbeg = ((int64_t)blockIdx.x * PWPB + threadIdx.x / WAVE) * A.docs_per_wave;
    if (dbeg >= A.n_docs) return;
    const int64_t dend = A.n_docs - dbeg < A.docs_per_wave ? A.n_docs : dbeg + A.docs_per_wave;
    RowsLds& L = lds[threadIdx.x / WAVE];
    const int Lm = A.max_len, Lq = Lm >> 2;
    const int limit = Lm - 1;                                   // position max_len-1 is eos or padding
    const int stop = Lm;
    auto emit = [&](int doc, int pos, int32_t id) { if (pos < limit) L.rows[doc * Lm + pos] = id; };
    for (int64_t d0 = dbeg; d0 < dend; d0 += dps) {
        const int g = (int)(dend - d0 < dps ? dend - d0 : dps);
        if (lane < g) {
            L.doc_ntok[lane] = 1;
            emit(lane, 0, T.bos_id);                                                               // tokenize.py:134-135
        }
        for (int tx = 0; tx < A.n_texts; ++tx) {
            const GzTextBufs& X = A.X[tx];
            // lane k holds the first word of document k (lane g: one past the group's last word) and the token count
            // document k starts this text with; the walk below reads them with v_readlane (k is wave-uniform)
            const uint32_t dwv = lane <= g ? X.docw0[d0 + lane] : 0xFFFFFFFFu;
            const int ntokv = lane < g ? L.doc_ntok[lane] : 0;
            const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, 0), w1 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, g);
            int cur = 0;
            while (cur + 1 < g && (uint32_t)__builtin_amdgcn_readlane((int)dwv, cur + 1) <= w0) ++cur;
            int cur_n = __builtin_amdgcn_readlane(ntokv, cur);      // tokens `cur` holds before the chunk's first lane
            for (uint32_t c = w0; c < w1; c += WAVE) {
                // a chunk that lies inside ONE document whose row is already full has nothing to add
                if (cur_n >= stop && (cur + 1 >= g || (uint32_t)__builtin_amdgcn_readlane((int)dwv, cur + 1) >= c + WAVE)) continue;
                const uint32_t w = c + lane;
                int doc = cur, start = cur_n;
                int kk = cur + 1;
                while (kk < g) {
                    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, kk);
                    if (s0 >= c + WAVE) break;
                    const bool ge = w >= s0;
                    doc = ge ? kk : doc;
                    start = ge ? __builtin_amdgcn_readlane(ntokv, kk) : start;
                    ++kk;
                }
                const bool valid = w < w1 && start < stop;                           // a full row reads nothing more
                const uint32_t rec = valid ? X.wtok[w] : 0u;
                const bool miss = (rec & W_MISS) != 0;
                const int cnt = valid ? (miss ? miss_count(rec) : 1) : 0;
                int total;
                const int excl = wave_excl_sum(cnt, lane, total);
                int segb = 0, seg0 = 0;                                               // seg0: wave-uniform copy for `cur`
                for (int k2 = cur + 1; k2 < kk; ++k2) {
                    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)dwv, k2);
                    const int e = s0 - c < (uint32_t)WAVE ? __builtin_amdgcn_readlane(excl, (int)(s0 - c)) : total;
                    segb = w >= s0 ? e : segb;
                    if (lane == 0) L.doc_ntok[cur] = cur_n + (e - seg0);
                    cur = k2; cur_n = __builtin_amdgcn_readlane(ntokv, k2); seg0 = e;
                }
                cur_n += total - seg0;
                if (valid) {
                    const int pos = start + (excl - segb);
                    if (!miss) emit(doc, pos, (int32_t)rec);
                    else {
                        const int32_t* src = miss_pieces(X, rec, w);
                        for (int k = 0; k < cnt && pos + k < limit; ++k) emit(doc, pos + k, src[k]);
                    }
                }
            }
            if (lane == 0) L.doc_ntok[cur] = cur_n;
            // A eos [eos B eos]   (tokenize.py:134-135, :237-239)
            const int reps = (A.n_texts > 1 && tx == 0) ? 2 : 1;
            if (lane < g) {
                const int p = L.doc_ntok[lane];
                for (int k = 0; k < reps; ++k) emit(lane, p + k, T.eos_id);
                L.doc_ntok[lane] = p + reps;
            }
        }
        // the g rows are one contiguous span of the outputs and of the LDS buffer: 16 bytes per lane and step
        int32_t* ids = A.ids + d0 * (int64_t)Lm;
        int32_t* mask = A.mask + d0 * (int64_t)Lm;
        const int n16 = g * Lq;
        for (int idx = lane; idx < n16; idx += WAVE) {
            int j, q;
            if (lq_shift >= 0) { j = idx >> lq_shift; q = idx & (Lq - 1); }
            else { j = idx / Lq; q = idx - j * Lq; }
            const int Tn = L.doc_ntok[j];
            const bool cut = Tn >= Lm;                                               // __padding: tokens[:max_len-1] + [eos]
            const int first = cut ? Lm - 1 : Tn;
            const int32_t tailv = cut ? T.eos_id : T.pad_id;
            const int p = 4 * q;
            v4i v = *reinterpret_cast<const v4i*>(&L.rows[4 * idx]);
            v.x = p < first ? v.x : tailv;
            v.y = p + 1 < first ? v.y : tailv;
            v.z = p + 2 < first ? v.z : tailv;
            v.w = p + 3 < first ? v.w : tailv;
            nt_store4(ids + 4 * idx, v.x, v.y, v.z, v.w);
            nt_store4(mask + 4 * idx, v.x != T.pad_id, v.y != T.pad_id, v.z != T.pad_id, v.w != T.pad_id);   // :148-152
        }
        if (lane < g) { const int Tn = L.doc_ntok[lane]; A.n_real[d0 + lane] = Tn < Lm ? Tn : Lm; }
    }
}

// -----------------------------------------------------------------------------------------------------------------
// K3 for single texts (the bulk of every workload), dense layouts, max_len a multiple of 4 and <= CAP: the same rows,
// built for memory-level parallelism.  The kernels above walk their words chunk by chunk, one dependent load per
// chunk; here a wave works in ROUNDS of as many documents as fit its LDS (CAP words, CAP tokens):
//   1. one load: first-word indices of the next documents;
//   2. the word records of ALL of them by LDS-DMA (global_load_lds, one per document and 64 words, all in flight at
//      once, no registers), only the first max_len-1 words of a document: later ones cannot reach the row;
//   3. document by document out of LDS: token counts, prefix sum, positions; ids of table hits go to the token buffer,
//      words the merge kernels produced go on a list;
//   4. the list in one sweep: byte offset (waux), then the pieces (mtok), four loads in flight per lane;
//   5. rows out: 16 bytes per lane, ids with the truncation / padding tail and mask = ids != pad, written once.
// Three or four dependent memory round trips per ROUND instead of one or two per 64 words.
// -----------------------------------------------------------------------------------------------------------------
namespace {
#ifndef GZ_ROWS_RMAX
#define GZ_ROWS_RMAX 16
#endif
#ifndef GZ_ROWS_MLCAP
#define GZ_ROWS_MLCAP 96
#endif
constexpr int RMAX = GZ_ROWS_RMAX;            // documents per round at most
constexpr int MLCAP = GZ_ROWS_MLCAP;          // merged words per round on the LDS list (more: handled in place); with CAP = 512
                                              // the workgroup's LDS stays under 20 KB: 8 workgroups = 32 waves per CU
template <int CAP>
struct alignas(16) Rows1Lds {
    uint32_t wt[CAP];                         // word records of the round's documents, document after document
    int32_t tok[CAP + 4];                     // their rows without padding: bos, tokens, eos (at most max_len-1 each)
    uint32_t mlw[MLCAP];                      // merged words: place of the tokens (near record), or 1 << 31 | index of the word's slot in wt, which receives it ...
    uint32_t mld[MLCAP];                      // ... first token's place in tok | pieces to copy << 16
    int32_t dtb[RMAX];                        // per document: start in tok
    int32_t dfirst[RMAX];                     // ... stored entries (positions below it come from tok) | cut << 30
};
}  // namespace

#ifndef GZ_ROWS_WPB
#define GZ_ROWS_WPB 4
#endif
constexpr int RWPB = GZ_ROWS_WPB;             // waves per workgroup of gz_rows1_kernel (a workgroup's wave slots and LDS come free when its LAST wave has drained its stores)
template <int CAP>
__global__ __launch_bounds__(WAVE * RWPB) void gz_rows1_kernel(const GzDeviceTables* __restrict__ Tp, GzAsmArgs A, int lq_shift, int dbg_in)
{
    const int dbg = GZ_DIAG_ON ? dbg_in : 0;                    // timing switches: diagnostic builds only
    typedef const uint32_t __attribute__((address_space(1)))* g_u32;
    typedef uint32_t __attribute__((address_space(3)))* l_u32;
    __shared__ Rows1Lds<CAP> lds[RWPB];
    const GzDeviceTables T = *Tp;
    const int lane = lane_id();
    const int64_t dbeg = ((int64_t)blockIdx.x * RWPB + threadIdx.x / WAVE) * A.docs_per_wave;
    if (dbeg >= A.n_docs) return;
    const int64_t dend = A.n_docs - dbeg < A.docs_per_wave ? A.n_docs : dbeg + A.docs_per_wave;
    Rows1Lds<CAP>& L = lds[threadIdx.x / WAVE];
    const GzTextBufs& X = A.X[0];
    const int Lm = A.max_len, Lq = Lm >> 2;
    const int limit = Lm - 1;                                   // position max_len-1 is eos or padding
    PROF_DECL;                                                  // (diagnostic build: cycles per phase of a round, gz_prof[24 ..])
    for (int64_t da = dbeg; da < dend;) {
        PROF(6);
        PROF_CNT(10, 1);
        // ---- 1. the next documents and how many of their words can matter
        int nd = (int)(dend - da < RMAX ? dend - da : RMAX);
        const uint32_t dwv = X.docw0[da + (lane < nd ? lane : nd)];
        const uint32_t dwn = (uint32_t)__shfl_down((int)dwv, 1, WAVE);
        (void)GZ_CHK(511, dwv, X.wmax + 1);
        (void)GZ_CHK(512, (lane < nd && dwv > dwn) ? 1 : 0, 1);                 // (first-word indices do not decrease)
        const int kw = (lane < nd && !(dbg & 1)) ? (int)(dwn - dwv < (uint32_t)limit ? dwn - dwv : (uint32_t)limit) : 0;   // (dbg: timing diagnostics only)
        int tot;
        const int lb = wave_excl_sum(kw, lane, tot);
        {
            const uint64_t fit = wballot(lane < nd && lb + kw <= CAP);          // a prefix of the lanes (kw <= limit < CAP: never empty)
            nd = __ffsll((unsigned long long)~fit) - 1;
        }
        PROF(0);
        // ---- 2. word records -> LDS, every load in flight at once
        for (int j = 0; j < nd; ++j) {
            const uint32_t w0j = (uint32_t)__builtin_amdgcn_readlane((int)dwv, j);
            const int kwj = __builtin_amdgcn_readlane(kw, j), lbj = __builtin_amdgcn_readlane(lb, j);
            for (int c = 0; c < kwj; c += WAVE)
                if (c + lane < kwj)
                    __builtin_amdgcn_global_load_lds((g_u32)(X.wtok + w0j + c + lane), (l_u32)(L.wt + lbj + c), 4, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PROF(1);
        // ---- 3. positions, document by document
        int tb = 0, nml = 0, my_tb = 0, my_run = 0;
        bool far_seen = false;                                                    // (wave-uniform) a waux load is under way
        for (int j = 0; j < nd; ++j) {
            const uint32_t w0j = (uint32_t)__builtin_amdgcn_readlane((int)dwv, j);
            const int kwj = __builtin_amdgcn_readlane(kw, j), lbj = __builtin_amdgcn_readlane(lb, j);
            const int nml0 = nml;
            int run = 1;                                                          // bos
            for (int c = 0; c < kwj && run < limit; c += WAVE) {
                const bool valid = c + lane < kwj;
                const uint32_t rec = valid ? L.wt[lbj + c + lane] : 0u;
                const bool miss = (rec & W_MISS) != 0 && !(dbg & 32);                // (dbg 32, timing diagnostics: every word taken for a table hit)
                const int cnt = valid ? (miss ? miss_count(rec) : 1) : 0;
                int total;
                const int pos = run + wave_excl_sum(cnt, lane, total);
                const bool room = valid && pos < limit && tb + pos < CAP;
                if (room && !miss) L.tok[tb + pos] = (int32_t)rec;
                const bool lst = room && miss;
                const uint64_t mb = wballot(lst);
                if (mb) {
                    const int at = nml + below(mb);
                    const int n = cnt < limit - pos ? cnt : limit - pos;
                    if (lst) {
                        if (at < MLCAP) {
                            // near record (nearly all): the place of the pieces is in the record.  Far record: it travels by
                            // LDS-DMA from waux into the word's own record slot -- the record is in a register by now --
                            // while the remaining documents are walked
                            const bool near = (rec & W_NEAR) != 0;
                            L.mlw[at] = near ? rec & (W_NEAR_MAX - 1u) : 0x80000000u | (uint32_t)(lbj + c + lane);
                            L.mld[at] = (uint32_t)(tb + pos) | ((uint32_t)n << 16);
                            if (!near) __builtin_amdgcn_global_load_lds((g_u32)(X.waux + w0j + (uint32_t)(c + lane)), (l_u32)(L.wt + lbj + c), 4, 0, 0);
                        } else {                                                  // list full: copy the pieces here and now
                            const int32_t* src = miss_pieces(X, rec, w0j + (uint32_t)(c + lane));
                            for (int k = 0; k < n && tb + pos + k < CAP; ++k) L.tok[tb + pos + k] = src[k];
                        }
                    }
                    far_seen |= wballot(lst && !(rec & W_NEAR)) != 0;
                    nml += __popcll(mb);
                    if (nml > MLCAP) nml = MLCAP;
                }
                run += total;
            }
            // (a document cut to its first max_len-1 words has run >= max_len-1: its row is full either way)
            const int Tn = run + 1;                                               // + eos            tokenize.py:134-135
            const bool cut = Tn >= Lm;                                            // __padding: tokens[:max_len-1] + [eos]
            const int first = cut ? limit : Tn;
            if (tb + first > CAP) { nml = nml0; nd = j; break; }                  // does not fit this round (j >= 1: first < CAP)
            if (lane == j) { my_tb = tb; my_run = run; }                          // (lane j keeps document j's figures: written out below, all at once)
            tb += first;
        }
        if (lane < nd) {
            const int Tn = my_run + 1;
            const bool cut = Tn >= Lm;
            L.tok[my_tb] = T.bos_id;
            if (my_run < limit) L.tok[my_tb + my_run] = T.eos_id;
            L.dtb[lane] = my_tb;
            L.dfirst[lane] = (cut ? limit : Tn) | (cut ? 1 << 30 : 0);
            A.n_real[da + lane] = Tn < Lm ? Tn : Lm;
        }
        PROF(2);
        // ---- 4. pieces of the merged words (their offsets have arrived in LDS): up to four pieces per lane and trip in flight
        if (dbg & 16) nml = 0;                                                    // (dbg 16, timing diagnostics: no piece pass at all)
        if (nml && far_seen) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int m0 = 0; m0 < nml; m0 += WAVE) {
            const bool on = m0 + lane < nml;
            const uint32_t md = on ? L.mld[m0 + lane] : 0u;
            const int dst = (int)(md & 0xFFFFu), n = (int)(md >> 16);
            uint32_t place = on ? L.mlw[m0 + lane] : 0u;
            place = (place & 0x80000000u) ? L.wt[place & 0x7FFFFFFFu] : (uint32_t)X.B + 32u + place;
            if (on && !GZ_CHK(513, (uint64_t)place + (uint32_t)n, 2 * (X.B + 32) + 1)) place = 0u;
            const int32_t* src = X.mtok + place;
            for (int k0 = 0; wballot(k0 < n) != 0; k0 += 4) {
                int32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = (k0 + k < n && !(dbg & 8)) ? src[k0 + k] : 0;          // (dbg 8, timing diagnostics: no piece loads)
#pragma unroll
                for (int k = 0; k < 4; ++k) if (k0 + k < n) L.tok[dst + k0 + k] = v[k];
            }
        }
        PROF(3);
        // ---- 5. rows out: the nd rows are one contiguous span of the outputs
        int32_t* ids = A.ids + da * (int64_t)Lm;
        int32_t* mask = A.mask + da * (int64_t)Lm;
        const int n16 = nd * Lq;
        for (int idx = lane; idx < n16; idx += WAVE) {
            int j, q;
            if (lq_shift >= 0) { j = idx >> lq_shift; q = idx & (Lq - 1); }
            else { j = idx / Lq; q = idx - j * Lq; }
            const int df = L.dfirst[j];
            const int first = df & 0xFFFF;
            const int32_t tailv = (df >> 30) ? T.eos_id : T.pad_id;
            const int p = 4 * q;
            // (a quad at or past the row's stored entries is all tail: it reads the row's first quad instead, so that every
            // read stays inside tok[]: dtb[j] + first <= CAP, and a quad that starts below `first` ends below first + 3)
            const int32_t* t = L.tok + L.dtb[j] + (p < first ? p : 0);
            const int32_t a0 = t[0], a1 = t[1], a2 = t[2], a3 = t[3];
            const int32_t v0 = p < first ? a0 : tailv, v1 = p + 1 < first ? a1 : tailv;
            const int32_t v2 = p + 2 < first ? a2 : tailv, v3 = p + 3 < first ? a3 : tailv;
            if (!(dbg & 4)) nt_store4(ids + 4 * idx, v0, v1, v2, v3);
            if (!(dbg & 2)) nt_store4(mask + 4 * idx, v0 != T.pad_id, v1 != T.pad_id, v2 != T.pad_id, v3 != T.pad_id);     // :148-152
        }
        PROF(4);
        if (dbg & 64) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); PROF(5); }       // (dbg 64: ... and until the stores are acknowledged)
        da += nd;
    }
    // (one wave in 61 reports: 150 000 waves adding to the same twelve words would take longer than the kernel)
    if (((int64_t)blockIdx.x * RWPB + threadIdx.x / WAVE) % 61 == 0) PROF_FLUSH(24);
}

// -----------------------------------------------------------------------------------------------------------------
// K3 for single texts WITHOUT padding (max_len None -- the reference's default -- or padding False: tokenize.py:247 then leaves
// the rows as encode() made them): row d = bos, every token of the document's words, eos (tokenize.py:134-135) at row_off[d],
// attention_mask = ids != pad (:148-152).  A row's place depends on every row before it, so the walk of gz_rows1_kernel is made
// TWICE:
//   count  (WRITE = false) the row lengths -> n_real; gz_rowlen_kernel and the 64-bit scan then make row_off -- and the total that
//          the caller's capacity is checked against;
//   write  (WRITE = true) the rows, every token written ONCE, at its final place: the documents of a round are one contiguous
//          span of the output, and the wave's LDS token buffer is that span.
// (gz_assemble_kernel + gz_finalize_kernel -- still the path of pairs and of the padded ragged shapes -- put the rows at worst-case
// places of a raw area and copy them from there: every token written twice and read once.)
// A round holds the documents whose words (both passes) and tokens (write pass: the count pass's lengths) fit CAP; a document that
// does not fit alone takes a plain walk of 64 words at a time straight to memory.
// -----------------------------------------------------------------------------------------------------------------
namespace {
template <int CAP, bool WRITE> struct RowsrLds : Rows1Lds<CAP> {};
template <int CAP> struct alignas(16) RowsrLds<CAP, false> {     // the count pass: the word records only (more waves per CU)
    uint32_t wt[CAP];
    int32_t tok[4];
    uint32_t mlw[1], mld[1];
};
}  // namespace

template <int CAP, bool WRITE>
__global__ __launch_bounds__(WAVE * PWPB) void gz_rowsr_kernel(const GzDeviceTables* __restrict__ Tp, GzAsmArgs A)
{
    typedef const uint32_t __attribute__((address_space(1)))* g_u32;
    typedef uint32_t __attribute__((address_space(3)))* l_u32;
    __shared__ RowsrLds<CAP, WRITE> lds[PWPB];
    const GzDeviceTables T = *Tp;
    const int lane = lane_id();
    const int64_t dbeg = ((int64_t)blockIdx.x * PWPB + threadIdx.x / WAVE) * A.docs_per_wave;
    if (dbeg >= A.n_docs) return;
    if (WRITE && A.row_off[A.n_docs] > A.capacity) {            // (every wave reads the same total: none writes)
        if (dbeg == 0 && lane == 0) *A.error_flag = 1;
        return;
    }
    const int64_t dend = A.n_docs - dbeg < A.docs_per_wave ? A.n_docs : dbeg + A.docs_per_wave;
    RowsrLds<CAP, WRITE>& L = lds[threadIdx.x / WAVE];
    const GzTextBufs& X = A.X[0];
    // one document alone, 64 words at a time (more words, or more tokens, than the LDS buffers hold)
    auto plain = [&](int64_t d, uint32_t w0, uint32_t w1) {
        int32_t* ids = nullptr;
        int32_t* mask = nullptr;
        if (WRITE) {
            const int64_t o = A.row_off[d];
            ids = A.ids + o; mask = A.mask + o;
            if (lane == 0) { ids[0] = T.bos_id; mask[0] = T.bos_id != T.pad_id ? 1 : 0; }
        }
        int64_t run = 1;                                                          // bos
        for (uint32_t c = w0; c < w1; c += WAVE) {
            const uint32_t w = c + (uint32_t)lane;
            const bool valid = w < w1;
            const uint32_t rec = valid ? X.wtok[w] : 0u;
            const bool miss = (rec & W_MISS) != 0;
            const int cnt = valid ? (miss ? miss_count(rec) : 1) : 0;
            int total;
            const int excl = wave_excl_sum(cnt, lane, total);
            if (WRITE && valid) {
                const int64_t pos = run + excl;
                if (!miss) { ids[pos] = (int32_t)rec; mask[pos] = (int32_t)rec != T.pad_id ? 1 : 0; }
                else {
                    const int32_t* src = miss_pieces(X, rec, w);
                    for (int k = 0; k < cnt; ++k) { const int32_t v = src[k]; ids[pos + k] = v; mask[pos + k] = v != T.pad_id ? 1 : 0; }
                }
            }
            run += total;
        }
        if (lane == 0) {
            if (WRITE) { ids[run] = T.eos_id; mask[run] = T.eos_id != T.pad_id ? 1 : 0; }
            else A.n_real[d] = (int32_t)(run + 1);
        }
    };
    for (int64_t da = dbeg; da < dend;) {
        // ---- 1. the next documents: their words, and (write pass) the row lengths the count pass left in n_real
        int nd = (int)(dend - da < RMAX ? dend - da : RMAX);
        const uint32_t dwv = X.docw0[da + (lane < nd ? lane : nd)];
        const uint32_t dwn = (uint32_t)__shfl_down((int)dwv, 1, WAVE);
        (void)GZ_CHK(521, dwv, X.wmax + 1);
        const uint32_t nwords = lane < nd ? dwn - dwv : 0u;
        const int kw = (int)(nwords < (uint32_t)(CAP + 1) ? nwords : (uint32_t)(CAP + 1));        // (CAP + 1: does not fit)
        int ntk = 0;
        if (WRITE && lane < nd) ntk = A.n_real[da + lane];
        const int ntc = (ntk >= 0 && ntk < CAP + 1) ? ntk : CAP + 1;
        int tot, ttot = 0;
        const int lb = wave_excl_sum(kw, lane, tot);
        const int tbv = WRITE ? wave_excl_sum(ntc, lane, ttot) : 0;                                // the document's start in tok
        {
            const uint64_t fit = wballot(lane < nd && lb + kw <= CAP && (!WRITE || tbv + ntc <= CAP));     // a prefix of the lanes
            nd = __ffsll((unsigned long long)~fit) - 1;
        }
        if (nd == 0) {
            plain(da, (uint32_t)__builtin_amdgcn_readlane((int)dwv, 0), (uint32_t)__builtin_amdgcn_readlane((int)dwv, 1));
            da += 1;
            continue;
        }
        // ---- 2. word records -> LDS, every load in flight at once
        for (int j = 0; j < nd; ++j) {
            const uint32_t w0j = (uint32_t)__builtin_amdgcn_readlane((int)dwv, j);
            const int kwj = __builtin_amdgcn_readlane(kw, j), lbj = __builtin_amdgcn_readlane(lb, j);
            for (int c = 0; c < kwj; c += WAVE)
                if (c + lane < kwj)
                    __builtin_amdgcn_global_load_lds((g_u32)(X.wtok + w0j + c + lane), (l_u32)(L.wt + lbj + c), 4, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // ---- 3. positions, document by document
        int nml = 0, my_run = 0;
        bool far_seen = false;                                                    // (wave-uniform) a waux load is under way
        for (int j = 0; j < nd; ++j) {
            const uint32_t w0j = (uint32_t)__builtin_amdgcn_readlane((int)dwv, j);
            const int kwj = __builtin_amdgcn_readlane(kw, j), lbj = __builtin_amdgcn_readlane(lb, j);
            const int tb = WRITE ? __builtin_amdgcn_readlane(tbv, j) : 0;
            int run = 1;                                                          // bos
            for (int c = 0; c < kwj; c += WAVE) {
                const bool valid = c + lane < kwj;
                const uint32_t rec = valid ? L.wt[lbj + c + lane] : 0u;
                const bool miss = (rec & W_MISS) != 0;
                const int cnt = valid ? (miss ? miss_count(rec) : 1) : 0;
                int total;
                const int pos = run + wave_excl_sum(cnt, lane, total);
                if (WRITE) {
                    const bool room = valid && tb + pos < CAP;                    // (always, when both passes count alike: the round was planned by tokens)
                    if (room && !miss) L.tok[tb + pos] = (int32_t)rec;
                    const bool lst = room && miss;
                    const uint64_t mb = wballot(lst);
                    if (mb) {
                        const int at = nml + below(mb);
                        const int n = cnt < CAP - (tb + pos) ? cnt : CAP - (tb + pos);
                        if (lst) {
                            if (at < MLCAP) {
                                const bool near = (rec & W_NEAR) != 0;
                                L.mlw[at] = near ? rec & (W_NEAR_MAX - 1u) : 0x80000000u | (uint32_t)(lbj + c + lane);
                                L.mld[at] = (uint32_t)(tb + pos) | ((uint32_t)n << 16);
                                if (!near) __builtin_amdgcn_global_load_lds((g_u32)(X.waux + w0j + (uint32_t)(c + lane)), (l_u32)(L.wt + lbj + c), 4, 0, 0);
                            } else {                                              // list full: copy the pieces here and now
                                const int32_t* src = miss_pieces(X, rec, w0j + (uint32_t)(c + lane));
                                for (int k = 0; k < n; ++k) L.tok[tb + pos + k] = src[k];
                            }
                        }
                        far_seen |= wballot(lst && !(rec & W_NEAR)) != 0;
                        nml += __popcll(mb);
                        if (nml > MLCAP) nml = MLCAP;
                    }
                }
                run += total;
            }
            if (lane == j) my_run = run;
        }
        if (lane < nd) {
            if (WRITE) {
                L.tok[tbv] = T.bos_id;
                if (tbv + my_run < CAP) L.tok[tbv + my_run] = T.eos_id;
            } else A.n_real[da + lane] = my_run + 1;                              // bos, the tokens, eos
        }
        if (WRITE) {
            // ---- 4. pieces of the merged words (their offsets have arrived in LDS): up to four pieces per lane and trip in flight
            if (nml && far_seen) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (int m0 = 0; m0 < nml; m0 += WAVE) {
                const bool on = m0 + lane < nml;
                const uint32_t md = on ? L.mld[m0 + lane] : 0u;
                const int dst = (int)(md & 0xFFFFu), n = (int)(md >> 16);
                uint32_t place = on ? L.mlw[m0 + lane] : 0u;
                place = (place & 0x80000000u) ? L.wt[place & 0x7FFFFFFFu] : (uint32_t)X.B + 32u + place;
                if (on && !GZ_CHK(523, (uint64_t)place + (uint32_t)n, 2 * (X.B + 32) + 1)) place = 0u;
                const int32_t* src = X.mtok + place;
                for (int k0 = 0; wballot(k0 < n) != 0; k0 += 4) {
                    int32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = k0 + k < n ? src[k0 + k] : 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (k0 + k < n) L.tok[dst + k0 + k] = v[k];
                }
            }
            // ---- 5. rows out: the nd rows are one contiguous span of the outputs, tok[0 .. span) in order
            const int span = __builtin_amdgcn_readlane(tbv, nd - 1) + __builtin_amdgcn_readlane(ntc, nd - 1);
            const int64_t o0 = A.row_off[da];
            int32_t* ids = A.ids + o0;
            int32_t* mask = A.mask + o0;
            for (int i = lane; i < span; i += WAVE) {
                const int32_t v = L.tok[i];
                __builtin_nontemporal_store(v, ids + i);
                __builtin_nontemporal_store(v != T.pad_id ? 1 : 0, mask + i);                         // :148-152
            }
        }
        da += nd;
    }
}

// -----------------------------------------------------------------------------------------------------------------
// Exchange step helpers: dense rows <-> their leading (non-padding) entries
// -----------------------------------------------------------------------------------------------------------------
__global__ void gz_copy_counts_kernel(const int32_t* n_real, int64_t n, uint32_t* out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)n_real[i];
}

// E = int32_t, or uint16_t when every id of the vocabulary fits 16 bits (half the bytes on the xGMI link).
// A wave takes CK consecutive rows and reads the first 64 entries of each side by side (a row's real entries are ~ 45: one trip; four rows per
// wave: 178 us for the 1.25 M rows of a shard, eight: 154, sixteen: 145-150);
// what a row has beyond 64 follows row by row.
#ifndef GZ_CK
#define GZ_CK 8
#endif
constexpr int CK = GZ_CK;
template <typename E>
__global__ __launch_bounds__(WAVE * PWPB) void gz_compact_kernel(const int32_t* rows, const uint32_t* off, int64_t n_rows,
                                                                  int32_t row_len, E* out, uint32_t* first /* may be null: [n_rows] where each row starts */)
{
    const int lane = lane_id();
    const int64_t r0 = ((int64_t)blockIdx.x * PWPB + threadIdx.x / WAVE) * CK;
    if (r0 >= n_rows) return;
    const int nr = (int)(n_rows - r0 < CK ? n_rows - r0 : CK);
    const uint32_t ov = off[r0 + (lane < nr ? lane : nr)];           // lane k: where row r0 + k starts (lane nr: where the last one ends)
    if (first && lane < nr) first[r0 + lane] = ov;
    uint32_t o[CK], t[CK];
    int32_t v[CK];
#pragma unroll
    for (int k = 0; k < CK; ++k) {
        o[k] = (uint32_t)__builtin_amdgcn_readlane((int)ov, k < nr ? k : nr);
        t[k] = (uint32_t)__builtin_amdgcn_readlane((int)ov, k < nr ? k + 1 : nr) - o[k];
        v[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < CK; ++k) if ((uint32_t)lane < t[k]) v[k] = rows[(r0 + k) * (int64_t)row_len + lane];
#pragma unroll
    for (int k = 0; k < CK; ++k) if ((uint32_t)lane < t[k]) out[o[k] + lane] = (E)v[k];
#pragma unroll
    for (int k = 0; k < CK; ++k) {
        if (t[k] <= (uint32_t)WAVE) continue;                        // (wave-uniform)
        const int32_t* src = rows + (r0 + k) * (int64_t)row_len;
        for (uint32_t i = WAVE + lane; i < t[k]; i += WAVE) out[o[k] + i] = (E)src[i];
    }
}

template <typename E>
__global__ __launch_bounds__(WAVE * PWPB) void gz_expand_kernel(const E* compact, const uint32_t* first, const int32_t* n_real, int64_t n_rows,
                                                                 int32_t row_len, int32_t pad_id, int32_t* ids, int32_t* mask, uint32_t total, int32_t* bad)
{
    // (row r's entries: n_real[r] of them from first[r] on -- the block says where every row starts: its rows may lie in any order)
    // A block comes from another process: a row that claims more entries than a row holds, or entries beyond the `total` the block
    // was announced with (a truncated block, one in another layout), is written as padding only and reported through `bad` --
    // never followed.
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * PWPB + threadIdx.x / WAVE;
    if (r >= n_rows) return;
    const uint32_t o = first[r];
    uint32_t t = (uint32_t)n_real[r];
    if (t > (uint32_t)row_len || (uint64_t)o + t > (uint64_t)total) {
        if (lane == 0) atomicOr(bad, 1);
        t = 0;
    }
    int32_t* di = ids + r * (int64_t)row_len;
    int32_t* dm = mask + r * (int64_t)row_len;
    for (int i = lane; i < row_len; i += WAVE) {
        const int32_t v = (uint32_t)i < t ? (int32_t)compact[o + i] : pad_id;
        di[i] = v;
        dm[i] = v != pad_id ? 1 : 0;                       // attention mask (tokenize.py:148-152)
    }
}

void gz_launch_row_offsets(const int32_t* n_real, int64_t n_rows, uint32_t* off /* n_rows+1 */, hipStream_t s)
{
    if (n_rows >= 8 * SC32) {                                    // many rows: local scans, their bases, the sum (gz_kernels.hip)
        hipLaunchKernelGGL(gz_scan32x_local_kernel, dim3((unsigned)(n_rows / SC32 + 1)), dim3(1024), 0, s, n_real, n_rows, off);
        hipLaunchKernelGGL(gz_scan32x_bases_kernel, dim3(1), dim3(1024), 0, s, off, n_rows);
        hipLaunchKernelGGL(gz_scan32x_add_kernel, dim3((unsigned)(n_rows / 256 + 1)), dim3(256), 0, s, off, n_rows);
        return;
    }
    if (n_rows > 0) hipLaunchKernelGGL(gz_copy_counts_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, n_real, n_rows, off);
    hipLaunchKernelGGL(gz_scan32_kernel, dim3(1), dim3(1024), 0, s, off, n_rows, (uint32_t*)nullptr);
}

void gz_launch_compact(const int32_t* rows, const uint32_t* off, int64_t n_rows, int32_t row_len, void* out, int bits, uint32_t* first, hipStream_t s)
{
    if (n_rows <= 0) return;
    const dim3 grid((unsigned)((n_rows + PWPB * CK - 1) / (PWPB * CK))), block(WAVE * PWPB);
    if (bits == 16) hipLaunchKernelGGL(gz_compact_kernel<uint16_t>, grid, block, 0, s, rows, off, n_rows, row_len, (uint16_t*)out, first);
    else hipLaunchKernelGGL(gz_compact_kernel<int32_t>, grid, block, 0, s, rows, off, n_rows, row_len, (int32_t*)out, first);
}

void gz_launch_expand(const void* compact, int bits, const uint32_t* first, const int32_t* n_real, int64_t n_rows, int32_t row_len, int32_t pad_id,
                      int32_t* ids, int32_t* mask, uint32_t total, int32_t* bad, hipStream_t s)
{
    if (n_rows <= 0) return;
    const dim3 grid((unsigned)((n_rows + PWPB - 1) / PWPB)), block(WAVE * PWPB);
    if (bits == 16) hipLaunchKernelGGL(gz_expand_kernel<uint16_t>, grid, block, 0, s, (const uint16_t*)compact, first, n_real, n_rows, row_len, pad_id, ids, mask, total, bad);
    else hipLaunchKernelGGL(gz_expand_kernel<int32_t>, grid, block, 0, s, (const int32_t*)compact, first, n_real, n_rows, row_len, pad_id, ids, mask, total, bad);
}

// -----------------------------------------------------------------------------------------------------------------
// (the launchers that need gz_hot.inc's kernels are defined there)
void gz_launch_hot_words(const GzOptions& O, const GzDeviceTables* T, const GzDeviceTables& Th, const GzTextBufs& X, int use_words, hipStream_t s);
void gz_launch_hot_pre(const GzDeviceTables* T, const GzDeviceTables& Th, const GzTextBufs& X, int use_words, hipStream_t s);
void gz_launch_hot_miss(const GzOptions& O, const GzDeviceTables* T, const GzDeviceTables& Th, const GzTextBufs& X, int use_words, hipStream_t s);
// (the merge stage of a BPE-dropout call: gz_dropout.inc)
void gz_launch_drop_miss(const GzOptions& O, const GzDeviceTables* T, const GzDeviceTables& Th, const GzTextBufs& X, int64_t n_docs, const GzDrop& R, hipStream_t s);
void gz_launch_drop_wide(const GzDeviceTables* T, const GzTextBufs& X, int64_t n_docs, const GzDrop& R, hipStream_t s);

void gz_launch_pipeline_text(const GzOptions& O, const GzDeviceTables* T, const GzDeviceTables& Th, const GzTextBufs& X, int64_t n_docs, int use_words, int32_t* long_flag,
                             hipStream_t s, hipStream_t side, hipEvent_t ev_fork0, hipEvent_t ev_fork, hipEvent_t ev_join, hipEvent_t ev_brk, const GzDrop* drop)
{
    const int fork_side = O.side;                              // 0: everything on one stream (tests)
    bool par0 = false;
    // bitmaps cover positions 0 .. B (inclusive), rounded up to whole tiles.  The document-start bits depend on the offsets
    // only: when those are readable now (ev_brk given), the 36 MB clear + gz_brk_kernel run on the SIDE stream, i.e. under the
    // kernels the main stream still has queued from the call before (its row kernel).  The side stream is in order, and every
    // earlier reader of this bitmap (classification, word kernel, long-word kernel) lies before something it has waited for.
    const size_t bm_bytes = (size_t)((X.B + TILE) / TILE) * (TILE / 8) + 64;
    const int brk_on = O.brk_side;                             // 0: on the main stream (tests)
    const bool brk_side = brk_on && fork_side && side && ev_fork0 && ev_fork && ev_join && ev_brk;
    hipStream_t sb = brk_side ? side : s;
    hipMemsetAsync(X.brk, 0, bm_bytes, sb);
    if (n_docs > 1)
        hipLaunchKernelGGL(gz_brk_kernel, dim3((unsigned)((n_docs + 255) / 256)), dim3(256), 0, sb, X.off, n_docs,
                           reinterpret_cast<uint32_t*>(X.brk));
    // block flags, the control words and the wide-word count behind them (one buffer): cleared with the start bits -- their users
    // in the call before (word kernel, scans, pre-pass; wide / long kernels on the side stream itself) are all ordered before it
    hipMemsetAsync(X.blklong, 0, (size_t)(X.ctl + 65 - X.blklong) * 4, sb);
    if (brk_side) { hipEventRecord(ev_brk, side); hipStreamWaitEvent(s, ev_brk, 0); }
    const unsigned nb = (unsigned)((X.nblk + PWPB - 1) / PWPB);
    // exclusive scans over the nblk block counts (+ the total at [nblk]): one workgroup for small batches, the chained
    // multi-workgroup scan beyond a few trips of it (tickets: ctl[2], ctl[3]; call numbers: X.epoch + 1, + 2)
    const int64_t scan_multi = O.scan_multi;
    auto scan32 = [&](uint32_t* v, uint32_t* grp, int which) {
        if (X.nblk < scan_multi)
            hipLaunchKernelGGL(gz_scan32_kernel, dim3(1), dim3(1024), 0, s, v, X.nblk, grp);
        else
            hipLaunchKernelGGL(gz_scan32m_kernel, dim3((unsigned)((X.nblk + SCH) / SCH)), dim3(256), 0, s, v, X.nblk, grp,
                               reinterpret_cast<unsigned long long*>(X.lookback), X.ctl + 2 + which, X.epoch + 1u + (uint32_t)which, long_flag - 3);
    };
    // (timing experiment, diagnostic build, ablate bit 0: the word kernel classifies its own tiles, see gz_words2_kernel -- the block
    //  counts, their scan and the bitmaps of the call BEFORE, on the same text, stay in place)
    if (!(GZ_DIAG_ON && (use_words & 0x100))) {
        hipLaunchKernelGGL(gz_classify_kernel, dim3(nb), dim3(WAVE * PWPB), 0, s, X);
        scan32(X.blkcnt, nullptr, 0);
    }
    // the first word of every document is only needed by the row kernel: it goes on the side stream, BESIDE THE WORD KERNEL (the
    // join before the row kernel covers it).  (Round 3 ran it with the wide-word kernels beside the merge kernel -- one fork
    // instead of two; the merge kernel is now shorter than those three together, and the row kernel waited for the side stream.)
    // (a dropout call's merge kernels look a word's document up in docw0: there it stays on the main stream, before them)
    par0 = fork_side && side && ev_fork0 && ev_fork && ev_join && !drop;
    if (par0) {
        hipEventRecord(ev_fork0, s); hipStreamWaitEvent(side, ev_fork0, 0);
        hipLaunchKernelGGL(gz_docw0_kernel, dim3((unsigned)((n_docs + 1 + 255) / 256)), dim3(256), 0, side, X, n_docs);
    } else hipLaunchKernelGGL(gz_docw0_kernel, dim3((unsigned)((n_docs + 1 + 255) / 256)), dim3(256), 0, s, X, n_docs);
    gz_launch_hot_words(O, T, Th, X, use_words, s);
    scan32(X.blkmiss, X.grpblk, 1);
    auto wide = [&](hipStream_t q) {
        if (drop) { gz_launch_drop_wide(T, X, n_docs, *drop, q); return; }
        const int ldw = Th.pair_ph.nbuckets <= GZ_PH_LDS_BUCKETS ? 1 : 0;
        hipLaunchKernelGGL(gz_miss_wide_kernel, dim3(nb < 2048u ? nb : 2048u), dim3(WAVE * PWPB), ldw ? (size_t)Th.pair_ph.nbuckets * 2 : 0, q, T, X, long_flag, ldw);   // (grid-stride over the list)
        hipLaunchKernelGGL(gz_long_kernel, dim3(nb < 1024u ? nb : 1024u), dim3(WAVE * PWPB), 0, q, T, X, (const int32_t*)long_flag);
    };
    // the pre-pass sorts the misses and hands the words of more than 16 symbols to the wide-word kernels, which then run
    // on the side stream BESIDE the merge kernel (they touch disjoint words)
    gz_launch_hot_pre(T, Th, X, use_words, s);
    const bool par = fork_side && side && ev_fork && ev_join;
    if (par) {
        hipEventRecord(ev_fork, s); hipStreamWaitEvent(side, ev_fork, 0);
        wide(side);
        hipEventRecord(ev_join, side);
    }
    if (drop) gz_launch_drop_miss(O, T, Th, X, n_docs, *drop, s);
    else gz_launch_hot_miss(O, T, Th, X, use_words, s);
    if (par) hipStreamWaitEvent(s, ev_join, 0);
    else wide(s);
}

// single texts without padding: pass 0 = the row lengths -> A.n_real, pass 1 = the rows at A.row_off (gz_rowsr_kernel); between the two
// the caller runs gz_launch_rowscan over n_real
void gz_launch_rows_ragged(const GzDeviceTables* T, const GzAsmArgs& A0, int pass, int64_t text_bytes, hipStream_t s)
{
    GzAsmArgs A = A0;
    if (A.n_docs <= 0) return;
    // long documents: few per wave and the large buffers (a document of more than CAP words or tokens takes the slow walk)
    const int64_t avg = text_bytes / A.n_docs;
    const bool big = avg > 1024;
    A.docs_per_wave = big ? 1 : 8;
    const int64_t waves = (A.n_docs + A.docs_per_wave - 1) / A.docs_per_wave;
    const int64_t blocks = (waves + PWPB - 1) / PWPB;
    if (big) {
        if (pass == 0) hipLaunchKernelGGL((gz_rowsr_kernel<1536, false>), dim3((unsigned)blocks), dim3(WAVE * PWPB), 0, s, T, A);
        else hipLaunchKernelGGL((gz_rowsr_kernel<1536, true>), dim3((unsigned)blocks), dim3(WAVE * PWPB), 0, s, T, A);
    } else {
        if (pass == 0) hipLaunchKernelGGL((gz_rowsr_kernel<512, false>), dim3((unsigned)blocks), dim3(WAVE * PWPB), 0, s, T, A);
        else hipLaunchKernelGGL((gz_rowsr_kernel<512, true>), dim3((unsigned)blocks), dim3(WAVE * PWPB), 0, s, T, A);
    }
}

void gz_launch_assemble(const GzOptions& O, const GzDeviceTables* T, const GzAsmArgs& A0, hipStream_t s)
{
    GzAsmArgs A = A0;
    const int which = O.assemble;                              // tests: 1 scatter kernel, 2 LDS rows, 3 default
    if (which >= 3 && A.dense && A.n_texts == 1 && A.max_len >= 4 && (A.max_len & 3) == 0 && A.max_len <= 1024) {
        // single texts: rounds of bulk-loaded documents (gz_rows1_kernel)
        const int Lq = A.max_len >> 2;
        int lq_shift = -1;
        if ((Lq & (Lq - 1)) == 0) { lq_shift = 0; while ((1 << lq_shift) < Lq) ++lq_shift; }
        // a wave takes ONE round of documents (a wave's next loads would wait behind its own row stores: vmcnt counts both in
        // issue order); many more waves than wave slots, so that the last ones do not idle the chip
#ifndef GZ_ROWS_DPW_DEFAULT
#define GZ_ROWS_DPW_DEFAULT 8
#endif
        // (rows of more than 512 entries: ONE document per wave -- BASELINE configs[4], 50 k long documents, max_len 1024: 167 us with
        //  four per wave, 153 with two, 149 with one: few waves, and each full row is a long gather of records and pieces)
        int64_t dpw = A.max_len <= 256 ? GZ_ROWS_DPW_DEFAULT : A.max_len <= 512 ? 4 : 1;
#if defined(GZ_DIAG) || defined(GZ_ABLATE)
        const int dpw_env = O.rows_dpw;
        const int dbg = O.rows_dbg;                            // timing diagnostics only (diagnostic builds): results are wrong when set
#else
        const int dpw_env = 0, dbg = 0;
#endif
        if (dpw_env > 0) dpw = dpw_env;
        A.docs_per_wave = (int32_t)dpw;
        const int64_t waves = (A.n_docs + dpw - 1) / dpw;
        const int64_t blocks = (waves + PWPB - 1) / PWPB;
        if (blocks <= 0) return;
#ifndef GZ_ROWS_CAP
#define GZ_ROWS_CAP 512
#endif
        // (round 6 measured a form of this kernel with the loads and the stores of a round in DIFFERENT waves -- producer and consumer waves
        //  of persistent workgroups, a round handed over in LDS: commits d395452 and the one after it, profiles/r06_ab_variants.txt series 6 --
        //  and it loses: loads and stores do not overlap in the memory system either)
        const int64_t rblocks = (waves + RWPB - 1) / RWPB;
        if (A.max_len <= 256) hipLaunchKernelGGL(gz_rows1_kernel<GZ_ROWS_CAP>, dim3((unsigned)rblocks), dim3(WAVE * RWPB), 0, s, T, A, lq_shift, dbg);
        else hipLaunchKernelGGL(gz_rows1_kernel<1024>, dim3((unsigned)rblocks), dim3(WAVE * RWPB), 0, s, T, A, lq_shift, dbg);
        return;
    }
    if (which >= 2 && A.dense && A.max_len >= 4 && (A.max_len & 3) == 0 && A.max_len <= RB_TOK) {
        // whole rows through LDS: dps rows share a wave's 4-KiB buffer; a wave walks ~16 documents, sub-group by sub-group
        int dps = RB_TOK / A.max_len;
        if (dps > GMAX) dps = GMAX;
        const int Lq = A.max_len >> 2;
        int lq_shift = -1;
        if ((Lq & (Lq - 1)) == 0) { lq_shift = 0; while ((1 << lq_shift) < Lq) ++lq_shift; }
        int64_t dpw = (GMAX / dps) * dps;
        const int64_t by_waves = (A.n_docs / 16384) / dps * dps;                       // keep >= 16 K waves when possible
        if (dpw > by_waves) dpw = by_waves;
        if (dpw < dps) dpw = dps;
        A.docs_per_wave = (int32_t)dpw;
        const int64_t waves = (A.n_docs + dpw - 1) / dpw;
        const int64_t blocks = (waves + PWPB - 1) / PWPB;
        if (blocks > 0) hipLaunchKernelGGL(gz_rows_kernel, dim3((unsigned)blocks), dim3(WAVE * PWPB), 0, s, T, A, dps, lq_shift);
        return;
    }
    const int64_t waves = (A.n_docs + A.docs_per_wave - 1) / A.docs_per_wave;
    const int64_t blocks = (waves + PWPB - 1) / PWPB;
    if (blocks > 0) hipLaunchKernelGGL(gz_assemble_kernel, dim3((unsigned)blocks), dim3(WAVE * PWPB), 0, s, T, A);
}
