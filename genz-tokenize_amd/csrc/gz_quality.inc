// gz_quality.inc -- the text half of the Gopher quality rule (Rae et al., 2021, table A1), included by gz_kernels.hip: per-document
// character, word, symbol, line and paragraph signals from packed UTF-8 in HBM, and the duplicate lines and paragraphs of a document.
// The rule is stated in include/genz_tokenize.h ("---- quality") and restated in plain Python in tests/quality_oracle.py.
//
//   gz_quality_walk_kernel<W>  one wave per document, QZ_WPB documents per workgroup, QZ_TRIP = 256 bytes per trip: a lane takes 4
//                              consecutive bytes in one (unaligned) dword load -- the next trip's dword is in flight while this trip's
//                              is classified --, and sees its neighbours' dwords by DPP shifts, so every byte class (the whitespace of
//                              is_ws1/2/3, word, '\n', '.', '#', character start, letter, bullet, ellipsis) is LOCAL to a lane: no
//                              whitespace spill and no previous-byte bit cross a trip, only the trip's last dword does.
//                              What is sequential -- the newlines of the open gap (saturating at 2), the open run of dots (mod 3), "the
//                              open word has a letter", "the last word byte ended an ellipsis", "a word was seen" -- a lane learns from
//                              BALLOTS of its lower lanes' one- and two-bit summaries (find the highest lower lane that breaks the chain,
//                              count what lies between by popcount): no shuffle, no LDS.  Counts stay in per-lane registers until the
//                              document ends: ten wave sums a document, not a trip.
//        W = false (pass A)    the nine text-only signals and the document's line and paragraph counts, into the WORKSPACE, and the
//                              control words the host reads back once: the totals, the extent, "a document is too long", "offsets
//                              decrease" -- so that every refusal comes before anything of the caller's is written
//        W = true  (pass B)    the spans.  Span hashes come WITHOUT a second pass over the bytes and without a segmented scan: with
//                              F(x) = sum over q < x of (byte[q] + 1) * R^q (two independent 32-bit lanes of arithmetic, R1 and R2
//                              odd), the polynomial of a span [s, e) is (F(e) - F(s)) * R^-s -- a function of its bytes alone.  ONE
//                              unsegmented wave scan of the lanes' sums gives F at every byte and serves lines and paragraphs both;
//                              a second scan carries the characters and the heads before a lane.  A head writes its span's head half
//                              (start, F, characters, R^-start, document) and the END half of the span before it: position, F and
//                              characters at the last word byte before the head, fetched from the highest lower lane that has a
//                              word byte (four shuffles a trip) -- trailing whitespace never enters a hash, nothing looks ahead.
//   gz_quality_insert_kernel   a lane per span: h = mix(polynomial, length, characters, kind, document) & hmask (switch
//                              quality_hash_bits); one open-addressing table per call, a slot = tag << 32 | span index, claimed by a
//                              64-bit CAS from 0; on an equal tag the occupant is the same key only if kind, document and length agree
//                              and the BYTES are equal (dwords where both spans are aligned alike) -- then atomicMin leaves the
//                              smallest span index; else the next slot.  Spans above QZ_LONG bytes go to a list instead ...
//   gz_quality_insert_long_kernel  ... and are inserted a WAVE per span: the lanes compare 256 bytes a step.
//   gz_quality_resolve_kernel  after the kernel boundary, a wave per document: first = the index in its span's slot; the five
//                              duplicate signals reduced in registers, *_first and *_span written when asked for.
//
// Vector stores and vector atomics only.  Every order-dependent value is an integer sum (the totals) or a minimum (a slot's span
// index); which of two different keys with equal tags sits first along a probe sequence varies, and no answer reads it: a lookup
// compares bytes.  A hash decides where to look, never whether two spans are equal, nor whether they stand in the same document.
// No load falls outside [text + off[0], text + off[n_docs]): a dword load lies inside its document, the last bytes of a document and of
// a span are read one by one.

namespace {

constexpr int QZ_WPB = GZ_QUALITY_WPB;             // waves (documents) per workgroup of the walk and of the resolve
constexpr int QZ_TRIP = WAVE * 4;                  // bytes of one trip of the walk
constexpr uint32_t QZ_LONG = 512;                  // spans above this many bytes are compared a wave per span
constexpr uint32_t QZ_R1 = 0x01000193u, QZ_R2 = 0x9E3779B1u;      // the two polynomials' bases (odd: invertible mod 2^32)

constexpr uint32_t qz_inv32(uint32_t a) { uint32_t x = a; for (int k = 0; k < 5; ++k) x *= 2u - a * x; return x; }
constexpr uint32_t qz_pow32(uint32_t a, uint32_t n) { uint32_t r = 1; for (; n; n >>= 1, a *= a) if (n & 1u) r *= a; return r; }
constexpr uint32_t QZ_I1 = qz_inv32(QZ_R1), QZ_I2 = qz_inv32(QZ_R2);
static_assert(QZ_R1 * QZ_I1 == 1u && QZ_R2 * QZ_I2 == 1u, "inverse of the polynomial bases");

__device__ __forceinline__ uint32_t qz_dpow(uint32_t a, uint32_t n) { uint32_t r = 1; for (; n; n >>= 1, a *= a) if (n & 1u) r *= a; return r; }

// the dword at p[i .. i + 4) of a document of len bytes; bytes at or past len read as 0 and are never loaded
__device__ __forceinline__ uint32_t qz_load4(const uint8_t* p, int64_t i, int64_t len)
{
    typedef uint32_t __attribute__((aligned(1))) u32_u;
    if (i + 4 <= len) return *reinterpret_cast<const u32_u*>(p + i);
    uint32_t v = 0;
    for (int k = 0; k < 3; ++k) if (i + k < len) v |= (uint32_t)p[i + k] << (8 * k);
    return v;
}

// a letter begins at a byte outside 0x80..0xBF: A-Z, a-z, or a code point >= U+00C0 other than U+00D7, U+00F7, U+2000..U+2BFF,
// U+3000..U+303F, U+FE00..U+FE0F and everything >= U+1F000 (a range rule, not Unicode's Alphabetic property).  The code point of a
// lead byte is put together from as many following bytes as the lead announces, whatever they are (absent ones are 0).
__device__ __forceinline__ bool qz_letter(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3)
{
    if (b0 < 0x80u) return ((b0 | 0x20u) - 0x61u) < 26u;
    if (b0 < 0xC0u) return false;
    const uint32_t cp = b0 < 0xE0u ? (b0 & 0x1Fu) << 6 | (b1 & 0x3Fu)
                      : b0 < 0xF0u ? (b0 & 0x0Fu) << 12 | (b1 & 0x3Fu) << 6 | (b2 & 0x3Fu)
                                   : (b0 & 0x07u) << 18 | (b1 & 0x3Fu) << 12 | (b2 & 0x3Fu) << 6 | (b3 & 0x3Fu);
    return cp >= 0xC0u && cp != 0xD7u && cp != 0xF7u && !(cp >= 0x2000u && cp <= 0x2BFFu) && !(cp >= 0x3000u && cp <= 0x303Fu) &&
           !(cp >= 0xFE00u && cp <= 0xFE0Fu) && cp < 0x1F000u;
}

// inclusive wave scan of u32 sums (wrapping), all in DPP as wave_excl_sum
__device__ __forceinline__ uint32_t qz_scan(uint32_t v, uint32_t& total)
{
    int x = (int)v;
    x = (int)((uint32_t)x + (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false));
    x = (int)((uint32_t)x + (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false));
    x = (int)((uint32_t)x + (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false));
    x = (int)((uint32_t)x + (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false));
    x = (int)((uint32_t)x + (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false));
    x = (int)((uint32_t)x + (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false));
    total = (uint32_t)__builtin_amdgcn_readlane(x, WAVE - 1);
    return (uint32_t)x;
}
__device__ __forceinline__ uint32_t qz_wave_sum(uint32_t v) { return (uint32_t)wave_sum((int)v); }

// The highest lane of `m` below the lanes of `below` (lt_mask(lane), or all ones: the state behind the trip): -1 when there is none.
// `between` = the lanes above it inside `below`.
__device__ __forceinline__ int qz_last(uint64_t m, uint64_t below, uint64_t& between)
{
    m &= below;
    if (!m) { between = below; return -1; }
    const int hl = 63 - __builtin_clzll(m);
    between = below & ~((2ull << hl) - 1ull);
    return hl;
}

// The walk of one document by one wave.  p = its first byte, len < 2^31 its bytes.
template <bool WRITE>
__device__ void qz_walk(const GzQualityArgs& A, int64_t d, const uint8_t* p, int64_t len)
{
    const int lane = lane_id();
    const uint64_t lt = lt_mask(lane);
    uint32_t a_chars = 0, a_words = 0, a_wchars = 0, a_alpha = 0, a_hash = 0, a_ell = 0, a_lines = 0, a_bul = 0, a_elll = 0, a_paras = 0;
    // what crosses a trip (the same in every lane): the dword before the trip, the open gap's newlines (0..2), "the last word byte
    // ended an ellipsis", "a word was seen", the open run of dots mod 3, "the open word has a letter"
    uint32_t c_prev = 0, c_g = 0, c_e = 0, c_seen = 0, c_dot = 0, c_al = 0;
    // pass B: F1, F2 and the characters before the trip, the lines and paragraphs before it, the end half at the last word byte,
    // and the lane's powers R^i, R^-i at its first byte i of the trip
    uint32_t c_f1 = 0, c_f2 = 0, c_ch = 0, c_nl = 0, c_np = 0, c_we = 0, c_wf1 = 0, c_wf2 = 0, c_wc = 0;
    uint32_t r1 = 0, r2 = 0, i1 = 0, i2 = 0;
    uint32_t lbase = 0, pbase = 0;
    if (WRITE) {
        r1 = qz_dpow(QZ_R1, 4u * lane); r2 = qz_dpow(QZ_R2, 4u * lane); i1 = qz_dpow(QZ_I1, 4u * lane); i2 = qz_dpow(QZ_I2, 4u * lane);
        lbase = A.loff[d]; pbase = (uint32_t)A.n_lines + A.poff[d];
    }
    uint32_t nxt = qz_load4(p, 4 * lane, len);
    for (int64_t t = 0; t < len; t += QZ_TRIP) {
        const int64_t i = t + 4 * lane;
        const uint32_t cur = nxt;
        nxt = qz_load4(p, i + QZ_TRIP, len);
        uint32_t pw = (uint32_t)__shfl_up((int)cur, 1, WAVE), nw = (uint32_t)__shfl_down((int)cur, 1, WAVE);
        const uint32_t n0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt);
        if (lane == 0) pw = c_prev;
        if (lane == WAVE - 1) nw = n0;
        c_prev = (uint32_t)__builtin_amdgcn_readlane((int)cur, WAVE - 1);
        // bytes -4 .. 7 around the lane's first byte
        const uint64_t lo = (uint64_t)pw | (uint64_t)cur << 32;
        auto B = [&](int k) -> uint32_t { return k < 4 ? (uint32_t)(lo >> (8 * (k + 4))) & 0xFFu : (nw >> (8 * (k - 4))) & 0xFFu; };
        // word bits of bytes -1 .. 4 (bit k + 1): inside the document and part of no whitespace character
        uint32_t W = 0;
#pragma unroll
        for (int k = -1; k <= 4; ++k) {
            const uint32_t m2 = B(k - 2), m1 = B(k - 1), b0 = B(k), p1 = B(k + 1), p2 = B(k + 2);
            const bool ws = is_ws1(b0) || is_ws2(b0, p1) || is_ws2(m1, b0) || is_ws3(b0, p1, p2) || is_ws3(m1, b0, p1) || is_ws3(m2, m1, b0);
            const bool in = i + k >= 0 && i + k < len;
            W |= (uint32_t)(in && !ws) << (k + 1);
        }
        const uint32_t Wn = (W >> 1) & 0xFu, ST = Wn & ~W & 0xFu, LB = Wn & ~(W >> 2);
        uint32_t NL = 0, DOT = 0, CS = 0, LET = 0, BUL = 0, EE = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t m2 = B(k - 2), m1 = B(k - 1), b0 = B(k), p1 = B(k + 1), p2 = B(k + 2), p3 = B(k + 3);
            const bool in = i + k < len;
            NL |= (uint32_t)(in && b0 == 0x0Au) << k;
            CS |= (uint32_t)(in && (b0 & 0xC0u) != 0x80u) << k;
            if (!WRITE) {
                DOT |= (uint32_t)(in && b0 == 0x2Eu) << k;
                a_hash += in && b0 == 0x23u;
                a_ell += in && b0 == 0xE2u && p1 == 0x80u && p2 == 0xA6u;                           // U+2026 begins here
                LET |= (uint32_t)(in && qz_letter(b0, p1, p2, p3)) << k;
                BUL |= (uint32_t)(b0 == 0x2Du || b0 == 0x2Au || (b0 == 0xE2u && ((p1 == 0x80u && p2 == 0xA2u) || (p1 == 0x97u && p2 == 0x8Fu)))) << k;
                EE |= (uint32_t)((b0 == 0x2Eu && m1 == 0x2Eu && m2 == 0x2Eu) || (b0 == 0xA6u && m1 == 0x80u && m2 == 0xE2u)) << k;   // "..." or U+2026 ends here
            }
        }
        // the lane's own summaries: newlines behind its last word byte (all of them when it has none), the ellipsis bit of that byte
        uint32_t g_loc = 0, e_loc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (Wn >> k & 1u) { g_loc = 0; e_loc = EE >> k & 1u; }
            else g_loc += NL >> k & 1u;
        }
        const uint64_t HASW = wballot(Wn != 0), G1 = wballot(g_loc >= 1), G2 = wballot(g_loc >= 2), EB = wballot(e_loc != 0);
        // the gap state in front of the lanes of `below`
        auto gap_in = [&](uint64_t below, uint32_t& g, uint32_t& e, uint32_t& seen) {
            uint64_t bt;
            const int hl = qz_last(HASW, below, bt);
            const uint32_t nls = (uint32_t)__popcll(G1 & bt) + (uint32_t)__popcll(G2 & bt);
            if (hl < 0) { g = c_g + nls; e = c_e; seen = c_seen; }
            else { g = (uint32_t)(G1 >> hl & 1ull) + (uint32_t)(G2 >> hl & 1ull) + nls; e = (uint32_t)(EB >> hl & 1ull); seen = 1; }
            g = g < 2 ? g : 2;
        };
        uint32_t g, e, seen;
        gap_in(lt, g, e, seen);
        // heads of the lane's four bytes
        uint32_t HL = 0, HP = 0;
        {
            uint32_t gg = g, ss = seen, ee = e;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (Wn >> k & 1u) {
                    if (ST >> k & 1u) {
                        const bool hl_ = !ss || gg >= 1, hp_ = !ss || gg >= 2;
                        HL |= (uint32_t)hl_ << k; HP |= (uint32_t)hp_ << k;
                        if (!WRITE && hl_ && ss) a_elll += ee;
                    }
                    ss = 1; gg = 0; ee = EE >> k & 1u;
                } else if (NL >> k & 1u) gg = gg < 2 ? gg + 1 : 2;
            }
        }
        if (!WRITE) {
            a_chars += (uint32_t)__popc(CS); a_wchars += (uint32_t)__popc(CS & Wn); a_words += (uint32_t)__popc(ST);
            a_lines += (uint32_t)__popc(HL); a_paras += (uint32_t)__popc(HP); a_bul += (uint32_t)__popc(HL & BUL);
            // runs of dots: a run of k dots counts k / 3.  A lane's trailing dots (0..3 unless all four are dots)
            uint32_t run = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) run = (DOT >> k & 1u) ? run + 1 : 0;
            const uint64_t NFULL = wballot(DOT != 0xFu), A0 = wballot((run & 1u) != 0), A1 = wballot((run & 2u) != 0);
            auto dot_in = [&](uint64_t below, uint32_t n_below) -> uint32_t {
                uint64_t bt;
                const int hl = qz_last(NFULL, below, bt);
                return hl < 0 ? c_dot + n_below : (uint32_t)(A0 >> hl & 1ull) + 2u * (uint32_t)(A1 >> hl & 1ull) + (n_below - 1u - (uint32_t)hl);   // (4 = 1 mod 3)
            };
            uint32_t r = dot_in(lt, (uint32_t)lane) % 3u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (DOT >> k & 1u) { if (++r == 3u) { ++a_ell; r = 0; } }
                else r = 0;
            }
            c_dot = (uint32_t)__builtin_amdgcn_readlane((int)r, WAVE - 1);
            // words that hold a letter, counted at their last byte.  A lane's letters behind its last non-word byte
            uint32_t tl = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) tl = (Wn >> k & 1u) ? tl | (LET >> k & 1u) : 0;
            const uint64_t NALL = wballot(Wn != 0xFu), TL = wballot(tl != 0);
            auto al_in = [&](uint64_t below) -> uint32_t {
                uint64_t bt;
                const int hl = qz_last(NALL, below, bt);
                return hl < 0 ? (c_al | (uint32_t)((TL & bt) != 0)) : ((uint32_t)(TL >> hl & 1ull) | (uint32_t)((TL & bt) != 0));
            };
            uint32_t al = al_in(lt);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (Wn >> k & 1u) {
                    if (ST >> k & 1u) al = 0;
                    al |= LET >> k & 1u;
                    if (LB >> k & 1u) a_alpha += al;
                }
            }
            c_al = al_in(~0ull);
        } else {
            // F and the characters and heads in front of the lane
            uint32_t s1 = 0, s2 = 0;
            {
                uint32_t q1 = r1, q2 = r2;
#pragma unroll
                for (int k = 0; k < 4; ++k) { s1 += (B(k) + 1u) * q1; s2 += (B(k) + 1u) * q2; q1 *= QZ_R1; q2 *= QZ_R2; }
            }
            uint32_t t1, t2, tc;
            const uint32_t cnt = (uint32_t)__popc(CS) | (uint32_t)__popc(HL) << 12 | (uint32_t)__popc(HP) << 22;
            uint32_t f1 = c_f1 + qz_scan(s1, t1) - s1, f2 = c_f2 + qz_scan(s2, t2) - s2;
            const uint32_t ex = qz_scan(cnt, tc) - cnt;
            uint32_t ch = c_ch + (ex & 0xFFFu), kl = c_nl + (ex >> 12 & 0x3FFu), kp = c_np + (ex >> 22);
            // the lane's end half at its last word byte
            uint32_t we = 0, wf1 = 0, wf2 = 0, wc = 0;
            {
                uint32_t x1 = f1, x2 = f2, xc = ch, q1 = r1, q2 = r2;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    x1 += (B(k) + 1u) * q1; x2 += (B(k) + 1u) * q2; xc += CS >> k & 1u; q1 *= QZ_R1; q2 *= QZ_R2;
                    if (Wn >> k & 1u) { we = (uint32_t)i + k + 1u; wf1 = x1; wf2 = x2; wc = xc; }
                }
            }
            // ... and the one in front of the lane: the highest lower lane with a word byte, else the trip's carry
            uint64_t bt;
            const int hl = qz_last(HASW, lt, bt);
            const int src = hl < 0 ? lane : hl;
            uint32_t pe = (uint32_t)__shfl((int)we, src, WAVE), pf1 = (uint32_t)__shfl((int)wf1, src, WAVE),
                     pf2 = (uint32_t)__shfl((int)wf2, src, WAVE), pc = (uint32_t)__shfl((int)wc, src, WAVE);
            if (hl < 0) { pe = c_we; pf1 = c_wf1; pf2 = c_wf2; pc = c_wc; }
            uint32_t x1 = f1, x2 = f2, xc = ch, q1 = r1, q2 = r2, j1 = i1, j2 = i2, ss = seen;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (HL >> k & 1u) {
                    const uint32_t ql = lbase + kl;
                    if (GZ_CHK(701, ql, A.n_lines)) {
                        A.sp_start[ql] = (uint32_t)i + k; A.sp_cs[ql] = xc; A.sp_fs1[ql] = x1; A.sp_fs2[ql] = x2; A.sp_i1[ql] = j1; A.sp_i2[ql] = j2;
                        A.sp_doc[ql] = (uint32_t)d;
                        if (ss) { A.sp_end[ql - 1] = pe; A.sp_ce[ql - 1] = pc; A.sp_fe1[ql - 1] = pf1; A.sp_fe2[ql - 1] = pf2; }
                    }
                    ++kl;
                    if (HP >> k & 1u) {
                        const uint32_t qp = pbase + kp;
                        if (GZ_CHK(702, qp, A.n_spans)) {
                            A.sp_start[qp] = (uint32_t)i + k; A.sp_cs[qp] = xc; A.sp_fs1[qp] = x1; A.sp_fs2[qp] = x2; A.sp_i1[qp] = j1; A.sp_i2[qp] = j2;
                            A.sp_doc[qp] = (uint32_t)d;
                            if (ss) { A.sp_end[qp - 1] = pe; A.sp_ce[qp - 1] = pc; A.sp_fe1[qp - 1] = pf1; A.sp_fe2[qp - 1] = pf2; }
                        }
                        ++kp;
                    }
                }
                x1 += (B(k) + 1u) * q1; x2 += (B(k) + 1u) * q2; xc += CS >> k & 1u; q1 *= QZ_R1; q2 *= QZ_R2; j1 *= QZ_I1; j2 *= QZ_I2;
                if (Wn >> k & 1u) { ss = 1; pe = (uint32_t)i + k + 1u; pf1 = x1; pf2 = x2; pc = xc; }
            }
            // behind the trip
            c_f1 += t1; c_f2 += t2; c_ch += tc & 0xFFFu; c_nl += tc >> 12 & 0x3FFu; c_np += tc >> 22;
            c_we = (uint32_t)__builtin_amdgcn_readlane((int)pe, WAVE - 1); c_wf1 = (uint32_t)__builtin_amdgcn_readlane((int)pf1, WAVE - 1);
            c_wf2 = (uint32_t)__builtin_amdgcn_readlane((int)pf2, WAVE - 1); c_wc = (uint32_t)__builtin_amdgcn_readlane((int)pc, WAVE - 1);
            constexpr uint32_t RT1 = qz_pow32(QZ_R1, QZ_TRIP), RT2 = qz_pow32(QZ_R2, QZ_TRIP), IT1 = qz_pow32(QZ_I1, QZ_TRIP), IT2 = qz_pow32(QZ_I2, QZ_TRIP);
            r1 *= RT1; r2 *= RT2; i1 *= IT1; i2 *= IT2;
        }
        gap_in(~0ull, c_g, c_e, c_seen);
    }
    if (WRITE) {
        if (lane == 0 && c_seen) {                                        // the last line and the last paragraph end at the last word byte
            const uint32_t ql = lbase + c_nl - 1u, qp = pbase + c_np - 1u;
            if (GZ_CHK(703, ql, A.n_lines)) { A.sp_end[ql] = c_we; A.sp_ce[ql] = c_wc; A.sp_fe1[ql] = c_wf1; A.sp_fe2[ql] = c_wf2; }
            if (GZ_CHK(704, qp, A.n_spans)) { A.sp_end[qp] = c_we; A.sp_ce[qp] = c_wc; A.sp_fe1[qp] = c_wf1; A.sp_fe2[qp] = c_wf2; }
        }
        return;
    }
    uint32_t* const acc[10] = {&a_chars, &a_words, &a_wchars, &a_alpha, &a_hash, &a_ell, &a_lines, &a_bul, &a_elll, &a_paras};
    uint32_t tot[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) tot[k] = qz_wave_sum(*acc[k]);
    if (lane != 0) return;
    tot[8] += c_seen ? c_e : 0u;                                          // the last line's ellipsis
    A.lcnt[d] = tot[6]; A.pcnt[d] = tot[9];
    atomicAdd(&A.ctl[GZ_QC_LINES], (unsigned long long)tot[6]);
    atomicAdd(&A.ctl[GZ_QC_PARAS], (unsigned long long)tot[9]);
    constexpr int row[10] = {GZ_Q_N_CHARS, GZ_Q_N_WORDS, GZ_Q_WORD_CHARS, GZ_Q_N_ALPHA_WORDS, GZ_Q_N_HASH, GZ_Q_N_ELLIPSIS, GZ_Q_N_LINES,
                             GZ_Q_N_BULLET_LINES, GZ_Q_N_ELLIPSIS_LINES, GZ_Q_N_PARAGRAPHS};
#pragma unroll
    for (int k = 0; k < 10; ++k) A.wsig[(int64_t)row[k] * A.n_docs + d] = (int32_t)tot[k];
}

__device__ __forceinline__ bool qz_is_line(const GzQualityArgs& A, uint32_t q) { return (int64_t)q < A.n_lines; }
__device__ __forceinline__ const uint8_t* qz_bytes(const GzQualityArgs& A, uint32_t q) { return A.text + A.off[A.sp_doc[q]] + A.sp_start[q]; }

__device__ __forceinline__ unsigned long long qz_hash(const GzQualityArgs& A, uint32_t q)
{
    const uint32_t x1 = (A.sp_fe1[q] - A.sp_fs1[q]) * A.sp_i1[q], x2 = (A.sp_fe2[q] - A.sp_fs2[q]) * A.sp_i2[q];
    const uint32_t len = A.sp_end[q] - A.sp_start[q], chars = A.sp_ce[q] - A.sp_cs[q];
    unsigned long long h = bm_mix64((unsigned long long)x1 | (unsigned long long)x2 << 32);
    h = bm_mix64(h ^ ((unsigned long long)len << 32 | chars));
    h = bm_mix64(h ^ ((unsigned long long)A.sp_doc[q] << 1 | (unsigned long long)qz_is_line(A, q)));
    return h & A.hmask;
}

// kind, document and length of spans q and o agree (their bytes are compared next)
__device__ __forceinline__ bool qz_alike(const GzQualityArgs& A, uint32_t q, uint32_t o)
{
    return qz_is_line(A, q) == qz_is_line(A, o) && A.sp_doc[q] == A.sp_doc[o] && A.sp_end[q] - A.sp_start[q] == A.sp_end[o] - A.sp_start[o];
}

// n bytes at a and b are equal: dwords where both are aligned alike, bytes in front, behind, and otherwise
__device__ __forceinline__ bool qz_equal(const uint8_t* a, const uint8_t* b, uint32_t n)
{
    uint32_t k = 0;
    if ((((uintptr_t)a ^ (uintptr_t)b) & 3u) == 0) {
        for (; k < n && ((uintptr_t)(a + k) & 3u); ++k) if (a[k] != b[k]) return false;
        for (; k + 4 <= n; k += 4) if (*reinterpret_cast<const uint32_t*>(a + k) != *reinterpret_cast<const uint32_t*>(b + k)) return false;
    }
    for (; k < n; ++k) if (a[k] != b[k]) return false;
    return true;
}

// ... by a whole wave: every lane gets the answer
__device__ __forceinline__ bool qz_equal_wave(const uint8_t* a, const uint8_t* b, uint32_t n)
{
    const int lane = lane_id();
    if ((((uintptr_t)a ^ (uintptr_t)b) & 3u) == 0) {
        const uint32_t head = (uint32_t)(-(intptr_t)a & 3) < n ? (uint32_t)(-(intptr_t)a & 3) : n, words = (n - head) / 4;
        bool diff = false;
        for (uint32_t k = lane; k < head; k += WAVE) diff |= a[k] != b[k];
        for (uint32_t k = head + 4 * words + lane; k < n; k += WAVE) diff |= a[k] != b[k];
        if (wballot(diff)) return false;
        const uint32_t* const wa = reinterpret_cast<const uint32_t*>(a + head);
        const uint32_t* const wb = reinterpret_cast<const uint32_t*>(b + head);
        for (uint32_t k0 = 0; k0 < words; k0 += WAVE) {
            const uint32_t k = k0 + lane;
            if (wballot(k < words && wa[k] != wb[k])) return false;
        }
        return true;
    }
    for (uint32_t k0 = 0; k0 < n; k0 += WAVE) {
        const uint32_t k = k0 + lane;
        if (wballot(k < n && a[k] != b[k])) return false;
    }
    return true;
}

}  // namespace

template <bool WRITE>
__global__ __launch_bounds__(WAVE * QZ_WPB) void gz_quality_walk_kernel(GzQualityArgs A)
{
    const int64_t d = (int64_t)blockIdx.x * QZ_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= A.n_docs) return;
    const int64_t o = A.off[d];
    int64_t len = A.off[d + 1] - o;
    if (!WRITE && lane_id() == 0) {                                       // what the host reads back: the extent, and the documents it refuses
        if (d == 0) { A.ctl[GZ_QC_OFF0] = (unsigned long long)o; A.ctl[GZ_QC_OFFN] = (unsigned long long)A.off[A.n_docs]; }
        if (o < 0 || len < 0) atomicOr(&A.ctl[GZ_QC_FLAGS], 1ull);
        else if (len >= ((int64_t)1 << 31)) atomicOr(&A.ctl[GZ_QC_FLAGS], 2ull);
    }
    if (o < 0 || len < 0 || len >= ((int64_t)1 << 31)) len = 0;           // (nothing of such a call reaches the caller)
    qz_walk<WRITE>(A, d, A.text + o, len);
}

__global__ __launch_bounds__(256) void gz_quality_insert_kernel(GzQualityArgs A)
{
    const int64_t q64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q64 >= A.n_spans) return;
    const uint32_t q = (uint32_t)q64, len = A.sp_end[q] - A.sp_start[q];
    if (len > QZ_LONG) {                                                  // a wave per span does these
        A.long_list[atomicAdd(&A.ctl[GZ_QC_LONG], 1ull)] = q;
        return;
    }
    const unsigned long long h = qz_hash(A, q);
    const unsigned long long mine = ((h >> 32) | 0x80000000ull) << 32 | q;
    const uint8_t* const mb = qz_bytes(A, q);
    uint64_t s = h & A.mask;
    for (;;) {
        const unsigned long long cur = atomicCAS(&A.table[s], 0ull, mine);
        if (cur == 0) break;
        if ((cur >> 32) == (mine >> 32)) {
            const uint32_t o = (uint32_t)cur;
            if (o == q || (qz_alike(A, q, o) && qz_equal(mb, qz_bytes(A, o), len))) { atomicMin(&A.table[s], mine); break; }
        }
        s = (s + 1) & A.mask;
    }
    A.sp_slot[q] = (uint32_t)s;
}

__global__ __launch_bounds__(WAVE * QZ_WPB) void gz_quality_insert_long_kernel(GzQualityArgs A)
{
    const uint32_t w = blockIdx.x * QZ_WPB + threadIdx.x / WAVE;
    if (w >= A.ctl[GZ_QC_LONG]) return;
    const int lane = lane_id();
    const uint32_t q = A.long_list[w], len = A.sp_end[q] - A.sp_start[q];
    const unsigned long long h = qz_hash(A, q);
    const unsigned long long mine = ((h >> 32) | 0x80000000ull) << 32 | q;
    const uint8_t* const mb = qz_bytes(A, q);
    uint64_t s = h & A.mask;
    for (;;) {
        unsigned long long cur = 0;
        if (lane == 0) cur = atomicCAS(&A.table[s], 0ull, mine);
        cur = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)cur) |
              (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(cur >> 32)) << 32;
        if (cur == 0) break;
        if ((cur >> 32) == (mine >> 32)) {
            const uint32_t o = (uint32_t)cur;
            if (o == q || (qz_alike(A, q, o) && qz_equal_wave(mb, qz_bytes(A, o), len))) {
                if (lane == 0) atomicMin(&A.table[s], mine);
                break;
            }
        }
        s = (s + 1) & A.mask;
    }
    if (lane == 0) A.sp_slot[q] = (uint32_t)s;
}

__global__ __launch_bounds__(WAVE * QZ_WPB) void gz_quality_resolve_kernel(GzQualityArgs A)
{
    const int64_t d = (int64_t)blockIdx.x * QZ_WPB + (int64_t)(threadIdx.x / WAVE);
    if (d >= A.n_docs) return;
    const int lane = lane_id();
    uint32_t dup[2] = {0, 0}, dch[2] = {0, 0};
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
        const uint32_t* const off = kind ? A.poff : A.loff;
        const uint32_t lo = off[d], n = off[d + 1] - lo, base = (kind ? (uint32_t)A.n_lines : 0u) + lo;
        int64_t* const span = kind ? A.para_span : A.line_span;
        int32_t* const first = kind ? A.para_first : A.line_first;
        for (uint32_t k = lane; k < n; k += WAVE) {
            const uint32_t q = base + k, f = (uint32_t)A.table[A.sp_slot[q]];
            if (f != q) { ++dup[kind]; dch[kind] += A.sp_ce[q] - A.sp_cs[q]; }
            if (first) first[lo + k] = (int32_t)(f - base);
            if (span) { span[2 * (int64_t)(lo + k)] = A.sp_start[q]; span[2 * (int64_t)(lo + k) + 1] = A.sp_end[q]; }
        }
        dup[kind] = qz_wave_sum(dup[kind]); dch[kind] = qz_wave_sum(dch[kind]);
    }
    if (lane >= GZ_Q_SIGNALS || !A.signals) return;                      // a lane a row: pass A's ten from the workspace beside the four of this kernel
    const int32_t v = lane == GZ_Q_DUP_LINES ? (int32_t)dup[0] : lane == GZ_Q_DUP_LINE_CHARS ? (int32_t)dch[0]
                    : lane == GZ_Q_DUP_PARAGRAPHS ? (int32_t)dup[1] : lane == GZ_Q_DUP_PARAGRAPH_CHARS ? (int32_t)dch[1]
                    : A.wsig[(int64_t)lane * A.n_docs + d];
    A.signals[(int64_t)lane * A.n_docs + d] = v;
}

// pass A: the text-only signals into wsig, lcnt / pcnt, and the control words (cleared by the caller)
void gz_launch_quality_count(const GzQualityArgs& A, hipStream_t s)
{
    if (A.n_docs > 0) hipLaunchKernelGGL(gz_quality_walk_kernel<false>, dim3((unsigned)((A.n_docs + QZ_WPB - 1) / QZ_WPB)), dim3(WAVE * QZ_WPB), 0, s, A);
}

// pass B, the table and the resolve: loff / poff scanned, n_lines / n_spans read back, the table and n_long cleared by the caller
void gz_launch_quality_spans(const GzQualityArgs& A, int64_t long_max, hipStream_t s)
{
    if (A.n_docs <= 0) return;
    const dim3 docs((unsigned)((A.n_docs + QZ_WPB - 1) / QZ_WPB)), wpb(WAVE * QZ_WPB);
    if (A.n_spans > 0) {
        hipLaunchKernelGGL(gz_quality_walk_kernel<true>, docs, wpb, 0, s, A);
        hipLaunchKernelGGL(gz_quality_insert_kernel, dim3((unsigned)((A.n_spans + 255) / 256)), dim3(256), 0, s, A);
        if (long_max > 0) hipLaunchKernelGGL(gz_quality_insert_long_kernel, dim3((unsigned)((long_max + QZ_WPB - 1) / QZ_WPB)), wpb, 0, s, A);
    }
    hipLaunchKernelGGL(gz_quality_resolve_kernel, docs, wpb, 0, s, A);
}
