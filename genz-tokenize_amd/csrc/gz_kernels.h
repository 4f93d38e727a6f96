// Kernel argument blocks and launchers (gz_kernels.hip) used by the C ABI (gz_api.cpp).
#pragma once
#include "gz_common.h"
#include "gz_packfit.h"
#include <hip/hip_runtime.h>

constexpr int GZ_WAVES_PER_BLOCK = 2;
constexpr int GZ_MAX_DOCS_PER_WAVE = 16;  // a wave owns up to this many consecutive documents
constexpr int32_t GZ_NONE_ = -1;        // == GZ_NONE of the public header

// max_len / padding / truncation of Tokenize.__call__ (tokenize.py:184-190)
struct GzShape {
    int32_t max_len;      // meaningful only when pad_mode
    int32_t pad_mode;     // `max_len is not None and padding` (tokenize.py:247, :256)
    int32_t truncation;
};

struct GzFinalizeArgs {
    const int64_t* text_off; const int64_t* pair_off;
    int64_t n_docs;
    GzShape S;
    const int32_t* raw; const int32_t* n_raw;
    int64_t* row_off;     // [n_docs+1] (written by the scan that precedes the finalize kernel)
    int64_t capacity;
    int32_t* ids; int32_t* mask; int32_t* n_real;
    int32_t* error_flag;  // set to 1 when row_off[n_docs] > capacity
};

struct GzPairArgs {
    int64_t n_docs;
    GzShape S;            // dense when row_off == nullptr (rows of max_len)
    const int64_t* row_off; int64_t capacity;
    const int32_t* ids;
    int32_t* seq; int32_t* tt; int32_t* pair_len; int32_t* status;
};

// ---- multi-kernel pipeline (gz_pipeline.inc) ---------------------------------------------------------------------
struct GzTextBufs {              // one text (A or B) of a batch and its per-call workspace
    const uint8_t* tb;           // first byte of the batch (text + off[0])
    const int64_t* off;          // [n_docs+1] absolute offsets
    int64_t B;                   // bytes of the batch
    int64_t nblk;                // 4-KiB blocks covering positions 0 .. B
    uint16_t* brk;               // bitmaps, 16 bits per 16 bytes: document starts / word starts / word ends
    uint16_t* st;
    uint16_t* en;
    uint32_t* blkcnt;            // [nblk+1] words per block, then (scanned in place) index of each block's first word
    uint32_t* docw0;             // [n_docs+1] index of each document's first word
    uint32_t* wtok;              // [words] id, or a merged word's record (far: MISS | token count; near: count and place in one word)
    uint32_t* waux;              // [words] far records only: where the word's tokens are (mtok[waux ...]; wide / long words: their byte offset)
    uint4* mlist;                // [words] the misses of block b, compact, at mlist[blkcnt[b] ...]: {word index, byte offset, pending record, 0}
    uint32_t* blkmiss;           // [nblk+1] number of misses per block; scanned in place before the merge pre-pass ([nblk] = total)
    uint32_t* grpblk;            // [words/64 + 2] block that holds miss number 64 g (written by the scan)
    uint32_t* tcnt;              // [words/1024 + 8] per 3 072-miss tile of mq: records the merge kernel takes | its chunks of 64 with a word of > 8 symbols << 16 (gz_mpre_kernel)
    int64_t wmax;                // upper bound of the number of words (sizes of the per-word arrays)
    uint32_t* ctl;               // [64] zeroed per call: [0] words for gz_long_kernel, [1] unused, [2] [3] ticket counters of the
                                 // chained scans, [4] cursor of the compact token area; wlist == ctl + 64
    uint4* mq;                   // [words] the misses, tile by tile (1 024) sorted by symbol count: {word index, byte offset, record, 0}
    uint64_t* lookback;          // [nblk / 4 + 2] chained-scan words of gz_scan32m_kernel {status:2, call:30, value:32}; never cleared
    uint32_t epoch;              // call number written into / expected in the chained-scan words
    uint32_t near_lim;           // places of the compact token area below this get near records (2^25; switch near_limit: smaller, for tests)
    uint32_t* blklong;           // [nblk] block holds a word for gz_long_kernel (zeroed per call)
    uint32_t* wlist;             // [0] count, then the words (indices) that need 32 or 64 lanes (zeroed count per call); from the END of the
                                 // array down (wlist[wmax + 6 - k]): the words gz_long_kernel takes
    uint16_t* tilecnt;           // [4 * nblk] word starts of the block that lie before each of its four 1-KiB tiles
    int32_t* mtok;               // [2 (B + 32)]: [0, B + 32) tokens of wide / long words, at the word's byte offset; from B + 32 on the
                                 // compact token area of gz_miss2_kernel (places handed out by gz_mpre_kernel, cursor: ctl[4])
};

struct GzAsmArgs {
    GzTextBufs X[2];
    int32_t n_texts;             // 1, or 2 in pair mode
    int64_t n_docs;
    int32_t dense, max_len;
    int32_t* ids; int32_t* mask; int32_t* raw; int32_t* n_real;
    int32_t docs_per_wave;
    // gz_rowsr_kernel (single texts without padding): the rows' places (write pass), the caller's capacity and the flag raised beyond it
    const int64_t* row_off; int64_t capacity; int32_t* error_flag;
};

// BPE-dropout (gz_dropout.inc): what the merge stage of a dropout call draws from
struct GzDrop {
    uint64_t thr;                // a candidate merge is skipped when its draw is below this (0 .. 2^32: 2^32 drops everything)
    uint64_t seed;
    int64_t doc0;                // global index D of the first document of the text the kernels see (doc_base + the sub-batch's first document)
};

// T_host: the host copy of the table descriptor (table sizes decide launch shapes)
// side / ev_fork0 / ev_fork / ev_join (may be null): a second stream on which gz_docw0_kernel runs beside the word kernel and
// the rare wide-word kernels beside the merge kernel
void gz_launch_pipeline_text(const GzOptions& O, const GzDeviceTables* T_dev, const GzDeviceTables& T_host, const GzTextBufs& X, int64_t n_docs, int use_words,
                             int32_t* long_flag /* device int, zeroed by the caller */, hipStream_t s,
                             hipStream_t side = nullptr, hipEvent_t ev_fork0 = nullptr, hipEvent_t ev_fork = nullptr, hipEvent_t ev_join = nullptr,
                             hipEvent_t ev_brk = nullptr /* non-null: X.off is readable NOW (no copy of it is queued on s): the document-start
                                                            bits are prepared on the side stream, under whatever s is still running */,
                             const GzDrop* drop = nullptr /* non-null: a BPE-dropout call -- the merge stage is gz_dropout.inc's (use_words must be 0) */);
void gz_launch_bpe_word_drop(const GzDeviceTables* T_dev, const uint8_t* word, int64_t nbytes, uint32_t* arena, int32_t* out, int32_t cap, int32_t* n_out,
                             const GzDrop& R, uint32_t word_index, hipStream_t s);
void gz_launch_pick(const int64_t* off, const int64_t* off2, int64_t n_docs, int nsub, int64_t* out /* 2*(nsub+1) */, hipStream_t s);
void gz_launch_row_offsets(const int32_t* n_real, int64_t n_rows, uint32_t* off, hipStream_t s);
// first (may be null): receives where each row's entries start (= off[r]): the second array of an exchange block
void gz_launch_compact(const int32_t* rows, const uint32_t* off, int64_t n_rows, int32_t row_len, void* out, int bits /* 32 | 16 */, uint32_t* first,
                       hipStream_t s);
// row r: n_real[r] entries from first[r] on (scanned offsets, or a block's own array: the rows then lie in any order)
void gz_launch_expand(const void* compact, int bits, const uint32_t* first, const int32_t* n_real, int64_t n_rows, int32_t row_len, int32_t pad_id,
                      int32_t* ids, int32_t* mask, uint32_t total /* entries the compact array holds */, int32_t* bad /* set when a row does not fit */, hipStream_t s);
void gz_launch_assemble(const GzOptions& O, const GzDeviceTables* T_dev, const GzAsmArgs& A, hipStream_t s);
void gz_launch_rows_ragged(const GzDeviceTables* T_dev, const GzAsmArgs& A, int pass, int64_t text_bytes, hipStream_t s);
// small batches, one launch (gz_small.inc): G documents per workgroup, G <= GZ_SMALL_DOCS_PER_WG and every group of G
// documents (A and B texts together) <= GZ_SMALL_DOC_BYTES.  poff == nullptr: single texts.  dense: rows of max_len into
// ids / mask; else: unpadded rows into the raw area `ids` (document d at (bytes before d) + 2 d per text) and their
// lengths into n_real.  arena: [text bytes + pair bytes + 32] words of scratch for very long words.
constexpr int GZ_SMALL_DOC_BYTES = 4096, GZ_SMALL_DOCS_PER_WG = 64;
// layout 2 (rows without padding, ONE workgroup: (n_docs + G - 1) / G == 1): the kernel also makes row_off[n_docs + 1] and writes
// ids / mask at their final places (no rowlen / scan / finalize behind it); beyond `capacity` entries: *error_flag = 1, nothing written
void gz_launch_small(const GzDeviceTables* T_dev, const uint8_t* text0, const int64_t* off, int64_t base, const uint8_t* pair0, const int64_t* poff,
                     int64_t pbase, int64_t n_docs, int G, int layout /* 1 dense, 0 raw area, 2 placed */, int max_len, int use_words, int32_t* ids,
                     int32_t* mask, int32_t* n_real, int32_t* arena, int64_t* row_off, int64_t capacity, int32_t* error_flag, hipStream_t s);

void gz_launch_rowscan(const GzFinalizeArgs& F, int64_t* row_len_tmp, hipStream_t s);
void gz_launch_finalize(const GzDeviceTables& T, const GzFinalizeArgs& F, hipStream_t s);
void gz_launch_pair(const GzDeviceTables& T, const GzPairArgs& P, hipStream_t s);
void gz_launch_bpe_word(const GzDeviceTables* T_dev, const uint8_t* word, int64_t nbytes, uint32_t* arena,
                        int32_t* out, int32_t cap, int32_t* n_out, hipStream_t s);
// batch decode: out == nullptr -> row_bytes[n_rows] + out_off[n_rows + 1] (exclusive scan); else write the text
void gz_launch_decode(const GzDecTable& D, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int64_t* row_bytes,
                      int64_t* out_off, uint8_t* out, int64_t capacity, hipStream_t s);

// overlapping max_len windows over ragged rows (gz_window.inc).  Count pass: n_win[n_rows] and their exclusive scan win_off[n_rows + 1].
// Fill pass: the n_win = win_off[n_rows] window rows; out_mask, win_doc, win_start, win_n_real may be null.
struct GzWinArgs {
    const int32_t* ids; const int64_t* row_off; int64_t n_rows;      // row r = ids[row_off[r] .. row_off[r + 1]) (absolute offsets)
    const int64_t* win_off; int64_t n_win;
    int32_t max_len, room, step, skip_front, skip_back;             // room = max_len - 2, step = room - stride
    int32_t bos_id, eos_id, pad_id;
    int32_t* out_ids; int32_t* out_mask;                            // [n_win, max_len]
    int32_t* win_doc; int32_t* win_start; int32_t* win_n_real;      // [n_win]
};
void gz_launch_window_count(const int64_t* row_off, int64_t n_rows, int32_t room, int32_t step, int32_t skip, int64_t* n_win, int64_t* win_off,
                            hipStream_t s);
void gz_launch_window_fill(const GzWinArgs& A, hipStream_t s);

// question-context windows with answer positions (gz_pairwin.inc).  Count pass: n_win[n_rows], pair_q[n_rows] and the exclusive scan
// win_off[n_rows + 1].  Fill pass: the n_win = win_off[n_rows] window rows; every output but out_ids may be null.
struct GzPairWinArgs {
    const int32_t* q_ids; const int64_t* q_off; int64_t n_q;        // question row i = q_ids[q_off[i] .. q_off[i + 1]) (absolute offsets)
    const int32_t* c_ids; const int64_t* c_off; int64_t n_rows;     // context row r likewise: pair r
    const int32_t* q_row;                                           // [n_rows] the question of pair r; null: question r
    const int32_t* ans;                                             // [n_rows, 2] body positions [a0, a1); may be null
    const int64_t* win_off; int64_t n_win;
    int32_t* pair_q;                                                // [n_rows] q of every pair: written by the count pass, read by the fill pass
    int32_t max_len, stride, max_q, skip_front, skip_back;
    int32_t bos_id, eos_id, pad_id;
    int32_t* out_ids; int32_t* out_mask; int32_t* out_type;         // [n_win, max_len]
    int32_t* win_pair; int32_t* win_start; int32_t* win_n_real; int32_t* win_q_len;      // [n_win]
    int32_t* start_pos; int32_t* end_pos; int32_t* has_answer;      // [n_win]; written where ans is given
};
void gz_launch_pairwin_count(const GzPairWinArgs& A, int64_t* n_win, int64_t* win_off, hipStream_t s);
void gz_launch_pairwin_fill(const GzPairWinArgs& A, hipStream_t s);
// word ranges -> body-token ranges (gz_pairwin.inc): cnt64 [n_words + 1] and tok_off [n_words + 2] are scratch
struct GzSpanTokArgs {
    const int64_t* word_off; int64_t n_docs, n_words;               // absolute; n_words = word_off[n_docs] - word_off[0]
    const int32_t* mark_words; const int64_t* mark_off; int64_t n_marks;      // mark_words [n_marks, 2] from 0; mark_off absolute
    const int64_t* tok_off;                                         // [n_words + 1] exclusive scan of the counts, from 0
    int32_t* out;                                                   // [n_marks, 2] from 0
};
void gz_launch_span_tokens(GzSpanTokArgs A, const int32_t* counts, int64_t* cnt64, int64_t* tok_off, hipStream_t s);

// short documents packed into rows of max_len (gz_packrows.inc).  Maps: doc_len, seg_off (its scan), the row heads row by row
// (pack_off[0 .. R], R -> *total), doc_row, doc_col.  Fill: the R rows; out_mask, out_seg, out_pos may be null.
constexpr int GZ_PACK_TILE = 1024;      // documents per tile of the break chain
constexpr int GZ_PACK_GROUP = 16;       // tiles per group
struct GzPackArgs {
    const int32_t* ids; const int64_t* row_off; int64_t n_rows;     // row r = ids[row_off[r] .. row_off[r + 1]) (absolute offsets); n_rows < 2^31 - 4096
    int32_t max_len, skip_front, skip_back;
    int32_t bos_id, eos_id, pad_id;
    int32_t* doc_row; int32_t* doc_col; int32_t* doc_len;           // [n_rows]; doc_len may be null
    int64_t* pack_off; int64_t* seg_off;                            // [n_rows + 1] (R + 1 entries of pack_off are written)
    // workspace of the maps: len64 [n_rows + 1], jc [2 n_rows], nxt [n_rows], jc2 [2 * groups * gz_pack_entries(max_len)], tile [2 * tiles], total [1]
    int64_t* len64; int32_t* jc; int32_t* nxt; int32_t* jc2; int32_t* tile; int64_t* total;
    int64_t capacity;                                               // rows the cell arrays hold: the fill writes nothing when *total exceeds it
    int32_t* out_ids; int32_t* out_mask; int32_t* out_seg; int32_t* out_pos;     // [*total, max_len]
    const int32_t* row_docs; int64_t fit_rows;                      // best-fit order only (gz_packfit.inc): the packed order [n_rows] and R
};
inline int64_t gz_pack_tiles(int64_t n_rows) { return (n_rows + GZ_PACK_TILE - 1) / GZ_PACK_TILE; }
inline int64_t gz_pack_groups(int64_t n_rows) { return (gz_pack_tiles(n_rows) + GZ_PACK_GROUP - 1) / GZ_PACK_GROUP; }
inline int32_t gz_pack_entries(int32_t max_len)                     // where a chain can enter a group: its first max_len / 2 documents
{
    return max_len / 2 < GZ_PACK_TILE * GZ_PACK_GROUP ? max_len / 2 : GZ_PACK_TILE * GZ_PACK_GROUP;
}
void gz_launch_pack_maps(const GzPackArgs& A, bool with_col /* false: a fill follows and writes doc_col */, hipStream_t s);
void gz_launch_pack_col(const GzPackArgs& A, hipStream_t s);
void gz_launch_pack_fill(const GzPackArgs& A, hipStream_t s);     // R = *A.total, read on the device

// best-fit packing (gz_packfit.inc; the rule and the host plan: gz_packfit.h).  P holds the batch, the cell arrays and the maps
// (doc_row, doc_col, doc_len and pack_off are never null here; seg_off may be; P.len64 [n_rows + 1] is scratch; the break chain's
// workspace is not used).  hist: len, rank and the column scan -> rank, tab, hist.  maps, once the plan is on the device: pack_off,
// doc_row, doc_col, row_docs, seg_off.  fill: the R rows.
constexpr int GZ_FIT_TILE = 1024;       // documents per tile of the rank pass
constexpr int GZ_FIT_MAX_LEN = 4096;    // = GZ_PACK_FIT_MAX_LEN: the histogram, the tiles' length tables and the plan are sized by max_len
struct GzFitArgs {
    GzPackArgs P;                                                   // (P.row_docs and P.fit_rows are set by the fill's launcher)
    int32_t* row_docs;                                              // [n_rows]
    int32_t* rank; int32_t* tab; int32_t* hist;                     // [n_rows], [gz_fit_tiles * (max_len + 1)], [max_len + 1]
    const GzFitEvent* ev; const int32_t* ev_off; const GzFitSeg* seg; int32_t n_seg;       // the plan: ev_off [max_len + 2], seg with its closing entry
    int64_t R;
};
inline int64_t gz_fit_tiles(int64_t n_rows) { return (n_rows + GZ_FIT_TILE - 1) / GZ_FIT_TILE; }
void gz_launch_packfit_hist(const GzFitArgs& F, hipStream_t s);
void gz_launch_packfit_maps(const GzFitArgs& F, hipStream_t s);
void gz_launch_packfit_fill(const GzFitArgs& F, hipStream_t s);

// masked-LM inputs and labels over dense rows (gz_mask.inc): one launch; ids, out_ids and labels are [n_rows, row_len] and disjoint
constexpr int GZ_MASK_LDS_MAX_BYTES = 48 * 1024;      // the continuation bitmap goes to LDS up to this size (393 216 ids)
struct GzMaskArgs {
    const int32_t* ids; int64_t n_rows; int32_t row_len;            // n_rows >= 1, row_len >= 1
    int64_t row_base;                                               // the global index of cell (r, c) is (row_base + r) * row_len + c, < 2^63
    uint32_t key0, key1;                                            // the seed's low and high word
    uint64_t t_sel, t1, t2;                                         // thresholds in [0, 2^32], t1 <= t2 (2^32: always)
    int32_t rand_lo; uint32_t rand_span;                            // random replacements: rand_lo + mulhi32(x2, rand_span), rand_span = rand_hi - rand_lo >= 1
    int32_t mask_id, ignore_index, whole_word;
    int32_t pad_id, bos_id, eos_id;                                 // protected beside mask_id
    const uint32_t* cont_bits; int32_t n_ids;                       // the decoder snapshot's continuation bitmap: bit id of word id / 32 set when the word ends in "@@"
    int32_t bits_in_lds;                                            // 1: the LDS form is wanted (the launcher takes it when the bitmap fits: (n_ids + 31) / 32 words of dynamic LDS)
    int32_t* out_ids; int32_t* labels;
    int32_t* n_chosen;                                              // [n_rows], may be null
    int32_t rows_per_wave;                                          // set by the launcher
};
void gz_launch_mask(GzMaskArgs A, hipStream_t s);

// span-corruption inputs and targets over dense rows (gz_infill.inc): one launch; ids, out_ids and out_mask are [n_rows, row_len],
// labels and dec_ids [n_rows, dec_width], the three counts [n_rows]; all disjoint
struct GzInfillArgs {
    const int32_t* ids; int64_t n_rows; int32_t row_len;            // n_rows >= 1, row_len >= 1
    int64_t row_base;                                               // the global index of cell (r, c) is (row_base + r) * row_len + c, < 2^63
    uint32_t key0, key1;                                            // the seed's low and high word
    uint64_t t_start;                                               // a span begins at a start whose x0 is below it; in [0, 2^32] (2^32: always)
    uint64_t len_t[15]; int32_t n_len;                              // len = 1 + #{k : x1 >= len_t[k]}; non-decreasing, in [0, 2^32]; words from n_len - 1 on hold 2^32; 1 <= n_len <= 16
    int32_t mask_id, ignore_index, whole_word, dec_width;           // dec_width >= 1
    int32_t pad_id, bos_id, eos_id;                                 // protected beside mask_id
    const uint32_t* cont_bits; int32_t n_ids;                       // the continuation bitmap of GzMaskArgs
    int32_t bits_in_lds;                                            // as in GzMaskArgs (the switch mask_lds)
    int32_t* out_ids; int32_t* labels;
    int32_t* out_mask; int32_t* dec_ids;                            // each may be null
    int32_t* enc_len; int32_t* dec_len; int32_t* n_spans;           // [n_rows], each may be null
    int32_t rows_per_wave;                                          // set by the launcher
};
void gz_launch_infill(GzInfillArgs A, hipStream_t s);

// Pieces of ragged rows (gz_pieces.inc): a row's body, the row without its skips, is cut into pieces of 4096 positions and a wave owns
// one piece; a row with fewer positions, or none, has one piece.  Positions: GZ_PIECES_SHINGLES -- runs of w ids, one run when the
// body is shorter than w and not empty (MinHash); GZ_PIECES_NGRAMS -- runs of w ids, none below w (n-gram overlap, repeats).
// The count pass: n_pieces[n_rows], their exclusive scan piece_off[n_rows + 1], rebased[n_rows + 1] = row_off - row_off[0] (may be
// null), and *totals, cleared first: n_pos = the positions of all rows (only with want_pos, which goes with GZ_PIECES_NGRAMS: only
// the n-gram calls size a table by it), too_long = 1 when a body holds 2^31 ids or more.
enum GzPieceRule { GZ_PIECES_SHINGLES, GZ_PIECES_NGRAMS };
struct GzPieceTotals { unsigned long long n_pos; uint32_t too_long, unused; };     // (unused: the clear and the copy back are 16 whole bytes)
void gz_launch_piece_count(GzPieceRule rule, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t w, int64_t* n_pieces,
                           int64_t* piece_off, int64_t* rebased, bool want_pos, GzPieceTotals* totals, hipStream_t s);

// MinHash signatures of ragged rows and near-duplicate groups from signatures (gz_minhash.inc)
struct GzMinhashArgs {
    const int32_t* ids; const int64_t* row_off; int64_t n_rows;      // row r = ids[row_off[r] .. row_off[r + 1]) (absolute offsets); bodies shorter than 2^31
    int32_t skip_front, skip_back, shingle, num_perm;               // skips 0 or 1, 1 <= shingle <= 32, 1 <= num_perm <= 256
    uint32_t seed_lo, seed_hi;
    const int64_t* piece_off; int64_t n_pieces;                     // of the count pass; n_pieces = piece_off[n_rows]
    int32_t one_each;                                               // set by the launcher: n_pieces == n_rows, piece p is row p
    uint32_t* sig;                                                  // [n_rows, num_perm]
    int32_t* n_shingles;                                            // [n_rows], may be null
};
void gz_launch_minhash_sig(GzMinhashArgs A, hipStream_t s);        // fills sig with 0xFFFFFFFF first when a row has more than one piece
struct GzMinhashGroupArgs {
    const uint32_t* sig; int64_t n_rows;                            // [n_rows, num_perm]; 1 <= n_rows < 2^31 - 4096
    int32_t num_perm, bands, min_agree;                             // bands divides num_perm, 1 <= min_agree <= num_perm
    int32_t* group;                                                 // [n_rows]: the labels, and the forest while the bands are linked
    unsigned long long* keys; uint32_t* reps; uint64_t cap;         // the table: cap = gz_minhash_cap(n_rows) slots
    uint8_t* empty;                                                 // [n_rows]
    unsigned long long* n_groups;                                   // rows with group[d] == d
};
inline uint64_t gz_minhash_cap(int64_t n_rows)                      // a power of two, at least twice the rows (and at least 64)
{
    uint64_t cap = 64;
    while (cap < 2 * (uint64_t)n_rows) cap <<= 1;
    return cap;
}
void gz_launch_minhash_groups(const GzMinhashGroupArgs& A, hipStream_t s);     // init, then per band clear / insert / link, then flatten + count

// exact token n-gram overlap against a held-out set (gz_ngram.inc); pieces of n-gram positions at the index's width
struct GzNgramArgs {
    const int32_t* ids; const int64_t* row_off; int64_t n_rows;      // the rows walked: row r = ids[row_off[r] .. row_off[r + 1]); bodies shorter than 2^31
    int32_t skip_front, skip_back, n;                               // skips 0 or 1, 1 <= n <= 32
    const int64_t* piece_off; int64_t n_pieces;                     // of the count pass; n_pieces = piece_off[n_rows]
    int32_t one_each;                                               // set by the launcher: n_pieces == n_rows, piece p is row p
    unsigned long long* table; uint64_t mask;                       // the index: slots - 1 (a power of two of slots, at least twice the positions)
    uint64_t hmask;                                                 // hash bits kept (switch ngram_hash_bits)
    const int32_t* ref_ids; const int64_t* ref_off; int64_t ref_rows;     // the index's id copy, its offsets from 0, its rows (< 2^31)
    unsigned long long* n_distinct;                                 // build: successful claims are added
    int32_t* n_grams; int32_t* n_hits; int32_t* n_covered; int32_t* first_hit; int32_t* first_ref;   // query: [n_rows], each may be null --
                                                                    // but first_hit is needed where first_ref is given
    uint8_t* covered;                                               // query: covered[k] belongs to ids[k]; may be null
};
inline uint64_t gz_ngram_slots(int64_t n_positions)                 // the smallest power of two that is at least twice the positions
{
    uint64_t cap = 1;
    while (cap < 2 * (uint64_t)n_positions) cap <<= 1;
    return cap;
}
void gz_launch_ngram_insert(GzNgramArgs A, hipStream_t s);          // into a cleared table
void gz_launch_ngram_query(GzNgramArgs A, hipStream_t s);           // presets the counts when a row has more than one piece; then resolves first_ref

// n-gram repetition inside a document (gz_repeat.inc); pieces of n-gram positions at the call's smallest width
struct GzRepeatArgs {
    const int32_t* ids; const int64_t* row_off; int64_t n_rows;      // row r = ids[row_off[r] .. row_off[r + 1]) (absolute offsets); bodies shorter than 2^31
    int64_t off0;                                                   // row_off[0]: a slot's position counts from here (fewer than 2^32 - 1 ids behind it)
    int32_t skip_front, skip_back, n, k;                            // skips 0 or 1; this launch's width, 1 <= n <= 32, and its index in the caller's list
    const int64_t* piece_off; int64_t n_pieces;                     // of the count pass; n_pieces = piece_off[n_rows]
    int32_t one_each;                                               // n_pieces == n_rows, piece p is row p
    unsigned long long* table; uint32_t* count; uint64_t mask;      // slots - 1 (a power of two of slots, at least twice the positions at the smallest width)
    uint64_t hmask;                                                 // hash bits kept (switch repeat_hash_bits)
    unsigned long long* top;                                        // [n_rows] where a row has several pieces and a top output is asked for, else null
    int32_t* n_grams; int32_t* n_distinct; int32_t* n_repeated; int32_t* n_covered; int32_t* top_count; int32_t* top_pos;   // this width's
                                                                    // [n_rows], each may be null
    uint16_t* covered;                                              // covered[i] belongs to ids[i]; may be null
};
// One width: clears the table and the counts, presets the add / max cells where a row has several pieces, inserts, queries, unpacks.
void gz_launch_repeat_width(GzRepeatArgs A, hipStream_t s);

// word spans, word ids and aligned labels (gz_align.inc)
constexpr int64_t GZ_SPAN_BLOCK = 4096;                            // bytes of packed text per block of the span kernels
inline int64_t gz_span_blocks(int64_t text_bytes) { return (text_bytes + GZ_SPAN_BLOCK - 1) / GZ_SPAN_BLOCK; }
struct GzSpanArgs {
    const uint8_t* text; const int64_t* text_off; int64_t n_docs;   // document d = text[text_off[d] .. text_off[d + 1]) (absolute offsets)
    int64_t B;                                                      // text_off[n_docs] - text_off[0]
    int32_t unit;                                                   // 0 code points, 1 bytes
    uint32_t* brk;                                                  // B / 32 + 4 words: the launcher clears them, then one bit a document start
    uint32_t* gran;                                                 // 256 * blocks words: (starts | leads << 16) before a granule, inside its block
    int64_t* blk_s; int64_t* blk_l;                                 // [blocks] starts / leads of a block
    int64_t* base_s; int64_t* base_l;                               // [blocks + 1] their exclusive scans
    int64_t* lead0;                                                 // [n_docs + 1] leads before a document's first byte
    int64_t* blk_doc;                                               // [blocks + 1] the document of a block's first byte; [blocks] = n_docs - 1
    uint32_t* too_long;                                             // set when a document holds 2^31 bytes or more (cleared first)
    int64_t* word_off;                                              // [n_docs + 1] out
    int32_t* span; int64_t n_words;                                 // write pass: [n_words, 2] out, n_words = word_off[n_docs]
};
void gz_launch_span_count(const GzSpanArgs& A, hipStream_t s);      // everything but span: word_off, lead0 and the scans the write pass reads
void gz_launch_span_write(const GzSpanArgs& A, hipStream_t s);
struct GzAlignArgs {
    const uint32_t* tok_off;                                        // [n_words + 1] exclusive scan of the piece counts, from 0, wrapping
    int32_t rows_per_block;                                         // set by the launcher
    const int64_t* word_off; int64_t n_docs, n_words;               // absolute; n_words = word_off[n_docs] - word_off[0]
    const int32_t* row_doc; const int32_t* row_start; int64_t n_rows;     // each may be null: row r is document r / start 0
    int32_t max_len;
    const int32_t* word_labels;                                     // indexed as counts (absolute); needed where labels is given
    int32_t continuation; const int32_t* cont_map; int32_t n_map; int32_t ignore_index;
    int32_t* word_ids; int32_t* labels; int32_t* n_real;            // [n_rows, max_len] x 2, [n_rows]; each may be null
};
void gz_launch_align_scan(const int32_t* counts, const int64_t* word_off, int64_t n_words, uint32_t* tok_off /* n_words + 1 */, hipStream_t s);
void gz_launch_align_rows(GzAlignArgs A, hipStream_t s);
struct GzSpanLabArgs {
    const int32_t* span; const int64_t* word_off; int64_t n_docs, n_words;      // span[word_off[d] .. word_off[d + 1]) are document d's words (absolute)
    const int32_t* marks; const int64_t* mark_off; int64_t n_marks;             // marks[mark_off[d] .. mark_off[d + 1]) are its marks (absolute)
    int32_t scheme, outside;                                        // 0 plain, 1 BIO
    uint32_t* owner;                                                // [n_words] scratch, from 0; needed where word_labels is given
    int32_t* word_labels;                                           // indexed as span (absolute); may be null
    int32_t* mark_words;                                            // [n_marks, 2] from 0; may be null
};
void gz_launch_span_labels(const GzSpanLabArgs& A, hipStream_t s);

// text pre-pass (gz_preproc.inc): one filter over documents that sit in the slots of a packed text
struct GzPpArgs {
    const uint8_t* in; const int64_t* in_off;   // slot of document d = in[in_off[d] - in_off[0] ... (in_abs: see below)
    const int64_t* in_len;                      // ... its current length (nullptr: the whole slot, in_off[d+1] - in_off[d])
    int32_t in_abs;                             // 1: `in` is the caller's text, document d at in[in_off[d] ...] (absolute, as gz_encode_batch_device)
    int64_t n_docs;
    uint8_t* out;                               // pass 1: same slots, another buffer
    int64_t* out_len;                           // pass 1: the new lengths
    int64_t* aux;                               // [n_docs] html: position of the unclosed '<' (pass 0 -> pass 1)
    int32_t op;                                 // GZ_PP_*
    int64_t skip_upto;                          // documents whose INPUT slot is at most this long are left alone (gz_pp_fused_kernel did them); -1: none
};
struct GzPpFusedArgs {                          // the whole chain for short documents, on chip (gz_pp_fused_kernel)
    const uint8_t* in; const int64_t* in_off;   // the caller's text, absolute offsets
    int64_t n_docs;
    uint8_t* out; int64_t* out_len;             // the documents' slots of the chain's LAST buffer, their final lengths
    int32_t n_ops; int32_t ops[16];
    uint32_t* n_long;                           // += documents too long for this kernel (zeroed by the caller)
    uint32_t* out_len32;                        // the same lengths as 32-bit words (0 for a document left to the chain): input of the chained scan
};
#ifndef GZ_PPF_CAP
#define GZ_PPF_CAP 4096
#endif
constexpr int GZ_PP_FUSED_MAX_BYTES = GZ_PPF_CAP;     // == PPF_CAP (gz_preproc.inc)
void gz_launch_preprocess(const GzPpArgs& A, int pass, hipStream_t s);
void gz_launch_preprocess_fused(const GzPpFusedArgs& A, hipStream_t s);
void gz_launch_scan64(const int64_t* len, int64_t n, int64_t* out_off /* n+1 */, hipStream_t s);
void gz_launch_pp_pack(const uint8_t* in, const int64_t* in_off, const int64_t* len, int64_t n_docs, uint8_t* out, const int64_t* out_off,
                       hipStream_t s);
// the tail of the pre-pass when gz_pp_fused_kernel did every document: exclusive scan of the 32-bit lengths IN PLACE (chained scan
// over many workgroups, total at [n_docs]; lb / ctl / epoch as gz_scan32m_kernel wants them: ctl[1] = ticket counter, ctl[2] = time-out
// flag, both zeroed by the caller), then the slots -> the packed text (out may be null; documents that end beyond capacity are not
// written), four documents per wave, and out_off as 64-bit offsets
void gz_launch_pp_tail(const uint8_t* slots, const int64_t* in_off, uint32_t* len32, int64_t n_docs, uint8_t* out, int64_t capacity, int64_t* out_off,
                       unsigned long long* lb, uint32_t* ctl, uint32_t epoch, hipStream_t s);

// BM25 / BM25Plus index and scoring (gz_bm25.inc; genz_tokenize/ranking.py of the reference)
struct GzBm25Slot { unsigned long long key; uint32_t a, b; };     // open-addressing slot, key 0: empty
struct GzBm25Args {
    const uint8_t* tb;                  // document d = tb[off[d] .. off[d+1]) (absolute offsets)
    const int64_t* off;
    int64_t n_docs, n_words;
    int64_t lo, hi;                     // the offsets must lie in [lo, hi] (else ctl[1] is raised and the document counts as empty)
    uint32_t* ctl;                      // [0] words left for the next de-duplication round, [1] bad offsets, [2] an append: dead terms live again
    uint32_t* wcnt;                     // [n_docs] words per document (fieldLens)
    uint32_t* woff;                     // [n_docs + 1] index of each document's first word
    int64_t* wstart; int64_t* wend;     // [n_words] absolute byte range of every word
    uint32_t* wdoc;                     // [n_words] its document
    unsigned long long* whash;          // [n_words] table key of its bytes
    unsigned long long hmask;           // hash bits kept (switch bm25_hash_bits)
    uint32_t* rep;                      // [n_words] representative: the first word in the corpus with the same bytes
    uint32_t* wslot;                    // [n_words] its slot in the de-duplication table, later in the pair table
    GzBm25Slot* dtab; unsigned long long dmask;      // de-duplication table: key = hash, a = ~(smallest word index)
    uint32_t* flag; uint32_t* scan;     // [n_words + 1] flags and their exclusive scan
    uint32_t* term;                     // [n_words] term id
    int64_t* tstart; uint32_t* tlen;    // [n_terms] bytes of every term (its representative's)
    GzBm25Slot* ttab; unsigned long long tmask;      // term table: key = hash, a = term id (one slot per term)
    GzBm25Slot* ptab; unsigned long long pmask;      // pair table: key = (doc << 32 | term) + 1, a = count, b = ~(first word index)
    uint32_t* df;                       // [n_terms]
    uint32_t* dfs;                      // [GZ_BM25_DF_SHARDS * n_terms] df counted per document mod GZ_BM25_DF_SHARDS (zeroed by the caller)
    int64_t n_terms;
    unsigned long long* sig;            // [n_docs * 4] 256-bit term signature per document
    uint2* ent;                         // [n_ent] (term, count), doc-major, first-occurrence order inside a document
    uint32_t* eoff;                     // [n_docs + 1] each document's first entry
    // an append (gz_bm25_append): the batch's documents, words and new terms are numbered from 0 in the arrays above, which point at
    // the tails of the index's own; these bases make the index's numbers of them (all 0 in a build)
    int64_t obase;                      // added to every off[d]: the batch's text lies behind the index's own
    uint32_t doc_base;                  // wdoc = doc_base + d
    uint32_t term_base;                 // term id of a new term = term_base + (representatives before it)
    uint32_t ent_base;                  // eoff[d] = ent_base + (entries of the batch before d); ent points at entry ent_base
};
enum { GZ_BM25_COUNT, GZ_BM25_WORDS, GZ_BM25_HASH, GZ_BM25_DEDUP_INS, GZ_BM25_DEDUP_RES, GZ_BM25_FIRST, GZ_BM25_TERM, GZ_BM25_PAIR_INS,
       GZ_BM25_PAIR_FIRST, GZ_BM25_DF, GZ_BM25_ENT, GZ_BM25_KNOWN };
constexpr uint32_t GZ_BM25_KNOWN_WORD = 0xFFFFFFFFu;      // rep[] of a batch word that is a term of the index already (an append)
constexpr int GZ_BM25_DF_SHARDS = 16;
struct GzBm25Look {
    const uint8_t* tb; const int64_t* tstart; const uint32_t* tlen; const uint32_t* df;
    const GzBm25Slot* ttab; unsigned long long tmask, hmask;
    const uint8_t* qtext; const int64_t* qoff; int64_t n;        // query word i = qtext[qoff[i] .. qoff[i+1])
    int32_t* term_out; int32_t* df_out;
};
struct GzBm25Score {
    const uint32_t* dl; const unsigned long long* sig; const uint32_t* eoff; const uint2* ent;
    const GzBm25Slot* ptab; unsigned long long pmask;
    int64_t n_docs;
    const int32_t* qterm; const double* qidf; const int64_t* qoff; int64_t n_q;   // query q = words qoff[q] .. qoff[q+1] (absolute)
    double kp1, k1, omb, b, avg, delta;                            // k1 + 1, k1, 1 - b, b, avgFieldLen, delta (host-computed)
    int32_t plus;                                                  // 1: BM25Plus
    double* out;                                                   // [n_q, n_docs]
};
// a removal (gz_bm25_remove): live arrays are read, the staged ones (...2) written
struct GzBm25Rm {
    const int64_t* ids; int64_t n_ids;  // the documents to remove (device memory; any order, duplicates allowed)
    int64_t n_docs;                     // documents of the index before the removal
    uint32_t* ctl;                      // [1] an id outside [0, n_docs), [2] terms whose df reached 0, [4..5] (64 bits) words of the removed documents
    uint32_t* gone;                     // [n_docs] 1: the document goes (cleared by the caller)
    uint32_t* before;                   // [n_docs + 1] exclusive scan of gone: new id = old id - before[old id]
    uint32_t* kcnt; uint32_t* neoff;    // [n_docs + 1] entries a document keeps, and their exclusive scan (the new eoff by OLD id)
    const uint32_t* dl; const unsigned long long* sig; const uint32_t* eoff; const uint2* ent;
    uint32_t* dl2; unsigned long long* sig2; uint32_t* eoff2; uint2* ent2;
    GzBm25Slot* ptab2; unsigned long long pmask2;    // the fresh pair table (cleared by the caller)
    uint32_t* df2;                      // a copy of df: the removed documents' entries are taken off it
    // a positional index (seq non-null): the kept documents' words move to their new places
    const uint32_t* seq; int64_t n_words;            // [n_words] the term id of every word, doc-major
    uint32_t* kdl;                      // [n_docs] words a document keeps (none when it goes)
    uint32_t* woff; uint32_t* nwoff;    // [n_docs + 1] exclusive scans of dl and of kdl: a document's first word, old and new (by OLD id)
    uint32_t* seq2;                     // [nwoff[n_docs]]
};
enum { GZ_BM25_RM_MARK, GZ_BM25_RM_COUNT, GZ_BM25_RM_DOCS, GZ_BM25_RM_ENT, GZ_BM25_RM_SEQ };
void gz_launch_bm25_remove(int step, const GzBm25Rm& R, hipStream_t s);
// the canonical numbering of the live terms (order of first occurrence in the current documents: a fresh build's), for a
// compaction (gz_bm25_compact) and the vocabulary read (gz_bm25_terms): live arrays are read, workspace and the staged /
// output arrays (...2) written
struct GzBm25Cp {
    int64_t n_docs, n_ent, n_terms;     // of the live index; n_terms counts the dead terms too
    int64_t n_new;                      // live terms = flags raised (the host knows it: n_live)
    const uint8_t* tb; const int64_t* tstart; const uint32_t* tlen; const uint32_t* df;
    const uint2* ent; const uint32_t* eoff;
    uint32_t* ctl;                      // [1] the index contradicts itself (a term id out of range, df > 0 without an entry, ...)
    uint32_t* first;                    // [n_terms] smallest entry index that holds the term (all ones: none; set by the caller)
    uint32_t* flag; uint32_t* scan;     // [n_ent + 1] entry e is its term's first, and the exclusive scan
    uint32_t* newid;                    // [n_terms] new id (all ones: a dead term)
    uint32_t* order;                    // [n_new] old id of new term n
    uint32_t* nlen; uint32_t* toff;     // [n_new + 1] bytes of new term n, and their exclusive scan (toff[n_new] = all bytes)
    uint8_t* arena;                     // [toff[n_new]] the live terms' bytes in new-id order (null: not gathered)
    int64_t* tstart2;                   // [n_new] = toff; close != 0: [n_new + 1], the total included (offsets of gz_bm25_terms)
    int32_t close;
    uint32_t* tlen2; uint32_t* df2;     // [n_new] (tlen2 may be null)
    uint2* ent2;                        // [n_ent] the entries under the new ids
    unsigned long long* sig2;           // [n_docs * 4] signatures of the new ids
    GzBm25Slot* ptab2; unsigned long long pmask2;    // the fresh pair table (cleared by the caller)
    const uint32_t* seq; uint32_t* seq2; int64_t n_words;      // a positional index: every word's term id, old and under the new ids
};
enum { GZ_BM25_CP_FIRST, GZ_BM25_CP_FLAG, GZ_BM25_CP_NEWID, GZ_BM25_CP_GATHER, GZ_BM25_CP_ENT, GZ_BM25_CP_SEQ };
void gz_launch_bm25_compact(int step, const GzBm25Cp& C, hipStream_t s);
// the term table into a fresh one (cleared by the caller): a = newid[a], slots of dead terms (newid all ones) are dropped
void gz_launch_bm25_rekey(const GzBm25Slot* from, int64_t n_slots, const uint32_t* newid, GzBm25Slot* to, unsigned long long mask, hipStream_t s);
// step: GZ_BM25_*; list / n / next: the de-duplication round's words (list null: all), the next round's list
// (GZ_BM25_KNOWN: next = the words that are no term of the index yet, the first round's list)
void gz_launch_bm25(int step, const GzBm25Args& A, const uint32_t* list, int64_t n, uint32_t* next, hipStream_t s);
// exclusive scan of u32: out[n + 1] (out[n] = total), bsum: (n + 4095) / 4096 + 1 words of workspace
void gz_launch_bm25_scan(const uint32_t* in, int64_t n, uint32_t* out, uint32_t* bsum, hipStream_t s);
// every used slot of `from` (n_slots of them) enters `to` (cleared by the caller, mask + 1 slots, more than there are keys) with its a and b
void gz_launch_bm25_rehash(const GzBm25Slot* from, int64_t n_slots, GzBm25Slot* to, unsigned long long mask, hipStream_t s);
void gz_launch_bm25_lookup(const GzBm25Look& L, hipStream_t s);
void gz_launch_bm25_score(const GzBm25Score& S, hipStream_t s);

// BM25 top-k (gz_topk.inc): selection over score rows in HBM, level after level until one tile per row is left
constexpr int GZ_TOPK_TILE_MAX = 4096;    // elements per workgroup of a selection level (16 per thread, in registers)
constexpr int GZ_TOPK_SORT = 1024;        // == GZ_BM25_TOPK_MAX of the public header: the last level's sort in LDS
struct GzTopk {
    const double* scores;                 // [rows, n_docs] the score rows
    int64_t n_docs, rows, k;              // k = min(k, n_docs) <= GZ_TOPK_SORT
    int64_t tile;                         // documents per workgroup of the first level (1 .. GZ_TOPK_TILE_MAX)
    unsigned long long* ckey[2];          // candidates between levels (ping-pong): [rows, m1] and [rows, m2] of gz_topk_sizes
    uint32_t* cidx[2];
    int64_t* doc_out; double* score_out;  // [rows, k]
};
// candidates per row that a level over m elements in tiles of `tile` keeps
inline int64_t gz_topk_level(int64_t m, int64_t tile, int64_t k) { return (m + tile - 1) / tile * (k < tile ? k : tile); }
// candidates per row of the first level's output (m1) and of the second's (m2); 0 where that level is the last
inline void gz_topk_sizes(int64_t n_docs, int64_t tile, int64_t k, int64_t& m1, int64_t& m2)
{
    m1 = m2 = 0;
    if ((n_docs + tile - 1) / tile <= 1) return;
    m1 = gz_topk_level(n_docs, tile, k);
    if ((m1 + GZ_TOPK_TILE_MAX - 1) / GZ_TOPK_TILE_MAX > 1) m2 = gz_topk_level(m1, GZ_TOPK_TILE_MAX, k);
}
void gz_launch_topk(const GzTopk& T, hipStream_t s);

// BM25 vocabulary queries (gz_vocab.inc): query words against every live term, addressed by the canonical numbering of GzBm25Cp
// (new id n = table term order[n], nlen[n] bytes at tb + tstart[order[n]]); the index is only read
constexpr int GZ_VOCAB_EDIT_MAX = 64;     // == GZ_BM25_EDIT_MAX of the public header: a query word's code points, one state bit each
struct GzBm25Vocab {
    const uint8_t* tb; const int64_t* tstart; const uint32_t* df; const uint32_t* order; const uint32_t* nlen;
    int64_t n_new;                        // live terms
    // the chunk: `rows` words.  GZ_BM25_VC_EDIT: word r = code points cps[cpoff[r] .. cpoff[r + 1]) (at most GZ_VOCAB_EDIT_MAX);
    // GZ_BM25_VC_PREFIX: word r = wbytes[woff[r] .. woff[r + 1])
    const uint32_t* cps; const uint32_t* cpoff;
    const uint8_t* wbytes; const int64_t* woff;
    int64_t rows;
    int32_t max_edits;
    double* keys;                         // [rows, n_new] -(distance * 2^32) + df of a matching term (prefix: df), else NaN
    uint32_t* cnt;                        // [rows] matching terms (cleared by the caller)
    // GZ_BM25_VC_UNPACK: the selection over the key rows (gz_launch_topk's doc_out / score_out) -> the outputs
    const int64_t* sel_id; const double* sel_key; int64_t k;
    int32_t prefix;                       // 1: the keys are df alone
    int64_t* ids_out; int32_t* dist_out; int32_t* df_out;     // [rows, k]; -1 / -1 / 0 from cnt[r] on (dist_out may be null)
    int64_t* cnt_out;                     // [rows]
    // GZ_BM25_VC_LEN / GZ_BM25_VC_GATHER: listed terms (canonical ids; -1: no term)
    const int64_t* ids; int64_t n_ids;
    uint32_t* len_out;                    // [n_ids] bytes of every listed term
    const int64_t* boff; uint8_t* bytes;  // [n_ids + 1] the lengths' exclusive scan; term i -> bytes[boff[i] .. boff[i + 1])
};
enum { GZ_BM25_VC_EDIT, GZ_BM25_VC_PREFIX, GZ_BM25_VC_UNPACK, GZ_BM25_VC_LEN, GZ_BM25_VC_GATHER };
void gz_launch_bm25_vocab(int step, const GzBm25Vocab& V, hipStream_t s);

// BM25 search (gz_search.inc): term-major postings, and the matching documents of every query counted, scored and ranked
constexpr int GZ_SEARCH_TILE = 2048;      // bitmap words per workgroup of the counting / candidate kernels (8 per thread)
struct GzBm25Post {
    int64_t n_docs, n_terms, n_ent;
    const uint32_t* eoff; const uint2* ent;
    const uint32_t* poff;                 // [n_terms + 1] exclusive scan of df
    uint32_t* cur;                        // [n_terms] entries of the term placed so far (cleared by the caller)
    uint32_t* pdoc;                       // [n_ent] the documents of term t at poff[t] .. poff[t + 1], in no particular order
    uint32_t* ctl;                        // [1] df and the entries contradict each other
};
void gz_launch_bm25_post(const GzBm25Post& P, hipStream_t s);
struct GzBm25Search {
    GzBm25Score S;                        // the index's arrays and the scoring parameters (its query fields are not read)
    const uint32_t* poff; const uint32_t* pdoc;
    int64_t n_docs, n_terms, n_ent;
    // the chunk: `rows` queries, row r = words qoff[r] .. qoff[r + 1] (absolute indices into qterm / qidf), n_qw words in all
    const int32_t* qterm; const double* qidf; const int64_t* qoff;
    int64_t rows, n_qw;
    // mode 1 ("all"): a document matches when it holds every word of the row (0: at least one); xoff non-null: and none of the
    // row's excluded terms xterm[xoff[r]] .. xterm[xoff[r + 1]] (absolute indices; -1 is skipped)
    int32_t mode;
    const int32_t* xterm; const int64_t* xoff;
    int64_t w64;                          // bitmap words per row = ceil(n_docs / 64)
    unsigned long long* bm;               // [rows, w64] bit d of row r: document d matches query r (cleared by the caller)
    uint32_t* wrow; uint32_t* wns;        // [n_qw] row of every word, slices of its postings list
    uint32_t* wsoff;                      // [n_qw + 1] exclusive scan of wns
    int64_t n_tiles;                      // tiles of a row's bitmap
    uint32_t* tcnt; uint32_t* tbase;      // [rows, n_tiles] set bits of every tile, and their exclusive scan along the row
    uint32_t* cnt;                        // [rows] matching documents
    int64_t* cnt_out;                     // [rows] the same as int64 (may be null)
    // the rows row0 .. row0 + (rows of the launch) scored together: candidate lists of stride M (the largest of their counts)
    int64_t row0, M;
    uint32_t* cand;                       // [., M] the matching documents in ascending id
    double* csc;                          // [., M] their scores, NaN behind the row's count
    const int64_t* pos; const double* psc;  // [., k2] the selection's positions into the candidate list and scores
    int64_t k2, kk;                       // k2 = min(kk, M)
    int64_t* doc_out; double* score_out;  // [., kk]: -1 / NaN behind the row's count
    // a phrase search (phoff non-null; a positional index): of the marked documents only those stay in which the terms
    // phterm[phoff[r]] .. phterm[phoff[r + 1]] (absolute indices; at most GZ_PHRASE_MAX; -1: no document holds it) stand next to each
    // other in this order; a row without phrase terms is left alone
    const int32_t* phterm; const int64_t* phoff;
    const uint32_t* seq; const uint32_t* woff; int64_t n_words;    // document d = seq[woff[d] .. woff[d + 1])
    uint32_t* ctl;                        // [1] the word offsets contradict n_words
};
constexpr int GZ_PHRASE_MAX = 64;         // == GZ_BM25_PHRASE_MAX of the public header: a lane per phrase term
enum { GZ_BM25_SR_WORDS, GZ_BM25_SR_MARK, GZ_BM25_SR_COUNT, GZ_BM25_SR_ROWS, GZ_BM25_SR_CAND, GZ_BM25_SR_SCORE, GZ_BM25_SR_OUT,
       GZ_BM25_SR_DRIVER, GZ_BM25_SR_FILTER, GZ_BM25_SR_PHRASE };
// rows: of the chunk (WORDS, DRIVER, MARK, FILTER, PHRASE, COUNT, ROWS), else of the launch (from row0)
void gz_launch_bm25_search(int step, const GzBm25Search& A, int64_t rows, hipStream_t s);

// BM25 search over word groups (gz_groups.inc): a group of alternative terms counts as one query word.  The chunk's GzBm25Search
// carries the flat alternative list as its word list (qterm; qoff[r] = aoff[goff[r]], so WORDS and MARK run unchanged); qidf is
// not read.  The alternatives of a group are distinct and valid: the entry point drops -1 and repeats.
struct GzBm25Group {
    GzBm25Search A;
    const int64_t* goff;                  // [rows + 1] row r = groups goff[r] .. goff[r + 1] (absolute indices into aoff / gidf / gmask)
    const int64_t* aoff;                  // [n_groups + 1] group g = alternatives aoff[g] .. aoff[g + 1] (absolute indices into A.qterm)
    const double* gidf;                   // [n_groups] the idf of every group (host-computed)
    unsigned long long* gmask;            // [n_groups, 4] the OR of the alternatives' signature bits (GZ_BM25_GR_MASK writes it)
    int64_t n_groups;                     // of the whole call (GZ_BM25_GR_MASK)
};
constexpr int GZ_GROUP_MAX = 64;          // == GZ_BM25_GROUP_MAX of the public header: distinct alternatives of a group
enum { GZ_BM25_GR_MASK, GZ_BM25_GR_DRIVER, GZ_BM25_GR_FILTER, GZ_BM25_GR_SCORE };
// rows: of the chunk (DRIVER, FILTER), of the launch from row0 (SCORE); MASK covers every group of the call
void gz_launch_bm25_groups(int step, const GzBm25Group& G, int64_t rows, hipStream_t s);

// BM25 snippets (gz_snippet.inc): where the query's words stand inside given documents of a positional index.  A pair r is
// (query r / k, document ids[r]); document d = seq[woff[d] .. woff[d + 1]).  An id outside [0, n_docs) is a pair without words.
struct GzBm25Snip {
    const uint32_t* seq; const uint32_t* woff; int64_t n_words, n_docs;
    const int32_t* qterm; const int64_t* qoff;      // query q = terms qoff[q] .. qoff[q + 1] (absolute indices; -1 matches nothing)
    const int64_t* ids; int64_t n_pairs, k;
    int64_t width;                                  // the window (GZ_BM25_SN_WINDOW), >= 1
    int32_t* start_out; int32_t* hits_out;          // [n_pairs] the smallest start with the most hits, and the hits; -1 / 0 without a document
    uint32_t* cnt;                                  // [n_pairs] occurrences of every pair (GZ_BM25_SN_COUNT)
    const uint32_t* base;                           // [n_pairs + 1] their exclusive scan (GZ_BM25_SN_FILL)
    int32_t* pos_out; int32_t* word_out;            // [base[n_pairs]] position in the document, first place of the word in the query
    uint32_t* ctl;                                  // [1] the word offsets contradict n_words, [4..5] (64 bits) all occurrences counted
};
enum { GZ_BM25_SN_WINDOW, GZ_BM25_SN_COUNT, GZ_BM25_SN_FILL };
void gz_launch_bm25_snippet(int step, const GzBm25Snip& A, hipStream_t s);

// BM25 proximity (gz_near.inc): the smallest window of a document of a positional index that holds every term of a set.  Set r =
// sterm[soff[r] .. soff[r + 1]) (absolute indices; at most GZ_NEAR_MAX; a repeated term counts once).
struct GzBm25Near {
    GzBm25Score S;                                  // the index's signatures and pair table (nothing else of it is read)
    const uint32_t* seq; const uint32_t* woff; int64_t n_words, n_docs, n_terms;    // document d = seq[woff[d] .. woff[d + 1])
    const int32_t* sterm; const int64_t* soff;
    // the near stage of a search chunk (GZ_BM25_SR_NEAR, behind GZ_BM25_SR_PHRASE): of the documents marked in row r only those stay
    // that hold every term of set r inside some win[r] consecutive words; a term -1 clears the row, a row without terms is left alone
    const int64_t* win;                             // [rows] >= 1 where the row has terms
    unsigned long long* bm; int64_t w64;            // [rows, w64] the chunk's bitmaps (GzBm25Search::bm)
    // the cover of pairs (GZ_BM25_NR_COVER): pair r = (query r / k, document ids[r]), set = the query's terms (-1 is ignored)
    const int64_t* ids; int64_t n_pairs, k;
    int32_t* start_out; int32_t* len_out; int32_t* words_out;   // [n_pairs] the shortest window with every term the document holds
                                                    // (ties: the smallest start), its length, and how many terms that is; (0, 0, 0)
                                                    // without any, (-1, 0, 0) for an id outside [0, n_docs)
    uint32_t* ctl;                                  // [1] the word offsets contradict n_words, or the pair table the words
};
constexpr int GZ_NEAR_MAX = 64;           // == GZ_BM25_NEAR_MAX of the public header: a lane per term of the set
enum { GZ_BM25_SR_NEAR, GZ_BM25_NR_COVER };
// rows: of the chunk (GZ_BM25_SR_NEAR)
void gz_launch_bm25_near(int step, const GzBm25Near& A, int64_t rows, hipStream_t s);

// BPE learner (gz_learn.inc): the counts of a word set on top of the word front it shares with the BM25 build and append (host side:
// bm_front_count and bm_front_words in gz_bm25_api.inc, the only callers of those kernels), and the merge loop of gz_bpe_learn.
// The words' symbols live in one flat array, word d = sym[woff[d] .. woff[d] + wlen[d]) (a merge shortens it in place, its slice
// stays where it is); the pair table is open addressing, key = (left << 32 | right) + 1 (0: empty), cnt = n(left, right); nothing is
// ever deleted, a count of 0 stays.
struct GzLearnSlot { unsigned long long key; long long cnt; };
struct GzLearn {
    int32_t* sym; const uint32_t* woff; uint32_t* wlen; const long long* cw; int64_t n_words;
    const uint32_t* longw; int64_t n_long;          // the words of more than GZ_LEARN_LANE_MAX initial symbols: a wave each
    GzLearnSlot* tab; unsigned long long mask;
    unsigned long long* ctl;                        // [0] best key, [1] best count, [2] keys in the table, [3] a probe found the table full
    unsigned long long* part; int32_t n_part;       // [2 * n_part] the reduction's per-workgroup bests (key, count)
    int32_t l, r, m;                                // the step: every l r becomes m
    long long* hist;                                // [2 * n_symbols] count of (symbol, is the word's last position)
};
constexpr int GZ_LEARN_LANE_MAX = 64;
enum { GZ_LEARN_PAIRS, GZ_LEARN_BEST, GZ_LEARN_APPLY, GZ_LEARN_HIST };
void gz_launch_learn(int step, const GzLearn& L, hipStream_t s);
// a table into a larger one (cleared by the caller): every key claims its own slot and takes its count along
void gz_launch_learn_rehash(const GzLearnSlot* from, int64_t n_slots, const GzLearn& to, hipStream_t s);
// The counts of a word set, behind GZ_BM25_FIRST and the scan of its flags: cnt[term of w] += weight[document of w] (1 without
// weights); the representatives write tstart / tlen.  cnt holds GZ_BM25_DF_SHARDS * n_terms zeroed counters, the sums end up in its
// first n_terms.  strict: a document that is not exactly one word raises ctl[1] bit 1.
void gz_launch_wordset_count(const GzBm25Args& A, const long long* weight, long long* cnt, int64_t n_terms, int strict, hipStream_t s);
// word t = tb[tstart[t] .. + tlen[t]) -> arena[toff[t] ..)
void gz_launch_wordset_gather(const uint8_t* tb, const int64_t* tstart, const uint32_t* tlen, const uint32_t* toff, uint8_t* arena, int64_t n,
                              hipStream_t s);
