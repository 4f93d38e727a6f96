/* genz_tokenize.h -- C ABI of the MI355X-native genz-tokenize hot path.
 *
 * This is the drop-in boundary underneath the reference's Python surface.  The
 * reference (DVNghiem/genz-tokenize v1.2.7) is pure Python and has no FFI of its
 * own, so every entry point below names the reference function it replaces
 * (paths relative to the reference checkout, genz_tokenize/tokenize.py).
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer it passes in;
 *   - every function returns GZ_OK (0) or a negative GZ_E_* code; no C++
 *     exception crosses this boundary; gz_last_error() gives the message;
 *   - a gz_ctx is bound to ONE GPU (one process per GPU is the multi-GPU model)
 *     and is not re-entrant; distinct contexts are independent;
 *   - there is NO CPU fallback: without a usable gfx950 device gz_create fails.
 *
 * Text is packed UTF-8: document i is text[text_off[i] .. text_off[i+1]).
 * Python's `None` inside sequence_id / token_type_ids is carried as GZ_NONE.
 */
#ifndef GENZ_TOKENIZE_H
#define GENZ_TOKENIZE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GZ_VERSION 0x010100   /* 1.1: gz_expand_block takes the block's entry total (the block layout itself is round 5's) */

#define GZ_OK            0
#define GZ_E_INVALID    -1   /* bad argument */
#define GZ_E_UTF8       -2   /* table file is not valid UTF-8 (reference: UnicodeDecodeError at tokenize.py:45/54) */
#define GZ_E_HIP        -3   /* HIP runtime error */
#define GZ_E_NOTABLES   -4   /* gz_load_tables has not succeeded on this context */
#define GZ_E_CAPACITY   -5   /* ragged output does not fit `capacity`; row_off[n_docs] holds the size needed */
#define GZ_E_LIMIT      -6   /* table exceeds 2^20-2 symbol ids (every merge line takes one: merge lines + other symbols) */
#define GZ_E_NOMEM      -7
#define GZ_E_RCCL       -8
#define GZ_E_NODEVICE   -9   /* no gfx950 device / HIP runtime unusable */

/* flags of gz_encode_batch*: the keyword arguments of Tokenize.__call__ (tokenize.py:184-190) */
#define GZ_PADDING       0x1u   /* padding=True                                   */
#define GZ_TRUNCATION    0x2u   /* truncation=True                                */
#define GZ_MAX_LEN_NONE  0x4u   /* max_len=None (the max_len argument is ignored) */
#define GZ_TIMING        0x100u /* record HIP events around the kernels (gz_timing) */
#define GZ_NO_WORD_TABLE 0x200u /* do not consult the whole-word table: every word runs the merge loop (same results) */
#define GZ_KEEP_WORDS    0x400u /* keep the per-word records of this call for gz_word_token_counts (return_offset=True): small
                                   batches otherwise run in ONE fused launch that keeps nothing per word */

#define GZ_NONE (-1)            /* Python None in sequence_id / token_type_ids */

typedef struct gz_ctx gz_ctx;

int  gz_version(void);

/* Tokenize.__init__ part 1 (tokenize.py:7-37): create a context on HIP device `device_id`. */
int  gz_create(int device_id, gz_ctx **out);
void gz_destroy(gz_ctx *ctx);
const char *gz_last_error(gz_ctx *ctx);   /* ctx may be NULL: error of the last failed gz_create on this thread */

/* add_vocab_file + add_bpe_file (tokenize.py:44-57) on RAW FILE BYTES, followed by the build of the
 * device-side tables (pair -> rank hash, rank -> merged symbol, symbol -> vocab ids, code point -> symbol).
 * specials_utf8 = { pad, bos, eos, mask, unk } as NUL-terminated UTF-8 (tokenize.py:7-12, :31-37).
 * Loader quirks L1-L8 of SURVEY.md are reproduced exactly. */
int  gz_load_tables(gz_ctx *ctx, const uint8_t *vocab, size_t vocab_len,
                    const uint8_t *bpe, size_t bpe_len, const char *const specials_utf8[5]);

/* The table cache behind gz_load_tables (reference: Tokenize.__init__ re-parses both files on every construction,
 * tokenize.py:39-42, and fromFile does so twice, :261-267).  The finished table images are kept in
 * $GZ_TABLE_CACHE (default ~/.cache/genz_tokenize_amd, created 0700; "0" / "off" disables) under the SHA-256 of the file
 * bytes, the specials, the file-format version and the BUILD IDENTITY of this library (a hash of its sources: images made by
 * another build are never loaded); a file whose key, length, checksum or section sizes do not fit, or that holds an index
 * outside the tables it indexes, is refused and the tables are rebuilt; a directory other users can write to is not used.
 * gz_table_cache_status: what the last gz_load_tables of this context did -- 0 no cache, 1 hit, 2 miss (built and written),
 * 3 a cache file was there and was refused (rebuilt and rewritten), 4 built, but the file could not be written.
 * gz_table_digest: SHA-256 over every device table image + the host-visible dictionaries (equal for built and cached loads). */
int  gz_table_cache_status(gz_ctx *ctx);
int  gz_table_digest(gz_ctx *ctx, uint8_t out[32]);

/* vocab_size() (tokenize.py:59-60), encoder[pad|bos|eos|mask|unk] looked up at call time
 * (tokenize.py:134,143,145,151,164-165), len(bpe_ranks), number of interned symbols. */
int  gz_table_info(gz_ctx *ctx, int32_t *vocab_size, int32_t special_ids[5],
                   int32_t *n_ranks, int32_t *n_symbols);

/* Enumerate the encoder dict built by gz_load_tables in insertion order (so the Python shim can expose
 * `encoder` / `decoder`, tokenize.py:31-40): entry i -> (utf8 pointer valid until the next gz_load_tables,
 * byte length, id).  Returns GZ_E_INVALID when i is out of range. */
int  gz_vocab_entry(gz_ctx *ctx, int64_t i, const uint8_t **utf8, int32_t *len, int32_t *id);
/* Same for bpe_ranks (tokenize.py:53-57): key i of the dict in insertion order.  The tuple's fields are
 * returned joined by single '\n' bytes (fields never contain whitespace); n_fields may be 0. */
int  gz_merge_entry(gz_ctx *ctx, int64_t i, const uint8_t **utf8, int32_t *len, int32_t *n_fields, int32_t *rank);

/* Tokenize.__call__ (tokenize.py:184-259) over a batch of documents, host buffers in, host buffers out.
 *
 *   text/text_off          packed UTF-8 and n_docs+1 byte offsets
 *   pair/pair_off          NULL,NULL -> pair_text=None for every document; otherwise every document is a pair
 *   max_len, flags         keyword arguments (see GZ_* flags)
 *
 * Output layout.  With GZ_PADDING|GZ_TRUNCATION, no GZ_MAX_LEN_NONE and max_len >= 1 every row has exactly
 * max_len entries ("dense": row i starts at i*max_len, capacity must be >= n_docs*max_len).  Otherwise rows are
 * ragged: row i occupies [row_off[i], row_off[i+1]) of each flat array; if row_off[n_docs] > capacity nothing is
 * written to the flat arrays and GZ_E_CAPACITY is returned with row_off filled in.
 *
 *   input_ids, attention_mask       always written (tokenize.py:250-251)
 *   token_type_ids, sequence_id     pair mode only (may be NULL otherwise); both start at row_off[i] like the
 *                                   input_ids row and never exceed it: sequence_id row i holds pair_len[2i]
 *                                   entries, token_type_ids row i holds pair_len[2i+1] entries (tokenize.py:252-258;
 *                                   values 0 / 1 / GZ_NONE / pad id / eos id, rules P1-P6)
 *   row_off  [n_docs+1]             may be NULL in dense mode
 *   pair_len [2*n_docs]             pair mode; may be NULL otherwise
 *   n_real   [n_docs]               entries of the row that are not padding added by rule D1 (may be NULL)
 *   status   [n_docs]               0 = ok, 1 = the reference raises ValueError("None is not in list") for
 *                                   this document (tokenize.py:157-160, rule P3); may be NULL in single mode
 */
int  gz_encode_batch(gz_ctx *ctx,
                     const uint8_t *text, const int64_t *text_off,
                     const uint8_t *pair, const int64_t *pair_off,
                     int64_t n_docs, int32_t max_len, uint32_t flags, int64_t capacity,
                     int32_t *input_ids, int32_t *attention_mask,
                     int32_t *token_type_ids, int32_t *sequence_id,
                     int64_t *row_off, int32_t *pair_len, int32_t *n_real, int32_t *status);

/* The same call with every pointer a DEVICE pointer on the context's GPU (inputs already resident in HBM,
 * outputs left in HBM).  Work is enqueued on the context's stream; gz_sync waits for it and returns the
 * deferred error of the enqueued work, if any.  Only the dense layout and the ragged layout with a
 * sufficient capacity are available here (GZ_E_CAPACITY is reported by gz_sync).
 * The input buffers must be COMPLETE when the call is made (whatever wrote them has been synchronised): the library reads
 * them on its own streams, which know nothing of the caller's, and part of that reading starts at once. */
int  gz_encode_batch_device(gz_ctx *ctx,
                            const uint8_t *text, const int64_t *text_off,
                            const uint8_t *pair, const int64_t *pair_off,
                            int64_t n_docs, int32_t max_len, uint32_t flags, int64_t capacity,
                            int32_t *input_ids, int32_t *attention_mask,
                            int32_t *token_type_ids, int32_t *sequence_id,
                            int64_t *row_off, int32_t *pair_len, int32_t *n_real, int32_t *status);
/* The same when the caller also has the offsets on the host (it usually built them there): the library then knows the
 * byte sizes of the batch without reading them back from the device, i.e. without a host round trip before the
 * kernels are enqueued. */
int  gz_encode_batch_device_h(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, const uint8_t *pair,
                              const int64_t *pair_off, int64_t n_docs, int32_t max_len, uint32_t flags, int64_t capacity,
                              int32_t *input_ids, int32_t *attention_mask, int32_t *token_type_ids, int32_t *sequence_id,
                              int64_t *row_off, int32_t *pair_len, int32_t *n_real, int32_t *status,
                              const int64_t *text_off_host, const int64_t *pair_off_host);
int  gz_sync(gz_ctx *ctx);

/* Token count of every word of the LAST encode call (for `return_offset=True`, tokenize.py:105,111-117,225-244):
 * which_text 0 = text, 1 = pair text.  counts[w] = pieces of word w (words of all documents, in order),
 * doc_first[d] = index of document d's first word (n_docs+1 entries, n_docs of that encode call), *n_words = words of
 * the whole call.  When the call has more than `capacity` words: GZ_E_CAPACITY, *n_words holds the word total of the WHOLE
 * call (all its sub-batches) -- a second call with that capacity fits -- and counts / doc_first are not written.
 * Valid until the next encode call on the context, of any entry point and of any size: the last encode call must have been
 * made with GZ_KEEP_WORDS and must not have been cut into more than two sub-batches (GZ_E_INVALID otherwise; nothing is
 * written).  A host call with n_docs == 0 and every gz_encode_batch_csr call keep nothing. */
int  gz_word_token_counts(gz_ctx *ctx, int which_text, int32_t *counts, int64_t capacity,
                          int64_t *doc_first, int64_t *n_words);

/* Tokenize.bpe(token) (tokenize.py:62-101) for one word: the pieces as interned symbol ids.
 * pieces[k] >= 0 is a symbol id (string via gz_symbol_utf8); pieces[k] < 0 is -(code point)-1 for a code
 * point that occurs in no merge and no vocab entry.  Returns the number of pieces or a GZ_E_* code
 * (GZ_E_CAPACITY if more than `cap`).  The last piece still carries the "</w>" marker. */
int64_t gz_bpe_word(gz_ctx *ctx, const uint8_t *word_utf8, int64_t len, int32_t *pieces, int64_t cap);
int  gz_symbol_utf8(gz_ctx *ctx, int32_t symbol, const uint8_t **utf8, int32_t *len);

/* ---- BPE-dropout (Provilkov et al., 2020): seeded, reproducible segmentation noise ----
 * gz_encode_batch for single texts with ONE change: while a word is segmented, each candidate merge is skipped with probability
 * p = drop_threshold / 2^32.  Words ("\S+\n?", the glued line feed included), initial symbols, ranks, the piece-to-id lookup,
 * bos / eos framing, truncation and padding are those of the plain call.  The reference has no dropout: the rule is this one
 * (tests/dropout_oracle.py states it in plain Python).
 *
 *   The draws of a word are a pure function of (seed, D, j, t, i): D = doc_base + d the global document index, j the index of the
 *   word within its document, t the merge iteration, i the position in the word's current symbol list.
 *     key(seed, D, j) = words 0, 1 of Philox4x32-10(counter (D lo, D hi, j, 0), key (seed lo, seed hi))
 *     u(key, t, i)    = word (i & 3) of Philox4x32-10(counter (t, i >> 2, 0, 0), key)
 *   (Philox4x32-10: multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten rounds, as the masked-LM rows.)
 *   A word of one symbol is its own piece.  Else, iteration t = 0, 1, ...: position i is LIVE when u(key, t, i) >= drop_threshold
 *   and the pair (s[i], s[i+1]) is in the merge table; no live position: the word is finished; else the smallest rank among the live
 *   positions is merged at every live position that holds it, left to right, never overlapping; t + 1 follows.
 *   - a dropped occurrence of the chosen pair stays unmerged in that iteration (as in subword-nmt);
 *   - an iteration merges at least once: at most n - 1 iterations for n symbols, no spins, no retries;
 *   - drop_threshold 0 gives the plain call's result bit for bit, 2^32 gives every word as its code points;
 *   - the whole-word tables are never consulted, at no threshold.
 *
 * gz_encode_dropout: host pointers, the outputs of gz_encode_batch for single texts (row_off for ragged layouts, n_real may be NULL).
 * gz_encode_dropout_device: the same, every pointer a DEVICE pointer; errors that are only known once the kernels have run are
 * reported by gz_sync, as for gz_encode_batch_device.
 * flags: GZ_PADDING, GZ_TRUNCATION, GZ_MAX_LEN_NONE and GZ_TIMING as on gz_encode_batch; GZ_NO_WORD_TABLE is accepted and has no
 * effect; GZ_KEEP_WORDS: GZ_E_INVALID.  drop_threshold > 2^32, doc_base < 0, doc_base + n_docs past 2^63: GZ_E_INVALID.
 * A dropout call always takes the batch pipeline (the switch `small` does not apply); where a call is cut into sub-batches (the switch
 * sub_batches) D continues across the cut, so the result does not depend on the cut -- nor on how a corpus is split into calls, as
 * long as doc_base says where each call's documents start.  It counts as an encode call for gz_word_token_counts and keeps nothing.
 *
 * gz_bpe_word_dropout: gz_bpe_word for word number word_index (0 .. 2^32 - 1) of document doc (>= 0), same outputs. */
int  gz_encode_dropout(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, int64_t n_docs, int32_t max_len, uint32_t flags,
                       int64_t capacity, uint64_t drop_threshold, uint64_t seed, int64_t doc_base,
                       int32_t *input_ids, int32_t *attention_mask, int64_t *row_off, int32_t *n_real);
int  gz_encode_dropout_device(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, int64_t n_docs, int32_t max_len, uint32_t flags,
                              int64_t capacity, uint64_t drop_threshold, uint64_t seed, int64_t doc_base,
                              int32_t *input_ids, int32_t *attention_mask, int64_t *row_off, int32_t *n_real);
int64_t gz_bpe_word_dropout(gz_ctx *ctx, const uint8_t *word_utf8, int64_t len, uint64_t drop_threshold, uint64_t seed, int64_t doc,
                            int64_t word_index, int32_t *pieces, int64_t cap);

/* Host path with the copies overlapped (SURVEY.md 8(d) timing (ii); replaces a loop of Tokenize.__call__ with
 * max_len, padding=True, truncation=True over host strings, tokenize.py:184-259): the result comes back in CSR form --
 * n_real[d] = entries of row d after truncation (tokenize.py:141-146), and the rows' real entries back to back in
 * `tokens` (uint16 when bits == 16 and every id of the vocabulary fits, else int32; capacity in entries).  The dense
 * [N, max_len] input_ids / attention_mask are `row padded with the pad id` and `1 for the first n_real[d] positions`
 * unless a real token equals the pad id (then mask = ids != pad, :148-152): a caller rebuilds them only where needed.
 * The batch is cut into sub-batches: text H2D, kernels and the D2H of the compact rows run on three streams.
 * `text` / `tokens` / `n_real` from gz_host_alloc (pinned) make both copies true DMA; pageable memory works, slower.
 * *total = entries written (or needed: GZ_E_CAPACITY).  Single texts only.
 * gz_host_free does not use the context (a pinned block may outlive it): ctx may be NULL there. */
int  gz_host_alloc(gz_ctx *ctx, size_t bytes, void **ptr);
int  gz_host_free(gz_ctx *ctx, void *ptr);
int  gz_encode_batch_csr(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, int64_t n_docs, int32_t max_len,
                         uint32_t flags, void *tokens, int64_t capacity, int32_t bits, int32_t *n_real, int64_t *total);

/* Device memory helpers so that a Python host needs nothing but ctypes (no torch in the product path). */
int  gz_device_alloc(gz_ctx *ctx, size_t bytes, void **dptr);
int  gz_device_free(gz_ctx *ctx, void *dptr);
int  gz_memcpy_h2d(gz_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
int  gz_memcpy_d2h(gz_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);

/* With GZ_TIMING: milliseconds (HIP events on the context's stream) of the kernels of the LAST encode call:
 * out[0] = the kernel pipeline of the call (split: brk / classify / scan / docw0; words; misses: scan / miss / miss_wide /
 * long; rows: rows1 | rows | assemble | rowsr's count pass), out[1] = ragged layouts: row lengths, scan, and the copy out of the raw
 * area or -- single texts without padding -- the rows written at their places, out[2] = pair type-id
 * kernel, out[3] = whole call on the stream.  Unused slots are 0. */
int  gz_timing(gz_ctx *ctx, double out_ms[4]);
/* GZ_TIMING calls can be chained without gz_sync in between (a dense call followed by a call that brings host copies
 * of its offsets is enqueued right behind it).  gz_timing_history synchronises and returns the duration of the main
 * kernels of the last (up to 1024, up to `max`) timed calls, oldest first, then forgets them. */
int  gz_timing_history(gz_ctx *ctx, double *out_ms, int32_t max, int32_t *n_out);

/* Offline / diagnostic table build on the HOST only (no GPU needed): the same builder gz_load_tables runs, with
 * the integer tables it would upload exposed read-only.  `which` (0 is retired -- the linear-probing pair table of rounds 1-3 -- and answers GZ_E_INVALID like any unknown value, with *data = NULL and *count = 0): 1 merges
 * (uint32 x4 [n_lines]: left,right,merged,0), 2 symbol ids (int32 x2 [n_symbols]: non-final, final), 3 BMP code
 * point table (uint32 x2 [65536]: plain, final), 4 astral table (uint32 x4 [slots]: cp,plain,final,0; may be
 * empty), 5 special ids (int32 [5]); the perfectly hashed pair table of the big pipeline's merge kernel: 6 entries (uint32 x2
 * [slots]: left | right << 20, right >> 12 | alias flag << 8 | rank << 9; 0xFFFFFFFF x2: empty), 7 displacement array (uint16
 * [buckets]), 8 its description (uint32 [7]: buckets, bucket shift, slot shift, slots, the two seeded multipliers, keys in
 * overflow buckets), 9 the hot set staged in LDS (uint32 x2 [4096], same entry form).  Pointers stay valid until
 * gz_host_tables_destroy (8: until the next call of this function on this thread). */
typedef struct gz_host_tables gz_host_tables;
int  gz_host_tables_create(const uint8_t *vocab, size_t vocab_len, const uint8_t *bpe, size_t bpe_len,
                           const char *const specials_utf8[5], gz_host_tables **out);
void gz_host_tables_destroy(gz_host_tables *t);
int  gz_host_tables_array(gz_host_tables *t, int which, const void **data, int64_t *count);
int  gz_host_tables_vocab_entry(gz_host_tables *t, int64_t i, const uint8_t **utf8, int32_t *len, int32_t *id);
int  gz_host_tables_merge_entry(gz_host_tables *t, int64_t i, const uint8_t **utf8, int32_t *len, int32_t *n_fields, int32_t *rank);
int  gz_host_tables_symbol(gz_host_tables *t, int32_t symbol, const uint8_t **utf8, int32_t *len);

/* Byte counts the library's 32-bit device paths take (no context, no GPU needed).  which = 0: bytes of ONE text (text, or pair
 * text) of an encode call from which the call answers GZ_E_LIMIT -- split the batch; 1: input bytes from which the text pre-pass
 * (gz_preprocess_batch[_device], which has no size limit of its own) leaves its 32-bit length scan for the 64-bit one.  Both are
 * below 2^32.  Unknown `which`: -1. */
int64_t gz_limit(int which);

/* Switches for tests and experiments: typed, named, range-checked -- the library reads NONE of them from the environment (its
 * documented environment is GZ_TABLE_CACHE, GZ_LOAD_TIMING, and for the Python package GZ_LIBRARY and GZ_PACK_THREADS).
 * ctx == NULL sets the process-wide defaults, which every context created afterwards copies and which the table builder reads
 * (the "builder" keys act only there); ctx != NULL sets one context.  The defaults are the product's behaviour.  Keys
 * (value range; default):
 *   small (0..1; 1)            small batches in one launch; 0: everything through the kernel pipeline
 *   small_wgs (1..2^20; 768)   workgroups the one-launch kernel aims for
 *   host_direct (0..2^20; 4096) host calls whose inputs and outputs both fit this many bytes are computed straight on the pinned staging
 *                              block (no copy in, no copy back); 0: never
 *   assemble (1..3; 3)         row writer of dense single texts: 3 rows1, 2 the pair-mode kernel, 1 the ragged layouts' scatter kernel;
 *                              single texts without padding: 3 counted, scanned, written once, < 3 through the raw area
 *   word_table (0..1; 1)       0: every word through the merge loop (as GZ_NO_WORD_TABLE on every call)
 *   pp_fused (0..1; 1)         0: the text pre-pass filter by filter for every document
 *   sub_batches (1..8; 1)      dense batches cut into document ranges on two streams
 *   docs_per_wave (0..16; 0)   documents per wave of the ragged row writer (0: by the batch's shape)
 *   side, brk_side (0..1; 1)   0: no side stream / control words prepared on the main stream
 *   scan_multi (>= 0; 8192)    block counts from which the chained multi-workgroup scan runs (0: always)
 *   near_limit (0..2^25; 2^25) token places below this get near records
 *   hot_wgs, hot_miss_wgs (0..65536; 0)   grids of the word / merge kernels (0: as many workgroups as the chip holds)
 *   m2_split_min (>= 0; 65536), m2_split_always (0..1; 0)   when the merge kernel's two instances share a launch
 *   builder: tab_slack (2..64; 16), ph_force_overflow (>= 0; 0), ph_hot_slots (0..8192; 1024), word_weights (0..2; 0)
 *   host_threads (0..256; 0)   worker threads of a large host call (0: by the processors this process may use, at most 32)
 *   dense_csr (0..1; 1)        a large dense single-text gz_encode_batch brings only the rows' real entries over the bus and pads them
 *                              into the caller's arrays on the host; 0: the dense rows cross
 *   host_hints (0..3; 0)       fresh output arrays of a large host call: bit 0 MADV_HUGEPAGE on them, bit 1 MADV_POPULATE_WRITE per piece
 *   mask_lds (0..1; 1)         masked-LM rows: the continuation bitmap is staged in LDS by every workgroup when it fits; 0: read from memory
 *   inject_bad_alloc (>= 0; 0) test hook: the k-th allocation site reached from now on throws std::bad_alloc (the call answers GZ_E_NOMEM)
 *   bm25_hash_bits (0..62; 0)  BM25 index builds keep only the low k bits of every word's hash (0: all of it)
 *   bm25_topk_chunk (1..2^30; 2^27)  BM25 top-k: doubles of score rows held in the context's workspace at a time (queries are
 *                              scored a chunk at a time, one row at least)
 *   bm25_topk_tile (0..4096; 0)  BM25 top-k: documents per workgroup of the first selection level (0: chosen per call)
 *   bm25_search_chunk (1..2^30; 2^27)  BM25 search: doubles of candidate scores held in the context's workspace at a time (queries
 *                              are marked, scored and ranked a chunk at a time, one row at least; the chunk's bitmap words obey it too)
 *   bm25_vocab_chunk (1..2^30; 2^23)  BM25 vocabulary queries (gz_bm25_similar, gz_bm25_prefix): doubles of key rows held in the
 *                              context's workspace at a time (the words are compared and ranked a chunk at a time, one row at least)
 *   learn_table_bits (0..30; 0)  gz_bpe_learn starts its pair table at 2^k slots, fills it again at twice the size while it proves
 *                              too small and grows it no further than the load rule asks (0: sized from the word set)
 *   ngram_hash_bits (0..32; 0)  gz_ngram_index_build* and the queries of that index keep only the low k bits of every n-gram's hash
 *                              (0: all of it); with k = 1 almost every probe collides in start slot and tag: results must not change
 *   repeat_hash_bits (0..32; 0)  gz_ngram_repeats* keep only the low k bits of every (row, n-gram) hash (0: all of it); with k = 1 almost
 *                              every probe collides in start slot and tag, between rows too: results must not change
 *   diagnostic build only: diag_poison (0..1), rows_dpw, rows_dbg, ablate, diag_guard (0..2: every device buffer its own mapping
 *                              between unmapped granules, no slack -- 1 the buffer ends at its mapping's last byte, 2 it starts at the first),
 *                              diag_exact (0..1: hipMalloc of exactly the bytes asked for), diag_fresh (0..256: v > 0 fills every fresh
 *                              allocation with byte v - 1), diag_fresh_only (-1 | k: ... only the k-th allocation of the context)
 * Returns GZ_OK, or GZ_E_INVALID for an unknown key or a value out of range (nothing is changed then). */
int  gz_debug_set(gz_ctx *ctx, const char *key, int64_t value);

/* ---- batch decode ------------------------------------------------------------------------
 * gz_decoder_snapshot: build the id -> word map from the tables loaded so far, the way the reference builds
 *   `decoder` ONCE in __init__ (tokenize.py:40: {v: k for k, v in encoder.items()} -- on an id collision the last
 *   word wins).  Later gz_load_tables calls do not change the snapshot.
 * gz_decode_batch: Tokenize.decode (tokenize.py:137-139) + __convert_token_to_string (:123-124) for n_rows id lists:
 *     ' '.join(decoder.get(i, unk) for i in row).replace('@@ ', '')
 *   ids      int32, rows packed back to back; row r = ids[row_off[r] .. row_off[r+1])
 *   unk      the caller's unk_token string (the reference reads self.unk_token at call time)
 *   out      UTF-8 bytes of all rows back to back; out_off[n_rows+1] their byte offsets
 *   Returns GZ_E_CAPACITY when `capacity` is too small; out_off is valid then (out_off[n_rows] = bytes needed).
 * gz_decode_batch_device: the same with ids / row_off / out / out_off resident in HBM (total_host = bytes needed or
 *   written); out_dev may be NULL to size the output only.  As in every *_device entry point the offsets are
 *   ABSOLUTE from the base pointer: row r = ids_dev[row_off_dev[r] .. row_off_dev[r+1]), row_off_dev[0] need not be 0. */
int  gz_decoder_snapshot(gz_ctx *ctx);
int  gz_decode_batch(gz_ctx *ctx, const int32_t *ids, const int64_t *row_off, int64_t n_rows, const uint8_t *unk, int32_t unk_len,
                     uint8_t *out, int64_t capacity, int64_t *out_off);
int  gz_decode_batch_device(gz_ctx *ctx, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows, const uint8_t *unk,
                            int32_t unk_len, uint8_t *out_dev, int64_t capacity, int64_t *out_off_dev, int64_t *total_host);

/* ---- overlapping max_len windows for long documents ----------------------------------------------------------------
 * Rows and masks of the reference are made by tokenize.py:141-152: a document longer than max_len keeps token[:max_len-1] + [eos]
 * and loses the rest, a shorter one is padded (:141-146); attention_mask is ids != pad (:148-152).  These calls keep the rest: they cut ragged rows -- what an encode call
 * with GZ_MAX_LEN_NONE leaves, or bare token lists -- into rows of max_len that overlap by `stride` tokens, each framed and
 * padded like a document.  Single texts only.  With L = max_len >= 3, 0 <= stride <= L - 3, room = L - 2, step = room - stride
 * and body = row r without its first skip_front and last skip_back entries (T = max(len - skip_front - skip_back, 0) tokens):
 *     n_win   = 1 if T <= room else 1 + ceil((T - room) / step)
 *     window j: start = j * step, chunk = body[start : min(start + room, T)]
 *     row     = [bos] + chunk + [eos] + [pad] * (room - len(chunk)),  n_real = len(chunk) + 2,  mask = (row != pad)
 *   The last window is shorter, not shifted back.  bos / eos / pad are the context's current special ids (gz_table_info).
 *   Window 0 is the reference's own padded / truncated row; chunk_0 ++ chunk_1[stride:] ++ ... is the body; every later window
 *   adds at least one token.
 *   skip_front = skip_back = 1: rows of an encode call (their frame is dropped); 0: bare bodies.  Each is 0 or 1; rows are
 *   shorter than 2^31 tokens.
 *   ids / row_off          packed int32 rows as gz_decode_batch takes them: row r = ids[row_off[r] .. row_off[r+1])
 *   input_ids, attention_mask  [W, max_len] int32;  win_doc / win_start / win_n_real  [W] int32: the source row, `start`, n_real
 *   win_off [n_rows+1]     int64: row r's windows are win_off[r] .. win_off[r+1]; win_off[n_rows] = W
 *   *total_host = W on GZ_OK and on GZ_E_CAPACITY.  input_ids == NULL sizes only (win_off and *total_host are filled).  When
 *   W > capacity_windows the call returns GZ_E_CAPACITY: win_off is valid and nothing is written to the other outputs.
 *   attention_mask, win_doc, win_start, win_n_real may each be NULL.  A max_len below 3 or a stride outside [0, max_len - 3] is
 *   GZ_E_INVALID.
 * gz_window_rows_device: every pointer but total_host is a DEVICE pointer; as in every *_device entry point the offsets are
 *   ABSOLUTE from the base pointer and row_off_dev[0] need not be 0.  Ordering: both passes run on the context's stream, which
 *   every stream an encode call forks has rejoined by the time that call returns -- a gz_encode_batch_device enqueued just
 *   before on the same context (ragged layout, no gz_sync in between) has written ids_dev / row_off_dev before they are read
 *   here, as with gz_decode_batch_device.  The call returns when the windows are complete; an error the encode call deferred
 *   (GZ_E_CAPACITY) is still reported by gz_sync, and rows of such a call must not be windowed.
 * gz_window_rows: host pointers; the rows go up through the library's pinned staging, the device form runs, only win_off and
 *   the windows come back. */
int  gz_window_rows(gz_ctx *ctx, const int32_t *ids, const int64_t *row_off, int64_t n_rows,
                    int32_t max_len, int32_t stride, int32_t skip_front, int32_t skip_back,
                    int32_t *input_ids, int32_t *attention_mask, int32_t *win_doc, int32_t *win_start,
                    int32_t *win_n_real, int64_t *win_off, int64_t capacity_windows, int64_t *total_host);
int  gz_window_rows_device(gz_ctx *ctx, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows,
                           int32_t max_len, int32_t stride, int32_t skip_front, int32_t skip_back,
                           int32_t *input_ids_dev, int32_t *attention_mask_dev, int32_t *win_doc_dev, int32_t *win_start_dev,
                           int32_t *win_n_real_dev, int64_t *win_off_dev, int64_t capacity_windows, int64_t *total_host);

/* ---- short documents packed back to back into rows of max_len ("sequence packing") ------------------------------------
 * A dense [N, max_len] batch of short documents is mostly padding.  These calls lay whole documents back to back into rows of
 * max_len instead and say, cell by cell, which document a cell belongs to and where in it, so that attention can be made
 * block-diagonal.  Single texts only.  With L = max_len >= 3 and body = row r without its first skip_front and last skip_back
 * entries (T = max(len - skip_front - skip_back, 0) tokens; the skips are 0 or 1 as in gz_window_rows):
 *     seg_r = [bos] + body[:min(T, L-2)] + [eos],   len_r = min(T, L-2) + 2      (2 <= len_r <= L)
 *   seg_r is the reference's own row for that text without its padding (tokenize.py:141-146): a document longer than a row is
 *   cut the reference's way (gz_window_rows keeps the rest; the two are not combined).
 *   Next-fit, order kept: used = 0, row = 0; for r = 0 .. n_rows-1: if used + len_r > L then row += 1, used = 0;
 *   doc_row[r] = row, doc_col[r] = used, used += len_r.  R = row + 1 (0 when n_rows = 0).  A document that fills its row exactly fits.
 *   input_ids [R, L]      the segments of a row back to back, then the pad id
 *   attention_mask [R, L] input_ids != pad (tokenize.py:148-152: a real token equal to the pad id gets 0)
 *   segment_ids [R, L]    1 + the document's index within its row, by position; 0 in the padding tail only
 *   position_ids [R, L]   column - doc_col inside a segment, 0 in the tail
 *   doc_row, doc_col, doc_len [n_rows] int32
 *   pack_off              int64: packed row i holds documents pack_off[i] .. pack_off[i+1].  R + 1 entries are written; the array
 *                         must hold n_rows + 1 (R <= n_rows, and R is not known before the call)
 *   seg_off [n_rows+1]    int64: the exclusive scan of doc_len (the cumulative sequence lengths of variable-length attention)
 *   *total_host = R on GZ_OK and on GZ_E_CAPACITY.  input_ids == NULL sizes only: the five maps and *total_host are filled.  When
 *   R > capacity_rows the call returns GZ_E_CAPACITY: the maps are valid and nothing is written to the four cell arrays.
 *   attention_mask, segment_ids, position_ids, doc_row, doc_col, doc_len and seg_off may each be NULL.  max_len < 3, a skip
 *   outside {0, 1} or n_rows >= 2^31 - 4096 is GZ_E_INVALID.
 * gz_pack_rows_device: every pointer but total_host is a DEVICE pointer; offsets are ABSOLUTE from the base pointer and
 *   row_off_dev[0] need not be 0.  Ordering: as gz_window_rows_device -- all passes run on the context's stream, behind a
 *   gz_encode_batch_device (ragged layout) enqueued just before with no gz_sync in between.  The call returns when the rows
 *   are complete.
 * gz_pack_rows: host pointers; the rows go up through the library's pinned staging, the device form runs, the maps and the
 *   packed rows come back. */
int  gz_pack_rows(gz_ctx *ctx, const int32_t *ids, const int64_t *row_off, int64_t n_rows,
                  int32_t max_len, int32_t skip_front, int32_t skip_back,
                  int32_t *input_ids, int32_t *attention_mask, int32_t *segment_ids, int32_t *position_ids,
                  int32_t *doc_row, int32_t *doc_col, int32_t *doc_len, int64_t *pack_off, int64_t *seg_off,
                  int64_t capacity_rows, int64_t *total_host);
int  gz_pack_rows_device(gz_ctx *ctx, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows,
                         int32_t max_len, int32_t skip_front, int32_t skip_back,
                         int32_t *input_ids_dev, int32_t *attention_mask_dev, int32_t *segment_ids_dev, int32_t *position_ids_dev,
                         int32_t *doc_row_dev, int32_t *doc_col_dev, int32_t *doc_len_dev, int64_t *pack_off_dev, int64_t *seg_off_dev,
                         int64_t capacity_rows, int64_t *total_host);

/* ---- best-fit packing: short documents packed into FULL rows of max_len ("sequence packing", best-fit-decreasing) ----------
 * gz_pack_rows keeps the documents' order and pays for it with padding.  These calls place the same segments by
 * best-fit-decreasing on their lengths (Krell et al., 2021) and fill the rows almost completely; the output is still dense
 * [R, L] rows with segment ids, so everything behind a pack call composes unchanged.  seg_r and len_r are gz_pack_rows' own:
 *     seg_r = [bos] + body[:min(T, L-2)] + [eos],   len_r = min(T, L-2) + 2      (2 <= len_r <= L)
 * The rule, with L = max_len in [3, GZ_PACK_FIT_MAX_LEN]:
 *   Take the documents in the order (len descending, index ascending).
 *   Rows are numbered in the order they are opened.  A row carries free (L at first) and stamp (the time of its last
 *   placement, a counter t that goes up by one per placed document).
 *   A document of length l goes into the row with the smallest (free, stamp) among the rows with free >= l; if there is none
 *   it opens row R, and R += 1.
 *   Then doc_row = row, doc_col = L - free, free -= l, stamp = ++t.
 * The result depends on the lengths and the documents' order alone, never on timing: a document's place follows from its rank
 * among the documents of its length, by index.  Rows come out ordered from the longest documents to the shortest.
 *   input_ids, attention_mask, segment_ids, position_ids [R, L]    as gz_pack_rows: the segments of a row back to back in column
 *                         order, then the pad id; mask = input_ids != pad; segment_ids = 1 + the document's position within its
 *                         row, 0 in the tail only; position_ids = column - doc_col, 0 in the tail
 *   doc_row, doc_col, doc_len [n_rows] int32, indexed by document
 *   row_docs [n_rows]     int32: the document indices sorted by (doc_row, doc_col) -- the packed order
 *   pack_off              int64: packed row i holds documents row_docs[pack_off[i] .. pack_off[i+1]), in column order.  R + 1
 *                         entries are written; the array must hold n_rows + 1
 *   seg_off [n_rows+1]    int64: the exclusive scan of doc_len[row_docs[.]] -- the cumulative sequence lengths in the order the
 *                         segments lie in the rows, which is what variable-length attention takes
 *   *total_host = R on GZ_OK and on GZ_E_CAPACITY.  input_ids == NULL sizes only: the maps and *total_host are filled.  When
 *   R > capacity_rows the call returns GZ_E_CAPACITY: the maps are valid and nothing is written to the four cell arrays.
 *   attention_mask, segment_ids, position_ids, doc_row, doc_col, doc_len, row_docs and seg_off may each be NULL.  GZ_E_INVALID:
 *   gz_pack_rows' conditions, and max_len > GZ_PACK_FIT_MAX_LEN (the length histogram and the plan are sized by max_len; longer
 *   rows are refused, not handled slowly).
 * gz_pack_rows_fit_device: every pointer but total_host is a DEVICE pointer; offsets are ABSOLUTE from the base pointer.
 *   Ordering: as gz_pack_rows_device -- all passes run on the context's stream, behind a gz_encode_batch_device (ragged layout)
 *   enqueued just before with no gz_sync in between.  The call waits for the device twice: for the length histogram (the
 *   sequential decisions are made on the host, over at most max_len bins), and when the rows are complete.
 * gz_pack_rows_fit: host pointers, through the library's pinned staging like gz_pack_rows.
 * gz_pack_rows_fit_info: the host plan of the context's last best-fit call over a non-empty batch -- its time in milliseconds, its
 *   events and its final segments (zeros before the first); each pointer may be NULL.
 * Not here: pair texts, max_len > 4096, the windows of over-long documents, 16-bit outputs. */
#define GZ_PACK_FIT_MAX_LEN 4096
int  gz_pack_rows_fit(gz_ctx *ctx, const int32_t *ids, const int64_t *row_off, int64_t n_rows,
                      int32_t max_len, int32_t skip_front, int32_t skip_back,
                      int32_t *input_ids, int32_t *attention_mask, int32_t *segment_ids, int32_t *position_ids,
                      int32_t *doc_row, int32_t *doc_col, int32_t *doc_len, int32_t *row_docs, int64_t *pack_off, int64_t *seg_off,
                      int64_t capacity_rows, int64_t *total_host);
int  gz_pack_rows_fit_device(gz_ctx *ctx, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows,
                             int32_t max_len, int32_t skip_front, int32_t skip_back,
                             int32_t *input_ids_dev, int32_t *attention_mask_dev, int32_t *segment_ids_dev, int32_t *position_ids_dev,
                             int32_t *doc_row_dev, int32_t *doc_col_dev, int32_t *doc_len_dev, int32_t *row_docs_dev,
                             int64_t *pack_off_dev, int64_t *seg_off_dev, int64_t capacity_rows, int64_t *total_host);
int  gz_pack_rows_fit_info(gz_ctx *ctx, double *plan_ms, int64_t *events, int64_t *segments);

/* ---- masked-LM inputs and labels over dense rows, whole-word ----------------------------------------------------------------
 * The reference reserves <mask> as id 3 (tokenize.py:11, :35) and never produces it.  These calls take dense [n_rows, row_len]
 * int32 rows -- the input_ids of an encode, window or pack call -- and make the inputs and labels of masked-language-model
 * training: some cells are chosen, a chosen cell becomes mask_id, a random id or stays, and labels holds the original id where a
 * cell was chosen.  With whole_word = 1 the pieces of a word ("xx@@ yy@@ zz") are chosen together.  The draw is counter-based: it
 * depends on the seed and the cell's global position alone, so a batch masked in chunks, or on another GPU, gives the same cells.
 *   PROTECTED cell   its id is the context's current pad, bos or eos id (gz_table_info) or mask_id: never chosen, passes through,
 *                    label = ignore_index
 *   CONTINUATION     an id of the decoder snapshot (gz_decoder_snapshot) whose word ends in the two bytes "@@"; an id outside the
 *                    snapshot or absent from it is none (the unk fallback of decode is not used)
 *   start(r, c)      the cell is not protected, and c == 0 or cell c-1 is protected or cell c-1 is no continuation: words never
 *                    run across a row edge or a protected cell (a packed row's eos / bos pair separates its documents)
 *   head(r, c)       of an unprotected cell: the largest c' <= c with start(r, c'); with whole_word = 0, c itself
 *   g(r, c)          (row_base + r) * row_len + c, unsigned 64-bit
 *   D(g)             Philox4x32-10, counter (g & 0xffffffff, g >> 32, 0, 0), key (seed & 0xffffffff, seed >> 32), multipliers
 *                    0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; outputs x0 .. x3
 *   chosen(r, c)     the cell is unprotected and D(g(r, head(r, c))).x0 < t_sel
 *   a chosen cell    a = D(g(r, c)).x1:  a < t1 -> mask_id;  else a < t2 -> rand_lo + mulhi32(D(g(r, c)).x2, rand_hi - rand_lo);
 *                    else the id stays
 *   input_ids [n_rows, row_len]  the replaced ids, everything else copied;  labels [n_rows, row_len]  the original id where chosen,
 *   ignore_index elsewhere;  n_chosen [n_rows] int32 (may be NULL): chosen cells of the row.  The attention mask is the caller's.
 *   t_sel, t1, t2 are integers in [0, 2^32] (2^32: always), t1 <= t2; seed is any 64-bit value (a new epoch is a new seed).
 *   mask(rows[a:b], row_base = a) == mask(rows)[a:b].
 *   GZ_E_INVALID: row_len < 1, n_rows < 0, row_base < 0, (row_base + n_rows) * row_len not below 2^63, a threshold above 2^32,
 *   t1 > t2, rand_lo >= rand_hi, whole_word outside {0, 1}, ids / input_ids / labels NULL with n_rows > 0, or buffers that overlap
 *   (heads are read from neighbours' original ids): nothing is written.  GZ_E_NOTABLES without a decoder snapshot.  n_rows == 0 is
 *   GZ_OK and launches nothing.
 * gz_mask_rows_device: every pointer is a DEVICE pointer.  Ordering: one launch on the context's stream, behind an encode, window
 *   or pack call enqueued just before on the same context with no gz_sync in between.  The call returns when the rows are complete.
 * gz_mask_rows: host pointers; the rows go up through the library's pinned staging, the device form runs, the three arrays come
 *   back. */
int  gz_mask_rows(gz_ctx *ctx, const int32_t *ids, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed,
                  uint64_t t_sel, uint64_t t1, uint64_t t2, int32_t rand_lo, int32_t rand_hi, int32_t mask_id,
                  int32_t whole_word, int32_t ignore_index, int32_t *input_ids, int32_t *labels, int32_t *n_chosen);
int  gz_mask_rows_device(gz_ctx *ctx, const int32_t *ids_dev, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed,
                         uint64_t t_sel, uint64_t t1, uint64_t t2, int32_t rand_lo, int32_t rand_hi, int32_t mask_id,
                         int32_t whole_word, int32_t ignore_index, int32_t *input_ids_dev, int32_t *labels_dev,
                         int32_t *n_chosen_dev);

/* ---- span-corruption inputs and targets over dense rows, for encoder-decoder models -----------------------------------------
 * The denoising objective of T5, MASS and BART-infilling: contiguous spans of whole words are chosen, each span collapses to ONE
 * mask_id in the encoder row, and the decoder is taught to write the spans back.  The reference ships seq2seq models
 * (models/base_model; DataCollection carries dec_input_ids beside input_ids) and reserves <mask> as id 3.  Unlike gz_mask_rows the
 * pass makes every row SHORTER and emits a second, ragged sequence.  BART's full-sequence target needs no call: it is the
 * caller's original row.
 * Rows are dense [n_rows, row_len] int32; pad, bos and eos are the context's current ids (gz_table_info); mask_id is an argument.
 * Taken from the mask rule above, unchanged:
 *   PROTECTED        the cell's id is pad, bos, eos or mask_id
 *   CONTINUATION     snapshot ids (gz_decoder_snapshot) whose word ends in "@@"; an id outside the snapshot is none
 *   start(r, c), head(r, c)   as above; whole_word = 0 makes every unprotected cell its own head
 *   g(r, c)          (row_base + r) * row_len + c, unsigned 64-bit
 *   D(g)             Philox4x32-10 with the same counter, key and constants (0xD2511F53 / 0xCD9E8D57, 0x9E3779B9 / 0xBB67AE85).
 *                    Only x0 and x1 are used here; the same seed gives draws correlated with gz_mask_rows, which is harmless
 * New here:
 *   n(r, c)          the number of starts in row r at columns <= c: the word ordinal of the cell.  It counts across protected cells
 *   span at a start s = (r, c_s)   a span begins there when D(g(s)).x0 < t_start.  Its length in words is
 *                    len(s) = 1 + #{k : D(g(s)).x1 >= len_t[k]}; len_t[0 .. n_len-2] are non-decreasing integers in [0, 2^32], so
 *                    len lies in [1, n_len]; 1 <= n_len <= 16
 *   chosen(r, c)     the cell is unprotected and some start s of row r begins a span with n(s) <= n(r, c) < n(s) + len(s).  A span
 *                    may count across a protected cell: harmless, protected cells are never chosen and split runs anyway.
 *                    Equivalent: with reach(s) = n(s) + len(s) at span starts and 0 elsewhere, and far(c) the running maximum of
 *                    reach over columns <= c, a cell is chosen when it is unprotected and far(head(c)) > n(c)
 *   run              a maximal stretch of consecutive columns of chosen cells; overlapping or touching spans merge into one run
 *   E(r)             the encoder sequence, over columns in ascending order: a pad cell contributes nothing, wherever it stands; a
 *                    non-pad cell that is not chosen contributes its id; the first cell of a run contributes mask_id; the other
 *                    cells of a run contribute nothing
 *   T(r)             the target: for each run in order, mask_id followed by the run's original ids; one eos closes the whole
 *                    sequence.  Hence len(T) = n_chosen + n_spans + 1
 * Outputs -- every cell is written exactly once and nothing is zeroed beforehand:
 *   input_ids         [n_rows, row_len]    E, then pad
 *   attention_mask    [n_rows, row_len]    1 over E, then 0
 *   labels            [n_rows, dec_width]  T[:dec_width], then ignore_index
 *   decoder_input_ids [n_rows, dec_width]  ([bos] + T[:-1])[:dec_width], then pad
 *   enc_len           [n_rows] int32       len(E)
 *   dec_len           [n_rows] int32       len(T) UNCLIPPED, so the caller sees an overflow of dec_width
 *   n_spans           [n_rows] int32       the number of runs
 *   attention_mask, decoder_input_ids and the three count arrays may each be NULL.  len(E) <= row_len always; len(T) can reach
 *   row_len + 2 (nine unprotected cells, whole_word = 0, t_start = 2^32: len(T) = 11), so dec_width is an argument of its own
 *   with a clipping rule: a cell of T at or beyond dec_width is dropped.  At p = 0.15 the mean len(T) is about row_len / 10.
 *   infill(rows[a:b], row_base = a) == infill(rows)[a:b] on all seven outputs.
 *   len_t is a HOST pointer in both forms (its words travel in the kernel arguments); NULL is allowed when n_len == 1.
 *   GZ_E_INVALID: row_len < 1, n_rows < 0, row_base < 0, (row_base + n_rows) * row_len not below 2^63, dec_width < 1, t_start above
 *   2^32, n_len outside [1, 16], len_t NULL with n_len > 1, a threshold above 2^32 or thresholds that decrease, whole_word outside
 *   {0, 1}, ids / input_ids / labels NULL with n_rows > 0, or any two of the buffers overlapping: nothing is written.
 *   GZ_E_NOTABLES without a decoder snapshot.  n_rows == 0 is GZ_OK and launches nothing.
 * gz_infill_rows_device: every pointer but len_t is a DEVICE pointer.  Ordering: one launch on the context's stream, behind an
 *   encode, window or pack call enqueued just before on the same context with no gz_sync in between.  The call returns when the
 *   rows are complete.
 * gz_infill_rows: host pointers; the rows go up through the library's pinned staging, the device form runs, the arrays that were
 *   asked for come back.
 * Not here: sentinel families (the vocabulary has one <mask>), zero-length insertions, sentence permutation, remapping the
 *   segment_ids / position_ids of packed rows through the compaction (packed rows are rows: their eos bos pairs split runs). */
int  gz_infill_rows(gz_ctx *ctx, const int32_t *ids, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed,
                    uint64_t t_start, const uint64_t *len_t, int32_t n_len, int32_t mask_id, int32_t whole_word,
                    int32_t ignore_index, int32_t dec_width, int32_t *input_ids, int32_t *attention_mask, int32_t *labels,
                    int32_t *decoder_input_ids, int32_t *enc_len, int32_t *dec_len, int32_t *n_spans);
int  gz_infill_rows_device(gz_ctx *ctx, const int32_t *ids_dev, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed,
                           uint64_t t_start, const uint64_t *len_t, int32_t n_len, int32_t mask_id, int32_t whole_word,
                           int32_t ignore_index, int32_t dec_width, int32_t *input_ids_dev, int32_t *attention_mask_dev,
                           int32_t *labels_dev, int32_t *decoder_input_ids_dev, int32_t *enc_len_dev, int32_t *dec_len_dev,
                           int32_t *n_spans_dev);

/* ---- near-duplicate documents by MinHash signatures ----------------------------------------------------------------------------
 * A web corpus holds mirrors, re-posts and near-copies; every pretraining recipe removes them before it packs and masks.  Two passes:
 * gz_minhash_rows* writes num_perm 32-bit minima over the hashes of every document's token shingles (its signature; the share of
 * slots in which two signatures agree estimates the Jaccard index of the two shingle sets), gz_minhash_groups* turns a
 * [n_rows, num_perm] signature matrix into one label a document, the smallest row of its near-duplicate group.  Both are pure
 * functions of their arguments: signatures made in many batches or on many GPUs are concatenated and grouped once.  Neither needs
 * the tables or the decoder snapshot.  All arithmetic is unsigned and wraps at 32 or 64 bits.
 *   fmix32(x)        x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16
 *   H(t[0..m))       MurmurHash3_x86_32, seed 0, over the m ids as little-endian 32-bit words (the bit pattern of the int32):
 *                    h = 0;  per id:  k = t * 0xCC9E2D51;  k = rotl(k, 15);  k *= 0x1B873593;  h ^= k;  h = rotl(h, 13);
 *                    h = h * 5 + 0xE6546B64;  then  h ^= 4 m;  h = fmix32(h)
 *   c_k              fmix32(seed_lo ^ fmix32(seed_hi + 0x9E3779B9 * (k + 1))),  k = 0 .. num_perm - 1,  seed_lo = seed & 0xFFFFFFFF,
 *                    seed_hi = seed >> 32
 *   g_k(x)           fmix32(x ^ c_k): a bijection of the 32-bit values for every k
 *   body of row r    ids[row_off[r] + skip_front .. row_off[r+1] - skip_back); the skips are 0 or 1 as in gz_window_rows; a row
 *                    shorter than its skips has an empty body
 *   shingles         of a body of n ids, width w = shingle:  n >= w: the n - w + 1 runs body[i .. i + w), each hashed with H;
 *                    0 < n < w: ONE shingle, the whole body, H over n ids (the 4 m term keeps it apart from every run of w);
 *                    n == 0: none.  n_shingles[r] is that count
 *   signature        sig[r][k] = min over the shingles s of g_k(H(s)); 0xFFFFFFFF in every slot for a body without shingles.  A row
 *                    all of whose slots are 0xFFFFFFFF is EMPTY to the second pass
 *   band key         bands divides num_perm, rows_per_band = num_perm / bands; for band j of row d:
 *                    z = 0x9E3779B97F4A7C15 * (j + 1);  for v in sig[d][j * rows_per_band .. (j + 1) * rows_per_band):
 *                    z = (z ^ v) * 0xFF51AFD7ED558CCD;  z ^= z >> 32;   key = z | 1   (never 0)
 *   rep_j(d)         the smallest non-EMPTY row with the same key in band j: d itself when there is none smaller
 *   agree(a, b)      the number of slots in which the two signatures are equal
 *   edges            d -- rep_j(d) for every band j with rep_j(d) != d and agree(d, rep_j(d)) >= min_agree
 *   group[d]         the smallest row of d's connected component: d itself for a row without edges and for an EMPTY row;
 *                    *n_groups_host = the number of rows with group[d] == d
 *   Only the smallest member of a bucket is asked: two rows that share a bucket with a third, smaller one that resembles neither
 *   are NOT joined through that band (another band usually joins them).
 *   minhash(rows[a:b]) == minhash(rows)[a:b]: a row's signature depends on its body, shingle, num_perm and seed alone.
 *   ids / row_off    packed int32 rows as gz_decode_batch takes them;  signatures [n_rows, num_perm] uint32, row-major;
 *   n_shingles [n_rows] int32, may be NULL;  group [n_rows] int32.
 *   GZ_E_INVALID, each with its own sentence in gz_last_error and before anything is launched or written: n_rows < 0; a skip
 *   outside {0, 1}; shingle outside 1..32; num_perm outside 1..256; bands < 1 or a bands that does not divide num_perm; min_agree
 *   outside 1..num_perm; n_rows >= 2^31 - 4096 (the group calls); a NULL required array with n_rows > 0 (n_groups_host is always
 *   required); output arrays that overlap the input or each other; bad or decreasing row offsets (the host form).  A body of 2^31
 *   ids or more is GZ_E_LIMIT and nothing is written.  n_rows == 0 is GZ_OK, launches nothing and sets *n_groups_host = 0.
 *   Workspace of the group calls: one band at a time goes through one open-addressing table of the smallest power of two of slots
 *   that is at least 2 * n_rows, 12 bytes a slot -- 24 to 48 bytes a document --, plus one byte a document.
 * gz_minhash_rows_device / gz_minhash_groups_device: every pointer but n_groups_host is a DEVICE pointer; offsets are ABSOLUTE
 *   from the base pointer and row_off_dev[0] need not be 0.  Ordering: all passes run on the context's stream, behind a
 *   gz_encode_batch_device (ragged layout) enqueued just before with no gz_sync in between.  The calls return when their outputs
 *   are complete.
 * gz_minhash_rows: / gz_minhash_groups: host pointers; the input goes up through the library's pinned staging, the device form
 *   runs, the outputs come back.
 * Not here: shingles over words or characters of the raw text, weighted MinHash, b-bit signatures, exact Jaccard verification of
 *   candidates, a persistent index that takes appends, removing the duplicates from the rows (the caller filters). */
int  gz_minhash_rows(gz_ctx *ctx, const int32_t *ids, const int64_t *row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                     int32_t shingle, int32_t num_perm, uint64_t seed, uint32_t *signatures, int32_t *n_shingles);
int  gz_minhash_rows_device(gz_ctx *ctx, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows, int32_t skip_front,
                            int32_t skip_back, int32_t shingle, int32_t num_perm, uint64_t seed, uint32_t *signatures_dev,
                            int32_t *n_shingles_dev);
int  gz_minhash_groups(gz_ctx *ctx, const uint32_t *signatures, int64_t n_rows, int32_t num_perm, int32_t bands, int32_t min_agree,
                       int32_t *group, int64_t *n_groups_host);
int  gz_minhash_groups_device(gz_ctx *ctx, const uint32_t *signatures_dev, int64_t n_rows, int32_t num_perm, int32_t bands,
                              int32_t min_agree, int32_t *group_dev, int64_t *n_groups_host);

/* ---- learn: BPE merges and a vocabulary from a corpus -------------------------------------------------------------------------
 * gz_load_tables takes any codes and vocab file; these calls make the two from text.  Two passes: gz_wordset_* reduces a corpus to
 * its distinct words with int64 counts, gz_bpe_learn runs the merge loop on such a word set.  No tables and no decoder snapshot
 * are needed.  The reference has no learner: the rule is this library's, and it is pinned by CLOSURE -- the tokenizer loaded with
 * the learnt files segments every training word exactly as the learner left it.
 *   words            the str.split() words of every document: maximal runs of characters outside the 29 whitespace code points (the
 *                    BM25 index's word rule; no '\n' is glued to a word).  The corpus is the multiset of its words: document order
 *                    and boundaries have no other effect.  A word set lists the distinct words in first-occurrence order
 *   symbols          byte strings.  A word is its code points, the last one with the four bytes "</w>" appended (a byte that starts
 *                    no well-formed UTF-8 sequence is a symbol of its own).  The distinct initial strings, sorted by bytes ascending,
 *                    get the ids 0, 1, 2, ...; a merged symbol's string is left + right and takes the next id -- unless a symbol
 *                    with that string exists already, whose id it REUSES (strings decide, as in the tokenizer; this matters only when
 *                    the text itself holds a literal "</w>")
 *   n(l, r)          the sum over the words w of count(w) * #{ i : s_i = l, s_(i+1) = r }, every adjacent position, overlaps
 *                    included: "a a a" counts (a, a) twice
 *   a step           the best pair has the largest n; among equal counts the smallest (id_l, id_r) wins.  Learning stops after
 *                    n_merges steps, when no pair is left, or when the best count is below min_frequency.  Else every occurrence of
 *                    the pair is merged, left to right and non-overlapping, in every word: aaaa -> aa aa, aaaaa -> aa aa a
 *   pieces           of every word's final segmentation: a piece that is not its word's last is written string + "@@", the last one
 *                    without its final four bytes (finality belongs to the position); a piece's count is the sum of count(w) over
 *                    its occurrences; pieces come largest count first, then by bytes ascending; a piece equal to one of the five
 *                    default special strings (<pad> <s> </s> <mask> <unk>) is left out, since a vocab line would move its id
 *   files            codes = "#version: 0.2\n" + "left right\n" per merge; vocab = "piece count\n" per piece
 * gz_wordset_build / gz_wordset_build_device: the word set of n_docs packed documents (layout of gz_bm25_build /
 *   gz_bm25_build_device: host pointers, or DEVICE pointers with ABSOLUTE offsets and text_bytes = the bytes from text_off_dev[0];
 *   the device text is read where it lies).  gz_wordset_from_counts: the word set of n_words given words with counts[i] >= 1 -- the
 *   way shards are merged: add the counts of equal words on the host, or pass them twice, they add up.  Every given word must be
 *   exactly one word of the rule above (not empty, no whitespace): GZ_E_INVALID otherwise.  Bytes + documents stay below 2^32 and the
 *   counts sum to less than 2^62 (GZ_E_LIMIT).
 * gz_wordset_info: distinct words, their bytes, the sum of the counts (each may be NULL).  gz_wordset_words: word_off [n_words + 1],
 *   counts [n_words], bytes (each may be NULL; GZ_E_CAPACITY when bytes_cap is too small, nothing is written then).
 * gz_bpe_learn: runs the rule on the word set; 0 <= n_merges <= GZ_BPE_MERGES_MAX and min_frequency >= 1, else GZ_E_INVALID with
 *   its own sentence before anything is launched.  GZ_E_LIMIT and nothing learnt: more than 2^31 - 1 symbol positions (the code
 *   points of the distinct words), or counts times symbols summing to 2^62 or more -- no count can wrap.  info[8] = merges done,
 *   symbols, bytes of the merge strings, pieces, bytes of the piece strings, slots of the pair table at the end, keys in it, times
 *   the table was filled again or grown.  The result stays with the word set until the next gz_bpe_learn on it.
 *   The pair table is open addressing over (l << 32 | r) with int64 counts; every count is an integer sum and the best pair a
 *   function of the counts: the result does not depend on the order of the atomics.  A full table is GZ_E_LIMIT, never a dropped
 *   count.  One 32-byte readback per merge.
 * gz_bpe_learn_result: merge_off [2 * merges + 1] and merge_bytes: left and right string of every merge back to back, in learning
 *   order; piece_off [pieces + 1], piece_count [pieces], piece_bytes: the pieces as the vocab file writes them, in its order.  Each
 *   pointer may be NULL; GZ_E_CAPACITY when a byte buffer is too small (sizes: info[2], info[4]); GZ_E_INVALID before a
 *   gz_bpe_learn has succeeded.
 * A word set belongs to its context and is destroyed before it.
 * Not here: unigram or WordPiece training, a character-coverage cut-off, learning over pre-tokenized ids, multi-GPU learning (shards
 *   merge through their word sets). */
#define GZ_BPE_MERGES_MAX (1 << 20)
typedef struct gz_wordset gz_wordset;
int  gz_wordset_build(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, int64_t n_docs, gz_wordset **out);
int  gz_wordset_build_device(gz_ctx *ctx, const uint8_t *text_dev, const int64_t *text_off_dev, int64_t n_docs, int64_t text_bytes,
                             gz_wordset **out);
int  gz_wordset_from_counts(gz_ctx *ctx, const uint8_t *words, const int64_t *word_off, const int64_t *counts, int64_t n_words,
                            gz_wordset **out);
int  gz_wordset_info(gz_wordset *ws, int64_t *n_words, int64_t *n_bytes, int64_t *total);
int  gz_wordset_words(gz_wordset *ws, int64_t *word_off, int64_t *counts, uint8_t *bytes, int64_t bytes_cap);
void gz_wordset_destroy(gz_wordset *ws);
int  gz_bpe_learn(gz_wordset *ws, int64_t n_merges, int64_t min_frequency, int64_t info[8]);
int  gz_bpe_learn_result(gz_wordset *ws, int64_t *merge_off, uint8_t *merge_bytes, int64_t merge_cap, int64_t *piece_off,
                         int64_t *piece_count, uint8_t *piece_bytes, int64_t piece_cap);

/* ---- token n-gram overlap against a held-out set ("decontamination") ------------------------------------------------------------
 * Between deduplication and packing a pretraining recipe finds the training documents that share token n-grams with a held-out set
 * -- benchmark questions, test splits, canaries -- and how much of each document is affected (GPT-3: 13-grams; PaLM: 8-grams;
 * Llama-2: the share of tokens covered by matching 10-grams).  An INDEX of the held-out rows' n-grams lives in device memory; a
 * query probes it once per token position.  Everything is exact: a hash decides where to look, never whether two n-grams are equal.
 * Neither call needs the tables or the decoder snapshot.  To find which benchmark items leaked, swap the roles: index a corpus shard
 * and query the benchmark.
 *   body of row r    ids[row_off[r] + skip_front .. row_off[r+1] - skip_back); the skips are 0 or 1 as in gz_window_rows; a row
 *                    shorter than its skips has an empty body
 *   n-grams          of a body of m ids, width n in 1..32: the max(0, m - n + 1) runs body[i .. i + n).  A body shorter than n has
 *                    NONE (unlike the one short shingle of gz_minhash_rows: a shorter run is not evidence of leakage)
 *   index            S = the set of all n-grams of all reference bodies; first(g) = the smallest reference row that holds g.  The
 *                    index owns a copy of the reference ids: the caller's buffers may be freed after the build.  An index with S
 *                    empty (no rows, or every body shorter than n) is legal
 *   query, row r     with body q of m ids:  n_grams[r] = max(0, m - n + 1);  hit(i) = q[i .. i + n) is in S;
 *                    n_hits[r] = the number of i with hit(i);
 *                    n_covered[r] = the number of body positions t for which some i has hit(i) and i <= t < i + n;
 *                    first_hit[r] = the smallest i with hit(i), -1 when there is none;
 *                    first_ref[r] = first(q[first_hit .. first_hit + n)), -1 when there is no hit;
 *                    covered (optional) = one uint8 per id of the input, covered[k] belongs to ids[k] for k in
 *                    [row_off[0], row_off[n_rows]): 1 on covered body positions, 0 elsewhere, the skipped frame cells included
 *   overlap(rows[a:b]) == overlap(rows)[a:b]: a row's outputs depend on its own body and the index alone; shards concatenate.
 *   The outputs are a pure function of (reference rows, n, query rows): not of launch geometry, scheduling or the hash.
 *   hash             two MurmurHash3_x86_32 streams over the n ids (little-endian 32-bit words), seeds 0 and 0x9E3779B9:
 *                    per id  k = t * 0xCC9E2D51;  k = rotl(k, 15);  k *= 0x1B873593;  and for both streams  h ^= k;  h = rotl(h, 13);
 *                    h = h * 5 + 0xE6546B64;  then each  h ^= 4 n;  h = fmix32(h);   h64 = H_0 << 32 | H_0x9E3779B9, cut to its low
 *                    ngram_hash_bits bits when that switch is set;  tag = h64 >> 32;  start slot = h64 & (slots - 1)
 *   table            open addressing, linear probing, slots = the smallest power of two that is at least twice the reference n-gram
 *                    positions (never more than half full), 8 bytes a slot: tag << 32 | (position + 1), position = the global
 *                    index of the n-gram's first id in the index's id copy; 0 = free.  Insert: 64-bit compare-and-swap on a free
 *                    slot; on a taken slot with an equal tag the n ids at the occupant's position are compared with the inserter's:
 *                    equal -- the slot is lowered to the inserter's position by a 64-bit atomic minimum (equal tags: the packed
 *                    order is the position order) and the insert is done; else the next slot.  Every occurrence of an n-gram ends
 *                    in one slot, which holds its smallest position; first(g) is the row of that position (a binary search in the
 *                    reference offsets): membership and first do not depend on the order of the inserts
 *   memory           the index: 4 bytes a reference id, 8 bytes a reference row, 8 bytes a slot -- 20 to 36 bytes a reference token
 *                    with one position a token; workspace of a build or a query: 16 bytes a row
 *   ids / row_off    packed int32 rows as gz_decode_batch takes them;  the five per-row outputs int32 [n_rows], each may be NULL;
 *                    covered uint8, may be NULL.
 *   GZ_E_INVALID, each with its own sentence in gz_last_error and before anything is launched or written: n_rows < 0; 2^31 reference
 *   rows or more; a skip outside {0, 1}; n outside 1..32; a NULL index or out handle; NULL ids or row_off with n_rows > 0; output
 *   arrays that overlap the input or each other; bad or decreasing row offsets (the host form); an index of another context.
 *   GZ_E_LIMIT and nothing built or written: reference ids that total 2^32 - 1 or more (a slot holds position + 1 in 32 bits: shard the
 *   held-out set), or a body of 2^31 ids or more.  n_rows == 0 is GZ_OK and launches nothing (a build then gives the empty index).
 * gz_ngram_index_build: host pointers; the rows go up through the library's pinned staging.  gz_ngram_index_build_device: DEVICE
 *   pointers; offsets are ABSOLUTE from the base pointer and row_off_dev[0] need not be 0.  Ordering: every pass runs on the
 *   context's stream, behind a gz_encode_batch_device (ragged layout) enqueued just before with no gz_sync in between.  The index
 *   is complete on return.
 * gz_ngram_index_info: info[8] = n, reference rows, reference ids, n-gram positions, distinct n-grams, table slots, device bytes of
 *   this index, device bytes of all live n-gram indexes of its context.
 * gz_ngram_index_destroy: frees the index (NULL is fine).  An index belongs to its context and is destroyed before it; gz_destroy
 *   frees what is left.
 * gz_ngram_overlap: host pointers, the outputs come back.  gz_ngram_overlap_device: every pointer a DEVICE pointer, offsets ABSOLUTE
 *   as above, same ordering; the call returns when its outputs are complete.  Both use the index's n; the skips are the call's own.
 * Not here: appending to a live index, saving and loading one, multi-GPU indexes (shards query one replicated index), removing or
 *   splitting the contaminated spans, text or character n-grams, exact whole-document deduplication, approximate (Bloom) tables,
 *   per-reference-row "seen" marks. */
typedef struct gz_ngram_index gz_ngram_index;
int  gz_ngram_index_build(gz_ctx *ctx, const int32_t *ids, const int64_t *row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                          int32_t n, gz_ngram_index **out);
int  gz_ngram_index_build_device(gz_ctx *ctx, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows, int32_t skip_front,
                                 int32_t skip_back, int32_t n, gz_ngram_index **out);
int  gz_ngram_index_info(gz_ngram_index *index, int64_t info[8]);
void gz_ngram_index_destroy(gz_ngram_index *index);
int  gz_ngram_overlap(gz_ctx *ctx, gz_ngram_index *index, const int32_t *ids, const int64_t *row_off, int64_t n_rows, int32_t skip_front,
                      int32_t skip_back, int32_t *n_grams, int32_t *n_hits, int32_t *n_covered, int32_t *first_hit, int32_t *first_ref,
                      uint8_t *covered);
int  gz_ngram_overlap_device(gz_ctx *ctx, gz_ngram_index *index, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows,
                             int32_t skip_front, int32_t skip_back, int32_t *n_grams_dev, int32_t *n_hits_dev, int32_t *n_covered_dev,
                             int32_t *first_hit_dev, int32_t *first_ref_dev, uint8_t *covered_dev);

/* ---- align: word spans, word ids and aligned token labels ("token classification") --------------------------------------------
 * The reference's return_offset says which tokens belong to which word (tokenize.py:105-117); a tagger over word-segmented text
 * (NER, POS) also needs where each word stands in its text, the word of every cell of a row, and labels [N, max_len] made from word
 * labels or from annotated character spans.  Three calls, single texts only, every output an exact integer.
 * Definitions:
 *   words of a document   the matches of \S+\n? over the document, Unicode whitespace as str.isspace (what the encoder splits on);
 *                         a document boundary ends a word.  Document d has W_d words.
 *   per-word quantities   word j has c_j >= 1 pieces (gz_word_token_counts); C_j = the exclusive scan of c within the document;
 *                         T_d = the sum of c_j.
 *   row geometry          a row is (doc, start) with room = max_len - 2.  Its chunk is the body tokens start .. min(start + room,
 *                         T_doc) - 1, empty when start >= T_doc.  Cell 0 is bos, cells 1..n the chunk, cell n + 1 eos, the rest pad.
 *                         start = 0 is the reference's padded / truncated row (tokenize.py:141-146); (win_doc, win_start) of
 *                         gz_window_rows are its windows.
 * gz_word_spans / gz_word_spans_device: where each word stands.  text / text_off [n_docs + 1] as gz_wordset_build[_device] takes
 *   them (the device form: ABSOLUTE offsets and text_bytes = the bytes from text_off_dev[0]; text_off_dev[0] need not be 0).
 *   unit: 0 code points (Python str indices), 1 bytes.
 *   span [W, 2] int32     [begin, end) of the \S+ part of every word, relative to its document's start.  The glued line feed is not
 *                         inside: the word ends with one exactly when the character at `end` is "\n".
 *   word_off [n_docs + 1] int64: the index of every document's first word; word_off[n_docs] = W.
 *   A code point index is the number of bytes that are not 10xxxxxx since the document's start: exact for Python strings encoded
 *   with surrogatepass (lone surrogates and 4-byte characters included); for bytes that are not UTF-8 the byte unit is exact and the
 *   code point unit is that count.  Nothing leaves its document.
 *   *total_host = W on GZ_OK and on GZ_E_CAPACITY.  span == NULL sizes only (word_off and *total_host are filled).  W >
 *   capacity_words is GZ_E_CAPACITY: word_off is valid and span is untouched.  A document of 2^31 bytes or more, or W >= 2^31,
 *   is GZ_E_LIMIT.  For structurally valid UTF-8 word_off equals doc_first of gz_word_token_counts on the same batch.
 * gz_align_rows / gz_align_rows_device: word ids and labels, cell by cell.
 *   counts [W] int32, word_off [n_docs + 1] int64: exactly what gz_word_token_counts returns.  row_doc, row_start [n_rows] int32:
 *   row_doc == NULL means row r is document r and n_rows == n_docs; row_start == NULL means every start is 0.  max_len >= 3.
 *   word_labels [W] int32 (optional), indexed as counts.  continuation: 0 ignore, 1 same, 2 map (cont_map [n_map] int32).
 *   word_ids, labels [n_rows, max_len] int32, n_real [n_rows] int32; each may be NULL; labels requires word_labels.
 *     chunk cell holding body token t: word_ids = the j with C_j <= t < C_{j+1};  bos, eos, pad: word_ids = -1, labels = ignore_index
 *     label of a chunk cell: the first piece (t == C_j) carries word_labels[j]; a later piece carries ignore_index (ignore),
 *     word_labels[j] (same), or (map) cont_map[v] for 0 <= v < n_map, else v unchanged, with v = word_labels[j].
 *   The rule is per token, not per row: a window that begins inside a word begins with a continuation cell.  n_real = chunk length + 2.
 *   The host form refuses (GZ_E_INVALID, each with its own sentence): a count below 1, decreasing offsets, a row_doc outside
 *   [0, n_docs), a negative row_start, max_len < 3, labels without word_labels, map mode without a map.  The device form takes
 *   n_words = word_off_dev[n_docs] - word_off_dev[0] as an argument and trusts what it cannot read: counts, offsets, row_doc and
 *   row_start are the caller's promise (offsets and documents out of range are clamped into the arrays, a negative start reads as 0).
 * gz_span_labels / gz_span_labels_device: word labels from character annotations.
 *   span, word_off of gz_word_spans.  marks [S, 3] int32: (begin, end, label) in the same unit, grouped by document with mark_off
 *   [n_docs + 1] int64, in any order within a document.  scheme: 0 plain, 1 BIO.
 *   word_labels [W] int32; mark_words [S, 2] int32: the doc-relative [first word, last word + 1) a mark overlaps, or (-1, -1).
 *   Either may be NULL.  A mark with end <= begin overlaps nothing; otherwise it overlaps word [b, e) iff begin < e and b < end
 *   (touching is not overlapping; a mark over whitespace only, or past the document's end, overlaps nothing).  A word's owner is
 *   the SMALLEST MARK INDEX among the marks overlapping it.  plain: the owner's label, else `outside`.  BIO (labels >= 0): outside is
 *   0; 2 * label + 1 when the previous word of the document has a different owner or there is none, else 2 * label + 2 -- a mark whose
 *   first word was taken by an earlier mark still begins with a B.  The host form refuses a negative label under BIO and bad offsets;
 *   the device form takes n_words and n_marks and trusts what it cannot read.
 * Ordering: every pass runs on the context's stream; the calls return when their outputs are complete.
 * Not here: sentence pairs; character spans of sub-word pieces (an unk piece has no length in the tables); a device form of
 *   gz_word_token_counts; IOBES and other schemes; an encode call that aligns on the device in one go. */
int  gz_word_spans(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, int64_t n_docs, int32_t unit, int32_t *span,
                   int64_t *word_off, int64_t capacity_words, int64_t *total_host);
int  gz_word_spans_device(gz_ctx *ctx, const uint8_t *text_dev, const int64_t *text_off_dev, int64_t n_docs, int64_t text_bytes,
                          int32_t unit, int32_t *span_dev, int64_t *word_off_dev, int64_t capacity_words, int64_t *total_host);
int  gz_align_rows(gz_ctx *ctx, const int32_t *counts, const int64_t *word_off, int64_t n_docs, const int32_t *row_doc,
                   const int32_t *row_start, int64_t n_rows, int32_t max_len, const int32_t *word_labels, int32_t continuation,
                   const int32_t *cont_map, int32_t n_map, int32_t ignore_index, int32_t *word_ids, int32_t *labels, int32_t *n_real);
int  gz_align_rows_device(gz_ctx *ctx, const int32_t *counts_dev, const int64_t *word_off_dev, int64_t n_docs, int64_t n_words,
                          const int32_t *row_doc_dev, const int32_t *row_start_dev, int64_t n_rows, int32_t max_len,
                          const int32_t *word_labels_dev, int32_t continuation, const int32_t *cont_map_dev, int32_t n_map,
                          int32_t ignore_index, int32_t *word_ids_dev, int32_t *labels_dev, int32_t *n_real_dev);
int  gz_span_labels(gz_ctx *ctx, const int32_t *span, const int64_t *word_off, int64_t n_docs, const int32_t *marks,
                    const int64_t *mark_off, int32_t scheme, int32_t outside, int32_t *word_labels, int32_t *mark_words);
int  gz_span_labels_device(gz_ctx *ctx, const int32_t *span_dev, const int64_t *word_off_dev, int64_t n_docs, int64_t n_words,
                           const int32_t *marks_dev, const int64_t *mark_off_dev, int64_t n_marks, int32_t scheme, int32_t outside,
                           int32_t *word_labels_dev, int32_t *mark_words_dev);

/* ---- pair windows: question-context windows with answer positions ("extractive question answering", "reranking") ----------------
 * The reference's pair row is <s> question </s></s> context </s> cut at max_len (tokenize.py:141-146): an answer behind the cut is
 * lost.  gz_window_rows keeps a long document whole but puts no question in front and makes no type ids.  These calls repeat the
 * question in front of EVERY window of its context, say which cells are question and which context, and carry an answer's body
 * positions into row columns -- the (start, end) target of an extractive QA model.  One question may serve many contexts (a
 * query and its k retrieved documents for a cross-encoder).
 * Inputs: question rows and context rows, both packed int32 rows as gz_window_rows takes them, with ONE skip_front / skip_back pair
 *   (each 0 or 1) applied to both; an optional q_row [N]: pair r uses question row q_row[r]; NULL means pair r uses question r, and
 *   then NQ == N.  L = max_len, s = stride, mq = max_query_len.
 *   The call is valid iff L >= 5, 0 <= mq <= L - 5 and 0 <= s <= L - 5 - mq.  Otherwise it returns GZ_E_INVALID and writes nothing.
 * For pair r, let Q be the question body of Tq tokens and body the context body of T tokens.  A row shorter than its skips has an
 * empty body.
 *     q      = min(Tq, mq)                    (the question keeps its FIRST q tokens)
 *     room   = L - 4 - q   (>= s + 1)         step = room - s  (>= 1)
 *     n_win  = 1 if T <= room else 1 + ceil((T - room) / step)
 *     window j: start = j * step, chunk = body[start : min(start + room, T)], n = len(chunk)
 *     row    = [bos] + Q[:q] + [eos, eos] + chunk + [eos] + [pad] * (room - n)      n_real = q + 4 + n
 *     mask   = (row != pad)                                    (tokenize.py:148-152, as everywhere)
 *     type   = 0 on columns < q + 2, 1 on columns q + 2 .. n_real - 1, the pad id behind them
 *     ctx_col = q + 3                                          (column of chunk[0])
 *   The last window is shorter, not shifted back.  bos / eos / pad are the context's current special ids.
 * Answers are optional: ans [N, 2] int32, holding the [a0, a1) body positions of the context.
 *   An answer is present iff 0 <= a0 < a1 <= T.  Anything else means "no answer"; no input is invalid on the device.
 *   Window j holds the answer iff start <= a0 and a1 <= start + n.
 *   If it does, start_pos = ctx_col + a0 - start, end_pos = ctx_col + a1 - 1 - start and has_answer = 1.
 *   Otherwise start_pos = end_pos = 0 (the bos column, the SQuAD convention) and has_answer = 0.
 *   Without ans, all three outputs may be NULL (they are not written then).
 * Laws:
 *   1. Equality with the reference.  A pair with T >= 1, Tq <= mq and q + 4 + T <= L has one window, and its row and mask are those of
 *      the reference __call__(question, context, max_len=L), which is what gz_encode_batch with pair texts returns.  If n_real < L the
 *      type row is the reference's token_type_ids too.  If n_real == L the reference puts the eos id into the last cell (its
 *      token-type pass overruns); here that cell is 1 and every other cell agrees: the ONE deviation.  T == 0 (the reference leaves
 *      None cells) is outside the law.
 *   2. Chunks rejoin.  chunk_0 ++ chunk_1[s:] ++ ... is the context body.  Every later window adds at least one token.
 *   3. Question placement.  Columns 1 .. q of every window of pair r are Q[:q].
 *   4. Answers.  An answer with a1 - a0 <= s + 1 is held by at least one window.  An answer longer than room is held by none.  Where
 *      one is held, row[start_pos : end_pos + 1] == body[a0:a1].
 * gz_pair_window_rows / gz_pair_window_rows_device, with the window calls' conventions:
 *   q_ids / q_off [NQ + 1], ids / row_off [N + 1]   packed rows, ABSOLUTE offsets from their base pointers (off[0] need not be 0)
 *   input_ids, attention_mask, token_type_ids   [W, max_len] int32
 *   win_pair, win_start, win_n_real, win_q_len, start_pos, end_pos, has_answer   [W] int32: the pair, `start`, n_real, q and the answer
 *   win_off [N + 1]        int64: pair r's windows are win_off[r] .. win_off[r+1]; win_off[N] = W
 *   *total_host = W on GZ_OK and on GZ_E_CAPACITY.  input_ids == NULL sizes only (win_off and *total_host are filled).  When
 *   W > capacity_windows the call returns GZ_E_CAPACITY: win_off is valid and nothing is written to the other outputs.  Each
 *   secondary output (everything but input_ids and win_off) may be NULL.  n_rows == 0 is GZ_OK and launches nothing.
 *   GZ_E_INVALID, each with its own sentence in gz_last_error and before anything is launched or written: a negative n_rows,
 *   n_questions or capacity_windows; a skip outside {0, 1}; max_len < 5; max_query_len outside [0, max_len - 5]; stride outside
 *   [0, max_len - 5 - max_query_len]; q_row NULL with n_questions != n_rows.  GZ_E_NOTABLES without tables.
 *   The device form: every pointer but total_host is a DEVICE pointer.  It cannot read q_row beforehand: an entry outside [0, NQ) is an
 *   EMPTY question (q = 0), and no address is formed from it.  The host form refuses such an entry, and bad or decreasing offsets of
 *   either row set (GZ_E_INVALID); rows go up through the library's pinned staging, only win_off and the windows come back.
 *   Ordering: both passes run on the context's stream, as gz_window_rows_device -- rows of a gz_encode_batch_device enqueued just
 *   before on the same context are complete when they are read here.  The call returns when the windows are complete.
 * gz_span_tokens / gz_span_tokens_device: the word ranges gz_span_labels returns as body-token ranges.
 *   counts [W] int32, word_off [n_docs + 1] int64 of gz_word_token_counts; mark_words [S, 2] int32 from 0 and mark_off [n_docs + 1]
 *   int64 of gz_span_labels.  span_tokens [S, 2] int32: for a mark with the word range [f, e) of its document, with C the exclusive
 *   scan of that document's counts (C[W_d] = T_d), (C[f], C[e]) = [first token of the first word, last token of the last word + 1)
 *   in body positions; a (-1, -1) range stays (-1, -1).  The host form refuses a count below 1, a range that is neither (-1, -1) nor ordered inside the batch's words, and bad
 *   offsets; the device form takes n_words and n_marks, trusts what it cannot read and clamps a range into its document's words.
 * Not here: several answers per pair; answers finer than words (an unk piece has no length in the tables); truncating the question
 *   from the left, "longest first" truncation; windows aligned to word boundaries; the reference's overrun and None quirks beyond law
 *   1; pair forms of packs, masks, infill and dropout; 16-bit outputs; multi-GPU forms (shards concatenate). */
int  gz_pair_window_rows(gz_ctx *ctx, const int32_t *q_ids, const int64_t *q_off, int64_t n_questions, const int32_t *ids,
                         const int64_t *row_off, int64_t n_rows, const int32_t *q_row, const int32_t *ans, int32_t max_len,
                         int32_t stride, int32_t max_query_len, int32_t skip_front, int32_t skip_back, int32_t *input_ids,
                         int32_t *attention_mask, int32_t *token_type_ids, int32_t *win_pair, int32_t *win_start,
                         int32_t *win_n_real, int32_t *win_q_len, int32_t *start_pos, int32_t *end_pos, int32_t *has_answer,
                         int64_t *win_off, int64_t capacity_windows, int64_t *total_host);
int  gz_pair_window_rows_device(gz_ctx *ctx, const int32_t *q_ids_dev, const int64_t *q_off_dev, int64_t n_questions,
                                const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows, const int32_t *q_row_dev,
                                const int32_t *ans_dev, int32_t max_len, int32_t stride, int32_t max_query_len, int32_t skip_front,
                                int32_t skip_back, int32_t *input_ids_dev, int32_t *attention_mask_dev, int32_t *token_type_ids_dev,
                                int32_t *win_pair_dev, int32_t *win_start_dev, int32_t *win_n_real_dev, int32_t *win_q_len_dev,
                                int32_t *start_pos_dev, int32_t *end_pos_dev, int32_t *has_answer_dev, int64_t *win_off_dev,
                                int64_t capacity_windows, int64_t *total_host);
int  gz_span_tokens(gz_ctx *ctx, const int32_t *counts, const int64_t *word_off, int64_t n_docs, const int32_t *mark_words,
                    const int64_t *mark_off, int32_t *span_tokens);
int  gz_span_tokens_device(gz_ctx *ctx, const int32_t *counts_dev, const int64_t *word_off_dev, int64_t n_docs, int64_t n_words,
                           const int32_t *mark_words_dev, const int64_t *mark_off_dev, int64_t n_marks, int32_t *span_tokens_dev);

/* ---- repeats: n-gram repetition inside a document ("quality filtering") ---------------------------------------------------------------
 * Beside deduplication and decontamination a pretraining recipe drops documents that repeat themselves: boiler-plate, menu spam,
 * "aaaa aaaa aaaa" pages, degenerate generations.  The rule of Gopher (Rae et al., 2021, table A1), taken over by MassiveText,
 * RefinedWeb and FineWeb, asks for the share of a document inside its MOST FREQUENT n-gram (n = 2..4) and inside n-grams that occur
 * MORE THAN ONCE (n = 5..10).  One call answers both for up to 16 widths.  It compares a document with itself: gz_minhash_rows compares
 * documents with each other, and an n-gram index is one set for all rows that does not count.  Neither form needs the tables or the
 * decoder snapshot.
 *   body of row r    q = ids[row_off[r] + skip_front .. row_off[r+1] - skip_back), m ids; the skips are 0 or 1 exactly as in
 *                    gz_minhash_rows and gz_ngram_overlap; a row shorter than its skips has an empty body
 *   widths           a list of 1..16 distinct integers, each in 1..32, in the caller's order; k indexes it
 *   n-grams          for width n the G = max(0, m - n + 1) runs q[i:i+n].  A body shorter than n has none.  c(g) = the number of
 *                    positions whose n-gram is g; occurrences may overlap, so [5, 5, 5] holds (5, 5) twice.  first(g) = the smallest
 *                    such position.
 *   per row r and width k, all int32 and laid out [K, N] (K = n_widths, N = n_rows; entry k * N + r):
 *     n_grams[k, r]    = G
 *     n_distinct[k, r] = the number of different n-grams.  G - n_distinct is then the number of later occurrences, which is what some
 *                        implementations of the Gopher rule count
 *     n_repeated[k, r] = the positions i with c(q[i:i+n]) >= 2.  The first occurrence counts too.
 *     n_covered[k, r]  = the body tokens t with some repeated position i, i <= t < i + n.  Each token counts once.
 *     top_count[k, r]  = max c(g), or 0 when G == 0
 *     top_pos[k, r]    = first(g) of the n-gram with the largest count; among equal counts it is the one with the smallest first.
 *                        -1 when G == 0
 *   covered (optional) one uint16 per id of the input in the input's own layout: covered[i] belongs to ids[i] for i in
 *                    [row_off[0], row_off[n_rows]).  Bit k is set when the token is covered at widths[k].  0 on frame cells.
 *   repetition(rows[a:b]) == repetition(rows)[:, a:b]: a row's outputs depend on its own body and widths alone, never on another
 *   row, even an identical neighbour; shards concatenate.  The outputs are a pure function of (rows, widths): not of launch geometry,
 *   scheduling or the hash.  A hash decides where to look, never whether two n-grams are equal, nor whether they stand in the same row.
 *   table            one table a call, allocated once and cleared per width: open addressing, linear probing, slots = the smallest
 *                    power of two that is at least twice the call's n-gram positions at the smallest width (never more than half
 *                    full).  A slot has two parts: 8 bytes, tag << 32 | (position + 1), position = the global index of the n-gram's
 *                    first id in the caller's flat ids relative to row_off[0], 0 = free; and 4 bytes in a parallel array, the
 *                    occurrence count.  The key of a slot is (row, n-gram).  Insert: 64-bit compare-and-swap on a free slot; on a
 *                    taken slot whose tag agrees the occupant is the same key only if its position lies inside this row's n-gram
 *                    positions AND the n ids are equal: then the slot is lowered to the smaller position by a 64-bit atomic minimum;
 *                    otherwise the next slot.  Then the count of the slot the occurrence ended in is incremented.  A slot once taken
 *                    holds one key for good, so every occurrence of a key ends in the same slot, whatever the order.  Query: every
 *                    position probes and reads (first, c); the row's top is the maximum of c << 32 | (0xFFFFFFFF - first); coverage
 *                    comes from the ballot of the repeated positions as gz_ngram_overlap derives it from its hits.  All
 *                    order-dependent state is an integer minimum, maximum or sum.
 *   hash             the 64-bit hash of gz_ngram_index_build over the n ids, then the row mixed in:  h64 ^= mix(r),
 *                    mix(r): x = r + 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;
 *                    x ^ x >> 31 (the finalizer of splitmix64);  h64 is cut to its low repeat_hash_bits bits when that switch is set;
 *                    tag = h64 >> 32;  start slot = h64 & (slots - 1).  Correctness does not depend on it.
 *   memory           workspace of the context, kept between calls: 12 bytes a slot -- 24 to 48 bytes a token with one position a
 *                    token -- plus 16 bytes a row for piece counts and their scan, plus 8 bytes a row where a body has more than
 *                    4096 n-grams and top_count or top_pos is asked for
 *   ids / row_off    packed int32 rows as gz_decode_batch takes them (any integers: word ids give word n-grams); widths on the HOST
 *                    in both forms; every output pointer may be NULL.
 *   GZ_E_INVALID, each with its own sentence in gz_last_error, before anything is launched and with the outputs untouched: n_rows < 0;
 *   a skip outside {0, 1}; n_widths outside 1..16; NULL widths; a width outside 1..32; a repeated width; NULL ids or row_off with
 *   n_rows > 0; bad or decreasing row offsets (the host form); output arrays that overlap the input or each other.
 *   GZ_E_LIMIT and nothing written: a body of 2^31 ids or more, or 2^32 - 1 ids or more in the call (a slot holds position + 1 in 32
 *   bits: shard the rows).  n_rows == 0 is GZ_OK and touches nothing.
 * gz_ngram_repeats: host pointers; the rows go up through the library's pinned staging and the outputs come back.
 * gz_ngram_repeats_device: ids, row_off and the outputs DEVICE pointers; offsets are ABSOLUTE from the base pointer and row_off_dev[0]
 *   need not be 0.  Ordering: every pass runs on the context's stream, behind a gz_encode_batch_device (ragged layout) enqueued just
 *   before with no gz_sync in between; the call returns when its outputs are complete.
 * Not here: character weighting of the shares, line and paragraph duplicates and the other Gopher heuristics (word lengths, symbol
 *   ratios, stop words), which work on text; a table in LDS for short rows; removing the repeated spans (the caller reads covered);
 *   repetition across documents (gz_minhash_rows, gz_ngram_index_build); multi-GPU forms (shards concatenate). */
int  gz_ngram_repeats(gz_ctx *ctx, const int32_t *ids, const int64_t *row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                      const int32_t *widths, int32_t n_widths, int32_t *n_grams, int32_t *n_distinct, int32_t *n_repeated,
                      int32_t *n_covered, int32_t *top_count, int32_t *top_pos, uint16_t *covered);
int  gz_ngram_repeats_device(gz_ctx *ctx, const int32_t *ids_dev, const int64_t *row_off_dev, int64_t n_rows, int32_t skip_front,
                             int32_t skip_back, const int32_t *widths, int32_t n_widths, int32_t *n_grams_dev, int32_t *n_distinct_dev,
                             int32_t *n_repeated_dev, int32_t *n_covered_dev, int32_t *top_count_dev, int32_t *top_pos_dev,
                             uint16_t *covered_dev);

/* ---- text pre-pass: the string filters of genz_tokenize/preprocess.py on packed documents ----
 *   GZ_PP_HTML     remove_html          preprocess.py:5-9     re.sub(r'<[^>]*>', '', txt)
 *   GZ_PP_UNICODE  convert_unicode      preprocess.py:16-36   base letter + combining tone mark -> precomposed letter
 *   GZ_PP_PUNCT    remove_punctuations  preprocess.py:39-44   drop string.punctuation
 *   GZ_PP_EMOJI    remove_emoji         preprocess.py:47-72   drop the listed ranges, then ' '.join(s.split())
 *   GZ_PP_URL      remove_URL           preprocess.py:75-80   re.sub(r'http\S+', '', txt)
 * `ops[n_ops]` are applied in order to every document (vncore_tokenize, preprocess.py:83-89, talks to an external Java
 * server and is not part of this library).  Input and output use the packed layout of gz_encode_batch (the output can
 * be handed straight to it).  No filter grows a document, so capacity = input bytes always suffices; GZ_E_CAPACITY
 * is returned otherwise and out_off is still valid.  No tables are needed.
 * gz_preprocess_batch_device: the same with text / offsets / outputs resident in HBM; text_bytes = bytes of the input
 * text = text_off_dev[n_docs] - text_off_dev[0]; *total_host = bytes written (or needed); out_dev may be NULL to size the
 * output only.  Offsets are ABSOLUTE from the base pointer (document d = text_dev[text_off_dev[d] ..), exactly like
 * gz_encode_batch_device; text_off_dev[0] need not be 0.  The output offsets start at 0. */
#define GZ_PP_HTML    1
#define GZ_PP_UNICODE 2
#define GZ_PP_PUNCT   3
#define GZ_PP_EMOJI   4
#define GZ_PP_URL     5
int  gz_preprocess_batch(gz_ctx *ctx, const int32_t *ops, int32_t n_ops, const uint8_t *text, const int64_t *text_off,
                         int64_t n_docs, uint8_t *out, int64_t capacity, int64_t *out_off);
int  gz_preprocess_batch_device(gz_ctx *ctx, const int32_t *ops, int32_t n_ops, const uint8_t *text_dev, const int64_t *text_off_dev,
                                int64_t n_docs, int64_t text_bytes, uint8_t *out_dev, int64_t capacity, int64_t *out_off_dev,
                                int64_t *total_host);

/* ---- model-feed hand-off --------------------------------------------------------------------
 * Zero-copy export of an output buffer to a framework through DLPack.  gz_block_create takes ownership of a pointer
 * obtained from gz_device_alloc (refcount 1); gz_block_dlpack returns a malloc'ed DLManagedTensor (dlpack.h layout,
 * device type kDLROCM) that holds one more reference and whose deleter is a C function of this library, safe to call
 * at interpreter shutdown; the HBM allocation is freed when the last reference goes.  The fields a consumer sees
 * are the reference's DataCollection names (models/bert/dataset.py:7-28): input_ids, attention_mask, token_type_ids. */
typedef struct gz_block gz_block;
int   gz_block_create(gz_ctx *ctx, void *dptr, gz_block **out);
void  gz_block_release(gz_block *block);
void *gz_block_dlpack(gz_block *block, int32_t ndim, const int64_t *shape, int32_t dtype_code, int32_t dtype_bits);
/* Destructor for a PyCapsule named "dltensor" that wraps gz_block_dlpack's result (pass its address to PyCapsule_New):
 * a capsule nobody consumed gives its reference to the block back; a consumed one ("used_dltensor") is left alone.
 * (No reference counterpart: models/bert/dataset.py:7-28 builds tf tensors from Python lists.) */
void gz_dlpack_capsule_destructor(void *capsule);

/* Multi-GPU exchange step (one process per GPU, RCCL over xGMI).  rank 0 creates an id, every rank calls
 * gz_comm_init with it; gz_gather_rows sends each rank's [n_rows, row_len] int32 device block to `root`,
 * which receives them back to back in rank order (grouped ncclSend/ncclRecv: each peer uses its own link). */
int  gz_comm_unique_id(uint8_t id_out[128]);
/* The exchange operations (gz_compact_rows, gz_gather_rows, gz_expand_rows) run on a stream of their own: they start
 * when the encode call they belong to has finished and overlap the kernels of LATER encode calls; an encode call in
 * turn waits for every exchange operation issued before it (it may overwrite the buffers they read).  By default they
 * belong to the most recent encode call; gz_exchange_select(ctx, 1) makes the following ones belong to the call
 * before it (double buffering: enqueue step k, then exchange step k-1).  gz_sync waits for both streams. */
int  gz_exchange_select(gz_ctx *ctx, int back);
int  gz_comm_init(gz_ctx *ctx, const uint8_t id[128], int rank, int world);
int  gz_gather_rows(gz_ctx *ctx, const int32_t *send_dev, int64_t n_rows_local, int32_t row_len,
                    int32_t *recv_dev, const int64_t *rows_per_rank, int root);
/* Every gz_gather_rows is bracketed by a pair of events on the exchange stream: this call synchronises that stream and
 * returns, oldest first, the time from the moment the gather COULD start (the encode call it belongs to was done, earlier
 * exchange operations had drained) to its last byte received / sent, of the last (up to 64, up to `max`) gathers, then
 * forgets them. */
int  gz_exchange_timing_history(gz_ctx *ctx, double *out_ms, int32_t max, int32_t *n_out);

/* Compact form of dense rows for the exchange step: most of a [n_rows, row_len] block is padding, so a rank sends
 * only the n_real[i] leading entries of every row (+ the counts) and the root re-creates padding and mask.
 *   gz_compact_rows   rows_dev [n_rows,row_len] + n_real_dev [n_rows] -> out_dev (concatenated leading entries);
 *                     *total_host = number of entries written (the call synchronises the context's stream).
 *                     PRECONDITION, of gz_compact_rows[16] and gz_compact_block alike: every n_real[i] lies in [0, row_len].
 *                     The compact calls do not check it (the rows are the caller's own): a larger or a negative count
 *                     reads beyond the row, behind the last row beyond rows_dev.
 *   gz_expand_rows    the inverse on the receiving side: compact_dev + n_real_dev -> ids_dev, mask_dev
 *                     ([n_rows,row_len] each; padding = the pad id of the loaded tables, mask = id != pad) */
int  gz_compact_rows(gz_ctx *ctx, const int32_t *rows_dev, const int32_t *n_real_dev, int64_t n_rows, int32_t row_len,
                     int32_t *out_dev, int64_t *total_host);
int  gz_expand_rows(gz_ctx *ctx, const int32_t *compact_dev, const int32_t *n_real_dev, int64_t n_rows, int32_t row_len,
                    int32_t *ids_dev, int32_t *mask_dev);
/* The same with 16-bit entries (half the bytes on the link): only when every id of the loaded vocabulary fits 16 bits
 * (GZ_E_LIMIT otherwise); lossless. */
int  gz_compact_rows16(gz_ctx *ctx, const int32_t *rows_dev, const int32_t *n_real_dev, int64_t n_rows, int32_t row_len,
                       uint16_t *out_dev, int64_t *total_host);
int  gz_expand_rows16(gz_ctx *ctx, const uint16_t *compact_dev, const int32_t *n_real_dev, int64_t n_rows, int32_t row_len,
                      int32_t *ids_dev, int32_t *mask_dev);
/* One rank's whole message of the exchange step as ONE block (one ncclSend per peer and shard):
 *     block_dev = [ int32 n_real[n_rows] | uint32 first[n_rows] | the rows' real entries, `bits` (16 | 32) bits each ]
 * row r's entries are the n_real[r] ones from entry first[r] on (round 4: no `first` -- the receiver scanned n_real again).
 * gz_compact_block writes it from dense rows (total_host receives the number of entries; the block is 2 n_rows + ceil(total * bits /
 * 32) int32 words long), gz_expand_block is the inverse on the receiving side: `total_entries` is the entry count the block was
 * announced with (what gz_block_total / gz_compact_block returned on the sending side).  A block comes from another process: a row
 * that claims more than row_len entries, or entries beyond total_entries -- a truncated block, one written in another layout -- is
 * written as padding only, never followed, and the next gz_sync answers GZ_E_INVALID.
 * gz_encode_emit_block arms the NEXT encode call (a dense one: GZ_E_INVALID from that call otherwise) to leave its block in block_dev
 * (2 n_docs + ceil(n_docs * max_len * bits / 32) words at most) as part of the call itself: the scan of the row lengths and the
 * compact kernel run right behind the call's kernels on the call's own stream (beside the NEXT call's kernels, on the exchange
 * stream, the same work costs those kernels more than it takes here), and nothing of it waits for the host.  gz_block_total(back)
 * waits for the encode call `back` (0..2) calls ago and returns its block's number of entries (GZ_E_INVALID when that call emitted
 * none).  An arming holds for ONE gz_encode_batch_device[_h] call -- whether that call makes the block or fails; block_dev == NULL disarms. */
int  gz_encode_emit_block(gz_ctx *ctx, int32_t *block_dev, int32_t bits);
int  gz_block_total(gz_ctx *ctx, int32_t back, int64_t *total_host);
int  gz_compact_block(gz_ctx *ctx, const int32_t *rows_dev, const int32_t *n_real_dev, int64_t n_rows, int32_t row_len,
                      int32_t bits, int32_t *block_dev, int64_t *total_host);
int  gz_expand_block(gz_ctx *ctx, const int32_t *block_dev, int32_t bits, int64_t n_rows, int32_t row_len, int64_t total_entries,
                     int32_t *ids_dev, int32_t *mask_dev);

/* ---- BM25 / BM25Plus ranking (genz_tokenize/ranking.py of the reference, numpy only) ---------------------------------
 * An index over packed documents: str.split() words (maximal runs of code points that are not among the 29 of str.isspace();
 * terms are compared by their exact UTF-8 bytes), fieldLens, document frequencies and per-document term counts, built on the
 * GPU and owned by the context it was built on (destroy every index before its context; gz_destroy frees what is left).
 *   gz_bm25_build          host text / offsets (document d = text[text_off[d] .. text_off[d+1]))
 *   gz_bm25_build_device   the same resident in HBM (offsets ABSOLUTE from the base pointer, text_bytes = text_off_dev[n_docs] -
 *                          text_off_dev[0]); a document outside those bytes is refused with GZ_E_INVALID.  The index keeps a copy
 *                          of the text: the caller's buffers may go once the call has returned.
 *   gz_bm25_build_ex       gz_bm25_build with flags.  0: the same index, buffer for buffer.  GZ_BM25_POSITIONS: a POSITIONAL index,
 *                          which additionally owns seq, uint32 [n_words]: the term id of every word of every document, documents in
 *                          id order, words in str.split() order -- what a phrase search reads.  Its word offsets (document d =
 *                          seq[woff[d] .. woff[d + 1]), the exclusive scan of fieldLens) are derived on the device by the first call
 *                          that reads positions and dropped by every change, as the postings are.  Every call below maintains seq
 *                          with the guarantees it gives for the other arrays: gz_bm25_append puts the batch's term ids behind the
 *                          index's words (the buffer grows geometrically), gz_bm25_remove moves the kept documents' words into a
 *                          fresh buffer, gz_bm25_compact renumbers them -- after it seq, like everything else, is the fresh
 *                          positional build's -- and an error leaves the index as it was.  A positional build ends in the form a
 *                          compaction gives: it never needs the documents' text again, so its text copy holds the terms' bytes only
 *                          (out[0] of gz_bm25_footprint) and a compacted positional index equals a fresh positional build of its
 *                          documents in every buffer, gz_bm25_footprint's three numbers included.  Another flag bit: GZ_E_INVALID.
 *   gz_bm25_build_device_ex  gz_bm25_build_device with the same flags
 *   gz_bm25_flags          the flags the index was built with
 *   gz_bm25_sequence       the positional store read back into host memory: terms_out[n_words] = seq (n_words of gz_bm25_info; ids as
 *                          gz_bm25_lookup answers them) and doc_off_out[n_docs + 1] = the word offsets.  GZ_E_INVALID on an index
 *                          built without GZ_BM25_POSITIONS.  The index is not modified (the word offsets may be derived).
 *   gz_bm25_info           documents, distinct terms (those some document has), words (all documents)
 *   gz_bm25_field_lengths  fieldLens (ranking.py:21): words of every document, out[n_docs]
 *   gz_bm25_lookup         query words (packed like documents, host buffers) -> term id (-1 when no document has it) and df
 *                          (documents that contain it, ranking.py:29-31)
 *   gz_bm25_score          scores[n_queries * n_docs] (row q = query q) into host memory: query q = the term ids
 *                          terms[query_off[q] .. query_off[q+1]) (-1 allowed), in order, with the caller's idf of every word
 *                          (the reference computes idf with a scalar np.log on the host, ranking.py:31).
 *                          params = { k1 + 1, k1, 1 - b, b, avgFieldLen, delta } as the caller computes them; plus = 0 BM25
 *                          (ranking.py:33-45), 1 BM25Plus (:52-63).  Every score is the reference's IEEE double to the bit.
 *   gz_bm25_score_device   the same into scores_dev (HBM): enqueued on the context's stream, gz_sync waits for it
 *   gz_bm25_topk           the k' = min(k, n_docs) best documents of every query, row-major [n_queries, k'] into doc_out (int64)
 *                          and score_out: with S the scores of gz_bm25_score, row q is np.argsort(-S[q], kind="stable")[:k'] and
 *                          S[q] at those ids, original bits.  Higher scores first, +0.0 and -0.0 tie, every NaN below every number,
 *                          ties to the lower document index.  Query arguments as gz_bm25_score.  k < 1: GZ_E_INVALID; k' above
 *                          GZ_BM25_TOPK_MAX: GZ_E_LIMIT.  Nothing outside the [n_queries, k'] outputs is written.  The scores stay
 *                          in HBM (a chunk of queries at a time, switch bm25_topk_chunk); only ids and scores cross to the host.
 *   gz_bm25_topk_device    the same into doc_out_dev / score_out_dev (HBM): enqueued on the context's stream, gz_sync waits for it
 *   gz_bm25_search         the matching documents of every query, ranked: document d MATCHES query q when it holds at least one of
 *                          q's words (term ids >= 0; repeated words count once; this does not depend on params).  count_out[q]
 *                          (int64) = the matching documents, which may exceed k.  Row q of doc_out / score_out [n_queries, k'],
 *                          k' = min(k, n_docs): gz_bm25_topk's total order restricted to the matching documents -- with S the
 *                          scores of gz_bm25_score, [i for i in np.argsort(-S[q], kind="stable") if d_i matches][:k'] and S[q] at
 *                          those ids, original bits; positions behind count_out[q] hold id -1 and the NaN 0x7FF8000000000000.
 *                          Query arguments and errors as gz_bm25_topk (k < 1: GZ_E_INVALID; k' above GZ_BM25_TOPK_MAX:
 *                          GZ_E_LIMIT; GZ_E_NOMEM).  Nothing outside the [n_queries, k'] and [n_queries] outputs is written.
 *                          The matching documents come from term-major postings, a derived structure the first search or match
 *                          count builds on the device and later ones reuse; every successful append, removal or compaction
 *                          drops it and the next search builds it again.  Only the matching documents are scored and ranked (a
 *                          chunk of queries at a time, switch bm25_search_chunk).  On any error the index answers every call as
 *                          before, whether or not the postings were built.
 *   gz_bm25_search_device  the same with the three outputs in HBM: enqueued on the context's stream, gz_sync waits for it (the call
 *                          itself waits for each chunk's counts, which size its workspace)
 *   gz_bm25_match_count    count_out[q] of gz_bm25_search alone (host memory); for a query of one word it is the word's df
 *   gz_bm25_search_bool    gz_bm25_search with another notion of a match.  With R = the distinct terms of query q, X = the distinct
 *                          terms ex_terms[ex_off[q] .. ex_off[q + 1]) (ids as gz_bm25_lookup answers them; -1 is ignored; ex_off
 *                          NULL: X is empty) and W(d) = the terms of document d:
 *                            mode GZ_BM25_MATCH_ANY: d matches iff R and W(d) share a term, and X and W(d) share none;
 *                            mode GZ_BM25_MATCH_ALL: d matches iff R is not empty, every term of R is in W(d), and X and W(d)
 *                            share none -- a query without words matches nothing, and so does one with a word that no document
 *                            holds (term -1).
 *                          A term both in R and in X excludes every document that holds it.  Repeated words count once for
 *                          matching (and as often as they occur in the scores S).  Excluded terms never enter a score: S, the
 *                          order, count_out, the rows and their -1 / NaN padding are gz_bm25_search's with this set of matching
 *                          documents.  GZ_E_INVALID: a mode other than the two, an excluded id outside [-1, n_terms), ex_off
 *                          (n_queries + 1 offsets into ex_terms) decreasing, a non-empty range with ex_terms NULL; k and every
 *                          other error as gz_bm25_search.  On any error the index answers every call as before.  In mode ALL only
 *                          the postings of each query's rarest word are marked; a filter stage then clears, from the marked
 *                          documents, those that lack a required term or hold an excluded one (signature, then pair table),
 *                          and everything behind it is gz_bm25_search's.  With mode ANY and no excluded term the work is exactly
 *                          gz_bm25_search's.
 *   gz_bm25_search_bool_device  the same with the three outputs in HBM, as gz_bm25_search_device
 *   gz_bm25_match_count_bool    count_out[q] of gz_bm25_search_bool alone (host memory)
 *   gz_bm25_search_phrase  gz_bm25_search_bool with an exact phrase per query on top.  With P = ph_terms[ph_off[q] .. ph_off[q + 1])
 *                          (the ex_terms / ex_off conventions: absolute int64 offsets, ids as gz_bm25_lookup answers them, -1 = a
 *                          word no document holds; ph_off NULL: no phrases, the call is gz_bm25_search_bool) and seq(d) the term
 *                          ids of document d's words in order: d matches q iff it matches under mode and ex_terms as there AND P
 *                          is empty or seq(d)[i .. i + len(P)) == P for some i.  So a phrase with a term -1 matches nothing, a
 *                          phrase of one word means "holds this word", a phrase never matches across two documents, and a phrase
 *                          with repeated words finds overlapping starts.  The phrase is a filter only: its terms enter no score;
 *                          S, the order, count_out, the rows and their padding are gz_bm25_search's with this set of matching
 *                          documents.  Needs an index built with GZ_BM25_POSITIONS (else GZ_E_INVALID, also for empty phrases);
 *                          GZ_E_INVALID: a phrase id outside [-1, n_terms), ph_off decreasing, a non-empty range with ph_terms
 *                          NULL; GZ_E_LIMIT: a phrase of more than GZ_BM25_PHRASE_MAX words; every other error as
 *                          gz_bm25_search_bool.  On any error the index answers every call as before.  One more stage behind the
 *                          marking and the filter: a wave per 64-bit word of a row's bitmap rejects a marked document that lacks
 *                          a phrase term (signature, pair table), else walks the document's range of seq, 64 start positions a
 *                          trip, comparing the phrase's rarest term first; everything behind the bitmap is gz_bm25_search's.
 *   gz_bm25_search_phrase_device  the same with the three outputs in HBM, as gz_bm25_search_device
 *   gz_bm25_match_count_phrase    count_out[q] of gz_bm25_search_phrase alone (host memory)
 *   gz_bm25_snippets       where the words of a query stand INSIDE given documents: a positional index's second reader.  terms /
 *                          query_off as gz_bm25_search (a term -1 matches nothing, a repeated term changes nothing; the length of a
 *                          query has no limit), ids[n_queries * k] (int64, host memory) the documents of every query -- what
 *                          gz_bm25_search or gz_bm25_topk wrote goes in as it is -- and pair r = q * k + j is (query q, document
 *                          ids[r]).  With seq(d) the term ids of document d's words in order, n their number and h[p] = 1 where
 *                          seq(d)[p] is a term of the query: over the starts s in [0, max(1, n - width + 1)), hits(s) = the sum of
 *                          h[s .. s + width) inside the document; start_out[r] = the SMALLEST s with the largest hits(s),
 *                          hits_out[r] = that sum (both int32).  A document without words gives (0, 0), n <= width gives start 0
 *                          and all of the document's hits, a query without terms gives hits 0 and start 0; a window never
 *                          reaches into the next document.  An id -1 (the padding of gz_bm25_search) gives start -1, hits 0.
 *                          GZ_E_INVALID: an index without GZ_BM25_POSITIONS, a term outside [-1, n_terms), query_off decreasing,
 *                          width < 1, k < 0, an id outside [-1, n_docs) (checked before any launch: nothing is written);
 *                          GZ_E_LIMIT: 2^31 pairs or more; GZ_E_HIP: the index's fieldLens and seq contradict each other.
 *                          n_queries * k == 0: GZ_OK, nothing written.  Derives the word offsets if the index has none and
 *                          nothing else: no postings are built.  A wave per pair: the query's terms sit in the lanes, 64 at a
 *                          time; hits(0) is counted, then the starts are walked 64 a trip -- hits(s) - hits(s - 1) =
 *                          h[s - 1 + width] - h[s - 1], a wave prefix sum plus a carry, a wave arg-max with ties to the lower
 *                          start kept across trips only when strictly greater.  The index is not modified.
 *   gz_bm25_snippets_device  the same with ids, start_out and hits_out in HBM: the doc_out of gz_bm25_search_device goes straight in.
 *                          The ids are not looked at by the host: an id outside [-1, n_docs) is treated as -1 (start -1, hits 0)
 *                          and never read through.  The call returns after the kernel has run (its check of the word offsets is
 *                          read back).
 *   gz_bm25_occurrences    every place of a query word in the documents of gz_bm25_snippets' pairs (host memory): pair r owns
 *                          [pair_off_out[r], pair_off_out[r + 1]) of pos_out / word_out (int32), ascending in pos_out -- the
 *                          positions p with h[p] = 1 -- and word_out = the FIRST place of that term in the query (an index into
 *                          terms[query_off[q] ..), so a repeated query word is reported under its first place).  An id -1 owns
 *                          nothing.  Sizes first, as gz_bm25_terms: a call with pos_out == NULL fills pair_off_out[n_queries * k + 1]
 *                          (pair_off_out[0] = 0) and T = its last entry is the room the two arrays need; a call with pos_out !=
 *                          NULL and cap >= T fills all three.  cap < T: GZ_E_CAPACITY, nothing written.  GZ_E_LIMIT: 2^32
 *                          occurrences or more in one call, or 2^31 pairs; every other error as gz_bm25_snippets (no width).  A
 *                          count kernel (ballot popcounts per pair), the scan of the counts, a fill kernel that writes at the
 *                          pair's base + the set bits of the ballot below the lane: no atomic decides an order.
 *   gz_bm25_search_near    gz_bm25_search_phrase with a proximity constraint per query on top: the positional index's third reader.
 *                          With S = the SET of near_terms[near_off[q] .. near_off[q + 1]) (the ex_terms / ex_off conventions; a
 *                          repeated id counts once; near_off NULL: no near sets, the call is gz_bm25_search_phrase), w =
 *                          near_window[q] (int64 [n_queries], read only when near_off is not NULL) and seq(d) the term ids of
 *                          document d's n words in order: d matches q iff it matches under mode, ex_terms and ph_terms as there
 *                          AND S is empty or some min(w, n) consecutive words of d hold every term of S, in any order.  So a set
 *                          with a term -1 matches nothing, neither does a window smaller than the set; a window of n or more means
 *                          "holds all of them", a window never reaches into a neighbouring document, and a set of one term with
 *                          window 1 is that one-word phrase.  A filter only: the near terms enter no score; scores, order,
 *                          count_out, the rows and their padding are gz_bm25_search's with this set of matching documents.  Needs
 *                          an index built with GZ_BM25_POSITIONS (else GZ_E_INVALID, also for empty sets); GZ_E_INVALID: a near id
 *                          outside [-1, n_terms), near_off decreasing, a non-empty range with near_terms NULL, near_window NULL, a
 *                          window < 1 in a row that has near terms; GZ_E_LIMIT: a range of more than GZ_BM25_NEAR_MAX entries;
 *                          every other error as gz_bm25_search_phrase.  On any error the index answers every call as before.  One
 *                          more stage behind the phrase stage: a wave per 64-bit word of a row's bitmap, lane j holding term j of
 *                          the set, rejects a marked document that lacks a term (signature, pair table) and else walks the
 *                          document's range of seq 64 positions a trip: for every term a ballot of its occurrences, a lane's last
 *                          occurrence at or before it from the ballot or from a carry of the trips before, the minimum over the
 *                          terms = the start of the shortest window ending there; the document stays at the first trip with a
 *                          window of at most w words.  Without near terms nothing of it is launched, allocated or derived.
 *   gz_bm25_search_near_device  the same with the three outputs in HBM, as gz_bm25_search_device
 *   gz_bm25_match_count_near    count_out[q] of gz_bm25_search_near alone (host memory)
 *   gz_bm25_cover          the shortest passage of a document that holds all the query words it has.  terms / query_off / ids / k and
 *                          the pairs as gz_bm25_snippets, but a query is a SET of at most GZ_BM25_NEAR_MAX entries (a repeated id
 *                          counts once, -1 is ignored).  With R = the terms of the set that document ids[r] holds at all:
 *                          words_out[r] = |R|; over all windows [i, j) of the document's words that hold every term of R, the one
 *                          with the smallest (j - i, i): start_out[r] = i, len_out[r] = j - i (all int32, host memory).  R empty
 *                          gives (0, 0, 0); an id -1 gives start -1, length 0, words 0.  words_out[r] == the distinct known terms
 *                          of the query says that the cover is complete.  GZ_E_INVALID: an index without GZ_BM25_POSITIONS, a
 *                          term outside [-1, n_terms), query_off decreasing, k < 0, an id outside [-1, n_docs) (checked before
 *                          any launch: nothing is written); GZ_E_LIMIT: a query range of more than GZ_BM25_NEAR_MAX entries, 2^31
 *                          pairs or more; GZ_E_HIP: the index contradicts itself.  n_queries * k == 0: GZ_OK, nothing written.
 *                          Derives the word offsets if the index has none and nothing else.  A wave per pair: the terms the
 *                          document lacks (signature, pair table) leave the set, then the walk of gz_bm25_search_near keeps the
 *                          wave minimum of (length << 32) | start.  The index is not modified.
 *   gz_bm25_cover_device   the same with ids and the three outputs in HBM: the doc_out of gz_bm25_search_near_device (or of any
 *                          _device search) goes straight in.  The ids are not looked at by the host: an id outside [-1, n_docs) is
 *                          treated as -1 and never read through.  The call returns after the kernel has run.
 *   gz_bm25_search_groups  gz_bm25_search_bool over WORD GROUPS: a group is a set of alternative terms that counts as one query word
 *                          -- the primitive under fuzzy, prefix and synonym search.  Query q = the groups group_off[q] ..
 *                          group_off[q + 1]; group g = the alternatives alt_terms[alt_off[g] .. alt_off[g + 1]) with the idf
 *                          group_idf[g] (absolute indices, as query_off / ex_off; host memory).  With A_g the DISTINCT alternatives
 *                          of g that are not -1 (a repeat counts once) and c(a, d) the count of term a in document d:
 *                          f_g(d) = the sum of c(a, d) over A_g.  mode GZ_BM25_MATCH_ANY: d matches iff some f_g(d) > 0;
 *                          GZ_BM25_MATCH_ALL: iff the query has a group and every f_g(d) > 0 (an empty A_g: nothing matches);
 *                          ex_terms / ex_off as gz_bm25_search_bool.  The score is gz_bm25_score's sum with group g where a word
 *                          stands: f = f_g(d), idf = group_idf[g], groups in order, a group listed twice summed twice; the caller
 *                          computes group_idf from df_g = the documents with f_g > 0 (gz_bm25_match_count over A_g as a query).
 *                          With every group a single term the outputs equal gz_bm25_search_bool's bit for bit.  Outputs, order,
 *                          padding and k as gz_bm25_search.  GZ_E_INVALID (checked before any launch, nothing written): NULL
 *                          group_off / params / outputs, NULL alt_off or group_idf with groups, NULL alt_terms with alternatives,
 *                          decreasing or negative offsets, a term outside [-1, n_terms), a bad mode, k < 1, bad ex_off;
 *                          GZ_E_LIMIT: a group of more than GZ_BM25_GROUP_MAX distinct alternatives, k' above GZ_BM25_TOPK_MAX.
 *                          On the device (gz_groups.inc): the flat alternative list is marked as a word list; with
 *                          GZ_BM25_MATCH_ALL only the group with the smallest sum of postings-list lengths; a filter and a score
 *                          kernel add up a group's alternatives per document, behind a 256-bit mask of the group's signature bits
 *                          that rejects most documents without a probe.  The index is not modified.
 *   gz_bm25_search_groups_device  the same with the three outputs in HBM, as gz_bm25_search_device
 *   gz_bm25_match_count_groups    count_out[q] of gz_bm25_search_groups alone (host memory; no idf, no params, no k)
 *   gz_bm25_append        n_docs more documents behind the index's own (host text / offsets as gz_bm25_build): afterwards the index
 *                          answers every call above exactly as one built over all the documents in one go does -- term ids, df,
 *                          fieldLens, scores and top-k to the bit.  The batch's words are resolved against the live term table,
 *                          only its unknown words are de-duplicated, and the per-document arrays grow at their tails; the index's
 *                          buffers have a capacity and grow geometrically, so the work is proportional to the batch unless a
 *                          buffer grows.  n_docs == 0: GZ_OK, nothing changes.  On any error (GZ_E_NOMEM, GZ_E_INVALID for
 *                          offsets that decrease or leave the text, GZ_E_LIMIT when all bytes + all documents would reach 2^32)
 *                          the index answers as before the call.  The index keeps the hash mask it was built with.
 *   gz_bm25_append_device  the same for a batch resident in HBM (offsets ABSOLUTE from the base pointer, text_bytes =
 *                          text_off_dev[n_docs] - text_off_dev[0], as gz_bm25_build_device); GZ_E_LIMIT is answered before
 *                          anything is read
 *   gz_bm25_remove         the documents doc_ids[0 .. n_ids) (host memory; any order, duplicates allowed) leave the index: afterwards
 *                          it answers every call above exactly as one built over the remaining documents, in their old order, does
 *                          -- df, fieldLens, counts, scores and top-k to the bit.  Documents are renumbered: new id = old id - the
 *                          number of removed documents before it.  Term ids may differ from that build's (it numbers terms by first
 *                          occurrence in what remains); a word no remaining document has is answered -1 with df 0 by
 *                          gz_bm25_lookup and is not counted by gz_bm25_info, and a later append brings it back.  The work is
 *                          proportional to the index: fieldLens, signatures and entries are compacted into fresh buffers of the
 *                          same capacity, the pair table is filled again.  The index's copy of the text is not touched: its
 *                          device memory is not reclaimed, and the removed bytes still count towards GZ_E_LIMIT of an append,
 *                          until gz_bm25_compact.
 *                          n_ids == 0: GZ_OK, nothing changes.  On any error (GZ_E_INVALID for an id outside [0, n_docs),
 *                          GZ_E_NOMEM) the index answers as before the call.
 *   gz_bm25_remove_device  the same for ids resident in HBM
 *   gz_bm25_compact        the index becomes the one gz_bm25_build gives for its current documents: afterwards it answers every
 *                          call above exactly as that build does, and now gz_bm25_lookup's term ids are that build's too (terms
 *                          are numbered by first occurrence in the current documents; dead terms leave the term table).  The text
 *                          copy shrinks to the live terms' bytes -- the figure GZ_E_LIMIT of an append counts -- and every buffer
 *                          to the size a build gives it for the same counts: device memory that appends and removals left behind
 *                          is given back.  Device-only, no text is tokenised or hashed again.  Appends and removals work on the
 *                          compacted index as before.  On GZ_E_NOMEM the index answers as before the call.
 *   gz_bm25_terms          the vocabulary, of an index in any state, which is not modified: the T live terms (T = n_terms of
 *                          gz_bm25_info) in the order of their first occurrence in the current documents -- the order of the ids
 *                          that gz_bm25_lookup answers once the index is compacted -- as term_off[T + 1] (term i = bytes[term_off[i]
 *                          .. term_off[i + 1]), term_off[0] = 0) and df[T].  Sizes first: a call with bytes == NULL fills term_off
 *                          and df (either may be NULL), and B = term_off[T] is the room the bytes need; a second call with
 *                          bytes != NULL and bytes_cap >= B copies them (and fills term_off / df again where they are not NULL).
 *                          bytes_cap < B: GZ_E_CAPACITY, nothing written.  term_off and bytes both NULL: GZ_E_INVALID.
 *   gz_bm25_similar        typo-tolerant word lookup over the vocabulary of an index in any state, which is not modified.  The ids are
 *                          those of gz_bm25_terms (T live terms in first-occurrence order).  words / word_off: n_words packed words
 *                          as for gz_bm25_lookup (host buffers; a word is taken whole, whitespace included).  For word w the
 *                          matching terms are those within max_edits (0 .. GZ_BM25_EDIT_MAX) of it in Levenshtein distance -- unit
 *                          cost insertion, deletion, substitution of code points, no transposition; the empty word's distance to a
 *                          term is the term's length.  count_out[w] = their number (it may exceed k'), and row w of the
 *                          [n_words, k'] outputs, k' = min(k, T), holds the first k' of them in ascending (distance, -df, id) with
 *                          their distances and dfs; positions from count_out[w] on hold id -1, distance -1, df 0.  Every word is
 *                          compared with every live term on the device (gz_vocab.inc: a bit-parallel recurrence, a lane per term),
 *                          a chunk of words at a time (switch bm25_vocab_chunk), and ranked by gz_bm25_topk's selection; only the
 *                          outputs cross.  GZ_E_INVALID: k < 1, max_edits out of range, decreasing offsets, bytes that are not
 *                          structurally valid UTF-8 (lead and continuation bytes; surrogates pass); GZ_E_LIMIT: a word of more
 *                          than GZ_BM25_EDIT_MAX code points, k' above GZ_BM25_TOPK_MAX.  Nothing is written on an error.
 *   gz_bm25_prefix         the same for "terms that start with the word": byte-wise, which for structurally valid UTF-8 is
 *                          code-point-wise; the empty word matches every term.  Order (-df, id); outputs, padding, k and errors as
 *                          gz_bm25_similar (no distances, a word of any length, its bytes are not examined).
 *   gz_bm25_term_bytes     the bytes of listed terms only: ids[n_ids] are ids of gz_bm25_terms' numbering, -1 = no term (no bytes).
 *                          Sizes first, as gz_bm25_terms: a call with bytes == NULL fills off_out[n_ids + 1] (term i of the list =
 *                          bytes[off_out[i] .. off_out[i + 1]), off_out[0] = 0); a call with bytes != NULL and bytes_cap >=
 *                          off_out[n_ids] gathers them on the device and copies them (off_out is filled again unless NULL).
 *                          bytes_cap too small: GZ_E_CAPACITY, nothing written.  GZ_E_INVALID: an id outside [-1, T), off_out and
 *                          bytes both NULL.  The vocabulary as a whole is not read back.
 *   gz_bm25_footprint      host bookkeeping, no device work: out[0] = bytes of the text copy in use (what GZ_E_LIMIT of an append
 *                          counts), out[1] = terms held in the term table, dead ones included, out[2] = device bytes allocated
 *                          to the index's ten buffers, capacities included, to its postings while they exist and, for a
 *                          positional index, to seq and (while they exist) the word offsets
 * Switch bm25_hash_bits (gz_debug_set, read when an index is built): keep only the low k bits of the words' hash (collisions are
 * resolved by comparing bytes, so results do not change). */
#define GZ_BM25_TOPK_MAX 1024
#define GZ_BM25_MATCH_ANY 0
#define GZ_BM25_MATCH_ALL 1
#define GZ_BM25_POSITIONS 1
#define GZ_BM25_PHRASE_MAX 64
#define GZ_BM25_NEAR_MAX 64
#define GZ_BM25_EDIT_MAX 64
#define GZ_BM25_GROUP_MAX 64
typedef struct gz_bm25 gz_bm25;
int  gz_bm25_build(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, int64_t n_docs, gz_bm25 **out);
int  gz_bm25_build_device(gz_ctx *ctx, const uint8_t *text_dev, const int64_t *text_off_dev, int64_t n_docs, int64_t text_bytes,
                          gz_bm25 **out);
int  gz_bm25_build_ex(gz_ctx *ctx, const uint8_t *text, const int64_t *text_off, int64_t n_docs, int32_t flags, gz_bm25 **out);
int  gz_bm25_build_device_ex(gz_ctx *ctx, const uint8_t *text_dev, const int64_t *text_off_dev, int64_t n_docs, int64_t text_bytes,
                             int32_t flags, gz_bm25 **out);
int  gz_bm25_flags(gz_bm25 *index, int32_t *flags);
int  gz_bm25_sequence(gz_bm25 *index, int32_t *terms_out /* n_words */, int64_t *doc_off_out /* n_docs + 1 */);
int  gz_bm25_info(gz_bm25 *index, int64_t *n_docs, int64_t *n_terms, int64_t *n_words);
int  gz_bm25_field_lengths(gz_bm25 *index, int32_t *out);
int  gz_bm25_lookup(gz_bm25 *index, const uint8_t *words, const int64_t *word_off, int64_t n_words, int32_t *term_out, int32_t *df_out);
int  gz_bm25_score(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                   const double params[6], int32_t plus, double *scores);
int  gz_bm25_score_device(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                          const double params[6], int32_t plus, double *scores_dev);
int  gz_bm25_topk(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                  const double params[6], int32_t plus, int64_t k, int64_t *doc_out, double *score_out);
int  gz_bm25_topk_device(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                         const double params[6], int32_t plus, int64_t k, int64_t *doc_out_dev, double *score_out_dev);
int  gz_bm25_search(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                    const double params[6], int32_t plus, int64_t k, int64_t *doc_out, double *score_out, int64_t *count_out);
int  gz_bm25_search_device(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                           const double params[6], int32_t plus, int64_t k, int64_t *doc_out_dev, double *score_out_dev,
                           int64_t *count_out_dev);
int  gz_bm25_match_count(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, int64_t *count_out);
int  gz_bm25_search_bool(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                         const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t *ex_terms, const int64_t *ex_off,
                         int64_t *doc_out, double *score_out, int64_t *count_out);
int  gz_bm25_search_bool_device(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                                const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t *ex_terms,
                                const int64_t *ex_off, int64_t *doc_out_dev, double *score_out_dev, int64_t *count_out_dev);
int  gz_bm25_match_count_bool(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, int32_t mode,
                              const int32_t *ex_terms, const int64_t *ex_off, int64_t *count_out);
int  gz_bm25_search_phrase(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                           const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t *ex_terms, const int64_t *ex_off,
                           const int32_t *ph_terms, const int64_t *ph_off, int64_t *doc_out, double *score_out, int64_t *count_out);
int  gz_bm25_search_phrase_device(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                                  const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t *ex_terms,
                                  const int64_t *ex_off, const int32_t *ph_terms, const int64_t *ph_off, int64_t *doc_out_dev,
                                  double *score_out_dev, int64_t *count_out_dev);
int  gz_bm25_match_count_phrase(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, int32_t mode,
                                const int32_t *ex_terms, const int64_t *ex_off, const int32_t *ph_terms, const int64_t *ph_off,
                                int64_t *count_out);
int  gz_bm25_search_near(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                         const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t *ex_terms, const int64_t *ex_off,
                         const int32_t *ph_terms, const int64_t *ph_off, const int32_t *near_terms, const int64_t *near_off,
                         const int64_t *near_window, int64_t *doc_out, double *score_out, int64_t *count_out);
int  gz_bm25_search_near_device(gz_bm25 *index, const int32_t *terms, const double *idf, const int64_t *query_off, int64_t n_queries,
                                const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t *ex_terms,
                                const int64_t *ex_off, const int32_t *ph_terms, const int64_t *ph_off, const int32_t *near_terms,
                                const int64_t *near_off, const int64_t *near_window, int64_t *doc_out_dev, double *score_out_dev,
                                int64_t *count_out_dev);
int  gz_bm25_match_count_near(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, int32_t mode,
                              const int32_t *ex_terms, const int64_t *ex_off, const int32_t *ph_terms, const int64_t *ph_off,
                              const int32_t *near_terms, const int64_t *near_off, const int64_t *near_window, int64_t *count_out);
int  gz_bm25_cover(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, const int64_t *ids, int64_t k,
                   int32_t *start_out, int32_t *len_out, int32_t *words_out);
int  gz_bm25_cover_device(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, const int64_t *ids_dev,
                          int64_t k, int32_t *start_out_dev, int32_t *len_out_dev, int32_t *words_out_dev);
int  gz_bm25_search_groups(gz_bm25 *index, const int32_t *alt_terms, const int64_t *alt_off, const double *group_idf,
                           const int64_t *group_off, int64_t n_queries, const double params[6], int32_t plus, int64_t k, int32_t mode,
                           const int32_t *ex_terms, const int64_t *ex_off, int64_t *doc_out, double *score_out, int64_t *count_out);
int  gz_bm25_search_groups_device(gz_bm25 *index, const int32_t *alt_terms, const int64_t *alt_off, const double *group_idf,
                                  const int64_t *group_off, int64_t n_queries, const double params[6], int32_t plus, int64_t k,
                                  int32_t mode, const int32_t *ex_terms, const int64_t *ex_off, int64_t *doc_out_dev,
                                  double *score_out_dev, int64_t *count_out_dev);
int  gz_bm25_match_count_groups(gz_bm25 *index, const int32_t *alt_terms, const int64_t *alt_off, const int64_t *group_off,
                                int64_t n_queries, int32_t mode, const int32_t *ex_terms, const int64_t *ex_off, int64_t *count_out);
int  gz_bm25_snippets(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, const int64_t *ids, int64_t k,
                      int64_t width, int32_t *start_out, int32_t *hits_out);
int  gz_bm25_snippets_device(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, const int64_t *ids_dev,
                             int64_t k, int64_t width, int32_t *start_out_dev, int32_t *hits_out_dev);
int  gz_bm25_occurrences(gz_bm25 *index, const int32_t *terms, const int64_t *query_off, int64_t n_queries, const int64_t *ids, int64_t k,
                         int64_t *pair_off_out, int32_t *pos_out, int32_t *word_out, int64_t cap);
int  gz_bm25_append(gz_bm25 *index, const uint8_t *text, const int64_t *text_off, int64_t n_docs);
int  gz_bm25_append_device(gz_bm25 *index, const uint8_t *text_dev, const int64_t *text_off_dev, int64_t n_docs, int64_t text_bytes);
int  gz_bm25_remove(gz_bm25 *index, const int64_t *doc_ids, int64_t n_ids);
int  gz_bm25_remove_device(gz_bm25 *index, const int64_t *doc_ids_dev, int64_t n_ids);
int  gz_bm25_compact(gz_bm25 *index);
int  gz_bm25_terms(gz_bm25 *index, int64_t *term_off, int32_t *df, uint8_t *bytes, int64_t bytes_cap);
int  gz_bm25_similar(gz_bm25 *index, const uint8_t *words, const int64_t *word_off, int64_t n_words, int32_t max_edits, int64_t k,
                     int64_t *ids_out, int32_t *dist_out, int32_t *df_out, int64_t *count_out);
int  gz_bm25_prefix(gz_bm25 *index, const uint8_t *words, const int64_t *word_off, int64_t n_words, int64_t k, int64_t *ids_out,
                    int32_t *df_out, int64_t *count_out);
int  gz_bm25_term_bytes(gz_bm25 *index, const int64_t *ids, int64_t n_ids, int64_t *off_out /* n_ids + 1 */, uint8_t *bytes,
                        int64_t bytes_cap);
int  gz_bm25_footprint(gz_bm25 *index, int64_t out[3]);
void gz_bm25_destroy(gz_bm25 *index);

#ifdef __cplusplus
}
#endif
#endif /* GENZ_TOKENIZE_H */
