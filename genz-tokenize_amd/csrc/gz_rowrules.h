// gz_rowrules.h -- the rules every row-shaping call shares, as plain host C++ (no HIP, no context: tests/test_row_rules.py compiles
// this file alone): the check of a host CSR input, the dense-row rule, the MinHash argument rules (tests/test_minhash_surface.py
// compiles them alone too), the n-gram overlap argument rules (tests/test_ngram_surface.py), the n-gram repeats argument rules
// (tests/test_repeat_surface.py), the question-context window rules (tests/test_pairwin_surface.py) and the pairwise-disjoint check of a
// call's arrays.
#pragma once
#include <cstddef>
#include <cstdint>

// A host CSR input: rows r = payload[off[r] .. off[r + 1]) in elements, absolute offsets (off[0] need not be 0).
// *n = elements of the batch.  ROWS_OK, or which of the caller's two messages to report ("bad ... offsets", "... offsets must not
// decrease"), in that order of precedence.
enum RowsFault { ROWS_OK = 0, ROWS_BAD = 1, ROWS_DECREASE = 2 };
inline RowsFault rows_offsets_check(const void* payload, const int64_t* off, int64_t n_rows, int64_t* n)
{
    *n = (int64_t)((uint64_t)off[n_rows] - (uint64_t)off[0]);          // (unsigned: absurd offsets wrap to a refusal, they do not overflow)
    if (*n < 0 || (*n > 0 && !payload)) return ROWS_BAD;
    for (int64_t r = 0; r < n_rows; ++r) if (off[r + 1] < off[r]) return ROWS_DECREASE;
    return ROWS_OK;
}

// dense [n_rows, row_len] rows whose first row is row row_base of the caller's data set: every cell's global index fits 63 bits
inline bool dense_rule_ok(int64_t n_rows, int32_t row_len, int64_t row_base, int32_t whole_word)
{
    if (row_len < 1 || n_rows < 0 || row_base < 0 || (whole_word != 0 && whole_word != 1)) return false;
    const unsigned __int128 cells = ((unsigned __int128)row_base + (unsigned __int128)n_rows) * (unsigned __int128)row_len;
    return (cells >> 63) == 0;
}

// MinHash (gz_minhash_rows*, gz_minhash_groups*): the sentence of the first rule an argument list breaks, or nullptr.  Every refusal
// has its own sentence; the order below is the order they are reported in.
inline const char* minhash_rows_fault(int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t shingle, int32_t num_perm)
{
    if (n_rows < 0) return "minhash rows need n_rows >= 0";
    if (skip_front < 0 || skip_front > 1 || skip_back < 0 || skip_back > 1) return "minhash rows need skips of 0 or 1";
    if (shingle < 1 || shingle > 32) return "minhash rows need a shingle width in 1..32";
    if (num_perm < 1 || num_perm > 256) return "minhash rows need num_perm in 1..256";
    return nullptr;
}
inline const char* minhash_groups_fault(int64_t n_rows, int32_t num_perm, int32_t bands, int32_t min_agree)
{
    if (n_rows < 0) return "minhash groups need n_rows >= 0";
    if (n_rows >= (int64_t)INT32_MAX - 4096) return "minhash groups need fewer than 2^31 - 4096 rows";
    if (num_perm < 1 || num_perm > 256) return "minhash groups need num_perm in 1..256";
    if (bands < 1) return "minhash groups need bands >= 1";
    if (num_perm % bands != 0) return "minhash groups need a number of bands that divides num_perm";
    if (min_agree < 1 || min_agree > num_perm) return "minhash groups need min_agree in 1..num_perm";
    return nullptr;
}
// the longest body of a host CSR input whose offsets passed rows_offsets_check: a body of 2^31 ids or more is refused (GZ_E_LIMIT)
inline bool minhash_bodies_fit(const int64_t* off, int64_t n_rows, int32_t skip_front, int32_t skip_back)
{
    for (int64_t r = 0; r < n_rows; ++r)
        if (off[r + 1] - off[r] - skip_front - skip_back >= ((int64_t)1 << 31)) return false;
    return true;
}

// n-gram overlap (gz_ngram_index_build*, gz_ngram_overlap*; tests/test_ngram_surface.py compiles these alone): the sentence of the first
// rule an argument list breaks, or nullptr, in the order they are reported in.  first_ref is an int32 a query row: the reference rows
// stay below 2^31.
inline const char* ngram_build_fault(int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t n)
{
    if (n_rows < 0) return "n-gram index needs n_rows >= 0";
    if (n_rows > (int64_t)INT32_MAX) return "n-gram index needs fewer than 2^31 reference rows";
    if (skip_front < 0 || skip_front > 1 || skip_back < 0 || skip_back > 1) return "n-gram index needs skips of 0 or 1";
    if (n < 1 || n > 32) return "n-gram index needs a width n in 1..32";
    return nullptr;
}
inline const char* ngram_overlap_fault(int64_t n_rows, int32_t skip_front, int32_t skip_back)
{
    if (n_rows < 0) return "n-gram overlap needs n_rows >= 0";
    if (skip_front < 0 || skip_front > 1 || skip_back < 0 || skip_back > 1) return "n-gram overlap needs skips of 0 or 1";
    return nullptr;
}
// the reference ids an index takes: a slot holds position + 1 in 32 bits, so 2^32 - 1 ids or more are refused (GZ_E_LIMIT); so is a
// body of 2^31 ids or more (minhash_bodies_fit)
inline bool ngram_ids_fit(int64_t n_ids) { return n_ids >= 0 && (uint64_t)n_ids < 0xFFFFFFFFull; }
// What the n-gram positions of n_rows rows that hold n_ids ids between them can add up to at width n: a row of L ids has between
// L - skip_front - skip_back - (n - 1) and L of them.  A position total outside that range read back from the device is no total: a
// table sized by one that is too small is one a probe loop never leaves.  The range holds for offsets that do not decrease -- the
// host forms check that, the device forms take it from their caller (offsets that go back and forth can add up to more than n_ids
// and are refused here, where the sum once sized a table).  n_ids >= 0, n_rows >= 0, skips 0 or 1, 1 <= n <= 32.
inline bool ngram_positions_possible(int64_t n_pos, int64_t n_ids, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t n)
{
    const int64_t lost = (int64_t)skip_front + skip_back + n - 1;                  // (at most 33 a row)
    int64_t least = n_ids;
    if (lost) least = n_rows > n_ids / lost ? 0 : n_ids - n_rows * lost;          // (the product is at most n_ids: it does not wrap)
    return n_pos >= least && n_pos <= n_ids;
}

// n-gram repeats (gz_ngram_repeats*; tests/test_repeat_surface.py compiles this alone): the sentence of the first rule an argument
// list breaks, or nullptr, in the order they are reported in.  The ids of a call obey ngram_ids_fit (a slot holds position + 1 in 32
// bits) and its bodies minhash_bodies_fit.
inline const char* repeat_fault(int64_t n_rows, int32_t skip_front, int32_t skip_back, const int32_t* widths, int32_t n_widths)
{
    if (n_rows < 0) return "n-gram repeats need n_rows >= 0";
    if (skip_front < 0 || skip_front > 1 || skip_back < 0 || skip_back > 1) return "n-gram repeats need skips of 0 or 1";
    if (n_widths < 1 || n_widths > 16) return "n-gram repeats need 1..16 widths";
    if (!widths) return "n-gram repeats need the widths";
    uint64_t seen = 0;                                                 // bit n: width n stands earlier in the list
    for (int32_t k = 0; k < n_widths; ++k) {
        if (widths[k] < 1 || widths[k] > 32) return "n-gram repeats need every width in 1..32";
        if (seen >> widths[k] & 1u) return "n-gram repeats need distinct widths";
        seen |= (uint64_t)1 << widths[k];
    }
    return nullptr;
}

// Word spans, aligned rows, span labels (gz_word_spans*, gz_align_rows*, gz_span_labels*; tests/test_align_surface.py compiles these
// alone): the sentence of the first rule broken, or nullptr, in the order they are reported in.  The *_data_fault rules read the
// caller's arrays, so only the host forms can apply them; the device forms trust what they cannot read.
inline const char* word_spans_fault(int64_t n_docs, int32_t unit, int64_t capacity_words)
{
    if (n_docs < 0) return "word spans need n_docs >= 0";
    if (unit != 0 && unit != 1) return "word spans need unit 0 (code points) or 1 (bytes)";
    if (capacity_words < 0) return "word spans need capacity_words >= 0";
    return nullptr;
}
inline const char* align_rows_fault(int64_t n_docs, int64_t n_rows, bool have_row_doc, int32_t max_len, int32_t continuation, bool have_map,
                                    int32_t n_map, bool want_labels, bool have_word_labels)
{
    if (n_docs < 0 || n_rows < 0) return "aligned rows need n_docs >= 0 and n_rows >= 0";
    if (max_len < 3) return "aligned rows need max_len >= 3";
    if (!have_row_doc && n_rows != n_docs) return "aligned rows without row_doc need n_rows == n_docs";
    if (continuation < 0 || continuation > 2) return "aligned rows need continuation 0 (ignore), 1 (same) or 2 (map)";
    if (n_map < 0) return "aligned rows need n_map >= 0";
    if (continuation == 2 && (!have_map || n_map < 1)) return "aligned rows in map mode need a cont_map of at least one entry";
    if (want_labels && !have_word_labels) return "aligned rows need word_labels where labels are asked for";
    if ((uint64_t)n_rows > (uint64_t)(INT64_MAX / 4) / (uint64_t)max_len) return "aligned rows need n_rows * max_len * 4 below 2^63";
    return nullptr;
}
// counts: the n counts of the batch (already at its first word); row_doc / row_start may be null
inline const char* align_data_fault(const int32_t* counts, int64_t n, const int32_t* row_doc, const int32_t* row_start, int64_t n_rows, int64_t n_docs)
{
    for (int64_t i = 0; i < n; ++i) if (counts[i] < 1) return "aligned rows: a word's piece count is below 1";
    if (row_doc) for (int64_t r = 0; r < n_rows; ++r) if (row_doc[r] < 0 || (int64_t)row_doc[r] >= n_docs) return "aligned rows: a row_doc lies outside [0, n_docs)";
    if (row_start) for (int64_t r = 0; r < n_rows; ++r) if (row_start[r] < 0) return "aligned rows: a row_start is negative";
    return nullptr;
}
inline const char* span_labels_fault(int64_t n_docs, int32_t scheme)
{
    if (n_docs < 0) return "span labels need n_docs >= 0";
    if (scheme != 0 && scheme != 1) return "span labels need scheme 0 (plain) or 1 (BIO)";
    return nullptr;
}
// marks: the n_marks (begin, end, label) triples of the batch (already at its first mark).  BIO writes 2 * label + 2.
inline const char* span_labels_data_fault(const int32_t* marks, int64_t n_marks, int32_t scheme)
{
    if (scheme != 1) return nullptr;
    for (int64_t m = 0; m < n_marks; ++m) {
        if (marks[3 * m + 2] < 0) return "span labels under BIO need labels >= 0";
        if (marks[3 * m + 2] >= (1 << 30) - 1) return "span labels under BIO need labels below 2^30 - 1";
    }
    return nullptr;
}

// Question-context windows and span tokens (gz_pair_window_rows*, gz_span_tokens*; tests/test_pairwin_surface.py compiles these alone):
// the sentence of the first rule broken, or nullptr, in the order they are reported in.  With L = max_len the call is valid iff
// L >= 5, 0 <= max_query_len <= L - 5 and 0 <= stride <= L - 5 - max_query_len (room = L - 4 - q >= stride + 1 for every q <=
// max_query_len: every window adds a token).  pairwin_data_fault reads the caller's q_row, so only the host form can apply it; the
// device form reads an entry outside [0, n_questions) as an empty question.
inline const char* pairwin_fault(int64_t n_rows, int64_t n_questions, bool have_q_row, int32_t max_len, int32_t stride, int32_t max_query_len,
                                 int32_t skip_front, int32_t skip_back, int64_t capacity_windows)
{
    if (n_rows < 0 || n_questions < 0) return "pair windows need n_rows >= 0 and n_questions >= 0";
    if (capacity_windows < 0) return "pair windows need capacity_windows >= 0";
    if (skip_front < 0 || skip_front > 1 || skip_back < 0 || skip_back > 1) return "pair windows need skips of 0 or 1";
    if (max_len < 5) return "pair windows need max_len >= 5";
    if (max_query_len < 0 || max_query_len > max_len - 5) return "pair windows need max_query_len in [0, max_len - 5]";
    if (stride < 0 || stride > max_len - 5 - max_query_len) return "pair windows need a stride in [0, max_len - 5 - max_query_len]";
    if (!have_q_row && n_questions != n_rows) return "pair windows without q_row need n_questions == n_rows";
    return nullptr;
}
inline const char* pairwin_data_fault(const int32_t* q_row, int64_t n_rows, int64_t n_questions)
{
    if (q_row) for (int64_t r = 0; r < n_rows; ++r) if (q_row[r] < 0 || (int64_t)q_row[r] >= n_questions) return "pair windows: a q_row lies outside [0, n_questions)";
    return nullptr;
}
inline const char* span_tokens_fault(int64_t n_docs) { return n_docs < 0 ? "span tokens need n_docs >= 0" : nullptr; }
// counts: the n counts of the batch; mark_words: the n_marks (first, last + 1) pairs of the batch; W_d of a mark is only known with
// its document, so the ranges are checked against the whole batch here and clamped into their document on the device
inline const char* span_tokens_data_fault(const int32_t* counts, int64_t n, const int32_t* mark_words, int64_t n_marks)
{
    for (int64_t i = 0; i < n; ++i) if (counts[i] < 1) return "span tokens: a word's piece count is below 1";
    for (int64_t m = 0; m < n_marks; ++m) {
        const int32_t f = mark_words[2 * m], l = mark_words[2 * m + 1];
        if (f == -1 && l == -1) continue;
        if (f < 0 || l < f || (int64_t)l > n) return "span tokens: a word range is neither (-1, -1) nor 0 <= first <= last + 1 <= words";
    }
    return nullptr;
}

// An array of a call: where it starts and how many bytes the call touches.  ABSENT: a null address or zero bytes.  (The callers
// spelled this two ways, "zero bytes" for masked rows and "null address" for infill rows; with n_rows > 0 and row_len >= 1, which
// both have checked by then, every array that is given has bytes and every array with bytes that is left out is null: one rule.)
struct Span { uintptr_t p; uintptr_t n; };
inline Span span_of(const void* p, uintptr_t bytes) { return Span{(uintptr_t)p, bytes}; }

// no two present arrays share a byte (arrays that touch end to start are fine)
inline bool disjoint(const Span* s, int k)
{
    for (int a = 0; a < k; ++a)
        for (int b = a + 1; b < k; ++b) {
            if (!s[a].p || !s[a].n || !s[b].p || !s[b].n) continue;
            if (s[a].p >= s[b].p ? s[a].p - s[b].p < s[b].n : s[b].p - s[a].p < s[a].n) return false;       // (differences: no end address to wrap)
        }
    return true;
}
