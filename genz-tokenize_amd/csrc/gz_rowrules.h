// gz_rowrules.h -- the rules every row-shaping call shares, as plain host C++ (no HIP, no context: tests/test_row_rules.py compiles
// this file alone): the check of a host CSR input, the dense-row rule and the pairwise-disjoint check of a call's arrays.
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
