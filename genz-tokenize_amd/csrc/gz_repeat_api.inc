// n-gram repetition inside a document behind the C ABI (gz_ngram_repeats, gz_ngram_repeats_device).  Included by gz_api.cpp behind
// gz_ngram_api.inc, whose "internal" sentence it shares, and gz_rows_api.inc, whose row front both forms use (RowsIn, rows_check,
// rows_stage, StagedOut for the host form; rows_extent_device for the device form's extent; pieces_count_locked and its limit sentence
// for the count pass); the kernels are in gz_repeat.inc and gz_pieces.inc, the argument rules without HIP in them in gz_rowrules.h
// (repeat_fault).
//
// A call owns nothing beyond the context's workspace: the row front's w_pieces (16 bytes a row: piece counts and their scan, then the
// position total and the too-long flag), w_rp_tab (12 bytes a slot: the slots, then their counts) and, only where a row has several
// pieces and a top output is asked for, w_rp_top (8 bytes a row).  It waits once for the piece count, the positions and the flag, then runs the
// widths in the caller's order on the context's stream, and waits for its outputs.

namespace {
const char* const kRepeatBuffers = "n-gram repeats need ids and row_off";
const char* const kRepeatDisjoint = "n-gram repeats need output arrays that overlap neither the input nor each other";
const char* const kRepeatIdsLimit = "n-gram repeats take fewer than 2^32 - 1 ids a call: shard the rows";

struct RepeatOut { int32_t* v[6]; uint16_t* covered; };              // Context.REPEAT_OUT's order, each [n_widths, n_rows]; covered indexed like ids

// ids / covered at: the first id of the call and the cell that belongs to it; n_ids of them.  n_rows > 0.
bool repeat_disjoint(const void* ids_at, uintptr_t n_ids, const int64_t* row_off, int64_t n_rows, int32_t n_widths, const RepeatOut& O, const void* covered_at)
{
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 1024)) return false;                                 // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows, per = n * (uintptr_t)n_widths * 4u;
    const Span s[9] = {span_of(ids_at, n_ids * 4u), span_of(row_off, (n + 1) * 8u), span_of(O.v[0], per), span_of(O.v[1], per), span_of(O.v[2], per),
                       span_of(O.v[3], per), span_of(O.v[4], per), span_of(O.v[5], per), span_of(covered_at, n_ids * 2u)};
    return disjoint(s, 9);
}

// The call on the context's stream, behind whatever it holds; the caller waits for the outputs.  Every pointer of O a device pointer.
// Nothing is written to the outputs when a body is too long.  n_rows > 0; off0 = row_off[0], n_ids = row_off[n_rows] - off0.
int repeats_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int64_t off0, int64_t n_ids, int32_t skip_front, int32_t skip_back,
                   const int32_t* widths, int32_t n_widths, const RepeatOut& O)
{
    int rc;
    int32_t n_min = widths[0];
    for (int32_t k = 1; k < n_widths; ++k) n_min = widths[k] < n_min ? widths[k] : n_min;
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, n_min, GZ_PIECES_NGRAMS, true, nullptr, &P))) return rc;
    if (!ngram_positions_possible(P.n_pos, n_ids, n_rows, skip_front, skip_back, n_min)) return fail(c, GZ_E_HIP, "%s", kNgramPositions);
    const int64_t n_pieces = P.n_pieces;
    const uint64_t slots = gz_ngram_slots(P.n_pos);
    if ((rc = ensure(c, c->w_rp_tab, (size_t)slots * 12))) return rc;
    const bool want_top = O.v[4] || O.v[5];
    if (n_pieces != n_rows && want_top && (rc = ensure(c, c->w_rp_top, (size_t)n_rows * 8))) return rc;
    const int bits = c->opt.repeat_hash_bits;
    GzRepeatArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.off0 = off0;
    A.skip_front = skip_front; A.skip_back = skip_back;
    A.piece_off = P.piece_off; A.n_pieces = n_pieces;
    A.table = (unsigned long long*)c->w_rp_tab.p; A.count = (uint32_t*)(A.table + slots); A.mask = slots - 1;
    A.hmask = bits > 0 ? (1ull << bits) - 1ull : ~0ull;
    A.top = n_pieces != n_rows && want_top ? (unsigned long long*)c->w_rp_top.p : nullptr;
    A.covered = O.covered;
    for (int32_t k = 0; k < n_widths; ++k) {
        A.n = widths[k]; A.k = k;
        int32_t** const dst[6] = {&A.n_grams, &A.n_distinct, &A.n_repeated, &A.n_covered, &A.top_count, &A.top_pos};
        for (int i = 0; i < 6; ++i) *dst[i] = O.v[i] ? O.v[i] + (size_t)k * (size_t)n_rows : nullptr;
        gz_launch_repeat_width(A, c->stream);
    }
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_ngram_repeats_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                            const int32_t* widths, int32_t n_widths, int32_t* n_grams_dev, int32_t* n_distinct_dev, int32_t* n_repeated_dev,
                            int32_t* n_covered_dev, int32_t* top_count_dev, int32_t* top_pos_dev, uint16_t* covered_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = repeat_fault(n_rows, skip_front, skip_back, widths, n_widths)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!row_off_dev) return fail(c, GZ_E_INVALID, "%s", kRepeatBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    int64_t off0 = 0, n_ids = 0;
    if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
    if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kRepeatBuffers);
    if (!ngram_ids_fit(n_ids)) return fail(c, GZ_E_LIMIT, "%s", kRepeatIdsLimit);
    const RepeatOut O{{n_grams_dev, n_distinct_dev, n_repeated_dev, n_covered_dev, top_count_dev, top_pos_dev}, covered_dev};
    if (!repeat_disjoint(n_ids ? ids_dev + off0 : nullptr, (uintptr_t)n_ids, row_off_dev, n_rows, n_widths, O, covered_dev && n_ids ? covered_dev + off0 : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kRepeatDisjoint);
    if ((rc = repeats_locked(c, ids_dev, row_off_dev, n_rows, off0, n_ids, skip_front, skip_back, widths, n_widths, O))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_repeats(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back, const int32_t* widths,
                     int32_t n_widths, int32_t* n_grams, int32_t* n_distinct, int32_t* n_repeated, int32_t* n_covered, int32_t* top_count,
                     int32_t* top_pos, uint16_t* covered)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = repeat_fault(n_rows, skip_front, skip_back, widths, n_widths)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!row_off || (!ids && row_off[n_rows] != row_off[0])) return fail(c, GZ_E_INVALID, "%s", kRepeatBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    if (!ngram_ids_fit(in.n)) return fail(c, GZ_E_LIMIT, "%s", kRepeatIdsLimit);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    const RepeatOut O{{n_grams, n_distinct, n_repeated, n_covered, top_count, top_pos}, covered};
    if (!repeat_disjoint(in.n ? ids + row_off[0] : nullptr, (uintptr_t)in.n, row_off, n_rows, n_widths, O, covered && in.n ? covered + row_off[0] : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kRepeatDisjoint);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, 0))) return rc;
    const size_t per = (size_t)n_rows * (size_t)n_widths * 4;
    StagedOut S;
    S.add(covered && in.n ? covered + row_off[0] : nullptr, (size_t)in.n * 2, true);
    for (int i = 0; i < 6; ++i) S.add(O.v[i], per, false);
    if ((rc = staged_ensure(c, S))) return rc;
    const RepeatOut D{{S.dev(1), S.dev(2), S.dev(3), S.dev(4), S.dev(5), S.dev(6)}, S.e[0].dev ? (uint16_t*)S.e[0].dev - row_off[0] : nullptr};
    if ((rc = repeats_locked(c, (const int32_t*)in.d_payload, in.d_off, n_rows, row_off[0], in.n, skip_front, skip_back, widths, n_widths, D))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

}  // extern "C"
