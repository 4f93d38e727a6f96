// Duplicate substrings across the rows of a call, and the cut of marked ids, behind the C ABI (gz_substr_dups, gz_substr_dups_device,
// gz_cut_rows, gz_cut_rows_device).  Included by gz_api.cpp behind gz_repeat_api.inc and gz_rows_api.inc, whose row front every form
// uses (RowsIn, rows_check, rows_stage, StagedOut for the host forms; rows_extent_device for the device forms' extent;
// pieces_count_locked and its limit sentence for the count pass); the kernels are in gz_substr.inc and gz_pieces.inc, the argument
// rules without HIP in them in gz_rowrules.h (substr_fault, cut_fault).
//
// gz_substr_dups takes its table and the slot words as the n-gram index build takes its table -- a buffer of the call's own, sized by
// the positions the count pass reports: 8 bytes a slot and 4 bytes an id, 20 to 36 bytes a token with one position a token -- and
// gives it back before it returns (SubstrTable).  What stays with the context is small: w_pieces (16 bytes a row), w_ss_aux (4 bytes
// a row, only where first_src is asked for without first_dup), and for the cut w_ss_cut (16 bytes a piece) and, host form, w_ss_drop
// (the staged drop bytes).  A dups call waits once for the piece count, the positions and the flag, and once for its outputs; a cut
// call once for the piece count and once for its outputs (the host form a third time, for the total it copies back).

namespace {
const char* const kSubstrBuffers = "duplicate substrings need ids and row_off";
const char* const kSubstrDisjoint = "duplicate substrings need output arrays that overlap neither the input nor each other";
const char* const kSubstrIdsLimit = "duplicate substrings take fewer than 2^32 - 1 ids a call: shard the rows";
const char* const kCutBuffers = "cut rows need ids, row_off, drop, out_row_off and, for rows that hold ids, out_ids";
const char* const kCutDisjoint = "cut rows need output arrays that overlap neither the input nor each other";
const char* const kCutIdsLimit = "cut rows take fewer than 2^32 - 1 ids a call: shard the rows";

struct SubstrOut { int32_t* n_grams; int32_t* n_later; int32_t* n_dup; int32_t* first_dup; int32_t* first_src; uint8_t* dup; };
struct SubstrTable { DBuf buf; ~SubstrTable() { release(buf); } };   // (a free waits for the device: nothing of the call is in flight behind it)

// ids / dup at: the first id of the call and the cell that belongs to it; n_ids of them.  n_rows > 0.
bool substr_disjoint(const void* ids_at, uintptr_t n_ids, const int64_t* row_off, int64_t n_rows, const SubstrOut& O, const void* dup_at)
{
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 16)) return false;                                   // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows;
    const Span s[8] = {span_of(ids_at, n_ids * 4u), span_of(row_off, (n + 1) * 8u), span_of(O.n_grams, n * 4u), span_of(O.n_later, n * 4u),
                       span_of(O.n_dup, n * 4u), span_of(O.first_dup, n * 4u), span_of(O.first_src, n * 4u), span_of(dup_at, n_ids)};
    return disjoint(s, 8);
}

// The call on the context's stream, behind whatever it holds; the caller waits for the outputs and then lets T go.  Every pointer of
// O a device pointer, O.dup indexed like ids_dev.  Nothing is written to the outputs when a body is too long.  n_rows > 0;
// off0 = row_off[0], n_ids = row_off[n_rows] - off0.
int substr_dups_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int64_t off0, int64_t n_ids, int32_t skip_front,
                       int32_t skip_back, int32_t n, SubstrOut O, SubstrTable& T)
{
    int rc;
    alloc_site(c);
    if (O.first_src && !O.first_dup) {                                              // (first_src is resolved from first_dup)
        if ((rc = ensure(c, c->w_ss_aux, (size_t)n_rows * 4 + 16))) return rc;
        O.first_dup = (int32_t*)c->w_ss_aux.p;
    }
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, n, GZ_PIECES_NGRAMS, true, nullptr, &P))) return rc;
    if (!ngram_positions_possible(P.n_pos, n_ids, n_rows, skip_front, skip_back, n)) return fail(c, GZ_E_HIP, "%s", kNgramPositions);
    const uint64_t slots = gz_substr_slots(P.n_pos);
    if ((rc = ensure(c, T.buf, (size_t)slots * 8 + (size_t)n_ids * 4 + 16))) return rc;
    const int bits = c->opt.substr_hash_bits;
    GzSubstrArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.off0 = off0; A.n_ids = n_ids;
    A.skip_front = skip_front; A.skip_back = skip_back; A.n = n;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.table = (unsigned long long*)T.buf.p; A.mask = slots - 1; A.slot_of = (uint32_t*)(A.table + slots);
    A.hmask = bits > 0 ? (1ull << bits) - 1ull : ~0ull;
    A.n_grams = O.n_grams; A.n_later = O.n_later; A.n_dup = O.n_dup; A.first_dup = O.first_dup; A.first_src = O.first_src; A.dup = O.dup;
    gz_launch_substr_dups(A, c->stream);
    return GZ_OK;
}

struct CutOut { int32_t* out_ids; int64_t* out_row_off; int32_t* n_kept; };

// ids / drop at: the first id of the call and the byte that belongs to it; n_ids of them.  n_rows > 0.
bool cut_disjoint(const void* ids_at, uintptr_t n_ids, const int64_t* row_off, int64_t n_rows, const void* drop_at, const CutOut& O)
{
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 16)) return false;                                   // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows;
    const Span s[6] = {span_of(ids_at, n_ids * 4u), span_of(row_off, (n + 1) * 8u), span_of(drop_at, n_ids), span_of(O.out_ids, n_ids * 4u),
                       span_of(O.out_row_off, (n + 1) * 8u), span_of(O.n_kept, n * 4u)};
    return disjoint(s, 6);
}

// The cut on the context's stream, behind whatever it holds; the caller waits for the outputs.  Every pointer a device pointer,
// drop_dev indexed like ids_dev.  Nothing is written when a row is too long.  n_rows > 0.
int cut_rows_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int64_t n_ids, const uint8_t* drop_dev, const CutOut& O)
{
    int rc;
    alloc_site(c);
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, 0, 0, 1, GZ_PIECES_NGRAMS, false, nullptr, &P))) return rc;
    if (P.n_pieces < n_rows || P.n_pieces > n_rows + n_ids / 4096)          // (a row of m ids has max(1, ceil(m / 4096)) pieces)
        return fail(c, GZ_E_HIP, "%s", kNgramPositions);
    if ((rc = ensure(c, c->w_ss_cut, ((size_t)P.n_pieces * 2 + 1) * 8))) return rc;
    GzCutArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.n_ids = n_ids; A.drop = drop_dev;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.piece_kept = (int64_t*)c->w_ss_cut.p; A.piece_base = A.piece_kept + P.n_pieces;
    A.out_ids = O.out_ids; A.out_row_off = O.out_row_off; A.n_kept = O.n_kept;
    gz_launch_cut_rows(A, c->stream);
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_substr_dups_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t n,
                          int32_t* n_grams_dev, int32_t* n_later_dev, int32_t* n_dup_dev, int32_t* first_dup_dev, int32_t* first_src_dev, uint8_t* dup_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = substr_fault(n_rows, skip_front, skip_back, n)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!row_off_dev) return fail(c, GZ_E_INVALID, "%s", kSubstrBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    SubstrTable T;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    int64_t off0 = 0, n_ids = 0;
    if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
    if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kSubstrBuffers);
    if (!ngram_ids_fit(n_ids)) return fail(c, GZ_E_LIMIT, "%s", kSubstrIdsLimit);
    const SubstrOut O{n_grams_dev, n_later_dev, n_dup_dev, first_dup_dev, first_src_dev, dup_dev};
    if (!substr_disjoint(n_ids ? ids_dev + off0 : nullptr, (uintptr_t)n_ids, row_off_dev, n_rows, O, dup_dev && n_ids ? dup_dev + off0 : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kSubstrDisjoint);
    if ((rc = substr_dups_locked(c, ids_dev, row_off_dev, n_rows, off0, n_ids, skip_front, skip_back, n, O, T))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_substr_dups(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t n, int32_t* n_grams,
                   int32_t* n_later, int32_t* n_dup, int32_t* first_dup, int32_t* first_src, uint8_t* dup)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = substr_fault(n_rows, skip_front, skip_back, n)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!row_off || (!ids && row_off[n_rows] != row_off[0])) return fail(c, GZ_E_INVALID, "%s", kSubstrBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    if (!ngram_ids_fit(in.n)) return fail(c, GZ_E_LIMIT, "%s", kSubstrIdsLimit);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    const SubstrOut O{n_grams, n_later, n_dup, first_dup, first_src, dup};
    if (!substr_disjoint(in.n ? ids + row_off[0] : nullptr, (uintptr_t)in.n, row_off, n_rows, O, dup && in.n ? dup + row_off[0] : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kSubstrDisjoint);
    std::lock_guard<std::mutex> lk(c->mu);
    SubstrTable T;
    if ((rc = rows_stage(c, in, 0))) return rc;
    const size_t per_row = (size_t)n_rows * 4;
    StagedOut S;
    S.add(dup && in.n ? dup + row_off[0] : nullptr, (size_t)in.n, true);
    S.add(n_grams, per_row, false); S.add(n_later, per_row, false); S.add(n_dup, per_row, false); S.add(first_dup, per_row, false);
    S.add(first_src, per_row, false);
    if ((rc = staged_ensure(c, S))) return rc;
    const SubstrOut D{S.dev(1), S.dev(2), S.dev(3), S.dev(4), S.dev(5), S.e[0].dev ? (uint8_t*)S.e[0].dev - row_off[0] : nullptr};
    if ((rc = substr_dups_locked(c, (const int32_t*)in.d_payload, in.d_off, n_rows, row_off[0], in.n, skip_front, skip_back, n, D, T))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

int gz_cut_rows_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, const uint8_t* drop_dev, int32_t* out_ids_dev,
                       int64_t* out_row_off_dev, int32_t* n_kept_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = cut_fault(n_rows)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!row_off_dev || !out_row_off_dev) return fail(c, GZ_E_INVALID, "%s", kCutBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    int64_t off0 = 0, n_ids = 0;
    if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
    if (n_ids > 0 && (!ids_dev || !drop_dev || !out_ids_dev)) return fail(c, GZ_E_INVALID, "%s", kCutBuffers);
    if (!ngram_ids_fit(n_ids)) return fail(c, GZ_E_LIMIT, "%s", kCutIdsLimit);
    const CutOut O{out_ids_dev, out_row_off_dev, n_kept_dev};
    if (!cut_disjoint(n_ids ? ids_dev + off0 : nullptr, (uintptr_t)n_ids, row_off_dev, n_rows, n_ids ? drop_dev + off0 : nullptr, O))
        return fail(c, GZ_E_INVALID, "%s", kCutDisjoint);
    if ((rc = cut_rows_locked(c, ids_dev, row_off_dev, n_rows, n_ids, drop_dev, O))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_cut_rows(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, const uint8_t* drop, int32_t* out_ids, int64_t* out_row_off,
                int32_t* n_kept)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = cut_fault(n_rows)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!row_off || !out_row_off || (row_off[n_rows] != row_off[0] && (!ids || !drop || !out_ids))) return fail(c, GZ_E_INVALID, "%s", kCutBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    if (!ngram_ids_fit(in.n)) return fail(c, GZ_E_LIMIT, "%s", kCutIdsLimit);
    if (!minhash_bodies_fit(row_off, n_rows, 0, 0)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    const CutOut O{out_ids, out_row_off, n_kept};
    if (!cut_disjoint(in.n ? ids + row_off[0] : nullptr, (uintptr_t)in.n, row_off, n_rows, in.n ? drop + row_off[0] : nullptr, O))
        return fail(c, GZ_E_INVALID, "%s", kCutDisjoint);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, 0))) return rc;
    if ((rc = ensure(c, c->w_ss_drop, (size_t)in.n + 16))) return rc;
    if (in.n && (rc = copy_in(c, c->w_ss_drop.p, drop + row_off[0], (size_t)in.n, c->stream))) return rc;
    StagedOut S;
    S.add(in.n ? out_ids : nullptr, (size_t)in.n * 4, true);
    S.add(out_row_off, (size_t)(n_rows + 1) * 8, false); S.add(n_kept, (size_t)n_rows * 4, false);
    if ((rc = staged_ensure(c, S))) return rc;
    const CutOut D{S.dev(0), (int64_t*)S.e[1].dev, S.dev(2)};
    if ((rc = cut_rows_locked(c, (const int32_t*)in.d_payload, in.d_off, n_rows, in.n, (const uint8_t*)c->w_ss_drop.p - row_off[0], D))) return rc;
    int64_t total = 0;                                                                // only the kept ids come back: the caller's array stays as it was behind them
    if ((rc = read_total(c, D.out_row_off + n_rows, nullptr, &total))) return rc;
    if (total < 0 || total > in.n) return fail(c, GZ_E_HIP, "%s", kNgramPositions);
    S.e[0].bytes = (size_t)total * 4;
    if (!total) S.e[0].dev = nullptr;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

}  // extern "C"
