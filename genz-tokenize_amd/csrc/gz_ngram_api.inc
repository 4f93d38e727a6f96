// Exact token n-gram overlap against a held-out set behind the C ABI (gz_ngram_index_*, gz_ngram_overlap*).  Included by gz_api.cpp
// behind gz_rows_api.inc, whose row front both forms use (RowsIn, rows_check, rows_stage, StagedOut for the host forms;
// rows_extent_device for the device form's extent; pieces_count_locked and its limit sentence for the count pass); the kernels are in
// gz_ngram.inc and gz_pieces.inc, the argument rules without HIP in them in gz_rowrules.h.
//
// An index owns three device buffers: a copy of the reference ids (so the caller's may go), the rows' offsets from 0 and the table.
// It belongs to its context: every call on it runs on the context's stream under the context's lock, and gz_destroy frees what is
// left.  The build waits three times (the ids' extent in the device form, the positions, the distinct count), a query once (the
// piece count) before its launch and once for its outputs.

struct gz_ngram_index {
    gz_ctx* c = nullptr;
    int32_t n = 0, skip_front = 0, skip_back = 0;
    int64_t n_rows = 0, n_ids = 0, n_pos = 0, n_distinct = 0;
    uint64_t slots = 0, hmask = ~0ull;
    DBuf ids, off, table;
    ~gz_ngram_index() { release(ids); release(off); release(table); }
    int64_t device_bytes() const { return (int64_t)(ids.cap + off.cap + table.cap); }
};

namespace {
void ngram_index_free(gz_ngram_index* ix) { delete ix; }

const char* const kNgramBuildBuffers = "n-gram index needs ids and row_off";
const char* const kNgramOverlapBuffers = "n-gram overlap needs ids and row_off";
const char* const kNgramOverlapDisjoint = "n-gram overlap needs output arrays that overlap neither the input nor each other";
const char* const kNgramIdsLimit = "an n-gram index takes fewer than 2^32 - 1 reference ids: shard the held-out set";

const char* const kNgramPositions = "internal: the n-gram positions read back from the device do not fit the rows";

// The index of the rows ids_dev[row_off_dev[r] .. row_off_dev[r + 1]) (absolute offsets; the ids lie in [off0, off0 + n_ids)), on the
// context's stream behind whatever it holds.  Nothing is handed out before the index is complete.
int ngram_build_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int64_t off0, int64_t n_ids,
                       int32_t skip_front, int32_t skip_back, int32_t n, gz_ngram_index** out)
{
    alloc_site(c);
    std::unique_ptr<gz_ngram_index> ix(new gz_ngram_index());
    ix->c = c; ix->n = n; ix->skip_front = skip_front; ix->skip_back = skip_back; ix->n_rows = n_rows; ix->n_ids = n_ids;
    const int bits = c->opt.ngram_hash_bits;
    ix->hmask = bits > 0 ? (1ull << bits) - 1ull : ~0ull;
    int rc;
    if ((rc = ensure(c, ix->ids, (size_t)n_ids * 4 + 16)) || (rc = ensure(c, ix->off, (size_t)(n_rows + 1) * 8))) return rc;
    if (n_ids) HIPCHK(c, hipMemcpyAsync(ix->ids.p, ids_dev + off0, (size_t)n_ids * 4, hipMemcpyDeviceToDevice, c->stream));
    Pieces P{nullptr, 0, 0};
    if (n_rows > 0) {
        if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, n, GZ_PIECES_NGRAMS, true, (int64_t*)ix->off.p, &P))) return rc;
        if (!ngram_positions_possible(P.n_pos, n_ids, n_rows, skip_front, skip_back, n)) return fail(c, GZ_E_HIP, "%s", kNgramPositions);
    } else HIPCHK(c, hipMemsetAsync(ix->off.p, 0, 8, c->stream));
    ix->n_pos = P.n_pos;
    ix->slots = gz_ngram_slots(ix->n_pos);
    if ((rc = ensure(c, ix->table, (size_t)ix->slots * 8)) || (rc = ensure(c, c->w_ng_aux, 16))) return rc;
    HIPCHK(c, hipMemsetAsync(ix->table.p, 0, (size_t)ix->slots * 8, c->stream));
    if (ix->n_pos > 0) {
        HIPCHK(c, hipMemsetAsync(c->w_ng_aux.p, 0, 8, c->stream));
        GzNgramArgs A{};
        A.ids = A.ref_ids = (const int32_t*)ix->ids.p; A.row_off = A.ref_off = (const int64_t*)ix->off.p; A.n_rows = A.ref_rows = n_rows;
        A.skip_front = skip_front; A.skip_back = skip_back; A.n = n;
        A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
        A.table = (unsigned long long*)ix->table.p; A.mask = ix->slots - 1; A.hmask = ix->hmask;
        A.n_distinct = (unsigned long long*)c->w_ng_aux.p;
        gz_launch_ngram_insert(A, c->stream);
        if ((rc = read_total(c, (const int64_t*)c->w_ng_aux.p, nullptr, &ix->n_distinct))) return rc;
    } else HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    alloc_site(c);
    c->ngram_live.push_back(ix.get());
    *out = ix.release();
    return GZ_OK;
}

struct NgramOut { int32_t* n_grams; int32_t* n_hits; int32_t* n_covered; int32_t* first_hit; int32_t* first_ref; uint8_t* covered; };

// the handle and the argument rules of a query; c and ix not null
int ngram_overlap_rule(gz_ctx* c, gz_ngram_index* ix, int64_t n_rows, int32_t skip_front, int32_t skip_back)
{
    if (ix->c != c) return fail(c, GZ_E_INVALID, "the n-gram index belongs to another context");
    if (const char* why = ngram_overlap_fault(n_rows, skip_front, skip_back)) return fail(c, GZ_E_INVALID, "%s", why);
    return GZ_OK;
}

// ids_bytes / covered at: what the call knows of the ids' extent (the host form: all of it; the device form: their first word).  n_rows > 0.
bool ngram_overlap_disjoint(const void* ids, uintptr_t ids_bytes, const int64_t* row_off, int64_t n_rows, const NgramOut& O, const void* covered_at,
                            uintptr_t covered_bytes)
{
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 16)) return false;                                   // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows;
    const Span s[8] = {span_of(ids, ids_bytes), span_of(row_off, (n + 1) * 8u), span_of(O.n_grams, n * 4u), span_of(O.n_hits, n * 4u),
                       span_of(O.n_covered, n * 4u), span_of(O.first_hit, n * 4u), span_of(O.first_ref, n * 4u), span_of(covered_at, covered_bytes)};
    return disjoint(s, 8);
}

// The query on the context's stream, behind whatever it holds; the caller waits for the outputs.  Every pointer of O a device pointer,
// O.covered indexed like ids_dev.  Nothing is written to the outputs when a body is too long.  n_rows > 0.
int ngram_overlap_locked(gz_ctx* c, gz_ngram_index* ix, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front,
                         int32_t skip_back, NgramOut O)
{
    int rc;
    if (O.first_ref && !O.first_hit) {                                              // (first_ref is resolved from first_hit)
        if ((rc = ensure(c, c->w_ng_aux, (size_t)n_rows * 4 + 16))) return rc;
        O.first_hit = (int32_t*)((uint8_t*)c->w_ng_aux.p + 16);
    }
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, ix->n, GZ_PIECES_NGRAMS, false, nullptr, &P))) return rc;
    GzNgramArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows;
    A.skip_front = skip_front; A.skip_back = skip_back; A.n = ix->n;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.table = (unsigned long long*)ix->table.p; A.mask = ix->slots - 1; A.hmask = ix->hmask;
    A.ref_ids = (const int32_t*)ix->ids.p; A.ref_off = (const int64_t*)ix->off.p; A.ref_rows = ix->n_rows;
    A.n_grams = O.n_grams; A.n_hits = O.n_hits; A.n_covered = O.n_covered; A.first_hit = O.first_hit; A.first_ref = O.first_ref; A.covered = O.covered;
    gz_launch_ngram_query(A, c->stream);
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_ngram_index_build_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                                int32_t n, gz_ngram_index** out)
try {
    if (!c) return GZ_E_INVALID;
    if (!out) return fail(c, GZ_E_INVALID, "n-gram index needs an out handle");
    if (const char* why = ngram_build_fault(n_rows, skip_front, skip_back, n)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows > 0 && !row_off_dev) return fail(c, GZ_E_INVALID, "%s", kNgramBuildBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t off0 = 0, n_ids = 0;
    if (n_rows > 0) {
        int rc;
        if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
        if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kNgramBuildBuffers);
        if (!ngram_ids_fit(n_ids)) return fail(c, GZ_E_LIMIT, "%s", kNgramIdsLimit);
    }
    return ngram_build_locked(c, ids_dev, row_off_dev, n_rows, off0, n_ids, skip_front, skip_back, n, out);
} GZ_CATCH(c)

int gz_ngram_index_build(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t n,
                         gz_ngram_index** out)
try {
    if (!c) return GZ_E_INVALID;
    if (!out) return fail(c, GZ_E_INVALID, "n-gram index needs an out handle");
    if (const char* why = ngram_build_fault(n_rows, skip_front, skip_back, n)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows > 0 && (!row_off || (!ids && row_off[n_rows] != row_off[0]))) return fail(c, GZ_E_INVALID, "%s", kNgramBuildBuffers);
    const int64_t zero = 0;
    RowsIn in{ids, n_rows > 0 ? row_off : &zero, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    if (!ngram_ids_fit(in.n)) return fail(c, GZ_E_LIMIT, "%s", kNgramIdsLimit);
    if (!minhash_bodies_fit(in.off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, 0))) return rc;
    return ngram_build_locked(c, (const int32_t*)in.d_payload, in.d_off, n_rows, in.off[0], in.n, skip_front, skip_back, n, out);
} GZ_CATCH(c)

int gz_ngram_index_info(gz_ngram_index* ix, int64_t info[8])
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!info) return fail(c, GZ_E_INVALID, "n-gram index info needs info[8]");
    std::lock_guard<std::mutex> lk(c->mu);
    int64_t live = 0;
    for (const gz_ngram_index* x : c->ngram_live) live += x->device_bytes();
    const int64_t v[8] = {ix->n, ix->n_rows, ix->n_ids, ix->n_pos, ix->n_distinct, (int64_t)ix->slots, ix->device_bytes(), live};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

void gz_ngram_index_destroy(gz_ngram_index* ix)
try {
    if (!ix) return;
    gz_ctx* c = ix->c;
    std::lock_guard<std::mutex> lk(c->mu);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);                             // (a query into device memory may still read the index)
    auto& v = c->ngram_live;
    v.erase(std::remove(v.begin(), v.end(), ix), v.end());
    delete ix;
} GZ_CATCH_VOID

int gz_ngram_overlap_device(gz_ctx* c, gz_ngram_index* ix, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front,
                            int32_t skip_back, int32_t* n_grams_dev, int32_t* n_hits_dev, int32_t* n_covered_dev, int32_t* first_hit_dev,
                            int32_t* first_ref_dev, uint8_t* covered_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (!ix) return fail(c, GZ_E_INVALID, "n-gram overlap needs an index");
    int rc;
    if ((rc = ngram_overlap_rule(c, ix, n_rows, skip_front, skip_back))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!ids_dev || !row_off_dev) return fail(c, GZ_E_INVALID, "%s", kNgramOverlapBuffers);
    const NgramOut O{n_grams_dev, n_hits_dev, n_covered_dev, first_hit_dev, first_ref_dev, covered_dev};
    if (!ngram_overlap_disjoint(ids_dev, 4, row_off_dev, n_rows, O, nullptr, 0)) return fail(c, GZ_E_INVALID, "%s", kNgramOverlapDisjoint);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ngram_overlap_locked(c, ix, ids_dev, row_off_dev, n_rows, skip_front, skip_back, O))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_overlap(gz_ctx* c, gz_ngram_index* ix, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                     int32_t* n_grams, int32_t* n_hits, int32_t* n_covered, int32_t* first_hit, int32_t* first_ref, uint8_t* covered)
try {
    if (!c) return GZ_E_INVALID;
    if (!ix) return fail(c, GZ_E_INVALID, "n-gram overlap needs an index");
    int rc;
    if ((rc = ngram_overlap_rule(c, ix, n_rows, skip_front, skip_back))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!row_off || (!ids && row_off[n_rows] != row_off[0])) return fail(c, GZ_E_INVALID, "%s", kNgramOverlapBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    const NgramOut O{n_grams, n_hits, n_covered, first_hit, first_ref, covered};
    if (!ngram_overlap_disjoint(in.n ? ids + row_off[0] : nullptr, (uintptr_t)in.n * 4u, row_off, n_rows, O, covered && in.n ? covered + row_off[0] : nullptr,
                                (uintptr_t)in.n))
        return fail(c, GZ_E_INVALID, "%s", kNgramOverlapDisjoint);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, 0))) return rc;
    const size_t per_row = (size_t)n_rows * 4;
    StagedOut S;
    S.add(covered && in.n ? covered + row_off[0] : nullptr, (size_t)in.n, true);
    S.add(n_grams, per_row, false); S.add(n_hits, per_row, false); S.add(n_covered, per_row, false); S.add(first_hit, per_row, false);
    S.add(first_ref, per_row, false);
    if ((rc = staged_ensure(c, S))) return rc;
    const NgramOut D{S.dev(1), S.dev(2), S.dev(3), S.dev(4), S.dev(5), S.e[0].dev ? (uint8_t*)S.e[0].dev - row_off[0] : nullptr};
    if ((rc = ngram_overlap_locked(c, ix, (const int32_t*)in.d_payload, in.d_off, n_rows, skip_front, skip_back, D))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

}  // extern "C"
