// Token n-gram language model and perplexity behind the C ABI (gz_ngram_lm_build*, gz_ngram_lm_info, gz_ngram_lm_destroy,
// gz_ngram_lm_score*).  Included by gz_api.cpp behind gz_ngram_api.inc, whose "internal" sentence it shares, and gz_rows_api.inc, whose
// row front both forms use (RowsIn, rows_check, rows_stage, StagedOut for the host forms; rows_extent_device for the device forms'
// extent; pieces_count_locked and its limit sentence for the count pass, at width 1: a position a body token); the kernels are in
// gz_lm.inc and gz_pieces.inc, the argument rules without HIP in them in gz_rowrules.h (lm_build_fault, lm_score_fault, lm_grams_possible,
// lm_slots).
//
// A model owns two device buffers: a copy of the training ids (so the caller's may go) and the table.  It belongs to its context:
// every call on it runs on the context's stream under the context's lock, and gz_destroy frees what is left.  The build waits three
// times (the ids' extent in the device form; the pieces with the gram positions of every order; the distinct grams), a score call
// once (the piece count) before its launch and once for its outputs.  Workspace: the row front's w_pieces and w_lm_aux (128 bytes:
// gram positions and claims per order).

struct gz_ngram_lm {
    gz_ctx* c = nullptr;
    int32_t order = 0, skip_front = 0, skip_back = 0, hash_bits = 0;
    int64_t n_rows = 0, n_ids = 0, T = 0, n_total = 0;
    int64_t n_grams[GZ_LM_MAX_ORDER] = {}, n_distinct[GZ_LM_MAX_ORDER] = {};
    uint64_t slots = 0, hmask = ~0ull;
    DBuf ids, table;
    // modified Kneser-Ney (gz_lm_kn_api.inc): the sidecar and what the derivation read back; nothing of it exists before the first prepare
    bool kn_ready = false;
    DBuf kn_left, kn_rec;
    int64_t kn_cells[GZ_LM_KN_CELLS] = {};
    double kn_D[GZ_LM_MAX_ORDER][3] = {};
    bool kn_fallback[GZ_LM_MAX_ORDER] = {};
    ~gz_ngram_lm() { release(ids); release(table); release(kn_left); release(kn_rec); }
    int64_t device_bytes() const { return (int64_t)(ids.cap + table.cap); }
};

namespace {
void ngram_lm_free(gz_ngram_lm* lm) { delete lm; }

const char* const kLmBuildBuffers = "n-gram model needs ids and row_off";
const char* const kLmScoreBuffers = "perplexity needs ids and row_off";
const char* const kLmDisjoint = "perplexity needs output arrays that overlap neither the input nor each other";
const char* const kLmIdsLimit = "an n-gram model takes fewer than 2^32 - 1 training ids: shard the corpus and add the scores' counts on the host";
const char* const kLmEmpty = "an n-gram model needs at least one training token";

bool lm_live(gz_ctx* c, const gz_ngram_lm* lm) { return std::find(c->lm_live.begin(), c->lm_live.end(), lm) != c->lm_live.end(); }

// The model of the rows ids_dev[row_off_dev[r] .. row_off_dev[r + 1]) (absolute offsets; the ids lie in [off0, off0 + n_ids)), on the
// context's stream behind whatever it holds.  Nothing is handed out before the model is complete.
int lm_build_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int64_t off0, int64_t n_ids, int32_t skip_front,
                    int32_t skip_back, int32_t order, gz_ngram_lm** out)
{
    if (n_rows == 0 || n_ids == 0) return fail(c, GZ_E_INVALID, "%s", kLmEmpty);
    alloc_site(c);
    std::unique_ptr<gz_ngram_lm> lm(new gz_ngram_lm());
    lm->c = c; lm->order = order; lm->skip_front = skip_front; lm->skip_back = skip_back; lm->n_rows = n_rows; lm->n_ids = n_ids;
    lm->hash_bits = c->opt.lm_hash_bits;
    lm->hmask = lm->hash_bits > 0 ? (1ull << lm->hash_bits) - 1ull : ~0ull;
    int rc;
    if ((rc = ensure(c, c->w_lm_aux, 2 * GZ_LM_MAX_ORDER * 8))) return rc;
    unsigned long long* const d_grams = (unsigned long long*)c->w_lm_aux.p;
    unsigned long long* const d_claims = d_grams + GZ_LM_MAX_ORDER;
    GzPinned* const h = c->pin;
    for (int k = 0; k < GZ_LM_MAX_ORDER; ++k) h->lm_stats[k] = 0;
    gz_launch_lm_count(row_off_dev, n_rows, skip_front, skip_back, order, d_grams, c->stream);
    HIPCHK(c, hipMemcpyAsync(h->lm_stats, d_grams, GZ_LM_MAX_ORDER * 8, hipMemcpyDeviceToHost, c->stream));
    Pieces P{nullptr, 0, 0};
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, 1, GZ_PIECES_NGRAMS, true, nullptr, &P))) return rc;     // (waits)
    if (!ngram_positions_possible(P.n_pos, n_ids, n_rows, skip_front, skip_back, 1) || h->lm_stats[0] != P.n_pos) return fail(c, GZ_E_HIP, "%s", kNgramPositions);
    lm->T = P.n_pos;
    if (lm->T == 0) return fail(c, GZ_E_INVALID, "%s", kLmEmpty);
    for (int k = 0; k < order; ++k) {
        if (!lm_grams_possible(h->lm_stats[k], lm->T, n_rows, k + 1)) return fail(c, GZ_E_HIP, "%s", kNgramPositions);
        lm->n_grams[k] = h->lm_stats[k];
        lm->n_total += h->lm_stats[k];
    }
    lm->slots = lm_slots(lm->n_total);
    if ((rc = ensure(c, lm->ids, (size_t)n_ids * 4 + 16)) || (rc = ensure(c, lm->table, (size_t)lm->slots * 16))) return rc;
    HIPCHK(c, hipMemcpyAsync(lm->ids.p, ids_dev + off0, (size_t)n_ids * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(lm->table.p, 0, (size_t)lm->slots * 16, c->stream));
    GzLmArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.off0 = off0;
    A.skip_front = skip_front; A.skip_back = skip_back; A.order = order;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.table = (unsigned long long*)lm->table.p; A.mask = lm->slots - 1; A.hmask = lm->hmask;
    A.ref_ids = (const int32_t*)lm->ids.p; A.ref_n_ids = n_ids;
    A.stats = d_claims; A.combine = c->opt.lm_combine;
    gz_launch_lm_build(A, c->stream);
    for (int k = 0; k < GZ_LM_MAX_ORDER; ++k) h->lm_stats[k] = 0;
    HIPCHK(c, hipMemcpyAsync(h->lm_stats, d_claims, GZ_LM_MAX_ORDER * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    for (int k = 0; k < order; ++k) lm->n_distinct[k] = h->lm_stats[k];
    alloc_site(c);
    c->lm_live.push_back(lm.get());
    *out = lm.release();
    return GZ_OK;
}

struct LmOut { int32_t* n_tokens; uint64_t* bits_fx; int32_t* n_order; uint8_t* token_order; uint32_t* token_num; uint32_t* token_den; };

// the handle and the argument rules of a score call; c not null.  The caller holds the context's lock and keeps it for as long as it
// reads the model: gz_ngram_lm_destroy takes the same lock, so a model found live here stays live until the caller lets go.
int lm_score_rule(gz_ctx* c, gz_ngram_lm* lm, int64_t n_rows, int32_t skip_front, int32_t skip_back, double alpha)
{
    if (!lm) return fail(c, GZ_E_INVALID, "perplexity needs a model");
    if (!lm_live(c, lm)) return fail(c, GZ_E_INVALID, "the n-gram model is destroyed or belongs to another context");
    if (const char* why = lm_score_fault(n_rows, skip_front, skip_back, alpha)) return fail(c, GZ_E_INVALID, "%s", why);
    return GZ_OK;
}

// ids_at / tok_*: the first id of the call and the cells that belong to it; n_ids of them.  n_rows > 0.
bool lm_disjoint(const void* ids_at, uintptr_t n_ids, const int64_t* row_off, int64_t n_rows, int32_t order, const LmOut& O, const void* tok_order_at,
                 const void* tok_num_at, const void* tok_den_at)
{
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 64)) return false;                                   // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows;
    const Span s[8] = {span_of(ids_at, n_ids * 4u), span_of(row_off, (n + 1) * 8u), span_of(O.n_tokens, n * 4u), span_of(O.bits_fx, n * 8u),
                       span_of(O.n_order, n * 4u * (uintptr_t)(order + 1)), span_of(tok_order_at, n_ids), span_of(tok_num_at, n_ids * 4u),
                       span_of(tok_den_at, n_ids * 4u)};
    return disjoint(s, 8);
}

// The score call on the context's stream, behind whatever it holds; the caller waits for the outputs.  Every pointer of O a device
// pointer, the per-token ones indexed like ids_dev.  Nothing is written to the outputs when a body is too long.  n_rows > 0.
int lm_score_locked(gz_ctx* c, gz_ngram_lm* lm, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                    double alpha, const LmOut& O)
{
    int rc;
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, 1, GZ_PIECES_NGRAMS, false, nullptr, &P))) return rc;
    GzLmArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows;
    A.skip_front = skip_front; A.skip_back = skip_back; A.order = lm->order;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.table = (unsigned long long*)lm->table.p; A.mask = lm->slots - 1; A.hmask = lm->hmask;
    A.ref_ids = (const int32_t*)lm->ids.p; A.ref_n_ids = lm->n_ids;
    A.T = (uint32_t)lm->T; A.lam = -std::log2(alpha);
    A.n_tokens = O.n_tokens; A.bits_fx = (unsigned long long*)O.bits_fx; A.n_order = O.n_order;
    A.token_order = O.token_order; A.token_num = O.token_num; A.token_den = O.token_den;
    gz_launch_lm_score(A, c->stream);
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_ngram_lm_build_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                             int32_t order, gz_ngram_lm** out)
try {
    if (!c) return GZ_E_INVALID;
    if (!out) return fail(c, GZ_E_INVALID, "n-gram model needs an out handle");
    if (const char* why = lm_build_fault(n_rows, skip_front, skip_back, order)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows > 0 && !row_off_dev) return fail(c, GZ_E_INVALID, "%s", kLmBuildBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t off0 = 0, n_ids = 0;
    if (n_rows > 0) {
        int rc;
        if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
        if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kLmBuildBuffers);
        if (!ngram_ids_fit(n_ids)) return fail(c, GZ_E_LIMIT, "%s", kLmIdsLimit);
    }
    return lm_build_locked(c, ids_dev, row_off_dev, n_rows, off0, n_ids, skip_front, skip_back, order, out);
} GZ_CATCH(c)

int gz_ngram_lm_build(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t order,
                      gz_ngram_lm** out)
try {
    if (!c) return GZ_E_INVALID;
    if (!out) return fail(c, GZ_E_INVALID, "n-gram model needs an out handle");
    if (const char* why = lm_build_fault(n_rows, skip_front, skip_back, order)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows > 0 && (!row_off || (!ids && row_off[n_rows] != row_off[0]))) return fail(c, GZ_E_INVALID, "%s", kLmBuildBuffers);
    const int64_t zero = 0;
    RowsIn in{ids, n_rows > 0 ? row_off : &zero, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    if (!ngram_ids_fit(in.n)) return fail(c, GZ_E_LIMIT, "%s", kLmIdsLimit);
    if (!minhash_bodies_fit(in.off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_rows == 0 || in.n == 0) return fail(c, GZ_E_INVALID, "%s", kLmEmpty);
    if ((rc = rows_stage(c, in, 0))) return rc;
    return lm_build_locked(c, (const int32_t*)in.d_payload, in.d_off, n_rows, in.off[0], in.n, skip_front, skip_back, order, out);
} GZ_CATCH(c)

int gz_ngram_lm_info(gz_ngram_lm* lm, int64_t info[24])
try {
    if (!lm) return GZ_E_INVALID;
    gz_ctx* c = lm->c;
    if (!info) return fail(c, GZ_E_INVALID, "n-gram model info needs info[24]");
    std::lock_guard<std::mutex> lk(c->mu);
    const int64_t v[8] = {lm->order, lm->n_rows, lm->n_ids, lm->T, (int64_t)lm->slots, lm->device_bytes(), lm->hash_bits, lm->n_total};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    for (int k = 0; k < GZ_LM_MAX_ORDER; ++k) { info[8 + k] = lm->n_grams[k]; info[16 + k] = lm->n_distinct[k]; }
    return GZ_OK;
} GZ_CATCH(lm ? lm->c : nullptr)

void gz_ngram_lm_destroy(gz_ngram_lm* lm)
try {
    if (!lm) return;
    gz_ctx* c = lm->c;
    std::lock_guard<std::mutex> lk(c->mu);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);                             // (a score call into device memory may still read the model)
    auto& v = c->lm_live;
    v.erase(std::remove(v.begin(), v.end(), lm), v.end());
    delete lm;
} GZ_CATCH_VOID

int gz_ngram_lm_score_device(gz_ctx* c, gz_ngram_lm* lm, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front,
                             int32_t skip_back, double alpha, int32_t* n_tokens_dev, uint64_t* bits_fx_dev, int32_t* n_order_dev, uint8_t* token_order_dev,
                             uint32_t* token_num_dev, uint32_t* token_den_dev)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = lm_score_rule(c, lm, n_rows, skip_front, skip_back, alpha))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!row_off_dev) return fail(c, GZ_E_INVALID, "%s", kLmScoreBuffers);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t off0 = 0, n_ids = 0;
    if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
    if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kLmScoreBuffers);
    const LmOut O{n_tokens_dev, bits_fx_dev, n_order_dev, token_order_dev, token_num_dev, token_den_dev};
    const bool at = n_ids > 0;
    if (!lm_disjoint(at ? ids_dev + off0 : nullptr, (uintptr_t)n_ids, row_off_dev, n_rows, lm->order, O, at && O.token_order ? O.token_order + off0 : nullptr,
                     at && O.token_num ? O.token_num + off0 : nullptr, at && O.token_den ? O.token_den + off0 : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kLmDisjoint);
    if ((rc = lm_score_locked(c, lm, ids_dev, row_off_dev, n_rows, skip_front, skip_back, alpha, O))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_lm_score(gz_ctx* c, gz_ngram_lm* lm, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                      double alpha, int32_t* n_tokens, uint64_t* bits_fx, int32_t* n_order, uint8_t* token_order, uint32_t* token_num, uint32_t* token_den)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = lm_score_rule(c, lm, n_rows, skip_front, skip_back, alpha))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!row_off || (!ids && row_off[n_rows] != row_off[0])) return fail(c, GZ_E_INVALID, "%s", kLmScoreBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    const LmOut O{n_tokens, bits_fx, n_order, token_order, token_num, token_den};
    const bool at = in.n > 0;
    if (!lm_disjoint(at ? ids + row_off[0] : nullptr, (uintptr_t)in.n, row_off, n_rows, lm->order, O, at && token_order ? token_order + row_off[0] : nullptr,
                     at && token_num ? token_num + row_off[0] : nullptr, at && token_den ? token_den + row_off[0] : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kLmDisjoint);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    if ((rc = rows_stage(c, in, 0))) return rc;
    const size_t n = (size_t)n_rows;
    StagedOut S;
    S.add(at && token_order ? token_order + row_off[0] : nullptr, (size_t)in.n, true);
    S.add(at && token_num ? token_num + row_off[0] : nullptr, (size_t)in.n * 4, true);
    S.add(at && token_den ? token_den + row_off[0] : nullptr, (size_t)in.n * 4, true);
    S.add(n_tokens, n * 4, false); S.add(bits_fx, n * 8, false); S.add(n_order, n * 4 * (size_t)(lm->order + 1), false);
    if ((rc = staged_ensure(c, S))) return rc;
    const LmOut D{S.dev(3), (uint64_t*)S.e[4].dev, S.dev(5), S.e[0].dev ? (uint8_t*)S.e[0].dev - row_off[0] : nullptr,
                  S.e[1].dev ? (uint32_t*)S.e[1].dev - row_off[0] : nullptr, S.e[2].dev ? (uint32_t*)S.e[2].dev - row_off[0] : nullptr};
    if ((rc = lm_score_locked(c, lm, (const int32_t*)in.d_payload, in.d_off, n_rows, skip_front, skip_back, alpha, D))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

}  // extern "C"
