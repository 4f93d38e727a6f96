// Modified Kneser-Ney over an n-gram model behind the C ABI (gz_ngram_lm_kn_prepare, gz_ngram_lm_kn_info, gz_ngram_lm_kn_discounts,
// gz_ngram_lm_score_kn*).  Included by gz_api.cpp behind gz_lm_api.inc, whose model, liveness rule, lock discipline and row front it
// shares; the kernels are in gz_lm_kn.inc, the argument rules and the discounts without HIP in them in gz_rowrules.h (lm_kn_score_fault,
// lm_kn_discounts).
//
// The sidecar (4 + 16 bytes a slot) belongs to the model and is derived once, on the first prepare or score call: two clears, two
// launches, one wait for the 4 + 4 N cells.  A prepare that fails for memory frees what it took and leaves the model as it was: the
// Stupid Backoff calls never look at the sidecar.  A score call waits as gz_ngram_lm_score does.

namespace {
const char* const kKnCells = "internal: the Kneser-Ney derivation read back counts that do not add up";

int lm_kn_prepare_locked(gz_ctx* c, gz_ngram_lm* lm)
{
    if (lm->kn_ready) return GZ_OK;
    int rc;
    if ((rc = ensure(c, c->w_lm_aux, GZ_LM_KN_CELLS * 8))) return rc;
    if ((rc = ensure(c, lm->kn_left, (size_t)lm->slots * 4)) || (rc = ensure(c, lm->kn_rec, (size_t)lm->slots * 16))) {
        release(lm->kn_left); release(lm->kn_rec);
        return rc;
    }
    GzLmKnArgs K{};
    K.M.order = lm->order;
    K.M.table = (unsigned long long*)lm->table.p; K.M.mask = lm->slots - 1; K.M.hmask = lm->hmask;
    K.M.ref_ids = (const int32_t*)lm->ids.p; K.M.ref_n_ids = lm->n_ids;
    K.slots = lm->slots; K.left = (uint32_t*)lm->kn_left.p; K.rec = (uint32_t*)lm->kn_rec.p;
    K.cells = (unsigned long long*)c->w_lm_aux.p;
    gz_launch_lm_kn_derive(K, c->stream);
    GzPinned* const h = c->pin;
    for (int i = 0; i < GZ_LM_KN_CELLS; ++i) h->kn_cells[i] = -1;
    HIPCHK(c, hipMemcpyAsync(h->kn_cells, K.cells, GZ_LM_KN_CELLS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const int64_t* const v = h->kn_cells;
    bool ok = v[0] >= 1 && v[0] < ((int64_t)1 << 32) && v[1] >= 0 && v[2] >= 0 && v[3] >= 0 && v[1] + v[2] + v[3] == lm->n_distinct[0];
    for (int k = 0; k < lm->order && ok; ++k) {
        int64_t sum = 0;
        for (int j = 0; j < 4; ++j) { ok = ok && v[4 + 4 * k + j] >= 0; sum += v[4 + 4 * k + j]; }
        ok = ok && sum <= lm->n_distinct[k];
    }
    if (!ok) return fail(c, GZ_E_HIP, "%s", kKnCells);
    for (int i = 0; i < GZ_LM_KN_CELLS; ++i) lm->kn_cells[i] = v[i];
    for (int k = 0; k < lm->order; ++k) lm->kn_fallback[k] = lm_kn_discounts(lm->kn_cells + 4 + 4 * k, lm->kn_D[k]);
    lm->kn_ready = true;
    return GZ_OK;
}

struct LmKnOut { int32_t* n_tokens; uint64_t* bits_fx; int32_t* n_order; uint8_t* token_order; uint32_t* token_bits_fx; };

// the handle and the argument rules of a Kneser-Ney score call; c not null, the caller holds the context's lock (lm_score_rule)
int lm_kn_score_rule(gz_ctx* c, gz_ngram_lm* lm, int64_t n_rows, int32_t skip_front, int32_t skip_back, const double* discounts)
{
    if (!lm) return fail(c, GZ_E_INVALID, "perplexity needs a model");
    if (!lm_live(c, lm)) return fail(c, GZ_E_INVALID, "the n-gram model is destroyed or belongs to another context");
    if (const char* why = lm_kn_score_fault(n_rows, skip_front, skip_back, discounts, lm->order)) return fail(c, GZ_E_INVALID, "%s", why);
    return GZ_OK;
}

bool lm_kn_disjoint(const void* ids_at, uintptr_t n_ids, const int64_t* row_off, int64_t n_rows, int32_t order, const LmKnOut& O, const void* tok_order_at,
                    const void* tok_bits_at)
{
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 64)) return false;                                   // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows;
    const Span s[7] = {span_of(ids_at, n_ids * 4u), span_of(row_off, (n + 1) * 8u), span_of(O.n_tokens, n * 4u), span_of(O.bits_fx, n * 8u),
                       span_of(O.n_order, n * 4u * (uintptr_t)(order + 1)), span_of(tok_order_at, n_ids), span_of(tok_bits_at, n_ids * 4u)};
    return disjoint(s, 7);
}

// The score call on the context's stream, behind whatever it holds; the caller waits for the outputs.  Every pointer of O a device
// pointer, the per-token ones indexed like ids_dev.  Prepares the model first.  n_rows > 0.
int lm_kn_score_locked(gz_ctx* c, gz_ngram_lm* lm, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                       const double* discounts, const LmKnOut& O)
{
    int rc;
    if ((rc = lm_kn_prepare_locked(c, lm))) return rc;
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, 1, GZ_PIECES_NGRAMS, false, nullptr, &P))) return rc;
    GzLmKnArgs K{};
    GzLmArgs& A = K.M;
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows;
    A.skip_front = skip_front; A.skip_back = skip_back; A.order = lm->order;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.table = (unsigned long long*)lm->table.p; A.mask = lm->slots - 1; A.hmask = lm->hmask;
    A.ref_ids = (const int32_t*)lm->ids.p; A.ref_n_ids = lm->n_ids;
    A.n_tokens = O.n_tokens; A.bits_fx = (unsigned long long*)O.bits_fx; A.n_order = O.n_order; A.token_order = O.token_order;
    K.slots = lm->slots; K.left = (uint32_t*)lm->kn_left.p; K.rec = (uint32_t*)lm->kn_rec.p;
    K.token_bits_fx = O.token_bits_fx;
    for (int k = 0; k < lm->order; ++k)
        for (int j = 0; j < 3; ++j) K.D[k][j] = discounts ? discounts[3 * k + j] : lm->kn_D[k][j];
    K.p0 = 1.0 / ((double)lm->n_distinct[0] + 1.0);
    K.A0 = (uint32_t)lm->kn_cells[0];
    for (int j = 0; j < 3; ++j) K.F0[j] = (uint32_t)lm->kn_cells[1 + j];
    gz_launch_lm_kn_score(K, c->stream);
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_ngram_lm_kn_prepare(gz_ctx* c, gz_ngram_lm* lm)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!lm) return fail(c, GZ_E_INVALID, "perplexity needs a model");
    if (!lm_live(c, lm)) return fail(c, GZ_E_INVALID, "the n-gram model is destroyed or belongs to another context");
    HIPCHK(c, hipSetDevice(c->device));
    return lm_kn_prepare_locked(c, lm);
} GZ_CATCH(c)

int gz_ngram_lm_kn_info(gz_ngram_lm* lm, int64_t info[48])
try {
    if (!lm) return GZ_E_INVALID;
    gz_ctx* c = lm->c;
    if (!info) return fail(c, GZ_E_INVALID, "Kneser-Ney info needs info[48]");
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = 0; i < 48; ++i) info[i] = 0;
    info[0] = lm->kn_ready ? 1 : 0; info[1] = lm->n_distinct[0]; info[2] = (int64_t)(lm->kn_left.cap + lm->kn_rec.cap); info[7] = lm->order;
    if (!lm->kn_ready) return GZ_OK;
    for (int i = 0; i < 4; ++i) info[3 + i] = lm->kn_cells[i];
    for (int i = 0; i < 4 * GZ_LM_MAX_ORDER; ++i) info[8 + i] = lm->kn_cells[4 + i];
    for (int k = 0; k < lm->order; ++k) info[40 + k] = lm->kn_fallback[k] ? 1 : 0;
    return GZ_OK;
} GZ_CATCH(lm ? lm->c : nullptr)

int gz_ngram_lm_kn_discounts(gz_ngram_lm* lm, double out[24])
try {
    if (!lm) return GZ_E_INVALID;
    gz_ctx* c = lm->c;
    if (!out) return fail(c, GZ_E_INVALID, "Kneser-Ney discounts need out[24]");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!lm->kn_ready) return fail(c, GZ_E_INVALID, "Kneser-Ney discounts need a prepared model (gz_ngram_lm_kn_prepare)");
    for (int k = 0; k < GZ_LM_MAX_ORDER; ++k)
        for (int j = 0; j < 3; ++j) out[3 * k + j] = k < lm->order ? lm->kn_D[k][j] : 0.0;
    return GZ_OK;
} GZ_CATCH(lm ? lm->c : nullptr)

int gz_ngram_lm_score_kn_device(gz_ctx* c, gz_ngram_lm* lm, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front,
                                int32_t skip_back, const double* discounts, int32_t* n_tokens_dev, uint64_t* bits_fx_dev, int32_t* n_order_dev,
                                uint8_t* token_order_dev, uint32_t* token_bits_fx_dev)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = lm_kn_score_rule(c, lm, n_rows, skip_front, skip_back, discounts))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!row_off_dev) return fail(c, GZ_E_INVALID, "%s", kLmScoreBuffers);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t off0 = 0, n_ids = 0;
    if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
    if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kLmScoreBuffers);
    const LmKnOut O{n_tokens_dev, bits_fx_dev, n_order_dev, token_order_dev, token_bits_fx_dev};
    const bool at = n_ids > 0;
    if (!lm_kn_disjoint(at ? ids_dev + off0 : nullptr, (uintptr_t)n_ids, row_off_dev, n_rows, lm->order, O, at && O.token_order ? O.token_order + off0 : nullptr,
                        at && O.token_bits_fx ? O.token_bits_fx + off0 : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kLmDisjoint);
    if ((rc = lm_kn_score_locked(c, lm, ids_dev, row_off_dev, n_rows, skip_front, skip_back, discounts, O))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_lm_score_kn(gz_ctx* c, gz_ngram_lm* lm, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                         const double* discounts, int32_t* n_tokens, uint64_t* bits_fx, int32_t* n_order, uint8_t* token_order, uint32_t* token_bits_fx)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = lm_kn_score_rule(c, lm, n_rows, skip_front, skip_back, discounts))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!row_off || (!ids && row_off[n_rows] != row_off[0])) return fail(c, GZ_E_INVALID, "%s", kLmScoreBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    const LmKnOut O{n_tokens, bits_fx, n_order, token_order, token_bits_fx};
    const bool at = in.n > 0;
    if (!lm_kn_disjoint(at ? ids + row_off[0] : nullptr, (uintptr_t)in.n, row_off, n_rows, lm->order, O, at && token_order ? token_order + row_off[0] : nullptr,
                        at && token_bits_fx ? token_bits_fx + row_off[0] : nullptr))
        return fail(c, GZ_E_INVALID, "%s", kLmDisjoint);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = rows_stage(c, in, 0))) return rc;
    const size_t n = (size_t)n_rows;
    StagedOut S;
    S.add(at && token_order ? token_order + row_off[0] : nullptr, (size_t)in.n, true);
    S.add(at && token_bits_fx ? token_bits_fx + row_off[0] : nullptr, (size_t)in.n * 4, true);
    S.add(n_tokens, n * 4, false); S.add(bits_fx, n * 8, false); S.add(n_order, n * 4 * (size_t)(lm->order + 1), false);
    if ((rc = staged_ensure(c, S))) return rc;
    const LmKnOut D{S.dev(2), (uint64_t*)S.e[3].dev, S.dev(4), S.e[0].dev ? (uint8_t*)S.e[0].dev - row_off[0] : nullptr,
                    S.e[1].dev ? (uint32_t*)S.e[1].dev - row_off[0] : nullptr};
    if ((rc = lm_kn_score_locked(c, lm, (const int32_t*)in.d_payload, in.d_off, n_rows, skip_front, skip_back, discounts, D))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

}  // extern "C"
