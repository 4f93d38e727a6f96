// Hashed n-gram class models behind the C ABI (gz_ngram_clf_create, _destroy, _fit*, _info, _totals, _counts, _weights, _set_counts,
// _set_weights, _score*).  Included by gz_api.cpp behind gz_lm_kn_api.inc; it shares gz_lm_api.inc's lock discipline and
// gz_rows_api.inc's row front (RowsIn, rows_check, rows_stage, StagedOut for the host forms; rows_extent_device for the device forms'
// extent; pieces_count_locked at width 1: a position a body token); the kernels are in gz_clf.inc, the argument rules without HIP in
// them in gz_rowrules.h (clf_create_fault, clf_rows_fault).
//
// A model owns its counts [B][C], its weights [B][C] and, where C is no power of two, the weights again at [B][CP].  The class totals
// and what was seen live on the host.  It belongs to its context: every call on it runs on the context's stream under the context's
// lock, and gz_destroy frees what is left.  A fit waits twice before its launch (the piece count; the features and pieces per class
// with the labels' check: a refusal leaves the model as it was) and once behind it; a score call derives the weights when the counts
// changed, waits once for the piece count and once for its outputs.

struct gz_ngram_clf {
    gz_ctx* c = nullptr;
    int32_t order = 0, bits = 0, n_classes = 0, cp = 0;
    double smoothing = 1.0;
    int64_t n_rows = 0, n_features = 0;
    uint64_t total[GZ_CLF_MAX_CLASSES] = {};
    bool given = false;                  // the weights are the caller's: no counts, no fits
    bool fresh = false;                  // the weights belong to the counts as they are
    DBuf count, w, wpad;
    ~gz_ngram_clf() { release(count); release(w); release(wpad); }
    size_t cells() const { return (size_t)n_classes << bits; }
    int64_t device_bytes() const { return (int64_t)(count.cap + w.cap + wpad.cap); }
    int32_t* padded() const { return (int32_t*)(cp == n_classes ? w.p : wpad.p); }
    bool fit_lds(const gz_ctx* ctx) const { return ctx->opt.clf_lds && ((size_t)4 << bits) <= GZ_CLF_LDS_BYTES; }
    bool score_lds(const gz_ctx* ctx) const { return ctx->opt.clf_lds && (((size_t)4 * (size_t)cp) << bits) <= GZ_CLF_LDS_BYTES; }
};

namespace {
void ngram_clf_free(gz_ngram_clf* clf) { delete clf; }

const char* const kClfHandle = "the class model is NULL, destroyed or belongs to another context";
const char* const kClfFitBuffers = "a class-model fit needs ids, row_off and labels";
const char* const kClfScoreBuffers = "class bits need ids and row_off";
const char* const kClfDisjoint = "class bits need output arrays that overlap neither the input nor each other";
const char* const kClfLabel = "a class-model fit needs every label in 0..n_classes-1";
const char* const kClfGiven = "the class model holds a caller's weights: it has no counts and takes no fits";
const char* const kClfTotal = "a class total would pass 2^32 - 1: fit shards into models of their own and add the scores";
const char* const kClfStats = "internal: the class-model rows pass read back counts that do not add up";

bool clf_live(gz_ctx* c, const gz_ngram_clf* clf) { return clf && std::find(c->clf_live.begin(), c->clf_live.end(), clf) != c->clf_live.end(); }

GzClfArgs clf_args(const gz_ngram_clf* clf)
{
    GzClfArgs A{};
    A.order = clf->order; A.bits = clf->bits; A.n_classes = clf->n_classes; A.cp = clf->cp;
    A.count = (uint32_t*)clf->count.p; A.w = (int32_t*)clf->w.p; A.wpad = clf->padded();
    return A;
}

// the weights of the counts as they are, or the padded copy of a caller's weights, on the context's stream
void clf_derive_locked(gz_ctx* c, gz_ngram_clf* clf)
{
    if (clf->fresh) return;
    GzClfArgs A = clf_args(clf);
    if (clf->given) A.count = nullptr;
    A.smoothing = clf->smoothing;
    for (int k = 0; k < clf->n_classes; ++k) A.tb[k] = (double)clf->total[k] + clf->smoothing * (double)((uint64_t)1 << clf->bits);
    gz_launch_clf_derive(A, c->stream);
    clf->fresh = true;
}

// The rows' features added to the counts, on the context's stream behind whatever it holds.  A refusal leaves the model unchanged.
int clf_fit_locked(gz_ctx* c, gz_ngram_clf* clf, const int32_t* ids_dev, const int64_t* row_off_dev, const int32_t* labels_dev, int64_t n_rows,
                   int32_t skip_front, int32_t skip_back)
{
    int rc;
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, 1, GZ_PIECES_NGRAMS, false, nullptr, &P))) return rc;
    if ((rc = ensure(c, c->w_clf_aux, (GZ_CLF_STATS + GZ_CLF_MAX_CLASSES) * 8))) return rc;
    unsigned long long* const d_stats = (unsigned long long*)c->w_clf_aux.p;
    GzClfArgs A = clf_args(clf);
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.skip_front = skip_front; A.skip_back = skip_back;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces; A.labels = labels_dev;
    gz_launch_clf_rows(A, d_stats, c->stream);
    int64_t* const h = c->pin->clf_stats;
    for (int i = 0; i < GZ_CLF_STATS; ++i) h[i] = -1;
    HIPCHK(c, hipMemcpyAsync(h, d_stats, GZ_CLF_STATS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (h[2 * GZ_CLF_MAX_CLASSES]) return fail(c, GZ_E_INVALID, "%s", kClfLabel);
    int64_t pieces = 0, features = 0;
    for (int k = 0; k < GZ_CLF_MAX_CLASSES; ++k) {
        if (h[k] < 0 || h[GZ_CLF_MAX_CLASSES + k] < 0 || (k >= clf->n_classes && (h[k] || h[GZ_CLF_MAX_CLASSES + k]))) return fail(c, GZ_E_HIP, "%s", kClfStats);
        if ((uint64_t)h[k] > 0xFFFFFFFFull - clf->total[k]) return fail(c, GZ_E_LIMIT, "%s", kClfTotal);
        pieces += h[GZ_CLF_MAX_CLASSES + k]; features += h[k];
    }
    if (pieces != P.n_pieces) return fail(c, GZ_E_HIP, "%s", kClfStats);
    if ((rc = ensure(c, c->w_clf_sort, (size_t)P.n_pieces * 8))) return rc;
    A.sorted = (int64_t*)c->w_clf_sort.p;
    gz_launch_clf_fit(A, h + GZ_CLF_MAX_CLASSES, d_stats + GZ_CLF_STATS, clf->fit_lds(c), c->stream);
    for (int k = 0; k < clf->n_classes; ++k) clf->total[k] += (uint64_t)h[k];
    clf->n_rows += n_rows; clf->n_features += features; clf->fresh = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}

// the handle and the argument rules of a fit or score call; c not null, the caller holds the context's lock and keeps it
int clf_rows_rule(gz_ctx* c, gz_ngram_clf* clf, int64_t n_rows, int32_t skip_front, int32_t skip_back)
{
    if (!clf_live(c, clf)) return fail(c, GZ_E_INVALID, "%s", kClfHandle);
    if (const char* why = clf_rows_fault(n_rows, skip_front, skip_back)) return fail(c, GZ_E_INVALID, "%s", why);
    return GZ_OK;
}

struct ClfOut { int32_t* n_features; int64_t* bits_fx; int32_t* best; };

bool clf_disjoint(const void* ids_at, uintptr_t n_ids, const int64_t* row_off, int64_t n_rows, int32_t n_classes, const ClfOut& O)
{
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 64)) return false;                                   // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows;
    const Span s[5] = {span_of(ids_at, n_ids * 4u), span_of(row_off, (n + 1) * 8u), span_of(O.n_features, n * 4u),
                       span_of(O.bits_fx, n * 8u * (uintptr_t)n_classes), span_of(O.best, n * 4u)};
    return disjoint(s, 5);
}

// The score call on the context's stream, behind whatever it holds; the caller waits for the outputs.  n_rows > 0.
int clf_score_locked(gz_ctx* c, gz_ngram_clf* clf, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                     const ClfOut& O)
{
    int rc;
    clf_derive_locked(c, clf);
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, 1, GZ_PIECES_NGRAMS, false, nullptr, &P))) return rc;
    GzClfArgs A = clf_args(clf);
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.skip_front = skip_front; A.skip_back = skip_back;
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.n_features = O.n_features; A.bits_fx = (long long*)O.bits_fx; A.best = O.best;
    if (O.best && !O.bits_fx && P.n_pieces != n_rows) {                             // (a long row's best comes from its complete sums)
        if ((rc = ensure(c, c->w_clf_bits, (size_t)n_rows * (size_t)clf->n_classes * 8))) return rc;
        A.bits_fx = (long long*)c->w_clf_bits.p;
    }
    gz_launch_clf_score(A, clf->score_lds(c), c->stream);
    return GZ_OK;
}

// a whole array of the model to or from the host, under the lock
int clf_read(gz_ctx* c, void* out, const void* dev, size_t bytes)
{
    int rc;
    HostPool pool(pool_threads(c, bytes));
    if ((rc = copy_out(c, out, dev, bytes, c->stream, &pool))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_ngram_clf_create(gz_ctx* c, int32_t order, int32_t bits, int32_t n_classes, double smoothing, gz_ngram_clf** out)
try {
    if (!c) return GZ_E_INVALID;
    if (!out) return fail(c, GZ_E_INVALID, "a class model needs an out handle");
    if (const char* why = clf_create_fault(order, bits, n_classes, smoothing)) return fail(c, GZ_E_INVALID, "%s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    alloc_site(c);
    std::unique_ptr<gz_ngram_clf> clf(new gz_ngram_clf());
    clf->c = c; clf->order = order; clf->bits = bits; clf->n_classes = n_classes; clf->cp = gz_clf_cp(n_classes); clf->smoothing = smoothing;
    int rc;
    const size_t cells = clf->cells(), padded = (size_t)clf->cp << bits;
    if ((rc = ensure(c, clf->count, cells * 4)) || (rc = ensure(c, clf->w, cells * 4))) return rc;
    if (clf->cp != n_classes && (rc = ensure(c, clf->wpad, padded * 4))) return rc;
    HIPCHK(c, hipMemsetAsync(clf->count.p, 0, cells * 4, c->stream));
    if (clf->wpad.p) HIPCHK(c, hipMemsetAsync(clf->wpad.p, 0, padded * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    alloc_site(c);
    c->clf_live.push_back(clf.get());
    *out = clf.release();
    return GZ_OK;
} GZ_CATCH(c)

void gz_ngram_clf_destroy(gz_ngram_clf* clf)
try {
    if (!clf) return;
    gz_ctx* c = clf->c;
    std::lock_guard<std::mutex> lk(c->mu);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);                             // (a score call into device memory may still read the model)
    auto& v = c->clf_live;
    v.erase(std::remove(v.begin(), v.end(), clf), v.end());
    delete clf;
} GZ_CATCH_VOID

int gz_ngram_clf_fit_device(gz_ctx* c, gz_ngram_clf* clf, const int32_t* ids_dev, const int64_t* row_off_dev, const int32_t* labels_dev, int64_t n_rows,
                            int32_t skip_front, int32_t skip_back)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = clf_rows_rule(c, clf, n_rows, skip_front, skip_back))) return rc;
    if (clf->given) return fail(c, GZ_E_INVALID, "%s", kClfGiven);
    if (n_rows == 0) return GZ_OK;
    if (!row_off_dev || !labels_dev) return fail(c, GZ_E_INVALID, "%s", kClfFitBuffers);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t off0 = 0, n_ids = 0;
    if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
    if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kClfFitBuffers);
    return clf_fit_locked(c, clf, ids_dev, row_off_dev, labels_dev, n_rows, skip_front, skip_back);
} GZ_CATCH(c)

int gz_ngram_clf_fit(gz_ctx* c, gz_ngram_clf* clf, const int32_t* ids, const int64_t* row_off, const int32_t* labels, int64_t n_rows, int32_t skip_front,
                     int32_t skip_back)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = clf_rows_rule(c, clf, n_rows, skip_front, skip_back))) return rc;
    if (clf->given) return fail(c, GZ_E_INVALID, "%s", kClfGiven);
    if (n_rows == 0) return GZ_OK;
    if (!row_off || !labels || (!ids && row_off[n_rows] != row_off[0])) return fail(c, GZ_E_INVALID, "%s", kClfFitBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    for (int64_t r = 0; r < n_rows; ++r)
        if (labels[r] < 0 || labels[r] >= clf->n_classes) return fail(c, GZ_E_INVALID, "%s", kClfLabel);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    if ((rc = rows_stage(c, in, 0))) return rc;
    if ((rc = ensure(c, c->w_clf_lab, (size_t)n_rows * 4)) || (rc = copy_in(c, c->w_clf_lab.p, labels, (size_t)n_rows * 4, c->stream))) return rc;
    return clf_fit_locked(c, clf, (const int32_t*)in.d_payload, in.d_off, (const int32_t*)c->w_clf_lab.p, n_rows, skip_front, skip_back);
} GZ_CATCH(c)

int gz_ngram_clf_info(gz_ctx* c, gz_ngram_clf* clf, int64_t info[16])
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!clf_live(c, clf)) return fail(c, GZ_E_INVALID, "%s", kClfHandle);
    if (!info) return fail(c, GZ_E_INVALID, "class model info needs info[16]");
    const int64_t v[16] = {clf->order, clf->bits, clf->n_classes, clf->n_rows, clf->n_features, clf->device_bytes(), clf->given ? 1 : 0,
                           clf->fresh ? 1 : 0, clf->fit_lds(c) ? 1 : 0, clf->score_lds(c) ? 1 : 0, (int64_t)GZ_CLF_LDS_BYTES, clf->cp, 0, 0, 0, 0};
    for (int i = 0; i < 16; ++i) info[i] = v[i];
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_clf_totals(gz_ctx* c, gz_ngram_clf* clf, uint64_t* out)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!clf_live(c, clf)) return fail(c, GZ_E_INVALID, "%s", kClfHandle);
    if (!out) return fail(c, GZ_E_INVALID, "class totals need out[n_classes]");
    if (clf->given) return fail(c, GZ_E_INVALID, "%s", kClfGiven);
    for (int k = 0; k < clf->n_classes; ++k) out[k] = clf->total[k];
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_clf_counts(gz_ctx* c, gz_ngram_clf* clf, uint32_t* out)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!clf_live(c, clf)) return fail(c, GZ_E_INVALID, "%s", kClfHandle);
    if (!out) return fail(c, GZ_E_INVALID, "class counts need out[B * n_classes]");
    if (clf->given) return fail(c, GZ_E_INVALID, "%s", kClfGiven);
    HIPCHK(c, hipSetDevice(c->device));
    return clf_read(c, out, clf->count.p, clf->cells() * 4);
} GZ_CATCH(c)

int gz_ngram_clf_weights(gz_ctx* c, gz_ngram_clf* clf, int32_t* out)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!clf_live(c, clf)) return fail(c, GZ_E_INVALID, "%s", kClfHandle);
    if (!out) return fail(c, GZ_E_INVALID, "class weights need out[B * n_classes]");
    HIPCHK(c, hipSetDevice(c->device));
    clf_derive_locked(c, clf);
    return clf_read(c, out, clf->w.p, clf->cells() * 4);
} GZ_CATCH(c)

int gz_ngram_clf_set_counts(gz_ctx* c, gz_ngram_clf* clf, const uint32_t* counts)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!clf_live(c, clf)) return fail(c, GZ_E_INVALID, "%s", kClfHandle);
    if (!counts) return fail(c, GZ_E_INVALID, "class counts need counts[B * n_classes]");
    if (clf->given) return fail(c, GZ_E_INVALID, "%s", kClfGiven);
    uint64_t total[GZ_CLF_MAX_CLASSES] = {};
    const size_t B = (size_t)1 << clf->bits, C = (size_t)clf->n_classes;
    for (size_t b = 0; b < B; ++b)
        for (size_t k = 0; k < C; ++k) total[k] += counts[b * C + k];
    int64_t features = 0;
    for (size_t k = 0; k < C; ++k) {
        if (total[k] > 0xFFFFFFFFull) return fail(c, GZ_E_LIMIT, "%s", kClfTotal);
        features += (int64_t)total[k];
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = copy_in(c, clf->count.p, counts, B * C * 4, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < C; ++k) clf->total[k] = total[k];
    clf->n_rows = 0; clf->n_features = features; clf->fresh = false;
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_clf_set_weights(gz_ctx* c, gz_ngram_clf* clf, const int32_t* weights)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!clf_live(c, clf)) return fail(c, GZ_E_INVALID, "%s", kClfHandle);
    if (!weights) return fail(c, GZ_E_INVALID, "class weights need weights[B * n_classes]");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = copy_in(c, clf->w.p, weights, clf->cells() * 4, c->stream))) return rc;
    clf->given = true; clf->fresh = false;
    for (int k = 0; k < GZ_CLF_MAX_CLASSES; ++k) clf->total[k] = 0;
    clf->n_rows = clf->n_features = 0;
    clf_derive_locked(c, clf);                                   // (the copy at [B][CP])
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_clf_score_device(gz_ctx* c, gz_ngram_clf* clf, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front,
                              int32_t skip_back, int32_t* n_features_dev, int64_t* bits_fx_dev, int32_t* best_dev)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = clf_rows_rule(c, clf, n_rows, skip_front, skip_back))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!row_off_dev) return fail(c, GZ_E_INVALID, "%s", kClfScoreBuffers);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t off0 = 0, n_ids = 0;
    if ((rc = rows_extent_device(c, row_off_dev, n_rows, &off0, &n_ids))) return rc;
    if (n_ids > 0 && !ids_dev) return fail(c, GZ_E_INVALID, "%s", kClfScoreBuffers);
    const ClfOut O{n_features_dev, bits_fx_dev, best_dev};
    if (!clf_disjoint(n_ids > 0 ? ids_dev + off0 : nullptr, (uintptr_t)n_ids, row_off_dev, n_rows, clf->n_classes, O)) return fail(c, GZ_E_INVALID, "%s", kClfDisjoint);
    if ((rc = clf_score_locked(c, clf, ids_dev, row_off_dev, n_rows, skip_front, skip_back, O))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_ngram_clf_score(gz_ctx* c, gz_ngram_clf* clf, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                       int32_t* n_features, int64_t* bits_fx, int32_t* best)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the model is looked at, and held to the end)
    int rc;
    if ((rc = clf_rows_rule(c, clf, n_rows, skip_front, skip_back))) return rc;
    if (n_rows == 0) return GZ_OK;
    if (!row_off || (!ids && row_off[n_rows] != row_off[0])) return fail(c, GZ_E_INVALID, "%s", kClfScoreBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    const ClfOut O{n_features, bits_fx, best};
    if (!clf_disjoint(in.n > 0 ? ids + row_off[0] : nullptr, (uintptr_t)in.n, row_off, n_rows, clf->n_classes, O)) return fail(c, GZ_E_INVALID, "%s", kClfDisjoint);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    if ((rc = rows_stage(c, in, 0))) return rc;
    const size_t n = (size_t)n_rows;
    StagedOut S;
    S.add(n_features, n * 4, false); S.add(bits_fx, n * 8 * (size_t)clf->n_classes, false); S.add(best, n * 4, false);
    if ((rc = staged_ensure(c, S))) return rc;
    const ClfOut D{S.dev(0), (int64_t*)S.e[1].dev, S.dev(2)};
    if ((rc = clf_score_locked(c, clf, (const int32_t*)in.d_payload, in.d_off, n_rows, skip_front, skip_back, D))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

}  // extern "C"
