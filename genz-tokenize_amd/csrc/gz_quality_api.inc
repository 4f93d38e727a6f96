// Text quality signals and the duplicate lines and paragraphs of a document behind the C ABI (gz_text_signals, gz_text_signals_device).
// Included by gz_api.cpp behind gz_bm25_api.inc, whose scan (bm_scan, BMW_BSUM) turns the line and paragraph counts into offsets, and
// gz_rows_api.inc, whose row front stages the host form's text (RowsIn, rows_check, rows_stage); the kernels are in gz_quality.inc,
// the argument rules without HIP in them in gz_rowrules.h (quality_fault, quality_disjoint, quality_spans_fit).
//
// A call owns nothing beyond the context's workspace (w_q, QW_*): 56 bytes of control words, 64 bytes a document (counts, scans and
// pass A's signals), 48 bytes a span (both halves, document, slot), 8 bytes a slot, 4 bytes a possible long span.  It waits ONCE, for
// the control words of pass A -- totals, extent, refusals --, and nothing of the caller's is written before that wait is over.

namespace {
enum { QW_CTL, QW_CNT, QW_OFF, QW_SIG, QW_SPAN, QW_TAB, QW_LONG, QW_STAGE };
const char* const kQualityOffsets = "text signals need offsets that do not decrease";
const char* const kQualityDocLimit = "a document holds 2^31 bytes or more: split it";
const char* const kQualityDocsLimit = "text signals take fewer than 2^31 documents a call: shard them";
const char* const kQualitySpanLimit = "text signals take fewer than 2^32 - 1 lines plus paragraphs a call: shard the documents";
const char* const kQualityDisjoint = "text signals need output arrays that overlap neither the input nor each other";

// The call on the context's stream, behind whatever it holds; the caller waits for the outputs.  D: the outputs as DEVICE pointers;
// `seen`: the arrays as the caller passed them (text biased like text_dev), for the overlap rule.  n_docs > 0.
// totals (may be null): the lines and the paragraphs of the call.
int quality_locked(gz_ctx* c, const uint8_t* text_dev, const int64_t* off_dev, int64_t n_docs, const QualityOut& D, const void* seen_text,
                   const void* seen_off, const QualityOut& seen, uint64_t* totals)
{
    int rc;
    DBuf* const w = c->w_q;
    const size_t N = (size_t)n_docs;
    if ((rc = ensure(c, w[QW_CTL], 64)) || (rc = ensure(c, w[QW_CNT], N * 8)) || (rc = ensure(c, w[QW_OFF], (N + 1) * 8)) ||
        (rc = ensure(c, w[QW_SIG], N * 4 * GZ_Q_SIGNALS)) || (rc = bm_alloc(c, c->w_bm[BMW_BSUM], (N / 4096 + 2) * 4)))
        return rc;
    GzQualityArgs A{};
    A.text = text_dev; A.off = off_dev; A.n_docs = n_docs;
    A.wsig = (int32_t*)w[QW_SIG].p; A.signals = D.signals;
    A.lcnt = (uint32_t*)w[QW_CNT].p; A.pcnt = A.lcnt + N; A.ctl = (unsigned long long*)w[QW_CTL].p;
    uint32_t* const loff = (uint32_t*)w[QW_OFF].p;
    uint32_t* const poff = loff + N + 1;
    A.loff = loff; A.poff = poff;
    HIPCHK(c, hipMemsetAsync(A.ctl, 0, 64, c->stream));
    gz_launch_quality_count(A, c->stream);
    if ((rc = bm_scan(c, A.lcnt, n_docs, loff)) || (rc = bm_scan(c, A.pcnt, n_docs, poff))) return rc;
    unsigned long long h[GZ_QC_WORDS] = {};
    if ((rc = copy_out_small(c, h, A.ctl, sizeof h, c->stream))) return rc;
    if (h[GZ_QC_FLAGS] & 1ull) return fail(c, GZ_E_INVALID, "%s", kQualityOffsets);
    if (h[GZ_QC_FLAGS] & 2ull) return fail(c, GZ_E_LIMIT, "%s", kQualityDocLimit);
    const uint64_t L = h[GZ_QC_LINES], P = h[GZ_QC_PARAS];
    if (!quality_spans_fit(L, P)) return fail(c, GZ_E_LIMIT, "%s", kQualitySpanLimit);
    const int64_t off0 = (int64_t)h[GZ_QC_OFF0], n_bytes = (int64_t)(h[GZ_QC_OFFN] - h[GZ_QC_OFF0]);
    if (!quality_disjoint((const uint8_t*)seen_text + off0, (uintptr_t)n_bytes, seen_off, n_docs, GZ_Q_SIGNALS, L, P, seen))
        return fail(c, GZ_E_INVALID, "%s", kQualityDisjoint);
    if (totals) { totals[0] = L; totals[1] = P; }
    if (D.line_off) HIPCHK(c, hipMemcpyAsync(D.line_off, loff, (N + 1) * 4, hipMemcpyDeviceToDevice, c->stream));
    if (D.para_off) HIPCHK(c, hipMemcpyAsync(D.para_off, poff, (N + 1) * 4, hipMemcpyDeviceToDevice, c->stream));
    if (!D.signals && !D.line_span && !D.line_first && !D.para_span && !D.para_first) return GZ_OK;
    const size_t S = (size_t)(L + P);
    const uint64_t slots = gz_quality_slots((int64_t)S);
    uint64_t long_max = 2 * ((uint64_t)n_bytes / 513u);                    // lines and paragraphs above 512 bytes: no more than fit the text
    if (long_max > S) long_max = S;
    if ((rc = ensure(c, w[QW_SPAN], (S + 1) * 4 * GZ_QUALITY_SPAN_WORDS)) || (rc = ensure(c, w[QW_TAB], (size_t)slots * 8)) ||
        (rc = ensure(c, w[QW_LONG], ((size_t)long_max + 1) * 4)))
        return rc;
    uint32_t* const sp = (uint32_t*)w[QW_SPAN].p;
    uint32_t** const dst[GZ_QUALITY_SPAN_WORDS] = {&A.sp_start, &A.sp_end, &A.sp_cs, &A.sp_ce, &A.sp_fs1, &A.sp_fs2, &A.sp_fe1, &A.sp_fe2,
                                                   &A.sp_i1, &A.sp_i2, &A.sp_doc, &A.sp_slot};
    for (int k = 0; k < GZ_QUALITY_SPAN_WORDS; ++k) *dst[k] = sp + (size_t)k * S;
    A.n_lines = (int64_t)L; A.n_spans = (int64_t)S;
    A.table = (unsigned long long*)w[QW_TAB].p; A.mask = slots - 1;
    const int bits = c->opt.quality_hash_bits;
    A.hmask = bits > 0 ? (1ull << bits) - 1ull : ~0ull;
    A.long_list = (uint32_t*)w[QW_LONG].p;
    A.line_span = D.line_span; A.line_first = D.line_first; A.para_span = D.para_span; A.para_first = D.para_first;
    if (S) HIPCHK(c, hipMemsetAsync(A.table, 0, (size_t)slots * 8, c->stream));
    gz_launch_quality_spans(A, (int64_t)long_max, c->stream);
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_text_signals_device(gz_ctx* c, const uint8_t* text_dev, const int64_t* off_dev, int64_t n_docs, int32_t* signals_dev, uint32_t* line_off_dev,
                           int64_t* line_span_dev, int32_t* line_first_dev, uint32_t* para_off_dev, int64_t* para_span_dev, int32_t* para_first_dev)
try {
    if (!c) return GZ_E_INVALID;
    const QualityOut O{signals_dev, line_off_dev, line_span_dev, line_first_dev, para_off_dev, para_span_dev, para_first_dev};
    if (const char* why = quality_fault(n_docs, text_dev, off_dev, O)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_docs == 0) return GZ_OK;
    if (n_docs >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kQualityDocsLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = quality_locked(c, text_dev, off_dev, n_docs, O, text_dev, off_dev, O, nullptr))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_text_signals(gz_ctx* c, const uint8_t* text, const int64_t* off, int64_t n_docs, int32_t* signals, uint32_t* line_off, int64_t* line_span,
                    int32_t* line_first, uint32_t* para_off, int64_t* para_span, int32_t* para_first)
try {
    if (!c) return GZ_E_INVALID;
    const QualityOut O{signals, line_off, line_span, line_first, para_off, para_span, para_first};
    if (const char* why = quality_fault(n_docs, text, off, O)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_docs == 0) return GZ_OK;
    if (n_docs >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kQualityDocsLimit);
    RowsIn in{text, off, n_docs, 1};
    int rc;
    if ((rc = rows_check(c, in, RowsWords{kQualityOffsets, kQualityOffsets}))) return rc;
    for (int64_t d = 0; d < n_docs; ++d) if (off[d + 1] - off[d] >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kQualityDocLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, 0))) return rc;
    // The outputs' places in the workspace.  Lines <= paragraphs' bound: a word heads each, and a word needs a byte and, unless it
    // ends its document, a separator; the staged arrays are sized by that bound, the copies by the totals of the call.
    const size_t N = (size_t)n_docs, bound = ((size_t)in.n + N) / 2 + 1;
    const size_t bytes[7] = {N * 4 * GZ_Q_SIGNALS, (N + 1) * 4, bound * 16, bound * 4, (N + 1) * 4, bound * 16, bound * 4};
    void* const host[7] = {signals, line_off, line_span, line_first, para_off, para_span, para_first};
    size_t at[7], total = 0;
    for (int k = 0; k < 7; ++k) { at[k] = total; if (host[k]) total += (bytes[k] + 255) & ~(size_t)255; }
    if ((rc = ensure(c, c->w_q[QW_STAGE], total + 256))) return rc;
    uint8_t* const st = (uint8_t*)c->w_q[QW_STAGE].p;
    auto dev = [&](int k) -> void* { return host[k] ? st + at[k] : nullptr; };
    const QualityOut D{(int32_t*)dev(0), (uint32_t*)dev(1), (int64_t*)dev(2), (int32_t*)dev(3), (uint32_t*)dev(4), (int64_t*)dev(5), (int32_t*)dev(6)};
    uint64_t totals[2] = {0, 0};
    if ((rc = quality_locked(c, (const uint8_t*)in.d_payload, in.d_off, n_docs, D, text, off, O, totals))) return rc;
    const size_t out_bytes[7] = {bytes[0], bytes[1], (size_t)totals[0] * 16, (size_t)totals[0] * 4, bytes[4], (size_t)totals[1] * 16, (size_t)totals[1] * 4};
    size_t largest = 0;
    for (int k = 0; k < 7; ++k) if (host[k] && out_bytes[k] > largest) largest = out_bytes[k];
    HostPool pool(pool_threads(c, largest));
    for (int k = 0; k < 7; ++k)
        if (host[k] && (rc = copy_out(c, host[k], dev(k), out_bytes[k], c->stream, &pool))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

}  // extern "C"
