// The BM25 index behind the C ABI: the index, its workspace and the host code of every gz_bm25_* call, then the entry points.
// Included by gz_api.cpp behind gz_ctx, fail, HIPCHK, ensure and the copy helpers; the kernels are in gz_bm25.inc, gz_topk.inc,
// gz_vocab.inc, gz_search.inc, gz_groups.inc, gz_snippet.inc and gz_near.inc.
// A build, an append and a word set (gz_learn_api.inc) begin with the same word front -- count, scan, words, hash, de-duplication
// rounds, first, scan: bm_front_count and bm_front_words, the only callers of those kernels.  What the host and the device forms of
// their entry points repeat is in bm_host_offsets, bm_upload, bm_read_off0 and bm_hmask.
// What changes a live index -- append, remove, compact -- has one shape: a core in three phases (A: workspace and tails only, B: every
// remaining allocation, through bm_stage and its size rule, C: one commit() that nothing below can undo), run by bm25_change, which
// owns the lock, the stage-before-drain order and the dropping of the derived lists.  The searches have theirs in bm25_search_entry.

// ---- BM25 index (gz_bm25.inc) ------------------------------------------------------------------------------------------
struct gz_bm25 {
    gz_ctx* c = nullptr;
    int64_t n_docs = 0, n_words = 0, n_terms = 0, n_ent = 0, off0 = 0;
    int64_t n_live = 0;                  // terms with df > 0: a removal (gz_bm25_remove) leaves dead terms in the table, n_terms counts them too
    int64_t text_bytes = 0;              // bytes of `text` in use: an append (gz_bm25_append) puts its batch behind them
    unsigned long long hmask = 0, pmask = 0, tmask = 0;
    // the index: a copy of the text (the terms' bytes), fieldLens, signatures, doc-major (term, count) entries, the (document, term)
    // pair table, the term table, the terms' byte ranges and df
    DBuf text, dl, sig, eoff, ent, ptab, ttab, tstart, tlen, df;
    // derived from the entries and df by the first search (bm25_postings), dropped by every change of the index: the term-major
    // postings (gz_search.inc)
    DBuf poff, pdoc;
    bool has_post = false;
    // a positional index (flags & GZ_BM25_POSITIONS) owns seq: the term id of every word, documents in id order, words in
    // str.split() order -- n_words of them; every change of the index maintains it.  woff, the exclusive scan of dl (document d =
    // seq[woff[d] .. woff[d + 1])), is derived like the postings: by the first call that reads positions, dropped by every change
    int32_t flags = 0;
    DBuf seq, woff;
    bool has_woff = false;
    ~gz_bm25() { for (DBuf* b : {&text, &dl, &sig, &eoff, &ent, &ptab, &ttab, &tstart, &tlen, &df, &poff, &pdoc, &seq, &woff}) release(*b); }
};

namespace {
enum { BMW_OFF, BMW_WOFF, BMW_BSUM, BMW_CTL, BMW_WSTART, BMW_WEND, BMW_WDOC, BMW_HASH, BMW_REP, BMW_SLOT, BMW_LIST0, BMW_LIST1, BMW_DTAB,
       BMW_FLAG, BMW_SCAN, BMW_TERM, BMW_DFS, BMW_QTEXT, BMW_QOFF, BMW_QRES, BMW_QTERM, BMW_QIDF, BMW_SCORES,
       BMW_CKEY0, BMW_CIDX0, BMW_CKEY1, BMW_CIDX1, BMW_TOUT,
       BMW_CP_FIRST, BMW_CP_NEWID, BMW_CP_ORDER, BMW_CP_NLEN, BMW_CP_TOFF,          // the canonical numbering (bm25_number)
       BMW_V_OFF, BMW_V_DF, BMW_V_BYTES,                                            // what gz_bm25_terms hands out
       BMW_P_CUR,                                                                   // the postings' cursors (bm25_postings)
       BMW_S_BM, BMW_S_WROW, BMW_S_WNS, BMW_S_WSOFF, BMW_S_TCNT, BMW_S_TBASE, BMW_S_CNT,     // a search chunk (bm25_search_locked)
       BMW_S_CAND, BMW_S_CSC, BMW_S_POS, BMW_S_PSC,
       BMW_S_XTERM, BMW_S_XOFF,                                                     // the excluded terms of a boolean search
       BMW_S_PHTERM, BMW_S_PHOFF,                                                   // the phrase terms of a phrase search
       BMW_SN_IDS, BMW_SN_OUT, BMW_SN_CNT, BMW_SN_OFF, BMW_SN_POS, BMW_SN_WORD,     // snippets and occurrences (bm25_snip_*)
       BMW_S_NRTERM, BMW_S_NROFF, BMW_S_NRWIN,                                      // the near terms and windows of a near search
       BMW_VC_WORDS, BMW_VC_OFF, BMW_VC_CNT, BMW_VC_OUT,                            // the words, counts and outputs of a vocabulary query (bm25_vocab_locked)
       BMW_G_GOFF, BMW_G_AOFF, BMW_G_IDF, BMW_G_MASK,                               // the groups of a grouped search (bm25_search_locked)
       BMW_COUNT };
static_assert(BMW_COUNT <= (int)(sizeof(gz_ctx::w_bm) / sizeof(DBuf)), "gz_ctx::w_bm is too small");

// Every error return of an index build drains the context's stream before the buffers the call owns (the index under
// construction) are freed: declared AFTER the index, destroyed before it.
struct BmDrain { gz_ctx* c; ~BmDrain() { hipStreamSynchronize(c->stream); } };

// Where the outputs of a call live (and the ids a snippet or cover call reads): the host forms go through the context's workspace
// and copy, the _device forms read and write the caller's device memory directly.
enum class BmMem { Host, Device };

// a device buffer of the BM25 paths: an allocation site of the inject_bad_alloc switch
int bm_alloc(gz_ctx* c, DBuf& b, size_t bytes)
{
    alloc_site(c);
    return ensure(c, b, bytes ? bytes : 16);
}

uint64_t bm_pow2(uint64_t x)
{
    uint64_t p = 16;
    while (p < x) p <<= 1;
    return p;
}

// every word needs a byte and, unless it ends its document, a separator: words <= (bytes + documents) / 2, which keeps word indices,
// term ids and entry offsets in 31 bits
int bm_limits(gz_ctx* c, int64_t text_bytes, int64_t n_docs)
{
    if (text_bytes + n_docs >= ((int64_t)1 << 32))
        return fail(c, GZ_E_LIMIT, "BM25 index: %lld bytes + %lld documents; the index takes fewer than 2^32", (long long)text_bytes, (long long)n_docs);
    return GZ_OK;
}

int bm_scan(gz_ctx* c, const uint32_t* in, int64_t n, uint32_t* out)
{
    gz_launch_bm25_scan(in, n, out, (uint32_t*)c->w_bm[BMW_BSUM].p, c->stream);
    return GZ_OK;
}

int bm_read_u32(gz_ctx* c, const uint32_t* src, int64_t& v)
{
    uint32_t x = 0;
    int rc = copy_out_small(c, &x, src, 4, c->stream);
    v = x;
    return rc;
}

// ---- what the entry points of the host and the device forms share ---------------------------------------------------------------
// a host form's packed offsets: n + 1 of them that do not decrease, over bytes that are there
int bm_host_offsets(gz_ctx* c, const uint8_t* text, const int64_t* off, int64_t n)
{
    const int64_t nbytes = off[n] - off[0];
    if (nbytes < 0 || (nbytes > 0 && !text)) return fail(c, GZ_E_INVALID, "bad text offsets");
    for (int64_t d = 0; d < n; ++d) if (off[d + 1] < off[d]) return fail(c, GZ_E_INVALID, "text offsets must not decrease");
    return GZ_OK;
}

// a host form's text and offsets on the device: the nbytes from off[0] on into `text_buf`, the n + 1 offsets into the workspace
int bm_upload(gz_ctx* c, DBuf& text_buf, const uint8_t* text, const int64_t* off, int64_t n, int64_t nbytes)
{
    DBuf& o = c->w_bm[BMW_OFF];
    int rc;
    if ((rc = bm_alloc(c, text_buf, (size_t)nbytes + 16)) || (rc = bm_alloc(c, o, (size_t)(n + 1) * 8))) return rc;
    if (nbytes && (rc = copy_in(c, text_buf.p, text + off[0], (size_t)nbytes, c->stream))) return rc;
    return copy_in(c, o.p, off, (size_t)(n + 1) * 8, c->stream);
}

// a device form's first offset, read back: the base of its text
int bm_read_off0(gz_ctx* c, const int64_t* off_dev, int64_t& off0)
{
    const int rc = copy_out_small(c, &off0, off_dev, 8, c->stream);
    return rc ? rc : off0 < 0 ? fail(c, GZ_E_INVALID, "negative text offset") : GZ_OK;
}

// the word hashes' mask: the whole hash but its top bit, or the low bits the switch bm25_hash_bits leaves (forced collisions)
unsigned long long bm_hmask(const gz_ctx* c)
{
    const int bits = c->opt.bm25_hash_bits;
    return bits > 0 ? (1ull << bits) - 1ull : ~0ull >> 1;
}

// ---- the word front: what a build, an append and a word set (gz_learn_api.inc) begin with ----------------------------------------
// Count, scan, words, hash, de-duplication rounds, first, scan: one function per host round trip that sizes the next buffers, both
// on the GzBm25Args the caller has begun to fill.  Workspace only: whatever else the kernels write is the caller's, so an append
// keeps its rule (tails beyond the counts).
//
// The documents' words are counted into A.wcnt (the caller's: fieldLens, their staged tail, a buffer of a word set) and scanned
// into woff; A.n_words = W.  The caller has set tb, off, n_docs, lo, hi, obase, hmask and the bases.  `whose` opens the refusal of
// offsets that decrease or leave [lo, hi].
int bm_front_count(gz_ctx* c, GzBm25Args& A, const char* whose, int64_t& W)
{
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    const int64_t N = A.n_docs, text_bytes = A.hi - A.lo, wmax = (text_bytes + N) / 2 + 1;
    int rc;
    if ((rc = bm_alloc(c, w[BMW_WOFF], (size_t)(N + 1) * 4)) || (rc = bm_alloc(c, w[BMW_CTL], 64)) ||
        (rc = bm_alloc(c, w[BMW_BSUM], (size_t)((N > wmax ? N : wmax) / 4096 + 2) * 4)))
        return rc;
    A.ctl = (uint32_t*)w[BMW_CTL].p; A.woff = (uint32_t*)w[BMW_WOFF].p;
    HIPCHK(c, hipMemsetAsync(A.ctl, 0, 64, s));
    gz_launch_bm25(GZ_BM25_COUNT, A, nullptr, 0, nullptr, s);
    if ((rc = bm_scan(c, A.wcnt, N, A.woff))) return rc;
    int64_t bad = 0;
    if ((rc = bm_read_u32(c, A.ctl + 1, bad)) || (rc = bm_read_u32(c, A.woff + N, W))) return rc;
    if (bad) return fail(c, GZ_E_INVALID, "%s offsets decrease or leave the %lld bytes of text", whose, (long long)text_bytes);
    A.n_words = W;
    return GZ_OK;
}

// The words' byte ranges and hashes, then the distinct ones among them: rep, flag and its scan; T = the words that are the first
// of their bytes.  Where the kernels are to write term ids, the caller has set A.term (and a build A.ptab, which they leave alone).
// known (an append; A.ttab, tmask, tstart and tlen are the live term table's): the words that are terms already leave first, and
// T counts the new terms.  The de-duplication table has load <= 3/4 of the words that enter the first round.
int bm_front_words(gz_ctx* c, GzBm25Args& A, bool known, int64_t& T)
{
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    const int64_t W = A.n_words;
    const size_t w1 = (size_t)W + 1;
    int rc;
    if ((rc = bm_alloc(c, w[BMW_WSTART], w1 * 8)) || (rc = bm_alloc(c, w[BMW_WEND], w1 * 8)) || (rc = bm_alloc(c, w[BMW_WDOC], w1 * 4)) ||
        (rc = bm_alloc(c, w[BMW_HASH], w1 * 8)) || (rc = bm_alloc(c, w[BMW_REP], w1 * 4)) || (rc = bm_alloc(c, w[BMW_SLOT], w1 * 4)) ||
        (rc = bm_alloc(c, w[BMW_LIST0], w1 * 4)) || (rc = bm_alloc(c, w[BMW_LIST1], w1 * 4)) ||
        (rc = bm_alloc(c, w[BMW_FLAG], w1 * 4)) || (rc = bm_alloc(c, w[BMW_SCAN], w1 * 4)))
        return rc;
    A.wstart = (int64_t*)w[BMW_WSTART].p; A.wend = (int64_t*)w[BMW_WEND].p; A.wdoc = (uint32_t*)w[BMW_WDOC].p;
    A.whash = (unsigned long long*)w[BMW_HASH].p; A.rep = (uint32_t*)w[BMW_REP].p; A.wslot = (uint32_t*)w[BMW_SLOT].p;
    A.flag = (uint32_t*)w[BMW_FLAG].p; A.scan = (uint32_t*)w[BMW_SCAN].p;
    gz_launch_bm25(GZ_BM25_WORDS, A, nullptr, 0, nullptr, s);
    gz_launch_bm25(GZ_BM25_HASH, A, nullptr, 0, nullptr, s);
    const uint32_t* list = nullptr;                           // (no list: every word)
    int64_t n = W;
    if (known) {
        list = (const uint32_t*)w[BMW_LIST1].p;
        gz_launch_bm25(GZ_BM25_KNOWN, A, nullptr, 0, (uint32_t*)w[BMW_LIST1].p, s);
        if ((rc = bm_read_u32(c, A.ctl, n))) return rc;
    }
    const uint64_t slots = bm_pow2((uint64_t)n + (uint64_t)n / 3 + 16);
    if ((rc = bm_alloc(c, w[BMW_DTAB], slots * 16))) return rc;
    A.dtab = (GzBm25Slot*)w[BMW_DTAB].p; A.dmask = slots - 1;
    // each round settles at least the word that wins each slot, so the rounds end; with the whole hash there is one
    for (int64_t k = 0; n > 0; ++k) {
        uint32_t* next = (uint32_t*)w[BMW_LIST0 + (k & 1)].p;
        HIPCHK(c, hipMemsetAsync(A.dtab, 0, slots * 16, s));
        HIPCHK(c, hipMemsetAsync(A.ctl, 0, 4, s));
        gz_launch_bm25(GZ_BM25_DEDUP_INS, A, list, n, nullptr, s);
        gz_launch_bm25(GZ_BM25_DEDUP_RES, A, list, n, next, s);
        if ((rc = bm_read_u32(c, A.ctl, n))) return rc;
        list = next;
    }
    gz_launch_bm25(GZ_BM25_FIRST, A, nullptr, 0, nullptr, s);
    if ((rc = bm_scan(c, A.flag, W, A.scan))) return rc;
    return bm_read_u32(c, A.scan + W, T);
}

// The build after the text is in ix->text: off_dev = the documents' absolute offsets (device), text_bytes = bytes from off[0].
// Four host round trips: the word count, each de-duplication round's leftovers (one round unless hashes collide), the term count
// and the entry count size the next buffers.
int bm25_build_core(gz_ctx* c, gz_bm25* ix, const int64_t* off_dev, int64_t text_bytes)
{
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    const int64_t N = ix->n_docs;
    const bool pos = (ix->flags & GZ_BM25_POSITIONS) != 0;
    int rc;
    GzBm25Args A{};
    A.tb = (const uint8_t*)ix->text.p - ix->off0;
    A.off = off_dev; A.n_docs = N; A.lo = ix->off0; A.hi = ix->off0 + text_bytes;
    ix->text_bytes = text_bytes;
    ix->hmask = A.hmask = bm_hmask(c);
    if ((rc = bm_alloc(c, ix->dl, (size_t)N * 4)) || (rc = bm_alloc(c, ix->sig, (size_t)N * 32)) || (rc = bm_alloc(c, ix->eoff, (size_t)(N + 1) * 4)))
        return rc;
    A.wcnt = (uint32_t*)ix->dl.p; A.sig = (unsigned long long*)ix->sig.p; A.eoff = (uint32_t*)ix->eoff.p;
    if (N) HIPCHK(c, hipMemsetAsync(A.sig, 0, (size_t)N * 32, s));
    int64_t W = 0, T = 0;
    if ((rc = bm_front_count(c, A, "BM25 index: document", W))) return rc;
    ix->n_words = W;
    const uint64_t slots = bm_pow2((uint64_t)W + (uint64_t)W / 3 + 16);           // load <= 3/4 in the pair table
    if ((rc = bm_alloc(c, pos ? ix->seq : w[BMW_TERM], pos ? (size_t)W * 4 : ((size_t)W + 1) * 4)) || (rc = bm_alloc(c, ix->ptab, slots * 16)))
        return rc;
    A.term = (uint32_t*)(pos ? ix->seq : w[BMW_TERM]).p;     // (a positional index owns the words' term ids: they are its seq)
    A.ptab = (GzBm25Slot*)ix->ptab.p; A.pmask = ix->pmask = slots - 1;
    if ((rc = bm_front_words(c, A, false, T))) return rc;

    // ---- term table, pairs, df, signatures, entries
    ix->n_terms = ix->n_live = T;
    const uint64_t tslots = bm_pow2(2 * (uint64_t)T + 16);
    if ((rc = bm_alloc(c, ix->tstart, (size_t)T * 8)) || (rc = bm_alloc(c, ix->tlen, (size_t)T * 4)) || (rc = bm_alloc(c, ix->df, (size_t)T * 4)) ||
        (rc = bm_alloc(c, ix->ttab, tslots * 16)) || (rc = bm_alloc(c, w[BMW_DFS], (size_t)T * 4 * GZ_BM25_DF_SHARDS)))
        return rc;
    A.n_terms = T; A.dfs = (uint32_t*)w[BMW_DFS].p;
    A.tstart = (int64_t*)ix->tstart.p; A.tlen = (uint32_t*)ix->tlen.p; A.df = (uint32_t*)ix->df.p;
    A.ttab = (GzBm25Slot*)ix->ttab.p; A.tmask = ix->tmask = tslots - 1;
    HIPCHK(c, hipMemsetAsync(A.ttab, 0, tslots * 16, s));
    HIPCHK(c, hipMemsetAsync(A.ptab, 0, slots * 16, s));
    if (T) HIPCHK(c, hipMemsetAsync(A.dfs, 0, (size_t)T * 4 * GZ_BM25_DF_SHARDS, s));
    gz_launch_bm25(GZ_BM25_TERM, A, nullptr, 0, nullptr, s);
    gz_launch_bm25(GZ_BM25_PAIR_INS, A, nullptr, 0, nullptr, s);
    gz_launch_bm25(GZ_BM25_PAIR_FIRST, A, nullptr, 0, nullptr, s);
    gz_launch_bm25(GZ_BM25_DF, A, nullptr, 0, nullptr, s);
    if ((rc = bm_scan(c, A.flag, W, A.scan))) return rc;
    int64_t E = 0;
    if ((rc = bm_read_u32(c, A.scan + W, E))) return rc;
    ix->n_ent = E;
    if ((rc = bm_alloc(c, ix->ent, (size_t)E * 8))) return rc;
    A.ent = (uint2*)ix->ent.p;
    gz_launch_bm25(GZ_BM25_ENT, A, nullptr, 0, nullptr, s);
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}

// ---- append (gz_bm25_append) ---------------------------------------------------------------------------------------------------
// The index's buffers have a capacity (DBuf::cap) and grow geometrically.  A buffer that must grow is STAGED: a larger one is
// allocated, the live bytes are copied (a table is re-hashed) into it, and the live buffer stays as it is until commit() swaps
// the two -- after the last allocation of the call.  The stage is declared BEFORE the call's BmDrain: whatever it still holds
// (the fresh buffers of a failed call, the old ones of a successful one) is freed after the stream has drained.
struct BmStage {
    static constexpr int MAX = 12;
    DBuf* live[MAX] = {};
    DBuf fresh[MAX];
    int n = 0;
    ~BmStage() { for (int i = 0; i < n; ++i) release(fresh[i]); }
    void commit() { for (int i = 0; i < n; ++i) std::swap(*live[i], fresh[i]); }
};

// How large a staged buffer is.  Grow (an append): the live buffer itself while it has the room, else a staged one of at least twice
// its capacity.  Same (a removal): the live one's capacity, so that a later append finds the same room.  Exact (a compaction, a
// table to re-hash into, the derived lists): what a build gives a buffer of `need` bytes (bm_alloc's).
enum class BmSize { Grow, Same, Exact };

// `need` bytes behind *p, the first `keep` of them copied from the live buffer: a fresh buffer in the stage -- or, BmSize::Grow with
// room, the live buffer itself.  An allocation site of the inject_bad_alloc switch either way.
int bm_stage(gz_ctx* c, BmStage& st, DBuf& live, size_t keep, size_t need, BmSize size, void** p)
{
    alloc_site(c);
    if (size == BmSize::Grow && live.p && need <= live.cap) { *p = live.p; return GZ_OK; }
    if (st.n >= BmStage::MAX) return fail(c, GZ_E_HIP, "BM25 index: stage overflow");
    const size_t bytes = size == BmSize::Grow ? std::max(need, 2 * live.cap)
                       : size == BmSize::Same ? std::max(need ? need : 16, live.cap > 256 ? live.cap - 256 : 0)    // (ensure adds the 256 again)
                       : need ? need : 16;
    DBuf& f = st.fresh[st.n];
    int rc = ensure(c, f, bytes);
    if (rc) return rc;
    st.live[st.n++] = &live;
    if (keep) HIPCHK(c, hipMemcpyAsync(f.p, live.p, keep, hipMemcpyDeviceToDevice, c->stream));
    *p = f.p;
    return GZ_OK;
}

// n documents behind the index's own.  text_host / text_dev (one of them): the batch's first byte; off_dev: its n + 1 offsets in
// device memory, absolute from a base under which the first byte is batch_off0; add: its bytes.
// Phase A computes the batch's words and new terms beside the live index (tails beyond the counts, workspace, staged copies);
// phase B makes every remaining allocation; only then phase C commits the staged buffers and writes the term table, the pair
// table, df, the signatures and the entries.  A return before phase C leaves the index answering as before.  The word count, the
// unknown-word count, the collision rounds, the new-term count and the entry count are host round trips, as in the build.
int bm25_append_core(gz_ctx* c, gz_bm25* ix, BmStage& st, const uint8_t* text_host, const uint8_t* text_dev, const int64_t* off_dev,
                     int64_t batch_off0, int64_t n, int64_t add)
{
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    const int64_t N0 = ix->n_docs, T0 = ix->n_terms, E0 = ix->n_ent, used = ix->text_bytes, W0 = ix->n_words;
    const bool pos = (ix->flags & GZ_BM25_POSITIONS) != 0;
    int rc;
    // ---- phase A: the text, then the word front with the known terms taken out
    void* p_text = nullptr; void* p_dl = nullptr;
    auto grow = [&](DBuf& live, size_t keep, size_t need, void** p) { return bm_stage(c, st, live, keep, need, BmSize::Grow, p); };
    if ((rc = grow(ix->text, (size_t)used, (size_t)(used + add) + 16, &p_text)) || (rc = grow(ix->dl, (size_t)N0 * 4, (size_t)(N0 + n) * 4, &p_dl)))
        return rc;
    if (add && text_host && (rc = copy_in(c, (uint8_t*)p_text + used, text_host, (size_t)add, s))) return rc;
    if (add && text_dev) HIPCHK(c, hipMemcpyAsync((uint8_t*)p_text + used, text_dev, (size_t)add, hipMemcpyDeviceToDevice, s));
    GzBm25Args A{};
    A.tb = (const uint8_t*)p_text - ix->off0;
    A.off = off_dev; A.n_docs = n; A.lo = ix->off0 + used; A.hi = A.lo + add; A.obase = A.lo - batch_off0;
    A.hmask = ix->hmask;                                     // (the index's own: the switch's value of today does not enter)
    A.doc_base = (uint32_t)N0; A.term_base = (uint32_t)T0; A.ent_base = (uint32_t)E0;
    A.wcnt = (uint32_t*)p_dl + N0;
    int64_t W = 0, Tn = 0;
    if ((rc = bm_front_count(c, A, "BM25 append: document", W))) return rc;
    // the batch's term ids: workspace, or -- a positional index -- the tail of seq behind the index's own words
    void* p_seq = nullptr;
    if (pos ? (rc = grow(ix->seq, (size_t)W0 * 4, (size_t)(W0 + W) * 4, &p_seq)) : (rc = bm_alloc(c, w[BMW_TERM], ((size_t)W + 1) * 4))) return rc;
    A.term = pos ? (uint32_t*)p_seq + W0 : (uint32_t*)w[BMW_TERM].p;
    A.tstart = (int64_t*)ix->tstart.p; A.tlen = (uint32_t*)ix->tlen.p;          // (read only in this phase)
    A.ttab = (GzBm25Slot*)ix->ttab.p; A.tmask = ix->tmask;
    if ((rc = bm_front_words(c, A, true, Tn))) return rc;

    // ---- phase B: room for the new terms, pairs, rows and entries (W bounds the new pairs and entries: their count is known
    // only once the pair table has been written)
    const int64_t T1 = T0 + Tn, P1 = E0 + W;
    void *p_tstart, *p_tlen, *p_df, *p_sig, *p_eoff, *p_ent;
    if ((rc = grow(ix->tstart, (size_t)T0 * 8, (size_t)T1 * 8, &p_tstart)) || (rc = grow(ix->tlen, (size_t)T0 * 4, (size_t)T1 * 4, &p_tlen)) ||
        (rc = grow(ix->df, (size_t)T0 * 4, (size_t)T1 * 4, &p_df)) || (rc = grow(ix->sig, (size_t)N0 * 32, (size_t)(N0 + n) * 32, &p_sig)) ||
        (rc = grow(ix->eoff, (size_t)(N0 + 1) * 4, (size_t)(N0 + n + 1) * 4, &p_eoff)) || (rc = grow(ix->ent, (size_t)E0 * 8, (size_t)P1 * 8, &p_ent)))
        return rc;
    uint64_t tslots = ix->tmask + 1, pslots = ix->pmask + 1;
    void* p_ttab = ix->ttab.p; void* p_ptab = ix->ptab.p;
    if (2 * (uint64_t)T1 > tslots) {                          // load <= 1/2, as the build leaves it
        const uint64_t old = tslots;
        tslots = bm_pow2(4 * (uint64_t)T1 + 16);
        if ((rc = bm_stage(c, st, ix->ttab, 0, tslots * 16, BmSize::Exact, &p_ttab))) return rc;
        HIPCHK(c, hipMemsetAsync(p_ttab, 0, tslots * 16, s));
        gz_launch_bm25_rehash((const GzBm25Slot*)ix->ttab.p, (int64_t)old, (GzBm25Slot*)p_ttab, tslots - 1, s);
    }
    if ((uint64_t)P1 + (uint64_t)P1 / 3 + 16 > pslots) {      // load <= 3/4
        const uint64_t old = pslots;
        pslots = bm_pow2(2 * ((uint64_t)P1 + (uint64_t)P1 / 3) + 16);
        if (pslots > (1ull << 32)) pslots = 1ull << 32;       // (slot numbers are 32-bit; P1 < 2^31 still fits at <= 3/4)
        if ((rc = bm_stage(c, st, ix->ptab, 0, pslots * 16, BmSize::Exact, &p_ptab))) return rc;
        HIPCHK(c, hipMemsetAsync(p_ptab, 0, pslots * 16, s));
        gz_launch_bm25_rehash((const GzBm25Slot*)ix->ptab.p, (int64_t)old, (GzBm25Slot*)p_ptab, pslots - 1, s);
    }
    HIPCHK(c, hipGetLastError());

    // ---- phase C: nothing below allocates.  The staged buffers become the index's, then the live structures are written.
    st.commit();
    ix->tmask = tslots - 1; ix->pmask = pslots - 1;
    A.tstart = (int64_t*)p_tstart; A.tlen = (uint32_t*)p_tlen; A.df = (uint32_t*)p_df;
    A.ttab = (GzBm25Slot*)p_ttab; A.tmask = ix->tmask; A.ptab = (GzBm25Slot*)p_ptab; A.pmask = ix->pmask;
    A.dfs = A.df; A.n_terms = 0;                              // one df counter per term: the shards of the build collapse onto df itself
    A.sig = (unsigned long long*)p_sig; A.eoff = (uint32_t*)p_eoff + N0; A.ent = (uint2*)p_ent + E0;
    if (Tn) HIPCHK(c, hipMemsetAsync(A.df + T0, 0, (size_t)Tn * 4, s));
    HIPCHK(c, hipMemsetAsync(A.sig + N0 * 4, 0, (size_t)n * 32, s));
    gz_launch_bm25(GZ_BM25_TERM, A, nullptr, 0, nullptr, s);
    gz_launch_bm25(GZ_BM25_PAIR_INS, A, nullptr, 0, nullptr, s);
    gz_launch_bm25(GZ_BM25_PAIR_FIRST, A, nullptr, 0, nullptr, s);
    if ((rc = bm_scan(c, A.flag, W, A.scan))) return rc;
    gz_launch_bm25(GZ_BM25_ENT, A, nullptr, 0, nullptr, s);
    int64_t E = 0, revived = 0;
    if ((rc = bm_read_u32(c, A.scan + W, E)) || (rc = bm_read_u32(c, A.ctl + 2, revived))) return rc;
    HIPCHK(c, hipGetLastError());
    ix->n_docs = N0 + n; ix->n_words += W; ix->n_terms = T1; ix->n_ent = E0 + E; ix->text_bytes = used + add;
    ix->n_live += Tn + revived;                               // (dead terms of a removal that the batch brought back)
    return GZ_OK;
}

// ---- remove (gz_bm25_remove) ---------------------------------------------------------------------------------------------------
// The documents ids_dev[0 .. n_ids) leave the index.  Phase A marks them and scans the marks and the kept entry counts (workspace
// only); phase B makes every allocation: staged fieldLens, signatures, eoff, entries, pair table and a copy of df; then the
// kernels compact the live arrays into the staged ones, fill the pair table and take the removed documents off the copy of df --
// the live index is only read.  Phase C, after the last round trip, swaps the buffers in.  A return before it leaves the index
// answering as before.  The text copy, the term table and the terms' byte ranges stay: a term without documents is a dead entry
// (df 0) that a later append may bring back.
int bm25_remove_core(gz_ctx* c, gz_bm25* ix, BmStage& st, const int64_t* ids_dev, int64_t n_ids)
{
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    const int64_t N = ix->n_docs, T = ix->n_terms;
    const bool pos = (ix->flags & GZ_BM25_POSITIONS) != 0;
    int rc;
    // ---- phase A
    const size_t n1 = (size_t)N + 1;
    if ((rc = bm_alloc(c, w[BMW_FLAG], n1 * 4)) || (rc = bm_alloc(c, w[BMW_SCAN], n1 * 4)) || (rc = bm_alloc(c, w[BMW_SLOT], n1 * 4)) ||
        (rc = bm_alloc(c, w[BMW_WOFF], n1 * 4)) || (rc = bm_alloc(c, w[BMW_CTL], 64)) || (rc = bm_alloc(c, w[BMW_BSUM], (size_t)(N / 4096 + 2) * 4)))
        return rc;
    // (a positional index: the words every document keeps, and the word offsets before and after -- scans of fieldLens)
    if (pos && ((rc = bm_alloc(c, w[BMW_REP], n1 * 4)) || (rc = bm_alloc(c, w[BMW_LIST0], n1 * 4)) || (rc = bm_alloc(c, w[BMW_LIST1], n1 * 4))))
        return rc;
    GzBm25Rm R{};
    R.ids = ids_dev; R.n_ids = n_ids; R.n_docs = N;
    R.ctl = (uint32_t*)w[BMW_CTL].p; R.gone = (uint32_t*)w[BMW_FLAG].p; R.before = (uint32_t*)w[BMW_SCAN].p;
    R.kcnt = (uint32_t*)w[BMW_SLOT].p; R.neoff = (uint32_t*)w[BMW_WOFF].p;
    R.dl = (const uint32_t*)ix->dl.p; R.sig = (const unsigned long long*)ix->sig.p; R.eoff = (const uint32_t*)ix->eoff.p;
    R.ent = (const uint2*)ix->ent.p;
    if (pos) {
        R.seq = (const uint32_t*)ix->seq.p; R.n_words = ix->n_words;
        R.kdl = (uint32_t*)w[BMW_REP].p; R.woff = (uint32_t*)w[BMW_LIST0].p; R.nwoff = (uint32_t*)w[BMW_LIST1].p;
    }
    HIPCHK(c, hipMemsetAsync(R.ctl, 0, 64, s));
    HIPCHK(c, hipMemsetAsync(R.gone, 0, n1 * 4, s));
    gz_launch_bm25_remove(GZ_BM25_RM_MARK, R, s);
    int64_t bad = 0;
    if ((rc = bm_read_u32(c, R.ctl + 1, bad))) return rc;
    if (bad) return fail(c, GZ_E_INVALID, "BM25 remove: a document id outside [0, %lld)", (long long)N);
    gz_launch_bm25_remove(GZ_BM25_RM_COUNT, R, s);
    if ((rc = bm_scan(c, R.gone, N, R.before)) || (rc = bm_scan(c, R.kcnt, N, R.neoff))) return rc;
    if (pos && ((rc = bm_scan(c, R.dl, N, R.woff)) || (rc = bm_scan(c, R.kdl, N, R.nwoff)))) return rc;
    int64_t n_gone = 0, E1 = 0, Wold = ix->n_words, W1 = 0;
    if ((rc = bm_read_u32(c, R.before + N, n_gone)) || (rc = bm_read_u32(c, R.neoff + N, E1))) return rc;
    if (pos && ((rc = bm_read_u32(c, R.woff + N, Wold)) || (rc = bm_read_u32(c, R.nwoff + N, W1)))) return rc;
    if (Wold != ix->n_words) return fail(c, GZ_E_HIP, "BM25 remove: fieldLens sum to %lld words, the index holds %lld", (long long)Wold, (long long)ix->n_words);
    if (n_gone == 0) return GZ_OK;
    const int64_t N1 = N - n_gone;

    // ---- phase B: every allocation of the call
    const uint64_t pslots = ix->pmask + 1;
    void *p_dl, *p_sig, *p_eoff, *p_ent, *p_ptab, *p_df;
    auto same = [&](DBuf& live, size_t keep, size_t need, void** p) { return bm_stage(c, st, live, keep, need, BmSize::Same, p); };
    if ((rc = same(ix->dl, 0, (size_t)N1 * 4, &p_dl)) || (rc = same(ix->sig, 0, (size_t)N1 * 32, &p_sig)) ||
        (rc = same(ix->eoff, 0, (size_t)(N1 + 1) * 4, &p_eoff)) || (rc = same(ix->ent, 0, (size_t)E1 * 8, &p_ent)) ||
        (rc = same(ix->ptab, 0, pslots * 16, &p_ptab)) || (rc = same(ix->df, (size_t)T * 4, (size_t)T * 4, &p_df)))
        return rc;
    void* p_seq = nullptr;
    if (pos && (rc = same(ix->seq, 0, (size_t)W1 * 4, &p_seq))) return rc;
    R.seq2 = (uint32_t*)p_seq;
    R.dl2 = (uint32_t*)p_dl; R.sig2 = (unsigned long long*)p_sig; R.eoff2 = (uint32_t*)p_eoff; R.ent2 = (uint2*)p_ent;
    R.ptab2 = (GzBm25Slot*)p_ptab; R.pmask2 = ix->pmask; R.df2 = (uint32_t*)p_df;
    HIPCHK(c, hipMemsetAsync(p_ptab, 0, pslots * 16, s));
    gz_launch_bm25_remove(GZ_BM25_RM_DOCS, R, s);
    gz_launch_bm25_remove(GZ_BM25_RM_ENT, R, s);
    if (pos) gz_launch_bm25_remove(GZ_BM25_RM_SEQ, R, s);
    uint32_t out[4] = {};                                     // ctl[2 .. 5]: dead terms, -, words of the removed documents (64 bits)
    if ((rc = copy_out_small(c, out, R.ctl + 2, 16, s))) return rc;
    int64_t bad_seq = 0;
    if (pos && (rc = bm_read_u32(c, R.ctl + 1, bad_seq))) return rc;
    HIPCHK(c, hipGetLastError());
    if (bad_seq || (pos && ix->n_words - (int64_t)((uint64_t)out[2] | (uint64_t)out[3] << 32) != W1))
        return fail(c, GZ_E_HIP, "BM25 remove: the index's fieldLens and word sequence contradict each other");

    // ---- phase C: nothing below can fail
    st.commit();
    ix->n_docs = N1; ix->n_ent = E1; ix->n_live -= (int64_t)out[0];
    ix->n_words -= (int64_t)((uint64_t)out[2] | (uint64_t)out[3] << 32);
    return GZ_OK;
}

// ---- compact (gz_bm25_compact) and the vocabulary (gz_bm25_terms) ----------------------------------------------------------------
// The canonical numbering of the live terms, into the context's workspace: the index is only read.  On return C holds the live
// arrays and the workspace (newid, order, nlen, toff), C.n_new == ix->n_live is verified and B = the live terms' bytes.  Two host
// round trips: the number of flags and B.
int bm25_number(gz_ctx* c, gz_bm25* ix, GzBm25Cp& C, int64_t& B)
{
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    const int64_t T = ix->n_terms, E = ix->n_ent;
    int rc;
    const size_t e1 = (size_t)E + 1, t1 = (size_t)T + 1;
    if ((rc = bm_alloc(c, w[BMW_CTL], 64)) || (rc = bm_alloc(c, w[BMW_BSUM], (size_t)((E > T ? E : T) / 4096 + 2) * 4)) ||
        (rc = bm_alloc(c, w[BMW_FLAG], e1 * 4)) || (rc = bm_alloc(c, w[BMW_SCAN], e1 * 4)) || (rc = bm_alloc(c, w[BMW_CP_FIRST], t1 * 4)) ||
        (rc = bm_alloc(c, w[BMW_CP_NEWID], t1 * 4)) || (rc = bm_alloc(c, w[BMW_CP_ORDER], t1 * 4)) || (rc = bm_alloc(c, w[BMW_CP_NLEN], t1 * 4)) ||
        (rc = bm_alloc(c, w[BMW_CP_TOFF], t1 * 4)))
        return rc;
    C = GzBm25Cp{};
    C.n_docs = ix->n_docs; C.n_ent = E; C.n_terms = T; C.n_new = ix->n_live;
    C.tb = (const uint8_t*)ix->text.p - ix->off0; C.tstart = (const int64_t*)ix->tstart.p; C.tlen = (const uint32_t*)ix->tlen.p;
    C.df = (const uint32_t*)ix->df.p; C.ent = (const uint2*)ix->ent.p; C.eoff = (const uint32_t*)ix->eoff.p;
    C.ctl = (uint32_t*)w[BMW_CTL].p; C.flag = (uint32_t*)w[BMW_FLAG].p; C.scan = (uint32_t*)w[BMW_SCAN].p;
    C.first = (uint32_t*)w[BMW_CP_FIRST].p; C.newid = (uint32_t*)w[BMW_CP_NEWID].p; C.order = (uint32_t*)w[BMW_CP_ORDER].p;
    C.nlen = (uint32_t*)w[BMW_CP_NLEN].p; C.toff = (uint32_t*)w[BMW_CP_TOFF].p;
    HIPCHK(c, hipMemsetAsync(C.ctl, 0, 64, s));
    HIPCHK(c, hipMemsetAsync(C.first, 0xFF, t1 * 4, s));
    gz_launch_bm25_compact(GZ_BM25_CP_FIRST, C, s);
    gz_launch_bm25_compact(GZ_BM25_CP_FLAG, C, s);
    if ((rc = bm_scan(c, C.flag, E, C.scan))) return rc;
    int64_t n_new = 0;
    if ((rc = bm_read_u32(c, C.scan + E, n_new))) return rc;
    if (n_new != ix->n_live)
        return fail(c, GZ_E_HIP, "BM25 index: %lld terms have a first entry, %lld are live", (long long)n_new, (long long)ix->n_live);
    gz_launch_bm25_compact(GZ_BM25_CP_NEWID, C, s);
    if ((rc = bm_scan(c, C.nlen, n_new, C.toff))) return rc;
    if ((rc = bm_read_u32(c, C.toff + n_new, B))) return rc;
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}

// The index becomes the one a fresh build of its current documents gives, term ids included.  Phase A numbers the live terms
// (workspace only); phase B makes every allocation: all ten buffers staged, each of the size gz_bm25_build gives it for the same
// counts (the text: the live terms' bytes), so capacities that appends and removals left behind are given back; then the kernels
// fill the staged buffers from the live index, which is only read.  Phase C, after the last round trip, swaps them in.  A return
// before it leaves the index answering as before.
int bm25_compact_core(gz_ctx* c, gz_bm25* ix, BmStage& st)
{
    hipStream_t s = c->stream;
    const int64_t N = ix->n_docs, E = ix->n_ent;
    int rc;
    // ---- phase A
    GzBm25Cp C;
    int64_t B = 0;
    if ((rc = bm25_number(c, ix, C, B))) return rc;
    const int64_t T1 = C.n_new;

    // ---- phase B: every allocation of the call, sized as bm25_build_core sizes them
    const uint64_t pslots = bm_pow2((uint64_t)ix->n_words + (uint64_t)ix->n_words / 3 + 16), tslots = bm_pow2(2 * (uint64_t)T1 + 16);
    void *p_text, *p_dl, *p_sig, *p_eoff, *p_ent, *p_ptab, *p_ttab, *p_tstart, *p_tlen, *p_df;
    auto exact = [&](DBuf& live, size_t need, void** p) { return bm_stage(c, st, live, 0, need, BmSize::Exact, p); };
    if ((rc = exact(ix->text, (size_t)B + 16, &p_text)) || (rc = exact(ix->dl, (size_t)N * 4, &p_dl)) ||
        (rc = exact(ix->sig, (size_t)N * 32, &p_sig)) || (rc = exact(ix->eoff, (size_t)(N + 1) * 4, &p_eoff)) ||
        (rc = exact(ix->ent, (size_t)E * 8, &p_ent)) || (rc = exact(ix->ptab, pslots * 16, &p_ptab)) ||
        (rc = exact(ix->ttab, tslots * 16, &p_ttab)) || (rc = exact(ix->tstart, (size_t)T1 * 8, &p_tstart)) ||
        (rc = exact(ix->tlen, (size_t)T1 * 4, &p_tlen)) || (rc = exact(ix->df, (size_t)T1 * 4, &p_df)))
        return rc;
    const bool pos = (ix->flags & GZ_BM25_POSITIONS) != 0;
    void* p_seq = nullptr;
    if (pos && (rc = exact(ix->seq, (size_t)ix->n_words * 4, &p_seq))) return rc;
    if (pos) { C.seq = (const uint32_t*)ix->seq.p; C.seq2 = (uint32_t*)p_seq; C.n_words = ix->n_words; }
    C.arena = (uint8_t*)p_text; C.tstart2 = (int64_t*)p_tstart; C.tlen2 = (uint32_t*)p_tlen; C.df2 = (uint32_t*)p_df;
    C.ent2 = (uint2*)p_ent; C.sig2 = (unsigned long long*)p_sig; C.ptab2 = (GzBm25Slot*)p_ptab; C.pmask2 = pslots - 1;
    HIPCHK(c, hipMemsetAsync(p_ptab, 0, pslots * 16, s));
    HIPCHK(c, hipMemsetAsync(p_ttab, 0, tslots * 16, s));
    if (N) HIPCHK(c, hipMemcpyAsync(p_dl, ix->dl.p, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(p_eoff, ix->eoff.p, (size_t)(N + 1) * 4, hipMemcpyDeviceToDevice, s));
    gz_launch_bm25_compact(GZ_BM25_CP_GATHER, C, s);
    gz_launch_bm25_rekey((const GzBm25Slot*)ix->ttab.p, (int64_t)(ix->tmask + 1), C.newid, (GzBm25Slot*)p_ttab, tslots - 1, s);
    gz_launch_bm25_compact(GZ_BM25_CP_ENT, C, s);
    if (pos) gz_launch_bm25_compact(GZ_BM25_CP_SEQ, C, s);    // (a word whose term has no new id raises the same flag)
    int64_t bad = 0;
    if ((rc = bm_read_u32(c, C.ctl + 1, bad))) return rc;
    HIPCHK(c, hipGetLastError());
    if (bad) return fail(c, GZ_E_HIP, "BM25 compact: the index's entries, df and term table contradict each other");

    // ---- phase C: nothing below can fail
    st.commit();
    ix->n_terms = T1; ix->text_bytes = B; ix->off0 = 0;
    ix->pmask = pslots - 1; ix->tmask = tslots - 1;
    return GZ_OK;
}

// ---- what every change of a live index goes through -----------------------------------------------------------------------------
// the postings (gz_search.inc) leave: the index has changed (or is to equal a fresh build).  After the stream has drained: a search
// enqueued into device memory may still read them.
void bm25_drop_postings(gz_bm25* ix)
{
    if (!ix->has_post && !ix->has_woff) return;
    hipStreamSynchronize(ix->c->stream);
    release(ix->poff);
    release(ix->pdoc);
    release(ix->woff);                            // (a positional index's word offsets: derived from fieldLens in the same way)
    ix->has_post = ix->has_woff = false;
}

// core(stage) under the context's lock, which the caller holds: one of the three cores above, behind whatever the entry point
// still has to check or upload.  The stage is declared BEFORE the drain: whatever it still holds when the core returns -- the fresh
// buffers of a failed call, the old ones of a successful one -- is freed after the stream has drained.  On success the derived
// lists leave.
template <class Core>
int bm25_change_locked(gz_ctx* c, gz_bm25* ix, Core&& core)
{
    BmStage st;
    BmDrain drain{c};
    const int rc = core(st);
    if (!rc) bm25_drop_postings(ix);
    return rc;
}

// the same behind the lock and on the context's device: gz_bm25_append, gz_bm25_remove, their _device forms and gz_bm25_compact
template <class Core>
int bm25_change(gz_bm25* ix, Core&& core)
{
    gz_ctx* c = ix->c;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return bm25_change_locked(c, ix, core);
}

// The last step of a POSITIONAL build.  Such an index never needs the documents' text again, only its terms' bytes, so the build
// ends in the canonical form a compaction gives: the text copy is the live terms' bytes in first-occurrence order and every
// buffer has the size its counts ask for.  A fresh positional build and a compacted positional index of the same documents are
// then the same index, footprint included.  (Term ids and seq are the build's already: the numbering pass is the identity.)
int bm25_build_finish(gz_ctx* c, gz_bm25* ix)
{
    if (!(ix->flags & GZ_BM25_POSITIONS)) return GZ_OK;
    return bm25_change_locked(c, ix, [&](BmStage& st) { return bm25_compact_core(c, ix, st); });       // (a fresh index has no lists to drop)
}

int bm_adopt(gz_ctx* c, std::unique_ptr<gz_bm25>& ix, gz_bm25** out)
{
    alloc_site(c);
    c->bm25_live.push_back(ix.get());
    *out = ix.release();
    return GZ_OK;
}

// the query arrays of a scoring / top-k call -> the context's workspace, and the scoring kernel's arguments for all of them
// (S.out unset)
int bm25_query_in(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* qoff, int64_t nq, const double* P, int32_t plus,
                  GzBm25Score& S)
{
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    const int64_t nw = qoff[nq] - qoff[0];
    int rc;
    if ((rc = bm_alloc(c, w[BMW_QTERM], (size_t)nw * 4)) || (rc = bm_alloc(c, w[BMW_QIDF], (size_t)nw * 8)) ||
        (rc = bm_alloc(c, w[BMW_QOFF], (size_t)(nq + 1) * 8)))
        return rc;
    if (nw && ((rc = copy_in(c, w[BMW_QTERM].p, terms + qoff[0], (size_t)nw * 4, s)) ||
               (idf && (rc = copy_in(c, w[BMW_QIDF].p, idf + qoff[0], (size_t)nw * 8, s)))))       // (a match count has no idf and no P)
        return rc;
    if ((rc = copy_in(c, w[BMW_QOFF].p, qoff, (size_t)(nq + 1) * 8, s))) return rc;
    S = GzBm25Score{};
    S.dl = (const uint32_t*)ix->dl.p; S.sig = (const unsigned long long*)ix->sig.p; S.eoff = (const uint32_t*)ix->eoff.p;
    S.ent = (const uint2*)ix->ent.p; S.ptab = (const GzBm25Slot*)ix->ptab.p; S.pmask = ix->pmask; S.n_docs = ix->n_docs;
    S.qterm = (const int32_t*)w[BMW_QTERM].p - qoff[0]; S.qidf = (const double*)w[BMW_QIDF].p - qoff[0];
    S.qoff = (const int64_t*)w[BMW_QOFF].p; S.n_q = nq;
    if (P) { S.kp1 = P[0]; S.k1 = P[1]; S.omb = P[2]; S.b = P[3]; S.avg = P[4]; S.delta = P[5]; }
    S.plus = plus ? 1 : 0;
    return GZ_OK;
}

// the query arrays of a scoring call -> the kernel; out in host memory: into the context's workspace and back to out
int bm25_score_locked(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* qoff, int64_t nq, const double* P, int32_t plus,
                      double* out, BmMem mem)
{
    double* out_dev = mem == BmMem::Device ? out : nullptr;        // (null as well for a device form that has nothing to write)
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t N = ix->n_docs;
    GzBm25Score S;
    int rc = bm25_query_in(ix, terms, idf, qoff, nq, P, plus, S);
    if (rc) return rc;
    if (!out_dev && (rc = bm_alloc(c, w[BMW_SCORES], (size_t)(nq * N) * 8))) return rc;
    S.out = out_dev ? out_dev : (double*)w[BMW_SCORES].p;
    gz_launch_bm25_score(S, s);
    HIPCHK(c, hipGetLastError());
    if (out_dev) return GZ_OK;
    HostPool pool(pool_threads(c, (size_t)(nq * N) * 8));
    return copy_out(c, out, S.out, (size_t)(nq * N) * 8, s, &pool);
}

int bm25_score_args(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* qoff, int64_t nq, const double* P, const void* out)
{
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!qoff || nq < 0 || !P || (!out && nq > 0 && ix->n_docs > 0)) return fail(c, GZ_E_INVALID, "bad arguments");
    if (ix->n_docs > 0 && nq > ((int64_t)1 << 59) / ix->n_docs) return fail(c, GZ_E_LIMIT, "scores[%lld, %lld] too large", (long long)nq, (long long)ix->n_docs);
    const int64_t nw = qoff[nq] - qoff[0];
    if (nw < 0 || (nw > 0 && (!terms || !idf))) return fail(c, GZ_E_INVALID, "bad query offsets");
    for (int64_t q = 0; q < nq; ++q) if (qoff[q + 1] < qoff[q]) return fail(c, GZ_E_INVALID, "query offsets must not decrease");
    for (int64_t j = qoff[0]; j < qoff[nq]; ++j)
        if (terms[j] < -1 || terms[j] >= ix->n_terms) return fail(c, GZ_E_INVALID, "term id %d out of range", terms[j]);
    return GZ_OK;
}

static_assert(GZ_TOPK_SORT == GZ_BM25_TOPK_MAX, "the last selection level sorts GZ_BM25_TOPK_MAX winners in LDS");
static_assert(GZ_PHRASE_MAX == GZ_BM25_PHRASE_MAX && GZ_PHRASE_MAX <= 64, "the phrase kernel holds a phrase term per lane");
static_assert(GZ_NEAR_MAX == GZ_BM25_NEAR_MAX && GZ_NEAR_MAX <= 64, "the near and cover kernels hold a term of the set per lane");

// k (>= 1) -> k' = min(k, documents), refused above GZ_BM25_TOPK_MAX
int bm25_topk_k(gz_bm25* ix, int64_t k, int64_t& kk)
{
    if (k < 1) return fail(ix->c, GZ_E_INVALID, "k = %lld; top-k takes k >= 1", (long long)k);
    kk = k < ix->n_docs ? k : ix->n_docs;
    if (kk > GZ_BM25_TOPK_MAX) return fail(ix->c, GZ_E_LIMIT, "k = %lld over %lld documents; top-k takes at most %d", (long long)k,
                                            (long long)ix->n_docs, GZ_BM25_TOPK_MAX);
    return GZ_OK;
}

// documents per workgroup of the first selection level: bm25_topk_tile when it is set, else enough tiles for ~2048 workgroups over
// the chunk's rows (8 per CU), at least 4 k' (each tile keeps k' candidates) and 256, at most GZ_TOPK_TILE_MAX
int64_t bm25_topk_tile(const gz_ctx* c, int64_t rows, int64_t N, int64_t kk)
{
    int64_t t = c->opt.bm25_topk_tile;
    if (t <= 0) {
        const int64_t per_row = (2048 + rows - 1) / rows;
        t = std::max<int64_t>((N + per_row - 1) / per_row, std::max<int64_t>(256, 4 * kk));
        t = std::min<int64_t>(t, GZ_TOPK_TILE_MAX);
    }
    return std::max<int64_t>(t, (N + ((int64_t)1 << 30) - 1) >> 30);        // (tiles of a row fit a grid dimension)
}

// Score rows, a chunk of queries at a time, into the context's workspace (at most bm25_topk_chunk doubles, one row at least), and
// the selection levels over them; ids / scores into doc / score in device memory, or into host memory after every chunk
int bm25_topk_locked(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* qoff, int64_t nq, const double* P, int32_t plus,
                     int64_t kk, int64_t* doc, double* score, BmMem mem)
{
    const bool dev = mem == BmMem::Device;
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t N = ix->n_docs;
    if (nq == 0 || N == 0) return GZ_OK;
    const int64_t rmax = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>((int64_t)c->opt.bm25_topk_chunk / N, 1), 65535), nq);
    const int64_t tile = bm25_topk_tile(c, rmax, N, kk);
    int64_t m1, m2;
    gz_topk_sizes(N, tile, kk, m1, m2);
    GzBm25Score S;
    int rc = bm25_query_in(ix, terms, idf, qoff, nq, P, plus, S);
    if (rc) return rc;
    if ((rc = bm_alloc(c, w[BMW_SCORES], (size_t)(rmax * N) * 8)) || (rc = bm_alloc(c, w[BMW_CKEY0], (size_t)(rmax * m1) * 8)) ||
        (rc = bm_alloc(c, w[BMW_CIDX0], (size_t)(rmax * m1) * 4)) || (rc = bm_alloc(c, w[BMW_CKEY1], (size_t)(rmax * m2) * 8)) ||
        (rc = bm_alloc(c, w[BMW_CIDX1], (size_t)(rmax * m2) * 4)) || (!dev && (rc = bm_alloc(c, w[BMW_TOUT], (size_t)(rmax * kk) * 16))))
        return rc;
    GzTopk T{};
    T.scores = (const double*)w[BMW_SCORES].p; T.n_docs = N; T.k = kk; T.tile = tile;
    T.ckey[0] = (unsigned long long*)w[BMW_CKEY0].p; T.cidx[0] = (uint32_t*)w[BMW_CIDX0].p;
    T.ckey[1] = (unsigned long long*)w[BMW_CKEY1].p; T.cidx[1] = (uint32_t*)w[BMW_CIDX1].p;
    const int64_t* qoff_dev = S.qoff;
    for (int64_t q0 = 0; q0 < nq; q0 += rmax) {
        const int64_t rows = std::min(rmax, nq - q0);
        S.qoff = qoff_dev + q0; S.n_q = rows; S.out = (double*)w[BMW_SCORES].p;
        gz_launch_bm25_score(S, s);
        T.rows = rows;
        T.doc_out = dev ? doc + q0 * kk : (int64_t*)w[BMW_TOUT].p;
        T.score_out = dev ? score + q0 * kk : (double*)w[BMW_TOUT].p + rmax * kk;
        gz_launch_topk(T, s);
        HIPCHK(c, hipGetLastError());
        if (!dev && ((rc = copy_out(c, doc + q0 * kk, T.doc_out, (size_t)(rows * kk) * 8, s)) ||
                     (rc = copy_out(c, score + q0 * kk, T.score_out, (size_t)(rows * kk) * 8, s))))
            return rc;
    }
    return GZ_OK;
}

// ---- vocabulary queries (gz_bm25_similar, gz_bm25_prefix, gz_bm25_term_bytes; gz_vocab.inc) --------------------------------------
static_assert(GZ_VOCAB_EDIT_MAX == GZ_BM25_EDIT_MAX, "the distance kernel holds a state bit per code point of the query word");

// A packed word's code points behind `out`, read as gz_vocab.inc's kernel reads the terms: structural UTF-8 -- the lead byte's class
// and as many continuation bytes; surrogates and overlong forms pass.  False: the bytes are not that.
bool vc_decode(const uint8_t* p, int64_t n, std::vector<uint32_t>& out)
{
    for (int64_t i = 0; i < n;) {
        const uint32_t b0 = p[i];
        const int want = b0 < 0x80 ? 1 : b0 < 0xC0 ? 0 : b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : b0 < 0xF8 ? 4 : 0;
        if (!want || i + want > n) return false;
        uint32_t cp = want == 1 ? b0 : want == 2 ? (b0 & 0x1F) : want == 3 ? (b0 & 0x0F) : (b0 & 0x07);
        for (int k = 1; k < want; ++k) {
            if ((p[i + k] & 0xC0) != 0x80) return false;
            cp = (cp << 6) | (p[i + k] & 0x3F);
        }
        out.push_back(cp);
        i += want;
    }
    return true;
}

int bm25_vocab_args(gz_bm25* ix, const uint8_t* words, const int64_t* word_off, int64_t n, int64_t k)
{
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!word_off || n < 0) return fail(c, GZ_E_INVALID, "bad arguments");
    if (k < 1) return fail(c, GZ_E_INVALID, "k = %lld; a vocabulary query takes k >= 1", (long long)k);
    const int64_t nbytes = word_off[n] - word_off[0];
    if (nbytes < 0 || (nbytes > 0 && !words)) return fail(c, GZ_E_INVALID, "bad word offsets");
    for (int64_t i = 0; i < n; ++i) if (word_off[i + 1] < word_off[i]) return fail(c, GZ_E_INVALID, "word offsets must not decrease");
    return GZ_OK;
}

// Key rows of a chunk of words at a time in the context's workspace (at most bm25_vocab_chunk doubles, one row at least, at most
// 65535 rows), the selection levels over them, and the chunk's unpacked rows to the host.  cps / cpoff: the words' code points
// (gz_bm25_similar); null: a prefix query over the packed bytes.  The canonical numbering is scratch, as in gz_bm25_terms.
int bm25_vocab_locked(gz_bm25* ix, const uint8_t* words, const int64_t* word_off, int64_t nq, const std::vector<uint32_t>* cps,
                      const std::vector<uint32_t>* cpoff, int32_t max_edits, int64_t k, int64_t* ids_out, int32_t* dist_out, int32_t* df_out,
                      int64_t* count_out)
{
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t T = ix->n_live, kk = k < T ? k : T;
    if (kk > GZ_BM25_TOPK_MAX)
        return fail(c, GZ_E_LIMIT, "k = %lld over %lld terms; a vocabulary query takes at most %d", (long long)k, (long long)T, GZ_BM25_TOPK_MAX);
    if (nq == 0) return GZ_OK;
    if (!count_out || (kk > 0 && (!ids_out || !df_out || (cps && !dist_out)))) return fail(c, GZ_E_INVALID, "bad arguments");
    if (T == 0) {
        std::memset(count_out, 0, (size_t)nq * 8);
        return GZ_OK;
    }
    BmDrain drain{c};
    GzBm25Cp C;
    int64_t B = 0, bad = 0;
    int rc;
    if ((rc = bm25_number(c, ix, C, B)) || (rc = bm_read_u32(c, C.ctl + 1, bad))) return rc;
    if (bad) return fail(c, GZ_E_HIP, "BM25 vocabulary: the index's entries and df contradict each other");
    const int64_t rmax = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>((int64_t)c->opt.bm25_vocab_chunk / T, 1), 65535), nq);
    const int64_t tile = bm25_topk_tile(c, rmax, T, kk);
    int64_t m1, m2;
    gz_topk_sizes(T, tile, kk, m1, m2);
    const int64_t nbytes = word_off[nq] - word_off[0];
    const size_t wbytes = cps ? cps->size() * 4 : (size_t)nbytes, obytes = cps ? (size_t)(nq + 1) * 4 : (size_t)(nq + 1) * 8;
    if ((rc = bm_alloc(c, w[BMW_SCORES], (size_t)(rmax * T) * 8)) || (rc = bm_alloc(c, w[BMW_CKEY0], (size_t)(rmax * m1) * 8)) ||
        (rc = bm_alloc(c, w[BMW_CIDX0], (size_t)(rmax * m1) * 4)) || (rc = bm_alloc(c, w[BMW_CKEY1], (size_t)(rmax * m2) * 8)) ||
        (rc = bm_alloc(c, w[BMW_CIDX1], (size_t)(rmax * m2) * 4)) || (rc = bm_alloc(c, w[BMW_TOUT], (size_t)(rmax * kk) * 16)) ||
        (rc = bm_alloc(c, w[BMW_VC_WORDS], wbytes + 16)) || (rc = bm_alloc(c, w[BMW_VC_OFF], obytes)) ||
        (rc = bm_alloc(c, w[BMW_VC_CNT], (size_t)rmax * 4)) || (rc = bm_alloc(c, w[BMW_VC_OUT], (size_t)(rmax * kk) * 16 + (size_t)rmax * 8)))
        return rc;
    if (cps) {
        if ((rc = copy_in(c, w[BMW_VC_WORDS].p, cps->data(), wbytes, s)) || (rc = copy_in(c, w[BMW_VC_OFF].p, cpoff->data(), obytes, s))) return rc;
    } else if ((nbytes && (rc = copy_in(c, w[BMW_VC_WORDS].p, words + word_off[0], wbytes, s))) ||
               (rc = copy_in(c, w[BMW_VC_OFF].p, word_off, obytes, s)))
        return rc;
    GzBm25Vocab V{};
    V.tb = C.tb; V.tstart = C.tstart; V.df = C.df; V.order = C.order; V.nlen = C.nlen; V.n_new = T;
    V.max_edits = max_edits; V.prefix = cps ? 0 : 1;
    V.keys = (double*)w[BMW_SCORES].p; V.cnt = (uint32_t*)w[BMW_VC_CNT].p;
    V.sel_id = (const int64_t*)w[BMW_TOUT].p; V.sel_key = (const double*)w[BMW_TOUT].p + rmax * kk; V.k = kk;
    V.ids_out = (int64_t*)w[BMW_VC_OUT].p; V.cnt_out = V.ids_out + rmax * kk;
    V.dist_out = (int32_t*)(V.cnt_out + rmax); V.df_out = V.dist_out + rmax * kk;
    GzTopk K{};
    K.scores = V.keys; K.n_docs = T; K.k = kk; K.tile = tile;
    K.ckey[0] = (unsigned long long*)w[BMW_CKEY0].p; K.cidx[0] = (uint32_t*)w[BMW_CIDX0].p;
    K.ckey[1] = (unsigned long long*)w[BMW_CKEY1].p; K.cidx[1] = (uint32_t*)w[BMW_CIDX1].p;
    K.doc_out = (int64_t*)w[BMW_TOUT].p; K.score_out = (double*)w[BMW_TOUT].p + rmax * kk;
    for (int64_t q0 = 0; q0 < nq; q0 += rmax) {
        const int64_t rows = std::min(rmax, nq - q0);
        V.rows = K.rows = rows;
        if (cps) { V.cps = (const uint32_t*)w[BMW_VC_WORDS].p; V.cpoff = (const uint32_t*)w[BMW_VC_OFF].p + q0; }
        else { V.wbytes = (const uint8_t*)w[BMW_VC_WORDS].p - word_off[0]; V.woff = (const int64_t*)w[BMW_VC_OFF].p + q0; }
        HIPCHK(c, hipMemsetAsync(V.cnt, 0, (size_t)rows * 4, s));
        gz_launch_bm25_vocab(cps ? GZ_BM25_VC_EDIT : GZ_BM25_VC_PREFIX, V, s);
        gz_launch_topk(K, s);
        gz_launch_bm25_vocab(GZ_BM25_VC_UNPACK, V, s);
        HIPCHK(c, hipGetLastError());
        if ((rc = copy_out(c, ids_out + q0 * kk, V.ids_out, (size_t)(rows * kk) * 8, s)) ||
            (cps && (rc = copy_out(c, dist_out + q0 * kk, V.dist_out, (size_t)(rows * kk) * 4, s))) ||
            (rc = copy_out(c, df_out + q0 * kk, V.df_out, (size_t)(rows * kk) * 4, s)) ||
            (rc = copy_out(c, count_out + q0, V.cnt_out, (size_t)rows * 8, s)))
            return rc;
    }
    return GZ_OK;
}

// ---- search (gz_bm25_search, gz_bm25_match_count; gz_search.inc) -----------------------------------------------------------------
// The word offsets of a positional index as it is, unless it has them: woff = the scan of fieldLens, staged and entered after the
// round trip as the postings are.  Its total must be the index's word count: the bound of every read of seq.
int bm25_word_offsets(gz_bm25* ix)
{
    if (ix->has_woff) return GZ_OK;
    gz_ctx* c = ix->c;
    const int64_t N = ix->n_docs;
    int rc;
    BmStage st;
    BmDrain drain{c};
    void* p_woff;
    if ((rc = bm_stage(c, st, ix->woff, 0, (size_t)(N + 1) * 4, BmSize::Exact, &p_woff)) || (rc = bm_alloc(c, c->w_bm[BMW_BSUM], (size_t)(N / 4096 + 2) * 4)))
        return rc;
    if ((rc = bm_scan(c, (const uint32_t*)ix->dl.p, N, (uint32_t*)p_woff))) return rc;
    int64_t total = 0;
    if ((rc = bm_read_u32(c, (const uint32_t*)p_woff + N, total))) return rc;
    HIPCHK(c, hipGetLastError());
    if (total != ix->n_words)
        return fail(c, GZ_E_HIP, "BM25 positions: fieldLens sum to %lld words, the index holds %lld", (long long)total, (long long)ix->n_words);
    st.commit();
    ix->has_woff = true;
    return GZ_OK;
}

// The term-major postings of the index as it is, unless it has them: poff = the scan of df, pdoc filled from the entries.  Both
// are staged and enter the index after the last round trip: a return before that leaves the index without postings, as it was.
int bm25_postings(gz_bm25* ix)
{
    if (ix->has_post) return GZ_OK;
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    const int64_t T = ix->n_terms, E = ix->n_ent;
    int rc;
    BmStage st;
    BmDrain drain{c};
    void *p_poff, *p_pdoc;
    if ((rc = bm_stage(c, st, ix->poff, 0, (size_t)(T + 1) * 4, BmSize::Exact, &p_poff)) || (rc = bm_stage(c, st, ix->pdoc, 0, (size_t)E * 4, BmSize::Exact, &p_pdoc)) ||
        (rc = bm_alloc(c, w[BMW_P_CUR], (size_t)T * 4)) || (rc = bm_alloc(c, w[BMW_CTL], 64)) ||
        (rc = bm_alloc(c, w[BMW_BSUM], (size_t)(T / 4096 + 2) * 4)))
        return rc;
    GzBm25Post P{};
    P.n_docs = ix->n_docs; P.n_terms = T; P.n_ent = E;
    P.eoff = (const uint32_t*)ix->eoff.p; P.ent = (const uint2*)ix->ent.p;
    P.poff = (const uint32_t*)p_poff; P.pdoc = (uint32_t*)p_pdoc; P.cur = (uint32_t*)w[BMW_P_CUR].p; P.ctl = (uint32_t*)w[BMW_CTL].p;
    HIPCHK(c, hipMemsetAsync(P.ctl, 0, 64, s));
    if (T) HIPCHK(c, hipMemsetAsync(P.cur, 0, (size_t)T * 4, s));
    if ((rc = bm_scan(c, (const uint32_t*)ix->df.p, T, (uint32_t*)p_poff))) return rc;
    gz_launch_bm25_post(P, s);
    int64_t bad = 0, total = 0;
    if ((rc = bm_read_u32(c, P.ctl + 1, bad)) || (rc = bm_read_u32(c, P.poff + T, total))) return rc;
    HIPCHK(c, hipGetLastError());
    if (bad || total != E) return fail(c, GZ_E_HIP, "BM25 postings: the index's entries (%lld) and df (%lld) contradict each other", (long long)E, (long long)total);
    st.commit();
    ix->has_post = true;
    return GZ_OK;
}

int bm25_match_args(gz_bm25* ix, const int32_t* terms, const int64_t* qoff, int64_t nq, const void* out)
{
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!qoff || nq < 0 || (!out && nq > 0)) return fail(c, GZ_E_INVALID, "bad arguments");
    const int64_t nw = qoff[nq] - qoff[0];
    if (nw < 0 || (nw > 0 && !terms)) return fail(c, GZ_E_INVALID, "bad query offsets");
    for (int64_t q = 0; q < nq; ++q) if (qoff[q + 1] < qoff[q]) return fail(c, GZ_E_INVALID, "query offsets must not decrease");
    for (int64_t j = qoff[0]; j < qoff[nq]; ++j)
        if (terms[j] < -1 || terms[j] >= ix->n_terms) return fail(c, GZ_E_INVALID, "term id %d out of range", terms[j]);
    return GZ_OK;
}

// what the _bool entry points take on top: the mode, and the excluded terms of every query
int bm25_bool_args(gz_bm25* ix, int64_t nq, int32_t mode, const int32_t* xterm, const int64_t* xoff)
{
    gz_ctx* c = ix->c;
    if (mode != GZ_BM25_MATCH_ANY && mode != GZ_BM25_MATCH_ALL) return fail(c, GZ_E_INVALID, "match mode %d: GZ_BM25_MATCH_ANY or GZ_BM25_MATCH_ALL", mode);
    if (!xoff) return GZ_OK;
    for (int64_t q = 0; q < nq; ++q) if (xoff[q + 1] < xoff[q]) return fail(c, GZ_E_INVALID, "excluded-term offsets must not decrease");
    if (xoff[nq] > xoff[0] && !xterm) return fail(c, GZ_E_INVALID, "excluded-term offsets without terms");
    for (int64_t j = xoff[0]; j < xoff[nq]; ++j)
        if (xterm[j] < -1 || xterm[j] >= ix->n_terms) return fail(c, GZ_E_INVALID, "excluded term id %d out of range", xterm[j]);
    return GZ_OK;
}

// what the _phrase entry points take on top: the phrase terms of every query (phoff null: none)
int bm25_phrase_args(gz_bm25* ix, int64_t nq, const int32_t* phterm, const int64_t* phoff)
{
    gz_ctx* c = ix->c;
    if (!phoff) return GZ_OK;
    if (!(ix->flags & GZ_BM25_POSITIONS)) return fail(c, GZ_E_INVALID, "a phrase search needs an index built with GZ_BM25_POSITIONS");
    for (int64_t q = 0; q < nq; ++q) {
        if (phoff[q + 1] < phoff[q]) return fail(c, GZ_E_INVALID, "phrase-term offsets must not decrease");
        if (phoff[q + 1] - phoff[q] > GZ_BM25_PHRASE_MAX)
            return fail(c, GZ_E_LIMIT, "a phrase of %lld words; a phrase takes at most %d", (long long)(phoff[q + 1] - phoff[q]), GZ_BM25_PHRASE_MAX);
    }
    if (phoff[nq] > phoff[0] && !phterm) return fail(c, GZ_E_INVALID, "phrase-term offsets without terms");
    for (int64_t j = phoff[0]; j < phoff[nq]; ++j)
        if (phterm[j] < -1 || phterm[j] >= ix->n_terms) return fail(c, GZ_E_INVALID, "phrase term id %d out of range", phterm[j]);
    return GZ_OK;
}

// what the _near entry points take on top: the near terms and the window of every query (nroff null: none)
int bm25_near_args(gz_bm25* ix, int64_t nq, const int32_t* nrterm, const int64_t* nroff, const int64_t* nrwin)
{
    gz_ctx* c = ix->c;
    if (!nroff) return GZ_OK;
    if (!(ix->flags & GZ_BM25_POSITIONS)) return fail(c, GZ_E_INVALID, "a near search needs an index built with GZ_BM25_POSITIONS");
    if (!nrwin && nq > 0) return fail(c, GZ_E_INVALID, "near-term offsets without windows");
    for (int64_t q = 0; q < nq; ++q) {
        if (nroff[q + 1] < nroff[q]) return fail(c, GZ_E_INVALID, "near-term offsets must not decrease");
        if (nroff[q + 1] - nroff[q] > GZ_BM25_NEAR_MAX)
            return fail(c, GZ_E_LIMIT, "%lld near terms; a query takes at most %d", (long long)(nroff[q + 1] - nroff[q]), GZ_BM25_NEAR_MAX);
        if (nroff[q + 1] > nroff[q] && nrwin[q] < 1)
            return fail(c, GZ_E_INVALID, "window = %lld; a near search takes a window >= 1", (long long)nrwin[q]);
    }
    if (nroff[nq] > nroff[0] && !nrterm) return fail(c, GZ_E_INVALID, "near-term offsets without terms");
    for (int64_t j = nroff[0]; j < nroff[nq]; ++j)
        if (nrterm[j] < -1 || nrterm[j] >= ix->n_terms) return fail(c, GZ_E_INVALID, "near term id %d out of range", nrterm[j]);
    return GZ_OK;
}

static_assert(GZ_GROUP_MAX == GZ_BM25_GROUP_MAX, "the group kernels and the public header agree on a group's size");

// what the _groups entry points check before anything is allocated or launched: group g of query q (group_off[q] <= g <
// group_off[q + 1]) = the alternatives alt_terms[alt_off[g] .. alt_off[g + 1]), each in [-1, n_terms)
int bm25_group_args(gz_bm25* ix, const int32_t* aterm, const int64_t* aoff, const double* gidf, bool need_idf, const int64_t* goff, int64_t nq)
{
    gz_ctx* c = ix->c;
    if (!goff || nq < 0) return fail(c, GZ_E_INVALID, "bad arguments");
    if (goff[0] < 0) return fail(c, GZ_E_INVALID, "bad group offsets");
    for (int64_t q = 0; q < nq; ++q) if (goff[q + 1] < goff[q]) return fail(c, GZ_E_INVALID, "group offsets must not decrease");
    const int64_t g0 = goff[0], g1 = goff[nq];
    if (g1 == g0) return GZ_OK;
    if (!aoff || (need_idf && !gidf)) return fail(c, GZ_E_INVALID, "group offsets without alternatives or idf");
    if (aoff[g0] < 0) return fail(c, GZ_E_INVALID, "bad alternative offsets");
    for (int64_t g = g0; g < g1; ++g) if (aoff[g + 1] < aoff[g]) return fail(c, GZ_E_INVALID, "alternative offsets must not decrease");
    if (aoff[g1] > aoff[g0] && !aterm) return fail(c, GZ_E_INVALID, "alternative offsets without terms");
    for (int64_t j = aoff[g0]; j < aoff[g1]; ++j)
        if (aterm[j] < -1 || aterm[j] >= ix->n_terms) return fail(c, GZ_E_INVALID, "alternative term id %d out of range", aterm[j]);
    return GZ_OK;
}

// The groups of a call as the kernels take them (gz_groups.inc), all offsets from 0: the DISTINCT alternatives of every group that
// are terms at all (-1 dropped, a repeat counted once; ascending id, which no answer depends on), the groups of every row, and
// the row boundaries of the flat alternative list -- the "query offsets" of the word and marking kernels.
struct BmGroups {
    std::vector<int32_t> aterm;
    std::vector<int64_t> aoff, goff, rowoff;
    const double* gidf = nullptr;         // of the first group (null: a match count)
    int64_t ng = 0;
};

// (host memory only, before any launch) GZ_E_LIMIT: a group of more than GZ_BM25_GROUP_MAX distinct alternatives
int bm25_group_pack(gz_bm25* ix, const int32_t* aterm, const int64_t* aoff, const double* gidf, const int64_t* goff, int64_t nq, BmGroups& G)
{
    gz_ctx* c = ix->c;
    const int64_t g0 = goff[0];
    G.ng = goff[nq] - g0;
    alloc_site(c);
    G.goff.resize((size_t)nq + 1);
    G.rowoff.resize((size_t)nq + 1);
    G.aoff.resize((size_t)G.ng + 1);
    G.aoff[0] = 0;
    std::vector<int32_t> one;
    for (int64_t g = 0; g < G.ng; ++g) {
        one.clear();
        if (aoff[g0 + g + 1] > aoff[g0 + g]) one.assign(aterm + aoff[g0 + g], aterm + aoff[g0 + g + 1]);
        one.erase(std::remove(one.begin(), one.end(), -1), one.end());
        std::sort(one.begin(), one.end());
        one.erase(std::unique(one.begin(), one.end()), one.end());
        if ((int64_t)one.size() > GZ_BM25_GROUP_MAX)
            return fail(c, GZ_E_LIMIT, "a group of %lld distinct alternatives; a group takes at most %d", (long long)one.size(), GZ_BM25_GROUP_MAX);
        G.aterm.insert(G.aterm.end(), one.begin(), one.end());
        G.aoff[(size_t)g + 1] = (int64_t)G.aterm.size();
    }
    for (int64_t q = 0; q <= nq; ++q) {
        G.goff[(size_t)q] = goff[q] - g0;
        G.rowoff[(size_t)q] = G.aoff[(size_t)(goff[q] - g0)];
    }
    G.gidf = gidf && G.ng ? gidf + g0 : nullptr;
    return GZ_OK;
}

// An optional term list of a search (excluded, phrase or near terms): query q has term[off[q] .. off[q + 1]); off null: none
struct BmTermList { const int32_t* term = nullptr; const int64_t* off = nullptr; };

// One search call as its entry point received it: gz_bm25_search* and gz_bm25_match_count* fill one and call bm25_search_entry
struct BmSearchReq {
    const int32_t* terms = nullptr; const double* idf = nullptr; const int64_t* qoff = nullptr; int64_t nq = 0;       // the scored words
    const double* P = nullptr; int32_t plus = 0; int64_t k = 0;
    bool count_only = false;              // a match count: nothing behind the counts (idf, P, k, doc and score are not read)
    int32_t mode = GZ_BM25_MATCH_ANY;
    BmTermList ex, ph, nr;                // excluded, phrase and near terms
    const int64_t* nrwin = nullptr;       // the window of every query
    bool grouped = false;                 // a search over word groups: these four stand for terms / idf / qoff until they are packed
    const int32_t* alt_terms = nullptr; const int64_t* alt_off = nullptr; const double* group_idf = nullptr; const int64_t* group_off = nullptr;
    int64_t* doc = nullptr; double* score = nullptr; int64_t* cnt = nullptr; BmMem mem = BmMem::Host;                 // the outputs, all in mem
};

// A term list that has terms -> two slots of the workspace: term + off[0] (n x 4 bytes) and off ((nq + 1) x 8 bytes).  D.term is
// biased by -off[0], so that the list's own offsets index it.
int bm_side_list(gz_ctx* c, int term_slot, int off_slot, const BmTermList& L, int64_t nq, BmTermList& D)
{
    DBuf* w = c->w_bm;
    const int64_t n = L.off[nq] - L.off[0];
    int rc;
    if ((rc = bm_alloc(c, w[term_slot], (size_t)n * 4)) || (rc = bm_alloc(c, w[off_slot], (size_t)(nq + 1) * 8)) ||
        (rc = copy_in(c, w[term_slot].p, L.term + L.off[0], (size_t)n * 4, c->stream)) ||
        (rc = copy_in(c, w[off_slot].p, L.off, (size_t)(nq + 1) * 8, c->stream)))
        return rc;
    D.term = (const int32_t*)w[term_slot].p - L.off[0];
    D.off = (const int64_t*)w[off_slot].p;
    return GZ_OK;
}

// The kernels that walk the word sequence raise ctl[1] when the index's fieldLens and its sequence disagree: the read waits for
// them, `text` is the caller's refusal.  launch_check: the caller has not asked hipGetLastError since their launch.
int bm_seq_flag(gz_ctx* c, const uint32_t* ctl, bool launch_check, const char* text)
{
    int64_t bad = 0;
    int rc = bm_read_u32(c, ctl + 1, bad);
    if (rc) return rc;
    if (launch_check) HIPCHK(c, hipGetLastError());
    return bad ? fail(c, GZ_E_HIP, "%s", text) : GZ_OK;
}

// A validated search on the stream.  A chunk of queries at a time (its bitmaps hold at most bm25_search_chunk words, one row at
// least, at most 65535 rows): match() marks the documents of every query word's postings in the row's bitmap, counts and ranks
// the bits, and reads the counts back -- they size what follows.  Then, for runs of rows whose candidate scores (rows x the
// largest count among them) stay within bm25_search_chunk doubles, one row at least: rank().  Outputs into R.doc / R.score / R.cnt
// in device memory, or into host memory after every run.
// grp (null: none): the packed groups of a search over word groups (gz_groups.inc).  R.terms / R.qoff are then the alternatives and
// their row boundaries (grp->aterm, grp->rowoff; idf is not read): words and marking run unchanged over them, the group driver
// stands in for GZ_BM25_SR_DRIVER, the group filter for GZ_BM25_SR_FILTER and the group score for GZ_BM25_SR_SCORE.
// A list without terms, a call without groups: nothing of its stage is launched, allocated or derived.
struct BmSearch {
    gz_bm25* ix; const BmSearchReq& R; int64_t kk; const BmGroups* grp;
    gz_ctx* c = ix->c; DBuf* w = c->w_bm; hipStream_t s = c->stream;
    bool dev = R.mem == BmMem::Device;
    GzBm25Search A{}; GzBm25Near NR{}; GzBm25Group G{};
    BmTermList ex, ph, nr;                // the lists that have terms, in the workspace
    int64_t chunk = 0, W64 = 0, rmax = 0; // rmax: the rows of a chunk
    const int64_t* qoff_dev = nullptr;
    std::vector<uint32_t> cnt;            // the chunk's counts
    int setup();
    int match(int64_t q0, int64_t rows);
    int rank(int64_t q0, int64_t r0, int64_t n, int64_t M);
};

// the query arrays, the term lists and the groups into the workspace; the postings, and for phrase and near terms the word
// offsets, derived if they are not there; the chunk's buffers
int BmSearch::setup()
{
    const int64_t N = ix->n_docs, nq = R.nq;
    int rc;
    if ((rc = bm25_postings(ix)) || (rc = bm25_query_in(ix, R.terms, R.idf, R.qoff, nq, R.P, R.plus, A.S))) return rc;
    if (R.ex.off && R.ex.off[nq] > R.ex.off[0] && (rc = bm_side_list(c, BMW_S_XTERM, BMW_S_XOFF, R.ex, nq, ex))) return rc;
    A.xterm = ex.term;
    A.mode = R.mode;
    if (R.ph.off && R.ph.off[nq] > R.ph.off[0]) {
        if ((rc = bm25_word_offsets(ix)) || (rc = bm_side_list(c, BMW_S_PHTERM, BMW_S_PHOFF, R.ph, nq, ph)) || (rc = bm_alloc(c, w[BMW_CTL], 64)))
            return rc;
        A.phterm = ph.term;
        A.seq = (const uint32_t*)ix->seq.p; A.woff = (const uint32_t*)ix->woff.p; A.n_words = ix->n_words;
        A.ctl = (uint32_t*)w[BMW_CTL].p;
        HIPCHK(c, hipMemsetAsync(A.ctl, 0, 64, s));
    }
    if (R.nr.off && R.nr.off[nq] > R.nr.off[0]) {
        if ((rc = bm25_word_offsets(ix)) || (rc = bm_side_list(c, BMW_S_NRTERM, BMW_S_NROFF, R.nr, nq, nr)) ||
            (rc = bm_alloc(c, w[BMW_S_NRWIN], (size_t)nq * 8)) || (rc = bm_alloc(c, w[BMW_CTL], 64)) ||
            (rc = copy_in(c, w[BMW_S_NRWIN].p, R.nrwin, (size_t)nq * 8, s)))
            return rc;
        NR.S = A.S;
        NR.seq = (const uint32_t*)ix->seq.p; NR.woff = (const uint32_t*)ix->woff.p; NR.n_words = ix->n_words;
        NR.n_docs = N; NR.n_terms = ix->n_terms;
        NR.sterm = nr.term;
        NR.ctl = (uint32_t*)w[BMW_CTL].p;
        if (!ph.off) HIPCHK(c, hipMemsetAsync(NR.ctl, 0, 64, s));
    }
    if (grp) {
        const int64_t ng = grp->ng;
        if ((rc = bm_alloc(c, w[BMW_G_GOFF], (size_t)(nq + 1) * 8)) || (rc = bm_alloc(c, w[BMW_G_AOFF], (size_t)(ng + 1) * 8)) ||
            (rc = bm_alloc(c, w[BMW_G_IDF], (size_t)ng * 8)) || (rc = bm_alloc(c, w[BMW_G_MASK], (size_t)ng * 32)) ||
            (rc = copy_in(c, w[BMW_G_GOFF].p, grp->goff.data(), (size_t)(nq + 1) * 8, s)) ||
            (rc = copy_in(c, w[BMW_G_AOFF].p, grp->aoff.data(), (size_t)(ng + 1) * 8, s)) ||
            (grp->gidf && (rc = copy_in(c, w[BMW_G_IDF].p, grp->gidf, (size_t)ng * 8, s))))
            return rc;
        G.aoff = (const int64_t*)w[BMW_G_AOFF].p; G.gidf = (const double*)w[BMW_G_IDF].p;
        G.gmask = (unsigned long long*)w[BMW_G_MASK].p; G.n_groups = ng;
        G.A.qterm = A.S.qterm;
        gz_launch_bm25_groups(GZ_BM25_GR_MASK, G, 0, s);
    }
    chunk = c->opt.bm25_search_chunk;
    W64 = (N + 63) / 64;
    const int64_t n_tiles = (W64 + GZ_SEARCH_TILE - 1) / GZ_SEARCH_TILE;
    rmax = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(chunk / W64, 1), 65535), nq);
    int64_t wmax = 0;                                          // the most query words of a chunk
    for (int64_t q0 = 0; q0 < nq; q0 += rmax) wmax = std::max(wmax, R.qoff[std::min(q0 + rmax, nq)] - R.qoff[q0]);
    if ((rc = bm_alloc(c, w[BMW_S_BM], (size_t)(rmax * W64) * 8)) || (rc = bm_alloc(c, w[BMW_S_WROW], (size_t)wmax * 4)) ||
        (rc = bm_alloc(c, w[BMW_S_WNS], (size_t)(wmax + 1) * 4)) || (rc = bm_alloc(c, w[BMW_S_WSOFF], (size_t)(wmax + 1) * 4)) ||
        (rc = bm_alloc(c, w[BMW_BSUM], (size_t)(wmax / 4096 + 2) * 4)) || (rc = bm_alloc(c, w[BMW_S_TCNT], (size_t)(rmax * n_tiles) * 4)) ||
        (rc = bm_alloc(c, w[BMW_S_TBASE], (size_t)(rmax * n_tiles) * 4)) || (rc = bm_alloc(c, w[BMW_S_CNT], (size_t)rmax * 4)))
        return rc;
    alloc_site(c);
    cnt.resize((size_t)rmax);
    A.poff = (const uint32_t*)ix->poff.p; A.pdoc = (const uint32_t*)ix->pdoc.p;
    A.n_docs = N; A.n_terms = ix->n_terms; A.n_ent = ix->n_ent;
    A.qterm = A.S.qterm; A.qidf = A.S.qidf;
    A.w64 = W64; A.n_tiles = n_tiles; A.bm = (unsigned long long*)w[BMW_S_BM].p;
    A.wrow = (uint32_t*)w[BMW_S_WROW].p; A.wns = (uint32_t*)w[BMW_S_WNS].p; A.wsoff = (uint32_t*)w[BMW_S_WSOFF].p;
    A.tcnt = (uint32_t*)w[BMW_S_TCNT].p; A.tbase = (uint32_t*)w[BMW_S_TBASE].p; A.cnt = (uint32_t*)w[BMW_S_CNT].p;
    qoff_dev = A.S.qoff;
    return GZ_OK;
}

// The match stage of the chunk of `rows` queries from q0: words -> (driver) -> scan -> mark -> (filter) -> (phrase) -> (near) ->
// count -> rows, and the counts back.  mode GZ_BM25_MATCH_ALL: only the driver of every row is marked and the filter clears the
// documents that lack a word of the row; with excluded terms the filter clears the documents that hold one.  The phrase stage
// clears, in the rows that have phrase terms, the documents in which they do not stand next to each other; the near stage
// (gz_near.inc), in the rows that have near terms, those that do not hold all of them inside nrwin[row] consecutive words.
int BmSearch::match(int64_t q0, int64_t rows)
{
    int rc;
    A.qoff = qoff_dev + q0; A.rows = rows; A.n_qw = R.qoff[q0 + rows] - R.qoff[q0];
    A.cnt_out = dev ? R.cnt + q0 : nullptr;
    HIPCHK(c, hipMemsetAsync(A.bm, 0, (size_t)(rows * W64) * 8, s));
    if (A.n_qw > 0) {
        gz_launch_bm25_search(GZ_BM25_SR_WORDS, A, rows, s);
        A.xoff = ex.off && R.ex.off[q0 + rows] > R.ex.off[q0] ? ex.off + q0 : nullptr;
        if (grp) { G.A = A; G.goff = (const int64_t*)w[BMW_G_GOFF].p + q0; }        // (the chunk's rows; the group indices stay absolute)
        if (R.mode == GZ_BM25_MATCH_ALL) {
            if (grp) gz_launch_bm25_groups(GZ_BM25_GR_DRIVER, G, rows, s);
            else gz_launch_bm25_search(GZ_BM25_SR_DRIVER, A, rows, s);
        }
        if ((rc = bm_scan(c, A.wns, A.n_qw, A.wsoff))) return rc;
        gz_launch_bm25_search(GZ_BM25_SR_MARK, A, rows, s);
        if (R.mode == GZ_BM25_MATCH_ALL || A.xoff) {
            if (grp) gz_launch_bm25_groups(GZ_BM25_GR_FILTER, G, rows, s);
            else gz_launch_bm25_search(GZ_BM25_SR_FILTER, A, rows, s);
        }
        A.phoff = ph.off && R.ph.off[q0 + rows] > R.ph.off[q0] ? ph.off + q0 : nullptr;
        if (A.phoff) gz_launch_bm25_search(GZ_BM25_SR_PHRASE, A, rows, s);
        if (nr.off && R.nr.off[q0 + rows] > R.nr.off[q0]) {       // (the chunk's rows; the offsets and windows stay the absolute ones)
            NR.soff = nr.off + q0; NR.win = (const int64_t*)w[BMW_S_NRWIN].p + q0;
            NR.bm = A.bm; NR.w64 = W64;
            gz_launch_bm25_near(GZ_BM25_SR_NEAR, NR, rows, s);
        }
    }
    gz_launch_bm25_search(GZ_BM25_SR_COUNT, A, rows, s);
    gz_launch_bm25_search(GZ_BM25_SR_ROWS, A, rows, s);
    HIPCHK(c, hipGetLastError());
    if ((rc = copy_out_small(c, cnt.data(), A.cnt, (size_t)rows * 4, s))) return rc;
    if (ph.off) rc = bm_seq_flag(c, A.ctl, false, "BM25 phrase search: the index's fieldLens and word sequence contradict each other");
    else if (nr.off) rc = bm_seq_flag(c, NR.ctl, false, "BM25 near search: the index's fieldLens and word sequence contradict each other");
    if (rc) return rc;
    if (!dev && R.cnt) for (int64_t r = 0; r < rows; ++r) R.cnt[q0 + r] = (int64_t)cnt[(size_t)r];
    return GZ_OK;
}

// The rank stage of the run of n rows from r0 of the chunk from q0, M = the largest count among them: the candidates in ascending
// id -> their scores (or the group score) -> gz_launch_topk over them -> the positions mapped back to document ids, out
int BmSearch::rank(int64_t q0, int64_t r0, int64_t n, int64_t M)
{
    const int64_t k2 = std::min(kk, M);
    int rc;
    A.row0 = r0; A.M = M; A.k2 = k2; A.kk = kk;
    if (!dev && (rc = bm_alloc(c, w[BMW_TOUT], (size_t)(n * kk) * 16))) return rc;
    if (M > 0) {
        const int64_t tile = bm25_topk_tile(c, n, M, k2);
        int64_t m1, m2;
        gz_topk_sizes(M, tile, k2, m1, m2);
        if ((rc = bm_alloc(c, w[BMW_S_CAND], (size_t)(n * M) * 4)) || (rc = bm_alloc(c, w[BMW_S_CSC], (size_t)(n * M) * 8)) ||
            (rc = bm_alloc(c, w[BMW_CKEY0], (size_t)(n * m1) * 8)) || (rc = bm_alloc(c, w[BMW_CIDX0], (size_t)(n * m1) * 4)) ||
            (rc = bm_alloc(c, w[BMW_CKEY1], (size_t)(n * m2) * 8)) || (rc = bm_alloc(c, w[BMW_CIDX1], (size_t)(n * m2) * 4)) ||
            (rc = bm_alloc(c, w[BMW_S_POS], (size_t)(n * k2) * 8)) || (rc = bm_alloc(c, w[BMW_S_PSC], (size_t)(n * k2) * 8)))
            return rc;
        A.cand = (uint32_t*)w[BMW_S_CAND].p; A.csc = (double*)w[BMW_S_CSC].p;
        A.pos = (const int64_t*)w[BMW_S_POS].p; A.psc = (const double*)w[BMW_S_PSC].p;
        gz_launch_bm25_search(GZ_BM25_SR_CAND, A, n, s);
        if (grp) {
            G.A = A; G.goff = (const int64_t*)w[BMW_G_GOFF].p + q0;
            gz_launch_bm25_groups(GZ_BM25_GR_SCORE, G, n, s);
        } else {
            gz_launch_bm25_search(GZ_BM25_SR_SCORE, A, n, s);
        }
        GzTopk T{};
        T.scores = A.csc; T.n_docs = M; T.rows = n; T.k = k2; T.tile = tile;
        T.ckey[0] = (unsigned long long*)w[BMW_CKEY0].p; T.cidx[0] = (uint32_t*)w[BMW_CIDX0].p;
        T.ckey[1] = (unsigned long long*)w[BMW_CKEY1].p; T.cidx[1] = (uint32_t*)w[BMW_CIDX1].p;
        T.doc_out = (int64_t*)w[BMW_S_POS].p; T.score_out = (double*)w[BMW_S_PSC].p;
        gz_launch_topk(T, s);
    }
    A.doc_out = dev ? R.doc + (q0 + r0) * kk : (int64_t*)w[BMW_TOUT].p;
    A.score_out = dev ? R.score + (q0 + r0) * kk : (double*)w[BMW_TOUT].p + n * kk;
    gz_launch_bm25_search(GZ_BM25_SR_OUT, A, n, s);
    HIPCHK(c, hipGetLastError());
    if (!dev && ((rc = copy_out(c, R.doc + (q0 + r0) * kk, A.doc_out, (size_t)(n * kk) * 8, s)) ||
                 (rc = copy_out(c, R.score + (q0 + r0) * kk, A.score_out, (size_t)(n * kk) * 8, s))))
        return rc;
    return GZ_OK;
}

int bm25_search_locked(gz_bm25* ix, const BmSearchReq& R, int64_t kk, const BmGroups* grp)
{
    BmSearch S{ix, R, kk, grp};
    gz_ctx* c = ix->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (R.nq == 0) return GZ_OK;
    if (ix->n_docs == 0) {
        if (R.cnt && S.dev) HIPCHK(c, hipMemsetAsync(R.cnt, 0, (size_t)R.nq * 8, c->stream));
        if (R.cnt && !S.dev) std::memset(R.cnt, 0, (size_t)R.nq * 8);
        return GZ_OK;
    }
    int rc = S.setup();
    if (rc) return rc;
    for (int64_t q0 = 0; q0 < R.nq; q0 += S.rmax) {
        const int64_t rows = std::min(S.rmax, R.nq - q0);
        if ((rc = S.match(q0, rows))) return rc;
        if (R.count_only) continue;
        for (int64_t r0 = 0; r0 < rows;) {
            int64_t M = S.cnt[(size_t)r0], n = 1;
            for (; r0 + n < rows; ++n) {
                const int64_t M2 = std::max<int64_t>(M, S.cnt[(size_t)(r0 + n)]);
                if ((n + 1) * M2 > S.chunk) break;
                M = M2;
            }
            if ((rc = S.rank(q0, r0, n, M))) return rc;
            r0 += n;
        }
    }
    return GZ_OK;
}

// What the fifteen search entry points do: the checks, before anything is allocated or launched and in the order that decides
// which refusal a call with several faults gets (the group forms, the counts and the scored forms each have their own), the lock,
// the packing of the groups, the run
int bm25_search_entry(gz_bm25* ix, BmSearchReq& R)
{
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    const int64_t nq = R.nq;
    int64_t kk = 0;
    int rc;
    if (R.grouped) {
        if ((!R.count_only && (!R.P || ((!R.doc || !R.score) && nq > 0 && ix->n_docs > 0))) || nq < 0 || (!R.cnt && nq > 0))
            return fail(c, GZ_E_INVALID, "bad arguments");
        if ((rc = bm25_group_args(ix, R.alt_terms, R.alt_off, R.group_idf, !R.count_only, R.group_off, nq)) ||
            (!R.count_only && (rc = bm25_topk_k(ix, R.k, kk))) || (rc = bm25_bool_args(ix, nq, R.mode, R.ex.term, R.ex.off)))
            return rc;
    } else if (R.count_only) {
        if ((rc = bm25_match_args(ix, R.terms, R.qoff, nq, R.cnt)) || (rc = bm25_bool_args(ix, nq, R.mode, R.ex.term, R.ex.off)) ||
            (rc = bm25_phrase_args(ix, nq, R.ph.term, R.ph.off)) || (rc = bm25_near_args(ix, nq, R.nr.term, R.nr.off, R.nrwin)))
            return rc;
    } else {
        if ((rc = bm25_score_args(ix, R.terms, R.idf, R.qoff, nq, R.P, R.doc && R.score ? R.doc : nullptr)) || (rc = bm25_topk_k(ix, R.k, kk)) ||
            (rc = bm25_bool_args(ix, nq, R.mode, R.ex.term, R.ex.off)) || (rc = bm25_phrase_args(ix, nq, R.ph.term, R.ph.off)) ||
            (rc = bm25_near_args(ix, nq, R.nr.term, R.nr.off, R.nrwin)))
            return rc;
        if (!R.cnt && nq > 0) return fail(c, GZ_E_INVALID, "bad arguments");
    }
    std::lock_guard<std::mutex> lk(c->mu);
    BmGroups G;
    if (R.grouped) {
        if ((rc = bm25_group_pack(ix, R.alt_terms, R.alt_off, R.group_idf, R.group_off, nq, G))) return rc;
        R.terms = G.aterm.data(); R.idf = nullptr; R.qoff = G.rowoff.data();
    }
    return bm25_search_locked(ix, R, kk, R.grouped ? &G : nullptr);
}

// ---- snippets (gz_bm25_snippets, gz_bm25_occurrences; gz_snippet.inc) ------------------------------------------------------------
// what the snippet entry points check before anything is launched: a positional index, the packed query terms, k
int bm25_snip_args(gz_bm25* ix, const int32_t* terms, const int64_t* qoff, int64_t nq, int64_t k)
{
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!(ix->flags & GZ_BM25_POSITIONS)) return fail(c, GZ_E_INVALID, "snippets need an index built with GZ_BM25_POSITIONS");
    int rc = bm25_match_args(ix, terms, qoff, nq, ix);         // (the outputs are checked by the caller)
    if (rc) return rc;
    if (k < 0) return fail(c, GZ_E_INVALID, "k = %lld; snippets take k >= 0", (long long)k);
    if (k > 0 && nq > (((int64_t)1 << 31) - 1) / k) return fail(c, GZ_E_LIMIT, "%lld queries x %lld documents; a call takes fewer than 2^31 pairs", (long long)nq, (long long)k);
    return GZ_OK;
}

// the ids of a host form lie in [-1, n_docs) (ids in HBM are not looked at here: the kernels treat a bad one as -1)
int bm25_snip_ids(gz_bm25* ix, const int64_t* ids, int64_t n)
{
    for (int64_t r = 0; r < n; ++r)
        if (ids[r] < -1 || ids[r] >= ix->n_docs)
            return fail(ix->c, GZ_E_INVALID, "document id %lld outside [-1, %lld)", (long long)ids[r], (long long)ix->n_docs);
    return GZ_OK;
}

// the query arrays into the context's workspace, the word offsets derived if they are not there (nothing else is: no postings),
// and the kernels' arguments but for ids and outputs
int bm25_snip_in(gz_bm25* ix, const int32_t* terms, const int64_t* qoff, int64_t nq, int64_t k, GzBm25Snip& A)
{
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    int rc;
    if ((rc = bm25_word_offsets(ix))) return rc;
    GzBm25Score S;
    if ((rc = bm25_query_in(ix, terms, nullptr, qoff, nq, nullptr, 0, S)) || (rc = bm_alloc(c, w[BMW_CTL], 64))) return rc;
    A = GzBm25Snip{};
    A.seq = (const uint32_t*)ix->seq.p; A.woff = (const uint32_t*)ix->woff.p; A.n_words = ix->n_words; A.n_docs = ix->n_docs;
    A.qterm = S.qterm; A.qoff = S.qoff;
    A.n_pairs = nq * k; A.k = k; A.width = 1;
    A.ctl = (uint32_t*)w[BMW_CTL].p;
    HIPCHK(c, hipMemsetAsync(A.ctl, 0, 64, c->stream));
    return GZ_OK;
}

int bm25_snip_flag(gz_ctx* c, const GzBm25Snip& A)
{
    return bm_seq_flag(c, A.ctl, true, "BM25 snippets: the index's fieldLens and word sequence contradict each other");
}

// ids / start / hits in HBM, or (host memory) ids in and start / hits out through the workspace
int bm25_snippets_locked(gz_bm25* ix, const int32_t* terms, const int64_t* qoff, int64_t nq, int64_t k, int64_t width, const int64_t* ids,
                         int32_t* start, int32_t* hits, BmMem mem)
{
    const bool dev = mem == BmMem::Device;
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = nq * k;
    if (n == 0) return GZ_OK;
    GzBm25Snip A;
    int rc = bm25_snip_in(ix, terms, qoff, nq, k, A);
    if (rc) return rc;
    A.width = width;
    if (dev) {
        A.ids = ids; A.start_out = start; A.hits_out = hits;
    } else {
        if ((rc = bm_alloc(c, w[BMW_SN_IDS], (size_t)n * 8)) || (rc = bm_alloc(c, w[BMW_SN_OUT], (size_t)n * 8)) ||
            (rc = copy_in(c, w[BMW_SN_IDS].p, ids, (size_t)n * 8, s)))
            return rc;
        A.ids = (const int64_t*)w[BMW_SN_IDS].p; A.start_out = (int32_t*)w[BMW_SN_OUT].p; A.hits_out = A.start_out + n;
    }
    gz_launch_bm25_snippet(GZ_BM25_SN_WINDOW, A, s);
    if ((rc = bm25_snip_flag(c, A))) return rc;
    if (dev) return GZ_OK;
    if ((rc = copy_out(c, start, A.start_out, (size_t)n * 4, s)) || (rc = copy_out(c, hits, A.hits_out, (size_t)n * 4, s))) return rc;
    return GZ_OK;
}

// ---- proximity: the cover of pairs (gz_bm25_cover[_device]; gz_near.inc) -----------------------------------------------------------
// what the cover entry points check on top of bm25_snip_args: a query is a set of at most GZ_BM25_NEAR_MAX entries
int bm25_cover_args(gz_bm25* ix, const int64_t* qoff, int64_t nq)
{
    for (int64_t q = 0; q < nq; ++q)
        if (qoff[q + 1] - qoff[q] > GZ_BM25_NEAR_MAX)
            return fail(ix->c, GZ_E_LIMIT, "a cover over %lld terms; a query takes at most %d", (long long)(qoff[q + 1] - qoff[q]), GZ_BM25_NEAR_MAX);
    return GZ_OK;
}

// ids and the three outputs in HBM, or (host memory) ids in and the outputs out through the workspace
int bm25_cover_locked(gz_bm25* ix, const int32_t* terms, const int64_t* qoff, int64_t nq, int64_t k, const int64_t* ids, int32_t* start,
                      int32_t* len, int32_t* words, BmMem mem)
{
    const bool dev = mem == BmMem::Device;
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = nq * k;
    if (n == 0) return GZ_OK;
    int rc;
    if ((rc = bm25_word_offsets(ix))) return rc;
    GzBm25Near A{};
    if ((rc = bm25_query_in(ix, terms, nullptr, qoff, nq, nullptr, 0, A.S)) || (rc = bm_alloc(c, w[BMW_CTL], 64))) return rc;
    A.seq = (const uint32_t*)ix->seq.p; A.woff = (const uint32_t*)ix->woff.p; A.n_words = ix->n_words;
    A.n_docs = ix->n_docs; A.n_terms = ix->n_terms;
    A.sterm = A.S.qterm; A.soff = A.S.qoff;
    A.n_pairs = n; A.k = k;
    A.ctl = (uint32_t*)w[BMW_CTL].p;
    HIPCHK(c, hipMemsetAsync(A.ctl, 0, 64, s));
    if (dev) {
        A.ids = ids; A.start_out = start; A.len_out = len; A.words_out = words;
    } else {
        if ((rc = bm_alloc(c, w[BMW_SN_IDS], (size_t)n * 8)) || (rc = bm_alloc(c, w[BMW_SN_OUT], (size_t)n * 12)) ||
            (rc = copy_in(c, w[BMW_SN_IDS].p, ids, (size_t)n * 8, s)))
            return rc;
        A.ids = (const int64_t*)w[BMW_SN_IDS].p; A.start_out = (int32_t*)w[BMW_SN_OUT].p; A.len_out = A.start_out + n; A.words_out = A.len_out + n;
    }
    gz_launch_bm25_near(GZ_BM25_NR_COVER, A, 0, s);
    if ((rc = bm_seq_flag(c, A.ctl, true, "BM25 cover: the index's fieldLens, pair table and word sequence contradict each other"))) return rc;
    if (dev) return GZ_OK;
    if ((rc = copy_out(c, start, A.start_out, (size_t)n * 4, s)) || (rc = copy_out(c, len, A.len_out, (size_t)n * 4, s)) ||
        (rc = copy_out(c, words, A.words_out, (size_t)n * 4, s)))
        return rc;
    return GZ_OK;
}

int bm25_occurrences_locked(gz_bm25* ix, const int32_t* terms, const int64_t* qoff, int64_t nq, const int64_t* ids, int64_t k, int64_t* pair_off,
                            int32_t* pos_out, int32_t* word_out, int64_t cap)
{
    gz_ctx* c = ix->c;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = nq * k;
    if (n == 0) { pair_off[0] = 0; return GZ_OK; }
    GzBm25Snip A;
    int rc = bm25_snip_in(ix, terms, qoff, nq, k, A);
    if (rc) return rc;
    if ((rc = bm_alloc(c, w[BMW_SN_IDS], (size_t)n * 8)) || (rc = bm_alloc(c, w[BMW_SN_CNT], (size_t)n * 4)) ||
        (rc = bm_alloc(c, w[BMW_SN_OFF], (size_t)(n + 1) * 4)) || (rc = bm_alloc(c, w[BMW_BSUM], (size_t)(n / 4096 + 2) * 4)) ||
        (rc = copy_in(c, w[BMW_SN_IDS].p, ids, (size_t)n * 8, s)))
        return rc;
    A.ids = (const int64_t*)w[BMW_SN_IDS].p; A.cnt = (uint32_t*)w[BMW_SN_CNT].p; A.base = (const uint32_t*)w[BMW_SN_OFF].p;
    gz_launch_bm25_snippet(GZ_BM25_SN_COUNT, A, s);
    if ((rc = bm_scan(c, A.cnt, n, (uint32_t*)w[BMW_SN_OFF].p))) return rc;
    unsigned long long all = 0;                               // the 64-bit sum: the scan's total is only its low half
    if ((rc = copy_out_small(c, &all, A.ctl + 4, 8, s)) || (rc = bm25_snip_flag(c, A))) return rc;
    if (all >= (1ull << 32)) return fail(c, GZ_E_LIMIT, "%llu occurrences; a call takes fewer than 2^32", all);
    const int64_t T = (int64_t)all;
    if (pos_out && cap < T) return fail(c, GZ_E_CAPACITY, "BM25 occurrences: %lld of them, room for %lld", (long long)T, (long long)cap);
    alloc_site(c);
    std::vector<uint32_t> off((size_t)n + 1);
    if ((rc = copy_out(c, off.data(), A.base, (size_t)(n + 1) * 4, s))) return rc;
    if ((int64_t)off[(size_t)n] != T) return fail(c, GZ_E_HIP, "BM25 occurrences: the counts sum to %lld, their scan ends at %lld", (long long)T, (long long)off[(size_t)n]);
    if (pos_out && T > 0) {
        if ((rc = bm_alloc(c, w[BMW_SN_POS], (size_t)T * 4)) || (rc = bm_alloc(c, w[BMW_SN_WORD], (size_t)T * 4))) return rc;
        A.pos_out = (int32_t*)w[BMW_SN_POS].p; A.word_out = (int32_t*)w[BMW_SN_WORD].p;
        gz_launch_bm25_snippet(GZ_BM25_SN_FILL, A, s);
        HIPCHK(c, hipGetLastError());
        if ((rc = copy_out(c, pos_out, A.pos_out, (size_t)T * 4, s)) || (rc = copy_out(c, word_out, A.word_out, (size_t)T * 4, s))) return rc;
    }
    for (int64_t r = 0; r <= n; ++r) pair_off[r] = (int64_t)off[(size_t)r];
    return GZ_OK;
}
}  // namespace


extern "C" {

// ---- BM25 / BM25Plus ------------------------------------------------------------------------------------------------------
int gz_bm25_build(gz_ctx* c, const uint8_t* text, const int64_t* text_off, int64_t n_docs, gz_bm25** out)
{
    return gz_bm25_build_ex(c, text, text_off, n_docs, 0, out);
}

int gz_bm25_build_device(gz_ctx* c, const uint8_t* text_dev, const int64_t* text_off_dev, int64_t n_docs, int64_t text_bytes, gz_bm25** out)
{
    return gz_bm25_build_device_ex(c, text_dev, text_off_dev, n_docs, text_bytes, 0, out);
}

int gz_bm25_build_ex(gz_ctx* c, const uint8_t* text, const int64_t* text_off, int64_t n_docs, int32_t flags, gz_bm25** out)
try {
    if (!c || !out || !text_off || n_docs < 0) return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    *out = nullptr;
    if (flags & ~GZ_BM25_POSITIONS) return fail(c, GZ_E_INVALID, "BM25 build flags 0x%x: only GZ_BM25_POSITIONS is defined", (unsigned)flags);
    int rc;
    if ((rc = bm_host_offsets(c, text, text_off, n_docs))) return rc;
    const int64_t nbytes = text_off[n_docs] - text_off[0];
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = bm_limits(c, nbytes, n_docs))) return rc;
    alloc_site(c);
    std::unique_ptr<gz_bm25> ix(new gz_bm25());
    BmDrain drain{c};
    ix->c = c; ix->n_docs = n_docs; ix->off0 = text_off[0]; ix->flags = flags;
    if ((rc = bm_upload(c, ix->text, text, text_off, n_docs, nbytes))) return rc;
    if ((rc = bm25_build_core(c, ix.get(), (const int64_t*)c->w_bm[BMW_OFF].p, nbytes)) || (rc = bm25_build_finish(c, ix.get()))) return rc;
    return bm_adopt(c, ix, out);
} GZ_CATCH(c)

int gz_bm25_build_device_ex(gz_ctx* c, const uint8_t* text_dev, const int64_t* text_off_dev, int64_t n_docs, int64_t text_bytes, int32_t flags,
                            gz_bm25** out)
try {
    if (!c || !out || !text_off_dev || n_docs < 0 || text_bytes < 0 || (text_bytes > 0 && !text_dev))
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    *out = nullptr;
    if (flags & ~GZ_BM25_POSITIONS) return fail(c, GZ_E_INVALID, "BM25 build flags 0x%x: only GZ_BM25_POSITIONS is defined", (unsigned)flags);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = bm_limits(c, text_bytes, n_docs))) return rc;
    alloc_site(c);
    std::unique_ptr<gz_bm25> ix(new gz_bm25());
    BmDrain drain{c};
    int64_t off0 = 0;
    if ((rc = bm_read_off0(c, text_off_dev, off0))) return rc;
    ix->c = c; ix->n_docs = n_docs; ix->off0 = off0; ix->flags = flags;
    if ((rc = bm_alloc(c, ix->text, (size_t)text_bytes + 16))) return rc;
    if (text_bytes) HIPCHK(c, hipMemcpyAsync(ix->text.p, text_dev + off0, (size_t)text_bytes, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = bm25_build_core(c, ix.get(), text_off_dev, text_bytes)) || (rc = bm25_build_finish(c, ix.get()))) return rc;
    return bm_adopt(c, ix, out);
} GZ_CATCH(c)

int gz_bm25_append(gz_bm25* ix, const uint8_t* text, const int64_t* text_off, int64_t n_docs)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (n_docs < 0 || (n_docs > 0 && !text_off)) return fail(c, GZ_E_INVALID, "bad arguments");
    if (n_docs == 0) return GZ_OK;
    if (int rc = bm_host_offsets(c, text, text_off, n_docs)) return rc;
    const int64_t nbytes = text_off[n_docs] - text_off[0];
    return bm25_change(ix, [&](BmStage& st) -> int {             // (the offsets through the workspace, then as the device form)
        DBuf& off = c->w_bm[BMW_OFF];
        int rc;
        if ((rc = bm_limits(c, ix->text_bytes + nbytes, ix->n_docs + n_docs)) || (rc = bm_alloc(c, off, (size_t)(n_docs + 1) * 8)) ||
            (rc = copy_in(c, off.p, text_off, (size_t)(n_docs + 1) * 8, c->stream)))
            return rc;
        return bm25_append_core(c, ix, st, nbytes ? text + text_off[0] : nullptr, nullptr, (const int64_t*)off.p, text_off[0], n_docs, nbytes);
    });
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_append_device(gz_bm25* ix, const uint8_t* text_dev, const int64_t* text_off_dev, int64_t n_docs, int64_t text_bytes)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (n_docs < 0 || text_bytes < 0) return fail(c, GZ_E_INVALID, "bad arguments");
    if (n_docs == 0) return GZ_OK;
    return bm25_change(ix, [&](BmStage& st) -> int {
        int rc;
        if ((rc = bm_limits(c, ix->text_bytes + text_bytes, ix->n_docs + n_docs))) return rc;     // (before anything is read)
        if (!text_off_dev || (text_bytes > 0 && !text_dev)) return fail(c, GZ_E_INVALID, "bad arguments");
        int64_t off0 = 0;
        if ((rc = bm_read_off0(c, text_off_dev, off0))) return rc;
        return bm25_append_core(c, ix, st, nullptr, text_bytes ? text_dev + off0 : nullptr, text_off_dev, off0, n_docs, text_bytes);
    });
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_remove(gz_bm25* ix, const int64_t* doc_ids, int64_t n_ids)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (n_ids < 0 || (n_ids > 0 && !doc_ids)) return fail(c, GZ_E_INVALID, "bad arguments");
    if (n_ids == 0) return GZ_OK;
    return bm25_change(ix, [&](BmStage& st) -> int {             // (the ids through the workspace, then as the device form)
        DBuf& ids = c->w_bm[BMW_OFF];
        int rc;
        if ((rc = bm_alloc(c, ids, (size_t)n_ids * 8)) || (rc = copy_in(c, ids.p, doc_ids, (size_t)n_ids * 8, c->stream))) return rc;
        return bm25_remove_core(c, ix, st, (const int64_t*)ids.p, n_ids);
    });
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_remove_device(gz_bm25* ix, const int64_t* doc_ids_dev, int64_t n_ids)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (n_ids < 0 || (n_ids > 0 && !doc_ids_dev)) return fail(c, GZ_E_INVALID, "bad arguments");
    if (n_ids == 0) return GZ_OK;
    return bm25_change(ix, [&](BmStage& st) { return bm25_remove_core(c, ix, st, doc_ids_dev, n_ids); });
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_compact(gz_bm25* ix)
try {
    if (!ix) return GZ_E_INVALID;
    // (the derived lists leave as after every change: a fresh build has none, device memory included)
    return bm25_change(ix, [&](BmStage& st) { return bm25_compact_core(ix->c, ix, st); });
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_terms(gz_bm25* ix, int64_t* term_off, int32_t* df, uint8_t* bytes, int64_t bytes_cap)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if ((!term_off && !bytes) || (bytes && bytes_cap < 0)) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    BmDrain drain{c};
    GzBm25Cp C;
    int64_t B = 0;
    int rc;
    if ((rc = bm25_number(c, ix, C, B))) return rc;
    const int64_t T1 = C.n_new;
    if (bytes && bytes_cap < B) return fail(c, GZ_E_CAPACITY, "BM25 terms: %lld bytes, room for %lld", (long long)B, (long long)bytes_cap);
    if ((rc = bm_alloc(c, w[BMW_V_OFF], (size_t)(T1 + 1) * 8)) || (rc = bm_alloc(c, w[BMW_V_DF], (size_t)T1 * 4)) ||
        (bytes && (rc = bm_alloc(c, w[BMW_V_BYTES], (size_t)B + 16))))
        return rc;
    C.tstart2 = (int64_t*)w[BMW_V_OFF].p; C.close = 1; C.df2 = (uint32_t*)w[BMW_V_DF].p;
    C.arena = bytes ? (uint8_t*)w[BMW_V_BYTES].p : nullptr;
    gz_launch_bm25_compact(GZ_BM25_CP_GATHER, C, s);
    int64_t bad = 0;
    if ((rc = bm_read_u32(c, C.ctl + 1, bad))) return rc;
    HIPCHK(c, hipGetLastError());
    if (bad) return fail(c, GZ_E_HIP, "BM25 terms: the index's entries and df contradict each other");
    if (term_off && (rc = copy_out(c, term_off, C.tstart2, (size_t)(T1 + 1) * 8, s))) return rc;
    if (df && (rc = copy_out(c, df, C.df2, (size_t)T1 * 4, s))) return rc;
    if (bytes && (rc = copy_out(c, bytes, C.arena, (size_t)B, s))) return rc;
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_similar(gz_bm25* ix, const uint8_t* words, const int64_t* word_off, int64_t n_words, int32_t max_edits, int64_t k,
                    int64_t* ids_out, int32_t* dist_out, int32_t* df_out, int64_t* count_out)
try {
    int rc = bm25_vocab_args(ix, words, word_off, n_words, k);
    if (rc) return rc;
    gz_ctx* c = ix->c;
    if (max_edits < 0 || max_edits > GZ_BM25_EDIT_MAX)
        return fail(c, GZ_E_INVALID, "max_edits = %d; a vocabulary query takes 0 .. %d", max_edits, GZ_BM25_EDIT_MAX);
    std::vector<uint32_t> cps, cpoff((size_t)n_words + 1, 0u);
    for (int64_t i = 0; i < n_words; ++i) {
        const int64_t nb = word_off[i + 1] - word_off[i];
        if (nb && !vc_decode(words + word_off[i], nb, cps)) return fail(c, GZ_E_INVALID, "word %lld is not UTF-8", (long long)i);
        const size_t m = cps.size() - cpoff[(size_t)i];
        if (m > (size_t)GZ_BM25_EDIT_MAX)
            return fail(c, GZ_E_LIMIT, "word %lld has %lld code points; a vocabulary query takes at most %d", (long long)i, (long long)m, GZ_BM25_EDIT_MAX);
        cpoff[(size_t)i + 1] = (uint32_t)cps.size();
    }
    std::lock_guard<std::mutex> lk(c->mu);
    return bm25_vocab_locked(ix, words, word_off, n_words, &cps, &cpoff, max_edits, k, ids_out, dist_out, df_out, count_out);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_prefix(gz_bm25* ix, const uint8_t* words, const int64_t* word_off, int64_t n_words, int64_t k, int64_t* ids_out, int32_t* df_out,
                   int64_t* count_out)
try {
    const int rc = bm25_vocab_args(ix, words, word_off, n_words, k);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ix->c->mu);
    return bm25_vocab_locked(ix, words, word_off, n_words, nullptr, nullptr, 0, k, ids_out, nullptr, df_out, count_out);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_term_bytes(gz_bm25* ix, const int64_t* ids, int64_t n_ids, int64_t* off_out, uint8_t* bytes, int64_t bytes_cap)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (n_ids < 0 || (n_ids > 0 && !ids) || (!off_out && !bytes) || (bytes && bytes_cap < 0)) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t T = ix->n_live;
    for (int64_t i = 0; i < n_ids; ++i)
        if (ids[i] < -1 || ids[i] >= T) return fail(c, GZ_E_INVALID, "term id %lld out of range for %lld terms", (long long)ids[i], (long long)T);
    if (n_ids == 0) {
        if (off_out) off_out[0] = 0;
        return GZ_OK;
    }
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    BmDrain drain{c};
    std::vector<uint32_t> len((size_t)n_ids, 0u);
    std::vector<int64_t> off((size_t)n_ids + 1, 0);
    GzBm25Vocab V{};
    int rc;
    if (T > 0) {
        GzBm25Cp C;
        int64_t B = 0, bad = 0;
        if ((rc = bm25_number(c, ix, C, B)) || (rc = bm_read_u32(c, C.ctl + 1, bad))) return rc;
        if (bad) return fail(c, GZ_E_HIP, "BM25 vocabulary: the index's entries and df contradict each other");
        if ((rc = bm_alloc(c, w[BMW_VC_WORDS], (size_t)n_ids * 8)) || (rc = bm_alloc(c, w[BMW_VC_CNT], (size_t)n_ids * 4)) ||
            (rc = copy_in(c, w[BMW_VC_WORDS].p, ids, (size_t)n_ids * 8, s)))
            return rc;
        V.tb = C.tb; V.tstart = C.tstart; V.df = C.df; V.order = C.order; V.nlen = C.nlen; V.n_new = T;
        V.ids = (const int64_t*)w[BMW_VC_WORDS].p; V.n_ids = n_ids; V.len_out = (uint32_t*)w[BMW_VC_CNT].p;
        gz_launch_bm25_vocab(GZ_BM25_VC_LEN, V, s);
        HIPCHK(c, hipGetLastError());
        if ((rc = copy_out(c, len.data(), V.len_out, (size_t)n_ids * 4, s))) return rc;
    }
    for (int64_t i = 0; i < n_ids; ++i) off[(size_t)i + 1] = off[(size_t)i] + (int64_t)len[(size_t)i];
    const int64_t total = off[(size_t)n_ids];
    if (bytes && bytes_cap < total)
        return fail(c, GZ_E_CAPACITY, "BM25 term bytes: %lld bytes, room for %lld", (long long)total, (long long)bytes_cap);
    if (bytes && total > 0) {
        if ((rc = bm_alloc(c, w[BMW_VC_OFF], (size_t)(n_ids + 1) * 8)) || (rc = bm_alloc(c, w[BMW_VC_OUT], (size_t)total + 16)) ||
            (rc = copy_in(c, w[BMW_VC_OFF].p, off.data(), (size_t)(n_ids + 1) * 8, s)))
            return rc;
        V.boff = (const int64_t*)w[BMW_VC_OFF].p; V.bytes = (uint8_t*)w[BMW_VC_OUT].p;
        gz_launch_bm25_vocab(GZ_BM25_VC_GATHER, V, s);
        HIPCHK(c, hipGetLastError());
        if ((rc = copy_out(c, bytes, V.bytes, (size_t)total, s))) return rc;
    }
    if (off_out) std::memcpy(off_out, off.data(), (size_t)(n_ids + 1) * 8);
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_footprint(gz_bm25* ix, int64_t out[3])
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!out) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    for (const DBuf* b : {&ix->text, &ix->dl, &ix->sig, &ix->eoff, &ix->ent, &ix->ptab, &ix->ttab, &ix->tstart, &ix->tlen, &ix->df,
                          &ix->poff, &ix->pdoc,           // (the postings while they exist)
                          &ix->seq, &ix->woff})           // (a positional index: its words' term ids, and the word offsets while they exist)
        cap += b->cap;
    out[0] = ix->text_bytes; out[1] = ix->n_terms; out[2] = (int64_t)cap;
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_flags(gz_bm25* ix, int32_t* flags)
try {
    if (!ix) return GZ_E_INVALID;
    if (!flags) return fail(ix->c, GZ_E_INVALID, "bad arguments");
    *flags = ix->flags;
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_sequence(gz_bm25* ix, int32_t* terms_out, int64_t* doc_off_out)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!(ix->flags & GZ_BM25_POSITIONS)) return fail(c, GZ_E_INVALID, "the index was built without GZ_BM25_POSITIONS");
    if ((!terms_out && ix->n_words > 0) || !doc_off_out) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = bm25_word_offsets(ix))) return rc;
    const int64_t N = ix->n_docs;
    std::vector<uint32_t> off((size_t)N + 1);
    if ((rc = copy_out(c, off.data(), ix->woff.p, (size_t)(N + 1) * 4, c->stream))) return rc;
    for (int64_t d = 0; d <= N; ++d) doc_off_out[d] = (int64_t)off[(size_t)d];
    if (ix->n_words > 0 && (rc = copy_out(c, terms_out, ix->seq.p, (size_t)ix->n_words * 4, c->stream))) return rc;
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_info(gz_bm25* ix, int64_t* n_docs, int64_t* n_terms, int64_t* n_words)
try {
    if (!ix) return GZ_E_INVALID;
    if (n_docs) *n_docs = ix->n_docs;
    if (n_terms) *n_terms = ix->n_live;
    if (n_words) *n_words = ix->n_words;
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_field_lengths(gz_bm25* ix, int32_t* out)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!out && ix->n_docs > 0) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return copy_out(c, out, ix->dl.p, (size_t)ix->n_docs * 4, c->stream);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_lookup(gz_bm25* ix, const uint8_t* words, const int64_t* word_off, int64_t n, int32_t* term_out, int32_t* df_out)
try {
    if (!ix) return GZ_E_INVALID;
    gz_ctx* c = ix->c;
    if (!word_off || n < 0 || (n > 0 && (!term_out || !df_out))) return fail(c, GZ_E_INVALID, "bad arguments");
    const int64_t nbytes = word_off[n] - word_off[0];
    if (nbytes < 0 || (nbytes > 0 && !words)) return fail(c, GZ_E_INVALID, "bad word offsets");
    for (int64_t i = 0; i < n; ++i) if (word_off[i + 1] < word_off[i]) return fail(c, GZ_E_INVALID, "word offsets must not decrease");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return GZ_OK;
    DBuf* w = c->w_bm;
    hipStream_t s = c->stream;
    int rc;
    if ((rc = bm_alloc(c, w[BMW_QTEXT], (size_t)nbytes + 16)) || (rc = bm_alloc(c, w[BMW_QOFF], (size_t)(n + 1) * 8)) ||
        (rc = bm_alloc(c, w[BMW_QRES], (size_t)n * 8)))
        return rc;
    if (nbytes && (rc = copy_in(c, w[BMW_QTEXT].p, words + word_off[0], (size_t)nbytes, s))) return rc;
    if ((rc = copy_in(c, w[BMW_QOFF].p, word_off, (size_t)(n + 1) * 8, s))) return rc;
    GzBm25Look L{};
    L.tb = (const uint8_t*)ix->text.p - ix->off0; L.tstart = (const int64_t*)ix->tstart.p; L.tlen = (const uint32_t*)ix->tlen.p;
    L.df = (const uint32_t*)ix->df.p; L.ttab = (const GzBm25Slot*)ix->ttab.p; L.tmask = ix->tmask; L.hmask = ix->hmask;
    L.qtext = (const uint8_t*)w[BMW_QTEXT].p - word_off[0]; L.qoff = (const int64_t*)w[BMW_QOFF].p; L.n = n;
    L.term_out = (int32_t*)w[BMW_QRES].p; L.df_out = L.term_out + n;
    gz_launch_bm25_lookup(L, s);
    HIPCHK(c, hipGetLastError());
    if ((rc = copy_out(c, term_out, L.term_out, (size_t)n * 4, s)) || (rc = copy_out(c, df_out, L.df_out, (size_t)n * 4, s))) return rc;
    return GZ_OK;
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_score(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries, const double params[6],
                  int32_t plus, double* scores)
try {
    int rc = bm25_score_args(ix, terms, idf, query_off, n_queries, params, scores);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ix->c->mu);
    return bm25_score_locked(ix, terms, idf, query_off, n_queries, params, plus, scores, BmMem::Host);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_score_device(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries,
                         const double params[6], int32_t plus, double* scores_dev)
try {
    int rc = bm25_score_args(ix, terms, idf, query_off, n_queries, params, scores_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ix->c->mu);
    return bm25_score_locked(ix, terms, idf, query_off, n_queries, params, plus, scores_dev, BmMem::Device);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_topk(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries, const double params[6],
                 int32_t plus, int64_t k, int64_t* doc_out, double* score_out)
try {
    int rc = bm25_score_args(ix, terms, idf, query_off, n_queries, params, doc_out && score_out ? doc_out : nullptr);
    int64_t kk = 0;
    if (rc || (rc = bm25_topk_k(ix, k, kk))) return rc;
    std::lock_guard<std::mutex> lk(ix->c->mu);
    return bm25_topk_locked(ix, terms, idf, query_off, n_queries, params, plus, kk, doc_out, score_out, BmMem::Host);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_topk_device(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries,
                        const double params[6], int32_t plus, int64_t k, int64_t* doc_out_dev, double* score_out_dev)
try {
    int rc = bm25_score_args(ix, terms, idf, query_off, n_queries, params, doc_out_dev && score_out_dev ? doc_out_dev : nullptr);
    int64_t kk = 0;
    if (rc || (rc = bm25_topk_k(ix, k, kk))) return rc;
    std::lock_guard<std::mutex> lk(ix->c->mu);
    return bm25_topk_locked(ix, terms, idf, query_off, n_queries, params, plus, kk, doc_out_dev, score_out_dev, BmMem::Device);
} GZ_CATCH(ix ? ix->c : nullptr)

// The search family: every entry point fills a BmSearchReq with what it takes -- the lists of the wider forms stay unset -- and
// bm25_search_entry checks, locks and runs it.
int gz_bm25_search(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries, const double params[6],
                   int32_t plus, int64_t k, int64_t* doc_out, double* score_out, int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.doc = doc_out; R.score = score_out; R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_device(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries,
                          const double params[6], int32_t plus, int64_t k, int64_t* doc_out_dev, double* score_out_dev, int64_t* count_out_dev)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.doc = doc_out_dev; R.score = score_out_dev; R.cnt = count_out_dev; R.mem = BmMem::Device;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_match_count(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.qoff = query_off; R.nq = n_queries; R.count_only = true;
    R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_bool(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries, const double params[6],
                        int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms, const int64_t* ex_off, int64_t* doc_out, double* score_out,
                        int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off};
    R.doc = doc_out; R.score = score_out; R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_bool_device(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries,
                               const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms, const int64_t* ex_off,
                               int64_t* doc_out_dev, double* score_out_dev, int64_t* count_out_dev)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off};
    R.doc = doc_out_dev; R.score = score_out_dev; R.cnt = count_out_dev; R.mem = BmMem::Device;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_match_count_bool(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, int32_t mode, const int32_t* ex_terms,
                             const int64_t* ex_off, int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.qoff = query_off; R.nq = n_queries; R.count_only = true;
    R.mode = mode; R.ex = {ex_terms, ex_off};
    R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_phrase(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries, const double params[6],
                          int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms, const int64_t* ex_off, const int32_t* ph_terms,
                          const int64_t* ph_off, int64_t* doc_out, double* score_out, int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off}; R.ph = {ph_terms, ph_off};
    R.doc = doc_out; R.score = score_out; R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_phrase_device(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries,
                                 const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms, const int64_t* ex_off,
                                 const int32_t* ph_terms, const int64_t* ph_off, int64_t* doc_out_dev, double* score_out_dev,
                                 int64_t* count_out_dev)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off}; R.ph = {ph_terms, ph_off};
    R.doc = doc_out_dev; R.score = score_out_dev; R.cnt = count_out_dev; R.mem = BmMem::Device;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_match_count_phrase(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, int32_t mode,
                               const int32_t* ex_terms, const int64_t* ex_off, const int32_t* ph_terms, const int64_t* ph_off, int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.qoff = query_off; R.nq = n_queries; R.count_only = true;
    R.mode = mode; R.ex = {ex_terms, ex_off}; R.ph = {ph_terms, ph_off};
    R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_near(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries, const double params[6],
                        int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms, const int64_t* ex_off, const int32_t* ph_terms,
                        const int64_t* ph_off, const int32_t* near_terms, const int64_t* near_off, const int64_t* near_window, int64_t* doc_out,
                        double* score_out, int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off}; R.ph = {ph_terms, ph_off}; R.nr = {near_terms, near_off}; R.nrwin = near_window;
    R.doc = doc_out; R.score = score_out; R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_near_device(gz_bm25* ix, const int32_t* terms, const double* idf, const int64_t* query_off, int64_t n_queries,
                               const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms, const int64_t* ex_off,
                               const int32_t* ph_terms, const int64_t* ph_off, const int32_t* near_terms, const int64_t* near_off,
                               const int64_t* near_window, int64_t* doc_out_dev, double* score_out_dev, int64_t* count_out_dev)
try {
    BmSearchReq R;
    R.terms = terms; R.idf = idf; R.qoff = query_off; R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off}; R.ph = {ph_terms, ph_off}; R.nr = {near_terms, near_off}; R.nrwin = near_window;
    R.doc = doc_out_dev; R.score = score_out_dev; R.cnt = count_out_dev; R.mem = BmMem::Device;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_match_count_near(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, int32_t mode, const int32_t* ex_terms,
                             const int64_t* ex_off, const int32_t* ph_terms, const int64_t* ph_off, const int32_t* near_terms,
                             const int64_t* near_off, const int64_t* near_window, int64_t* count_out)
try {
    BmSearchReq R;
    R.terms = terms; R.qoff = query_off; R.nq = n_queries; R.count_only = true;
    R.mode = mode; R.ex = {ex_terms, ex_off}; R.ph = {ph_terms, ph_off}; R.nr = {near_terms, near_off}; R.nrwin = near_window;
    R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_groups(gz_bm25* ix, const int32_t* alt_terms, const int64_t* alt_off, const double* group_idf, const int64_t* group_off,
                          int64_t n_queries, const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms,
                          const int64_t* ex_off, int64_t* doc_out, double* score_out, int64_t* count_out)
try {
    BmSearchReq R;
    R.grouped = true; R.alt_terms = alt_terms; R.alt_off = alt_off; R.group_idf = group_idf; R.group_off = group_off;
    R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off};
    R.doc = doc_out; R.score = score_out; R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_search_groups_device(gz_bm25* ix, const int32_t* alt_terms, const int64_t* alt_off, const double* group_idf, const int64_t* group_off,
                                 int64_t n_queries, const double params[6], int32_t plus, int64_t k, int32_t mode, const int32_t* ex_terms,
                                 const int64_t* ex_off, int64_t* doc_out_dev, double* score_out_dev, int64_t* count_out_dev)
try {
    BmSearchReq R;
    R.grouped = true; R.alt_terms = alt_terms; R.alt_off = alt_off; R.group_idf = group_idf; R.group_off = group_off;
    R.nq = n_queries; R.P = params; R.plus = plus; R.k = k;
    R.mode = mode; R.ex = {ex_terms, ex_off};
    R.doc = doc_out_dev; R.score = score_out_dev; R.cnt = count_out_dev; R.mem = BmMem::Device;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_match_count_groups(gz_bm25* ix, const int32_t* alt_terms, const int64_t* alt_off, const int64_t* group_off, int64_t n_queries,
                               int32_t mode, const int32_t* ex_terms, const int64_t* ex_off, int64_t* count_out)
try {
    BmSearchReq R;
    R.grouped = true; R.alt_terms = alt_terms; R.alt_off = alt_off; R.group_off = group_off;
    R.nq = n_queries; R.count_only = true;
    R.mode = mode; R.ex = {ex_terms, ex_off};
    R.cnt = count_out; R.mem = BmMem::Host;
    return bm25_search_entry(ix, R);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_cover(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, const int64_t* ids, int64_t k, int32_t* start_out,
                  int32_t* len_out, int32_t* words_out)
try {
    int rc = bm25_snip_args(ix, terms, query_off, n_queries, k);
    if (rc || (rc = bm25_cover_args(ix, query_off, n_queries))) return rc;
    gz_ctx* c = ix->c;
    if (n_queries * k > 0 && (!ids || !start_out || !len_out || !words_out)) return fail(c, GZ_E_INVALID, "bad arguments");
    if ((rc = bm25_snip_ids(ix, ids, n_queries * k))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return bm25_cover_locked(ix, terms, query_off, n_queries, k, ids, start_out, len_out, words_out, BmMem::Host);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_cover_device(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, const int64_t* ids_dev, int64_t k,
                         int32_t* start_out_dev, int32_t* len_out_dev, int32_t* words_out_dev)
try {
    int rc = bm25_snip_args(ix, terms, query_off, n_queries, k);
    if (rc || (rc = bm25_cover_args(ix, query_off, n_queries))) return rc;
    gz_ctx* c = ix->c;
    if (n_queries * k > 0 && (!ids_dev || !start_out_dev || !len_out_dev || !words_out_dev)) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    return bm25_cover_locked(ix, terms, query_off, n_queries, k, ids_dev, start_out_dev, len_out_dev, words_out_dev, BmMem::Device);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_snippets(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, const int64_t* ids, int64_t k, int64_t width,
                     int32_t* start_out, int32_t* hits_out)
try {
    int rc = bm25_snip_args(ix, terms, query_off, n_queries, k);
    if (rc) return rc;
    gz_ctx* c = ix->c;
    if (width < 1) return fail(c, GZ_E_INVALID, "width = %lld; a snippet takes width >= 1", (long long)width);
    if (n_queries * k > 0 && (!ids || !start_out || !hits_out)) return fail(c, GZ_E_INVALID, "bad arguments");
    if ((rc = bm25_snip_ids(ix, ids, n_queries * k))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return bm25_snippets_locked(ix, terms, query_off, n_queries, k, width, ids, start_out, hits_out, BmMem::Host);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_snippets_device(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, const int64_t* ids_dev, int64_t k,
                            int64_t width, int32_t* start_out_dev, int32_t* hits_out_dev)
try {
    int rc = bm25_snip_args(ix, terms, query_off, n_queries, k);
    if (rc) return rc;
    gz_ctx* c = ix->c;
    if (width < 1) return fail(c, GZ_E_INVALID, "width = %lld; a snippet takes width >= 1", (long long)width);
    if (n_queries * k > 0 && (!ids_dev || !start_out_dev || !hits_out_dev)) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    return bm25_snippets_locked(ix, terms, query_off, n_queries, k, width, ids_dev, start_out_dev, hits_out_dev, BmMem::Device);
} GZ_CATCH(ix ? ix->c : nullptr)

int gz_bm25_occurrences(gz_bm25* ix, const int32_t* terms, const int64_t* query_off, int64_t n_queries, const int64_t* ids, int64_t k,
                        int64_t* pair_off_out, int32_t* pos_out, int32_t* word_out, int64_t cap)
try {
    int rc = bm25_snip_args(ix, terms, query_off, n_queries, k);
    if (rc) return rc;
    gz_ctx* c = ix->c;
    if (!pair_off_out || (n_queries * k > 0 && !ids) || (pos_out && (!word_out || cap < 0))) return fail(c, GZ_E_INVALID, "bad arguments");
    if ((rc = bm25_snip_ids(ix, ids, n_queries * k))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return bm25_occurrences_locked(ix, terms, query_off, n_queries, ids, k, pair_off_out, pos_out, word_out, cap);
} GZ_CATCH(ix ? ix->c : nullptr)

void gz_bm25_destroy(gz_bm25* ix)
try {
    if (!ix) return;
    gz_ctx* c = ix->c;
    std::lock_guard<std::mutex> lk(c->mu);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);                             // (a scoring call into device memory may still read the index)
    auto& v = c->bm25_live;
    v.erase(std::remove(v.begin(), v.end(), ix), v.end());
    delete ix;
} GZ_CATCH_VOID

}  // extern "C"
