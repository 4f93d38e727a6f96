// The word sets and the BPE learner behind the C ABI (gz_wordset_*, gz_bpe_learn*).  Included by gz_api.cpp behind gz_bm25_api.inc,
// whose workspace (BMW_*), word front (bm_front_count, bm_front_words), entry-point helpers, bm_alloc, bm_scan, bm_read_u32, bm_limits
// and BmDrain it shares; the kernels are in gz_learn.inc, the host rules in gz_learn_host.h.
//
// A word set lives on the host once it is built: the distinct words' bytes in first-occurrence order, their offsets and int64
// counts.  The build calls the word front the BM25 build and append call -- count, scan, words, hash, de-duplication rounds, first,
// scan: there is one copy of it, in gz_bm25_api.inc -- and follows it with one counting kernel and a gather; nothing of a BM25 index
// is made.  The counts form runs the same front with every given word as a document of its own and its count as the document's
// weight: words given twice add up.
//
// gz_bpe_learn: the host numbers the initial symbols and interns the merged ones (gz_learn_host.h), the device holds the words'
// symbols and the pair table.  Per step: the arg-best reduction, ONE small readback (the best key and count, the keys in the
// table, the overflow flag), the host's stop rule and interning, the apply kernels.  The table is sized before every step: the
// keys a step can add all hold the merged symbol m, so they are at most min(2 n(l, r), 2 S + 1) for S symbols, and the table grows
// (rehash into a larger one) while keys + that bound would pass 3/4 of the slots.  A probe that finds the table full all the same
// raises a flag and the call fails: nothing is dropped silently.

#include "gz_learn_host.h"

struct gz_wordset {
    gz_ctx* c = nullptr;
    std::vector<uint8_t> bytes;
    std::vector<int64_t> off{0}, cnt;
    int64_t total = 0;
    // the last gz_bpe_learn
    bool learnt = false;
    std::vector<std::string> merge_str;                         // left, right, left, right, ...
    std::vector<std::pair<std::string, int64_t>> piece;
};

namespace {

struct LnBufs {
    static constexpr int N = 12;
    DBuf b[N];
    ~LnBufs() { for (DBuf& x : b) release(x); }
};

// The distinct words of N documents and their counts into ws.  tb + off[d] = the first byte of document d (device), the offsets
// lie in [lo, lo + text_bytes]; weight (device, may be null): the count every word of document d stands for; strict: every document
// must be exactly one word.
int wordset_core(gz_ctx* c, gz_wordset* ws, LnBufs& B, const uint8_t* tb, const int64_t* off_dev, int64_t N, int64_t lo, int64_t text_bytes,
                 const long long* weight, bool strict)
{
    hipStream_t s = c->stream;
    int rc;
    // ---- the word front (gz_bm25_api.inc) on counters of the word set's own; no term ids, no table of an index
    GzBm25Args A{};
    A.tb = tb; A.off = off_dev; A.n_docs = N; A.lo = lo; A.hi = lo + text_bytes;
    A.hmask = bm_hmask(c);
    if ((rc = bm_alloc(c, B.b[0], (size_t)N * 4))) return rc;
    A.wcnt = (uint32_t*)B.b[0].p;
    int64_t W = 0, T = 0, bad = 0;
    if ((rc = bm_front_count(c, A, "word set:", W))) return rc;
    if (strict && W != N) return fail(c, GZ_E_INVALID, "word set: %lld words were given, they split into %lld", (long long)N, (long long)W);
    if ((rc = bm_front_words(c, A, false, T))) return rc;

    // ---- the counts, the distinct words' byte ranges, their bytes
    const size_t t1 = (size_t)T + 1;
    if ((rc = bm_alloc(c, B.b[1], t1 * 8 * GZ_BM25_DF_SHARDS)) || (rc = bm_alloc(c, B.b[2], t1 * 8)) || (rc = bm_alloc(c, B.b[3], t1 * 4)) || (rc = bm_alloc(c, B.b[4], t1 * 4)))
        return rc;
    long long* cnt = (long long*)B.b[1].p;
    A.tstart = (int64_t*)B.b[2].p; A.tlen = (uint32_t*)B.b[3].p;
    uint32_t* toff = (uint32_t*)B.b[4].p;
    HIPCHK(c, hipMemsetAsync(cnt, 0, t1 * 8 * GZ_BM25_DF_SHARDS, s));
    gz_launch_wordset_count(A, weight, cnt, T, strict ? 1 : 0, s);
    if ((rc = bm_scan(c, A.tlen, T, toff))) return rc;
    int64_t nbytes = 0;
    if ((rc = bm_read_u32(c, A.ctl + 1, bad)) || (rc = bm_read_u32(c, toff + T, nbytes))) return rc;
    if (bad) return fail(c, GZ_E_INVALID, "word set: a given word is not one word (it holds whitespace)");
    if ((rc = bm_alloc(c, B.b[5], (size_t)nbytes + 16))) return rc;
    gz_launch_wordset_gather(tb, A.tstart, A.tlen, toff, (uint8_t*)B.b[5].p, T, s);
    HIPCHK(c, hipGetLastError());
    alloc_site(c);
    std::vector<uint32_t> off32(t1);
    ws->bytes.resize((size_t)nbytes);
    ws->cnt.resize((size_t)T);
    if ((rc = copy_out(c, off32.data(), toff, t1 * 4, s)) || (rc = copy_out(c, ws->cnt.data(), cnt, (size_t)T * 8, s)) ||
        (rc = copy_out(c, ws->bytes.data(), B.b[5].p, (size_t)nbytes, s)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    ws->off.assign(off32.begin(), off32.end());
    ws->total = 0;
    for (int64_t v : ws->cnt) {
        if (v < 1 || v >= GZ_LEARN_COUNT_LIMIT - ws->total) return fail(c, GZ_E_LIMIT, "word set: the counts sum to 2^62 or more");
        ws->total += v;
    }
    return GZ_OK;
}

uint64_t ln_slots_for(uint64_t keys) { return bm_pow2(keys + keys / 3 + 16); }               // load <= 3/4

// the table of L into one of `slots` slots (fresh.p replaces tab.p); keys counted again, the overflow flag is the caller's to read
int ln_grow(gz_ctx* c, GzLearn& L, DBuf& tab, DBuf& fresh, uint64_t slots)
{
    hipStream_t s = c->stream;
    int rc;
    if ((rc = bm_alloc(c, fresh, (size_t)slots * 16))) return rc;
    HIPCHK(c, hipMemsetAsync(fresh.p, 0, (size_t)slots * 16, s));
    HIPCHK(c, hipMemsetAsync(L.ctl + 2, 0, 8, s));
    const GzLearnSlot* from = L.tab;
    const int64_t n_from = (int64_t)(L.mask + 1);
    L.tab = (GzLearnSlot*)fresh.p; L.mask = slots - 1;
    gz_launch_learn_rehash(from, n_from, L, s);
    HIPCHK(c, hipStreamSynchronize(s));                         // (the old table is freed next)
    std::swap(tab, fresh);
    release(fresh);
    return GZ_OK;
}

int learn_core(gz_ctx* c, gz_wordset* ws, LnBufs& B, int64_t n_merges, int64_t min_frequency, int64_t info[8])
{
    hipStream_t s = c->stream;
    int rc;
    alloc_site(c);
    LearnHost H;
    const int64_t D = (int64_t)ws->cnt.size();
    if (const char* why = H.init(ws->bytes.data(), ws->off.data(), ws->cnt.data(), D, (uint32_t)GZ_LEARN_LANE_MAX)) return fail(c, GZ_E_LIMIT, "%s", why);
    const int64_t P = (int64_t)H.flat.size();
    std::vector<uint32_t> wlen((size_t)D);
    for (int64_t d = 0; d < D; ++d) wlen[(size_t)d] = H.woff[(size_t)d + 1] - H.woff[(size_t)d];
    DBuf &d_sym = B.b[0], &d_woff = B.b[1], &d_wlen = B.b[2], &d_cw = B.b[3], &d_long = B.b[4], &d_tab = B.b[5], &d_ctl = B.b[6], &d_part = B.b[7],
         &d_hist = B.b[8], &d_fresh = B.b[9];
    if ((rc = bm_alloc(c, d_sym, (size_t)P * 4)) || (rc = bm_alloc(c, d_woff, (size_t)(D + 1) * 4)) || (rc = bm_alloc(c, d_wlen, (size_t)D * 4)) ||
        (rc = bm_alloc(c, d_cw, (size_t)D * 8)) || (rc = bm_alloc(c, d_long, H.longw.size() * 4)) || (rc = bm_alloc(c, d_ctl, 64)))
        return rc;
    if ((rc = copy_in(c, d_sym.p, H.flat.data(), (size_t)P * 4, s)) || (rc = copy_in(c, d_woff.p, H.woff.data(), (size_t)(D + 1) * 4, s)) ||
        (rc = copy_in(c, d_wlen.p, wlen.data(), (size_t)D * 4, s)) || (rc = copy_in(c, d_cw.p, ws->cnt.data(), (size_t)D * 8, s)) ||
        (rc = copy_in(c, d_long.p, H.longw.data(), H.longw.size() * 4, s)))
        return rc;
    GzLearn L{};
    L.sym = (int32_t*)d_sym.p; L.woff = (const uint32_t*)d_woff.p; L.wlen = (uint32_t*)d_wlen.p; L.cw = (const long long*)d_cw.p; L.n_words = D;
    L.longw = (const uint32_t*)d_long.p; L.n_long = (int64_t)H.longw.size();
    L.ctl = (unsigned long long*)d_ctl.p;

    // ---- the initial table.  Its keys are at most min(adjacent positions, S^2); the switch learn_table_bits starts from 2^bits
    // slots instead, and a table that proves too small is cleared, doubled and filled again (the words are not yet changed).
    const uint64_t S0 = (uint64_t)H.sym.size();
    const uint64_t bound0 = std::min<uint64_t>((uint64_t)H.adjacent, S0 * S0);
    const int tbits = c->opt.learn_table_bits;
    uint64_t slots = tbits > 0 ? 1ull << tbits : std::max<uint64_t>(ln_slots_for(bound0), 1ull << 16);
    int64_t n_grown = 0;
    unsigned long long ctl[4] = {};
    for (;; slots <<= 1, ++n_grown) {
        if ((rc = bm_alloc(c, d_tab, (size_t)slots * 16))) return rc;
        HIPCHK(c, hipMemsetAsync(d_tab.p, 0, (size_t)slots * 16, s));
        HIPCHK(c, hipMemsetAsync(L.ctl, 0, 64, s));
        L.tab = (GzLearnSlot*)d_tab.p; L.mask = slots - 1;
        gz_launch_learn(GZ_LEARN_PAIRS, L, s);
        if ((rc = copy_out_small(c, ctl, L.ctl, 32, s))) return rc;
        if (!ctl[3] && (ctl[2] + ctl[2] / 3 + 16 <= slots || tbits == 0)) break;
        if (slots >= (1ull << 40)) return fail(c, GZ_E_LIMIT, "BPE learner: the pair table passed 2^40 slots");
        release(d_tab);
    }
    const int max_part = 1024;
    if ((rc = bm_alloc(c, d_part, (size_t)max_part * 16))) return rc;
    L.part = (unsigned long long*)d_part.p;

    // ---- the steps
    int64_t done = 0;
    for (; done < n_merges; ++done) {
        L.n_part = (int32_t)std::min<uint64_t>((uint64_t)max_part, (slots + 2047) / 2048);
        gz_launch_learn(GZ_LEARN_BEST, L, s);
        if ((rc = copy_out_small(c, ctl, L.ctl, 32, s))) return rc;
        if (ctl[3]) return fail(c, GZ_E_LIMIT, "BPE learner: the pair table of %llu slots is full", (unsigned long long)slots);
        const long long best = (long long)ctl[1];
        if (best < 1 || best < min_frequency) break;
        const unsigned long long key = ctl[0] - 1ull;
        L.l = (int32_t)(key >> 32); L.r = (int32_t)(key & 0xFFFFFFFFull);
        if (L.l < 0 || L.r < 0 || (size_t)L.l >= H.sym.size() || (size_t)L.r >= H.sym.size())
            return fail(c, GZ_E_HIP, "BPE learner: the pair table holds a key of no symbol");
        if (H.sym.size() >= (size_t)INT32_MAX) return fail(c, GZ_E_LIMIT, "BPE learner: more than 2^31 - 1 symbols");
        alloc_site(c);
        L.m = H.merge(L.l, L.r);
        // every key the step can add holds m: at most 2 per merged occurrence, and at most 2 S + 1 in all
        const uint64_t add = std::min<uint64_t>(2ull * (uint64_t)best, 2ull * (uint64_t)H.sym.size() + 1ull);
        const uint64_t need = ctl[2] + add;
        if (need + need / 3 + 16 > slots) {
            slots = tbits > 0 ? ln_slots_for(need) : ln_slots_for(2 * need);
            if ((rc = ln_grow(c, L, d_tab, d_fresh, slots))) return rc;
            ++n_grown;
        }
        gz_launch_learn(GZ_LEARN_APPLY, L, s);
    }

    // ---- the final segmentation's pieces
    const size_t S = H.sym.size();
    if ((rc = bm_alloc(c, d_hist, S * 16))) return rc;
    L.hist = (long long*)d_hist.p;
    HIPCHK(c, hipMemsetAsync(d_hist.p, 0, S * 16, s));
    gz_launch_learn(GZ_LEARN_HIST, L, s);
    HIPCHK(c, hipGetLastError());
    alloc_site(c);
    std::vector<int64_t> hist(S * 2);
    if ((rc = copy_out(c, hist.data(), d_hist.p, S * 16, s)) || (rc = copy_out_small(c, ctl, L.ctl, 32, s))) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    if (ctl[3]) return fail(c, GZ_E_LIMIT, "BPE learner: the pair table of %llu slots is full", (unsigned long long)slots);
    ws->merge_str.clear();
    for (const auto& m : H.merges) { ws->merge_str.push_back(H.sym[(size_t)m.first]); ws->merge_str.push_back(H.sym[(size_t)m.second]); }
    H.pieces(hist.data(), ws->piece);
    ws->learnt = true;
    int64_t mb = 0, pb = 0;
    for (const std::string& x : ws->merge_str) mb += (int64_t)x.size();
    for (const auto& x : ws->piece) pb += (int64_t)x.first.size();
    const int64_t out[8] = {done, (int64_t)S, mb, (int64_t)ws->piece.size(), pb, (int64_t)slots, (int64_t)ctl[2], n_grown};
    for (int i = 0; i < 8; ++i) info[i] = out[i];
    return GZ_OK;
}

int wordset_adopt(gz_ctx* c, std::unique_ptr<gz_wordset>& ws, gz_wordset** out)
{
    (void)c;
    *out = ws.release();
    return GZ_OK;
}

}  // namespace

extern "C" {

int gz_wordset_build(gz_ctx* c, const uint8_t* text, const int64_t* text_off, int64_t n_docs, gz_wordset** out)
try {
    if (!c || !out || !text_off || n_docs < 0) return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    *out = nullptr;
    int rc;
    if ((rc = bm_host_offsets(c, text, text_off, n_docs))) return rc;
    const int64_t nbytes = text_off[n_docs] - text_off[0];
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = bm_limits(c, nbytes, n_docs))) return rc;
    alloc_site(c);
    std::unique_ptr<gz_wordset> ws(new gz_wordset());
    ws->c = c;
    LnBufs B;
    BmDrain drain{c};
    if ((rc = bm_upload(c, B.b[6], text, text_off, n_docs, nbytes))) return rc;
    if ((rc = wordset_core(c, ws.get(), B, (const uint8_t*)B.b[6].p - text_off[0], (const int64_t*)c->w_bm[BMW_OFF].p, n_docs, text_off[0], nbytes,
                           nullptr, false)))
        return rc;
    return wordset_adopt(c, ws, out);
} GZ_CATCH(c)

int gz_wordset_build_device(gz_ctx* c, const uint8_t* text_dev, const int64_t* text_off_dev, int64_t n_docs, int64_t text_bytes, gz_wordset** out)
try {
    if (!c || !out || !text_off_dev || n_docs < 0 || text_bytes < 0 || (text_bytes > 0 && !text_dev))
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = bm_limits(c, text_bytes, n_docs))) return rc;
    alloc_site(c);
    std::unique_ptr<gz_wordset> ws(new gz_wordset());
    ws->c = c;
    LnBufs B;
    BmDrain drain{c};
    int64_t off0 = 0;
    if ((rc = bm_read_off0(c, text_off_dev, off0))) return rc;
    // (the caller's text is read where it lies: nothing of it is kept)
    if ((rc = wordset_core(c, ws.get(), B, text_dev, text_off_dev, n_docs, off0, text_bytes, nullptr, false))) return rc;
    return wordset_adopt(c, ws, out);
} GZ_CATCH(c)

int gz_wordset_from_counts(gz_ctx* c, const uint8_t* words, const int64_t* word_off, const int64_t* counts, int64_t n_words, gz_wordset** out)
try {
    if (!c || !out || !word_off || n_words < 0 || (n_words > 0 && !counts)) return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    *out = nullptr;
    const int64_t nbytes = word_off[n_words] - word_off[0];
    if (nbytes < 0 || (nbytes > 0 && !words)) return fail(c, GZ_E_INVALID, "bad word offsets");
    int64_t total = 0;
    for (int64_t d = 0; d < n_words; ++d) {
        if (word_off[d + 1] <= word_off[d]) return fail(c, GZ_E_INVALID, "word set: word %lld is empty or its offsets decrease", (long long)d);
        if (counts[d] < 1) return fail(c, GZ_E_INVALID, "word set: count %lld of word %lld is below 1", (long long)counts[d], (long long)d);
        if (counts[d] >= GZ_LEARN_COUNT_LIMIT - total) return fail(c, GZ_E_LIMIT, "word set: the counts sum to 2^62 or more");
        total += counts[d];
    }
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = bm_limits(c, nbytes, n_words))) return rc;
    alloc_site(c);
    std::unique_ptr<gz_wordset> ws(new gz_wordset());
    ws->c = c;
    LnBufs B;
    BmDrain drain{c};
    if ((rc = bm_upload(c, B.b[6], words, word_off, n_words, nbytes)) || (rc = bm_alloc(c, B.b[7], (size_t)n_words * 8)) ||
        (rc = copy_in(c, B.b[7].p, counts, (size_t)n_words * 8, c->stream)))
        return rc;
    if ((rc = wordset_core(c, ws.get(), B, (const uint8_t*)B.b[6].p - word_off[0], (const int64_t*)c->w_bm[BMW_OFF].p, n_words, word_off[0], nbytes,
                           (const long long*)B.b[7].p, true)))
        return rc;
    return wordset_adopt(c, ws, out);
} GZ_CATCH(c)

int gz_wordset_info(gz_wordset* ws, int64_t* n_words, int64_t* n_bytes, int64_t* total)
{
    if (!ws) return GZ_E_INVALID;
    if (n_words) *n_words = (int64_t)ws->cnt.size();
    if (n_bytes) *n_bytes = (int64_t)ws->bytes.size();
    if (total) *total = ws->total;
    return GZ_OK;
}

int gz_wordset_words(gz_wordset* ws, int64_t* word_off, int64_t* counts, uint8_t* bytes, int64_t bytes_cap)
{
    if (!ws) return GZ_E_INVALID;
    gz_ctx* c = ws->c;
    if (bytes && bytes_cap < (int64_t)ws->bytes.size())
        return fail(c, GZ_E_CAPACITY, "word set: %lld bytes, room for %lld", (long long)ws->bytes.size(), (long long)bytes_cap);
    if (word_off) std::memcpy(word_off, ws->off.data(), ws->off.size() * 8);
    if (counts && !ws->cnt.empty()) std::memcpy(counts, ws->cnt.data(), ws->cnt.size() * 8);
    if (bytes && !ws->bytes.empty()) std::memcpy(bytes, ws->bytes.data(), ws->bytes.size());
    return GZ_OK;
}

void gz_wordset_destroy(gz_wordset* ws)
try {
    delete ws;
} GZ_CATCH_VOID

int gz_bpe_learn(gz_wordset* ws, int64_t n_merges, int64_t min_frequency, int64_t info[8])
try {
    if (!ws) return GZ_E_INVALID;
    gz_ctx* c = ws->c;
    if (!info) return fail(c, GZ_E_INVALID, "bad arguments");
    if (const char* why = learn_args_fault(n_merges, min_frequency)) return fail(c, GZ_E_INVALID, "%s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    ws->learnt = false;
    LnBufs B;
    BmDrain drain{c};
    return learn_core(c, ws, B, n_merges, min_frequency, info);
} GZ_CATCH(ws ? ws->c : nullptr)

int gz_bpe_learn_result(gz_wordset* ws, int64_t* merge_off, uint8_t* merge_bytes, int64_t merge_cap, int64_t* piece_off, int64_t* piece_count,
                        uint8_t* piece_bytes, int64_t piece_cap)
try {
    if (!ws) return GZ_E_INVALID;
    gz_ctx* c = ws->c;
    if (!ws->learnt) return fail(c, GZ_E_INVALID, "gz_bpe_learn_result: no gz_bpe_learn has succeeded on this word set");
    int64_t mb = 0, pb = 0;
    for (const std::string& x : ws->merge_str) mb += (int64_t)x.size();
    for (const auto& x : ws->piece) pb += (int64_t)x.first.size();
    if ((merge_bytes && merge_cap < mb) || (piece_bytes && piece_cap < pb))
        return fail(c, GZ_E_CAPACITY, "BPE learner: %lld merge bytes and %lld piece bytes, room for %lld and %lld", (long long)mb, (long long)pb,
                    (long long)merge_cap, (long long)piece_cap);
    int64_t o = 0;
    for (size_t i = 0; i < ws->merge_str.size(); ++i) {
        const std::string& x = ws->merge_str[i];
        if (merge_off) merge_off[i] = o;
        if (merge_bytes && !x.empty()) std::memcpy(merge_bytes + o, x.data(), x.size());
        o += (int64_t)x.size();
    }
    if (merge_off) merge_off[ws->merge_str.size()] = o;
    o = 0;
    for (size_t i = 0; i < ws->piece.size(); ++i) {
        const std::string& x = ws->piece[i].first;
        if (piece_off) piece_off[i] = o;
        if (piece_count) piece_count[i] = ws->piece[i].second;
        if (piece_bytes && !x.empty()) std::memcpy(piece_bytes + o, x.data(), x.size());
        o += (int64_t)x.size();
    }
    if (piece_off) piece_off[ws->piece.size()] = o;
    return GZ_OK;
} GZ_CATCH(ws ? ws->c : nullptr)

}  // extern "C"
