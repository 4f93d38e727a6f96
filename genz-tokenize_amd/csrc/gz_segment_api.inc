// Word segmentation by lexicon behind the C ABI (gz_lexicon_create, _info, _destroy, gz_segment_batch, gz_segment_batch_device).
// Included by gz_api.cpp behind gz_clf_api.inc; the kernels are in gz_segment.inc.  The whitespace pieces come from the word front of
// gz_bm25_api.inc -- bm_front_count and the GZ_BM25_WORDS kernel, with its workspace (BMW_*), bm_alloc, bm_scan and bm_read_u32: there
// is one splitter -- and the host forms stage their text through gz_rows_api.inc's row front (RowsIn, rows_check, rows_stage).
//
// A lexicon owns its open-addressing table (hash, cost, where the entry's bytes are), the entries' folded bytes and the bit filter
// over their hashes, all built on the host when it is created and uploaded once.  It belongs to its context: every call on it runs on
// the context's stream under the context's lock, and gz_destroy frees what is left.  A segment call waits for the piece count and
// the token count (they size the next buffers), for the output's size -- where a call that only sizes, or one whose output does not
// fit, ends, before any lexicon work -- and for its end.

struct gz_lexicon {
    gz_ctx* c = nullptr;
    int64_t n = 0, n_bytes = 0;
    int32_t K = 0, flags = 0;
    uint32_t max_len = 0;
    unsigned long long hmask = 0, tmask = 0;
    DBuf tab, ebytes, filter;
    hipEvent_t ev[5] = {};
    int64_t last[12] = {};               // the last segment call: documents, tokens, stretches, those of 1 / 2..8 / more tokens, the longest,
                                         // and the nanoseconds of front, candidates, walk, emit
    ~gz_lexicon()
    {
        release(tab); release(ebytes); release(filter);
        for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    }
    int64_t device_bytes() const { return (int64_t)(tab.cap + ebytes.cap + filter.cap); }
};

namespace {
void lexicon_free(gz_lexicon* lex) { delete lex; }

enum { SGW_WCNT, SGW_PTC, SGW_PTOFF, SGW_TSTART, SGW_TLEN, SGW_TDOC, SGW_TLSUM, SGW_DOCLEN, SGW_STATS, SGW_CAND, SGW_REACH, SGW_CLOSED, SGW_STARTS,
       SGW_CTL, SGW_CHOICE, SGW_JOIN, SGW_TOKOFF, SGW_OUT, SGW_COUNT };
static_assert(SGW_COUNT <= (int)(sizeof(gz_ctx::w_seg) / sizeof(DBuf)), "gz_ctx::w_seg is too small");

const char* const kLexHandle = "the lexicon is NULL, destroyed or belongs to another context";

bool lex_live(gz_ctx* c, const gz_lexicon* lex) { return lex && std::find(c->lex_live.begin(), c->lex_live.end(), lex) != c->lex_live.end(); }

// an entry as a refusal shows it: its index and its first bytes
const char* lex_name(const uint8_t* p, int64_t len, int64_t i)
{
    static thread_local std::string s;
    s = "entry " + std::to_string((long long)i) + " \"";
    s.append((const char*)p, (size_t)(len < 48 ? len : 48));
    s += len > 48 ? "...\"" : "\"";
    return s.c_str();
}

// the device outputs of a call; out null: the call only sizes.  stats, join and tok_off may be null: the first two then live in the
// workspace, the third is not made unless want_tok
struct SegOut { uint8_t* out; int64_t capacity; int64_t* out_off; int64_t* stats; uint8_t* join; int64_t* tok_off; bool want_tok; int64_t n_tokens; };

// The call on the context's stream.  tb + off[d] = document d's first byte (device); the offsets lie in [lo, lo + nbytes].  n_docs > 0.
int segment_core(gz_ctx* c, gz_lexicon* lex, const uint8_t* tb, const int64_t* off_dev, int64_t N, int64_t lo, int64_t nbytes, uint32_t flags,
                 uint32_t unk_cost, SegOut& O, int64_t* total)
{
    hipStream_t s = c->stream;
    DBuf* w = c->w_bm;
    DBuf* g = c->w_seg;
    int rc;
    *total = 0;
    HIPCHK(c, hipEventRecord(lex->ev[0], s));
    // ---- the word front: pieces per document, their scan, their byte ranges
    GzBm25Args A{};
    A.tb = tb; A.off = off_dev; A.n_docs = N; A.lo = lo; A.hi = lo + nbytes; A.hmask = bm_hmask(c);
    if ((rc = bm_alloc(c, g[SGW_WCNT], (size_t)N * 4))) return rc;
    A.wcnt = (uint32_t*)g[SGW_WCNT].p;
    int64_t W = 0, T = 0;
    if ((rc = bm_front_count(c, A, "segment: document", W))) return rc;
    const size_t w1 = (size_t)W + 1;
    // (a token has a byte: the scans below run over at most nbytes + 1 elements)
    if ((rc = bm_alloc(c, w[BMW_WSTART], w1 * 8)) || (rc = bm_alloc(c, w[BMW_WEND], w1 * 8)) || (rc = bm_alloc(c, w[BMW_WDOC], w1 * 4)) ||
        (rc = bm_alloc(c, w[BMW_BSUM], (size_t)((nbytes + N) / 4096 + 4) * 4)) || (rc = bm_alloc(c, g[SGW_PTC], w1 * 4)) || (rc = bm_alloc(c, g[SGW_PTOFF], (w1 + 1) * 4)))
        return rc;
    A.wstart = (int64_t*)w[BMW_WSTART].p; A.wend = (int64_t*)w[BMW_WEND].p; A.wdoc = (uint32_t*)w[BMW_WDOC].p;
    gz_launch_bm25(GZ_BM25_WORDS, A, nullptr, 0, nullptr, s);
    // ---- tokens
    GzSegArgs S{};
    S.tb = tb; S.off = off_dev; S.n_docs = N; S.lo = A.lo; S.hi = A.hi;
    S.wstart = A.wstart; S.wend = A.wend; S.wdoc = A.wdoc; S.woff = A.woff; S.n_pieces = W;
    S.split_punct = (flags & GZ_SEG_SPLIT_PUNCT) ? 1 : 0; S.fold_case = (lex->flags & GZ_LEX_FOLD_CASE) ? 1 : 0; S.K = lex->K; S.unk_cost = unk_cost;
    S.ptc = (uint32_t*)g[SGW_PTC].p; S.ptoff = (const uint32_t*)g[SGW_PTOFF].p;
    gz_launch_segment(GZ_SEG_COUNT, S, false, s);
    if ((rc = bm_scan(c, S.ptc, W, (uint32_t*)g[SGW_PTOFF].p)) || (rc = bm_read_u32(c, S.ptoff + W, T))) return rc;
    if (T > nbytes) return fail(c, GZ_E_HIP, "internal: segment counted %lld tokens in %lld bytes", (long long)T, (long long)nbytes);
    S.n_tokens = O.n_tokens = T;
    const size_t t1 = (size_t)T + 1;
    if ((rc = bm_alloc(c, g[SGW_TSTART], t1 * 4)) || (rc = bm_alloc(c, g[SGW_TLEN], t1 * 4)) || (rc = bm_alloc(c, g[SGW_TDOC], t1 * 4)) ||
        (rc = bm_alloc(c, g[SGW_TLSUM], (t1 + 1) * 4)) || (rc = bm_alloc(c, g[SGW_DOCLEN], (size_t)N * 8)))
        return rc;
    if (!O.stats) {
        if ((rc = bm_alloc(c, g[SGW_STATS], (size_t)N * 32))) return rc;
        O.stats = (int64_t*)g[SGW_STATS].p;
    }
    S.tstart = (uint32_t*)g[SGW_TSTART].p; S.tlen = (uint32_t*)g[SGW_TLEN].p; S.tdoc = (uint32_t*)g[SGW_TDOC].p; S.tlsum = (const uint32_t*)g[SGW_TLSUM].p;
    S.doclen = (int64_t*)g[SGW_DOCLEN].p; S.out_off = O.out_off; S.stats = (unsigned long long*)O.stats;
    gz_launch_segment(GZ_SEG_TOKENS, S, false, s);
    if ((rc = bm_scan(c, S.tlen, T, (uint32_t*)g[SGW_TLSUM].p))) return rc;
    // ---- the output's offsets follow from the token counts and lengths alone: sized here, before any lexicon work
    gz_launch_segment(GZ_SEG_DOCS, S, false, s);
    gz_launch_scan64(S.doclen, N, O.out_off, s);
    if ((rc = read_total(c, O.out_off + N, nullptr, total))) return rc;
    if (!O.out) return GZ_OK;
    if (*total > O.capacity) return fail(c, GZ_E_CAPACITY, "segment output needs %lld bytes, capacity is %lld", (long long)*total, (long long)O.capacity);
    for (int64_t& v : lex->last) v = 0;
    lex->last[0] = N; lex->last[1] = T;
    if (T == 0) { HIPCHK(c, hipGetLastError()); return GZ_OK; }
    // ---- candidates, stretches and the walk, the text
    if ((rc = bm_alloc(c, g[SGW_CAND], (size_t)T * (size_t)lex->K * 4)) || (rc = bm_alloc(c, g[SGW_REACH], (size_t)T)) || (rc = bm_alloc(c, g[SGW_CLOSED], (size_t)T)) ||
        (rc = bm_alloc(c, g[SGW_STARTS], (size_t)T * 4)) || (rc = bm_alloc(c, g[SGW_CTL], 64)) || (rc = bm_alloc(c, g[SGW_CHOICE], (size_t)T)))
        return rc;
    if (!O.join) {
        if ((rc = bm_alloc(c, g[SGW_JOIN], (size_t)T))) return rc;
        O.join = (uint8_t*)g[SGW_JOIN].p;
    }
    if (!O.tok_off && O.want_tok) {
        if ((rc = bm_alloc(c, g[SGW_TOKOFF], (size_t)T * 8))) return rc;
        O.tok_off = (int64_t*)g[SGW_TOKOFF].p;
    }
    S.tab = (const GzSegSlot*)lex->tab.p; S.tmask = lex->tmask; S.hmask = lex->hmask; S.ebytes = (const uint8_t*)lex->ebytes.p;
    S.filter = (const uint32_t*)lex->filter.p; S.max_len = lex->max_len;
    S.cand = (uint32_t*)g[SGW_CAND].p; S.reach = (uint8_t*)g[SGW_REACH].p; S.closed = (uint8_t*)g[SGW_CLOSED].p; S.starts = (uint32_t*)g[SGW_STARTS].p;
    S.ctl = (uint32_t*)g[SGW_CTL].p; S.choice = (uint8_t*)g[SGW_CHOICE].p; S.join = O.join; S.out = O.out; S.tok_off = O.tok_off;
    HIPCHK(c, hipMemsetAsync(S.ctl, 0, 64, s));
    HIPCHK(c, hipEventRecord(lex->ev[1], s));
    gz_launch_segment(GZ_SEG_CAND, S, c->opt.seg_lds != 0, s);
    HIPCHK(c, hipEventRecord(lex->ev[2], s));
    gz_launch_segment(GZ_SEG_MARK, S, false, s);
    gz_launch_segment(GZ_SEG_WALK, S, false, s);
    HIPCHK(c, hipEventRecord(lex->ev[3], s));
    gz_launch_segment(GZ_SEG_EMIT, S, false, s);
    HIPCHK(c, hipEventRecord(lex->ev[4], s));
    uint32_t ctl[8] = {};
    if ((rc = copy_out_small(c, ctl, S.ctl, sizeof ctl, s))) return rc;       // (waits for the stream)
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < 5; ++i) lex->last[2 + i] = ctl[i];
    for (int i = 0; i < 4; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, lex->ev[i], lex->ev[i + 1]) == hipSuccess) lex->last[7 + i] = (int64_t)((double)ms * 1e6);
    }
    return GZ_OK;
}

// the rules of a segment call that need no device; c not null
int segment_rule(gz_ctx* c, gz_lexicon* lex, int64_t n_docs, uint32_t flags, int64_t unk_cost, int64_t capacity, const void* out_off)
{
    if (!lex_live(c, lex)) return fail(c, GZ_E_INVALID, "%s", kLexHandle);
    if (n_docs < 0) return fail(c, GZ_E_INVALID, "segment: n_docs is negative");
    if (flags & ~(uint32_t)GZ_SEG_SPLIT_PUNCT) return fail(c, GZ_E_INVALID, "segment: unknown flags 0x%x", flags);
    if (unk_cost < 1 || unk_cost >= (int64_t)GZ_SEG_COST_LIMIT) return fail(c, GZ_E_INVALID, "segment: unk_cost %lld is outside [1, 2^24)", (long long)unk_cost);
    if (capacity < 0) return fail(c, GZ_E_INVALID, "segment: capacity is negative");
    if (!out_off) return fail(c, GZ_E_INVALID, "segment needs out_off[n_docs + 1]");
    return GZ_OK;
}

// word indices, token indices and the 32-bit scans of the front
int segment_limits(gz_ctx* c, int64_t nbytes, int64_t n_docs)
{
    if (nbytes + n_docs >= ((int64_t)1 << 31))
        return fail(c, GZ_E_LIMIT, "segment: %lld bytes + %lld documents; a call takes fewer than 2^31: split the batch", (long long)nbytes, (long long)n_docs);
    return GZ_OK;
}
}  // namespace

extern "C" {

int gz_lexicon_create(gz_ctx* c, const uint8_t* words, const int64_t* word_off, const int32_t* costs, int64_t n, int32_t max_syllables, uint32_t flags,
                      gz_lexicon** out)
try {
    if (!c) return GZ_E_INVALID;
    if (!out) return fail(c, GZ_E_INVALID, "a lexicon needs an out handle");
    *out = nullptr;
    if (max_syllables < 1 || max_syllables > GZ_SEG_MAX_SYLLABLES) return fail(c, GZ_E_INVALID, "lexicon: max_syllables %d is outside 1..%d", max_syllables, GZ_SEG_MAX_SYLLABLES);
    if (flags & ~(uint32_t)GZ_LEX_FOLD_CASE) return fail(c, GZ_E_INVALID, "lexicon: unknown flags 0x%x", flags);
    if (n < 0 || n >= ((int64_t)1 << 30) || !word_off || (n > 0 && (!words || !costs))) return fail(c, GZ_E_INVALID, "lexicon: bad arguments");
    if (word_off[n] - word_off[0] >= ((int64_t)1 << 32)) return fail(c, GZ_E_LIMIT, "lexicon: the entries take 2^32 bytes or more");
    const bool fold = (flags & GZ_LEX_FOLD_CASE) != 0;
    const unsigned long long hmask = c->opt.seg_hash_bits > 0 ? (1ull << c->opt.seg_hash_bits) - 1ull : ~0ull >> 1;
    alloc_site(c);
    // ---- the host's half: every entry checked, folded, hashed and placed
    const uint64_t slots = bm_pow2(2 * (uint64_t)n + 16);                  // load <= 1/2: a probe always meets an empty slot
    std::vector<GzSegSlot> tab((size_t)slots, GzSegSlot{0ull, 0u, 0u, 0u, 0u});
    std::vector<uint32_t> filter((size_t)1 << (GZ_SEG_FILTER_BITS - 5), 0u);
    std::vector<uint8_t> arena;
    arena.reserve((size_t)(word_off[n] - word_off[0]) + 16);
    uint32_t max_len = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = word_off[i + 1] - word_off[i];
        if (len < 0) return fail(c, GZ_E_INVALID, "lexicon: the offsets decrease at entry %lld", (long long)i);
        const uint8_t* const p = words + word_off[i];
        if (len == 0) return fail(c, GZ_E_INVALID, "lexicon: entry %lld is empty", (long long)i);
        if (!gz_is_plain_word(p, (size_t)len)) return fail(c, GZ_E_INVALID, "lexicon: %s holds whitespace or is not UTF-8", lex_name(p, len, i));
        int syll = 1;
        for (int64_t b = 0; b < len; ++b) syll += p[b] == '_';
        if (syll > max_syllables) return fail(c, GZ_E_INVALID, "lexicon: %s has %d syllables, max_syllables is %d", lex_name(p, len, i), syll, max_syllables);
        if (costs[i] < 1 || costs[i] >= (int32_t)GZ_SEG_COST_LIMIT) return fail(c, GZ_E_INVALID, "lexicon: cost %d of %s is outside [1, 2^24)", costs[i], lex_name(p, len, i));
        const uint32_t at = (uint32_t)arena.size();
        unsigned long long h = GZ_SEG_HASH_SEED;
        uint32_t p1 = 0u, p2 = 0u;
        for (int64_t b = 0; b < len; ++b) {
            const uint32_t f = fold ? gz_seg_fold(p2, p1, p[b]) : p[b];
            arena.push_back((uint8_t)f);
            h = gz_seg_hash_byte(h, f);
            p2 = p1; p1 = p[b];
        }
        const unsigned long long hk = gz_seg_hash_fin(h, (uint32_t)len) & hmask, key = hk | (1ull << 63);
        unsigned long long slot = gz_seg_slot(hk) & (slots - 1);
        for (; tab[(size_t)slot].key; slot = (slot + 1) & (slots - 1)) {
            const GzSegSlot& e = tab[(size_t)slot];
            if (e.key == key && e.len == (uint32_t)len && std::memcmp(arena.data() + e.off, arena.data() + at, (size_t)len) == 0)
                return fail(c, GZ_E_INVALID, "lexicon: %s is given twice%s", lex_name(p, len, i), fold ? " (after case folding)" : "");
        }
        tab[(size_t)slot] = GzSegSlot{key, (uint32_t)costs[i], (uint32_t)len, at, 0u};
        const uint32_t bit = (uint32_t)hk & ((1u << GZ_SEG_FILTER_BITS) - 1u);
        filter[bit >> 5] |= 1u << (bit & 31u);
        if ((uint32_t)len > max_len) max_len = (uint32_t)len;
    }
    // ---- the device's half
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::unique_ptr<gz_lexicon> lex(new gz_lexicon());
    lex->c = c; lex->n = n; lex->n_bytes = (int64_t)arena.size(); lex->K = max_syllables; lex->flags = (int32_t)flags; lex->max_len = max_len;
    lex->hmask = hmask; lex->tmask = slots - 1;
    int rc;
    if ((rc = bm_alloc(c, lex->tab, (size_t)slots * sizeof(GzSegSlot))) || (rc = bm_alloc(c, lex->ebytes, arena.size() + 16)) ||
        (rc = bm_alloc(c, lex->filter, filter.size() * 4)))
        return rc;
    BmDrain drain{c};                                                  // (an error below frees the lexicon: not under a copy in flight)
    if ((rc = copy_in(c, lex->tab.p, tab.data(), (size_t)slots * sizeof(GzSegSlot), c->stream)) ||
        (rc = copy_in(c, lex->ebytes.p, arena.data(), arena.size(), c->stream)) || (rc = copy_in(c, lex->filter.p, filter.data(), filter.size() * 4, c->stream)))
        return rc;
    for (hipEvent_t& e : lex->ev) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    alloc_site(c);
    c->lex_live.push_back(lex.get());
    *out = lex.release();
    return GZ_OK;
} GZ_CATCH(c)

void gz_lexicon_destroy(gz_lexicon* lex)
try {
    if (!lex) return;
    gz_ctx* c = lex->c;
    std::lock_guard<std::mutex> lk(c->mu);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    auto& v = c->lex_live;
    v.erase(std::remove(v.begin(), v.end(), lex), v.end());
    delete lex;
} GZ_CATCH_VOID

int gz_lexicon_info(gz_ctx* c, gz_lexicon* lex, int64_t info[24])
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!lex_live(c, lex)) return fail(c, GZ_E_INVALID, "%s", kLexHandle);
    if (!info) return fail(c, GZ_E_INVALID, "lexicon info needs info[24]");
    const int64_t v[12] = {lex->n, lex->K, lex->flags, lex->n_bytes, (int64_t)lex->tmask + 1, lex->device_bytes(), (int64_t)lex->max_len,
                           c->opt.seg_lds ? 1 : 0, GZ_SEG_TILE, 64, 0, 0};
    for (int i = 0; i < 12; ++i) { info[i] = v[i]; info[12 + i] = lex->last[i]; }
    return GZ_OK;
} GZ_CATCH(c)

int gz_segment_batch_device(gz_ctx* c, gz_lexicon* lex, const uint8_t* text_dev, const int64_t* text_off_dev, int64_t n_docs, uint32_t flags, int64_t unk_cost,
                            uint8_t* out_dev, int64_t capacity, int64_t* out_off_dev, int64_t* stats_dev, uint8_t* join_dev, int64_t* tok_off_dev,
                            int64_t* total_host)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the lexicon is looked at, and held to the end)
    int rc;
    if ((rc = segment_rule(c, lex, n_docs, flags, unk_cost, capacity, out_off_dev))) return rc;
    if (!total_host) return fail(c, GZ_E_INVALID, "segment needs total_host");
    if (!text_off_dev) return fail(c, GZ_E_INVALID, "segment needs text_off");
    *total_host = 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_docs == 0) {
        HIPCHK(c, hipMemsetAsync(out_off_dev, 0, 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return GZ_OK;
    }
    int64_t off0 = 0, nbytes = 0;
    if ((rc = rows_extent_device(c, text_off_dev, n_docs, &off0, &nbytes))) return rc;
    if (off0 < 0) return fail(c, GZ_E_INVALID, "negative text offset");
    if (nbytes > 0 && !text_dev) return fail(c, GZ_E_INVALID, "segment needs text");
    if ((rc = segment_limits(c, nbytes, n_docs))) return rc;
    SegOut O{out_dev, capacity, out_off_dev, stats_dev, join_dev, tok_off_dev, false, 0};
    return segment_core(c, lex, text_dev, text_off_dev, n_docs, off0, nbytes, flags, (uint32_t)unk_cost, O, total_host);
} GZ_CATCH(c)

int gz_segment_batch(gz_ctx* c, gz_lexicon* lex, const uint8_t* text, const int64_t* text_off, int64_t n_docs, uint32_t flags, int64_t unk_cost, uint8_t* out,
                     int64_t capacity, int64_t* out_off, int64_t* stats, uint8_t* join, int64_t* tok_off)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);                       // (before the lexicon is looked at, and held to the end)
    int rc;
    if ((rc = segment_rule(c, lex, n_docs, flags, unk_cost, capacity, out_off))) return rc;
    if (!text_off) return fail(c, GZ_E_INVALID, "segment needs text_off");
    if (n_docs == 0) { out_off[0] = 0; return GZ_OK; }
    RowsIn in{text, text_off, n_docs, 1};
    if ((rc = rows_check(c, in, kTextWords))) return rc;
    const int64_t nbytes = in.n;
    if ((rc = segment_limits(c, nbytes, n_docs))) return rc;
    if ((rc = rows_stage(c, in, (size_t)(n_docs + 1) * 8))) return rc;
    // the text on the device: never longer than the input, or than twice the input where punctuation is split off
    const int64_t bound = (flags & GZ_SEG_SPLIT_PUNCT) ? 2 * nbytes : nbytes;
    DBuf* g = c->w_seg;
    if (out && (rc = bm_alloc(c, g[SGW_OUT], (size_t)bound + 16))) return rc;
    SegOut O{out ? (uint8_t*)g[SGW_OUT].p : nullptr, bound, (int64_t*)in.d_keep, nullptr, nullptr, nullptr, tok_off != nullptr, 0};
    int64_t total = 0;
    if ((rc = segment_core(c, lex, (const uint8_t*)in.d_payload, in.d_off, n_docs, text_off[0], nbytes, flags, (uint32_t)unk_cost, O, &total))) return rc;
    HostPool pool(pool_threads(c, (size_t)total));
    if ((rc = copy_out(c, out_off, O.out_off, (size_t)(n_docs + 1) * 8, c->stream, &pool))) return rc;
    if (stats && (rc = copy_out(c, stats, O.stats, (size_t)n_docs * 32, c->stream, &pool))) return rc;
    if (!out) return GZ_OK;                                      // (sized: the offsets and every n_tokens are there)
    if (total > capacity) return fail(c, GZ_E_CAPACITY, "segment output needs %lld bytes, capacity is %lld", (long long)total, (long long)capacity);
    const size_t T = (size_t)O.n_tokens;
    if (join && T && (rc = copy_out(c, join, O.join, T, c->stream, &pool))) return rc;
    if (tok_off && T && (rc = copy_out(c, tok_off, O.tok_off, T * 8, c->stream, &pool))) return rc;
    if (total && (rc = copy_out(c, out, O.out, (size_t)total, c->stream, &pool))) return rc;
    return GZ_OK;
} GZ_CATCH(c)

}  // extern "C"
