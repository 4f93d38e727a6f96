// The row-shaping calls behind the C ABI: batch decode, overlapping windows, packed rows, masked-LM rows, span-corruption rows,
// MinHash signatures and groups; and what the n-gram calls (gz_ngram_api.inc, gz_repeat_api.inc) share with them: the piece count and the
// extent of a device input.
// Included by gz_api.cpp behind gz_ctx, fail, HIPCHK, ensure and the copy helpers; the kernels are in gz_decode.inc, gz_window.inc,
// gz_packrows.inc, gz_mask.inc, gz_infill.inc, gz_pieces.inc and gz_minhash.inc.  A call supplies its rule, its launch and its list of outputs; the row front
// below does the rest of a host form (DESIGN.md, "the row front"); its rules without HIP in them are in gz_rowrules.h.
// WORKSPACE: the host forms share w_rows_in, w_rows_off, w_rows_out[4] and w_rows_small, and the calls that divide rows into pieces
// (MinHash signatures, the n-gram index and its queries, n-gram repeats; host and device forms) share w_pieces.  That is sound
// because every use lies inside c->mu and every access -- copy, kernel, memset -- is enqueued on c->stream: a later call's accesses
// are ordered behind an earlier call's even where that one returned early.  A kernel's own scratch (w_win_cnt, the w_pk_* maps,
// w_dec_rb, the MinHash band table and EMPTY bytes, the n-gram and repeat tables) is not shared.

// ---- the row front -----------------------------------------------------------------------------------------------------
namespace {
// the wording of a CSR input's two refusals
struct RowsWords { const char* bad; const char* decrease; };
constexpr RowsWords kRowWords{"bad row offsets", "row offsets must not decrease"};
constexpr RowsWords kTextWords{"bad text offsets", "text offsets must not decrease"};

// A host CSR input (gz_rowrules.h) of `elem`-byte elements.  Two halves, because a refusal of the offsets comes before
// GZ_E_NOTABLES and so before the lock: rows_check validates and sets n; rows_stage, under c->mu, copies payload and offsets in and
// sets the device pointers -- d_payload is biased by off[0], so the absolute offsets index it as they index the caller's array --
// and d_keep, `keep_bytes` of the offsets buffer that are the call's own (its output offsets: they live through both passes).
struct RowsIn {
    const void* payload; const int64_t* off; int64_t n_rows; size_t elem;
    int64_t n = 0;
    const void* d_payload = nullptr; const int64_t* d_off = nullptr; void* d_keep = nullptr;
};
int rows_check(gz_ctx* c, RowsIn& in, const RowsWords& w)
{
    switch (rows_offsets_check(in.payload, in.off, in.n_rows, &in.n)) {
    case ROWS_BAD: return fail(c, GZ_E_INVALID, "%s", w.bad);
    case ROWS_DECREASE: return fail(c, GZ_E_INVALID, "%s", w.decrease);
    default: return GZ_OK;
    }
}
int rows_stage(gz_ctx* c, RowsIn& in, size_t keep_bytes)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)in.n * in.elem, off_bytes = (size_t)(in.n_rows + 1) * 8;
    int rc;
    if ((rc = ensure(c, c->w_rows_in, bytes + 16))) return rc;             // (slack: the pre-pass reads 16 bytes at a time)
    if ((rc = ensure(c, c->w_rows_off, off_bytes + keep_bytes))) return rc;
    if (bytes && (rc = copy_in(c, c->w_rows_in.p, (const uint8_t*)in.payload + in.off[0] * (int64_t)in.elem, bytes, c->stream))) return rc;
    if ((rc = copy_in(c, c->w_rows_off.p, in.off, off_bytes, c->stream))) return rc;
    in.d_payload = (const uint8_t*)c->w_rows_in.p - in.off[0] * (int64_t)in.elem;
    in.d_off = (const int64_t*)c->w_rows_off.p;
    in.d_keep = (uint8_t*)c->w_rows_off.p + off_bytes;
    return GZ_OK;
}

// The one scalar a two-pass call waits for: the int64 at `src` on the device after ONE hipStreamSynchronize of the context's stream.
// src == nullptr (an empty batch: no kernel wrote a total): 0, and the offsets word at `zero`, if given, is cleared in its place.
int read_total(gz_ctx* c, const int64_t* src, int64_t* zero, int64_t* total)
{
    *total = 0;
    int64_t* const h_total = &c->pin->read_total;
    *h_total = 0;
    if (src) HIPCHK(c, hipMemcpyAsync(h_total, src, 8, hipMemcpyDeviceToHost, c->stream));
    else if (zero) HIPCHK(c, hipMemsetAsync(zero, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *total = *h_total;
    return GZ_OK;
}

// The extent of a device CSR input of n_rows > 0 rows: *off0 = row_off[0], *n_ids = row_off[n_rows] - row_off[0], read from the device
// after one wait of the context's stream; a negative extent is refused.
int rows_extent_device(gz_ctx* c, const int64_t* row_off_dev, int64_t n_rows, int64_t* off0, int64_t* n_ids)
{
    int64_t* const h = c->pin->extent;
    h[0] = h[1] = 0;
    HIPCHK(c, hipMemcpyAsync(h, row_off_dev, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 1, row_off_dev + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *off0 = h[0];
    *n_ids = (int64_t)((uint64_t)h[1] - (uint64_t)h[0]);
    if (*n_ids < 0) return fail(c, GZ_E_INVALID, "bad row offsets");
    return GZ_OK;
}

// Rows divided into pieces (gz_pieces.inc; DESIGN.md, "the row front"): the count pass of the calls whose waves own a piece of a row's
// body -- MinHash signatures, the n-gram index and its queries, n-gram repeats.  w_pieces holds the counts, their scan, then the
// position total and the too-long flag: 16 bytes a row (plus 32).  ONE wait of the context's stream: piece_off (on the device, valid
// until the next count on this context), the pieces, the positions (0 unless want_pos), or GZ_E_LIMIT when a body holds 2^31 ids or
// more -- nothing was launched over the rows then.  rebased_dev: n_rows + 1 words for row_off - row_off[0], or null.  n_rows > 0.
const char* const kBodyLimit = "a row's body holds 2^31 ids or more: split the document";
struct Pieces { const int64_t* piece_off; int64_t n_pieces, n_pos; };
int pieces_count_locked(gz_ctx* c, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t w, GzPieceRule rule,
                        bool want_pos, int64_t* rebased_dev, Pieces* out)
{
    int rc;
    const size_t words = (size_t)n_rows + 1;
    if ((rc = ensure(c, c->w_pieces, words * 16 + sizeof(GzPieceTotals)))) return rc;
    int64_t* const cnt = (int64_t*)c->w_pieces.p;
    int64_t* const piece_off = cnt + words;
    GzPieceTotals* const totals = (GzPieceTotals*)(piece_off + words);
    gz_launch_piece_count(rule, row_off_dev, n_rows, skip_front, skip_back, w, cnt, piece_off, rebased_dev, want_pos, totals, c->stream);
    GzPinned* const h = c->pin;
    h->n_pieces = 0;
    h->pieces = GzPieceTotals{};
    HIPCHK(c, hipMemcpyAsync(&h->n_pieces, piece_off + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h->pieces, totals, sizeof *totals, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h->pieces.too_long) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    *out = Pieces{piece_off, h->n_pieces, (int64_t)h->pieces.n_pos};
    return GZ_OK;
}

// The outputs of a host form, in the order they are copied out.  staged_ensure gives every entry the caller wants (host != null) a
// place in the workspace -- the k-th large one w_rows_out[k], the small ones pieces of w_rows_small, 256 bytes apart at the least -- and leaves
// dev null for the others; staged_copy_out brings them back: the large ones under one HostPool sized by the largest, then the small
// ones on the caller's thread, then the check for a failed launch.
struct StagedOut {
    struct Entry { void* host; size_t bytes; bool large; void* dev; };
    Entry e[12];
    int n = 0;
    void add(void* host, size_t bytes, bool large) { e[n++] = Entry{host, bytes, large, nullptr}; }
    int32_t* dev(int k) const { return (int32_t*)e[k].dev; }
};
int staged_ensure(gz_ctx* c, StagedOut& S)
{
    int rc, k_large = 0;
    size_t small = 0;
    for (int k = 0; k < S.n; ++k) {
        StagedOut::Entry& E = S.e[k];
        if (!E.host) continue;
        if (E.large) {
            if ((rc = ensure(c, c->w_rows_out[k_large], E.bytes))) return rc;
            E.dev = c->w_rows_out[k_large++].p;
        } else small += (E.bytes + 255) & ~(size_t)255;
    }
    if (!small) return GZ_OK;
    if ((rc = ensure(c, c->w_rows_small, small))) return rc;
    uint8_t* at = (uint8_t*)c->w_rows_small.p;
    for (int k = 0; k < S.n; ++k)
        if (S.e[k].host && !S.e[k].large) { S.e[k].dev = at; at += (S.e[k].bytes + 255) & ~(size_t)255; }
    return GZ_OK;
}
int staged_copy_out(gz_ctx* c, const StagedOut& S)
{
    int rc;
    size_t largest = 0;
    for (int k = 0; k < S.n; ++k) if (S.e[k].dev && S.e[k].large && S.e[k].bytes > largest) largest = S.e[k].bytes;
    {
        HostPool pool(pool_threads(c, largest));
        for (int k = 0; k < S.n; ++k)
            if (S.e[k].dev && S.e[k].large && (rc = copy_out(c, S.e[k].host, S.e[k].dev, S.e[k].bytes, c->stream, &pool))) return rc;
    }
    for (int k = 0; k < S.n; ++k)
        if (S.e[k].dev && !S.e[k].large && (rc = copy_out(c, S.e[k].host, S.e[k].dev, S.e[k].bytes, c->stream))) return rc;
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}
}  // namespace

// ---- batch decode ----------------------------------------------------------------------------------------------------
namespace {
constexpr size_t GZ_DEC_UNK_MAX = 4096;

uint32_t dec_flags(const std::string& w)
{
    uint32_t f = (uint32_t)w.size();
    if (w.size() >= 2 && w[w.size() - 1] == '@' && w[w.size() - 2] == '@') f |= GZ_DEC_ENDS_ATAT;
    if (w.find("@@ ") != std::string::npos) f |= GZ_DEC_INNER;
    return f;
}

// the table entry of a word whose bytes are (or would be) at `off` of the byte arena
GzDecEntry dec_entry_of(const std::string& w, size_t off)
{
    GzDecEntry e{dec_flags(w), {(uint32_t)off, 0u, 0u}};
    if (w.size() <= 12 && !(e.len_flags & GZ_DEC_INNER)) {
        e.len_flags |= GZ_DEC_INLINE;
        e.w[0] = 0;
        for (size_t k = 0; k < w.size(); ++k) e.w[k >> 2] |= (uint32_t)(uint8_t)w[k] << (8 * (k & 3));
    }
    return e;
}

int dec_set_unk(gz_ctx* c, const uint8_t* unk, int32_t unk_len)
{
    if (unk_len < 0 || (size_t)unk_len > GZ_DEC_UNK_MAX) return fail(c, GZ_E_LIMIT, "unk string longer than %zu bytes", GZ_DEC_UNK_MAX);
    const std::string u((const char*)unk, (size_t)unk_len);
    if (c->dec_unk_set && u == c->dec_unk) return GZ_OK;
    int rcs;
    if (unk_len && (rcs = copy_in(c, (uint8_t*)c->t_dec_bytes.p + c->dec_bytes_len, unk, (size_t)unk_len, c->stream))) return rcs;
    const GzDecEntry e = dec_entry_of(u, c->dec_bytes_len);
    if ((rcs = copy_in(c, (GzDecEntry*)c->t_dec_entries.p + c->dec_n_ids, &e, sizeof e, c->stream))) return rcs;
    c->dec_unk = u;
    c->dec_unk_set = true;
    return GZ_OK;
}

// both passes; *total = bytes of the whole batch.  out_dev may be nullptr (sizes only).
int decode_device_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, const uint8_t* unk,
                         int32_t unk_len, uint8_t* out_dev, int64_t capacity, int64_t* out_off_dev, int64_t* total)
{
    if (!c->have_dec) return fail(c, GZ_E_NOTABLES, "gz_decoder_snapshot has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = dec_set_unk(c, unk, unk_len))) return rc;
    if ((rc = ensure(c, c->w_dec_rb, (size_t)(n_rows + 1) * 8))) return rc;
    GzDecTable D{(const GzDecEntry*)c->t_dec_entries.p, (const uint8_t*)c->t_dec_bytes.p, c->dec_n_ids};
    gz_launch_decode(D, ids_dev, row_off_dev, n_rows, (int64_t*)c->w_dec_rb.p, out_off_dev, nullptr, 0, c->stream);
    if ((rc = read_total(c, n_rows > 0 ? out_off_dev + n_rows : nullptr, out_off_dev, total))) return rc;
    if (!out_dev) return GZ_OK;
    if (*total > capacity) return fail(c, GZ_E_CAPACITY, "decode needs %lld bytes, capacity is %lld", (long long)*total, (long long)capacity);
    gz_launch_decode(D, ids_dev, row_off_dev, n_rows, nullptr, out_off_dev, out_dev, capacity, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}
}  // namespace

int gz_decoder_snapshot(gz_ctx* c)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_tables) return fail(c, GZ_E_NOTABLES, "gz_load_tables has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    // {v: k for k, v in encoder.items()} (tokenize.py:40): the last word wins on an id collision
    int32_t n_ids = 0;
    for (int32_t id : c->host.enc_ids) if (id + 1 > n_ids) n_ids = id + 1;
    std::vector<int64_t> last((size_t)n_ids, -1);
    for (size_t i = 0; i < c->host.enc_ids.size(); ++i) if (c->host.enc_ids[i] >= 0) last[(size_t)c->host.enc_ids[i]] = (int64_t)i;
    std::vector<GzDecEntry> ent((size_t)n_ids + 1, GzDecEntry{GZ_DEC_ABSENT, {0u, 0u, 0u}});
    std::string bytes;
    for (int32_t id = 0; id < n_ids; ++id) {
        if (last[(size_t)id] < 0) continue;
        const std::string& w = c->host.enc_words[(size_t)last[(size_t)id]];
        if (w.size() > GZ_DEC_LEN_MASK || bytes.size() + w.size() > 0xFFFF0000ull) return fail(c, GZ_E_LIMIT, "vocabulary too large for the decoder arena");
        ent[(size_t)id] = dec_entry_of(w, bytes.size());
        bytes += w;
    }
    ent[(size_t)n_ids] = GzDecEntry{GZ_DEC_INLINE, {0u, 0u, 0u}};                  // (the unk string: set per call, dec_set_unk)
    std::vector<uint32_t> cont((size_t)n_ids / 32 + 1, 0u);                       // which ids continue a word: one bit each (gz_mask_rows*)
    for (int32_t id = 0; id < n_ids; ++id)
        if (ent[(size_t)id].len_flags != GZ_DEC_ABSENT && (ent[(size_t)id].len_flags & GZ_DEC_ENDS_ATAT)) cont[(size_t)id >> 5] |= 1u << (id & 31);
    int rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = ensure(c, c->t_dec_entries, ent.size() * sizeof(GzDecEntry)))) return rc;
    if ((rc = ensure(c, c->t_dec_bytes, bytes.size() + GZ_DEC_UNK_MAX + 16))) return rc;
    if ((rc = ensure(c, c->t_dec_cont, cont.size() * 4))) return rc;
    if ((rc = copy_in(c, c->t_dec_entries.p, ent.data(), ent.size() * sizeof(GzDecEntry), c->stream))) return rc;
    if ((rc = copy_in(c, c->t_dec_cont.p, cont.data(), cont.size() * 4, c->stream))) return rc;
    if (!bytes.empty() && (rc = copy_in(c, c->t_dec_bytes.p, bytes.data(), bytes.size(), c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dec_n_ids = n_ids;
    c->dec_bytes_len = bytes.size();
    c->dec_unk_set = false;
    c->have_dec = true;
    return GZ_OK;
} GZ_CATCH(c)

int gz_decode_batch_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, const uint8_t* unk,
                           int32_t unk_len, uint8_t* out_dev, int64_t capacity, int64_t* out_off_dev, int64_t* total_host)
try {
    if (!c || !row_off_dev || !out_off_dev || !total_host || n_rows < 0 || (!unk && unk_len) || capacity < 0)
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    return decode_device_locked(c, ids_dev, row_off_dev, n_rows, unk, unk_len, out_dev, capacity, out_off_dev, total_host);
} GZ_CATCH(c)

int gz_decode_batch(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, const uint8_t* unk, int32_t unk_len,
                    uint8_t* out, int64_t capacity, int64_t* out_off)
try {
    if (!c || !row_off || !out_off || n_rows < 0 || (!unk && unk_len) || capacity < 0 || (capacity > 0 && !out))
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, (size_t)(n_rows + 1) * 8))) return rc;
    const int32_t* const ids_dev = (const int32_t*)in.d_payload;
    int64_t* const ooff = (int64_t*)in.d_keep;
    int64_t total = 0;
    if ((rc = decode_device_locked(c, ids_dev, in.d_off, n_rows, unk, unk_len, nullptr, 0, ooff, &total))) return rc;
    if ((rc = copy_out(c, out_off, ooff, (size_t)(n_rows + 1) * 8, c->stream))) return rc;
    if (total > capacity) return fail(c, GZ_E_CAPACITY, "decode needs %lld bytes, capacity is %lld", (long long)total, (long long)capacity);
    if (total == 0) return GZ_OK;
    StagedOut S;
    S.add(out, (size_t)total, true);
    if ((rc = staged_ensure(c, S))) return rc;
    GzDecTable D{(const GzDecEntry*)c->t_dec_entries.p, (const uint8_t*)c->t_dec_bytes.p, c->dec_n_ids};
    gz_launch_decode(D, ids_dev, in.d_off, n_rows, nullptr, ooff, (uint8_t*)S.e[0].dev, total, c->stream);
    return staged_copy_out(c, S);
} GZ_CATCH(c)

// ---- overlapping max_len windows ------------------------------------------------------------------------------------
namespace {
// the fill pass over win_off, enqueued on the context's stream; bos / eos / pad are the context's current special ids
void window_fill(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t max_len, int32_t stride, int32_t skip_front,
                 int32_t skip_back, const int64_t* win_off_dev, int64_t n_win, int32_t* out_ids, int32_t* out_mask, int32_t* win_doc,
                 int32_t* win_start, int32_t* win_n_real)
{
    GzWinArgs A{ids_dev, row_off_dev, n_rows, win_off_dev, n_win, max_len, max_len - 2, max_len - 2 - stride, skip_front, skip_back,
                c->dev.bos_id, c->dev.eos_id, c->dev.pad_id, out_ids, out_mask, win_doc, win_start, win_n_real};
    gz_launch_window_fill(A, c->stream);
}

// Both passes on the context's stream, behind whatever it holds (an encode call's forked streams have rejoined it when that call
// returns).  *total = windows of the batch.  out_ids == nullptr: the count pass only.
int window_device_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t max_len, int32_t stride,
                         int32_t skip_front, int32_t skip_back, int32_t* out_ids, int32_t* out_mask, int32_t* win_doc, int32_t* win_start,
                         int32_t* win_n_real, int64_t* win_off_dev, int64_t capacity, int64_t* total)
{
    if (!c->have_tables) return fail(c, GZ_E_NOTABLES, "gz_load_tables has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->w_win_cnt, (size_t)(n_rows + 1) * 8))) return rc;
    const int32_t room = max_len - 2, step = room - stride;
    gz_launch_window_count(row_off_dev, n_rows, room, step, skip_front + skip_back, (int64_t*)c->w_win_cnt.p, win_off_dev, c->stream);
    if ((rc = read_total(c, n_rows > 0 ? win_off_dev + n_rows : nullptr, win_off_dev, total))) return rc;
    if (!out_ids) return GZ_OK;
    if (*total > capacity) return fail(c, GZ_E_CAPACITY, "the batch makes %lld windows, capacity is %lld", (long long)*total, (long long)capacity);
    window_fill(c, ids_dev, row_off_dev, n_rows, max_len, stride, skip_front, skip_back, win_off_dev, *total, out_ids, out_mask, win_doc, win_start,
                win_n_real);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}

bool window_rule_ok(int32_t max_len, int32_t stride, int32_t skip_front, int32_t skip_back)
{
    return max_len >= 3 && stride >= 0 && stride <= max_len - 3 && skip_front >= 0 && skip_back >= 0 && skip_front <= 1 && skip_back <= 1;
}
}  // namespace

int gz_window_rows_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t max_len, int32_t stride,
                          int32_t skip_front, int32_t skip_back, int32_t* input_ids_dev, int32_t* attention_mask_dev, int32_t* win_doc_dev,
                          int32_t* win_start_dev, int32_t* win_n_real_dev, int64_t* win_off_dev, int64_t capacity_windows, int64_t* total_host)
try {
    if (!c || !row_off_dev || !win_off_dev || !total_host || n_rows < 0 || capacity_windows < 0)
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    if (!window_rule_ok(max_len, stride, skip_front, skip_back))
        return fail(c, GZ_E_INVALID, "windows need max_len >= 3, 0 <= stride <= max_len - 3 and skips of 0 or 1");
    std::lock_guard<std::mutex> lk(c->mu);
    return window_device_locked(c, ids_dev, row_off_dev, n_rows, max_len, stride, skip_front, skip_back, input_ids_dev, attention_mask_dev,
                                win_doc_dev, win_start_dev, win_n_real_dev, win_off_dev, capacity_windows, total_host);
} GZ_CATCH(c)

int gz_window_rows(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t max_len, int32_t stride, int32_t skip_front,
                   int32_t skip_back, int32_t* input_ids, int32_t* attention_mask, int32_t* win_doc, int32_t* win_start, int32_t* win_n_real,
                   int64_t* win_off, int64_t capacity_windows, int64_t* total_host)
try {
    if (!c || !row_off || !win_off || !total_host || n_rows < 0 || capacity_windows < 0)
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    if (!window_rule_ok(max_len, stride, skip_front, skip_back))
        return fail(c, GZ_E_INVALID, "windows need max_len >= 3, 0 <= stride <= max_len - 3 and skips of 0 or 1");
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, (size_t)(n_rows + 1) * 8))) return rc;
    const int32_t* const ids_dev = (const int32_t*)in.d_payload;
    int64_t* const woff = (int64_t*)in.d_keep;
    int64_t total = 0;
    if ((rc = window_device_locked(c, ids_dev, in.d_off, n_rows, max_len, stride, skip_front, skip_back, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   woff, 0, &total))) return rc;
    *total_host = total;
    if ((rc = copy_out(c, win_off, woff, (size_t)(n_rows + 1) * 8, c->stream))) return rc;
    if (!input_ids) return GZ_OK;
    if (total > capacity_windows)
        return fail(c, GZ_E_CAPACITY, "the batch makes %lld windows, capacity is %lld", (long long)total, (long long)capacity_windows);
    if (total == 0) return GZ_OK;
    const size_t cells = (size_t)total * (size_t)max_len * 4, per_win = (size_t)total * 4;
    StagedOut S;
    S.add(input_ids, cells, true); S.add(attention_mask, cells, true);
    S.add(win_doc, per_win, false); S.add(win_start, per_win, false); S.add(win_n_real, per_win, false);
    if ((rc = staged_ensure(c, S))) return rc;
    window_fill(c, ids_dev, in.d_off, n_rows, max_len, stride, skip_front, skip_back, woff, total, S.dev(0), S.dev(1), S.dev(2), S.dev(3), S.dev(4));
    return staged_copy_out(c, S);
} GZ_CATCH(c)

// ---- short documents packed into rows of max_len ------------------------------------------------------------------------
namespace {
// The maps of a batch on the context's stream, behind whatever it holds: doc_len, seg_off, the row heads in pack_off, doc_row, doc_col.
// A map the caller does not take lives in the context's workspace (pack_off is the caller's).  A gets the pointers the fill pass
// needs; *total = R, read back from the device.  fill: the fill pass goes right behind the maps -- it takes R from device memory,
// writes nothing when R exceeds A.capacity, and writes doc_col in place of the col pass -- so the host waits once, for everything.
int pack_maps_locked(gz_ctx* c, GzPackArgs& A, int64_t* total, bool fill)
{
    if (!c->have_tables) return fail(c, GZ_E_NOTABLES, "gz_load_tables has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = A.n_rows;
    int rc;
    if (!A.seg_off) { if ((rc = ensure(c, c->w_pk_seg, (size_t)(n + 1) * 8))) return rc; A.seg_off = (int64_t*)c->w_pk_seg.p; }
    if (!A.doc_row) { if ((rc = ensure(c, c->w_pk_drow, (size_t)(n + 1) * 4))) return rc; A.doc_row = (int32_t*)c->w_pk_drow.p; }
    if (!A.doc_col) { if ((rc = ensure(c, c->w_pk_dcol, (size_t)(n + 1) * 4))) return rc; A.doc_col = (int32_t*)c->w_pk_dcol.p; }
    const size_t tiles = (size_t)gz_pack_tiles(n), groups = (size_t)gz_pack_groups(n), K = (size_t)gz_pack_entries(A.max_len);
    if ((rc = ensure(c, c->w_pk_len, (size_t)(n + 1) * 8))) return rc;
    if ((rc = ensure(c, c->w_pk_jc, (size_t)(n + 1) * 8))) return rc;
    if ((rc = ensure(c, c->w_pk_nxt, (size_t)(n + 1) * 4))) return rc;
    if ((rc = ensure(c, c->w_pk_jc2, (groups * K + 1) * 8))) return rc;
    if ((rc = ensure(c, c->w_pk_tile, (tiles + 1) * 8))) return rc;
    A.len64 = (int64_t*)c->w_pk_len.p; A.jc = (int32_t*)c->w_pk_jc.p; A.nxt = (int32_t*)c->w_pk_nxt.p; A.jc2 = (int32_t*)c->w_pk_jc2.p; A.tile = (int32_t*)c->w_pk_tile.p;
    A.total = (int64_t*)c->w_pk_tile.p + tiles;
    A.bos_id = c->dev.bos_id; A.eos_id = c->dev.eos_id; A.pad_id = c->dev.pad_id;
    *total = 0;
    if (n > 0) {
        gz_launch_pack_maps(A, !fill, c->stream);
        if (fill) gz_launch_pack_fill(A, c->stream);
    } else HIPCHK(c, hipMemsetAsync(A.seg_off, 0, 8, c->stream));
    if ((rc = read_total(c, n > 0 ? A.total : nullptr, A.pack_off, total))) return rc;
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}

const char* const kPackRule = "packed rows need max_len >= 3, skips of 0 or 1 and fewer than 2^31 - 4096 documents";
bool pack_rule_ok(int64_t n_rows, int32_t max_len, int32_t skip_front, int32_t skip_back)
{
    return max_len >= 3 && skip_front >= 0 && skip_back >= 0 && skip_front <= 1 && skip_back <= 1 && n_rows < INT32_MAX - 4096;
}
}  // namespace

int gz_pack_rows_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t max_len, int32_t skip_front,
                        int32_t skip_back, int32_t* input_ids_dev, int32_t* attention_mask_dev, int32_t* segment_ids_dev, int32_t* position_ids_dev,
                        int32_t* doc_row_dev, int32_t* doc_col_dev, int32_t* doc_len_dev, int64_t* pack_off_dev, int64_t* seg_off_dev,
                        int64_t capacity_rows, int64_t* total_host)
try {
    if (!c || !row_off_dev || !pack_off_dev || !total_host || n_rows < 0 || capacity_rows < 0)
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    if (!pack_rule_ok(n_rows, max_len, skip_front, skip_back)) return fail(c, GZ_E_INVALID, "%s", kPackRule);
    std::lock_guard<std::mutex> lk(c->mu);
    GzPackArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.max_len = max_len; A.skip_front = skip_front; A.skip_back = skip_back;
    A.doc_row = doc_row_dev; A.doc_col = doc_col_dev; A.doc_len = doc_len_dev; A.pack_off = pack_off_dev; A.seg_off = seg_off_dev;
    A.capacity = capacity_rows;
    A.out_ids = input_ids_dev; A.out_mask = attention_mask_dev; A.out_seg = segment_ids_dev; A.out_pos = position_ids_dev;
    int rc;
    if ((rc = pack_maps_locked(c, A, total_host, input_ids_dev != nullptr))) return rc;
    if (!input_ids_dev || *total_host <= capacity_rows) return GZ_OK;
    gz_launch_pack_col(A, c->stream);                                      // (the fill wrote nothing, doc_col included: the maps are valid all the same)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return fail(c, GZ_E_CAPACITY, "the batch makes %lld packed rows, capacity is %lld", (long long)*total_host, (long long)capacity_rows);
} GZ_CATCH(c)

int gz_pack_rows(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t max_len, int32_t skip_front, int32_t skip_back,
                 int32_t* input_ids, int32_t* attention_mask, int32_t* segment_ids, int32_t* position_ids, int32_t* doc_row, int32_t* doc_col,
                 int32_t* doc_len, int64_t* pack_off, int64_t* seg_off, int64_t capacity_rows, int64_t* total_host)
try {
    if (!c || !row_off || !pack_off || !total_host || n_rows < 0 || capacity_rows < 0)
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    if (!pack_rule_ok(n_rows, max_len, skip_front, skip_back)) return fail(c, GZ_E_INVALID, "%s", kPackRule);
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, (size_t)(n_rows + 1) * 12))) return rc;              // kept through both passes: pack_off, then doc_len
    GzPackArgs A{};
    A.ids = (const int32_t*)in.d_payload; A.row_off = in.d_off; A.n_rows = n_rows;
    A.max_len = max_len; A.skip_front = skip_front; A.skip_back = skip_back;
    A.pack_off = (int64_t*)in.d_keep; A.doc_len = (int32_t*)(A.pack_off + n_rows + 1);          // (the other maps: the workspace's)
    int64_t total = 0;
    if ((rc = pack_maps_locked(c, A, &total, false))) return rc;
    *total_host = total;
    if ((rc = copy_out(c, pack_off, A.pack_off, (size_t)(total + 1) * 8, c->stream))) return rc;
    if (seg_off && (rc = copy_out(c, seg_off, A.seg_off, (size_t)(n_rows + 1) * 8, c->stream))) return rc;
    if (doc_row && (rc = copy_out(c, doc_row, A.doc_row, (size_t)n_rows * 4, c->stream))) return rc;
    if (doc_col && (rc = copy_out(c, doc_col, A.doc_col, (size_t)n_rows * 4, c->stream))) return rc;
    if (doc_len && (rc = copy_out(c, doc_len, A.doc_len, (size_t)n_rows * 4, c->stream))) return rc;
    if (!input_ids) return GZ_OK;
    if (total > capacity_rows)
        return fail(c, GZ_E_CAPACITY, "the batch makes %lld packed rows, capacity is %lld", (long long)total, (long long)capacity_rows);
    if (total == 0) return GZ_OK;
    const size_t cells = (size_t)total * (size_t)max_len * 4;
    StagedOut S;
    S.add(input_ids, cells, true); S.add(attention_mask, cells, true); S.add(segment_ids, cells, true); S.add(position_ids, cells, true);
    if ((rc = staged_ensure(c, S))) return rc;
    A.capacity = total;
    A.out_ids = S.dev(0); A.out_mask = S.dev(1); A.out_seg = S.dev(2); A.out_pos = S.dev(3);
    gz_launch_pack_fill(A, c->stream);
    return staged_copy_out(c, S);
} GZ_CATCH(c)

// ---- best-fit packing: short documents packed into FULL rows of max_len ----------------------------------------------------
namespace {
// The maps of a batch in best-fit order on the context's stream, behind whatever it holds (gz_packfit.inc): the histogram comes down
// through the pinned block (the first wait), the plan of gz_packfit.h runs on the host, the events and the final segments go up
// through the library's pinned staging, then pack_off, doc_row, doc_col, row_docs and seg_off (when F.P.seg_off is given) and, with
// `fill` and R <= F.P.capacity, the rows; the second wait is for all of that.  A map the caller does not take lives in the
// workspace (pack_off is the caller's).  *total = R, known from the plan.
int fit_maps_locked(gz_ctx* c, GzFitArgs& F, int64_t* total, bool fill)
{
    if (!c->have_tables) return fail(c, GZ_E_NOTABLES, "gz_load_tables has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    GzPackArgs& A = F.P;
    const int64_t n = A.n_rows;
    const int32_t L = A.max_len;
    int rc;
    *total = 0;
    if (n <= 0) {
        HIPCHK(c, hipMemsetAsync(A.pack_off, 0, 8, c->stream));
        if (A.seg_off) HIPCHK(c, hipMemsetAsync(A.seg_off, 0, 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return GZ_OK;
    }
    if (!A.doc_row) { if ((rc = ensure(c, c->w_pk_drow, (size_t)(n + 1) * 4))) return rc; A.doc_row = (int32_t*)c->w_pk_drow.p; }
    if (!A.doc_col) { if ((rc = ensure(c, c->w_pk_dcol, (size_t)(n + 1) * 4))) return rc; A.doc_col = (int32_t*)c->w_pk_dcol.p; }
    if (!A.doc_len) { if ((rc = ensure(c, c->w_pf_dlen, (size_t)(n + 1) * 4))) return rc; A.doc_len = (int32_t*)c->w_pf_dlen.p; }
    if (!F.row_docs) { if ((rc = ensure(c, c->w_pf_rdocs, (size_t)(n + 1) * 4))) return rc; F.row_docs = (int32_t*)c->w_pf_rdocs.p; }
    const size_t W = (size_t)L + 1, tiles = (size_t)gz_fit_tiles(n);
    if ((rc = ensure(c, c->w_pk_len, (size_t)(n + 1) * 8))) return rc;
    if ((rc = ensure(c, c->w_pf_rank, (size_t)(n + 1) * 4))) return rc;
    if ((rc = ensure(c, c->w_pf_tab, (tiles + 1) * W * 4))) return rc;
    A.len64 = (int64_t*)c->w_pk_len.p;
    F.rank = (int32_t*)c->w_pf_rank.p; F.tab = (int32_t*)c->w_pf_tab.p; F.hist = F.tab + tiles * W;
    A.bos_id = c->dev.bos_id; A.eos_id = c->dev.eos_id; A.pad_id = c->dev.pad_id;
    gz_launch_packfit_hist(F, c->stream);
    int32_t* const h = c->pin->fit_hist;
    HIPCHK(c, hipMemcpyAsync(h, F.hist, W * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    GzFitPlan& plan = c->fit_plan;                                         // (the context's: its tables keep their capacity from call to call)
    alloc_site(c);
    const auto t0 = std::chrono::steady_clock::now();
    gz_packfit_plan(h, L, plan);
    c->fit_plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->fit_events = (int64_t)plan.ev.size(); c->fit_segments = (int64_t)plan.seg.size() - 1;
    // events, ev_off and segments in ONE host block and one upload (16-byte aligned parts)
    const size_t ev_raw = plan.ev.size() * sizeof(GzFitEvent), off_raw = (W + 1) * 4, seg_bytes = plan.seg.size() * sizeof(GzFitSeg);
    const size_t ev_bytes = (ev_raw + 15) & ~(size_t)15, off_bytes = (off_raw + 15) & ~(size_t)15;
    std::vector<uint8_t>& up = c->fit_upload;
    up.assign(ev_bytes + off_bytes + seg_bytes, 0);
    if (ev_raw) std::memcpy(up.data(), plan.ev.data(), ev_raw);
    std::memcpy(up.data() + ev_bytes, plan.ev_off.data(), off_raw);
    std::memcpy(up.data() + ev_bytes + off_bytes, plan.seg.data(), seg_bytes);
    if ((rc = ensure(c, c->w_pf_plan, up.size()))) return rc;
    uint8_t* const d_plan = (uint8_t*)c->w_pf_plan.p;
    if ((rc = copy_in(c, d_plan, up.data(), up.size(), c->stream))) return rc;
    F.ev = (const GzFitEvent*)d_plan; F.ev_off = (const int32_t*)(d_plan + ev_bytes); F.seg = (const GzFitSeg*)(d_plan + ev_bytes + off_bytes);
    F.n_seg = (int32_t)plan.seg.size(); F.R = plan.R;
    *total = plan.R;
    gz_launch_packfit_maps(F, c->stream);
    if (fill && plan.R <= A.capacity) gz_launch_packfit_fill(F, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}

const char* const kFitRule = "best-fit packed rows need max_len <= 4096";
}  // namespace

int gz_pack_rows_fit_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t max_len, int32_t skip_front,
                            int32_t skip_back, int32_t* input_ids_dev, int32_t* attention_mask_dev, int32_t* segment_ids_dev,
                            int32_t* position_ids_dev, int32_t* doc_row_dev, int32_t* doc_col_dev, int32_t* doc_len_dev, int32_t* row_docs_dev,
                            int64_t* pack_off_dev, int64_t* seg_off_dev, int64_t capacity_rows, int64_t* total_host)
try {
    if (!c || !row_off_dev || !pack_off_dev || !total_host || n_rows < 0 || capacity_rows < 0)
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    if (!pack_rule_ok(n_rows, max_len, skip_front, skip_back)) return fail(c, GZ_E_INVALID, "%s", kPackRule);
    if (max_len > GZ_PACK_FIT_MAX_LEN) return fail(c, GZ_E_INVALID, "%s", kFitRule);
    std::lock_guard<std::mutex> lk(c->mu);
    GzFitArgs F{};
    GzPackArgs& A = F.P;
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows; A.max_len = max_len; A.skip_front = skip_front; A.skip_back = skip_back;
    A.doc_row = doc_row_dev; A.doc_col = doc_col_dev; A.doc_len = doc_len_dev; A.pack_off = pack_off_dev; A.seg_off = seg_off_dev;
    F.row_docs = row_docs_dev;
    A.capacity = capacity_rows;
    A.out_ids = input_ids_dev; A.out_mask = attention_mask_dev; A.out_seg = segment_ids_dev; A.out_pos = position_ids_dev;
    int rc;
    if ((rc = fit_maps_locked(c, F, total_host, input_ids_dev != nullptr))) return rc;
    if (!input_ids_dev || *total_host <= capacity_rows) return GZ_OK;
    return fail(c, GZ_E_CAPACITY, "the batch makes %lld packed rows, capacity is %lld", (long long)*total_host, (long long)capacity_rows);
} GZ_CATCH(c)

int gz_pack_rows_fit_info(gz_ctx* c, double* plan_ms, int64_t* events, int64_t* segments)
try {
    if (!c) return GZ_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (plan_ms) *plan_ms = c->fit_plan_ms;
    if (events) *events = c->fit_events;
    if (segments) *segments = c->fit_segments;
    return GZ_OK;
} GZ_CATCH(c)

int gz_pack_rows_fit(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t max_len, int32_t skip_front, int32_t skip_back,
                     int32_t* input_ids, int32_t* attention_mask, int32_t* segment_ids, int32_t* position_ids, int32_t* doc_row, int32_t* doc_col,
                     int32_t* doc_len, int32_t* row_docs, int64_t* pack_off, int64_t* seg_off, int64_t capacity_rows, int64_t* total_host)
try {
    if (!c || !row_off || !pack_off || !total_host || n_rows < 0 || capacity_rows < 0)
        return c ? fail(c, GZ_E_INVALID, "bad arguments") : GZ_E_INVALID;
    if (!pack_rule_ok(n_rows, max_len, skip_front, skip_back)) return fail(c, GZ_E_INVALID, "%s", kPackRule);
    if (max_len > GZ_PACK_FIT_MAX_LEN) return fail(c, GZ_E_INVALID, "%s", kFitRule);
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, (size_t)(n_rows + 1) * 8))) return rc;               // kept through both passes: pack_off
    GzFitArgs F{};
    GzPackArgs& A = F.P;
    A.ids = (const int32_t*)in.d_payload; A.row_off = in.d_off; A.n_rows = n_rows;
    A.max_len = max_len; A.skip_front = skip_front; A.skip_back = skip_back;
    A.pack_off = (int64_t*)in.d_keep;                                                 // (the other maps: the workspace's)
    if (seg_off) { if ((rc = ensure(c, c->w_pk_seg, (size_t)(n_rows + 1) * 8))) return rc; A.seg_off = (int64_t*)c->w_pk_seg.p; }
    int64_t total = 0;
    if ((rc = fit_maps_locked(c, F, &total, false))) return rc;
    *total_host = total;
    if ((rc = copy_out(c, pack_off, A.pack_off, (size_t)(total + 1) * 8, c->stream))) return rc;
    if (seg_off && (rc = copy_out(c, seg_off, A.seg_off, (size_t)(n_rows + 1) * 8, c->stream))) return rc;
    if (doc_row && (rc = copy_out(c, doc_row, A.doc_row, (size_t)n_rows * 4, c->stream))) return rc;
    if (doc_col && (rc = copy_out(c, doc_col, A.doc_col, (size_t)n_rows * 4, c->stream))) return rc;
    if (doc_len && (rc = copy_out(c, doc_len, A.doc_len, (size_t)n_rows * 4, c->stream))) return rc;
    if (row_docs && (rc = copy_out(c, row_docs, F.row_docs, (size_t)n_rows * 4, c->stream))) return rc;
    if (!input_ids) return GZ_OK;
    if (total > capacity_rows)
        return fail(c, GZ_E_CAPACITY, "the batch makes %lld packed rows, capacity is %lld", (long long)total, (long long)capacity_rows);
    if (total == 0) return GZ_OK;
    const size_t cells = (size_t)total * (size_t)max_len * 4;
    StagedOut S;
    S.add(input_ids, cells, true); S.add(attention_mask, cells, true); S.add(segment_ids, cells, true); S.add(position_ids, cells, true);
    if ((rc = staged_ensure(c, S))) return rc;
    A.capacity = total;
    A.out_ids = S.dev(0); A.out_mask = S.dev(1); A.out_seg = S.dev(2); A.out_pos = S.dev(3);
    gz_launch_packfit_fill(F, c->stream);
    return staged_copy_out(c, S);
} GZ_CATCH(c)

// ---- masked-LM inputs and labels over dense rows -------------------------------------------------------------------------
namespace {
struct MaskRule {
    int64_t n_rows; int32_t row_len; int64_t row_base; uint64_t seed, t_sel, t1, t2;
    int32_t rand_lo, rand_hi, mask_id, whole_word, ignore_index;
};
const char* const kMaskRule = "masked rows need row_len >= 1, n_rows >= 0, row_base >= 0, (row_base + n_rows) * row_len < 2^63, thresholds in "
                              "[0, 2^32] with t1 <= t2, rand_lo < rand_hi and whole_word 0 or 1";
bool mask_rule_ok(const MaskRule& M)
{
    constexpr uint64_t one = 1ull << 32;
    return dense_rule_ok(M.n_rows, M.row_len, M.row_base, M.whole_word) && M.t_sel <= one && M.t1 <= one && M.t2 <= one && M.t1 <= M.t2 &&
           M.rand_lo < M.rand_hi;
}
// the cell arrays and the counts are pairwise disjoint (the heads are read from neighbours' ORIGINAL ids); n_rows * row_len > 0
bool mask_buffers_ok(const MaskRule& M, const int32_t* ids, const int32_t* out_ids, const int32_t* labels, const int32_t* n_chosen)
{
    if (!ids || !out_ids || !labels) return false;
    if ((uint64_t)M.n_rows * (uint64_t)M.row_len > (uint64_t)(UINTPTR_MAX / 4)) return false;       // (the byte counts below do not wrap)
    const uintptr_t cells = (uintptr_t)M.n_rows * (uintptr_t)M.row_len * 4u;
    const Span s[4] = {span_of(ids, cells), span_of(out_ids, cells), span_of(labels, cells), span_of(n_chosen, (uintptr_t)M.n_rows * 4u)};
    return disjoint(s, 4);
}
// the one launch on the context's stream, behind whatever it holds
void mask_launch(gz_ctx* c, const MaskRule& M, const int32_t* ids_dev, int32_t* out_dev, int32_t* labels_dev, int32_t* n_chosen_dev)
{
    GzMaskArgs A{};
    A.ids = ids_dev; A.n_rows = M.n_rows; A.row_len = M.row_len; A.row_base = M.row_base;
    A.key0 = (uint32_t)M.seed; A.key1 = (uint32_t)(M.seed >> 32);
    A.t_sel = M.t_sel; A.t1 = M.t1; A.t2 = M.t2;
    A.rand_lo = M.rand_lo; A.rand_span = (uint32_t)M.rand_hi - (uint32_t)M.rand_lo;
    A.mask_id = M.mask_id; A.ignore_index = M.ignore_index; A.whole_word = M.whole_word;
    A.pad_id = c->dev.pad_id; A.bos_id = c->dev.bos_id; A.eos_id = c->dev.eos_id;
    A.cont_bits = (const uint32_t*)c->t_dec_cont.p; A.n_ids = c->dec_n_ids;
    A.bits_in_lds = c->opt.mask_lds;                                          // (the launcher drops it when the bitmap does not fit)
    A.out_ids = out_dev; A.labels = labels_dev; A.n_chosen = n_chosen_dev;
    gz_launch_mask(A, c->stream);
}
}  // namespace

int gz_mask_rows_device(gz_ctx* c, const int32_t* ids_dev, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed, uint64_t t_sel,
                        uint64_t t1, uint64_t t2, int32_t rand_lo, int32_t rand_hi, int32_t mask_id, int32_t whole_word, int32_t ignore_index,
                        int32_t* input_ids_dev, int32_t* labels_dev, int32_t* n_chosen_dev)
try {
    if (!c) return GZ_E_INVALID;
    const MaskRule M{n_rows, row_len, row_base, seed, t_sel, t1, t2, rand_lo, rand_hi, mask_id, whole_word, ignore_index};
    if (!mask_rule_ok(M)) return fail(c, GZ_E_INVALID, "%s", kMaskRule);
    if (n_rows > 0 && !mask_buffers_ok(M, ids_dev, input_ids_dev, labels_dev, n_chosen_dev))
        return fail(c, GZ_E_INVALID, "masked rows need ids, input_ids and labels, and buffers that do not overlap");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_dec) return fail(c, GZ_E_NOTABLES, "gz_decoder_snapshot has not been called");
    if (n_rows == 0) return GZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    mask_launch(c, M, ids_dev, input_ids_dev, labels_dev, n_chosen_dev);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_mask_rows(gz_ctx* c, const int32_t* ids, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed, uint64_t t_sel, uint64_t t1,
                 uint64_t t2, int32_t rand_lo, int32_t rand_hi, int32_t mask_id, int32_t whole_word, int32_t ignore_index, int32_t* input_ids,
                 int32_t* labels, int32_t* n_chosen)
try {
    if (!c) return GZ_E_INVALID;
    const MaskRule M{n_rows, row_len, row_base, seed, t_sel, t1, t2, rand_lo, rand_hi, mask_id, whole_word, ignore_index};
    if (!mask_rule_ok(M)) return fail(c, GZ_E_INVALID, "%s", kMaskRule);
    if (n_rows > 0 && !mask_buffers_ok(M, ids, input_ids, labels, n_chosen))
        return fail(c, GZ_E_INVALID, "masked rows need ids, input_ids and labels, and buffers that do not overlap");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_dec) return fail(c, GZ_E_NOTABLES, "gz_decoder_snapshot has not been called");
    if (n_rows == 0) return GZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)n_rows * (size_t)row_len * 4;
    StagedOut S;
    S.add(input_ids, cells, true); S.add(labels, cells, true); S.add(n_chosen, (size_t)n_rows * 4, false);
    int rc;
    if ((rc = ensure(c, c->w_rows_in, cells)) || (rc = copy_in(c, c->w_rows_in.p, ids, cells, c->stream)) || (rc = staged_ensure(c, S))) return rc;
    mask_launch(c, M, (const int32_t*)c->w_rows_in.p, S.dev(0), S.dev(1), S.dev(2));
    return staged_copy_out(c, S);
} GZ_CATCH(c)

// ---- span-corruption inputs and targets over dense rows -------------------------------------------------------------------
namespace {
struct InfillRule {
    int64_t n_rows; int32_t row_len; int64_t row_base; uint64_t seed, t_start; const uint64_t* len_t;
    int32_t n_len, mask_id, whole_word, ignore_index, dec_width;
};
struct InfillBufs {
    const int32_t* ids; int32_t* input_ids; int32_t* attention_mask; int32_t* labels; int32_t* decoder_input_ids;
    int32_t* enc_len; int32_t* dec_len; int32_t* n_spans;
};
const char* const kInfillRule = "infill rows need row_len >= 1, n_rows >= 0, row_base >= 0, (row_base + n_rows) * row_len < 2^63, dec_width >= 1, "
                                "t_start in [0, 2^32], 1 <= n_len <= 16 with n_len - 1 non-decreasing thresholds in [0, 2^32] and whole_word 0 or 1";
bool infill_rule_ok(const InfillRule& M)
{
    constexpr uint64_t one = 1ull << 32;
    if (!dense_rule_ok(M.n_rows, M.row_len, M.row_base, M.whole_word) || M.dec_width < 1) return false;
    if (M.t_start > one || M.n_len < 1 || M.n_len > 16) return false;
    if (M.n_len > 1 && !M.len_t) return false;
    for (int k = 0; k + 1 < M.n_len; ++k)
        if (M.len_t[k] > one || (k > 0 && M.len_t[k] < M.len_t[k - 1])) return false;
    return true;
}
// the eight arrays are pairwise disjoint (every cell is read from the ORIGINAL rows and written once); n_rows > 0
bool infill_buffers_ok(const InfillRule& M, const InfillBufs& B)
{
    if (!B.ids || !B.input_ids || !B.labels) return false;
    if ((uint64_t)M.n_rows * (uint64_t)M.row_len > (uint64_t)(UINTPTR_MAX / 4)) return false;       // (the byte counts below do not wrap)
    if ((uint64_t)M.n_rows * (uint64_t)M.dec_width > (uint64_t)(UINTPTR_MAX / 4)) return false;
    const uintptr_t cells = (uintptr_t)M.n_rows * (uintptr_t)M.row_len * 4u, dec = (uintptr_t)M.n_rows * (uintptr_t)M.dec_width * 4u,
                    cnt = (uintptr_t)M.n_rows * 4u;
    const Span s[8] = {span_of(B.ids, cells), span_of(B.input_ids, cells), span_of(B.attention_mask, cells), span_of(B.labels, dec),
                       span_of(B.decoder_input_ids, dec), span_of(B.enc_len, cnt), span_of(B.dec_len, cnt), span_of(B.n_spans, cnt)};
    return disjoint(s, 8);
}
// the one launch on the context's stream, behind whatever it holds; every pointer of B a device pointer
void infill_launch(gz_ctx* c, const InfillRule& M, const InfillBufs& B)
{
    GzInfillArgs A{};
    A.ids = B.ids; A.n_rows = M.n_rows; A.row_len = M.row_len; A.row_base = M.row_base;
    A.key0 = (uint32_t)M.seed; A.key1 = (uint32_t)(M.seed >> 32);
    A.t_start = M.t_start; A.n_len = M.n_len;
    for (int k = 0; k < 15; ++k) A.len_t[k] = k + 1 < M.n_len ? M.len_t[k] : 1ull << 32;       // (len_t is a host pointer: its words travel in the arguments)
    A.mask_id = M.mask_id; A.ignore_index = M.ignore_index; A.whole_word = M.whole_word; A.dec_width = M.dec_width;
    A.pad_id = c->dev.pad_id; A.bos_id = c->dev.bos_id; A.eos_id = c->dev.eos_id;
    A.cont_bits = (const uint32_t*)c->t_dec_cont.p; A.n_ids = c->dec_n_ids;
    A.bits_in_lds = c->opt.mask_lds;                                          // (the launcher drops it when the bitmap does not fit)
    A.out_ids = B.input_ids; A.out_mask = B.attention_mask; A.labels = B.labels; A.dec_ids = B.decoder_input_ids;
    A.enc_len = B.enc_len; A.dec_len = B.dec_len; A.n_spans = B.n_spans;
    gz_launch_infill(A, c->stream);
}
}  // namespace

int gz_infill_rows_device(gz_ctx* c, const int32_t* ids_dev, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed, uint64_t t_start,
                          const uint64_t* len_t, int32_t n_len, int32_t mask_id, int32_t whole_word, int32_t ignore_index, int32_t dec_width,
                          int32_t* input_ids_dev, int32_t* attention_mask_dev, int32_t* labels_dev, int32_t* decoder_input_ids_dev,
                          int32_t* enc_len_dev, int32_t* dec_len_dev, int32_t* n_spans_dev)
try {
    if (!c) return GZ_E_INVALID;
    const InfillRule M{n_rows, row_len, row_base, seed, t_start, len_t, n_len, mask_id, whole_word, ignore_index, dec_width};
    const InfillBufs B{ids_dev, input_ids_dev, attention_mask_dev, labels_dev, decoder_input_ids_dev, enc_len_dev, dec_len_dev, n_spans_dev};
    if (!infill_rule_ok(M)) return fail(c, GZ_E_INVALID, "%s", kInfillRule);
    if (n_rows > 0 && !infill_buffers_ok(M, B))
        return fail(c, GZ_E_INVALID, "infill rows need ids, input_ids and labels, and buffers that do not overlap");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_dec) return fail(c, GZ_E_NOTABLES, "gz_decoder_snapshot has not been called");
    if (n_rows == 0) return GZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    infill_launch(c, M, B);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_infill_rows(gz_ctx* c, const int32_t* ids, int64_t n_rows, int32_t row_len, int64_t row_base, uint64_t seed, uint64_t t_start,
                   const uint64_t* len_t, int32_t n_len, int32_t mask_id, int32_t whole_word, int32_t ignore_index, int32_t dec_width,
                   int32_t* input_ids, int32_t* attention_mask, int32_t* labels, int32_t* decoder_input_ids, int32_t* enc_len, int32_t* dec_len,
                   int32_t* n_spans)
try {
    if (!c) return GZ_E_INVALID;
    const InfillRule M{n_rows, row_len, row_base, seed, t_start, len_t, n_len, mask_id, whole_word, ignore_index, dec_width};
    if (!infill_rule_ok(M)) return fail(c, GZ_E_INVALID, "%s", kInfillRule);
    if (n_rows > 0 && !infill_buffers_ok(M, InfillBufs{ids, input_ids, attention_mask, labels, decoder_input_ids, enc_len, dec_len, n_spans}))
        return fail(c, GZ_E_INVALID, "infill rows need ids, input_ids and labels, and buffers that do not overlap");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_dec) return fail(c, GZ_E_NOTABLES, "gz_decoder_snapshot has not been called");
    if (n_rows == 0) return GZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)n_rows * (size_t)row_len * 4, dec = (size_t)n_rows * (size_t)dec_width * 4, cnt = (size_t)n_rows * 4;
    StagedOut S;
    S.add(input_ids, cells, true); S.add(attention_mask, cells, true); S.add(labels, dec, true); S.add(decoder_input_ids, dec, true);
    S.add(enc_len, cnt, false); S.add(dec_len, cnt, false); S.add(n_spans, cnt, false);
    int rc;
    if ((rc = ensure(c, c->w_rows_in, cells)) || (rc = copy_in(c, c->w_rows_in.p, ids, cells, c->stream)) || (rc = staged_ensure(c, S))) return rc;
    infill_launch(c, M, InfillBufs{(const int32_t*)c->w_rows_in.p, S.dev(0), S.dev(1), S.dev(2), S.dev(3), S.dev(4), S.dev(5), S.dev(6)});
    return staged_copy_out(c, S);
} GZ_CATCH(c)

// ---- near-duplicate documents by MinHash signatures ---------------------------------------------------------------------
namespace {
const char* const kMinhashRowsBuffers = "minhash rows need ids, row_off and signatures, and output arrays that overlap neither the input nor each other";
const char* const kMinhashGroupsBuffers = "minhash groups need signatures, group and n_groups_host, and arrays that do not overlap";

// n_rows > 0.  ids_bytes: what the call knows of the ids' extent (the host form: all of it; the device form: their first word)
bool minhash_rows_buffers_ok(const void* ids, uintptr_t ids_bytes, const int64_t* row_off, int64_t n_rows, int32_t num_perm, const uint32_t* signatures,
                             const int32_t* n_shingles)
{
    if (!row_off || !signatures) return false;
    if ((uint64_t)n_rows > (uint64_t)(UINTPTR_MAX / 4 / 256)) return false;                              // (the byte counts below do not wrap)
    const uintptr_t n = (uintptr_t)n_rows;
    const Span s[4] = {span_of(ids, ids_bytes), span_of(row_off, (n + 1) * 8u), span_of(signatures, n * (uintptr_t)num_perm * 4u), span_of(n_shingles, n * 4u)};
    return disjoint(s, 4);
}

// Both passes on the context's stream, behind whatever it holds; the caller waits for the signatures.  Nothing is written to the
// outputs when a body is too long.  n_rows > 0.
int minhash_rows_locked(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                        int32_t shingle, int32_t num_perm, uint64_t seed, uint32_t* sig_dev, int32_t* n_shingles_dev)
{
    int rc;
    Pieces P;
    if ((rc = pieces_count_locked(c, row_off_dev, n_rows, skip_front, skip_back, shingle, GZ_PIECES_SHINGLES, false, nullptr, &P))) return rc;
    GzMinhashArgs A{};
    A.ids = ids_dev; A.row_off = row_off_dev; A.n_rows = n_rows;
    A.skip_front = skip_front; A.skip_back = skip_back; A.shingle = shingle; A.num_perm = num_perm;
    A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32);
    A.piece_off = P.piece_off; A.n_pieces = P.n_pieces;
    A.sig = sig_dev; A.n_shingles = n_shingles_dev;
    gz_launch_minhash_sig(A, c->stream);
    return GZ_OK;
}

// All bands and the labels on the context's stream; *n_groups is read back, so the labels are complete on return.  n_rows > 0.
int minhash_groups_locked(gz_ctx* c, const uint32_t* sig_dev, int64_t n_rows, int32_t num_perm, int32_t bands, int32_t min_agree, int32_t* group_dev,
                          int64_t* n_groups)
{
    const uint64_t cap = gz_minhash_cap(n_rows);
    int rc;
    if ((rc = ensure(c, c->w_mh_keys, (size_t)cap * 8)) || (rc = ensure(c, c->w_mh_reps, (size_t)cap * 4)) ||
        (rc = ensure(c, c->w_mh_aux, (size_t)n_rows + 16))) return rc;
    GzMinhashGroupArgs A{};
    A.sig = sig_dev; A.n_rows = n_rows; A.num_perm = num_perm; A.bands = bands; A.min_agree = min_agree;
    A.group = group_dev;
    A.keys = (unsigned long long*)c->w_mh_keys.p; A.reps = (uint32_t*)c->w_mh_reps.p; A.cap = cap;
    A.n_groups = (unsigned long long*)c->w_mh_aux.p; A.empty = (uint8_t*)c->w_mh_aux.p + 8;
    gz_launch_minhash_groups(A, c->stream);
    if ((rc = read_total(c, (const int64_t*)A.n_groups, nullptr, n_groups))) return rc;
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}
}  // namespace

int gz_minhash_rows_device(gz_ctx* c, const int32_t* ids_dev, const int64_t* row_off_dev, int64_t n_rows, int32_t skip_front, int32_t skip_back,
                           int32_t shingle, int32_t num_perm, uint64_t seed, uint32_t* signatures_dev, int32_t* n_shingles_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = minhash_rows_fault(n_rows, skip_front, skip_back, shingle, num_perm)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!ids_dev || !minhash_rows_buffers_ok(ids_dev, 4, row_off_dev, n_rows, num_perm, signatures_dev, n_shingles_dev))
        return fail(c, GZ_E_INVALID, "%s", kMinhashRowsBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = minhash_rows_locked(c, ids_dev, row_off_dev, n_rows, skip_front, skip_back, shingle, num_perm, seed, signatures_dev, n_shingles_dev)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_minhash_rows(gz_ctx* c, const int32_t* ids, const int64_t* row_off, int64_t n_rows, int32_t skip_front, int32_t skip_back, int32_t shingle,
                    int32_t num_perm, uint64_t seed, uint32_t* signatures, int32_t* n_shingles)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = minhash_rows_fault(n_rows, skip_front, skip_back, shingle, num_perm)) return fail(c, GZ_E_INVALID, "%s", why);
    if (n_rows == 0) return GZ_OK;
    if (!row_off || !signatures) return fail(c, GZ_E_INVALID, "%s", kMinhashRowsBuffers);
    RowsIn in{ids, row_off, n_rows, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords))) return rc;
    if (!minhash_rows_buffers_ok(in.n ? ids + row_off[0] : nullptr, (uintptr_t)in.n * 4u, row_off, n_rows, num_perm, signatures, n_shingles))
        return fail(c, GZ_E_INVALID, "%s", kMinhashRowsBuffers);
    if (!minhash_bodies_fit(row_off, n_rows, skip_front, skip_back)) return fail(c, GZ_E_LIMIT, "%s", kBodyLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, 0))) return rc;
    StagedOut S;
    S.add(signatures, (size_t)n_rows * (size_t)num_perm * 4, true); S.add(n_shingles, (size_t)n_rows * 4, false);
    if ((rc = staged_ensure(c, S))) return rc;
    if ((rc = minhash_rows_locked(c, (const int32_t*)in.d_payload, in.d_off, n_rows, skip_front, skip_back, shingle, num_perm, seed,
                                  (uint32_t*)S.e[0].dev, S.dev(1)))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

int gz_minhash_groups_device(gz_ctx* c, const uint32_t* signatures_dev, int64_t n_rows, int32_t num_perm, int32_t bands, int32_t min_agree,
                             int32_t* group_dev, int64_t* n_groups_host)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = minhash_groups_fault(n_rows, num_perm, bands, min_agree)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!n_groups_host) return fail(c, GZ_E_INVALID, "%s", kMinhashGroupsBuffers);
    if (n_rows == 0) { *n_groups_host = 0; return GZ_OK; }
    const Span s[2] = {span_of(signatures_dev, (uintptr_t)n_rows * (uintptr_t)num_perm * 4u), span_of(group_dev, (uintptr_t)n_rows * 4u)};
    if (!signatures_dev || !group_dev || !disjoint(s, 2)) return fail(c, GZ_E_INVALID, "%s", kMinhashGroupsBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return minhash_groups_locked(c, signatures_dev, n_rows, num_perm, bands, min_agree, group_dev, n_groups_host);
} GZ_CATCH(c)

int gz_minhash_groups(gz_ctx* c, const uint32_t* signatures, int64_t n_rows, int32_t num_perm, int32_t bands, int32_t min_agree, int32_t* group,
                      int64_t* n_groups_host)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = minhash_groups_fault(n_rows, num_perm, bands, min_agree)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!n_groups_host) return fail(c, GZ_E_INVALID, "%s", kMinhashGroupsBuffers);
    if (n_rows == 0) { *n_groups_host = 0; return GZ_OK; }
    const size_t sig_bytes = (size_t)n_rows * (size_t)num_perm * 4;
    const Span s[3] = {span_of(signatures, sig_bytes), span_of(group, (uintptr_t)n_rows * 4u), span_of(n_groups_host, 8)};
    if (!signatures || !group || !disjoint(s, 3)) return fail(c, GZ_E_INVALID, "%s", kMinhashGroupsBuffers);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    StagedOut S;
    S.add(group, (size_t)n_rows * 4, true);
    int rc;
    if ((rc = ensure(c, c->w_rows_in, sig_bytes)) || (rc = copy_in(c, c->w_rows_in.p, signatures, sig_bytes, c->stream)) || (rc = staged_ensure(c, S)))
        return rc;
    int64_t n_groups = 0;
    if ((rc = minhash_groups_locked(c, (const uint32_t*)c->w_rows_in.p, n_rows, num_perm, bands, min_agree, S.dev(0), &n_groups))) return rc;
    if ((rc = staged_copy_out(c, S))) return rc;
    *n_groups_host = n_groups;
    return GZ_OK;
} GZ_CATCH(c)

// ---- word spans, word ids and aligned labels (gz_align.inc) ---------------------------------------------------------------
namespace {
constexpr RowsWords kWordWords{"bad word offsets", "word offsets must not decrease"};
constexpr RowsWords kMarkWords{"bad mark offsets", "mark offsets must not decrease"};
const char* const kSpanDocLimit = "a document holds 2^31 bytes or more: split it";
const char* const kSpanWordLimit = "the batch holds 2^31 words or more: split it";
// c->w_al: the span kernels' scans, the align call's token scan, the owners of span labels, and the staged inputs of the host forms
enum { ALW_BRK, ALW_GRAN, ALW_BLKS, ALW_BLKL, ALW_BASES, ALW_BASEL, ALW_LEAD0, ALW_BLKDOC, ALW_TOK, ALW_OWNER, ALW_IN0, ALW_IN1, ALW_IN2, ALW_IN3 };

// a host array the row front does not carry: `bytes` of it into w_al[k]; *dev = its device copy (nullptr for a null array)
int align_stage_bytes(gz_ctx* c, int k, const void* host, size_t bytes, const void** dev)
{
    *dev = nullptr;
    if (!host) return GZ_OK;
    int rc;
    if ((rc = ensure(c, c->w_al[k], bytes ? bytes : 16))) return rc;
    if (bytes && (rc = copy_in(c, c->w_al[k].p, host, bytes, c->stream))) return rc;
    *dev = c->w_al[k].p;
    return GZ_OK;
}
int align_stage(gz_ctx* c, int k, const int32_t* host, size_t bytes, const int32_t** dev) { return align_stage_bytes(c, k, host, bytes, (const void**)dev); }
int align_stage64(gz_ctx* c, int k, const int64_t* host, size_t bytes, const int64_t** dev) { return align_stage_bytes(c, k, host, bytes, (const void**)dev); }

// The count pass on the context's stream, behind whatever it holds: A.text, text_off, n_docs, B, unit and word_off are the caller's,
// the scans are the workspace's.  *total = W, read back from the device (the one wait of the pass); the limits are checked there.
int span_count_locked(gz_ctx* c, GzSpanArgs& A, int64_t* total)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nblk = (size_t)gz_span_blocks(A.B);
    int rc;
    if ((rc = ensure(c, c->w_al[ALW_BRK], (size_t)(A.B / 32 + 4) * 4)) || (rc = ensure(c, c->w_al[ALW_GRAN], (nblk * 256 + 1) * 4)) ||
        (rc = ensure(c, c->w_al[ALW_BLKS], (nblk + 1) * 8)) || (rc = ensure(c, c->w_al[ALW_BLKL], (nblk + 1) * 8)) ||
        (rc = ensure(c, c->w_al[ALW_BASES], (nblk + 2) * 8)) || (rc = ensure(c, c->w_al[ALW_BASEL], (nblk + 2) * 8)) ||
        (rc = ensure(c, c->w_al[ALW_LEAD0], (size_t)(A.n_docs + 2) * 8)) || (rc = ensure(c, c->w_al[ALW_BLKDOC], (nblk + 2) * 8))) return rc;
    A.brk = (uint32_t*)c->w_al[ALW_BRK].p; A.gran = (uint32_t*)c->w_al[ALW_GRAN].p;
    A.blk_s = (int64_t*)c->w_al[ALW_BLKS].p; A.blk_l = (int64_t*)c->w_al[ALW_BLKL].p;
    A.base_s = (int64_t*)c->w_al[ALW_BASES].p; A.base_l = (int64_t*)c->w_al[ALW_BASEL].p;
    A.lead0 = (int64_t*)c->w_al[ALW_LEAD0].p; A.blk_doc = (int64_t*)c->w_al[ALW_BLKDOC].p;
    A.too_long = (uint32_t*)(A.lead0 + A.n_docs + 1);
    A.span = nullptr; A.n_words = 0;
    gz_launch_span_count(A, c->stream);
    uint32_t* const h_long = &c->pin->span_long;
    *h_long = 0;
    HIPCHK(c, hipMemcpyAsync(h_long, A.too_long, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_total(c, A.word_off + A.n_docs, nullptr, total))) return rc;
    HIPCHK(c, hipGetLastError());
    if (*h_long) return fail(c, GZ_E_LIMIT, "%s", kSpanDocLimit);
    if (*total >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kSpanWordLimit);
    return GZ_OK;
}
}  // namespace

int gz_word_spans_device(gz_ctx* c, const uint8_t* text_dev, const int64_t* text_off_dev, int64_t n_docs, int64_t text_bytes, int32_t unit,
                         int32_t* span_dev, int64_t* word_off_dev, int64_t capacity_words, int64_t* total_host)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = word_spans_fault(n_docs, unit, capacity_words)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!text_off_dev || !word_off_dev || !total_host || text_bytes < 0 || (text_bytes > 0 && !text_dev)) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    GzSpanArgs A{};
    A.text = text_dev; A.text_off = text_off_dev; A.n_docs = n_docs; A.B = text_bytes; A.unit = unit; A.word_off = word_off_dev;
    int rc;
    if ((rc = span_count_locked(c, A, total_host))) return rc;
    if (!span_dev) return GZ_OK;
    if (*total_host > capacity_words)
        return fail(c, GZ_E_CAPACITY, "the batch has %lld words, capacity is %lld", (long long)*total_host, (long long)capacity_words);
    A.span = span_dev; A.n_words = *total_host;
    gz_launch_span_write(A, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_word_spans(gz_ctx* c, const uint8_t* text, const int64_t* text_off, int64_t n_docs, int32_t unit, int32_t* span, int64_t* word_off,
                  int64_t capacity_words, int64_t* total_host)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = word_spans_fault(n_docs, unit, capacity_words)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!text_off || !word_off || !total_host) return fail(c, GZ_E_INVALID, "bad arguments");
    RowsIn in{text, text_off, n_docs, 1};
    int rc;
    if ((rc = rows_check(c, in, kTextWords))) return rc;
    if (!minhash_bodies_fit(text_off, n_docs, 0, 0)) return fail(c, GZ_E_LIMIT, "%s", kSpanDocLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, (size_t)(n_docs + 1) * 8))) return rc;                  // kept through both passes: word_off
    GzSpanArgs A{};
    A.text = (const uint8_t*)in.d_payload; A.text_off = in.d_off; A.n_docs = n_docs; A.B = in.n; A.unit = unit; A.word_off = (int64_t*)in.d_keep;
    int64_t total = 0;
    if ((rc = span_count_locked(c, A, &total))) return rc;
    *total_host = total;
    if ((rc = copy_out(c, word_off, A.word_off, (size_t)(n_docs + 1) * 8, c->stream))) return rc;
    if (!span) return GZ_OK;
    if (total > capacity_words) return fail(c, GZ_E_CAPACITY, "the batch has %lld words, capacity is %lld", (long long)total, (long long)capacity_words);
    if (total == 0) return GZ_OK;
    StagedOut S;
    S.add(span, (size_t)total * 8, true);
    if ((rc = staged_ensure(c, S))) return rc;
    A.span = S.dev(0); A.n_words = total;
    gz_launch_span_write(A, c->stream);
    return staged_copy_out(c, S);
} GZ_CATCH(c)

namespace {
// the token scan and the one launch on the context's stream; every pointer of A a device pointer, A.tok_off is set here
int align_launch_locked(gz_ctx* c, GzAlignArgs& A, const int32_t* counts_dev)
{
    int rc;
    if ((rc = ensure(c, c->w_al[ALW_TOK], (size_t)(A.n_words + 2) * 4))) return rc;
    gz_launch_align_scan(counts_dev, A.word_off, A.n_words, (uint32_t*)c->w_al[ALW_TOK].p, c->stream);
    A.tok_off = (const uint32_t*)c->w_al[ALW_TOK].p;
    gz_launch_align_rows(A, c->stream);
    return GZ_OK;
}
}  // namespace

int gz_align_rows_device(gz_ctx* c, const int32_t* counts_dev, const int64_t* word_off_dev, int64_t n_docs, int64_t n_words, const int32_t* row_doc_dev,
                         const int32_t* row_start_dev, int64_t n_rows, int32_t max_len, const int32_t* word_labels_dev, int32_t continuation,
                         const int32_t* cont_map_dev, int32_t n_map, int32_t ignore_index, int32_t* word_ids_dev, int32_t* labels_dev, int32_t* n_real_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = align_rows_fault(n_docs, n_rows, row_doc_dev != nullptr, max_len, continuation, cont_map_dev != nullptr, n_map,
                                           labels_dev != nullptr, word_labels_dev != nullptr)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!word_off_dev || n_words < 0 || (n_words > 0 && !counts_dev)) return fail(c, GZ_E_INVALID, "bad arguments");
    if (n_words >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kSpanWordLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_rows == 0 || (!word_ids_dev && !labels_dev && !n_real_dev)) return GZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    GzAlignArgs A{};
    A.word_off = word_off_dev; A.n_docs = n_docs; A.n_words = n_words; A.row_doc = row_doc_dev; A.row_start = row_start_dev; A.n_rows = n_rows;
    A.max_len = max_len; A.word_labels = word_labels_dev; A.continuation = continuation; A.cont_map = cont_map_dev; A.n_map = n_map;
    A.ignore_index = ignore_index; A.word_ids = word_ids_dev; A.labels = labels_dev; A.n_real = n_real_dev;
    int rc;
    if ((rc = align_launch_locked(c, A, counts_dev))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_align_rows(gz_ctx* c, const int32_t* counts, const int64_t* word_off, int64_t n_docs, const int32_t* row_doc, const int32_t* row_start,
                  int64_t n_rows, int32_t max_len, const int32_t* word_labels, int32_t continuation, const int32_t* cont_map, int32_t n_map,
                  int32_t ignore_index, int32_t* word_ids, int32_t* labels, int32_t* n_real)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = align_rows_fault(n_docs, n_rows, row_doc != nullptr, max_len, continuation, cont_map != nullptr, n_map, labels != nullptr,
                                           word_labels != nullptr)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!word_off) return fail(c, GZ_E_INVALID, "bad arguments");
    RowsIn in{counts, word_off, n_docs, 4};
    int rc;
    if ((rc = rows_check(c, in, kWordWords))) return rc;
    if (in.n >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kSpanWordLimit);
    if (const char* why = align_data_fault(in.n ? counts + word_off[0] : nullptr, in.n, row_doc, row_start, n_rows, n_docs))
        return fail(c, GZ_E_INVALID, "%s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_rows == 0 || (!word_ids && !labels && !n_real)) return GZ_OK;
    if ((rc = rows_stage(c, in, 0))) return rc;
    GzAlignArgs A{};
    A.word_off = in.d_off; A.n_docs = n_docs; A.n_words = in.n; A.n_rows = n_rows; A.max_len = max_len;
    A.continuation = continuation; A.n_map = n_map; A.ignore_index = ignore_index;
    const int32_t* wl = nullptr;
    if ((rc = align_stage(c, ALW_IN0, row_doc, (size_t)n_rows * 4, &A.row_doc)) || (rc = align_stage(c, ALW_IN1, row_start, (size_t)n_rows * 4, &A.row_start)) ||
        (rc = align_stage(c, ALW_IN2, labels && word_labels ? word_labels + word_off[0] : nullptr, (size_t)in.n * 4, &wl)) ||
        (rc = align_stage(c, ALW_IN3, continuation == 2 ? cont_map : nullptr, (size_t)n_map * 4, &A.cont_map))) return rc;
    A.word_labels = wl ? wl - word_off[0] : nullptr;                          // (biased: indexed as the caller's array)
    const size_t cells = (size_t)n_rows * (size_t)max_len * 4;
    StagedOut S;
    S.add(word_ids, cells, true); S.add(labels, cells, true); S.add(n_real, (size_t)n_rows * 4, false);
    if ((rc = staged_ensure(c, S))) return rc;
    A.word_ids = S.dev(0); A.labels = S.dev(1); A.n_real = S.dev(2);
    if ((rc = align_launch_locked(c, A, (const int32_t*)in.d_payload))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)

int gz_span_labels_device(gz_ctx* c, const int32_t* span_dev, const int64_t* word_off_dev, int64_t n_docs, int64_t n_words, const int32_t* marks_dev,
                          const int64_t* mark_off_dev, int64_t n_marks, int32_t scheme, int32_t outside, int32_t* word_labels_dev, int32_t* mark_words_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = span_labels_fault(n_docs, scheme)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!word_off_dev || !mark_off_dev || n_words < 0 || n_marks < 0 || (n_words > 0 && !span_dev) || (n_marks > 0 && !marks_dev))
        return fail(c, GZ_E_INVALID, "bad arguments");
    if (n_words >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kSpanWordLimit);
    if (n_marks >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "span labels take fewer than 2^31 marks");
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_docs == 0 || (!word_labels_dev && !mark_words_dev)) return GZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->w_al[ALW_OWNER], (size_t)(n_words + 1) * 4))) return rc;
    GzSpanLabArgs A{span_dev, word_off_dev, n_docs, n_words, marks_dev, mark_off_dev, n_marks, scheme, outside,
                    word_labels_dev ? (uint32_t*)c->w_al[ALW_OWNER].p : nullptr, word_labels_dev, mark_words_dev};
    gz_launch_span_labels(A, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_span_labels(gz_ctx* c, const int32_t* span, const int64_t* word_off, int64_t n_docs, const int32_t* marks, const int64_t* mark_off, int32_t scheme,
                   int32_t outside, int32_t* word_labels, int32_t* mark_words)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = span_labels_fault(n_docs, scheme)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!word_off || !mark_off) return fail(c, GZ_E_INVALID, "bad arguments");
    RowsIn in{span, word_off, n_docs, 8}, mk{marks, mark_off, n_docs, 12};
    int rc;
    if ((rc = rows_check(c, in, kWordWords)) || (rc = rows_check(c, mk, kMarkWords))) return rc;
    if (in.n >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kSpanWordLimit);
    if (mk.n >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "span labels take fewer than 2^31 marks");
    if (const char* why = span_labels_data_fault(mk.n ? marks + 3 * mark_off[0] : nullptr, mk.n, scheme)) return fail(c, GZ_E_INVALID, "%s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_docs == 0) return GZ_OK;
    if ((rc = rows_stage(c, in, 0))) return rc;
    const int32_t* marks_dev = nullptr;
    const int64_t* moff_dev = nullptr;
    if ((rc = align_stage(c, ALW_IN0, mk.n ? marks + 3 * mark_off[0] : nullptr, (size_t)mk.n * 12, &marks_dev)) ||
        (rc = align_stage64(c, ALW_IN1, mark_off, (size_t)(n_docs + 1) * 8, &moff_dev)) || (rc = ensure(c, c->w_al[ALW_OWNER], (size_t)(in.n + 1) * 4))) return rc;
    StagedOut S;
    S.add(in.n ? word_labels : nullptr, (size_t)in.n * 4, true); S.add(mk.n ? mark_words : nullptr, (size_t)mk.n * 8, true);
    if (!S.e[0].host && !S.e[1].host) return GZ_OK;
    if ((rc = staged_ensure(c, S))) return rc;
    GzSpanLabArgs A{(const int32_t*)in.d_payload, in.d_off, n_docs, in.n, marks_dev ? marks_dev - 3 * mark_off[0] : nullptr, moff_dev, mk.n, scheme, outside,
                    S.dev(0) ? (uint32_t*)c->w_al[ALW_OWNER].p : nullptr, S.dev(0) ? S.dev(0) - word_off[0] : nullptr, S.dev(1)};
    gz_launch_span_labels(A, c->stream);
    return staged_copy_out(c, S);
} GZ_CATCH(c)

// ---- question-context windows with answer positions (gz_pairwin.inc) --------------------------------------------------------------
namespace {
constexpr RowsWords kQuestionWords{"bad question offsets", "question offsets must not decrease"};
struct PairWinOut {
    int32_t* ids; int32_t* mask; int32_t* type; int32_t* pair; int32_t* start; int32_t* n_real; int32_t* q_len;
    int32_t* start_pos; int32_t* end_pos; int32_t* has_answer;
};

// the geometry of a call and its inputs, every pointer a device pointer; bos / eos / pad are the context's current special ids
GzPairWinArgs pairwin_args(gz_ctx* c, const int32_t* q_ids, const int64_t* q_off, int64_t n_q, const int32_t* c_ids, const int64_t* c_off, int64_t n_rows,
                           const int32_t* q_row, const int32_t* ans, int32_t max_len, int32_t stride, int32_t max_q, int32_t skip_front, int32_t skip_back)
{
    GzPairWinArgs A{};
    A.q_ids = q_ids; A.q_off = q_off; A.n_q = n_q; A.c_ids = c_ids; A.c_off = c_off; A.n_rows = n_rows; A.q_row = q_row; A.ans = ans;
    A.max_len = max_len; A.stride = stride; A.max_q = max_q; A.skip_front = skip_front; A.skip_back = skip_back;
    A.bos_id = c->dev.bos_id; A.eos_id = c->dev.eos_id; A.pad_id = c->dev.pad_id;
    return A;
}

void pairwin_fill(gz_ctx* c, GzPairWinArgs A, const int64_t* win_off_dev, int64_t n_win, const PairWinOut& O)
{
    A.win_off = win_off_dev; A.n_win = n_win;
    A.out_ids = O.ids; A.out_mask = O.mask; A.out_type = O.type;
    A.win_pair = O.pair; A.win_start = O.start; A.win_n_real = O.n_real; A.win_q_len = O.q_len;
    A.start_pos = O.start_pos; A.end_pos = O.end_pos; A.has_answer = O.has_answer;
    gz_launch_pairwin_fill(A, c->stream);
}

// Both passes on the context's stream, behind whatever it holds.  *total = windows of the batch.  O.ids == nullptr: the count pass
// only.  A.pair_q is set here (the context's scratch: it lives from the count pass to the fill pass of the same call).
int pairwin_device_locked(gz_ctx* c, GzPairWinArgs& A, const PairWinOut& O, int64_t* win_off_dev, int64_t capacity, int64_t* total)
{
    if (!c->have_tables) return fail(c, GZ_E_NOTABLES, "gz_load_tables has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t cnt_bytes = (size_t)(A.n_rows + 2) * 8;
    if ((rc = ensure(c, c->w_pw_cnt, cnt_bytes + (size_t)(A.n_rows + 1) * 4))) return rc;
    A.pair_q = (int32_t*)((uint8_t*)c->w_pw_cnt.p + cnt_bytes);
    gz_launch_pairwin_count(A, (int64_t*)c->w_pw_cnt.p, win_off_dev, c->stream);
    if ((rc = read_total(c, A.n_rows > 0 ? win_off_dev + A.n_rows : nullptr, win_off_dev, total))) return rc;
    if (!O.ids) return GZ_OK;
    if (*total > capacity) return fail(c, GZ_E_CAPACITY, "the batch makes %lld windows, capacity is %lld", (long long)*total, (long long)capacity);
    pairwin_fill(c, A, win_off_dev, *total, O);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
}
}  // namespace

int gz_pair_window_rows_device(gz_ctx* c, const int32_t* q_ids_dev, const int64_t* q_off_dev, int64_t n_questions, const int32_t* ids_dev,
                               const int64_t* row_off_dev, int64_t n_rows, const int32_t* q_row_dev, const int32_t* ans_dev, int32_t max_len, int32_t stride,
                               int32_t max_query_len, int32_t skip_front, int32_t skip_back, int32_t* input_ids_dev, int32_t* attention_mask_dev,
                               int32_t* token_type_ids_dev, int32_t* win_pair_dev, int32_t* win_start_dev, int32_t* win_n_real_dev, int32_t* win_q_len_dev,
                               int32_t* start_pos_dev, int32_t* end_pos_dev, int32_t* has_answer_dev, int64_t* win_off_dev, int64_t capacity_windows,
                               int64_t* total_host)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = pairwin_fault(n_rows, n_questions, q_row_dev != nullptr, max_len, stride, max_query_len, skip_front, skip_back, capacity_windows))
        return fail(c, GZ_E_INVALID, "%s", why);
    if (!row_off_dev || !win_off_dev || !total_host || (n_questions > 0 && !q_off_dev)) return fail(c, GZ_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    GzPairWinArgs A = pairwin_args(c, q_ids_dev, q_off_dev, q_off_dev ? n_questions : 0, ids_dev, row_off_dev, n_rows, q_row_dev, ans_dev, max_len, stride,
                                   max_query_len, skip_front, skip_back);
    const PairWinOut O{input_ids_dev, attention_mask_dev, token_type_ids_dev, win_pair_dev, win_start_dev, win_n_real_dev, win_q_len_dev,
                       start_pos_dev, end_pos_dev, has_answer_dev};
    return pairwin_device_locked(c, A, O, win_off_dev, capacity_windows, total_host);
} GZ_CATCH(c)

int gz_pair_window_rows(gz_ctx* c, const int32_t* q_ids, const int64_t* q_off, int64_t n_questions, const int32_t* ids, const int64_t* row_off,
                        int64_t n_rows, const int32_t* q_row, const int32_t* ans, int32_t max_len, int32_t stride, int32_t max_query_len,
                        int32_t skip_front, int32_t skip_back, int32_t* input_ids, int32_t* attention_mask, int32_t* token_type_ids, int32_t* win_pair,
                        int32_t* win_start, int32_t* win_n_real, int32_t* win_q_len, int32_t* start_pos, int32_t* end_pos, int32_t* has_answer,
                        int64_t* win_off, int64_t capacity_windows, int64_t* total_host)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = pairwin_fault(n_rows, n_questions, q_row != nullptr, max_len, stride, max_query_len, skip_front, skip_back, capacity_windows))
        return fail(c, GZ_E_INVALID, "%s", why);
    if (!row_off || !win_off || !total_host || !q_off) return fail(c, GZ_E_INVALID, "bad arguments");
    RowsIn in{ids, row_off, n_rows, 4}, qs{q_ids, q_off, n_questions, 4};
    int rc;
    if ((rc = rows_check(c, in, kRowWords)) || (rc = rows_check(c, qs, kQuestionWords))) return rc;
    if (const char* why = pairwin_data_fault(q_row, n_rows, n_questions)) return fail(c, GZ_E_INVALID, "%s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = rows_stage(c, in, (size_t)(n_rows + 1) * 8))) return rc;                  // kept through both passes: win_off
    const int32_t *q_ids_dev = nullptr, *q_row_dev = nullptr, *ans_dev = nullptr;
    const int64_t* q_off_dev = nullptr;
    if ((rc = align_stage(c, ALW_IN0, qs.n ? q_ids + q_off[0] : nullptr, (size_t)qs.n * 4, &q_ids_dev)) ||
        (rc = align_stage64(c, ALW_IN1, q_off, (size_t)(n_questions + 1) * 8, &q_off_dev)) ||
        (rc = align_stage(c, ALW_IN2, n_rows ? q_row : nullptr, (size_t)n_rows * 4, &q_row_dev)) ||
        (rc = align_stage(c, ALW_IN3, n_rows ? ans : nullptr, (size_t)n_rows * 8, &ans_dev))) return rc;
    GzPairWinArgs A = pairwin_args(c, q_ids_dev ? q_ids_dev - q_off[0] : nullptr, q_off_dev, n_questions, (const int32_t*)in.d_payload, in.d_off, n_rows,
                                   q_row_dev, ans_dev, max_len, stride, max_query_len, skip_front, skip_back);       // (biased: indexed as the caller's array)
    int64_t* const woff = (int64_t*)in.d_keep;
    int64_t total = 0;
    if ((rc = pairwin_device_locked(c, A, PairWinOut{}, woff, 0, &total))) return rc;
    *total_host = total;
    if ((rc = copy_out(c, win_off, woff, (size_t)(n_rows + 1) * 8, c->stream))) return rc;
    if (!input_ids) return GZ_OK;
    if (total > capacity_windows)
        return fail(c, GZ_E_CAPACITY, "the batch makes %lld windows, capacity is %lld", (long long)total, (long long)capacity_windows);
    if (total == 0) return GZ_OK;
    const size_t cells = (size_t)total * (size_t)max_len * 4, per_win = (size_t)total * 4;
    StagedOut S;
    S.add(input_ids, cells, true); S.add(attention_mask, cells, true); S.add(token_type_ids, cells, true);
    S.add(win_pair, per_win, false); S.add(win_start, per_win, false); S.add(win_n_real, per_win, false); S.add(win_q_len, per_win, false);
    S.add(ans ? start_pos : nullptr, per_win, false); S.add(ans ? end_pos : nullptr, per_win, false); S.add(ans ? has_answer : nullptr, per_win, false);
    if ((rc = staged_ensure(c, S))) return rc;
    pairwin_fill(c, A, woff, total, PairWinOut{S.dev(0), S.dev(1), S.dev(2), S.dev(3), S.dev(4), S.dev(5), S.dev(6), S.dev(7), S.dev(8), S.dev(9)});
    return staged_copy_out(c, S);
} GZ_CATCH(c)

namespace {
// the scan and the one launch on the context's stream; every pointer a device pointer
int span_tokens_launch_locked(gz_ctx* c, GzSpanTokArgs A, const int32_t* counts_dev)
{
    int rc;
    if ((rc = ensure(c, c->w_pw_tok, (size_t)(2 * A.n_words + 4) * 8))) return rc;
    int64_t* const cnt64 = (int64_t*)c->w_pw_tok.p;
    gz_launch_span_tokens(A, counts_dev, cnt64, cnt64 + A.n_words + 1, c->stream);
    return GZ_OK;
}
}  // namespace

int gz_span_tokens_device(gz_ctx* c, const int32_t* counts_dev, const int64_t* word_off_dev, int64_t n_docs, int64_t n_words, const int32_t* mark_words_dev,
                          const int64_t* mark_off_dev, int64_t n_marks, int32_t* span_tokens_dev)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = span_tokens_fault(n_docs)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!word_off_dev || !mark_off_dev || n_words < 0 || n_marks < 0 || (n_words > 0 && !counts_dev) || (n_marks > 0 && (!mark_words_dev || !span_tokens_dev)))
        return fail(c, GZ_E_INVALID, "bad arguments");
    if (n_words >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kSpanWordLimit);
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_docs == 0 || n_marks == 0) return GZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = span_tokens_launch_locked(c, GzSpanTokArgs{word_off_dev, n_docs, n_words, mark_words_dev, mark_off_dev, n_marks, nullptr, span_tokens_dev}, counts_dev)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return GZ_OK;
} GZ_CATCH(c)

int gz_span_tokens(gz_ctx* c, const int32_t* counts, const int64_t* word_off, int64_t n_docs, const int32_t* mark_words, const int64_t* mark_off,
                   int32_t* span_tokens)
try {
    if (!c) return GZ_E_INVALID;
    if (const char* why = span_tokens_fault(n_docs)) return fail(c, GZ_E_INVALID, "%s", why);
    if (!word_off || !mark_off) return fail(c, GZ_E_INVALID, "bad arguments");
    RowsIn in{counts, word_off, n_docs, 4}, mk{mark_words, mark_off, n_docs, 8};
    int rc;
    if ((rc = rows_check(c, in, kWordWords)) || (rc = rows_check(c, mk, kMarkWords))) return rc;
    if (in.n >= ((int64_t)1 << 31)) return fail(c, GZ_E_LIMIT, "%s", kSpanWordLimit);
    if (mk.n > 0 && !span_tokens) return fail(c, GZ_E_INVALID, "bad arguments");
    if (const char* why = span_tokens_data_fault(in.n ? counts + word_off[0] : nullptr, in.n, mk.n ? mark_words : nullptr, mk.n)) return fail(c, GZ_E_INVALID, "%s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_docs == 0 || mk.n == 0) return GZ_OK;
    if ((rc = rows_stage(c, in, 0))) return rc;
    const int32_t* mw_dev = nullptr;
    const int64_t* moff_dev = nullptr;
    if ((rc = align_stage(c, ALW_IN0, mark_words, (size_t)mk.n * 8, &mw_dev)) || (rc = align_stage64(c, ALW_IN1, mark_off, (size_t)(n_docs + 1) * 8, &moff_dev)))
        return rc;
    StagedOut S;
    S.add(span_tokens, (size_t)mk.n * 8, true);
    if ((rc = staged_ensure(c, S))) return rc;
    if ((rc = span_tokens_launch_locked(c, GzSpanTokArgs{in.d_off, n_docs, in.n, mw_dev, moff_dev, mk.n, nullptr, S.dev(0)}, (const int32_t*)in.d_payload))) return rc;
    return staged_copy_out(c, S);
} GZ_CATCH(c)
