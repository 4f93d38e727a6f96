"""BM25 index / scoring timings on the configs[2] corpus (genz_tokenize.ranking, csrc/gz_bm25.inc).

    python tools/bm25_bench.py [--docs 1000000] [--reps 5] [--remove 10000] [--compact 10000] [--out profiles/bm25_bench.json]
    python tools/bm25_bench.py --search-only [--out profiles/bm25_bench.json]
    python tools/bm25_bench.py --phrase-only [--out profiles/bm25_bench.json]
    python tools/bm25_bench.py --vocab-only [--out profiles/bm25_bench.json]
    python tools/bm25_bench.py --snippet-only [--out profiles/bm25_bench.json]
    python tools/bm25_bench.py --near-only [--out profiles/bm25_bench.json]
    python tools/bm25_bench.py --groups-only [--out profiles/bm25_bench.json]

Host clock around call + synchronisation, after a warm-up call, median of --reps:
  build_device_ms      gz_bm25_build_device over text and offsets already in HBM (the call returns a finished index)
  score_q{1,64,256}_ms scoring Q queries of 8 words into device memory (gz_bm25_score_device + gz_sync)
  topk_q{1,64,256}_k{10,1000}_ms  the k best documents of Q queries into device memory (gz_bm25_topk_device + gz_sync): scoring,
                       a chunk of queries at a time, and the selection levels
Search (gz_bm25_search_device / gz_bm25_match_count; --search-only: the build, these rows and topk_q*_k10_ms alone, and with --out
they are merged into the file's record instead of replacing it):
  postings_build_ms    the first gz_bm25_match_count (one query of one absent word) on a freshly built index: the postings build plus
                       the marking and counting of that one empty row (the index build is not timed)
  search_q{1,64,256}_k10_ms        the 10 best MATCHING documents of the same Q queries into device memory, and the match counts
                       (gz_bm25_search_device + gz_sync), after a warm call that has built the postings
  search_rare_q{1,64,256}_k10_ms   the same for a second query set: 8 words each with 1 <= df <= N / 1000, drawn with a fixed seed
  topk_rare_q{1,64,256}_k10_ms     gz_bm25_topk_device over the rare-word queries (top_k's time does not depend on the words)
  match_fraction / match_fraction_rare   mean(count) / N over the 256 queries of each set
  search_drawn_q{1,64,256}_k10_ms  the same for a third query set, "drawn": 256 queries of 2-4 distinct words, each query's words taken
                       from one document (fixed seed), mode "any": gz_bm25_search_device, the path of the rows above
  search_all_drawn_q{1,64,256}_k10_ms  the drawn queries in mode "all" (gz_bm25_search_bool_device, GZ_BM25_MATCH_ALL): every word must
                       occur.  The two are timed in the same loop, alternating, after a warm call of each; the spread of the "any"
                       row's own repetitions (search_drawn_*_all_ms) is the margin below which a difference is none
  match_fraction_drawn / match_fraction_all_drawn   mean(count) / N over the 256 drawn queries, modes "any" and "all"
  ctor_ms              the Python constructor BM25(list of str): packing, host -> device, build, fieldLens, avgFieldLen
  topk_host_q256_k100_ms           BM25.top_k(256 queries, 100): ids and scores [256, 100] in host memory
  get_scores_host_q256_ms          BM25.get_scores(256 queries): the float64 [256, N] matrix in host memory
  get_scores_argpartition_q256_k100_ms  the same followed by np.argpartition and a sort of the 100 per row (what a caller does
                       without top_k; --host-reps reps)
Append (gz_bm25_append_device / BM25.add_documents; --append documents behind the --docs of the corpus, 0 skips these rows):
  append_device_ms     the batch, text and offsets already in HBM, behind an index of --docs documents whose buffers have the room:
                       --docs - --append documents are built, the batch before ours is appended (every buffer that grows doubles),
                       then ours is timed
  append_device_grow_ms  the same batch as the FIRST append to a freshly built index: its tail buffers (text, dl, signatures, eoff,
                       entries, term ranges, df) are full, so all of them grow; append_grow_tables says whether the two tables did
  append_python_ms     BM25.add_documents(list of --append str) on a model of --docs documents (first append: buffers grow)
  rebuild_device_ms    gz_bm25_build_device over the --docs + --append documents: what a caller paid before
  incremental_build_ms an index of --docs documents made by --docs / --append appends to an empty one (device text)
Remove (gz_bm25_remove_device / BM25.remove_documents; --remove random documents out of the --docs of the corpus, 0 skips these rows):
  remove_device_ms     the ids already in HBM, out of a freshly built index of --docs documents (the build is not timed)
  remove_python_ms     BM25.remove_documents(list of the same ids) on a model of --docs documents
  rebuild_remaining_device_ms  gz_bm25_build_device over the remaining --docs - --remove documents, text and offsets in HBM: what a
                       caller paid before, timed in the same run
Compact (gz_bm25_compact / gz_bm25_terms; --compact random documents are removed from the --docs of the corpus first, 0 skips these
rows; --compact-only: these rows alone, and with --out they are merged into the file's record instead of replacing it):
  compact_device_ms    gz_bm25_compact on an index of --docs documents after gz_bm25_remove_device of --compact ids (build and
                       removal are not timed)
  terms_device_ms      gz_bm25_terms on the same index before it is compacted: both calls of the sizes-first protocol, the numbering
                       on the device each time, offsets, df and bytes into host memory
  rebuild_remaining_device_ms  as in the remove rows, alternating with the two above in the same process (compact_over_rebuild is
                       taken against THIS run's figure; compact_bar_met: compact_device_ms below it)
  footprint_before / footprint_after  gz_bm25_footprint (text bytes in use, terms in the table, device bytes) around the compaction
  restate_q64_ms       the numpy restatement (tests/bm25_restate.py) scoring 64 queries on the host, on --restate-docs documents,
                       its postings built beforehand (not timed)
Phrase (gz_bm25_build_device_ex with GZ_BM25_POSITIONS, gz_bm25_search_phrase_device; --phrase-only: these rows alone, and with --out
they are merged into the file's record instead of replacing it):
  phrase_build_device_ms / phrase_build_positions_device_ms  gz_bm25_build_device[_ex] without and with positions, alternating in
                       one loop; phrase_device_bytes / phrase_positions_device_bytes: gz_bm25_footprint's device bytes of each
  phrase_all_q256_k10_ms   256 queries of two words -- two neighbouring words of one document each (fixed seed) -- in mode "all" without
                       a phrase (gz_bm25_search_bool_device + gz_sync): what the index could answer before.  A library without the
                       phrase entry points (an older build through GZ_LIBRARY) gives this row and the plain build alone
  phrase_search_q256_k10_ms  the same queries in mode "all" with the two words as the phrase (gz_bm25_search_phrase_device), timed
                       in the same loop, alternating with the row above, after a warm call of each that has derived the word offsets
  phrase_any_q256_k10_ms   the same with mode "any": every document with one of the two words is marked and goes through the phrase step
  phrase_match_fraction_all / _phrase / _any_phrase   mean(count) / N over the 256 queries
Snippets (BM25(..., positions=True).snippets / occurrences, gz_bm25_snippets_device; --snippet-only: these rows alone, and with --out
they are merged into the file's record instead of replacing it).  The model is BM25(list of str, positions=True) over the corpus; the
256 "drawn" queries (2-4 distinct words of one document each, fixed seed) and ids = search(queries, k)[0] for k = 10 and k = 1000;
width 32:
  snippet_device_q256_k{10,1000}_ms   gz_bm25_snippets_device + gz_sync, the ids already in HBM (what gz_bm25_search_device wrote)
  snippet_python_q256_k{10,1000}_ms   BM25.snippets(queries, ids, 32): terms looked up, ids in, starts and hits [256, k] out
  occurrences_python_q256_k{10,1000}_ms   BM25.occurrences(queries, ids): both calls of the sizes-first protocol
  snippet_host_loop_q256_k{10,1000}_ms    the host route they replace: texts[d].split() and the definition's loop over the starts for
                       every pair, plain Python (one repetition; k = 1000 only when the k = 10 figure scaled to its pairs stays under a minute)
  snippet_pairs_k* / snippet_pair_words_k* / occurrences_total_k*   pairs with a document, the words of their documents, all occurrences
Proximity (gz_bm25_search_near_device, gz_bm25_cover_device; --near-only: the phrase rows above and these, in one invocation and one
timing loop, and with --out they are merged into the file's record instead of replacing it).  The 256 two-word queries of the phrase
rows, the two words as the near set, window 8:
  near_all_w8_q256_k10_ms  mode "all" with the near set (gz_bm25_search_near_device + gz_sync), alternating with the phrase rows
  near_any_w8_q256_k10_ms  the same with mode "any": every document with one of the two words is marked and goes through the near step
  near_match_fraction_all / _any   mean(count) / N over the 256 queries
  cover_device_q256_k{10,1000}_ms  gz_bm25_cover_device + gz_sync over the ids that the mode "any" near search with that k left in HBM
  cover_pairs_k* / cover_pair_words_k*   pairs with a document, the words of their documents
Vocabulary (gz_bm25_similar, gz_bm25_prefix, gz_bm25_term_bytes; --vocab-only: these rows alone, and with --out they are merged into the
file's record instead of replacing it).  The index is gz_bm25_build_device over the corpus; the W words are terms of the vocabulary
(fixed seed) with one random edit each -- a code point substituted, deleted or inserted; a host clock around the call (its outputs
are on the host when it returns):
  vocab_similar_w{1,64,256}_ms   gz_bm25_similar, max_edits 2, k 10
  vocab_prefix_w{1,64,256}_ms    gz_bm25_prefix over the first three code points of the same words, k 10
  vocab_term_texts_w{1,64,256}_ms  gz_bm25_term_bytes of the W * 10 ids the similar call returned: both calls of the sizes-first protocol
  vocab_host_read_ms / vocab_host_loop_w1_ms   the host route they replace: gz_bm25_terms into a list of str, and one word against it in
                       plain Python (terms whose length differs by more than 2 skipped, a two-row Levenshtein for the rest; one repetition)
  vocab_similar_ms_per_word_w64 / _w256, vocab_key_rows_per_chunk, vocab_key_bytes   time / W, and the key rows held at a time:
                       min(W, max(1, 2^23 // terms)) rows of terms doubles (switch bm25_vocab_chunk)
Word groups (gz_bm25_search_groups_device; --groups-only: these rows alone, and with --out they are merged into the file's record
instead of replacing it).  The index is gz_bm25_build_device over the corpus; 256 queries of 2-4 distinct words, the first words of
documents drawn with a fixed seed; k = 10, outputs in HBM, gz_sync before the clock stops; the four calls of a case are interleaved
in every repetition.  An older build (through GZ_LIBRARY) gives the plain rows alone:
  groups_groups_single_{any,all}_q256_k10_ms   every word a group of its own ...
  groups_plain_single_{any,all}_q256_k10_ms    ... against gz_bm25_search[_bool]_device over the same words
  groups_groups_alt8_{any,all}_q256_k10_ms     every word a group of up to 8 alternatives: the word and its nearest terms
                       (gz_bm25_similar, max_edits 2), with the group's df from gz_bm25_match_count ...
  groups_plain_alt8_{any,all}_q256_k10_ms      ... against the plain search over the flattened alternatives as words: mode "any" marks
                       the same postings and probes as many (candidate, term) pairs; mode "all" there demands every spelling at once,
                       marks one word's postings and finds next to nothing -- it is no like-for-like row
  groups_*_match_fraction   mean(count) / N of each;  groups_alt8_mean_size   alternatives a group
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--reps 2)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "genz-tokenize_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import corpus  # noqa: E402
from genz_tokenize import _native  # noqa: E402
from genz_tokenize._packing import pack  # noqa: E402
from genz_tokenize.ranking import BM25  # noqa: E402


def median_ms(fn, reps):
    fn()                                                             # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def append_rows(ctx, res, n, batch, reps):
    """the append rows of the docstring: the corpus is n + batch documents"""
    t, o, _ = corpus.config_corpus(2, n_docs=n + batch)
    nbytes = int(o[-1])
    d_text, d_off = ctx.alloc(nbytes), ctx.alloc(8 * (n + batch + 1))
    ctx.h2d(d_text, t)
    ctx.h2d(d_off, o)
    # the batch's offsets are absolute in d_text: the entry point takes them from any base
    d_boff = d_off + 8 * n
    bbytes = int(o[-1] - o[n])
    d_poff = d_off + 8 * (n - batch)                                 # the batch before it
    pbytes = int(o[n] - o[n - batch])
    res.update(append_docs=batch, append_bytes=bbytes)

    ts = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        ix = ctx.bm25_build_device(d_text, d_off, n + batch, nbytes)
        ts.append((time.perf_counter() - t0) * 1e3)
        ctx.bm25_destroy(ix)
    res["rebuild_device_ms"], res["rebuild_device_all_ms"] = float(np.median(ts[1:])), [round(x, 3) for x in ts[1:]]

    grow, room = [], []
    for k in range(reps + 1):
        # growth: the first append to a fresh index of n documents
        ix = ctx.bm25_build_device(d_text, d_off, n, int(o[n]))
        t0 = time.perf_counter()
        ctx.bm25_append_device(ix, d_text, d_boff, batch, bbytes)
        grow.append((time.perf_counter() - t0) * 1e3)
        assert ctx.bm25_info(ix)[0] == n + batch
        ctx.bm25_destroy(ix)
        # capacity present: n - batch documents built, the batch before ours appended (every buffer doubles), then ours
        ix = ctx.bm25_build_device(d_text, d_off, n - batch, int(o[n - batch]))
        ctx.bm25_append_device(ix, d_text, d_poff, batch, pbytes)
        t0 = time.perf_counter()
        ctx.bm25_append_device(ix, d_text, d_boff, batch, bbytes)
        room.append((time.perf_counter() - t0) * 1e3)
        info = ctx.bm25_info(ix)
        ctx.bm25_destroy(ix)
    res["append_device_ms"], res["append_device_all_ms"] = float(np.median(room[1:])), [round(x, 3) for x in room[1:]]
    res["append_device_grow_ms"], res["append_device_grow_all_ms"] = float(np.median(grow[1:])), [round(x, 3) for x in grow[1:]]
    res["append_over_rebuild"] = round(res["append_device_ms"] / res["rebuild_device_ms"], 3)
    res["append_terms"], res["append_words"] = info[1:]

    # the whole index by appends of `batch` to an empty one
    e_off = ctx.alloc(8)
    ctx.h2d(e_off, np.zeros(1, np.int64))
    ts = []
    for k in range(min(reps, 3)):
        t0 = time.perf_counter()
        ix = ctx.bm25_build_device(None, e_off, 0, 0)
        for i in range(0, n, batch):
            m = min(batch, n - i)
            ctx.bm25_append_device(ix, d_text, d_off + 8 * i, m, int(o[i + m] - o[i]))
        ts.append((time.perf_counter() - t0) * 1e3)
        assert ctx.bm25_info(ix)[0] == n
        ctx.bm25_destroy(ix)
    res["incremental_build_ms"], res["incremental_build_all_ms"] = float(np.median(ts)), [round(x, 3) for x in ts]
    res["incremental_appends"] = (n + batch - 1) // batch
    for d in (e_off, d_text, d_off):
        ctx.free(d)

    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n + batch)]
    old, more = docs[:n], docs[n:]
    ts = []
    for k in range(min(reps, 3) + 1):
        m = BM25(old, ctx=ctx)
        t0 = time.perf_counter()
        m.add_documents(more)
        ts.append((time.perf_counter() - t0) * 1e3)
        del m
    res["append_python_ms"], res["append_python_all_ms"] = float(np.median(ts[1:])), [round(x, 3) for x in ts[1:]]


def remove_rows(ctx, res, n, k, reps):
    """the remove rows of the docstring"""
    t, o, _ = corpus.config_corpus(2, n_docs=n)
    nbytes = int(o[-1])
    ids = np.sort(np.random.default_rng(2).choice(n, size=k, replace=False)).astype(np.int64)
    keep = np.ones(n, bool)
    keep[ids] = False
    lens = np.diff(o)
    # the remaining documents, packed on the host (not timed), for the rebuild
    r_off = np.zeros(n - k + 1, np.int64)
    np.cumsum(lens[keep], out=r_off[1:])
    r_text = t[np.repeat(keep, lens)]
    assert len(r_text) == int(r_off[-1])
    d_text, d_off, d_ids = ctx.alloc(nbytes), ctx.alloc(8 * (n + 1)), ctx.alloc(8 * k)
    d_rtext, d_roff = ctx.alloc(max(len(r_text), 16)), ctx.alloc(8 * (n - k + 1))
    for d, h in ((d_text, t), (d_off, o), (d_ids, ids), (d_rtext, r_text), (d_roff, r_off)):
        ctx.h2d(d, h)
    res.update(remove_docs=k)
    rm, rb = [], []
    for _ in range(reps + 1):                                        # (the first of each is the warm-up)
        ix = ctx.bm25_build_device(d_text, d_off, n, nbytes)
        t0 = time.perf_counter()
        ctx.bm25_remove_device(ix, d_ids, k)
        rm.append((time.perf_counter() - t0) * 1e3)
        info = ctx.bm25_info(ix)
        ctx.bm25_destroy(ix)
        t0 = time.perf_counter()
        ix = ctx.bm25_build_device(d_rtext, d_roff, n - k, int(r_off[-1]))
        rb.append((time.perf_counter() - t0) * 1e3)
        assert ctx.bm25_info(ix) == info                             # documents, live terms and words of the fresh build
        ctx.bm25_destroy(ix)
    res["remove_device_ms"], res["remove_device_all_ms"] = float(np.median(rm[1:])), [round(x, 3) for x in rm[1:]]
    res["rebuild_remaining_device_ms"], res["rebuild_remaining_device_all_ms"] = float(np.median(rb[1:])), [round(x, 3) for x in rb[1:]]
    res["remove_over_rebuild"] = round(res["remove_device_ms"] / res["rebuild_remaining_device_ms"], 3)
    for d in (d_text, d_off, d_ids, d_rtext, d_roff):
        ctx.free(d)
    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n)]
    id_list = ids.tolist()
    ts = []
    for _ in range(min(reps, 3) + 1):
        m = BM25(docs, ctx=ctx)
        t0 = time.perf_counter()
        m.remove_documents(id_list)
        ts.append((time.perf_counter() - t0) * 1e3)
        del m
    res["remove_python_ms"], res["remove_python_all_ms"] = float(np.median(ts[1:])), [round(x, 3) for x in ts[1:]]


def compact_rows(ctx, res, n, k, reps):
    """the compact rows of the docstring"""
    t, o, _ = corpus.config_corpus(2, n_docs=n)
    nbytes = int(o[-1])
    ids = np.sort(np.random.default_rng(2).choice(n, size=k, replace=False)).astype(np.int64)
    keep = np.ones(n, bool)
    keep[ids] = False
    lens = np.diff(o)
    r_off = np.zeros(n - k + 1, np.int64)
    np.cumsum(lens[keep], out=r_off[1:])
    r_text = t[np.repeat(keep, lens)]
    d_text, d_off, d_ids = ctx.alloc(nbytes), ctx.alloc(8 * (n + 1)), ctx.alloc(8 * k)
    d_rtext, d_roff = ctx.alloc(max(len(r_text), 16)), ctx.alloc(8 * (n - k + 1))
    for d, h in ((d_text, t), (d_off, o), (d_ids, ids), (d_rtext, r_text), (d_roff, r_off)):
        ctx.h2d(d, h)
    res.update(compact_removed_docs=k)
    cp, tm, rb = [], [], []
    for _ in range(reps + 1):                                        # (the first of each is the warm-up)
        ix = ctx.bm25_build_device(d_text, d_off, n, nbytes)
        ctx.bm25_remove_device(ix, d_ids, k)
        before = ctx.bm25_footprint(ix)
        t0 = time.perf_counter()
        off, data, df = ctx.bm25_terms(ix)
        tm.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctx.bm25_compact(ix)
        cp.append((time.perf_counter() - t0) * 1e3)
        after, info = ctx.bm25_footprint(ix), ctx.bm25_info(ix)
        assert after[0] == int(off[-1]) == len(data) and after[1] == info[1] == len(df)
        ctx.bm25_destroy(ix)
        t0 = time.perf_counter()
        ix = ctx.bm25_build_device(d_rtext, d_roff, n - k, int(r_off[-1]))
        rb.append((time.perf_counter() - t0) * 1e3)
        assert ctx.bm25_info(ix) == info                             # documents, live terms and words of the fresh build
        ctx.bm25_destroy(ix)
    res["compact_device_ms"], res["compact_device_all_ms"] = float(np.median(cp[1:])), [round(x, 3) for x in cp[1:]]
    res["terms_device_ms"], res["terms_device_all_ms"] = float(np.median(tm[1:])), [round(x, 3) for x in tm[1:]]
    res["rebuild_remaining_device_ms"], res["rebuild_remaining_device_all_ms"] = float(np.median(rb[1:])), [round(x, 3) for x in rb[1:]]
    res["compact_over_rebuild"] = round(res["compact_device_ms"] / res["rebuild_remaining_device_ms"], 3)
    res["compact_bar_met"] = bool(res["compact_device_ms"] < res["rebuild_remaining_device_ms"])
    res["footprint_before"], res["footprint_after"] = list(before), list(after)
    for d in (d_text, d_off, d_ids, d_rtext, d_roff):
        ctx.free(d)


def search_rows(ctx, res, ix, n, d_text, d_off, nbytes, terms, idf, params, d_ids, d_sc, reps, drawn=None):
    """the search rows of the docstring; ix is the built index, terms / idf the 256 x 8 words of the tool's own queries, drawn =
    (terms, idf, offsets) of the 256 drawn queries (None: a library without gz_bm25_search_bool, their rows are left out)"""
    ts = []
    qoff1 = np.array([0, 1], np.int64)
    for _ in range(reps + 1):                                        # (the first is the warm-up)
        fresh = ctx.bm25_build_device(d_text, d_off, n, nbytes)
        t0 = time.perf_counter()
        ctx.bm25_match_count(fresh, np.array([-1], np.int32), qoff1)
        ts.append((time.perf_counter() - t0) * 1e3)
        ctx.bm25_destroy(fresh)
    res["postings_build_ms"], res["postings_build_all_ms"] = float(np.median(ts[1:])), [round(x, 3) for x in ts[1:]]
    # the rare-word set: 8 words each with 1 <= df <= N / 1000
    off, data, df = ctx.bm25_terms(ix)
    rare = np.flatnonzero((df >= 1) & (df <= max(1, n // 1000)))
    pick = np.random.default_rng(2).choice(rare, size=256 * 8, replace=True)
    raw = data.tobytes()
    rb, ro = pack([raw[int(off[i]):int(off[i + 1])].decode("utf-8", "surrogatepass") for i in pick])
    rterms, rdf = ctx.bm25_lookup(ix, rb, ro)
    assert (rterms >= 0).all() and np.array_equal(rdf, df[pick])
    ridf = np.array([np.log(1+(n-int(d)+0.5)/(int(d)+0.5)) for d in rdf])
    res["rare_df_max"], res["rare_df_mean"] = int(rdf.max()), round(float(rdf.mean()), 1)
    d_cnt = ctx.alloc(256 * 8)
    for name, tt, ii in (("", terms, idf), ("rare_", rterms, ridf)):
        for q in (1, 64, 256):
            qoff = np.arange(q + 1, dtype=np.int64) * 8

            def search():
                ctx.bm25_search(ix, tt[:8 * q], ii[:8 * q], qoff, params, False, 10, d_ids=d_ids, d_scores=d_sc, d_counts=d_cnt)
                ctx.sync()
            key = "search_%sq%d_k10" % (name, q)
            res[key + "_ms"], res[key + "_all_ms"] = median_ms(search, reps)
            if name:
                def topk():
                    ctx.bm25_topk(ix, tt[:8 * q], ii[:8 * q], qoff, params, False, 10, d_ids=d_ids, d_scores=d_sc)
                    ctx.sync()
                res["topk_rare_q%d_k10_ms" % q], res["topk_rare_q%d_k10_all_ms" % q] = median_ms(topk, reps)
        cnt = np.empty(256, np.int64)
        ctx.d2h(cnt, d_cnt)
        res["match_fraction" + ("_rare" if name else "")] = float(cnt.mean() / n)
    for q in (1, 64, 256) if drawn is not None else ():
        dterms, didf, doff = drawn
        qoff = doff[:q + 1]
        ts = {0: [], 1: []}
        for rep in range(reps + 1):                                  # (the first round is the warm-up of both)
            for mode in (0, 1):
                t0 = time.perf_counter()
                ctx.bm25_search(ix, dterms, didf, qoff, params, False, 10, d_ids=d_ids, d_scores=d_sc, d_counts=d_cnt, mode=mode)
                ctx.sync()
                if rep:
                    ts[mode].append((time.perf_counter() - t0) * 1e3)
                if q == 256 and rep == reps:
                    cnt = np.empty(256, np.int64)
                    ctx.d2h(cnt, d_cnt)
                    res["match_fraction_all_drawn" if mode else "match_fraction_drawn"] = float(cnt.mean() / n)
        for mode, key in ((0, "search_drawn_q%d_k10" % q), (1, "search_all_drawn_q%d_k10" % q)):
            res[key + "_ms"], res[key + "_all_ms"] = float(np.median(ts[mode])), [round(x, 3) for x in ts[mode]]
    ctx.free(d_cnt)
    for q in (1, 64, 256):
        res["search_q%d_k10_over_topk" % q] = round(res["search_q%d_k10_ms" % q] / res["topk_q%d_k10_ms" % q], 3)
        res["search_rare_q%d_k10_over_topk" % q] = round(res["search_rare_q%d_k10_ms" % q] / res["topk_rare_q%d_k10_ms" % q], 3)


def phrase_rows(ctx, res, t, o, reps, near=False):
    """the phrase rows of the docstring; near: the proximity rows beside them"""
    n, nbytes = len(o) - 1, int(o[-1])
    new = hasattr(ctx.lib, "gz_bm25_search_phrase_device")
    d_text, d_off = ctx.alloc(nbytes), ctx.alloc(8 * (n + 1))
    ctx.h2d(d_text, t)
    ctx.h2d(d_off, o)
    ts = {False: [], True: []}
    kept = {}
    for rep in range(reps + 1):                                      # (the first round is the warm-up of both)
        for pos in (False, True) if new else (False,):
            t0 = time.perf_counter()
            ix = ctx.bm25_build_device(d_text, d_off, n, nbytes, positions=True) if pos else ctx.bm25_build_device(d_text, d_off, n, nbytes)
            if rep:
                ts[pos].append((time.perf_counter() - t0) * 1e3)
            if rep == reps:
                kept[pos] = ix
            else:
                ctx.bm25_destroy(ix)
    res["phrase_build_device_ms"], res["phrase_build_device_all_ms"] = float(np.median(ts[False])), [round(x, 3) for x in ts[False]]
    res["phrase_device_bytes"] = ctx.bm25_footprint(kept[False])[2]
    if new:
        res["phrase_build_positions_device_ms"] = float(np.median(ts[True]))
        res["phrase_build_positions_device_all_ms"] = [round(x, 3) for x in ts[True]]
        res["phrase_positions_device_bytes"] = ctx.bm25_footprint(kept[True])[2]
        ctx.bm25_destroy(kept[False])
    ix = kept[new]
    raw = t.tobytes()
    rng = np.random.default_rng(5)
    pairs = []
    while len(pairs) < 256:
        i = int(rng.integers(n))
        ws = raw[o[i]:o[i + 1]].decode("utf-8").split()
        if len(ws) >= 2:
            j = int(rng.integers(len(ws) - 1))
            pairs.append(ws[j:j + 2])
    wb, wo = pack([w for p in pairs for w in p])
    terms, df = ctx.bm25_lookup(ix, wb, wo)
    assert (terms >= 0).all()
    idf = np.array([np.log(1+(n-int(d)+0.5)/(int(d)+0.5)) for d in df])
    qoff = np.arange(257, dtype=np.int64) * 2
    lens = ctx.bm25_field_lengths(ix)
    params = [2.2, 1.2, 0.25, 0.75, float(np.mean(lens)), 0.0]
    d_ids, d_sc, d_cnt = ctx.alloc(256 * 10 * 8), ctx.alloc(256 * 10 * 8), ctx.alloc(256 * 8)
    rows = [("phrase_all_q256_k10", 1, False, "phrase_match_fraction_all")]
    if new:
        rows += [("phrase_search_q256_k10", 1, True, "phrase_match_fraction_phrase"), ("phrase_any_q256_k10", 0, True, "phrase_match_fraction_any_phrase")]
    near = near and hasattr(ctx.lib, "gz_bm25_search_near_device")
    near_kw = dict(nr_terms=terms, nr_off=qoff, nr_window=np.full(256, 8, np.int64))
    if near:
        rows += [("near_all_w8_q256_k10", 1, "near", "near_match_fraction_all"), ("near_any_w8_q256_k10", 0, "near", "near_match_fraction_any")]
    ts = {r[0]: [] for r in rows}
    for rep in range(reps + 1):                                      # (the first round is the warm-up of all)
        for key, mode, phrase, frac in rows:
            kw = near_kw if phrase == "near" else dict(ph_terms=terms, ph_off=qoff) if phrase else {}
            t0 = time.perf_counter()
            ctx.bm25_search(ix, terms, idf, qoff, params, False, 10, d_ids=d_ids, d_scores=d_sc, d_counts=d_cnt, mode=mode, **kw)
            ctx.sync()
            if rep:
                ts[key].append((time.perf_counter() - t0) * 1e3)
            if rep == reps:
                cnt = np.empty(256, np.int64)
                ctx.d2h(cnt, d_cnt)
                res[frac] = float(cnt.mean() / n)
                if phrase:
                    assert (cnt >= 1).all()                          # (every phrase was taken from a document)
    for key, _, _, _ in rows:
        res[key + "_ms"], res[key + "_all_ms"] = float(np.median(ts[key])), [round(x, 3) for x in ts[key]]
    if new:
        res["phrase_over_all"] = round(res["phrase_search_q256_k10_ms"] / res["phrase_all_q256_k10_ms"], 3)
    if near:
        res["near_all_over_phrase"] = round(res["near_all_w8_q256_k10_ms"] / res["phrase_search_q256_k10_ms"], 3)
        res["near_any_over_phrase_any"] = round(res["near_any_w8_q256_k10_ms"] / res["phrase_any_q256_k10_ms"], 3)
        for k in (10, 1000):
            c_ids, c_sc = ctx.alloc(256 * k * 8), ctx.alloc(256 * k * 8)
            c_out = [ctx.alloc(256 * k * 4) for _ in range(3)]
            ctx.bm25_search(ix, terms, idf, qoff, params, False, k, d_ids=c_ids, d_scores=c_sc, d_counts=d_cnt, mode=0, **near_kw)
            ctx.sync()

            def cover():
                ctx.bm25_cover_device(ix, terms, qoff, c_ids, k, *c_out)
                ctx.sync()
            res["cover_device_q256_k%d_ms" % k], res["cover_device_q256_k%d_all_ms" % k] = median_ms(cover, reps)
            ids = np.empty(256 * k, np.int64)
            ctx.d2h(ids, c_ids)
            got = [np.empty(256 * k, np.int32) for _ in range(3)]
            for g, d in zip(got, c_out):
                ctx.d2h(g, d)
            have = ids >= 0
            # (every id came out of the near search: the cover is complete and fits the window)
            assert (got[0][~have] == -1).all() and (got[1][have] >= 1).all() and (got[1][have] <= 8).all() and (got[2][have] >= 1).all()
            res["cover_pairs_k%d" % k] = int(have.sum())
            res["cover_pair_words_k%d" % k] = int(np.asarray(lens, dtype=np.int64)[ids[have]].sum())
            for d in [c_ids, c_sc] + c_out:
                ctx.free(d)
    for d in (d_ids, d_sc, d_cnt, d_text, d_off):
        ctx.free(d)
    ctx.bm25_destroy(ix)


def snippet_rows(ctx, res, t, o, reps):
    """the snippet rows of the docstring"""
    n = len(o) - 1
    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n)]
    m = BM25(docs, ctx=ctx, positions=True)
    rng = np.random.default_rng(3)
    queries = []
    for i in rng.integers(n, size=256):
        ws = list(dict.fromkeys(docs[int(i)].split()))
        queries.append(" ".join(ws[int(j)] for j in rng.choice(len(ws), min(int(rng.integers(2, 5)), len(ws)), replace=False)))
    terms, qoff = m._query_terms(queries)
    width = 32

    def host_loop(ids):
        out = []
        for q, row in enumerate(ids.tolist()):
            R = set(queries[q].split())
            for d in row:
                if d < 0:
                    out.append((-1, 0))
                    continue
                W = docs[d].split()
                h = [1 if x in R else 0 for x in W]
                best_s, best = 0, -1
                for s in range(max(1, len(W) - width + 1)):
                    v = sum(h[s:s + width])
                    if v > best:
                        best_s, best = s, v
                out.append((best_s, best))
        return out

    for k in (10, 1000):
        ids = np.ascontiguousarray(m.search(queries, k)[0])
        kk = ids.shape[1]
        d_ids, d_s, d_h = ctx.alloc(ids.size * 8), ctx.alloc(ids.size * 4), ctx.alloc(ids.size * 4)
        ctx.h2d(d_ids, ids)

        def device():
            ctx.bm25_snippets_device(m._index, terms, qoff, d_ids, kk, width, d_s, d_h)
            ctx.sync()
        key = "q256_k%d" % k
        res["snippet_device_%s_ms" % key], res["snippet_device_%s_all_ms" % key] = median_ms(device, reps)
        res["snippet_python_%s_ms" % key], res["snippet_python_%s_all_ms" % key] = median_ms(lambda: m.snippets(queries, ids, width), reps)
        res["occurrences_python_%s_ms" % key], res["occurrences_python_%s_all_ms" % key] = median_ms(lambda: m.occurrences(queries, ids), reps)
        starts, hits = m.snippets(queries, ids, width)
        got = np.empty(ids.size, np.int32)
        ctx.d2h(got, d_s)
        assert np.array_equal(got.reshape(ids.shape), starts)
        lens = np.asarray(m.fieldLens, dtype=np.int64)
        res["snippet_pairs_k%d" % k] = int((ids >= 0).sum())
        res["snippet_pair_words_k%d" % k] = int(lens[ids[ids >= 0]].sum())
        res["occurrences_total_k%d" % k] = int(m.occurrences(queries, ids)[2][-1])
        if k == 10 or res["snippet_host_loop_q256_k10_ms"] * ids.size / 2560.0 < 60e3:
            t0 = time.perf_counter()
            want = host_loop(ids)
            res["snippet_host_loop_%s_ms" % key] = (time.perf_counter() - t0) * 1e3
            assert want == list(zip(starts.ravel().tolist(), hits.ravel().tolist()))
        for d in (d_ids, d_s, d_h):
            ctx.free(d)
    del m


def vocab_rows(ctx, res, t, o, reps):
    """the vocabulary rows of the docstring"""
    n, nbytes = len(o) - 1, int(o[-1])
    d_text, d_off = ctx.alloc(nbytes), ctx.alloc(8 * (n + 1))
    ctx.h2d(d_text, t)
    ctx.h2d(d_off, o)
    ix = ctx.bm25_build_device(d_text, d_off, n, nbytes)
    T = ctx.bm25_info(ix)[1]
    res["terms"] = T

    def read():
        off, data, _ = ctx.bm25_terms(ix)
        raw, off = data.tobytes(), off.tolist()
        return [raw[off[i]:off[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(off) - 1)]
    res["vocab_host_read_ms"], res["vocab_host_read_all_ms"] = median_ms(read, reps)
    V = read()
    rng = np.random.default_rng(7)
    words = []
    for i in rng.integers(T, size=256):
        w, c = V[int(i)], "abcdeghimnotu"[int(rng.integers(13))]
        p, op = int(rng.integers(len(w) + 1)), int(rng.integers(3))
        words.append(w[:p] + c + w[p:] if op == 0 or len(w) < 2 else w[:min(p, len(w) - 1)] + (c if op == 1 else "") + w[min(p, len(w) - 1) + 1:])
    rows = max(1, (1 << 23) // max(T, 1))
    for W in (1, 64, 256):
        wb, wo = pack(words[:W])
        pb, po = pack([w[:3] for w in words[:W]])
        res["vocab_similar_w%d_ms" % W], res["vocab_similar_w%d_all_ms" % W] = median_ms(lambda: ctx.bm25_similar(ix, wb, wo, 2, 10), reps)
        res["vocab_prefix_w%d_ms" % W], res["vocab_prefix_w%d_all_ms" % W] = median_ms(lambda: ctx.bm25_prefix(ix, pb, po, 10), reps)
        ids, dist, df, counts = ctx.bm25_similar(ix, wb, wo, 2, 10)
        res["vocab_term_texts_w%d_ms" % W], res["vocab_term_texts_w%d_all_ms" % W] = median_ms(lambda: ctx.bm25_term_bytes(ix, ids), reps)
        res["vocab_similar_mean_count_w%d" % W] = float(counts.mean())
        if W > 1:
            res["vocab_similar_ms_per_word_w%d" % W] = res["vocab_similar_w%d_ms" % W] / W
    res["vocab_key_rows_per_chunk"], res["vocab_key_bytes"] = min(256, rows), min(256, rows) * T * 8

    def lev(a, b):
        prev = list(range(len(b) + 1))
        for i, ca in enumerate(a, 1):
            cur = [i]
            for j, cb in enumerate(b, 1):
                cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
            prev = cur
        return prev[-1]
    w = words[0]
    ids, dist, df, counts = ctx.bm25_similar(ix, *pack([w]), 2, 10)
    _, _, DF = ctx.bm25_terms(ix)
    DF = DF.tolist()
    t0 = time.perf_counter()
    m = sorted((d, -DF[i], i) for i, x in enumerate(V) if abs(len(x) - len(w)) <= 2 for d in (lev(w, x),) if d <= 2)
    res["vocab_host_loop_w1_ms"] = (time.perf_counter() - t0) * 1e3
    assert int(counts[0]) == len(m) and ids[0].tolist()[:len(m)] == [x[2] for x in m[:10]] and dist[0].tolist()[:len(m)] == [x[0] for x in m[:10]]
    ctx.bm25_destroy(ix)
    ctx.free(d_text)
    ctx.free(d_off)


def groups_rows(ctx, res, t, o, reps):
    """the word-group rows of the docstring"""
    n, nbytes = len(o) - 1, int(o[-1])
    d_text, d_off = ctx.alloc(nbytes), ctx.alloc(8 * (n + 1))
    ctx.h2d(d_text, t)
    ctx.h2d(d_off, o)
    ix = ctx.bm25_build_device(d_text, d_off, n, nbytes)             # (a fresh build: the canonical ids are the lookup's)
    raw = t.tobytes()
    rng = np.random.default_rng(11)
    queries = []
    for d in rng.integers(n, size=4096):
        words = list(dict.fromkeys(raw[int(o[d]):int(o[d + 1])].decode("utf-8").split()))
        size = 2 + len(queries) % 3
        if len(words) >= size:
            queries.append(words[:size])
        if len(queries) == 256:
            break
    assert len(queries) == 256
    words = [w for q in queries for w in q]
    goff = np.zeros(257, np.int64)
    np.cumsum([len(q) for q in queries], out=goff[1:])
    G = len(words)
    terms, df = ctx.bm25_lookup(ix, *pack(words))
    assert (terms >= 0).all()
    ids, _, adf, counts = ctx.bm25_similar(ix, *pack(words), 2, 8)   # the word itself first, then the nearest terms, 8 in all
    assert (ids[:, 0] == terms).all()
    alts = [ids[g, :min(8, int(counts[g]))].astype(np.int32) for g in range(G)]
    aoff8 = np.zeros(G + 1, np.int64)
    np.cumsum([len(a) for a in alts], out=aoff8[1:])
    aterm8 = np.concatenate(alts)
    adf8 = np.concatenate([adf[g, :len(alts[g])] for g in range(G)])
    res["groups_alt8_mean_size"] = float(aoff8[-1] / G)

    def idf_of(d):
        return np.array([np.log(1+(n-int(x)+0.5)/(int(x)+0.5)) for x in d])
    gdf8 = ctx.bm25_match_count(ix, aterm8, aoff8)                   # df of a group: the documents that hold any alternative
    params = [2.2, 1.2, 0.25, 0.75, float(ctx.bm25_field_lengths(ix).mean()), 0.0]
    cases = {
        # name: (grouped arguments, the plain search that marks the same postings and probes as many candidates)
        "single": ((terms, np.arange(G + 1, dtype=np.int64), idf_of(df), goff), (terms, idf_of(df), goff)),
        "alt8": ((aterm8, aoff8, idf_of(gdf8), goff), (aterm8, idf_of(adf8), aoff8[goff])),
    }
    grouped = hasattr(ctx.lib, "gz_bm25_search_groups")              # (an older build through GZ_LIBRARY gives the plain rows alone)
    d_ids, d_sc, d_cnt = ctx.alloc(256 * 10 * 8), ctx.alloc(256 * 10 * 8), ctx.alloc(256 * 8)
    for name, (ga, pa) in cases.items():
        ts = {}
        for rep in range(reps + 1):                                  # (the first round is the warm-up of all four; interleaved)
            for mode in (0, 1):
                for kind in ("groups", "plain") if grouped else ("plain",):
                    t0 = time.perf_counter()
                    if kind == "groups":
                        ctx.bm25_search_groups(ix, ga[0], ga[1], ga[2], ga[3], params, False, 10, mode=mode, d_ids=d_ids, d_scores=d_sc, d_counts=d_cnt)
                    else:
                        ctx.bm25_search(ix, pa[0], pa[1], pa[2], params, False, 10, d_ids=d_ids, d_scores=d_sc, d_counts=d_cnt, mode=mode)
                    ctx.sync()
                    if rep:
                        ts.setdefault((kind, mode), []).append((time.perf_counter() - t0) * 1e3)
                    if rep == reps:
                        cnt = np.empty(256, np.int64)
                        ctx.d2h(cnt, d_cnt)
                        res["groups_%s_%s_%s_match_fraction" % (kind, name, ("any", "all")[mode])] = float(cnt.mean() / n)
        for (kind, mode), v in ts.items():
            key = "groups_%s_%s_%s_q256_k10" % (kind, name, ("any", "all")[mode])
            res[key + "_ms"], res[key + "_all_ms"] = float(np.median(v)), [round(x, 3) for x in v]
    for d in (d_ids, d_sc, d_cnt, d_text, d_off):
        ctx.free(d)
    ctx.bm25_destroy(ix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restate-docs", type=int, default=100_000)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", type=int, default=10_000, help="documents of the append rows (0: skip them)")
    ap.add_argument("--append-only", action="store_true", help="only the append rows (a trace of their kernels)")
    ap.add_argument("--remove", type=int, default=10_000, help="documents of the remove rows (0: skip them)")
    ap.add_argument("--remove-only", action="store_true", help="only the remove rows (a trace of their kernels)")
    ap.add_argument("--compact", type=int, default=10_000, help="documents removed before the compact rows (0: skip them)")
    ap.add_argument("--compact-only", action="store_true", help="only the compact rows; with --out they are merged into the file")
    ap.add_argument("--search-only", action="store_true", help="only the build, top-k (k = 10) and search rows; with --out they are merged into the file")
    ap.add_argument("--phrase-only", action="store_true", help="only the phrase rows; with --out they are merged into the file")
    ap.add_argument("--snippet-only", action="store_true", help="only the snippet rows; with --out they are merged into the file")
    ap.add_argument("--near-only", action="store_true", help="only the phrase and the proximity rows; with --out they are merged into the file")
    ap.add_argument("--vocab-only", action="store_true", help="only the vocabulary rows; with --out they are merged into the file")
    ap.add_argument("--groups-only", action="store_true", help="only the word-group rows; with --out they are merged into the file")
    a = ap.parse_args()
    if a.search_only:
        a.remove = a.compact = a.append = 0
    t, o, _ = corpus.config_corpus(2, n_docs=a.docs)
    n, nbytes = len(o) - 1, int(o[-1])
    ctx = _native.Context()
    res = dict(corpus="configs[2]", docs=n, text_bytes=nbytes, reps=a.reps)
    if a.phrase_only or a.near_only:
        phrase_rows(ctx, res, t, o, a.reps, near=a.near_only)
        print(json.dumps(res))
        if a.out:
            old = json.loads(open(a.out).read()) if os.path.exists(a.out) else {}
            old.update({k: v for k, v in res.items() if k.startswith(("phrase_", "near_", "cover_"))})
            old["near_rows_run" if a.near_only else "phrase_rows_run"] = dict(docs=n, reps=a.reps)
            with open(a.out, "w") as f:
                f.write(json.dumps(old) + "\n")
        return
    if a.groups_only:
        groups_rows(ctx, res, t, o, a.reps)
        print(json.dumps(res))
        if a.out:
            old = json.loads(open(a.out).read()) if os.path.exists(a.out) else {}
            old.update({k: v for k, v in res.items() if k.startswith("groups_")})
            old["groups_rows_run"] = dict(docs=n, reps=a.reps)
            with open(a.out, "w") as f:
                f.write(json.dumps(old) + "\n")
        return
    if a.vocab_only:
        vocab_rows(ctx, res, t, o, a.reps)
        print(json.dumps(res))
        if a.out:
            old = json.loads(open(a.out).read()) if os.path.exists(a.out) else {}
            old.update({k: v for k, v in res.items() if k.startswith("vocab_")})
            old["vocab_rows_run"] = dict(docs=n, reps=a.reps)
            with open(a.out, "w") as f:
                f.write(json.dumps(old) + "\n")
        return
    if a.snippet_only:
        snippet_rows(ctx, res, t, o, a.reps)
        print(json.dumps(res))
        if a.out:
            old = json.loads(open(a.out).read()) if os.path.exists(a.out) else {}
            old.update({k: v for k, v in res.items() if k.startswith(("snippet_", "occurrences_"))})
            old["snippet_rows_run"] = dict(docs=n, reps=a.reps)
            with open(a.out, "w") as f:
                f.write(json.dumps(old) + "\n")
        return
    if a.compact_only:
        compact_rows(ctx, res, n, a.compact, a.reps)
        line = json.dumps(res)
        print(line)
        if a.out:
            old = json.loads(open(a.out).read()) if os.path.exists(a.out) else {}
            old.update({k: v for k, v in res.items() if k.startswith(("compact_", "terms_device", "footprint_"))})
            old["compact_rows_run"] = dict(docs=n, reps=a.reps, rebuild_remaining_device_ms=res["rebuild_remaining_device_ms"])
            with open(a.out, "w") as f:
                f.write(json.dumps(old) + "\n")
        return
    if a.remove:
        remove_rows(ctx, res, n, a.remove, a.reps)
    if a.remove_only:
        print(json.dumps(res))
        return
    if a.compact:
        compact_rows(ctx, res, n, a.compact, a.reps)                 # (its rebuild_remaining_device_ms is the one recorded)
    if a.append:
        append_rows(ctx, res, n, a.append, a.reps)
    if a.append_only:
        print(json.dumps(res))
        return

    d_text, d_off = ctx.alloc(nbytes), ctx.alloc(8 * (n + 1))
    ctx.h2d(d_text, t)
    ctx.h2d(d_off, o)

    ts = []
    for k in range(a.reps + 1):                                      # (the first build is the warm-up)
        t0 = time.perf_counter()
        ix = ctx.bm25_build_device(d_text, d_off, n, nbytes)
        ts.append((time.perf_counter() - t0) * 1e3)
        if k < a.reps:
            ctx.bm25_destroy(ix)
    res["build_device_ms"], res["build_device_all_ms"] = float(np.median(ts[1:])), [round(x, 3) for x in ts[1:]]
    res["terms"], res["words"] = ctx.bm25_info(ix)[1:]
    lens = ctx.bm25_field_lengths(ix)
    avg = float(np.mean(lens))
    raw = t.tobytes()
    vocab = sorted({w for i in range(2000) for w in raw[o[i]:o[i + 1]].decode("utf-8").split()})
    rng = np.random.default_rng(1)
    queries = [" ".join(vocab[int(k)] for k in rng.integers(len(vocab), size=8)) for _ in range(256)]
    words = [w for q in queries for w in q.split()]
    wb, wo = pack(words)
    terms, df = ctx.bm25_lookup(ix, wb, wo)
    idf = np.array([np.log(1+(n-int(d)+0.5)/(int(d)+0.5)) for d in df])
    params = [2.2, 1.2, 0.25, 0.75, avg, 0.0]
    d_out = ctx.alloc(256 * n * 8) if not a.search_only else None
    for q in (1, 64, 256) if not a.search_only else ():
        qoff = np.arange(q + 1, dtype=np.int64) * 8

        def score():
            ctx.bm25_score(ix, terms[:8 * q], idf[:8 * q], qoff, params, False, d_out=d_out)
            ctx.sync()
        res["score_q%d_ms" % q], res["score_q%d_all_ms" % q] = median_ms(score, a.reps)
    if not a.search_only:
        res["score_q256_write_GBps"] = round(256 * n * 8 / res["score_q256_ms"] / 1e6, 1)
        ctx.free(d_out)
    d_ids, d_sc = ctx.alloc(256 * 1000 * 8), ctx.alloc(256 * 1000 * 8)
    for q in (1, 64, 256):
        qoff = np.arange(q + 1, dtype=np.int64) * 8
        for k in (10, 1000) if not a.search_only else (10,):
            def topk():
                ctx.bm25_topk(ix, terms[:8 * q], idf[:8 * q], qoff, params, False, k, d_ids=d_ids, d_scores=d_sc)
                ctx.sync()
            res["topk_q%d_k%d_ms" % (q, k)], res["topk_q%d_k%d_all_ms" % (q, k)] = median_ms(topk, a.reps)
    drawn = None
    if hasattr(ctx.lib, "gz_bm25_search_bool_device"):
        rng = np.random.default_rng(3)
        dq = []
        for i in rng.integers(n, size=256):
            ws = list(dict.fromkeys(raw[o[i]:o[i + 1]].decode("utf-8").split()))
            dq.append([ws[int(j)] for j in rng.choice(len(ws), min(int(rng.integers(2, 5)), len(ws)), replace=False)])
        db, do = pack([w for q in dq for w in q])
        dterms, ddf = ctx.bm25_lookup(ix, db, do)
        doff = np.zeros(257, np.int64)
        np.cumsum([len(q) for q in dq], out=doff[1:])
        drawn = (dterms, np.array([np.log(1+(n-int(d)+0.5)/(int(d)+0.5)) for d in ddf]), doff)
    search_rows(ctx, res, ix, n, d_text, d_off, nbytes, terms, idf, params, d_ids, d_sc, a.reps, drawn)
    for k in (10, 1000) if not a.search_only else ():
        res["topk_q256_k%d_over_score_pct" % k] = round(100 * (res["topk_q256_k%d_ms" % k] / res["score_q256_ms"] - 1), 1)
    ctx.free(d_ids)
    ctx.free(d_sc)
    ctx.bm25_destroy(ix)
    ctx.free(d_text)
    ctx.free(d_off)
    if a.search_only:
        line = json.dumps(res)
        print(line)
        if a.out:
            old = json.loads(open(a.out).read()) if os.path.exists(a.out) else {}
            old.update({k: v for k, v in res.items() if k.startswith(("search_", "postings_", "match_fraction", "topk_rare_", "rare_df_"))})
            old["search_rows_run"] = dict(docs=n, reps=a.reps, build_device_ms=res["build_device_ms"],
                                          **{k: v for k, v in res.items() if k.startswith("topk_q") and k.endswith("_k10_ms")})
            with open(a.out, "w") as f:
                f.write(json.dumps(old) + "\n")
        return

    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n)]
    holder = []
    res["ctor_ms"], res["ctor_all_ms"] = median_ms(lambda: (holder.clear(), holder.append(BM25(docs, ctx=ctx))), a.reps)
    m = holder[0]
    holder.clear()

    def host_topk():
        return m.top_k(queries, 100)

    def host_scores():
        return m.get_scores(queries)

    def host_argpartition():
        S = m.get_scores(queries)
        part = np.argpartition(-S, 99, axis=1)[:, :100]
        v = np.take_along_axis(S, part, 1)
        order = np.argsort(-v, axis=1, kind="stable")
        return np.take_along_axis(part, order, 1)
    res["topk_host_q256_k100_ms"], res["topk_host_q256_k100_all_ms"] = median_ms(host_topk, a.reps)
    res["get_scores_host_q256_ms"], res["get_scores_host_q256_all_ms"] = median_ms(host_scores, a.reps)
    res["get_scores_argpartition_q256_k100_ms"], res["get_scores_argpartition_q256_k100_all_ms"] = median_ms(host_argpartition, a.host_reps)
    del m

    if a.restate_docs:
        import bm25_restate as R
        sub = docs[:a.restate_docs]
        lens_s, freq_s = R.stats(sub)
        post = R.Postings(freq_s)
        avg_s = R.avg_field_len(lens_s)

        def restate():
            for q in queries[:64]:
                w = q.split()
                R.scores(lens_s, post, avg_s, w, [R.idf(len(sub), post.df(x)) for x in w], 0.75, 1.2)
        res["restate_docs"] = len(sub)
        res["restate_q64_ms"], _ = median_ms(restate, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
