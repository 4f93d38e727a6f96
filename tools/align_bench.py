"""Word spans and aligned rows (gz_word_spans_device, gz_align_rows_device, csrc/gz_align.inc) on the configs[2] corpus, beside the
calls they are measured against and the host route they replace.

    python tools/align_bench.py [--docs 1000000] [--reps 5] [--sample 2000] [--out profiles/align_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit, with GZ_KEEP_WORDS; the
text, the ragged rows, the piece counts and a label per word stay in HBM.  Host clock around the call plus gz_sync, after a warm-up
call, median of --reps, all in one run:
  spans_char_ms, spans_byte_ms   gz_word_spans_device, both passes (count, scans, the total's way to the host, write): W words
  align_dense_ms                 gz_align_rows_device over [N, 128] rows (row r = document r, start 0): word_ids, labels, n_real
  align_windows_ms               ... over the [Wn, 128] windows of gz_window_rows (stride 32), row_doc / row_start = their doc / start
  window_ms                      gz_window_rows_device (max_len 128, stride 32) filling input_ids and attention_mask of those Wn windows:
                                 as many cells, 8 bytes a cell out as well -- the yardstick for the align call
  word_counts_ms                 gz_wordset_build_device over the same text: the word front that walks the same words (count, scan, words,
                                 hash) and returns the distinct words' counts -- the yardstick for the span call
  host_spans_ms, host_align_ms   re.finditer per document, and numpy per document for the dense word ids, on the first --sample
                                 documents, scaled to the corpus
  ratios                         align_windows / window, align_dense per cell / window per cell, spans / word_counts, host / device
The device outputs are compared with plain Python on the first 4 096 documents (checked: true).  One JSON line on stdout."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "genz-tokenize_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORD = re.compile(r"\S+\n?")
CHECK_DOCS = 4096
L, STRIDE = 128, 32


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def host_spans(doc):
    """[begin, end) of every word of one str document, in code points"""
    out = []
    for m in WORD.finditer(doc):
        e = m.end()
        out.append((m.start(), e - 1 if doc[e - 1] == "\n" else e))
    return out


def host_word_ids(counts, max_len):
    """one dense row of word ids from a document's piece counts (numpy)"""
    row = np.full(max_len, -1, dtype=np.int32)
    body = np.repeat(np.arange(len(counts), dtype=np.int32), counts)[:max_len - 2]
    row[1:1 + len(body)] = body
    return row


def plain_rows(counts, labels, first, row_doc, row_start, max_len, cont_map):
    """the rule by loops: (word_ids, labels, n_real) of the given rows"""
    W, Lb, N = [], [], []
    for d, s in zip(row_doc, row_start):
        c = counts[first[d]:first[d + 1]]
        word_of = [j for j, k in enumerate(c) for _ in range(k)]
        head = [True if i == 0 or word_of[i - 1] != word_of[i] else False for i in range(len(word_of))]
        chunk = range(s, min(s + max_len - 2, len(word_of))) if s < len(word_of) else []
        wid, lab = [-1] * max_len, [-100] * max_len
        for i, t in enumerate(chunk):
            v = int(labels[first[d] + word_of[t]])
            wid[1 + i] = word_of[t]
            lab[1 + i] = v if head[t] else (cont_map[v] if 0 <= v < len(cont_map) else v)
        W.append(wid); Lb.append(lab); N.append(len(chunk) + 2)
    return np.array(W, dtype=np.int32), np.array(Lb, dtype=np.int32), np.array(N, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    from genz_tokenize import Tokenize, _native
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n, B = len(offs) - 1, int(offs[-1] - offs[0])
    tok = Tokenize()
    tok._sync_tables()
    ctx = tok._ctx
    cap = B + 2 * n
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    d_ids, d_mask, d_ro = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1))
    ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE | _native.GZ_KEEP_WORDS, cap, d_ids, d_mask, d_row_off=d_ro)
    ctx.sync()
    counts, first = ctx.word_token_counts(0, n, 1 << 16)
    counts = np.ascontiguousarray(counts)
    W = len(counts)
    labels = ((np.arange(W, dtype=np.int64) * 2654435761) % 9).astype(np.int32)       # a label per word: 0 .. 8 (BIO ids of four classes)
    cont_map = np.array([v + 1 if v % 2 else v for v in range(9)], dtype=np.int32)
    d_counts, d_first, d_labels, d_map = ctx.alloc(4 * W + 64), ctx.alloc(8 * (n + 1)), ctx.alloc(4 * W + 64), ctx.alloc(64)
    ctx.h2d(d_counts, counts); ctx.h2d(d_first, first); ctx.h2d(d_labels, labels); ctx.h2d(d_map, cont_map)

    # ---- spans, beside the word front
    d_span, d_woff = ctx.alloc(8 * W + 64), ctx.alloc(8 * (n + 1))
    span_ms, got_spans = {}, {}
    for unit, name in ((0, "char"), (1, "byte")):
        def spans():
            assert ctx.word_spans_device(d_t, d_to, n, B, unit, d_span, d_woff, W) == W
            ctx.sync()
        spans()
        span_ms[name] = median_ms(spans, args.reps)
        woff = np.empty(n + 1, dtype=np.int64)
        ctx.d2h(woff, d_woff)
        assert np.array_equal(woff, first)
        k = int(first[min(CHECK_DOCS, n)])
        got_spans[name] = np.empty((k, 2), dtype=np.int32)
        if k:
            ctx.d2h(got_spans[name], d_span)

    def word_counts():
        ctx.wordset_destroy(ctx.wordset_build_device(d_t, d_to, n, B))
        ctx.sync()
    word_counts()
    wc_ms, wc_all = median_ms(word_counts, args.reps)

    # ---- align over dense rows and over windows, beside the window call
    d_w, d_l, d_n = ctx.alloc(4 * n * L + 64), ctx.alloc(4 * n * L + 64), ctx.alloc(4 * n + 64)

    def dense():
        ctx.align_rows_device(d_counts, d_first, n, W, 0, 0, n, L, d_labels, 2, d_map, len(cont_map), -100, d_w, d_l, d_n)
        ctx.sync()
    dense()
    dense_ms, dense_all = median_ms(dense, args.reps)
    m = min(CHECK_DOCS, n)
    got_dense = [np.empty((m, L), dtype=np.int32), np.empty((m, L), dtype=np.int32), np.empty(m, dtype=np.int32)]
    for a, d in zip(got_dense, (d_w, d_l, d_n)):
        ctx.d2h(a, d)
    for d in (d_w, d_l, d_n):
        ctx.free(d)

    d_wo = ctx.alloc(8 * (n + 1))
    Wn = ctx.window_rows_device(d_ids, d_ro, n, L, STRIDE, 1, 1, 0, 0, 0, 0, 0, d_wo, 0)
    d_out, d_m, d_meta = ctx.alloc(4 * Wn * L + 64), ctx.alloc(4 * Wn * L + 64), ctx.alloc(12 * Wn + 64)

    def window():
        ctx.window_rows_device(d_ids, d_ro, n, L, STRIDE, 1, 1, d_out, d_m, d_meta, d_meta + 4 * Wn, d_meta + 8 * Wn, d_wo, Wn)
        ctx.sync()
    window()
    win_ms, win_all = median_ms(window, args.reps)
    d_ww, d_wl, d_wn = ctx.alloc(4 * Wn * L + 64), ctx.alloc(4 * Wn * L + 64), ctx.alloc(4 * Wn + 64)

    def windows():
        ctx.align_rows_device(d_counts, d_first, n, W, d_meta, d_meta + 4 * Wn, Wn, L, d_labels, 2, d_map, len(cont_map), -100, d_ww, d_wl, d_wn)
        ctx.sync()
    windows()
    alw_ms, alw_all = median_ms(windows, args.reps)
    win_off = np.empty(n + 1, dtype=np.int64)
    ctx.d2h(win_off, d_wo)
    mw = int(win_off[m])
    meta = np.empty((3, Wn), dtype=np.int32)
    ctx.d2h(meta, d_meta)
    got_win = [np.empty((mw, L), dtype=np.int32), np.empty((mw, L), dtype=np.int32), np.empty(mw, dtype=np.int32)]
    for a, d in zip(got_win, (d_ww, d_wl, d_wn)):
        if a.size:
            ctx.d2h(a, d)

    # ---- the host route on a sample, and the check on the first documents
    raw = text.tobytes()
    docs = [raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(m)]
    ns = min(args.sample, m)
    t0 = time.perf_counter()
    for d in docs[:ns]:
        host_spans(d)
    host_spans_ms = (time.perf_counter() - t0) * 1e3 * n / max(ns, 1)
    t0 = time.perf_counter()
    for i in range(ns):
        host_word_ids(counts[first[i]:first[i + 1]], L)
    host_align_ms = (time.perf_counter() - t0) * 1e3 * n / max(ns, 1)
    want_char = [s for d in docs for s in host_spans(d)]
    want_byte = [(len(d[:b].encode()), len(d[:e].encode())) for d in docs for b, e in host_spans(d)]
    checked = got_spans["char"].tolist() == [list(s) for s in want_char] and got_spans["byte"].tolist() == [list(s) for s in want_byte]
    want = plain_rows(counts, labels, first, range(m), [0] * m, L, cont_map.tolist())
    checked = checked and all(np.array_equal(a, b) for a, b in zip(got_dense, want))
    want = plain_rows(counts, labels, first, meta[0][:mw].tolist(), meta[1][:mw].tolist(), L, cont_map.tolist())
    checked = bool(checked and all(np.array_equal(a, b) for a, b in zip(got_win, want)))

    rec = {"bench": "align", "docs": n, "text_bytes": B, "words": W, "max_len": L, "stride": STRIDE, "windows": int(Wn),
           "spans_char_ms": round(span_ms["char"][0], 3), "spans_char_all_ms": span_ms["char"][1],
           "spans_byte_ms": round(span_ms["byte"][0], 3), "spans_byte_all_ms": span_ms["byte"][1],
           "word_counts_ms": round(wc_ms, 3), "word_counts_all_ms": wc_all,
           "align_dense_ms": round(dense_ms, 3), "align_dense_all_ms": dense_all, "dense_cells": n * L,
           "align_windows_ms": round(alw_ms, 3), "align_windows_all_ms": alw_all, "window_cells": int(Wn) * L,
           "window_ms": round(win_ms, 3), "window_all_ms": win_all,
           "host_spans_ms": round(host_spans_ms, 1), "host_align_ms": round(host_align_ms, 1), "host_sample": ns,
           "ratio_spans_to_word_counts": round(span_ms["char"][0] / wc_ms, 3),
           "ratio_align_windows_to_window": round(alw_ms / win_ms, 3),
           "ratio_align_dense_per_cell_to_window_per_cell": round((dense_ms / (n * L)) / (win_ms / (Wn * L)), 3),
           "speedup_spans": round(host_spans_ms / span_ms["char"][0], 1), "speedup_align_dense": round(host_align_ms / dense_ms, 1),
           "checked_docs": m, "checked": checked}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if checked else 1


if __name__ == "__main__":
    sys.exit(main())
