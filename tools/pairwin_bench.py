"""Question-context windows (gz_pair_window_rows_device, csrc/gz_pairwin.inc) on the configs[2] corpus, beside gz_window_rows_device.

    python tools/pairwin_bench.py [--docs 1000000] [--reps 5] [--out profiles/pairwin_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs), the documents the other row tools use) is encoded once on the device without a
length limit; the ragged rows stay in HBM as the contexts.  Question r is the first 8 + r % 9 body tokens of document r (8..16 tokens,
fewer where the document is shorter), framed like an encode result, and every context has an answer of 1..4 tokens somewhere in its
body.  max_query_len is 16.  For max_len in (128, 256) and stride in (0, 32), host clock around the call plus gz_sync, after a warm-up
call, median of --reps, both calls in the same visit over the same context rows:
  pair_ms, pair_windows        gz_pair_window_rows_device with all ten outputs: 12 W L bytes of cells (+ 28 W)
  window_ms, window_windows    gz_window_rows_device with all five outputs: 8 W' L bytes of cells (+ 12 W')
  pair_ns_per_byte, window_ns_per_byte    time over the cell bytes written
  ratio                        pair_ns_per_byte / window_ns_per_byte; goal_met: ratio <= 1.25 (a miss is written down as a miss)
  hbm_fraction                 (bytes written + 4 bytes a source token read) / pair_ms over HBM_PEAK_GBS (8000 GB/s, bench.py's constant)
No time is fixed in advance: the yardstick is the window call's time per output byte in the same run.
A numpy statement of the rule on the host must equal the device on the first 4096 pairs, every output (asserted).  One JSON line on
stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "genz-tokenize_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec peak: the constant of bench.py
MQ = 16
CHECK_PAIRS = 4096


def numpy_pair_windows(q_ids, q_off, ids, row_off, ans, L, s, mq, bos, eos, pad):
    """The rule over framed ragged rows (pair r uses question r), on the host: the dict the device call fills."""
    n = len(row_off) - 1
    Tq = np.maximum(np.diff(q_off) - 2, 0)
    T = np.maximum(np.diff(row_off) - 2, 0)
    q = np.minimum(Tq, mq)
    room = L - 4 - q
    step = room - s
    n_win = np.where(T <= room, 1, 1 + -(-(T - room) // step))
    win_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(n_win, out=win_off[1:])
    W = int(win_off[-1])
    pair = np.repeat(np.arange(n, dtype=np.int64), n_win)
    start = (np.arange(W, dtype=np.int64) - win_off[pair]) * step[pair]
    qw, nn = q[pair], np.clip(T[pair] - start, 0, room[pair])
    cols = np.arange(L, dtype=np.int64)[None, :]
    in_q = (cols >= 1) & (cols <= qw[:, None])
    in_c = (cols >= qw[:, None] + 3) & (cols < (qw + 3 + nn)[:, None])
    is_eos = (cols == qw[:, None] + 1) | (cols == qw[:, None] + 2) | (cols == (qw + 3 + nn)[:, None])
    out = np.full((W, L), pad, dtype=np.int32)
    out[:, 0] = bos
    out[is_eos] = eos
    out[in_q] = q_ids[(q_off[pair][:, None] + cols)[in_q]]                                   # column k holds Q[k - 1]: framed row entry k
    out[in_c] = ids[((row_off[pair] + 1 + start - qw - 3)[:, None] + cols)[in_c]]            # column q + 3 + k holds body[start + k]
    n_real = qw + 4 + nn
    typ = np.where(cols < qw[:, None] + 2, 0, np.where(cols < n_real[:, None], 1, pad)).astype(np.int32)
    a0, a1 = ans[pair, 0].astype(np.int64), ans[pair, 1].astype(np.int64)
    held = (0 <= a0) & (a0 < a1) & (a1 <= T[pair]) & (start <= a0) & (a1 <= start + nn)
    i32 = lambda a: a.astype(np.int32)
    return dict(input_ids=out, attention_mask=i32(out != pad), token_type_ids=typ, pair=i32(pair), start=i32(start), n_real=i32(n_real), q_len=i32(qw),
                start_positions=i32(np.where(held, qw + 3 + a0 - start, 0)), end_positions=i32(np.where(held, qw + 3 + a1 - 1 - start, 0)),
                has_answer=i32(held), win_off=win_off)


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    from genz_tokenize import Tokenize, _native
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n = len(offs) - 1
    tok = Tokenize()
    tok._sync_tables()
    ctx = tok._ctx
    pad, bos, eos = tok._special_ids()[:3]
    cap = int(offs[n] - offs[0]) + 2 * n
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    d_ids, d_mask, d_ro, d_wo = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1)), ctx.alloc(8 * (n + 1))
    ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE, cap, d_ids, d_mask, d_row_off=d_ro)
    ctx.sync()
    ctx.free(d_mask); ctx.free(d_t); ctx.free(d_to)
    row_off = np.empty(n + 1, dtype=np.int64)
    ctx.d2h(row_off, d_ro)
    ids = np.empty(int(row_off[n]), dtype=np.int32)
    ctx.d2h(ids, d_ids)
    T = np.maximum(np.diff(row_off) - 2, 0)
    body_tokens = int(T.sum())

    # questions: the first 8..16 body tokens of every document, framed; answers: 1..4 tokens somewhere in the body
    q_len = np.minimum(8 + np.arange(n, dtype=np.int64) % 9, T)
    q_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(q_len + 2, out=q_off[1:])
    q_ids = np.full(int(q_off[n]), eos, dtype=np.int32)
    q_ids[q_off[:-1]] = bos
    inside = np.arange(int(q_off[n]), dtype=np.int64) - np.repeat(q_off[:-1], q_len + 2)      # position within its framed row
    doc = np.repeat(np.arange(n, dtype=np.int64), q_len + 2)
    body = (inside >= 1) & (inside <= q_len[doc])
    q_ids[body] = ids[(row_off[doc] + inside)[body]]
    rng = np.random.default_rng(17)
    a0 = (rng.random(n) * np.maximum(T, 1)).astype(np.int64)
    ans = np.stack([a0, np.minimum(a0 + 1 + rng.integers(0, 4, size=n), T)], axis=1).astype(np.int32)
    ans[T == 0] = -1
    d_q, d_qo, d_ans = ctx.alloc(q_ids.nbytes + 64), ctx.alloc(q_off.nbytes), ctx.alloc(ans.nbytes + 64)
    ctx.h2d(d_q, q_ids); ctx.h2d(d_qo, q_off); ctx.h2d(d_ans, np.ascontiguousarray(ans))

    rows = []
    for L in (128, 256):
        for s in (0, 32):
            head = (d_q, d_qo, n, d_ids, d_ro, n, 0, d_ans, L, s, MQ, 1, 1)
            W = ctx.pair_window_rows_device(*head, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_wo, 0)
            cells = [ctx.alloc(4 * W * L) for _ in range(3)]
            d_meta = ctx.alloc(28 * W)
            meta = [d_meta + 4 * W * k for k in range(7)]

            def pair_call():
                ctx.pair_window_rows_device(*head, *cells, *meta, d_wo, W)
                ctx.sync()
            pair_call()
            pair_ms, pair_all = median_ms(pair_call, args.reps)
            n_real, q_w = np.empty(W, dtype=np.int32), np.empty(W, dtype=np.int32)
            ctx.d2h(n_real, meta[2]); ctx.d2h(q_w, meta[3])
            in_bytes = 4 * int((n_real.astype(np.int64) - 4).sum())                            # question and chunk tokens read
            has = np.empty(W, dtype=np.int32)
            ctx.d2h(has, meta[6])
            # the first pairs against the numpy statement of the rule, every output
            m = min(CHECK_PAIRS, n)
            want = numpy_pair_windows(q_ids, q_off[:m + 1], ids, row_off[:m + 1], ans[:m], L, s, MQ, bos, eos, pad)
            Wm = int(want["win_off"][m])
            wo = np.empty(n + 1, dtype=np.int64)
            ctx.d2h(wo, d_wo)
            assert np.array_equal(wo[:m + 1], want["win_off"]), "win_off differs from the numpy rule"
            for key, d, shape in [("input_ids", cells[0], (Wm, L)), ("attention_mask", cells[1], (Wm, L)), ("token_type_ids", cells[2], (Wm, L))] + \
                                 [(k, meta[i], (Wm,)) for i, k in enumerate(("pair", "start", "n_real", "q_len", "start_positions", "end_positions", "has_answer"))]:
                got = np.empty(shape, dtype=np.int32)
                if got.size:
                    ctx.d2h(got, d)
                assert np.array_equal(got, want[key]), "%s differs from the numpy rule at L=%d s=%d" % (key, L, s)
            for d in cells + [d_meta]:
                ctx.free(d)

            Ww = ctx.window_rows_device(d_ids, d_ro, n, L, s, 1, 1, 0, 0, 0, 0, 0, d_wo, 0)
            d_out, d_m, d_wm = ctx.alloc(4 * Ww * L), ctx.alloc(4 * Ww * L), ctx.alloc(12 * Ww)

            def window_call():
                ctx.window_rows_device(d_ids, d_ro, n, L, s, 1, 1, d_out, d_m, d_wm, d_wm + 4 * Ww, d_wm + 8 * Ww, d_wo, Ww)
                ctx.sync()
            window_call()
            win_ms, win_all = median_ms(window_call, args.reps)
            for d in (d_out, d_m, d_wm):
                ctx.free(d)
            pair_npb, win_npb = pair_ms * 1e6 / (12 * W * L), win_ms * 1e6 / (8 * Ww * L)
            out_bytes = 12 * W * L + 28 * W
            rows.append({"max_len": L, "stride": s, "max_query_len": MQ, "pair_windows": int(W), "pair_ms": round(pair_ms, 3), "pair_all_ms": pair_all,
                         "window_windows": int(Ww), "window_ms": round(win_ms, 3), "window_all_ms": win_all,
                         "pair_ns_per_byte": round(pair_npb, 6), "window_ns_per_byte": round(win_npb, 6), "ratio": round(pair_npb / win_npb, 3),
                         "goal_met": bool(pair_npb <= 1.25 * win_npb), "out_bytes": int(out_bytes), "in_bytes": int(in_bytes),
                         "achieved_gbs": round((out_bytes + in_bytes) / pair_ms / 1e6, 1),
                         "hbm_fraction": round((out_bytes + in_bytes) / pair_ms / 1e6 / HBM_PEAK_GBS, 4),
                         "windows_with_answer": int(has.sum()), "checked_pairs": int(m), "checked": True})
            print("# L=%d s=%d W=%d pair %.3f ms, W'=%d window %.3f ms, ratio per byte %.3f" % (L, s, W, pair_ms, Ww, win_ms, pair_npb / win_npb),
                  file=sys.stderr, flush=True)
    for d in (d_ids, d_ro, d_wo, d_q, d_qo, d_ans):
        ctx.free(d)
    rec = {"bench": "pairwin", "docs": n, "body_tokens": body_tokens, "question_tokens": int(q_len.sum()), "hbm_peak_gbs": HBM_PEAK_GBS,
           "goal": "pair_ns_per_byte <= 1.25 * window_ns_per_byte", "rows": rows}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
