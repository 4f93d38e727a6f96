"""Overlapping max_len windows (gz_window_rows_device, csrc/gz_window.inc) on the configs[2] corpus, and the host route they replace.

    python tools/window_bench.py [--docs 1000000] [--reps 5] [--host-reps 3] [--out profiles/window_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs): 5 % of the documents have 121-400 words) is encoded once on the device
without a length limit; the ragged rows stay in HBM.  For max_len in (128, 256) and stride in (0, 32), host clock around the call
plus gz_sync, after a warm-up call, median of --reps:
  window_device_ms     gz_window_rows_device over the resident rows: count pass, scan, the total's way to the host, fill pass
  windows, out_bytes   W and the bytes the fill pass writes (8 W L for ids and mask + 12 W for doc / start / n_real)
  in_bytes             4 bytes per chunk token read (the sum of n_real - 2)
  hbm_fraction         (out_bytes + in_bytes) / window_device_ms over HBM_PEAK_GBS (8000 GB/s, bench.py's constant)
  truncated_tokens     body tokens a dense max_len call drops (beyond the first window)
and, in the same run, the only route there was before (median of --host-reps):
  host_encode_ms       encode_packed(max_len=None): the ragged rows into host memory (encode_batch(max_len=None) without its
                       Python string packing, which is not timed)
  host_rule_ms         a vectorised numpy statement of the rule over those rows (64 K windows at a time)
  host_route_ms        their sum;  speedup = host_route_ms / window_device_ms
The numpy rows are compared with the device rows once per shape (checked: true).  One JSON line on stdout."""
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


def numpy_windows(ids, row_off, L, s, bos, eos, pad, chunk=1 << 16):
    """The rule over framed ragged rows, on the host: (input_ids [W, L], attention_mask [W, L], win_off [N+1])."""
    room, step, n = L - 2, L - 2 - s, len(row_off) - 1
    T = np.maximum(np.diff(row_off) - 2, 0)
    n_win = np.where(T <= room, 1, 1 + -(-(T - room) // step))
    win_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(n_win, out=win_off[1:])
    W = int(win_off[-1])
    doc = np.repeat(np.arange(n, dtype=np.int64), n_win)
    start = (np.arange(W, dtype=np.int64) - win_off[doc]) * step
    clen = np.clip(T[doc] - start, 0, room)
    first = row_off[doc] + 1 + start
    out = np.full((W, L), pad, dtype=np.int32)
    out[:, 0] = bos
    cols = np.arange(room, dtype=np.int64)[None, :]
    for lo in range(0, W, chunk):
        hi = min(lo + chunk, W)
        keep = cols < clen[lo:hi, None]
        src = first[lo:hi, None] + cols
        out[lo:hi, 1:L - 1][keep] = ids[src[keep]]
    out[np.arange(W), clen + 1] = eos
    return out, (out != pad).astype(np.int32), win_off


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
    ap.add_argument("--host-reps", type=int, default=3)
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
    body_tokens = int(np.maximum(np.diff(row_off) - 2, 0).sum())

    # the host route's first half does not depend on the window shape
    host = {}
    def host_encode():
        host["r"] = tok.encode_packed(text, offs, max_len=None)
    host_encode()
    enc_ms, enc_all = median_ms(host_encode, args.host_reps)
    h_ids, h_ro = host["r"]["input_ids"], host["r"]["row_off"]
    assert np.array_equal(h_ro, row_off)

    rows = []
    for L in (128, 256):
        for s in (0, 32):
            W = ctx.window_rows_device(d_ids, d_ro, n, L, s, 1, 1, 0, 0, 0, 0, 0, d_wo, 0)
            d_out, d_m, d_meta = ctx.alloc(4 * W * L), ctx.alloc(4 * W * L), ctx.alloc(12 * W)

            def device():
                ctx.window_rows_device(d_ids, d_ro, n, L, s, 1, 1, d_out, d_m, d_meta, d_meta + 4 * W, d_meta + 8 * W, d_wo, W)
                ctx.sync()
            device()
            dev_ms, dev_all = median_ms(device, args.reps)
            n_real = np.empty(W, dtype=np.int32)
            ctx.d2h(n_real, d_meta + 8 * W)
            in_bytes = 4 * int((n_real.astype(np.int64) - 2).sum())
            out_bytes = 8 * W * L + 12 * W
            res = {}
            def rule():
                res["r"] = numpy_windows(h_ids, h_ro, L, s, bos, eos, pad)
            rule()
            rule_ms, rule_all = median_ms(rule, args.host_reps)
            got_ids, got_mask = np.empty((W, L), dtype=np.int32), np.empty((W, L), dtype=np.int32)
            ctx.d2h(got_ids, d_out); ctx.d2h(got_mask, d_m)
            checked = bool(np.array_equal(got_ids, res["r"][0]) and np.array_equal(got_mask, res["r"][1]))
            first = int(np.minimum(np.maximum(np.diff(row_off) - 2, 0), L - 2).sum())
            rows.append({"max_len": L, "stride": s, "windows": int(W), "window_device_ms": round(dev_ms, 3), "window_device_all_ms": dev_all,
                         "out_bytes": int(out_bytes), "in_bytes": int(in_bytes),
                         "achieved_gbs": round((out_bytes + in_bytes) / dev_ms / 1e6, 1),
                         "hbm_fraction": round((out_bytes + in_bytes) / dev_ms / 1e6 / HBM_PEAK_GBS, 4),
                         "truncated_tokens": body_tokens - first, "host_encode_ms": round(enc_ms, 1), "host_rule_ms": round(rule_ms, 1),
                         "host_rule_all_ms": rule_all, "host_route_ms": round(enc_ms + rule_ms, 1),
                         "speedup": round((enc_ms + rule_ms) / dev_ms, 1), "checked": checked})
            del res, got_ids, got_mask
            for d in (d_out, d_m, d_meta):
                ctx.free(d)
            print("# L=%d s=%d W=%d device %.3f ms host %.1f ms" % (L, s, W, dev_ms, enc_ms + rule_ms), file=sys.stderr, flush=True)
    for d in (d_ids, d_ro, d_wo):
        ctx.free(d)
    rec = {"bench": "window", "docs": n, "body_tokens": body_tokens, "hbm_peak_gbs": HBM_PEAK_GBS, "host_encode_all_ms": enc_all, "rows": rows}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["checked"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
