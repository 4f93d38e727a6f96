"""Short documents packed into rows of max_len (gz_pack_rows_device, csrc/gz_packrows.inc) on the configs[2] corpus, the host route it
replaces, and the window call over the same rows.

    python tools/pack_bench.py [--docs 1000000] [--reps 5] [--host-reps 3] [--order kept|fit] [--out profiles/pack_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit; the ragged rows stay
in HBM.  For max_len in (128, 256), host clock around the call plus gz_sync, after a warm-up call, median of --reps:
  pack_device_ms       gz_pack_rows_device over the resident rows: every pass, the total's way to the host, the fill
  pack_maps_ms         the same call as a sizing call (input_ids NULL): everything but the fill (lengths, scan, break chain, mark,
                       columns, the total's round trip); pack_fill_ms = pack_device_ms - pack_maps_ms
  rows, fill_ratio     R and sum(len) / (R L); dense_ratio = sum(len) / (N L), what a dense [N, L] batch holds
  out_bytes, in_bytes  16 R L + 12 N + 8 R written; 4 sum(len) read + 16 N of offsets
  hbm_fraction         (out_bytes + in_bytes) / pack_device_ms over HBM_PEAK_GBS (8000 GB/s, bench.py's constant): the WHOLE call
  window_device_ms     gz_window_rows_device on the same rows and max_len, stride 0 (W windows, 8 W L + 12 W bytes out), same run
and, in the same run, the only route there was before (median of --host-reps):
  host_encode_ms       encode_packed(max_len=None): the ragged rows into host memory
  host_rule_ms         the rule on the host: the break chain with bisect over the scanned lengths, the cells with numpy
  host_route_ms        their sum;  speedup = host_route_ms / pack_device_ms
The host arrays are compared with the device's once per shape (checked: true).  One JSON line on stdout.
--order fit adds, per max_len and in the same run, on the same resident rows and with the same clocking (a "fit" object in the row):
  rows, fill_ratio     R and sum(len) / (R L) of gz_pack_rows_fit_device (best-fit order, csrc/gz_packfit.inc)
  rows_ok              rows <= the kept order's rows: the one hard condition; the exit status is 1 where it does not hold
  device_ms, maps_ms   the whole call and the sizing call; over_kept = device_ms / pack_device_ms (the bar: at most 1.25)
  plan_ms, events, segments   the host plan alone (gz_pack_rows_fit_info after the last call)
  checked_4096         the first 4 096 documents as a batch of their own: every array equals tests/packfit_oracle.py's"""
import argparse
import bisect
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


def host_packs(ids, row_off, L, bos, eos, pad, chunk=1 << 16):
    """The rule over framed ragged rows, on the host: (input_ids, attention_mask, segment_ids, position_ids [R, L], row_off [R+1])."""
    n = len(row_off) - 1
    ln = np.minimum(np.maximum(np.diff(row_off) - 2, 0), L - 2) + 2
    seg = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(ln, out=seg[1:])
    seg_l, heads, h = seg.tolist(), [], 0
    while h < n:                                                     # next-fit: the first document that no longer fits opens a row
        heads.append(h)
        h = bisect.bisect_right(seg_l, seg_l[h] + L, h + 1, min(n + 1, h + L // 2 + 1)) - 1
    pack_off = np.array(heads + [n], dtype=np.int64)
    R = len(heads)
    doc_row = np.repeat(np.arange(R, dtype=np.int64), np.diff(pack_off))
    first = doc_row * L + (seg[:-1] - seg[pack_off[doc_row]])        # the document's first cell in the flat output
    in_row = np.arange(n, dtype=np.int64) - pack_off[doc_row] + 1
    out = np.full(R * L, pad, dtype=np.int32)
    sid, pos_out = np.zeros(R * L, dtype=np.int32), np.zeros(R * L, dtype=np.int32)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        l = ln[lo:hi]
        pos = np.arange(int(l.sum()), dtype=np.int64) - np.repeat(seg[lo:hi] - seg[lo], l)
        cell = np.repeat(first[lo:hi], l) + pos
        last = np.repeat(l - 1, l)
        val = ids[np.minimum(np.repeat(row_off[lo:hi], l) + pos, len(ids) - 1)]     # (row r's entry `pos` is body token pos - 1)
        val[pos == 0] = bos
        val[pos == last] = eos
        out[cell], pos_out[cell], sid[cell] = val, pos, np.repeat(in_row[lo:hi], l)
    out = out.reshape(R, L)
    return out, (out != pad).astype(np.int32), sid.reshape(R, L), pos_out.reshape(R, L), pack_off


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def fit_row(ctx, tok, d_ids, d_ro, row_off, n, L, maps, d_po, d_so, sum_len, kept_ms, reps, special):
    """The best-fit call on the same resident rows: R, fill, the call, the sizing call, the plan's host time, the events."""
    import ctypes
    d_rd = ctx.alloc(4 * n)
    R = ctx.pack_rows_fit_device(d_ids, d_ro, n, L, 1, 1, 0, 0, 0, 0, *maps, d_rd, d_po, d_so, 0)
    d_out = [ctx.alloc(4 * R * L) for _ in range(4)]

    def device():
        ctx.pack_rows_fit_device(d_ids, d_ro, n, L, 1, 1, *d_out, *maps, d_rd, d_po, d_so, R)
        ctx.sync()

    def sizing():
        ctx.pack_rows_fit_device(d_ids, d_ro, n, L, 1, 1, 0, 0, 0, 0, *maps, d_rd, d_po, d_so, 0)
        ctx.sync()
    device()
    dev_ms, dev_all = median_ms(device, reps)
    sizing()
    map_ms, map_all = median_ms(sizing, reps)
    plan_ms, events, segments = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
    ctx._check(ctx.lib.gz_pack_rows_fit_info(ctx.handle, ctypes.byref(plan_ms), ctypes.byref(events), ctypes.byref(segments)))
    for d in d_out + [d_rd]:
        ctx.free(d)
    # the first 4 096 documents as a batch of their own, against the sequential rule
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import packfit_oracle as FO
    m = min(n, 4096)
    ids = np.empty(int(row_off[m] - row_off[0]), dtype=np.int32)
    ctx.d2h(ids, d_ids + 4 * int(row_off[0]))
    framed = [ids[row_off[r] - row_off[0]:row_off[r + 1] - row_off[0]].tolist() for r in range(m)]
    pad, bos, eos = special
    got = tok.pack_rows(framed, L, framed=True, order="fit")
    want = FO.batch([r[1:-1] for r in framed], L, bos, eos, pad, fast=True)
    checked = sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)
    return {"rows": int(R), "fill_ratio": round(sum_len / (R * L), 4), "device_ms": round(dev_ms, 3), "device_all_ms": dev_all,
            "maps_ms": round(map_ms, 3), "maps_all_ms": map_all, "fill_ms": round(dev_ms - map_ms, 3), "plan_ms": round(plan_ms.value, 4),
            "events": int(events.value), "segments": int(segments.value), "over_kept": round(dev_ms / kept_ms, 3), "checked_4096": bool(checked)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--order", choices=("kept", "fit"), default="kept")
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
    d_ids, d_mask, d_ro = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1))
    ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE, cap, d_ids, d_mask, d_row_off=d_ro)
    ctx.sync()
    ctx.free(d_mask); ctx.free(d_t); ctx.free(d_to)
    row_off = np.empty(n + 1, dtype=np.int64)
    ctx.d2h(row_off, d_ro)
    body_tokens = int(np.maximum(np.diff(row_off) - 2, 0).sum())
    d_maps, d_po, d_so, d_wo = ctx.alloc(12 * n), ctx.alloc(8 * (n + 1)), ctx.alloc(8 * (n + 1)), ctx.alloc(8 * (n + 1))
    maps = (d_maps, d_maps + 4 * n, d_maps + 8 * n)

    host = {}
    def host_encode():
        host["r"] = tok.encode_packed(text, offs, max_len=None)
    enc_ms = 0.0
    enc_all = []
    if args.host_reps:
        host_encode()
        enc_ms, enc_all = median_ms(host_encode, args.host_reps)
        h_ids, h_ro = host["r"]["input_ids"], host["r"]["row_off"]
        assert np.array_equal(h_ro, row_off)

    rows = []
    for L in (128, 256):
        R = ctx.pack_rows_device(d_ids, d_ro, n, L, 1, 1, 0, 0, 0, 0, *maps, d_po, d_so, 0)
        d_out = [ctx.alloc(4 * R * L) for _ in range(4)]

        def device():
            ctx.pack_rows_device(d_ids, d_ro, n, L, 1, 1, *d_out, *maps, d_po, d_so, R)
            ctx.sync()

        def sizing():
            ctx.pack_rows_device(d_ids, d_ro, n, L, 1, 1, 0, 0, 0, 0, *maps, d_po, d_so, 0)
            ctx.sync()
        device()
        dev_ms, dev_all = median_ms(device, args.reps)
        sizing()
        map_ms, map_all = median_ms(sizing, args.reps)
        doc_len = np.empty(n, dtype=np.int32)
        ctx.d2h(doc_len, maps[2])
        sum_len = int(doc_len.astype(np.int64).sum())
        out_bytes, in_bytes = 16 * R * L + 12 * n + 8 * R, 4 * sum_len + 16 * n
        # the window call on the same rows
        W = ctx.window_rows_device(d_ids, d_ro, n, L, 0, 1, 1, 0, 0, 0, 0, 0, d_wo, 0)
        d_w, d_wm, d_meta = ctx.alloc(4 * W * L), ctx.alloc(4 * W * L), ctx.alloc(12 * W)

        def window():
            ctx.window_rows_device(d_ids, d_ro, n, L, 0, 1, 1, d_w, d_wm, d_meta, d_meta + 4 * W, d_meta + 8 * W, d_wo, W)
            ctx.sync()
        window()
        win_ms, win_all = median_ms(window, args.reps)
        for d in (d_w, d_wm, d_meta):
            ctx.free(d)
        rec = {"max_len": L, "rows": int(R), "fill_ratio": round(sum_len / (R * L), 4), "dense_ratio": round(sum_len / (n * L), 4),
               "pack_device_ms": round(dev_ms, 3), "pack_device_all_ms": dev_all, "pack_maps_ms": round(map_ms, 3), "pack_maps_all_ms": map_all,
               "pack_fill_ms": round(dev_ms - map_ms, 3), "out_bytes": int(out_bytes), "in_bytes": int(in_bytes),
               "achieved_gbs": round((out_bytes + in_bytes) / dev_ms / 1e6, 1),
               "hbm_fraction": round((out_bytes + in_bytes) / dev_ms / 1e6 / HBM_PEAK_GBS, 4),
               "windows": int(W), "window_out_bytes": int(8 * W * L + 12 * W), "window_device_ms": round(win_ms, 3), "window_device_all_ms": win_all,
               "pack_over_window": round(dev_ms / win_ms, 3)}
        if args.host_reps:
            res = {}
            def rule():
                res["r"] = host_packs(h_ids, h_ro, L, bos, eos, pad)
            rule()
            rule_ms, rule_all = median_ms(rule, args.host_reps)
            checked = len(res["r"][4]) == R + 1
            got = np.empty((R, L), dtype=np.int32)
            for k in range(4):
                ctx.d2h(got, d_out[k])
                checked = checked and bool(np.array_equal(got, res["r"][k]))
            po = np.empty(R + 1, dtype=np.int64)
            ctx.d2h(po, d_po)
            checked = checked and bool(np.array_equal(po, res["r"][4]))
            rec.update({"host_encode_ms": round(enc_ms, 1), "host_rule_ms": round(rule_ms, 1), "host_rule_all_ms": rule_all,
                        "host_route_ms": round(enc_ms + rule_ms, 1), "speedup": round((enc_ms + rule_ms) / dev_ms, 1), "checked": checked})
            del res, got
        if args.order == "fit":
            rec["fit"] = fit_row(ctx, tok, d_ids, d_ro, row_off, n, L, maps, d_po, d_so, sum_len, dev_ms, args.reps, (pad, bos, eos))
            rec["fit"]["rows_ok"] = bool(rec["fit"]["rows"] <= rec["rows"])
        rows.append(rec)
        for d in d_out:
            ctx.free(d)
        print("# L=%d R=%d pack %.3f ms (maps %.3f) window %.3f ms host %s ms" %
              (L, R, dev_ms, map_ms, win_ms, rec.get("host_route_ms")), file=sys.stderr, flush=True)
        if "fit" in rec:
            print("# L=%d fit %s" % (L, json.dumps(rec["fit"])), file=sys.stderr, flush=True)
    for d in (d_ids, d_ro, d_maps, d_po, d_so, d_wo):
        ctx.free(d)
    rec = {"bench": "pack", "docs": n, "body_tokens": body_tokens, "hbm_peak_gbs": HBM_PEAK_GBS, "host_encode_all_ms": enc_all, "rows": rows}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r.get("checked", True) and r.get("fit", {}).get("checked_4096", True) and r.get("fit", {}).get("rows_ok", True) for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
