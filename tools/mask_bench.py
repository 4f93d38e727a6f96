"""Masked-LM inputs and labels (gz_mask_rows_device, csrc/gz_mask.inc) over the windows and the packed rows of the configs[2] corpus,
beside the window call that produces the same cells, and the numpy restatement of the rule on the host.

    python tools/mask_bench.py [--docs 1000000] [--reps 7] [--oracle-rows 4096] [--out profiles/mask_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit; its windows at
[W, 128] and [W, 256] (stride 0) and its packed rows at [R, 128] are made in HBM and stay there.  Per shape, host clock around
call + gz_sync, after a warm-up call of each, --reps rounds that run the three calls one after the other (interleaved), medians:
  window_ms            gz_window_rows_device filling the same [W, L] input_ids and attention_mask (8 bytes a cell out): the yardstick,
                       unchanged by this feature.  For the packed rows it is a window call over the first documents of the corpus whose
                       windows number R or a few less (window_rows; window_ms is scaled to R rows by that handful), writing into
                       scratch arrays of the same size in the same rounds
  mask_whole_word_ms   gz_mask_rows_device, whole_word = 1: 4 bytes a cell in, 8 out, one look at the continuation bitmap in LDS
  mask_per_token_ms    the same with whole_word = 0 (no bitmap)
  ratio_*              mask / window over the same cells; the goal is <= 1.5
  achieved_gbs         12 bytes a cell / mask_whole_word_ms;  hbm_fraction of HBM_PEAK_GBS (8000 GB/s, bench.py's constant)
  chosen_share         chosen cells / unprotected cells at p = 0.15, whole words
and once per shape the vectorised numpy oracle (tests/mask_oracle.py) over the first --oracle-rows rows: oracle_ns_per_cell, the
device's ns per cell beside it, and checked = the device's three arrays equal the oracle's on those rows.  One JSON line on stdout.

On a shared GPU every step gets a time limit of its own and the steps are chained, so that nothing starts behind a step that failed:
    timeout -k 10 600 python tools/mask_bench.py --out profiles/mask_bench.json && \\
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/mask_prof -- python tools/mask_bench.py --reps 3"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "genz-tokenize_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec peak: the constant of bench.py
SEED, P = 20240607, 0.15


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    import mask_oracle as MO
    from genz_tokenize import Tokenize, _native
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n = len(offs) - 1
    tok = Tokenize()
    tok._sync_tables()
    ctx = tok._ctx
    pad, bos, eos, mask_id = tok._special_ids()[:4]
    n_ids = tok.vocab_size()
    cont = MO.continuation_ids(tok.vocab_file)
    t_sel, t1, t2 = MO.thresholds(P)
    cap = int(offs[n] - offs[0]) + 2 * n
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    d_ids, d_am, d_ro = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1))
    ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE, cap, d_ids, d_am, d_row_off=d_ro)
    ctx.sync()
    for d in (d_am, d_t, d_to):
        ctx.free(d)
    d_off, d_wo = ctx.alloc(8 * (n + 1)), ctx.alloc(8 * (n + 1))
    d_maps, d_so = ctx.alloc(12 * n), ctx.alloc(8 * (n + 1))

    rows = []
    for kind, L in (("windows", 128), ("windows", 256), ("packs", 128)):
        if kind == "windows":
            R = ctx.window_rows_device(d_ids, d_ro, n, L, 0, 1, 1, 0, 0, 0, 0, 0, d_off, 0)
        else:
            R = ctx.pack_rows_device(d_ids, d_ro, n, L, 1, 1, 0, 0, 0, 0, d_maps, d_maps + 4 * n, d_maps + 8 * n, d_off, d_so, 0)
        cells = R * L
        d_rows, d_aux, d_out, d_lab, d_cnt = ctx.alloc(4 * cells), ctx.alloc(4 * cells), ctx.alloc(4 * cells), ctx.alloc(4 * cells), ctx.alloc(4 * R)

        n_win, W_win = n, R
        if kind == "packs":                                          # as many leading documents as make R windows, or a few less
            ctx.window_rows_device(d_ids, d_ro, n, L, 0, 1, 1, 0, 0, 0, 0, 0, d_wo, 0)
            win_off = np.empty(n + 1, dtype=np.int64)
            ctx.d2h(win_off, d_wo)
            n_win = int(np.searchsorted(win_off, R, side="right")) - 1
            W_win = int(win_off[n_win])

        def window():                                                # (packs: into the mask call's outputs, which the calls behind it in the round overwrite)
            if kind == "windows":
                ctx.window_rows_device(d_ids, d_ro, n, L, 0, 1, 1, d_rows, d_aux, 0, 0, 0, d_off, R)
            else:
                ctx.window_rows_device(d_ids, d_ro, n_win, L, 0, 1, 1, d_out, d_lab, 0, 0, 0, d_wo, W_win)
            ctx.sync()

        def mask(ww):
            ctx.mask_rows_device(d_rows, R, L, 0, (SEED, t_sel, t1, t2, 5, n_ids, mask_id, ww, -100), d_out, d_lab, d_cnt)
            ctx.sync()
        window()
        if kind == "packs":
            ctx.pack_rows_device(d_ids, d_ro, n, L, 1, 1, d_rows, d_aux, 0, 0, d_maps, d_maps + 4 * n, d_maps + 8 * n, d_off, d_so, R)
            ctx.sync()
        mask(0); mask(1)                                             # warm-up (whole_word = 1 last: its arrays are the ones checked below)
        t_win, t_ww, t_pt = [], [], []
        for _ in range(args.reps):                                   # interleaved: every round runs the yardstick and both forms
            t_win.append(timed(window))
            t_pt.append(timed(lambda: mask(0)))
            t_ww.append(timed(lambda: mask(1)))
        ww_ms, pt_ms = float(np.median(t_ww)), float(np.median(t_pt))
        rec = {"rows_from": kind, "max_len": L, "rows": int(R), "cells": int(cells), "mask_whole_word_ms": round(ww_ms, 3),
               "mask_whole_word_all_ms": [round(t, 3) for t in t_ww], "mask_per_token_ms": round(pt_ms, 3),
               "mask_per_token_all_ms": [round(t, 3) for t in t_pt], "bytes": int(12 * cells),
               "achieved_gbs": round(12 * cells / ww_ms / 1e6, 1), "hbm_fraction": round(12 * cells / ww_ms / 1e6 / HBM_PEAK_GBS, 4)}
        win_ms = float(np.median(t_win)) * R / W_win                 # (packs: W_win is R or a few rows less)
        rec.update({"window_ms": round(win_ms, 3), "window_all_ms": [round(t, 3) for t in t_win], "window_rows": int(W_win), "window_docs": int(n_win)})
        rec.update({"ratio_whole_word": round(ww_ms / win_ms, 3), "ratio_per_token": round(pt_ms / win_ms, 3), "goal_ratio": 1.5,
                    "goal_met": bool(ww_ms / win_ms <= 1.5)})
        # the oracle on the host over the first rows, and the device's arrays against it
        k = min(args.oracle_rows, R)
        head = np.empty((k, L), dtype=np.int32)
        ctx.d2h(head, d_rows)
        res = {}

        def oracle():
            res["r"] = MO.mask(head, cont, pad, bos, eos, mask_id, seed=SEED, t_sel=t_sel, t1=t1, t2=t2, rand_lo=5, rand_hi=n_ids, whole_word=True)
        orc_ms = min(timed(oracle), timed(oracle))
        got = {"input_ids": np.empty((k, L), np.int32), "labels": np.empty((k, L), np.int32), "n_chosen": np.empty(k, np.int32)}
        ctx.d2h(got["input_ids"], d_out); ctx.d2h(got["labels"], d_lab); ctx.d2h(got["n_chosen"], d_cnt)
        checked = all(bool(np.array_equal(got[key], res["r"][key])) for key in got)
        counts = np.empty(R, dtype=np.int32)
        ctx.d2h(counts, d_cnt)
        open_cells = int((~np.isin(head, [pad, bos, eos, mask_id])).sum())
        rec.update({"oracle_rows": int(k), "oracle_ms": round(orc_ms, 1), "oracle_ns_per_cell": round(orc_ms * 1e6 / (k * L), 2),
                    "device_ns_per_cell": round(ww_ms * 1e6 / cells, 5), "oracle_over_device": round(orc_ms / (k * L) / (ww_ms / cells), 0),
                    "chosen_cells": int(counts.astype(np.int64).sum()),
                    "chosen_share": round(int(got["n_chosen"].astype(np.int64).sum()) / max(open_cells, 1), 4), "checked": checked})
        rows.append(rec)
        for d in (d_rows, d_aux, d_out, d_lab, d_cnt):
            ctx.free(d)
        print("# %s L=%d R=%d window %.3f ms  mask whole-word %.3f ms (x%.2f)  per-token %.3f ms (x%.2f)  oracle %.1f ns/cell  checked %s" %
              (kind, L, R, win_ms, ww_ms, ww_ms / win_ms, pt_ms, pt_ms / win_ms, rec["oracle_ns_per_cell"], checked), file=sys.stderr, flush=True)
    for d in (d_ids, d_ro, d_off, d_wo, d_maps, d_so):
        ctx.free(d)
    rec = {"bench": "mask", "docs": n, "p": P, "seed": SEED, "reps": args.reps, "hbm_peak_gbs": HBM_PEAK_GBS, "rows": rows}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["checked"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
