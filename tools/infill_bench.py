"""Span-corruption inputs and targets (gz_infill_rows_device, csrc/gz_infill.inc) over the windows and the packed rows of the
configs[2] corpus -- the rows of tools/mask_bench.py --, beside the mask call over the same rows, and the numpy restatement of the
rule on the host.

    python tools/infill_bench.py [--docs 1000000] [--reps 7] [--oracle-rows 4096] [--out profiles/infill_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit; its windows at
[W, 128] and [W, 256] (stride 0) and its packed rows at [R, 128] are made in HBM and stay there.  Per shape, host clock around
call + gz_sync, after a warm-up call of each, --reps rounds that run the two calls one after the other (interleaved), medians:
  mask_ms              gz_mask_rows_device, whole words, p = 0.15, 80 / 10 / 10: 4 bytes a cell in, 8 out -- the yardstick, which
                       this feature does not touch
  infill_ms            gz_infill_rows_device, p = 0.15, geometric lengths with mean 3 (max 10), whole words, dec_width = L / 2, all
                       seven outputs: 4 bytes a cell in, 8 + 8 dec_width / L = 12 out
  ratio                infill / mask over the same rows; by bytes 16 / 12 = 1.33
  achieved_gbs         16 bytes a cell / infill_ms;  hbm_fraction of HBM_PEAK_GBS (8000 GB/s, bench.py's constant)
  chosen_share         (dec_len - n_spans - 1) summed / unprotected cells, over the oracle's rows
  clipped_rows         rows with dec_len > dec_width
and once per shape the numpy oracle (tests/infill_oracle.py) over the first --oracle-rows rows: oracle_ns_per_cell, the device's ns
per cell beside it, and checked = the device's seven arrays equal the oracle's on those rows.  One JSON line on stdout.

On a shared GPU the step gets a time limit of its own:
    timeout -k 10 600 python tools/infill_bench.py --out profiles/infill_bench.json"""
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
SEED, P, MEAN_SPAN, MAX_SPAN, LAW = 20240607, 0.15, 3.0, 10, "geometric"


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
    import infill_oracle as IO
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
    rule = tok._infill_rule(P, MEAN_SPAN, MAX_SPAN, LAW, SEED, True, None, 0, -100)
    t_start, len_t, n_len = rule[1], rule[2], rule[3]
    assert (t_start, len_t, n_len) == IO.rule_ints(P, MEAN_SPAN, MAX_SPAN, LAW)
    cap = int(offs[n] - offs[0]) + 2 * n
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    d_ids, d_am, d_ro = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1))
    ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE, cap, d_ids, d_am, d_row_off=d_ro)
    ctx.sync()
    for d in (d_am, d_t, d_to):
        ctx.free(d)
    d_off = ctx.alloc(8 * (n + 1))
    d_maps, d_so = ctx.alloc(12 * n), ctx.alloc(8 * (n + 1))

    rows = []
    for kind, L in (("windows", 128), ("windows", 256), ("packs", 128)):
        if kind == "windows":
            R = ctx.window_rows_device(d_ids, d_ro, n, L, 0, 1, 1, 0, 0, 0, 0, 0, d_off, 0)
        else:
            R = ctx.pack_rows_device(d_ids, d_ro, n, L, 1, 1, 0, 0, 0, 0, d_maps, d_maps + 4 * n, d_maps + 8 * n, d_off, d_so, 0)
        cells, W = R * L, L // 2
        d_rows, d_aux = ctx.alloc(4 * cells), ctx.alloc(4 * cells)
        if kind == "windows":
            ctx.window_rows_device(d_ids, d_ro, n, L, 0, 1, 1, d_rows, d_aux, 0, 0, 0, d_off, R)
        else:
            ctx.pack_rows_device(d_ids, d_ro, n, L, 1, 1, d_rows, d_aux, 0, 0, d_maps, d_maps + 4 * n, d_maps + 8 * n, d_off, d_so, R)
        ctx.sync()
        ctx.free(d_aux)
        d_mo, d_ml, d_mc = ctx.alloc(4 * cells), ctx.alloc(4 * cells), ctx.alloc(4 * R)       # the mask call's outputs
        sizes = dict(input_ids=(R, L), attention_mask=(R, L), labels=(R, W), decoder_input_ids=(R, W), enc_len=(R,), dec_len=(R,), n_spans=(R,))
        dev = {k: ctx.alloc(4 * int(np.prod(s))) for k, s in sizes.items()}

        def mask():
            ctx.mask_rows_device(d_rows, R, L, 0, (SEED, t_sel, t1, t2, 5, n_ids, mask_id, 1, -100), d_mo, d_ml, d_mc)
            ctx.sync()

        def infill():
            ctx.infill_rows_device(d_rows, R, L, 0, (SEED, t_start, len_t, n_len, mask_id, 1, -100, W), *[dev[k] for k in IO.KEYS])
            ctx.sync()
        mask(); infill()                                             # warm-up
        t_mk, t_if = [], []
        for _ in range(args.reps):                                   # interleaved: every round runs the yardstick and the new call
            t_mk.append(timed(mask))
            t_if.append(timed(infill))
        mk_ms, if_ms = float(np.median(t_mk)), float(np.median(t_if))
        rec = {"rows_from": kind, "max_len": L, "dec_width": W, "rows": int(R), "cells": int(cells), "infill_ms": round(if_ms, 3),
               "infill_all_ms": [round(t, 3) for t in t_if], "mask_ms": round(mk_ms, 3), "mask_all_ms": [round(t, 3) for t in t_mk],
               "ratio": round(if_ms / mk_ms, 3), "ratio_by_bytes": round(16 / 12, 3), "bytes": int(16 * cells),
               "achieved_gbs": round(16 * cells / if_ms / 1e6, 1), "hbm_fraction": round(16 * cells / if_ms / 1e6 / HBM_PEAK_GBS, 4)}
        # the oracle on the host over the first rows, and the device's arrays against it
        k = min(args.oracle_rows, R)
        head = np.empty((k, L), dtype=np.int32)
        ctx.d2h(head, d_rows)
        res = {}

        def oracle():
            res["r"] = IO.infill(head, cont, pad, bos, eos, mask_id, seed=SEED, t_start=t_start, len_t=len_t, n_len=n_len, whole_word=True, dec_width=W)
        orc_ms = min(timed(oracle), timed(oracle))
        got = {key: np.empty((k,) + s[1:], np.int32) for key, s in sizes.items()}
        for key in got:
            ctx.d2h(got[key], dev[key])
        checked = all(bool(np.array_equal(got[key], res["r"][key])) for key in got)
        dl, ns = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.int32)
        ctx.d2h(dl, dev["dec_len"]); ctx.d2h(ns, dev["n_spans"])
        open_cells = int((~np.isin(head, [pad, bos, eos, mask_id])).sum())
        chosen_head = int((got["dec_len"].astype(np.int64) - got["n_spans"] - 1).sum())
        rec.update({"oracle_rows": int(k), "oracle_ms": round(orc_ms, 1), "oracle_ns_per_cell": round(orc_ms * 1e6 / (k * L), 2),
                    "device_ns_per_cell": round(if_ms * 1e6 / cells, 5), "oracle_over_device": round(orc_ms / (k * L) / (if_ms / cells), 0),
                    "spans": int(ns.astype(np.int64).sum()), "chosen_cells": int((dl.astype(np.int64) - ns - 1).sum()),
                    "mean_dec_len": round(float(dl.mean()), 2), "clipped_rows": int((dl > W).sum()),
                    "chosen_share": round(chosen_head / max(open_cells, 1), 4), "checked": checked})
        rows.append(rec)
        for d in [d_rows, d_mo, d_ml, d_mc] + list(dev.values()):
            ctx.free(d)
        print("# %s L=%d R=%d mask %.3f ms  infill %.3f ms (x%.2f)  %.0f GB/s  oracle %.1f ns/cell  checked %s" %
              (kind, L, R, mk_ms, if_ms, if_ms / mk_ms, rec["achieved_gbs"], rec["oracle_ns_per_cell"], checked), file=sys.stderr, flush=True)
    for d in (d_ids, d_ro, d_off, d_maps, d_so):
        ctx.free(d)
    rec = {"bench": "infill", "docs": n, "p": P, "lengths": LAW, "mean_span": MEAN_SPAN, "max_span": MAX_SPAN, "seed": SEED, "reps": args.reps,
           "hbm_peak_gbs": HBM_PEAK_GBS, "rows": rows}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["checked"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
