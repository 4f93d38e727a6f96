"""n-gram repetition inside a document (gz_ngram_repeats_device; csrc/gz_repeat.inc) over the configs[2] corpus with its token rows
resident in HBM: the default nine widths, and n = 13 alone beside the same insert-all and probe-all work on a table without counts --
an n-gram index built over ALL the rows and those rows queried against it --, the MinHash signature call at 128 slots and the encode
launch of the same documents, measured in the same visit, and the Counter rule on the host.

    python tools/repeat_bench.py [--docs 1000000] [--n 13] [--reps 7] [--runs 2] [--oracle-rows 4096] [--out profiles/repeat_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit and stays there.  Host clock
around call + gz_sync, after a warm-up call of each; --reps rounds that run the calls one after the other (interleaved), medians;
--runs such series, each reported.
  nine         the six [9, N] arrays at widths 2..10, and with the covered bits as well: ms, positions, positions_per_s
  single       the six [1, N] arrays at n = --n: ms; index_build_ms (gz_ngram_index_build_device over all rows) and overlap_ms
               (gz_ngram_overlap_device of those rows against that index) beside it; ratio = ms / (index_build_ms + overlap_ms), the
               goal (not a gate) <= 1.25: a quarter for the count atomic, the 12-byte slot and the clear; minhash_ms and encode_ms
  oracle       tests/repeat_oracle.py (collections.Counter over tuples) over the first --oracle-rows documents at the nine widths:
               oracle_ns_per_token, the device's beside it, and checked = all six arrays and the covered bits equal the rule's there
One JSON line on stdout.

On a shared GPU every step gets a time limit of its own and the steps are chained, so that nothing starts behind a step that failed:
    timeout -k 10 900 python tools/repeat_bench.py --out profiles/repeat_bench.json"""
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

SEED = 20240607
NINE = (2, 3, 4, 5, 6, 7, 8, 9, 10)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=13)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--oracle-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    import repeat_oracle as RO
    from genz_tokenize import Tokenize, _native
    OUT = _native.Context.REPEAT_OUT
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n, w = len(offs) - 1, args.n
    tok = Tokenize()
    tok._sync_tables()
    ctx = tok._ctx
    cap = int(offs[n] - offs[0]) + 2 * n
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    d_ids, d_am, d_ro = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1))

    def encode():
        ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE, cap, d_ids, d_am, d_row_off=d_ro)
        ctx.sync()
    encode()
    row_off = np.empty(n + 1, dtype=np.int64)
    ctx.d2h(row_off, d_ro)
    total = int(row_off[n])
    K = len(NINE)
    d_out = ctx.alloc(4 * len(OUT) * K * n + 64)
    d_cov = ctx.alloc(2 * total + 64)
    d_sig, d_cnt = ctx.alloc(4 * 128 * n), ctx.alloc(4 * n)
    body = np.maximum(row_off[1:] - row_off[:-1] - 2, 0)
    tokens = int(body.sum())

    def outs(k):
        return [d_out + 4 * k * n * i for i in range(len(OUT))]

    def sign():
        ctx.minhash_rows_device(d_ids, d_ro, n, 1, 1, 5, 128, SEED, d_sig, d_cnt)
        ctx.sync()

    # the nine default widths
    positions9 = int(sum(np.maximum(body - v + 1, 0).sum() for v in NINE))
    nine_rows = []
    for name, cov in (("six [9, N] arrays", 0), ("six [9, N] arrays + covered bits", d_cov)):
        def nine():
            ctx.ngram_repeats_device(d_ids, d_ro, n, 1, 1, NINE, *outs(K), cov)
        nine()
        series = []
        for _ in range(args.runs):
            ts = [timed(nine) for _ in range(args.reps)]
            series.append((float(np.median(ts)), ts))
        ms = series[0][0]
        rec = {"outputs": name, "widths": list(NINE), "docs": int(n), "tokens": tokens, "positions": positions9, "ms": round(ms, 3),
               "ms_runs": [round(s[0], 3) for s in series], "all_ms": [[round(t, 3) for t in s[1]] for s in series],
               "positions_per_s": round(positions9 / ms * 1e3, 0), "ms_per_width": round(ms / K, 3)}
        nine_rows.append(rec)
        print("# nine widths (%s): %.3f ms (runs %s)  %.3e positions/s" % (name, ms, rec["ms_runs"], rec["positions_per_s"]), file=sys.stderr, flush=True)

    # one width, beside the index build over all rows and the query of those rows against it
    positions1 = int(np.maximum(body - w + 1, 0).sum())
    d_five = ctx.alloc(4 * 5 * n + 64)
    five = [d_five + 4 * n * k for k in range(5)]
    held = {}

    def single():
        ctx.ngram_repeats_device(d_ids, d_ro, n, 1, 1, (w,), *outs(1), 0)

    def build():
        if "h" in held:
            ctx.ngram_index_destroy(held.pop("h"))
        held["h"] = ctx.ngram_index_build_device(d_ids, d_ro, n, 1, 1, w)

    def overlap():
        ctx.ngram_overlap_device(held["h"], d_ids, d_ro, n, 1, 1, *five, 0)
    single(); build(); overlap(); sign(); encode()
    series = []
    for _ in range(args.runs):
        t = {k: [] for k in ("encode", "minhash", "build", "overlap", "single")}
        for _ in range(args.reps):
            t["encode"].append(timed(encode))
            t["minhash"].append(timed(sign))
            t["build"].append(timed(build))
            t["overlap"].append(timed(overlap))
            t["single"].append(timed(single))
        series.append(({k: float(np.median(v)) for k, v in t.items()}, t))
    info = ctx.ngram_index_info(held["h"])
    med = series[0][0]
    goal = 1.25
    single_rec = {"n": w, "docs": int(n), "tokens": tokens, "positions": positions1, "ms": round(med["single"], 3),
                  "ms_runs": [round(s[0]["single"], 3) for s in series], "all_ms": [[round(x, 3) for x in s[1]["single"]] for s in series],
                  "index_build_ms": round(med["build"], 3), "index_build_ms_runs": [round(s[0]["build"], 3) for s in series],
                  "overlap_ms": round(med["overlap"], 3), "overlap_ms_runs": [round(s[0]["overlap"], 3) for s in series],
                  "ratio": round(med["single"] / (med["build"] + med["overlap"]), 3),
                  "ratio_runs": [round(s[0]["single"] / (s[0]["build"] + s[0]["overlap"]), 3) for s in series], "goal": goal,
                  "goal_met": bool(med["single"] <= goal * (med["build"] + med["overlap"])),
                  "minhash_ms": round(med["minhash"], 3), "minhash_ms_runs": [round(s[0]["minhash"], 3) for s in series],
                  "encode_ms": round(med["encode"], 3), "encode_ms_runs": [round(s[0]["encode"], 3) for s in series],
                  "positions_per_s": round(positions1 / med["single"] * 1e3, 0), "index_slots": info["slots"], "index_distinct": info["n_distinct"]}
    print("# n = %d: %.3f ms (runs %s)  index build %.3f + overlap %.3f ms  ratio %.3f (goal <= %.2f: %s)  minhash %.3f ms  encode %.3f ms" %
          (w, med["single"], single_rec["ms_runs"], med["build"], med["overlap"], single_rec["ratio"], goal,
           "met" if single_rec["goal_met"] else "MISSED", med["minhash"], med["encode"]), file=sys.stderr, flush=True)
    ctx.ngram_index_destroy(held.pop("h"))

    # the rule on the host over the first documents, and the device's output against it
    k = min(args.oracle_rows, n)
    ctx.ngram_repeats_device(d_ids, d_ro, n, 1, 1, NINE, *outs(K), d_cov)
    got = np.empty((len(OUT), K, n), dtype=np.int32)
    ctx.d2h(got, d_out)
    got_cov = np.empty(int(row_off[k]), dtype=np.uint16)
    ctx.d2h(got_cov, d_cov)
    ids = np.empty(int(row_off[k]), dtype=np.int32)
    ctx.d2h(ids, d_ids)
    head = [ids[row_off[r]:row_off[r + 1]].tolist() for r in range(k)]
    res = {}

    def host_rule():
        res["r"] = RO.repetition(head, NINE, framed=True)
    orc_ms = timed(host_rule)
    checked = bool(all(np.array_equal(got[i][:, :k], res["r"][key]) for i, key in enumerate(OUT)) and np.array_equal(got_cov, res["r"]["covered"]))
    assert checked, "the device's outputs differ from the host rule on the first %d documents" % k
    head_tokens = int(res["r"]["body_len"].sum())
    b1 = np.maximum(body, 1).astype(np.float64)
    keep = np.ones(n, dtype=bool)
    for v, bound in Tokenize.REPEAT_TOP_MAX.items():
        keep &= v * got[4][NINE.index(v)] / b1 <= bound
    for v, bound in Tokenize.REPEAT_DUP_MAX.items():
        keep &= got[3][NINE.index(v)] / b1 <= bound
    oracle_rec = {"oracle_rows": int(k), "oracle_tokens": head_tokens, "widths": list(NINE), "oracle_ms": round(orc_ms, 1),
                  "oracle_ns_per_token": round(orc_ms * 1e6 / max(head_tokens, 1), 1),
                  "device_ns_per_token": round(nine_rows[0]["ms"] * 1e6 / max(tokens, 1), 4), "checked": checked,
                  "documents_with_a_repeated_5gram": int((got[2][NINE.index(5)] > 0).sum()), "documents_kept_by_default_bounds": int(keep.sum())}
    print("# rule on the host %.1f ns/token, device %.4f ns/token, checked %s; %d documents repeat a 5-gram, the default bounds keep %d" %
          (oracle_rec["oracle_ns_per_token"], oracle_rec["device_ns_per_token"], checked, oracle_rec["documents_with_a_repeated_5gram"],
           oracle_rec["documents_kept_by_default_bounds"]), file=sys.stderr, flush=True)
    for d in (d_t, d_to, d_ids, d_am, d_ro, d_out, d_cov, d_sig, d_cnt, d_five):
        ctx.free(d)
    rec = {"bench": "repeat", "docs": n, "seed": SEED, "reps": args.reps, "runs": args.runs, "piece": 4096, "nine": nine_rows, "single": single_rec,
           "oracle": oracle_rec}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
