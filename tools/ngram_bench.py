"""Exact token n-gram overlap (gz_ngram_index_build_device, gz_ngram_overlap_device; csrc/gz_ngram.inc) over the configs[2] corpus with
its token rows resident in HBM, against an index of reference documents at n = 13 -- beside the MinHash signature call at 128 slots
and the encode launch of the same documents, measured in the same visit, and the set-of-tuples rule on the host.

    python tools/ngram_bench.py [--docs 1000000] [--refs 10000] [--n 13] [--reps 7] [--runs 2] [--oracle-rows 4096] [--out profiles/ngram_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit and stays there.  The reference
set is --refs of its documents, evenly spaced (every 100th by default: one document in a hundred is contaminated in full, the others
share what running text shares by chance), gathered into rows of their own.  Host clock around call + gz_sync, after a warm-up call
of each; --reps rounds that run the encode launch, the signature pass and the query one after the other (interleaved), medians;
--runs such series, each reported.
  build        the index from the reference rows in HBM: ms, reference ids, n-gram positions, distinct n-grams, slots, device bytes
  query        the five per-document arrays over the whole corpus, and with the covered bytes as well: ms, positions probed, probes_per_s,
               minhash_ms and encode_ms beside it, ratio_to_minhash = ms / minhash_ms (the goal, not a gate: <= 1) and ratio_to_encode
  oracle       tests/ngram_oracle.py (a dict of tuples) over the first --oracle-rows documents against the same reference set:
               oracle_ns_per_token, the device's beside it, and checked = all five arrays and the covered bytes equal the oracle's there
One JSON line on stdout.

On a shared GPU every step gets a time limit of its own and the steps are chained, so that nothing starts behind a step that failed:
    timeout -k 10 900 python tools/ngram_bench.py --out profiles/ngram_bench.json"""
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
OUT = ("n_grams", "n_hits", "n_covered", "first_hit", "first_ref")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--refs", type=int, default=10_000)
    ap.add_argument("--n", type=int, default=13)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--oracle-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    import ngram_oracle as NO
    from genz_tokenize import Tokenize, _native
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
    ids = np.empty(total, dtype=np.int32)
    ctx.d2h(ids, d_ids)
    # the reference rows: evenly spaced documents of the corpus, gathered into rows of their own in HBM
    R = min(args.refs, n)
    picks = (np.arange(R, dtype=np.int64) * n) // R
    lens = row_off[picks + 1] - row_off[picks]
    ref_off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(lens, out=ref_off[1:])
    ref_ids = ids[np.repeat(row_off[picks] - ref_off[:-1], lens) + np.arange(ref_off[R], dtype=np.int64)]
    d_rids, d_rro = ctx.alloc(ref_ids.nbytes + 64), ctx.alloc(ref_off.nbytes)
    ctx.h2d(d_rids, ref_ids); ctx.h2d(d_rro, ref_off)
    d_out = ctx.alloc(4 * len(OUT) * n + 64)
    d_cov = ctx.alloc(total + 64)
    d_sig, d_cnt = ctx.alloc(4 * 128 * n), ctx.alloc(4 * n)
    outs = [d_out + 4 * n * k for k in range(len(OUT))]

    # build
    held = {}

    def build():
        if "h" in held:
            ctx.ngram_index_destroy(held.pop("h"))
        held["h"] = ctx.ngram_index_build_device(d_rids, d_rro, R, 1, 1, w)
    build()
    build_series = []
    for _ in range(args.runs):
        ts = [timed(build) for _ in range(args.reps)]
        build_series.append((float(np.median(ts)), ts))
    info = ctx.ngram_index_info(held["h"])
    build_rec = {"reference_docs": int(R), "n": w, "ms": round(build_series[0][0], 3), "ms_runs": [round(s[0], 3) for s in build_series],
                 "all_ms": [[round(t, 3) for t in s[1]] for s in build_series], "reference_ids": info["n_ids"], "positions": info["n_grams"],
                 "distinct": info["n_distinct"], "slots": info["slots"], "device_bytes": info["device_bytes"],
                 "bytes_per_reference_token": round(info["device_bytes"] / max(info["n_ids"] - 2 * R, 1), 2)}
    print("# build: %.3f ms (runs %s)  %d ids, %d positions, %d distinct, %d slots, %d bytes" %
          (build_rec["ms"], build_rec["ms_runs"], info["n_ids"], info["n_grams"], info["n_distinct"], info["slots"], info["device_bytes"]),
          file=sys.stderr, flush=True)

    # query, beside the signature call and the encode launch
    body = np.maximum(row_off[1:] - row_off[:-1] - 2, 0)
    positions = int(np.maximum(body - w + 1, 0).sum())
    tokens = int(body.sum())

    def sign():
        ctx.minhash_rows_device(d_ids, d_ro, n, 1, 1, 5, 128, SEED, d_sig, d_cnt)
        ctx.sync()
    query_rows = []
    for name, cov in (("five per-document arrays", 0), ("five per-document arrays + covered bytes", d_cov)):
        def query():
            ctx.ngram_overlap_device(held["h"], d_ids, d_ro, n, 1, 1, *outs, cov)
        query(); sign(); encode()
        series = []
        for _ in range(args.runs):
            t_q, t_sig, t_enc = [], [], []
            for _ in range(args.reps):
                t_enc.append(timed(encode))
                t_sig.append(timed(sign))
                t_q.append(timed(query))
            series.append((float(np.median(t_q)), float(np.median(t_sig)), float(np.median(t_enc)), t_q, t_sig, t_enc))
        ms, sig_ms, enc_ms = series[0][:3]
        rec = {"outputs": name, "docs": int(n), "tokens": tokens, "positions": positions, "ms": round(ms, 3), "ms_runs": [round(s[0], 3) for s in series],
               "all_ms": [[round(t, 3) for t in s[3]] for s in series], "minhash_ms": round(sig_ms, 3), "minhash_ms_runs": [round(s[1], 3) for s in series],
               "encode_ms": round(enc_ms, 3), "encode_ms_runs": [round(s[2], 3) for s in series], "probes_per_s": round(positions / ms * 1e3, 0),
               "ratio_to_minhash": round(ms / sig_ms, 3), "ratio_to_encode": round(ms / enc_ms, 3)}
        query_rows.append(rec)
        print("# query (%s): %.3f ms (runs %s)  %.3e probes/s  minhash %.3f ms  encode %.3f ms  ratio to minhash %.3f" %
              (name, ms, rec["ms_runs"], rec["probes_per_s"], sig_ms, enc_ms, rec["ratio_to_minhash"]), file=sys.stderr, flush=True)

    # the oracle on the host over the first documents, and the device's output against it
    k = min(args.oracle_rows, n)
    ctx.ngram_overlap_device(held["h"], d_ids, d_ro, n, 1, 1, *outs, d_cov)
    got = np.empty((len(OUT), n), dtype=np.int32)
    ctx.d2h(got, d_out)
    got_cov = np.empty(int(row_off[k]), dtype=np.uint8)
    ctx.d2h(got_cov, d_cov)
    head = [ids[row_off[r]:row_off[r + 1]].tolist() for r in range(k)]
    refs = [ref_ids[ref_off[r]:ref_off[r + 1]].tolist() for r in range(R)]
    res = {}

    def host_index():
        res["first"] = NO.index(refs, w, framed=True)

    def host_query():
        res["r"] = NO.overlap(res["first"], w, head, framed=True)
    index_ms = timed(host_index)
    orc_ms = min(timed(host_query), timed(host_query))
    checked = bool(all(np.array_equal(got[i][:k], res["r"][key]) for i, key in enumerate(OUT)) and np.array_equal(got_cov, res["r"]["covered"])
                   and info["n_distinct"] == len(res["first"]))
    assert checked, "the device's outputs differ from the host rule on the first %d documents" % k
    head_tokens = int(res["r"]["body_len"].sum())
    oracle_rec = {"oracle_rows": int(k), "oracle_tokens": head_tokens, "oracle_index_ms": round(index_ms, 1), "oracle_ms": round(orc_ms, 1),
                  "oracle_ns_per_token": round(orc_ms * 1e6 / max(head_tokens, 1), 1),
                  "device_ns_per_token": round(query_rows[0]["ms"] * 1e6 / max(tokens, 1), 4), "checked": checked,
                  "documents_with_hits": int((got[1] > 0).sum()), "tokens_covered": int(got[2].sum())}
    print("# oracle %.1f ns/token (index %.1f ms), device %.4f ns/token, checked %s; %d documents with hits, %d tokens covered" %
          (oracle_rec["oracle_ns_per_token"], index_ms, oracle_rec["device_ns_per_token"], checked, oracle_rec["documents_with_hits"],
           oracle_rec["tokens_covered"]), file=sys.stderr, flush=True)
    ctx.ngram_index_destroy(held.pop("h"))
    for d in (d_t, d_to, d_ids, d_am, d_ro, d_rids, d_rro, d_out, d_cov, d_sig, d_cnt):
        ctx.free(d)
    rec = {"bench": "ngram", "docs": n, "seed": SEED, "reps": args.reps, "runs": args.runs, "piece": 4096, "build": build_rec, "query": query_rows,
           "oracle": oracle_rec}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
