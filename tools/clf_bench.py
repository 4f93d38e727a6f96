"""Hashed n-gram class models (gz_ngram_clf_fit_device, gz_ngram_clf_score_device; csrc/gz_clf.inc) over the configs[2] corpus with its
token rows resident in HBM, as tools/lm_bench.py holds them: a two-class model of order 2 fitted on the first 100 000 documents (labels
alternate) and all documents scored, at 2^14 and at 2^20 buckets, each with the LDS paths on and off (switch clf_lds) -- beside the
order-2 language model's build over the same training rows and its perplexity call over the same documents, measured in the same
visit, and the Counter rule on the host.

    python tools/clf_bench.py [--docs 1000000] [--train 100000] [--bits 14,20] [--reps 5] [--oracle-rows 4096] [--out profiles/clf_bench.json]

Host clock around call + gz_sync, after a warm-up call of each; --reps rounds that run the calls one after the other (interleaved),
medians and the spread (max - min) of each.  A fit is timed into a fresh model (its creation not timed).
  settings     per bits: fit_ms and score_ms with clf_lds 1 and 0, which paths those were (fit_lds, score_lds), lm_build_ms and
               perplexity_ms beside them, score_ratio_to_perplexity (clf_lds 1), features, device bytes
  oracle       tests/clf_oracle.py over the first --oracle-rows documents (fitted and scored) at the first setting: counts and
               n_features equal, weights within 1, bits_fx equal to the device's weights summed at the oracle's buckets; asserted
One JSON line on stdout.

On a shared GPU every step gets a time limit of its own and the steps are chained, so that nothing starts behind a step that failed:
    timeout -k 10 900 python tools/clf_bench.py --out profiles/clf_bench.json"""
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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--train", type=int, default=100_000)
    ap.add_argument("--bits", default="14,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import clf_oracle as CO
    import corpus
    from genz_tokenize import Tokenize, _native
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n, N, C = len(offs) - 1, 2, 2
    R = min(args.train, n)
    tok = Tokenize()
    tok._sync_tables()
    ctx = tok._ctx
    cap = int(offs[n] - offs[0]) + 2 * n
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    d_ids, d_am, d_ro = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1))
    ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE, cap, d_ids, d_am, d_row_off=d_ro)
    ctx.sync()
    row_off = np.empty(n + 1, dtype=np.int64)
    ctx.d2h(row_off, d_ro)
    tokens = int(np.maximum(row_off[1:] - row_off[:-1] - 2, 0).sum())
    labels = (np.arange(n) % C).astype(np.int32)
    d_lab = ctx.alloc(labels.nbytes)
    ctx.h2d(d_lab, labels)
    d_out = ctx.alloc(4 * n + 8 * C * n + 4 * n + 64)                     # n_features, bits_fx, best
    d_nf, d_bits, d_best = d_out, d_out + 4 * n, d_out + 4 * n + 8 * C * n
    d_lm = ctx.alloc(8 * n + 4 * n + 4 * (N + 1) * n + 64)               # the perplexity call's bits_fx, n_tokens, n_order
    settings, oracle_rec = [], None
    for bits in [int(b) for b in args.bits.split(",")]:
        held = {}

        def fit(lds):
            if "clf" in held:
                ctx.ngram_clf_destroy(held.pop("clf"))
            _native.debug_set("clf_lds", lds, ctx)
            held["clf"] = ctx.ngram_clf_create(N, bits, C, 1.0)
            return timed(lambda: ctx.ngram_clf_fit_device(held["clf"], d_ids, d_ro, d_lab, R, 1, 1))

        def score(lds):
            _native.debug_set("clf_lds", lds, ctx)
            ctx.ngram_clf_score_device(held["clf"], d_ids, d_ro, n, 1, 1, d_nf, d_bits, d_best)

        def lm_build():
            if "lm" in held:
                ctx.ngram_lm_destroy(held.pop("lm"))
            held["lm"] = ctx.ngram_lm_build_device(d_ids, d_ro, R, 1, 1, N)

        def perplexity():
            ctx.ngram_lm_score_device(held["lm"], d_ids, d_ro, n, 1, 1, 0.4, d_lm + 8 * n, d_lm, d_lm + 12 * n, 0, 0, 0)
        fit(0); fit(1); score(1); score(0); lm_build(); perplexity()
        paths = {}
        t = {k: [] for k in ("fit_lds1", "fit_lds0", "score_lds1", "score_lds0", "lm_build", "perplexity")}
        for _ in range(args.reps):
            for lds in (1, 0):
                t["fit_lds%d" % lds].append(fit(lds))
                t["score_lds%d" % lds].append(timed(lambda: score(lds)))
                paths[lds] = ctx.ngram_clf_info(held["clf"])
            t["lm_build"].append(timed(lm_build))
            t["perplexity"].append(timed(perplexity))
        _native.debug_set("clf_lds", 1, ctx)
        med = {k: float(np.median(v)) for k, v in t.items()}
        info = paths[1]
        rec = {"bits": bits, "order": N, "classes": C, "train_docs": int(R), "features": info["n_features"], "device_bytes": info["device_bytes"],
               "fit_lds": info["fit_lds"], "score_lds": info["score_lds"],
               "score_ratio_to_perplexity": round(med["score_lds1"] / med["perplexity"], 3), "fit_ratio_to_lm_build": round(med["fit_lds1"] / med["lm_build"], 3),
               "tokens_per_s": round(tokens / med["score_lds1"] * 1e3, 0)}
        rec.update({k + "_ms": round(v, 3) for k, v in med.items()})
        rec.update({k + "_spread_ms": round(max(v) - min(v), 3) for k, v in t.items()})
        rec["all_ms"] = {k: [round(x, 3) for x in v] for k, v in t.items()}
        settings.append(rec)
        print("# bits %d: fit %.3f ms (clf_lds 0: %.3f), score %.3f ms (clf_lds 0: %.3f); lm build %.3f ms, perplexity %.3f ms" %
              (bits, med["fit_lds1"], med["fit_lds0"], med["score_lds1"], med["score_lds0"], med["lm_build"], med["perplexity"]), file=sys.stderr, flush=True)
        if oracle_rec is None:
            k = min(args.oracle_rows, R)
            ids = np.empty(int(row_off[k]), dtype=np.int32)
            ctx.d2h(ids, d_ids)
            docs = [ids[row_off[r]:row_off[r + 1]].tolist() for r in range(k)]
            t0 = time.perf_counter()
            count, _ = CO.fit(docs, labels[:k], N, bits, C, framed=True)
            w = CO.weights(count)
            want = CO.score(w, N, bits, docs, framed=True)
            host_ms = (time.perf_counter() - t0) * 1e3
            clf = ctx.ngram_clf_create(N, bits, C, 1.0)
            ctx.ngram_clf_fit_device(clf, d_ids, d_ro, d_lab, k, 1, 1)
            dw = ctx.ngram_clf_weights(clf, bits, C).astype(np.int64)
            ctx.ngram_clf_score_device(clf, d_ids, d_ro, k, 1, 1, d_nf, d_bits, d_best)
            nf, fx = np.empty(k, dtype=np.int32), np.empty((C, k), dtype=np.int64)
            ctx.d2h(nf, d_nf); ctx.d2h(fx, d_bits)
            sums = np.stack([dw[b].sum(axis=0) if len(b) else np.zeros(C, np.int64) for b in want["buckets"]], axis=1)
            checked = bool(np.array_equal(ctx.ngram_clf_counts(clf, bits, C), count) and np.abs(dw - w).max() <= 1 and np.array_equal(nf, want["n_features"])
                           and np.array_equal(fx, sums))
            ctx.ngram_clf_destroy(clf)
            assert checked, "the device's outputs differ from the host rule on the first %d documents" % k
            oracle_rec = {"oracle_rows": int(k), "bits": bits, "oracle_ms": round(host_ms, 1), "weights_max_diff": int(np.abs(dw - w).max()), "checked": checked}
            print("# oracle: %.0f ms on the host over %d documents; checked %s" % (host_ms, k, checked), file=sys.stderr, flush=True)
        ctx.ngram_clf_destroy(held.pop("clf"))
        ctx.ngram_lm_destroy(held.pop("lm"))
    for d in (d_t, d_to, d_ids, d_am, d_ro, d_lab, d_out, d_lm):
        ctx.free(d)
    rec = {"bench": "clf", "docs": n, "tokens": tokens, "reps": args.reps, "piece": 4096, "settings": settings, "oracle": oracle_rec}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
