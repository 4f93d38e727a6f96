"""Token n-gram language model and perplexity (gz_ngram_lm_build_device, gz_ngram_lm_score_device; csrc/gz_lm.inc) over the configs[2]
corpus with its token rows resident in HBM: a model of order 5 trained on the first 10 000 and the first 100 000 documents, all
documents scored -- beside the n-gram index build over the same training rows and the overlap query over the same documents at
n = 5, measured in the same visit, and the Counter-of-tuples rule on the host.

    python tools/lm_bench.py [--docs 1000000] [--train 10000,100000] [--order 5] [--reps 5] [--oracle-rows 4096] [--out profiles/lm_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit and stays there; the
training rows are its first documents, in place.  Host clock around call + gz_sync, after a warm-up call of each; --reps rounds that
run the calls one after the other (interleaved), medians.
  build        per training size: ms without and with the in-wave combining of equal unigrams and bigrams (switch lm_combine), the
               index build's ms beside them and ratio_to_index; training tokens, gram positions and distinct grams per order, slots,
               device bytes, bytes_per_training_token
  score        per training size: the per-document arrays over the whole corpus: ms, the overlap query's ms beside it and
               ratio_to_overlap; probes_per_position = 1 + the mean j below the order (from the order histogram: a position probes
               orders 1 .. min(j + 1, K)), tokens_per_s
  kneser_ney   per training size: kn_prepare_ms (the two derivation passes over a fresh model's table, with their clears and the read-back)
               and its ratio to the build; score_kn_ms over the whole corpus and its ratio to the Stupid Backoff score of the same round;
               the sidecar's bytes and bytes a training token; the discounts and which orders fell back.  tests/kn_oracle.py over the
               first --oracle-rows / 8 documents against the smallest model: counts of counts and n_order equal, bits_fx within n_tokens
  oracle       tests/lm_oracle.py over the first --oracle-rows documents against the smallest model: n_tokens and n_order equal,
               bits_fx within n_tokens (the bound of tests/test_gpu_lm.py); asserted
One JSON line on stdout.

On a shared GPU every step gets a time limit of its own and the steps are chained, so that nothing starts behind a step that failed:
    timeout -k 10 900 python tools/lm_bench.py --out profiles/lm_bench.json"""
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
    ap.add_argument("--train", default="10000,100000")
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    import kn_oracle as KO
    import lm_oracle as LO
    from genz_tokenize import Tokenize, _native
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n, N = len(offs) - 1, args.order
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
    body = np.maximum(row_off[1:] - row_off[:-1] - 2, 0)
    tokens = int(body.sum())
    d_out = ctx.alloc(8 * n + 4 * n + 4 * (N + 1) * n + 64)              # bits_fx, n_tokens, n_order
    d_bits, d_ntok, d_order = d_out, d_out + 8 * n, d_out + 12 * n
    d_kn = ctx.alloc(8 * n + 4 * n + 4 * (N + 1) * n + 64)               # the same three arrays for the Kneser-Ney calls
    d_ng = ctx.alloc(4 * 5 * n + 64)
    ng_outs = [d_ng + 4 * n * k for k in range(5)]
    rows = []
    first_model = None
    for R in [min(int(x), n) for x in args.train.split(",")]:
        held = {}

        def build(combine):
            if "lm" in held:
                ctx.ngram_lm_destroy(held.pop("lm"))
            _native.debug_set("lm_combine", combine, ctx)
            held["lm"] = ctx.ngram_lm_build_device(d_ids, d_ro, R, 1, 1, N)

        def build_index():
            if "ix" in held:
                ctx.ngram_index_destroy(held.pop("ix"))
            held["ix"] = ctx.ngram_index_build_device(d_ids, d_ro, R, 1, 1, N)

        def score():
            ctx.ngram_lm_score_device(held["lm"], d_ids, d_ro, n, 1, 1, 0.4, d_ntok, d_bits, d_order, 0, 0, 0)

        def overlap():
            ctx.ngram_overlap_device(held["ix"], d_ids, d_ro, n, 1, 1, *ng_outs, 0)

        def kn_prepare():                                               # (a model is derived once: a fresh one each time, its build not timed)
            build(1)
            return timed(lambda: ctx.ngram_lm_kn_prepare(held["lm"]))

        def score_kn():
            ctx.ngram_lm_score_kn_device(held["lm"], d_ids, d_ro, n, 1, 1, None, d_kn + 8 * n, d_kn, d_kn + 12 * n, 0, 0)
        build(1); build(0); build_index(); score(); overlap(); kn_prepare(); score_kn()
        t = {k: [] for k in ("plain", "combined", "index", "score", "overlap", "kn_prepare", "score_kn")}
        for _ in range(args.reps):
            t["combined"].append(timed(lambda: build(1)))
            t["plain"].append(timed(lambda: build(0)))
            t["index"].append(timed(build_index))
            t["score"].append(timed(score))
            t["overlap"].append(timed(overlap))
            t["kn_prepare"].append(kn_prepare())
            t["score_kn"].append(timed(score_kn))
        _native.debug_set("lm_combine", 1, ctx)
        med = {k: float(np.median(v)) for k, v in t.items()}
        info = ctx.ngram_lm_info(held["lm"])
        order = np.empty((N + 1, n), dtype=np.int32)
        ctx.d2h(order, d_order)
        hist = order.sum(axis=1, dtype=np.int64)
        # a position walks orders 1 .. j and one more unless j == K: at most j + 1 probes, fewer by one at j == K (counted from the host's body lengths)
        full = int(np.minimum(body, N - 1).sum())                       # positions with K < N all have K = i + 1: j == K is possible there as well
        probes = float((hist * np.minimum(np.arange(N + 1) + 1, N)).sum()) / max(tokens, 1)
        rec = {"train_docs": int(R), "order": N, "train_tokens": info["n_tokens"], "n_grams": list(info["n_grams"]), "n_distinct": list(info["n_distinct"]),
               "slots": info["slots"], "device_bytes": info["device_bytes"], "bytes_per_training_token": round(info["device_bytes"] / max(info["n_tokens"], 1), 2),
               "build_ms": round(med["plain"], 3), "build_combined_ms": round(med["combined"], 3), "index_build_ms": round(med["index"], 3),
               "build_ratio_to_index": round(med["plain"] / med["index"], 3), "score_ms": round(med["score"], 3), "overlap_ms": round(med["overlap"], 3),
               "score_ratio_to_overlap": round(med["score"] / med["overlap"], 3), "order_histogram": hist.tolist(),
               "probes_per_position_at_most": round(probes, 3), "positions_below_full_context": full, "tokens_per_s": round(tokens / med["score"] * 1e3, 0),
               "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()}}
        kn = ctx.ngram_lm_kn_info(held["lm"])
        rec.update({"kn_prepare_ms": round(med["kn_prepare"], 3), "kn_prepare_ratio_to_build": round(med["kn_prepare"] / med["combined"], 3),
                    "score_kn_ms": round(med["score_kn"], 3), "score_kn_ratio_to_score": round(med["score_kn"] / med["score"], 3),
                    "kn_sidecar_bytes": kn["sidecar_bytes"], "kn_sidecar_bytes_per_training_token": round(kn["sidecar_bytes"] / max(info["n_tokens"], 1), 2),
                    "kn_discounts": [[round(x, 6) for x in row] for row in kn["discounts"].tolist()], "kn_fallback": kn["fallback"].tolist(),
                    "kn_counts_of_counts": kn["counts_of_counts"].tolist()})
        rows.append(rec)
        print("# train %d docs: build %.3f ms (combined %.3f), index %.3f ms; score %.3f ms, overlap %.3f ms; <= %.2f probes/position; %.1f bytes/token" %
              (R, med["plain"], med["combined"], med["index"], med["score"], med["overlap"], probes, rec["bytes_per_training_token"]), file=sys.stderr, flush=True)
        print("# Kneser-Ney: prepare %.3f ms, score %.3f ms; sidecar %.1f bytes/token; fallback %s" %
              (med["kn_prepare"], med["score_kn"], rec["kn_sidecar_bytes_per_training_token"], rec["kn_fallback"]), file=sys.stderr, flush=True)
        if first_model is None:
            first_model = R
            k = min(args.oracle_rows, n)
            got_tok, got_bits = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.uint64)
            ctx.d2h(got_tok, d_ntok); ctx.d2h(got_bits, d_bits)
            ids = np.empty(int(row_off[max(R, k)]), dtype=np.int32)
            ctx.d2h(ids, d_ids)
            docs = [ids[row_off[r]:row_off[r + 1]].tolist() for r in range(max(R, k))]
            t0 = time.perf_counter()
            model = LO.train(docs[:R], N, framed=True)
            train_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            want = LO.score(model, N, docs[:k], 0.4, framed=True)
            score_ms = (time.perf_counter() - t0) * 1e3
            diff = np.abs(got_bits[:k].astype(np.int64) - want["bits_fx"].astype(np.int64))
            checked = bool(np.array_equal(got_tok[:k], want["n_tokens"]) and np.array_equal(order[:, :k], want["n_order"]) and (diff <= want["n_tokens"]).all()
                           and (info["n_grams"], info["n_distinct"]) == LO.grams(model, N))
            assert checked, "the device's outputs differ from the host rule on the first %d documents" % k
            head = int(want["n_tokens"].sum())
            oracle_rec = {"oracle_rows": int(k), "train_docs": int(R), "oracle_train_ms": round(train_ms, 1), "oracle_score_ms": round(score_ms, 1),
                          "oracle_ns_per_token": round(score_ms * 1e6 / max(head, 1), 1), "device_ns_per_token": round(med["score"] * 1e6 / max(tokens, 1), 4),
                          "bits_fx_max_diff": int(diff.max()), "checked": checked}
            print("# oracle: train %.0f ms, score %.1f ns/token; device %.4f ns/token; checked %s" %
                  (train_ms, oracle_rec["oracle_ns_per_token"], oracle_rec["device_ns_per_token"], checked), file=sys.stderr, flush=True)
            kk = max(k // 8, 1)
            kn_bits = np.empty(n, dtype=np.uint64)
            kn_order = np.empty((N + 1, n), dtype=np.int32)
            ctx.d2h(kn_bits, d_kn); ctx.d2h(kn_order, d_kn + 12 * n)
            t0 = time.perf_counter()
            derived = KO.derive(model, N)
            kn_want = KO.score(derived, N, docs[:kk], framed=True)
            kn_ms = (time.perf_counter() - t0) * 1e3
            kn_diff = np.abs(kn_bits[:kk].astype(np.int64) - kn_want["bits_fx"].astype(np.int64))
            kn_checked = bool(np.array_equal(kn_order[:, :kk], kn_want["n_order"]) and (kn_diff <= kn_want["n_tokens"]).all()
                              and np.array_equal(kn["counts_of_counts"], derived["n"]) and kn["V"] == derived["V"])
            assert kn_checked, "the device's Kneser-Ney outputs differ from the host rule on the first %d documents" % kk
            oracle_rec.update({"kn_oracle_rows": int(kk), "kn_oracle_ms": round(kn_ms, 1), "kn_bits_fx_max_diff": int(kn_diff.max()), "kn_checked": kn_checked})
        ctx.ngram_lm_destroy(held.pop("lm"))
        ctx.ngram_index_destroy(held.pop("ix"))
    for d in (d_t, d_to, d_ids, d_am, d_ro, d_out, d_kn, d_ng):
        ctx.free(d)
    rec = {"bench": "lm", "docs": n, "tokens": tokens, "reps": args.reps, "piece": 4096, "alpha": 0.4, "models": rows, "oracle": oracle_rec}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
