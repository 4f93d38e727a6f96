"""MinHash signatures (gz_minhash_rows_device, csrc/gz_minhash.inc) and near-duplicate groups (gz_minhash_groups_device) over the
configs[2] corpus with its token rows resident in HBM, beside the encode launch of the same documents, and the numpy restatement
of the rule on the host.

    python tools/minhash_bench.py [--docs 1000000] [--reps 7] [--runs 2] [--oracle-rows 4096] [--out profiles/minhash_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit and stays there.  Host clock
around call + gz_sync, after a warm-up call of each, --reps rounds that run the encode launch and the signature pass one after the
other (interleaved), medians; --runs such series, each reported.
  signatures   per (num_perm, shingle) = (128, 5), (64, 5), (256, 5), (128, 1), over the corpus and over the corpus with one document
               of 1 M tokens appended:  ms, shingles, evals_per_s = shingles * num_perm / time (hash evaluations g_k(H) a second),
               encode_ms (the yardstick, unchanged by this feature) and ratio = ms / encode_ms
  groups       per bands = 16, 32 at threshold 0.7 over the (128, 5) signatures of the corpus as it is and of the corpus with 10 % of
               its documents replaced by one-substitution copies of others:  ms, n_groups, passes (the labels are a forest that ONE
               pointer-jumping pass flattens once the bands are linked: there is no iteration to a fixed point to count)
  oracle       tests/minhash_oracle.py over the first --oracle-rows documents: oracle_ns_per_token, the device's beside it, and
               checked = the device's signatures and shingle counts equal the oracle's on those rows
One JSON line on stdout.

On a shared GPU every step gets a time limit of its own and the steps are chained, so that nothing starts behind a step that failed:
    timeout -k 10 900 python tools/minhash_bench.py --out profiles/minhash_bench.json"""
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
SHAPES = ((128, 5), (64, 5), (256, 5), (128, 1))
LONG_TOKENS = 1_000_000


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def with_copies(ids, row_off, share, lo, hi, rng):
    """The ragged rows with `share` of the documents replaced by copies of other documents, one body token of each copy substituted
    by a random id in [lo, hi).  Rows are framed: the first and last entry of a row are left alone.  -> (ids, row_off, n_copies)"""
    n = len(row_off) - 1
    src = np.arange(n, dtype=np.int64)
    targets = rng.choice(n, size=int(n * share), replace=False)
    keep = np.ones(n, dtype=bool)
    keep[targets] = False
    sources = np.flatnonzero(keep)
    src[targets] = sources[rng.integers(0, len(sources), size=len(targets))]
    lens = (row_off[1:] - row_off[:-1])[src]
    new_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=new_off[1:])
    gather = np.repeat(row_off[:-1][src] - new_off[:-1], lens) + np.arange(new_off[n], dtype=np.int64)
    out = ids[gather]
    body = lens[targets] - 2
    ok = body > 0
    at = new_off[:-1][targets][ok] + 1 + (rng.integers(0, 2 ** 31, size=int(ok.sum())) % body[ok])
    out[at] = rng.integers(lo, hi, size=len(at)).astype(np.int32)
    return out, new_off, int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--oracle-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    import minhash_oracle as MO
    from genz_tokenize import Tokenize, _native
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n = len(offs) - 1
    tok = Tokenize()
    tok._sync_tables()
    ctx = tok._ctx
    rng = np.random.default_rng(SEED)
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
    # the corpus with one long document appended, and the corpus with copies, beside it in HBM
    long_doc = np.concatenate([ids[:1], rng.integers(5, tok.vocab_size(), size=LONG_TOKENS).astype(np.int32), ids[total - 1:total]])
    ids_long = np.concatenate([ids, long_doc])
    ro_long = np.concatenate([row_off, [total + len(long_doc)]]).astype(np.int64)
    ids_dup, ro_dup, n_copies = with_copies(ids, row_off, 0.10, 5, tok.vocab_size(), rng)
    d_ids_long, d_ro_long = ctx.alloc(ids_long.nbytes + 64), ctx.alloc(ro_long.nbytes)
    ctx.h2d(d_ids_long, ids_long); ctx.h2d(d_ro_long, ro_long)
    d_ids_dup, d_ro_dup = ctx.alloc(ids_dup.nbytes + 64), ctx.alloc(ro_dup.nbytes)
    ctx.h2d(d_ids_dup, ids_dup); ctx.h2d(d_ro_dup, ro_dup)
    d_sig, d_cnt = ctx.alloc(4 * 256 * (n + 1)), ctx.alloc(4 * (n + 1))

    def shingles_of(ro, w):
        body = np.maximum(ro[1:] - ro[:-1] - 2, 0)
        return int(np.where(body >= w, body - w + 1, np.minimum(body, 1)).sum())

    sig_rows = []
    for name, di, dr, nn, ro in (("corpus", d_ids, d_ro, n, row_off), ("corpus + one document of 1 M tokens", d_ids_long, d_ro_long, n + 1, ro_long)):
        for K, w in SHAPES:
            def sign():
                ctx.minhash_rows_device(di, dr, nn, 1, 1, w, K, SEED, d_sig, d_cnt)
                ctx.sync()
            sign(); encode()
            series = []
            for _ in range(args.runs):
                t_sig, t_enc = [], []
                for _ in range(args.reps):
                    t_enc.append(timed(encode))
                    t_sig.append(timed(sign))
                series.append((float(np.median(t_sig)), float(np.median(t_enc)), t_sig, t_enc))
            sh = shingles_of(ro, w)
            ms, enc_ms = series[0][0], series[0][1]
            rec = {"rows": name, "docs": int(nn), "tokens": int(ro[-1] - 2 * nn), "num_perm": K, "shingle": w, "shingles": sh,
                   "ms": round(ms, 3), "ms_runs": [round(s[0], 3) for s in series], "all_ms": [[round(t, 3) for t in s[2]] for s in series],
                   "encode_ms": round(enc_ms, 3), "encode_ms_runs": [round(s[1], 3) for s in series],
                   "evals_per_s": round(sh * K / ms * 1e3, 0), "ratio_to_encode": round(ms / enc_ms, 3)}
            sig_rows.append(rec)
            print("# signatures %s K=%d w=%d: %.3f ms (runs %s)  %.3e evals/s  encode %.3f ms  ratio %.3f" %
                  (name, K, w, ms, rec["ms_runs"], rec["evals_per_s"], enc_ms, rec["ratio_to_encode"]), file=sys.stderr, flush=True)

    # the oracle on the host over the first documents, and the device's output against it
    k = min(args.oracle_rows, n)
    ctx.minhash_rows_device(d_ids, d_ro, n, 1, 1, 5, 128, SEED, d_sig, d_cnt)
    ctx.sync()
    got_sig, got_cnt = np.empty((k, 128), dtype=np.uint32), np.empty(k, dtype=np.int32)
    ctx.d2h(got_sig, d_sig); ctx.d2h(got_cnt, d_cnt)
    head = [ids[row_off[r]:row_off[r + 1]] for r in range(k)]
    res = {}

    def oracle():
        res["r"] = MO.batch(head, 128, 5, SEED, framed=True)
    orc_ms = min(timed(oracle), timed(oracle))
    checked = bool(np.array_equal(got_sig, res["r"]["signatures"]) and np.array_equal(got_cnt, res["r"]["n_shingles"]))
    head_tokens = int(row_off[k] - row_off[0]) - 2 * k
    dev = next(r for r in sig_rows if r["rows"] == "corpus" and (r["num_perm"], r["shingle"]) == (128, 5))
    oracle_rec = {"oracle_rows": int(k), "oracle_tokens": head_tokens, "oracle_ms": round(orc_ms, 1),
                  "oracle_ns_per_token": round(orc_ms * 1e6 / max(head_tokens, 1), 1),
                  "device_ns_per_token": round(dev["ms"] * 1e6 / max(dev["tokens"], 1), 4), "checked": checked}
    print("# oracle %.1f ns/token, device %.4f ns/token, checked %s" % (oracle_rec["oracle_ns_per_token"], oracle_rec["device_ns_per_token"], checked),
          file=sys.stderr, flush=True)

    # groups over the (128, 5) signatures of the corpus as it is and with copies
    d_group = ctx.alloc(4 * n)
    group_rows = []
    for name, di, dr in (("corpus", d_ids, d_ro), ("corpus with 10 % one-substitution copies", d_ids_dup, d_ro_dup)):
        ctx.minhash_rows_device(di, dr, n, 1, 1, 5, 128, SEED, d_sig, 0)
        ctx.sync()
        for B in (16, 32):
            out = {}

            def groups():
                out["n"] = ctx.minhash_groups_device(d_sig, n, 128, B, 90, d_group)
                ctx.sync()
            groups()
            series = []
            for _ in range(args.runs):
                ts = [timed(groups) for _ in range(args.reps)]
                series.append((float(np.median(ts)), ts))
            rec = {"rows": name, "docs": int(n), "copies": n_copies if di == d_ids_dup else 0, "num_perm": 128, "bands": B, "threshold": 0.7,
                   "min_agree": 90, "ms": round(series[0][0], 3), "ms_runs": [round(s[0], 3) for s in series],
                   "all_ms": [[round(t, 3) for t in s[1]] for s in series], "n_groups": int(out["n"]), "passes": 1}
            group_rows.append(rec)
            print("# groups %s B=%d: %.3f ms (runs %s)  n_groups %d" % (name, B, rec["ms"], rec["ms_runs"], rec["n_groups"]), file=sys.stderr, flush=True)
    for d in (d_t, d_to, d_ids, d_am, d_ro, d_ids_long, d_ro_long, d_ids_dup, d_ro_dup, d_sig, d_cnt, d_group):
        ctx.free(d)
    rec = {"bench": "minhash", "docs": n, "seed": SEED, "reps": args.reps, "runs": args.runs, "piece": 4096, "signatures": sig_rows,
           "groups": group_rows, "oracle": oracle_rec}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if checked else 1


if __name__ == "__main__":
    sys.exit(main())
