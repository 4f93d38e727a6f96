"""Exact duplicate substrings across documents (gz_substr_dups_device, gz_cut_rows_device; csrc/gz_substr.inc) over the configs[2]
corpus with its token rows resident in HBM: the mark call at n = 50 and at n = 13, the cut of the dup bytes, and -- alternating with
them in the same visit -- the nearest existing route with the same table traffic: the n = 13 index build over the same rows plus the
overlap query of the rows against themselves.  Then the dict-of-tuples rule on the host over the first documents.

    python tools/substr_bench.py [--docs 1000000] [--reps 5] [--runs 2] [--oracle-rows 4096] [--out profiles/substr_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is encoded once on the device without a length limit and stays there.  Host clock
around each call (the device forms return when their outputs are complete), after a warm-up call of each; --reps rounds that run the
four routes one after the other (interleaved), medians; --runs such series, each reported.
  dups_n50 / dups_n13   the five per-document arrays and the dup bytes: ms, positions, ns_per_token
  cut                   gz_cut_rows_device with drop = the dup bytes of n = 50: ms, ids kept
  index_overlap_n13     gz_ngram_index_build_device + gz_ngram_overlap_device (five arrays + covered bytes) of the rows against
                        themselves, index destroyed each round: ms; ratio = dups_n13 ms / this
  with_copies           the corpus holds no repeated 13-gram, so the rows above time the all-distinct case; here every tenth document
                        is replaced by a copy of the one before it: dups at n = 50 and the cut again, and the dup tokens and kept
                        ids checked against what was planted
  oracle                the rule over the first --oracle-rows documents ALONE (a shard is deduplicated against itself), at n = 50 and
                        n = 13: checked = all five arrays and the dup bytes of a device call over those rows equal it
One JSON line on stdout.

On a shared GPU every step gets a time limit of its own and the steps are chained, so that nothing starts behind a step that failed:
    timeout -k 10 900 python tools/substr_bench.py --out profiles/substr_bench.json"""
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

OUT = ("n_grams", "n_later", "n_dup", "first_dup", "first_src")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def host_rule(rows, n):
    """the rule over framed rows: a dict from n-gram to its first position, then the definitions"""
    first, out, dup = {}, {k: [] for k in OUT}, []
    for r, row in enumerate(rows):
        body = row[1:len(row) - 1] if len(row) > 2 else row[:0]
        d, lat = np.zeros(len(row), dtype=np.uint8), []
        for i in range(max(0, len(body) - n + 1)):
            if first.setdefault(body[i:i + n].tobytes(), (r, i)) != (r, i):
                lat.append(i)
                d[1 + i:1 + i + n] = 1
        vals = (max(0, len(body) - n + 1), len(lat), int(d.sum()), lat[0] if lat else -1, first[body[lat[0]:lat[0] + n].tobytes()][0] if lat else -1)
        for k, v in zip(OUT, vals):
            out[k].append(v)
        dup.append(d)
    return {k: np.array(v, dtype=np.int32) for k, v in out.items()}, np.concatenate(dup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--oracle-rows", type=int, default=4096)
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
    cap = int(offs[n] - offs[0]) + 2 * n
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    d_ids, d_am, d_ro = ctx.alloc(4 * cap + 64), ctx.alloc(4 * cap + 64), ctx.alloc(8 * (n + 1))
    ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE, cap, d_ids, d_am, d_row_off=d_ro)
    ctx.sync()
    row_off = np.empty(n + 1, dtype=np.int64)
    ctx.d2h(row_off, d_ro)
    total = int(row_off[n])
    body = np.maximum(np.diff(row_off) - 2, 0)
    tokens = int(body.sum())
    d_out, d_dup = ctx.alloc(4 * len(OUT) * n + 64), ctx.alloc(total + 64)
    d_cut, d_cro, d_kept = ctx.alloc(4 * total + 64), ctx.alloc(8 * (n + 1)), ctx.alloc(4 * n + 64)
    outs = [d_out + 4 * n * k for k in range(len(OUT))]

    def dups(w, rows=n):
        ctx.substr_dups_device(d_ids, d_ro, rows, 1, 1, w, *outs, d_dup)

    def cut():
        ctx.cut_rows_device(d_ids, d_ro, n, d_dup, d_cut, d_cro, d_kept)

    def index_overlap():
        h = ctx.ngram_index_build_device(d_ids, d_ro, n, 1, 1, 13)
        try:
            ctx.ngram_overlap_device(h, d_ids, d_ro, n, 1, 1, *outs, d_dup)
        finally:
            ctx.ngram_index_destroy(h)
    routes = {"dups_n13": lambda: dups(13), "index_overlap_n13": index_overlap, "dups_n50": lambda: dups(50), "cut": cut}
    for f in routes.values():
        f()
    series = []
    for _ in range(args.runs):
        ts = {k: [] for k in routes}
        for _ in range(args.reps):
            for k, f in routes.items():                                 # (the cut comes behind dups_n50: its drop bytes are that call's)
                ts[k].append(timed(f))
        series.append(ts)
    rec = {"bench": "substr", "docs": int(n), "tokens": tokens, "ids": total, "reps": args.reps, "runs": args.runs, "piece": 4096}
    for k in routes:
        med = [float(np.median(s[k])) for s in series]
        rec[k] = {"ms": round(med[0], 3), "ms_runs": [round(m, 3) for m in med], "all_ms": [[round(t, 3) for t in s[k]] for s in series],
                  "ns_per_token": round(med[0] * 1e6 / max(tokens, 1), 4)}
    for w in (13, 50):
        rec["dups_n%d" % w]["positions"] = int(np.maximum(body - w + 1, 0).sum())
    rec["dups_n13"]["ratio_to_index_overlap"] = round(rec["dups_n13"]["ms"] / rec["index_overlap_n13"]["ms"], 3)
    kept_off = np.empty(n + 1, dtype=np.int64)
    ctx.d2h(kept_off, d_cro)
    got = np.empty((len(OUT), n), dtype=np.int32)
    ctx.d2h(got, d_out)
    rec["cut"]["ids_kept"] = int(kept_off[n])
    rec["dups_n50"].update(documents_with_dups=int((got[1] > 0).sum()), tokens_dup=int(got[2].sum()))
    print("# dups n=50 %.3f ms, n=13 %.3f ms, cut %.3f ms, index + overlap n=13 %.3f ms (ratio %.3f); %d of %d tokens dup at n=50" %
          (rec["dups_n50"]["ms"], rec["dups_n13"]["ms"], rec["cut"]["ms"], rec["index_overlap_n13"]["ms"], rec["dups_n13"]["ratio_to_index_overlap"],
           rec["dups_n50"]["tokens_dup"], tokens), file=sys.stderr, flush=True)

    dups(13)
    ctx.d2h(got, d_out)
    rec["dups_n13"].update(documents_with_dups=int((got[1] > 0).sum()), tokens_dup=int(got[2].sum()))

    # the same calls where there IS something to find: every tenth document replaced by a copy of the one before it
    ids = np.empty(total, dtype=np.int32)
    ctx.d2h(ids, d_ids)
    src = np.arange(n, dtype=np.int64)
    src[9::10] -= 1
    lens = (row_off[1:] - row_off[:-1])[src]
    c_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=c_off[1:])
    c_ids = ids[np.repeat(row_off[src] - c_off[:-1], lens) + np.arange(c_off[n], dtype=np.int64)]
    d_cids, d_cro2 = ctx.alloc(c_ids.nbytes + 64), ctx.alloc(c_off.nbytes)
    ctx.h2d(d_cids, c_ids); ctx.h2d(d_cro2, c_off)

    def dups_copies():
        ctx.substr_dups_device(d_cids, d_cro2, n, 1, 1, 50, *outs, d_dup)

    def cut_copies():
        ctx.cut_rows_device(d_cids, d_cro2, n, d_dup, d_cut, d_cro, d_kept)
    dups_copies(); cut_copies()
    t_d, t_c = [], []
    for _ in range(args.reps):
        t_d.append(timed(dups_copies)); t_c.append(timed(cut_copies))
    ctx.d2h(got, d_out)
    ctx.d2h(kept_off, d_cro)
    c_body = np.maximum(lens - 2, 0)
    copied = np.zeros(n, dtype=bool)
    copied[9::10] = True
    want_dup = int(c_body[copied & (c_body >= 50)].sum()) + rec["dups_n50"]["tokens_dup"]       # (a copy is dup in full; nothing else repeats)
    assert int(got[2].sum()) == want_dup and int(kept_off[n]) == int(c_off[n]) - want_dup, (int(got[2].sum()), want_dup, int(kept_off[n]))
    rec["with_copies"] = {"copied_documents": int(copied.sum()), "ids": int(c_off[n]), "dups_n50_ms": round(float(np.median(t_d)), 3),
                          "cut_ms": round(float(np.median(t_c)), 3), "all_ms": [[round(t, 3) for t in t_d], [round(t, 3) for t in t_c]],
                          "tokens_dup": int(got[2].sum()), "documents_with_dups": int((got[1] > 0).sum()), "ids_kept": int(kept_off[n]), "checked": True}
    print("# every tenth document a copy: dups n=50 %.3f ms, cut %.3f ms, %d tokens dup (as planted), %d ids kept" %
          (rec["with_copies"]["dups_n50_ms"], rec["with_copies"]["cut_ms"], rec["with_copies"]["tokens_dup"], rec["with_copies"]["ids_kept"]),
          file=sys.stderr, flush=True)
    ctx.free(d_cids); ctx.free(d_cro2)

    # the rule on the host over the first documents alone, and a device call over those rows against it, at both widths
    k = min(args.oracle_rows, n)
    head_ids = np.empty(int(row_off[k]), dtype=np.int32)
    ctx.d2h(head_ids, d_ids)
    head = [head_ids[row_off[r]:row_off[r + 1]] for r in range(k)]
    head_tokens = int(body[:k].sum())
    rec["oracle"] = {"oracle_rows": int(k), "oracle_tokens": head_tokens}
    got_dup = np.empty(int(row_off[k]), dtype=np.uint8)
    for w in (50, 13):
        res = {}
        orc_ms = timed(lambda: res.update(r=host_rule(head, w)))
        dups(w, k)
        ctx.d2h(got, d_out)
        ctx.d2h(got_dup, d_dup)
        want, want_dup = res["r"]
        checked = bool(all(np.array_equal(got[i][:k], want[key]) for i, key in enumerate(OUT)) and np.array_equal(got_dup, want_dup))
        assert checked, "the device's outputs differ from the host rule on the first %d documents at n = %d" % (k, w)
        rec["oracle"]["n%d" % w] = {"oracle_ms": round(orc_ms, 1), "oracle_ns_per_token": round(orc_ms * 1e6 / max(head_tokens, 1), 1),
                                    "tokens_dup": int(want["n_dup"].sum()), "checked": checked}
        print("# oracle n=%d: %.1f ns/token, %d tokens dup, checked %s" % (w, rec["oracle"]["n%d" % w]["oracle_ns_per_token"], int(want["n_dup"].sum()), checked),
              file=sys.stderr, flush=True)
    for d in (d_t, d_to, d_ids, d_am, d_ro, d_out, d_dup, d_cut, d_cro, d_kept):
        ctx.free(d)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
