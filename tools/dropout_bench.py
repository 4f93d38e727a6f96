"""BPE-dropout encoding (gz_encode_dropout_device, csrc/gz_dropout.inc) over the configs[2] corpus resident in HBM, beside the plain
call that sends the same words through the merge loop without the draws.

    python tools/dropout_bench.py [--docs 1000000] [--reps 5] [--sample 20000] [--out profiles/dropout_bench.json]

The corpus (corpus.config_corpus(3, n_docs=--docs)) is copied to the device once; every call writes dense [N, 256] input_ids and
attention_mask into the same two device arrays.  Host clock around call + gz_sync, after a warm-up call of each, --reps rounds that
run the four calls one after the other (interleaved), medians:
  merge_loop_only_ms   gz_encode_batch_device under GZ_NO_WORD_TABLE: every word through gz_miss2_kernel, no draws -- the yardstick,
                       unchanged by this feature
  dropout_ms[p]        gz_encode_dropout_device at p = 0, 0.1 and 0.5 (p = 0 computes what the yardstick computes)
  ratio[p]             dropout_ms[p] / merge_loop_only_ms; no bar is set -- above 2 at p = 0.1 the time goes somewhere worth a sentence
  checked_p0           the rows of p = 0 equal the yardstick's, array for array
  tokens_per_word[p]   pieces / words over the first --sample documents (a ragged host call; words = whitespace-separated runs)
One JSON line on stdout.

On a shared GPU the step gets a time limit of its own:
    timeout -k 10 600 python tools/dropout_bench.py --out profiles/dropout_bench.json"""
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

SEED, L, PS = 20240607, 256, (0.0, 0.1, 0.5)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=20_000)
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
    d_t, d_to = ctx.alloc(text.nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_to, offs)
    cells = n * L
    d_ids, d_am, d_nr = ctx.alloc(4 * cells + 64), ctx.alloc(4 * cells + 64), ctx.alloc(4 * n + 64)
    flags = _native.GZ_PADDING | _native.GZ_TRUNCATION

    def plain():
        ctx.encode_device(d_t, d_to, 0, 0, n, L, flags | _native.GZ_NO_WORD_TABLE, cells, d_ids, d_am, d_n_real=d_nr, h_text_off=offs)
        ctx.sync()

    def drop(p):
        ctx.encode_dropout_device(d_t, d_to, n, L, flags, cells, int(p * 2 ** 32), SEED, 0, d_ids, d_am, None, d_nr)
        ctx.sync()
    k = min(n, 4096)
    head = {}
    for name, fn in (("plain", plain), ("p0", lambda: drop(0.0))):   # warm-up of both, and the rows of p = 0 against the yardstick's
        fn()
        head[name] = (np.empty((k, L), np.int32), np.empty((k, L), np.int32), np.empty(k, np.int32))
        for a, d in zip(head[name], (d_ids, d_am, d_nr)):
            ctx.d2h(a, d)
    checked = all(bool(np.array_equal(a, b)) for a, b in zip(head["plain"], head["p0"]))
    for p in PS[1:]:
        drop(p)
    t_plain, t_drop = [], {p: [] for p in PS}
    for _ in range(args.reps):                                       # interleaved: every round runs the yardstick and the three p
        t_plain.append(timed(plain))
        for p in PS:
            t_drop[p].append(timed(lambda: drop(p)))
    base = float(np.median(t_plain))
    rec = {"bench": "dropout", "docs": n, "max_len": L, "seed": SEED, "reps": args.reps, "text_mb": round(text.nbytes / 1e6, 1),
           "merge_loop_only_ms": round(base, 3), "merge_loop_only_all_ms": [round(t, 3) for t in t_plain], "checked_p0": checked,
           "dropout_ms": {}, "dropout_all_ms": {}, "ratio": {}, "tokens_per_word": {}}
    for p in PS:
        ms = float(np.median(t_drop[p]))
        rec["dropout_ms"][str(p)] = round(ms, 3)
        rec["dropout_all_ms"][str(p)] = [round(t, 3) for t in t_drop[p]]
        rec["ratio"][str(p)] = round(ms / base, 3)
    # pieces per word over the first documents (ragged host call)
    m = min(n, args.sample)
    sub, sub_off = text[int(offs[0]):int(offs[m])], offs[:m + 1] - offs[0]
    words = len(sub.tobytes().split())
    rec["sample_docs"], rec["sample_words"] = m, words
    for p in PS:
        r = tok.encode_dropout_packed(sub, sub_off, p=p, seed=SEED, max_len=None)
        rec["tokens_per_word"][str(p)] = round((int(r["row_off"][-1]) - 2 * m) / max(words, 1), 4)
    for d in (d_t, d_to, d_ids, d_am, d_nr):
        ctx.free(d)
    print("# %d docs: merge loop only %.3f ms; dropout %s; ratio %s; tokens/word %s; p = 0 checked %s" %
          (n, base, rec["dropout_ms"], rec["ratio"], rec["tokens_per_word"], checked), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if checked else 1


if __name__ == "__main__":
    sys.exit(main())
