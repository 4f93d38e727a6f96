"""What the BPE learner costs on the configs[2]-style corpus, text and offsets resident in HBM.  Numbers to write down, no bar.

    python tools/learn_bench.py [--docs 1000000] [--reps 3] [--merges 8000,50000] [--oracle-docs 10000] [--oracle-merges 2000]
                                [--out profiles/learn_bench.json]

  word_counts_device_ms   gz_wordset_build_device over the corpus (the call returns the distinct words and counts on the host)
  bm25_build_device_ms    gz_bm25_build_device over the same buffers, alternating with it in the same visit: the word front the two
                          share, plus the index the word set does not make
  learn_<M>               gz_bpe_learn + gz_bpe_learn_result on that word set for M merges, min_frequency 2: ms, merges done, us per
                          merge, symbols, and the pair table's slots, keys, fill and growths
  oracle_*                tests/learn_oracle.py (learn_indexed, plain Python) on the first --oracle-docs documents for --oracle-merges
                          merges against the device on the same documents: both times, and whether the two files are equal
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "genz-tokenize_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import corpus  # noqa: E402
import learn_oracle as LO  # noqa: E402
from genz_tokenize import _native, learn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--merges", default="8000,50000")
    ap.add_argument("--oracle-docs", type=int, default=10_000)
    ap.add_argument("--oracle-merges", type=int, default=2_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    ctx = _native.Context()
    t, o, _ = corpus.config_corpus(2, n_docs=a.docs)
    n, nbytes = a.docs, int(o[-1])
    res = dict(docs=n, text_bytes=nbytes)
    d_text, d_off = ctx.alloc(nbytes), ctx.alloc(8 * (n + 1))
    ctx.h2d(d_text, t)
    ctx.h2d(d_off, o)

    wc, bm = [], []
    ws = 0
    for k in range(a.reps + 1):                                      # (the first round is the warm-up)
        t0 = time.perf_counter()
        ix = ctx.bm25_build_device(d_text, d_off, n, nbytes)
        bm.append((time.perf_counter() - t0) * 1e3)
        res["bm25_terms"], res["bm25_words"] = ctx.bm25_info(ix)[1:]
        ctx.bm25_destroy(ix)
        if ws:
            ctx.wordset_destroy(ws)
        t0 = time.perf_counter()
        ws = ctx.wordset_build_device(d_text, d_off, n, nbytes)
        wc.append((time.perf_counter() - t0) * 1e3)
    res["word_counts_device_ms"], res["word_counts_device_all_ms"] = float(np.median(wc[1:])), [round(x, 3) for x in wc[1:]]
    res["bm25_build_device_ms"], res["bm25_build_device_all_ms"] = float(np.median(bm[1:])), [round(x, 3) for x in bm[1:]]
    res["distinct_words"], res["word_bytes"], res["total_words"] = ctx.wordset_info(ws)
    assert res["distinct_words"] == res["bm25_terms"] and res["total_words"] == res["bm25_words"]

    for m in [int(x) for x in a.merges.split(",") if x]:
        t0 = time.perf_counter()
        info = ctx.bpe_learn(ws, m, 2)[0]
        ms = (time.perf_counter() - t0) * 1e3
        done = int(info[0])
        res["learn_%d" % m] = dict(ms=round(ms, 3), merges_done=done, us_per_merge=round(ms * 1e3 / max(done, 1), 3), symbols=int(info[1]),
                                   table_slots=int(info[5]), table_keys=int(info[6]), table_fill=round(int(info[6]) / int(info[5]), 4),
                                   table_growths=int(info[7]))
    ctx.wordset_destroy(ws)

    if a.oracle_docs > 0:
        k = min(a.oracle_docs, n)
        sub_off = np.ascontiguousarray(o[:k + 1])
        t0 = time.perf_counter()
        dev = learn.learn_bpe_packed(t[:int(o[k])], sub_off, n_merges=a.oracle_merges, min_frequency=2, ctx=ctx)
        dev_ms = (time.perf_counter() - t0) * 1e3
        raw = t[:int(o[k])].tobytes()
        docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(k)]
        t0 = time.perf_counter()
        words, counts = LO.word_counts(docs)
        want = LO.learn_indexed(words, counts, a.oracle_merges, 2)
        host_ms = (time.perf_counter() - t0) * 1e3
        res.update(oracle_docs=k, oracle_merges=a.oracle_merges, oracle_merges_done=len(want.merges), oracle_host_ms=round(host_ms, 1),
                   oracle_device_ms=round(dev_ms, 3), oracle_files_equal=bool(dev.codes == want.codes and dev.vocab == want.vocab))

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
