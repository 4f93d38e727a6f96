"""Text quality signals (gz_text_signals_device; csrc/gz_quality.inc) over the configs[3] corpus resident in HBM, every 4 consecutive
documents joined by '\\n' and every 16th join '\\n\\n' (the corpus as it stands has almost no line breaks): the call with and without
the optional arrays, pass A with its scans alone (the offsets are the only outputs), the five-filter pre-pass chain over the same text
measured in the same visit, and the plain-Python rule on the host.

    python tools/quality_bench.py [--docs 1000000] [--reps 7] [--runs 2] [--oracle-docs 4096] [--out profiles/quality_bench.json]

Host clock around call + gz_sync, after a warm-up call of each; --reps rounds that run the calls one after the other (interleaved),
medians; --runs such series, each reported.  The tool asserts that the device's fourteen signals and six arrays equal
tests/quality_oracle.py on the first --oracle-docs joined documents.  One JSON line on stdout.

On a shared GPU the step gets a time limit of its own:
    timeout -k 10 900 python tools/quality_bench.py --out profiles/quality_bench.json"""
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


def joined(text, offs):
    """every 4 consecutive documents become one, joined by '\\n'; every 16th join is '\\n\\n'"""
    n = (len(offs) - 1) // 4 * 4
    lens = np.diff(offs[:n + 1])
    i = np.arange(n, dtype=np.int64)
    join = i - i // 4                                                 # (three joins a group; the last of a group has none behind it)
    sep = np.where(i % 4 == 3, 0, np.where(join % 16 == 15, 2, 1))
    starts = np.concatenate([[0], np.cumsum(lens + sep)])
    out = np.full(int(starts[-1]), 0x0A, dtype=np.uint8)
    raw = text[int(offs[0]):int(offs[n])]
    idx = np.arange(len(raw), dtype=np.int64) + np.repeat(starts[:-1] - (offs[:n] - offs[0]), lens)
    out[idx] = raw
    return out, np.ascontiguousarray(starts[::4], dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--oracle-docs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import corpus
    import quality_oracle as Q
    from genz_tokenize import _native
    text, offs, _ = corpus.config_corpus(3, n_docs=args.docs)
    text, offs = joined(np.ascontiguousarray(text, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.int64))
    n, nbytes = len(offs) - 1, int(offs[-1])
    ctx = _native.Context()
    d_t, d_o = ctx.alloc(nbytes + 64), ctx.alloc(offs.nbytes)
    ctx.h2d(d_t, text); ctx.h2d(d_o, offs)
    d_sig, d_lo, d_po = ctx.alloc(4 * 14 * n), ctx.alloc(4 * (n + 1)), ctx.alloc(4 * (n + 1))
    ctx.text_signals_device(d_t, d_o, n, 0, d_lo, 0, 0, d_po, 0, 0)
    lo, po = np.empty(n + 1, np.uint32), np.empty(n + 1, np.uint32)
    ctx.d2h(lo, d_lo); ctx.d2h(po, d_po)
    L, P = int(lo[n]), int(po[n])
    d_ls, d_lf, d_ps, d_pf = ctx.alloc(16 * L + 64), ctx.alloc(4 * L + 64), ctx.alloc(16 * P + 64), ctx.alloc(4 * P + 64)
    d_pp, d_ppo = ctx.alloc(nbytes + 64), ctx.alloc(8 * (n + 1))
    ops = [_native.GZ_PP_HTML, _native.GZ_PP_URL, _native.GZ_PP_UNICODE, _native.GZ_PP_EMOJI, _native.GZ_PP_PUNCT]
    calls = {
        "signals": lambda: ctx.text_signals_device(d_t, d_o, n, d_sig),
        "signals_and_arrays": lambda: ctx.text_signals_device(d_t, d_o, n, d_sig, d_lo, d_ls, d_lf, d_po, d_ps, d_pf),
        "pass_a_and_scans": lambda: ctx.text_signals_device(d_t, d_o, n, 0, d_lo, 0, 0, d_po, 0, 0),
        "preprocess_chain": lambda: ctx.preprocess_device(ops, d_t, d_o, n, nbytes, d_pp, nbytes, d_ppo),
    }
    for fn in calls.values():
        fn()
    series = []
    for _ in range(args.runs):
        t = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                t[k].append(timed(fn))
        series.append(t)
    med = {k: [round(float(np.median(s[k])), 3) for s in series] for k in calls}
    rec = {"bench": "quality", "docs": n, "bytes": nbytes, "lines": L, "paragraphs": P, "reps": args.reps, "runs": args.runs,
           "ms_runs": med, "all_ms": {k: [[round(x, 3) for x in s[k]] for s in series] for k in calls},
           "ratio_to_preprocess": {k: round(med[k][0] / med["preprocess_chain"][0], 3) for k in calls},
           "spans_ms": round(med["signals"][0] - med["pass_a_and_scans"][0], 3),
           "GB_per_s_text_read_twice": round(2 * nbytes / med["signals"][0] / 1e6, 1)}
    # the rule on the host over the first documents, and the device's outputs against it
    k = min(args.oracle_docs, n)
    calls["signals_and_arrays"]()
    got = {"signals": np.empty((14, n), np.int32), "line_span": np.empty((L, 2), np.int64), "line_first": np.empty(L, np.int32),
           "para_span": np.empty((P, 2), np.int64), "para_first": np.empty(P, np.int32)}
    for name, d in (("signals", d_sig), ("line_span", d_ls), ("line_first", d_lf), ("para_span", d_ps), ("para_first", d_pf)):
        ctx.d2h(got[name], d)
    ctx.d2h(lo, d_lo); ctx.d2h(po, d_po)
    raw = text.tobytes()
    docs = [raw[offs[i]:offs[i + 1]] for i in range(k)]
    res = {}
    orc_ms = timed(lambda: res.update(Q.signals(docs)))
    ok = all(np.array_equal(got["signals"][i][:k], res[name]) for i, name in enumerate(Q.NAMES))
    ok = ok and np.array_equal(lo[:k + 1], res["line_off"]) and np.array_equal(po[:k + 1], res["para_off"])
    for kind, off in (("line", lo), ("para", po)):
        ok = ok and np.array_equal(got[kind + "_span"][:off[k]], res[kind + "_span"]) and np.array_equal(got[kind + "_first"][:off[k]], res[kind + "_first"])
    assert ok, "the device's outputs differ from the host rule on the first %d documents" % k
    rec["oracle"] = {"docs": k, "bytes": int(offs[k]), "ns_per_byte": round(orc_ms * 1e6 / max(int(offs[k]), 1), 1),
                     "device_ns_per_byte": round(med["signals"][0] * 1e6 / nbytes, 4), "checked": bool(ok),
                     "documents_with_a_duplicate_line": int((got["signals"][9] > 0).sum())}
    for d in (d_t, d_o, d_sig, d_lo, d_po, d_ls, d_lf, d_ps, d_pf, d_pp, d_ppo):
        ctx.free(d)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
