"""Writes tests/golden/g8_bm25.jsonl.gz: the reference's BM25 / BM25Plus (genz_tokenize/ranking.py, numpy only) on hand-picked
edge cases and a few seeded corpora.

Run only in the build container (needs /root/reference, read-only).  The reference package is imported from there under its own
name, in this process only; the file written here is data (inputs + the reference's outputs):

    one JSON object per case: cls ("BM25" | "BM25Plus"), documents, queries, b, k1, delta (each as {"t": type, "v": value} -- ints stay
    ints), num_doc, fieldLens, avgFieldLen, frequency_word_in_doc (ordered [word, count] pairs per document), and per query: its
    words, df and idf of every word, and the scores ("int:0" for the int 0 of an empty query, else float.hex of the np.float64)

The reference is quadratic in the number of documents (cal_idf scans every document for every document), so corpora stay <= 400
documents.
"""
import gzip
import json
import os
import random
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, "/root/reference")
from genz_tokenize.ranking import BM25, BM25Plus  # noqa: E402  (the reference)

sys.path.insert(0, ROOT)
import corpus  # noqa: E402
import numpy as np  # noqa: E402

# the 29 code points of str.isspace()
WS = [chr(c) for c in list(range(0x09, 0x0E)) + list(range(0x1C, 0x21)) + [0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) +
      [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]]
assert len(WS) == 29 and all(c.isspace() for c in WS)


def num(x):
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise TypeError(x)
    return {"t": "int", "v": x} if isinstance(x, int) else {"t": "float", "v": float(x).hex()}


def score_repr(s):
    if type(s) is int:
        return "int:%d" % s
    assert type(s) is np.float64, type(s)
    return float(s).hex()


def case(cls, docs, queries, b=0.75, k1=1.2, delta=1.0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = BM25Plus(docs, b, k1, delta) if cls == "BM25Plus" else BM25(docs, b, k1)
        rec = dict(cls=cls, documents=docs, queries=queries, b=num(b), k1=num(k1), delta=num(delta), num_doc=m.num_doc,
                   fieldLens=list(m.fieldLens), avgFieldLen=float(m.avgFieldLen).hex(),
                   frequency_word_in_doc=[[[w, c] for w, c in f.items()] for f in m.frequency_word_in_doc], results=[])
        for q in queries:
            words = q.split()
            idf = [m.cal_idf(w) for w in words]
            df = [sum(1 if w in d else 0 for d in m.documents) for w in words]
            rec["results"].append(dict(words=words, df=df, idf=[float(v).hex() for v in idf], scores=[score_repr(s) for s in m.get_score(q)]))
    return rec


def edge_cases():
    out = []
    seps = "".join(WS)
    docs = ["a" + seps + "b", "a​b a﻿b", "x\x00y x\x00y z", "\ud800 \udfff \ud800", "\U0001F600 \U0010FFFF \U0001F600",
            "a b a b a", "", seps, "tiếng việt tiếng\nviệt\r\nnói", "a　b c\x85d\xa0e"]
    queries = ["a b", "a​b", "x\x00y", "\ud800 \udfff", "\U0001F600", "a a a", "absent", "", "   ", "việt tiếng nói c",
               "b　a", "a﻿b q a​b"]
    out.append(case("BM25", docs, queries))
    out.append(case("BM25Plus", docs, queries))
    out.append(case("BM25", [], ["a b", ""]))
    out.append(case("BM25Plus", [], ["a"]))
    out.append(case("BM25", ["", "", "   "], ["a", "", "b c"]))
    out.append(case("BM25Plus", ["", "\n"], ["a"], delta=-0.0))
    small = ["the cat sat", "the dog", "cat cat cat dog", "a b c d e f g", "the the the", "dog", "x"]
    sq = ["the cat", "dog dog", "zzz", "a g the", "cat the cat", ""]
    for b in (0, 1, 0.3, 1.5):
        for k1 in (0, 2):
            out.append(case("BM25", small, sq, b=b, k1=k1))
            out.append(case("BM25Plus", small, sq, b=b, k1=k1, delta=0.5))
    out.append(case("BM25", small, sq, b=1, k1=2))                                  # ints
    out.append(case("BM25Plus", small, sq, b=0, k1=0, delta=-0.0))
    out.append(case("BM25Plus", small, sq, b=0.75, k1=1.2, delta=-0.0))
    out.append(case("BM25", small, sq, b=1.5, k1=-1.0))                             # negative denominators
    return out


def seeded(cfg, n, seed, n_queries):
    t, o, _ = corpus.config_corpus(cfg, n_docs=n, seed=seed)
    raw = t.tobytes()
    docs = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n)]
    r = random.Random(seed)
    vocab = sorted({w for d in docs for w in d.split()})
    queries = []
    for _ in range(n_queries):
        k = r.randint(1, 8)
        words = [r.choice(vocab) if r.random() < 0.8 else "absent%d" % r.randint(0, 9) for _ in range(k)]
        if r.random() < 0.3:
            words.append(words[0])                                                   # a repeated word
        queries.append(" ".join(words))
    return docs, queries


def main():
    recs = edge_cases()
    for cfg, n, seed in ((2, 300, 11), (2, 400, 12), (4, 120, 13)):
        docs, queries = seeded(cfg, n, seed, 12)
        recs.append(case("BM25", docs, queries))
        recs.append(case("BM25Plus", docs, queries, b=0.3, k1=2.0, delta=0.5))
    path = os.path.join(ROOT, "tests", "golden", "g8_bm25.jsonl.gz")
    with gzip.open(path, "wt", encoding="ascii", compresslevel=9) as f:
        for r in recs:
            f.write(json.dumps(r, ensure_ascii=True) + "\n")
    print(path, os.path.getsize(path), "bytes,", len(recs), "cases")


if __name__ == "__main__":
    main()
