"""A vectorised numpy restatement of the reference's genz_tokenize/ranking.py (numpy only), for the BM25 tests.

    fieldLens / frequency_word_in_doc   ranking.py:14-26    document.split(), counts in first-occurrence order
    avgFieldLen                         ranking.py:27       np.mean(fieldLens)
    idf                                 ranking.py:29-31    np.log(1+(N-df+0.5)/(df+0.5)), a SCALAR np.log per query word
    BM25 score                          ranking.py:33-45    score = 0; score += idf*((f*(k1+1))/(f+k1*(1-b+b*(len(doc)/avg))))
    BM25Plus score                      ranking.py:52-63    ... idf*(... + delta)

The scores are computed for all documents at once with numpy's elementwise float64 operations (each one IEEE-rounded, never fused),
in the reference's order and association, so they equal the reference's scalar arithmetic bit for bit."""
import warnings

import numpy as np


def stats(documents):
    """(fieldLens list, frequency_word_in_doc list of dicts) as the reference builds them."""
    lens, freq = [], []
    for d in documents:
        words = d.split()
        f = {}
        for w in words:
            f[w] = f.get(w, 0) + 1
        lens.append(len(words))
        freq.append(f)
    return lens, freq


def avg_field_len(lens):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.mean(lens)


def idf(n_docs, df):
    return np.log(1+(n_docs-df+0.5)/(df+0.5))


def doc_freq(freq, word):
    return sum(1 for f in freq if word in f)


class Postings:
    """word -> (documents, counts) over frequency_word_in_doc: the f of a query word for every document at once."""

    def __init__(self, freq):
        self.n = len(freq)
        acc = {}
        for d, f in enumerate(freq):
            for w, c in f.items():
                acc.setdefault(w, ([], []))
                acc[w][0].append(d)
                acc[w][1].append(c)
        self.p = {w: (np.array(ds, dtype=np.int64), np.array(cs, dtype=np.float64)) for w, (ds, cs) in acc.items()}

    def get(self, w):
        f = np.zeros(self.n, dtype=np.float64)
        if w in self.p:
            f[self.p[w][0]] = self.p[w][1]
        return f

    def df(self, w):
        return len(self.p[w][0]) if w in self.p else 0


def scores(lens, freq, avg, words, idfs, b, k1, delta=None):
    """float64 [N] for one query's words (non-empty) with their idf; delta None: BM25, else BM25Plus.  freq: the list of dicts, or a
    Postings of it."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dl = np.asarray(lens, dtype=np.int64)
        K = np.float64(k1) * (np.float64(1 - b) + np.float64(b) * (dl / avg))
        kp1 = np.float64(k1 + 1)
        score = np.zeros(len(lens), dtype=np.float64)
        for w, v in zip(words, idfs):
            f = freq.get(w) if isinstance(freq, Postings) else np.array([fd.get(w, 0) for fd in freq], dtype=np.float64)
            t = (f * kp1) / (f + K)
            score = score + (np.float64(v) * t if delta is None else np.float64(v) * (t + np.float64(delta)))
        return score

