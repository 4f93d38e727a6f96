"""Oracles shared by the BM25 GPU tests (numpy only; nothing here touches the GPU).

    restate(m, queries)              get_scores: bm25_restate.scores row by row, the reference's arithmetic in its order
    topk_oracle / topk_check         top_k: np.argsort(-S, kind="stable")[:k'] and the scores' original bits
    matched / oracle / check         search, count_matches: with R = set(query.split()), X = set(exclude.split()) and W(d) the words of
                                     document d,  "any": R & W(d) and not X & W(d)    "all": R and R <= W(d) and not X & W(d);
                                     row q = [i for i in argsort(-S[q], stable) if matched[q, i]][:k'], -1 / the NaN PAD behind it
    gather / check_rows              the same for a batch that repeats a few distinct (query, exclude) pairs: the oracle once per
                                     pair, its rows gathered
    decoded                          term_sequences() as lists of words, to set against [d.split() for d in documents]
    vocab_oracle                     vocabulary(): the words of d.split() in first-occurrence order and their document frequencies
    WS / NEAR / sweep_docs           the document-side inputs: the 29 str.isspace() code points, their non-whitespace neighbours in the
                                     UTF-8 byte space, and every one of them at every byte offset of the first two 64-byte tiles
ids and counts are compared with ==, scores as uint64 bit patterns: there are no tolerances."""
import numpy as np

import bm25_restate as R
from genz_tokenize.ranking import BM25, BM25Plus

PAD = np.uint64(0x7FF8000000000000)
MODES = ("any", "all")
CLASSES = ("BM25", "BM25Plus")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model(cls, docs, ctx=None):
    """BM25 with its defaults, BM25Plus with b=0.3, k1=2.0, delta=0.5"""
    return BM25Plus(docs, 0.3, 2.0, 0.5, ctx=ctx) if cls == "BM25Plus" else BM25(docs, ctx=ctx)


def restate(m, queries, post=None):
    """float64 [len(queries), num_doc]: what get_scores(queries) must return, to the bit"""
    if post is None:
        post = R.Postings(m.frequency_word_in_doc)
    lens = m.fieldLens
    avg = R.avg_field_len(lens)
    delta = getattr(m, "delta", None)
    idf = {}
    out = np.zeros((len(queries), m.num_doc), dtype=np.float64)
    for q, text in enumerate(queries):
        words = text.split()
        for w in words:
            if w not in idf:
                idf[w] = R.idf(m.num_doc, post.df(w))
        if words:
            out[q] = R.scores(lens, post, avg, words, [idf[w] for w in words], m.b, m.k1, delta)
    return out


def topk_oracle(S, k):
    S = np.asarray(S, dtype=np.float64)
    kk = min(k, S.shape[1])
    ids = np.argsort(-S, axis=1, kind="stable")[:, :kk].astype(np.int64)
    return ids, bits(np.take_along_axis(S, ids, 1))


def topk_check(got, S, k, what=""):
    ids, sc = got
    want_ids, want_sc = topk_oracle(S, k)
    assert ids.dtype == np.int64 and sc.dtype == np.float64, what
    assert ids.shape == want_ids.shape and sc.shape == want_sc.shape, (what, ids.shape, want_ids.shape)
    assert np.array_equal(ids, want_ids), what
    assert np.array_equal(bits(sc), want_sc), what


def matched(post, queries, match="any", exclude=None):
    m = np.zeros((len(queries), post.n), dtype=bool)
    for q, text in enumerate(queries):
        need = set(text.split())
        if match == "any":
            for w in need:
                if w in post.p:
                    m[q, post.p[w][0]] = True
        elif need and all(w in post.p for w in need):
            m[q] = True
            for w in need:
                has = np.zeros(post.n, dtype=bool)
                has[post.p[w][0]] = True
                m[q] &= has
        if exclude is not None:
            for w in set(exclude[q].split()):
                if w in post.p:
                    m[q, post.p[w][0]] = False
    return m


def oracle(S, m, k):
    """(ids int64, scores as uint64 bits, counts int64) of search(queries, k) for the score rows S and the matched sets m"""
    S = np.asarray(S, dtype=np.float64)
    nq, n = S.shape
    kk = min(k, n)
    ids = np.full((nq, kk), -1, dtype=np.int64)
    sc = np.full((nq, kk), PAD, dtype=np.uint64)
    order = np.argsort(-S, axis=1, kind="stable")
    for q in range(nq):
        o = order[q][m[q][order[q]]][:kk]
        ids[q, :len(o)] = o
        sc[q, :len(o)] = bits(S[q, o])
    return ids, sc, m.sum(axis=1).astype(np.int64)


def gather(want, rows):
    """the oracle of a batch whose row r is the oracle's row rows[r]"""
    return tuple(x[rows] for x in want)


def check_rows(got, want, what=""):
    ids, sc, cnt = got
    want_ids, want_sc, want_cnt = want
    assert ids.dtype == np.int64 and sc.dtype == np.float64 and cnt.dtype == np.int64, what
    assert ids.shape == want_ids.shape and sc.shape == want_sc.shape and cnt.shape == want_cnt.shape, (what, ids.shape, want_ids.shape)
    assert np.array_equal(cnt, want_cnt), (what, np.flatnonzero(cnt != want_cnt)[:10].tolist())
    assert np.array_equal(ids, want_ids), (what, np.flatnonzero((ids != want_ids).any(axis=1))[:10].tolist())
    assert np.array_equal(bits(sc), want_sc), (what, np.flatnonzero((bits(sc) != want_sc).any(axis=1))[:10].tolist())


def check(got, S, m, k, what=""):
    check_rows(got, oracle(S, m, k), what)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


def decoded(m, compacted=False):
    """term_sequences() as lists of words: through vocabulary() on a compacted index, else through _lookup of the current words"""
    terms, off = m.term_sequences()
    assert terms.dtype == np.int32 and off.dtype == np.int64 and off.shape == (m.num_doc + 1,) and terms.shape == (int(off[-1]),)
    if compacted:
        words = m.vocabulary()[0]
        name = dict(enumerate(words))
    else:
        words = sorted({w for t in m._texts for w in t.split()})
        ids = m._lookup(words)[0].tolist() if words else []
        assert len(set(ids)) == len(ids) and -1 not in ids
        name = dict(zip(ids, words))
    t, o = terms.tolist(), off.tolist()
    return [[name[x] for x in t[o[d]:o[d + 1]]] for d in range(m.num_doc)]


def vocab_oracle(docs):
    """(words in the order of their first occurrence over d.split(), df list): what vocabulary() must return"""
    df = {}
    for d in docs:
        for w in dict.fromkeys(d.split()):
            df[w] = df.get(w, 0) + 1
    return list(df), list(df.values())


# ---- document-side inputs: where str.split() cuts, against the 64-byte tiles of the word walk -----------------------------------------
WS = [chr(c) for c in range(0x110000) if chr(c).isspace()]               # the 29 code points: 10 of 1 byte, 2 of 2 bytes, 17 of 3 bytes
# not whitespace, but next to it in the UTF-8 byte space: the controls around 09..0D and 1C..20, the C1 neighbours of 85 and A0, 85 / A0
# behind another lead byte, the neighbours of 1680, 2000..200A, 2028, 2029, 202F, 205F and 3000, the former whitespace 180E and 200B,
# and other lead bytes (EF, EE, ED of a lone surrogate, F0, F4)
NEAR = [chr(c) for c in (0x00, 0x08, 0x0E, 0x1B, 0x21, 0x7F,
                         0x80, 0x84, 0x86, 0x9F, 0xA1,
                         0x0485, 0x04A0,
                         0x167F, 0x1681, 0x180E, 0x1FFF,
                         0x200B, 0x200C, 0x2027, 0x202A, 0x202E, 0x2030, 0x205E, 0x2060, 0x2FFF, 0x3001,
                         0xFEFF, 0xE000, 0xD800, 0x1F600, 0x10FFFF)]
SWEEP_K = range(0, 131)


def encoded(text):
    """the bytes of a document as the index sees them (_packing.pack: UTF-8 with surrogatepass)"""
    return text.encode("utf-8", "surrogatepass")


def sweep_docs():
    """"x" * k + c + tail for every c of WS + NEAR, k in 0 .. 130 and tail in ("y", "", c + "z"): c's first byte at every lane of the
    first two tiles and at the start of the third; followed by a word, ending the document, and doubled"""
    return ["x" * k + c + tail for c in WS + NEAR for k in SWEEP_K for tail in ("y", "", c + "z")]
