"""One request through every door: the fifteen BM25 search entry points (bm25_tiny.ENTRIES) are widths of one search, so a request
sent through every entry point that can express it -- a null offset array for each list it does not use -- has one answer: ids,
score bits and counts are identical across the host and device forms, equal the match_count* forms' counts and what BM25.search /
search_near return, and a groups request of one-word groups equals the plain or boolean answer.  What the answers ARE is pinned
to the oracles by the other test_gpu_bm25*.py files; here only identity across the doors is asserted.  bm25_search_chunk = 2 * W64:
five queries take three chunks, and rows with more than three matches rank in runs of their own."""
import numpy as np
import pytest

import bm25_tiny as tiny
from genz_tokenize import _native
from genz_tokenize.ranking import BM25, BM25Plus

SOURCE = (7, 30, 64, 65, 129)          # query q = the distinct words of this document, so match="all" has something to find
K = 4
LISTS = {"ex_off": ("ex_terms",), "ph_off": ("ph_terms",), "nr_off": ("nr_terms", "nr_win")}


def strings():
    docs = tiny.documents()
    words = [docs[d].split() for d in SOURCE]
    queries = [" ".join(dict.fromkeys(w)) for w in words]
    exclude = [next(v for v in tiny.VOCAB if v not in w) if q % 2 == 0 else "" for q, w in enumerate(words)]
    phrase = [" ".join(w[1:3]) if q in (0, 2, 3) else "" for q, w in enumerate(words)]
    near = [w[0] + " " + w[-2] if q in (0, 1, 3) else "" for q, w in enumerate(words)]
    window = [len(w) if q == 0 else 3 for q, w in enumerate(words)]
    return docs, queries, exclude, phrase, near, window


def doors(req, grouped):
    """the entry points that can express req: those that take every list it uses (groups: no phrase and no near set)"""
    out = []
    for entry, fields in tiny.ENTRIES.items():
        if ("alt_terms" in fields) != grouped:
            continue
        if all(req[off] is None or off in fields for off in LISTS) and (req["mode"] == 0 or "mode" in fields):
            out.append(entry)
    return out


def send(ctx, index, entry, req):
    """(ids, score bits, counts) of a scored form -- the device forms through device memory --, (None, None, counts) of a count form"""
    nq = req["nq"]
    cnt = np.full(nq, -7, np.int64)
    if tiny.is_count(entry):
        rc = tiny.call(ctx.lib, index, entry, dict(req, cnt=cnt.ctypes.data))
        assert rc == _native.GZ_OK, (entry, rc)
        return None, None, cnt
    ids, sc = np.full((nq, K), -7, np.int64), np.full((nq, K), -7.0)
    if not tiny.is_device(entry):
        rc = tiny.call(ctx.lib, index, entry, dict(req, doc=ids.ctypes.data, score=sc.ctypes.data, cnt=cnt.ctypes.data))
        assert rc == _native.GZ_OK, (entry, rc)
        return ids, sc.view(np.uint64), cnt
    dev = [ctx.alloc(a.nbytes) for a in (ids, sc, cnt)]
    try:
        rc = tiny.call(ctx.lib, index, entry, dict(req, doc=dev[0], score=dev[1], cnt=dev[2]))
        assert rc == _native.GZ_OK, (entry, rc)
        ctx.sync()
        for d, a in zip(dev, (ids, sc, cnt)):
            ctx.d2h(a, d)
    finally:
        for d in dev:
            ctx.free(d)
    return ids, sc.view(np.uint64), cnt


@pytest.fixture(scope="module")
def world():
    ctx = _native.Context()
    docs = strings()[0]
    models = {(cls, pos): cls(docs, ctx=ctx, positions=pos) for cls in (BM25, BM25Plus) for pos in (True, False)}
    yield ctx, models
    models.clear()
    ctx.close()


@pytest.mark.gpu
def test_one_request_through_every_door(world):
    ctx, models = world
    _, queries, exclude, phrase, near, window = strings()
    nq = len(queries)
    _native.debug_set("bm25_search_chunk", 2 * tiny.W64, ctx)
    try:
        n_doors = 0
        for (cls, pos), m in models.items():
            _, terms, idf, qoff = m._queries(queries)
            assert (terms >= 0).all() and nq == 5
            xt, xo = m._exclusions(exclude, nq)
            base = dict(terms=terms, idf=idf, qoff=qoff, nq=nq, params=m._params(), plus=int(cls is BM25Plus), k=K, mode=0,
                        ex_terms=None, ex_off=None, ph_terms=None, ph_off=None, nr_terms=None, nr_off=None, nr_win=None)
            requests = [("plain", base, m.search(queries, K), m.count_matches(queries)),
                        ("all + exclude", dict(base, mode=1, ex_terms=xt, ex_off=xo), m.search(queries, K, "all", exclude),
                         m.count_matches(queries, "all", exclude))]
            if pos:
                pt, po = m._exclusions(phrase, nq)
                nt, no = m._sets(near)
                with_phrase = dict(requests[1][1], ph_terms=pt, ph_off=po)
                requests.append(("all + exclude + phrase", with_phrase, m.search(queries, K, "all", exclude, phrase),
                                 m.count_matches(queries, "all", exclude, phrase)))
                requests.append(("all + exclude + phrase + near", dict(with_phrase, nr_terms=nt, nr_off=no, nr_win=window),
                                 m.search_near(queries, K, near, window, "all", exclude, phrase),
                                 m.count_near(queries, near, window, "all", exclude, phrase)))
            for what, req, python, python_counts in requests:
                want = (python[0], python[1].view(np.uint64), python[2])
                assert np.array_equal(python_counts, want[2]), (cls, pos, what)
                # one-word groups: every word its own group, with the word's idf
                grouped = dict(req, alt_terms=terms, alt_off=np.arange(len(terms) + 1), group_idf=idf, group_off=qoff)
                for r, is_grouped in ((req, False), (grouped, True)):
                    for entry in doors(r, is_grouped):
                        got = send(ctx, m._index, entry, r)
                        for g, w, part in zip(got, want, ("ids", "score bits", "counts")):
                            assert g is None or np.array_equal(g, w), (cls.__name__, pos, what, entry, part, g, w)
                        n_doors += 1
            # the shapes this file is about: more than three matches in a row of the plain request, a match in every filtered one
            assert requests[0][2][2].max() > 3 and all(r[2][2].any() for r in requests), [r[2][2] for r in requests]
        # plain: 12 + 3 doors, boolean: 9 + 3, phrase: 6, near: 3 -- on the positional indexes; plain and boolean on the others
        assert n_doors == 2 * (15 + 12 + 6 + 3) + 2 * (15 + 12)
    finally:
        _native.debug_set("bm25_search_chunk", 1 << 27, ctx)
