"""The refusal matrix of the fifteen BM25 search entry points (gz_bm25_search, _bool, _phrase, _near, _groups; their _device and
gz_bm25_match_count* forms), called through ctypes on a tiny index: every bad call answers one exact (return code, gz_last_error
text), and of two faults at once the one that the entry point checks first.  EXPECT holds what the library answered before the
entry points were folded into one request and one prologue; nothing here is derived from the code under test.  A refused call
launches nothing: every output, host and device, keeps its fill."""
import ctypes

import numpy as np
import pytest

import bm25_tiny as tiny
from genz_tokenize import _native
from genz_tokenize.ranking import BM25

T = 12                                                # n_terms of the tiny index: the first id that is out of range
WIDE = list(range(65)) + [3, -1, 7]                   # a group of 65 distinct alternatives (a repeat and a -1 do not count), and one more

# (label, what the call changes in the good request; "index": None, "nopos" (built without positions) or "big" (1030 documents and terms))
CASES = [
    ("null index", dict(index=None)),
    ("null query_off", dict(qoff=None)),
    ("null group_off", dict(group_off=None)),
    ("n_queries -1", dict(nq=-1)),
    ("decreasing query_off", dict(qoff=[0, 2, 1])),
    ("decreasing ex_off", dict(ex_terms=[0, 1], ex_off=[0, 2, 1])),
    ("decreasing ph_off", dict(ph_terms=[0, 1], ph_off=[0, 2, 1])),
    ("decreasing near_off", dict(nr_terms=[0, 1], nr_off=[0, 2, 1], nr_win=[2, 2])),
    ("decreasing group_off", dict(group_off=[0, 2, 1])),
    ("decreasing alt_off", dict(alt_off=[0, 3, 2])),
    ("term id n_terms", dict(terms=[0, T, 2])),
    ("term id -2", dict(terms=[0, -2, 2])),
    ("excluded id n_terms", dict(ex_terms=[T], ex_off=[0, 1, 1])),
    ("excluded id -2", dict(ex_terms=[-2], ex_off=[0, 1, 1])),
    ("phrase id n_terms", dict(ph_terms=[T], ph_off=[0, 1, 1])),
    ("phrase id -2", dict(ph_terms=[-2], ph_off=[0, 1, 1])),
    ("near id n_terms", dict(nr_terms=[T], nr_off=[0, 1, 1], nr_win=[2, 2])),
    ("near id -2", dict(nr_terms=[-2], nr_off=[0, 1, 1], nr_win=[2, 2])),
    ("alternative id n_terms", dict(alt_terms=[0, T, 2])),
    ("alternative id -2", dict(alt_terms=[0, -2, 2])),
    ("query_off without terms", dict(terms=None)),
    ("query_off without idf", dict(idf=None)),
    ("ex_off without terms", dict(ex_terms=None, ex_off=[0, 1, 1])),
    ("ph_off without terms", dict(ph_terms=None, ph_off=[0, 1, 1])),
    ("near_off without terms", dict(nr_terms=None, nr_off=[0, 1, 1], nr_win=[2, 2])),
    ("alt_off without terms", dict(alt_terms=None)),
    ("group_off without idf", dict(group_idf=None)),
    ("group_off without alt_off", dict(alt_off=None)),
    ("null params", dict(params=None)),
    ("null doc_out", dict(doc=None)),
    ("null score_out", dict(score=None)),
    ("null doc_out and score_out", dict(doc=None, score=None)),
    ("null count_out", dict(cnt=None)),
    ("k 0", dict(k=0)),
    ("k' above GZ_BM25_TOPK_MAX", dict(index="big", k=1025)),
    ("mode 2", dict(mode=2)),
    ("phrase without positions", dict(index="nopos", ph_terms=[0], ph_off=[0, 1, 1])),
    ("near without positions", dict(index="nopos", nr_terms=[0], nr_off=[0, 1, 1], nr_win=[2, 2])),
    ("phrase of 65 words", dict(ph_terms=[0] * 65, ph_off=[0, 65, 65])),
    ("65 near terms", dict(nr_terms=[0] * 65, nr_off=[0, 65, 65], nr_win=[2, 2])),
    ("window 0", dict(nr_terms=[0], nr_off=[0, 1, 1], nr_win=[0, 5])),
    ("null windows", dict(nr_terms=[0], nr_off=[0, 1, 1], nr_win=None)),
    ("group of 65 alternatives", dict(index="big", alt_terms=WIDE, alt_off=[0, 67, 68])),
    # two faults at once: the order of the checks
    ("k 0 + mode 2", dict(k=0, mode=2)),
    ("k 0 + excluded id n_terms", dict(k=0, ex_terms=[T], ex_off=[0, 1, 1])),
    ("excluded id n_terms + null count_out", dict(ex_terms=[T], ex_off=[0, 1, 1], cnt=None)),
    ("null doc_out + decreasing group_off", dict(doc=None, group_off=[0, 2, 1])),
    ("null count_out + decreasing group_off", dict(cnt=None, group_off=[0, 2, 1])),
    ("null count_out + decreasing query_off", dict(cnt=None, qoff=[0, 2, 1])),
    ("null params + k 0", dict(params=None, k=0)),
    ("term id n_terms + k 0", dict(terms=[0, T, 2], k=0)),
    ("alternative id n_terms + k 0", dict(alt_terms=[0, T, 2], k=0)),
    ("mode 2 + phrase id n_terms", dict(mode=2, ph_terms=[T], ph_off=[0, 1, 1])),
    ("phrase id n_terms + window 0", dict(ph_terms=[T], ph_off=[0, 1, 1], nr_terms=[0], nr_off=[0, 1, 1], nr_win=[0, 5])),
    ("phrase without positions + null count_out", dict(index="nopos", ph_terms=[0], ph_off=[0, 1, 1], cnt=None)),
    ("phrase of 65 words + null count_out", dict(ph_terms=[0] * 65, ph_off=[0, 65, 65], cnt=None)),
    ("group of 65 alternatives + mode 2", dict(index="big", alt_terms=WIDE, alt_off=[0, 67, 68], mode=2)),
    ("group of 65 alternatives + excluded id n_terms", dict(index="big", alt_terms=WIDE, alt_off=[0, 67, 68], ex_terms=[1030], ex_off=[0, 1, 1])),
    ("group of 65 alternatives + k 0", dict(index="big", alt_terms=WIDE, alt_off=[0, 67, 68], k=0)),
]

# the entry points by what they take: a set name, "A & B" for those in both, "X | Y" for those in either
SETS = {"ALL": lambda f: True, "WORDS": lambda f: "terms" in f, "GROUPS": lambda f: "alt_terms" in f, "SCORED": lambda f: "k" in f,
        "COUNT": lambda f: "k" not in f, "MODE": lambda f: "mode" in f, "PHRASE": lambda f: "ph_off" in f, "NEAR": lambda f: "nr_off" in f}


def members(expr):
    return {e for e, f in tiny.ENTRIES.items() if any(all(SETS[n.strip()](f) for n in part.split("&")) for part in expr.split("|"))}


# label -> [return code, gz_last_error text (None: the call leaves the text as it was), the entry points that answer so]
EXPECT = {
    'null index': [[-1, None, 'ALL']],
    'null query_off': [[-1, 'bad arguments', 'WORDS']],
    'null group_off': [[-1, 'bad arguments', 'GROUPS']],
    'n_queries -1': [[-1, 'bad arguments', 'ALL']],
    'decreasing query_off': [[-1, 'query offsets must not decrease', 'WORDS']],
    'decreasing ex_off': [[-1, 'excluded-term offsets must not decrease', 'MODE']],
    'decreasing ph_off': [[-1, 'phrase-term offsets must not decrease', 'PHRASE']],
    'decreasing near_off': [[-1, 'near-term offsets must not decrease', 'NEAR']],
    'decreasing group_off': [[-1, 'group offsets must not decrease', 'GROUPS']],
    'decreasing alt_off': [[-1, 'alternative offsets must not decrease', 'GROUPS']],
    'term id n_terms': [[-1, 'term id 12 out of range', 'WORDS']],
    'term id -2': [[-1, 'term id -2 out of range', 'WORDS']],
    'excluded id n_terms': [[-1, 'excluded term id 12 out of range', 'MODE']],
    'excluded id -2': [[-1, 'excluded term id -2 out of range', 'MODE']],
    'phrase id n_terms': [[-1, 'phrase term id 12 out of range', 'PHRASE']],
    'phrase id -2': [[-1, 'phrase term id -2 out of range', 'PHRASE']],
    'near id n_terms': [[-1, 'near term id 12 out of range', 'NEAR']],
    'near id -2': [[-1, 'near term id -2 out of range', 'NEAR']],
    'alternative id n_terms': [[-1, 'alternative term id 12 out of range', 'GROUPS']],
    'alternative id -2': [[-1, 'alternative term id -2 out of range', 'GROUPS']],
    'query_off without terms': [[-1, 'bad query offsets', 'WORDS']],
    'query_off without idf': [[-1, 'bad query offsets', 'WORDS & SCORED']],
    'ex_off without terms': [[-1, 'excluded-term offsets without terms', 'MODE']],
    'ph_off without terms': [[-1, 'phrase-term offsets without terms', 'PHRASE']],
    'near_off without terms': [[-1, 'near-term offsets without terms', 'NEAR']],
    'alt_off without terms': [[-1, 'alternative offsets without terms', 'GROUPS']],
    'group_off without idf': [[-1, 'group offsets without alternatives or idf', 'GROUPS & SCORED']],
    'group_off without alt_off': [[-1, 'group offsets without alternatives or idf', 'GROUPS']],
    'null params': [[-1, 'bad arguments', 'SCORED']],
    'null doc_out': [[-1, 'bad arguments', 'SCORED']],
    'null score_out': [[-1, 'bad arguments', 'SCORED']],
    'null doc_out and score_out': [[-1, 'bad arguments', 'SCORED']],
    'null count_out': [[-1, 'bad arguments', 'ALL']],
    'k 0': [[-1, 'k = 0; top-k takes k >= 1', 'SCORED']],
    "k' above GZ_BM25_TOPK_MAX": [[-6, 'k = 1025 over 1030 documents; top-k takes at most 1024', 'SCORED']],
    'mode 2': [[-1, 'match mode 2: GZ_BM25_MATCH_ANY or GZ_BM25_MATCH_ALL', 'MODE']],
    'phrase without positions': [[-1, 'a phrase search needs an index built with GZ_BM25_POSITIONS', 'PHRASE']],
    'near without positions': [[-1, 'a near search needs an index built with GZ_BM25_POSITIONS', 'NEAR']],
    'phrase of 65 words': [[-6, 'a phrase of 65 words; a phrase takes at most 64', 'PHRASE']],
    '65 near terms': [[-6, '65 near terms; a query takes at most 64', 'NEAR']],
    'window 0': [[-1, 'window = 0; a near search takes a window >= 1', 'NEAR']],
    'null windows': [[-1, 'near-term offsets without windows', 'NEAR']],
    'group of 65 alternatives': [[-6, 'a group of 65 distinct alternatives; a group takes at most 64', 'GROUPS']],
    'k 0 + mode 2': [[-1, 'k = 0; top-k takes k >= 1', 'SCORED & MODE']],
    'k 0 + excluded id n_terms': [[-1, 'k = 0; top-k takes k >= 1', 'SCORED & MODE']],
    'excluded id n_terms + null count_out': [
        [-1, 'excluded term id 12 out of range', 'WORDS & SCORED & MODE'],
        [-1, 'bad arguments', 'COUNT & MODE | GROUPS'],
    ],
    'null doc_out + decreasing group_off': [[-1, 'bad arguments', 'GROUPS & SCORED']],
    'null count_out + decreasing group_off': [[-1, 'bad arguments', 'GROUPS']],
    'null count_out + decreasing query_off': [
        [-1, 'query offsets must not decrease', 'WORDS & SCORED'],
        [-1, 'bad arguments', 'WORDS & COUNT'],
    ],
    'null params + k 0': [[-1, 'bad arguments', 'SCORED']],
    'term id n_terms + k 0': [[-1, 'term id 12 out of range', 'WORDS & SCORED']],
    'alternative id n_terms + k 0': [[-1, 'alternative term id 12 out of range', 'GROUPS & SCORED']],
    'mode 2 + phrase id n_terms': [[-1, 'match mode 2: GZ_BM25_MATCH_ANY or GZ_BM25_MATCH_ALL', 'PHRASE']],
    'phrase id n_terms + window 0': [[-1, 'phrase term id 12 out of range', 'NEAR']],
    'phrase without positions + null count_out': [
        [-1, 'a phrase search needs an index built with GZ_BM25_POSITIONS', 'SCORED & PHRASE'],
        [-1, 'bad arguments', 'COUNT & PHRASE'],
    ],
    'phrase of 65 words + null count_out': [
        [-6, 'a phrase of 65 words; a phrase takes at most 64', 'SCORED & PHRASE'],
        [-1, 'bad arguments', 'COUNT & PHRASE'],
    ],
    'group of 65 alternatives + mode 2': [[-1, 'match mode 2: GZ_BM25_MATCH_ANY or GZ_BM25_MATCH_ALL', 'GROUPS']],
    'group of 65 alternatives + excluded id n_terms': [[-1, 'excluded term id 1030 out of range', 'GROUPS']],
    'group of 65 alternatives + k 0': [[-1, 'k = 0; top-k takes k >= 1', 'GROUPS & SCORED']],
}


def applies(entry, change):
    return all(f == "index" or f in tiny.ENTRIES[entry] for f in change)


def expected(entry, label):
    for rc, text, entries in EXPECT.get(label, ()):
        if entry in members(entries):
            return rc, text
    return None


class World:
    MARK = "width = 0; a snippet takes width >= 1"

    def __init__(self):
        self.ctx = _native.Context()
        docs = tiny.documents()
        self.models = {"pos": BM25(docs, ctx=self.ctx, positions=True), "nopos": BM25(docs, ctx=self.ctx),
                       "big": BM25(["b%d" % i for i in range(1030)], ctx=self.ctx)}
        assert self.ctx.bm25_info(self.models["pos"]._index)[:2] == (tiny.N_DOCS, T)
        assert self.ctx.bm25_info(self.models["big"]._index)[:2] == (1030, 1030)
        self.lib = self.ctx.lib
        self.host = [np.full((2, 4), 77, np.int64), np.full((2, 4), 7.5), np.full(2, 77, np.int64)]
        self.dev = [self.ctx.alloc(a.nbytes) for a in self.host]
        self.fill()
        self.good = dict(terms=[0, 1, 2], idf=[1.0, 1.5, 2.0], qoff=[0, 2, 3], nq=2, params=self.models["pos"]._params(), plus=0, k=4, mode=0,
                         ex_terms=None, ex_off=None, ph_terms=None, ph_off=None, nr_terms=None, nr_off=None, nr_win=None,
                         alt_terms=[0, 1, 2], alt_off=[0, 2, 3], group_idf=[1.0, 2.0], group_off=[0, 1, 2])

    def fill(self):
        self.host[0][:], self.host[1][:], self.host[2][:] = 77, 7.5, 77
        for d, a in zip(self.dev, self.host):
            self.ctx.h2d(d, np.full(a.nbytes, 0xA5, np.uint8))

    def last_error(self):
        return self.lib.gz_last_error(self.ctx.handle).decode("utf-8", "replace")

    def answer(self, entry, change):
        """(return code, text) of the good request with `change` applied; text None when the call left the text alone"""
        req = dict(self.good)
        outs = self.dev if tiny.is_device(entry) else [a.ctypes.data for a in self.host]
        req.update(doc=outs[0], score=outs[1], cnt=outs[2])
        req.update({f: v for f, v in change.items() if f != "index"})
        which = change.get("index", "pos")
        index = 0 if which is None else self.models[which]._index
        # a refusal of another entry point with a text no search call has: whether the call under test wrote a text shows
        pos = self.models["pos"]._index
        q = np.array([0, 0], np.int64)
        assert self.lib.gz_bm25_snippets(ctypes.c_void_p(pos), None, ctypes.c_void_p(q.ctypes.data), 1, None, 0, 0, None, None) == _native.GZ_E_INVALID
        assert self.last_error() == self.MARK
        rc = tiny.call(self.lib, index, entry, req)
        text = self.last_error()
        return rc, (None if text == self.MARK else text)

    def untouched(self):
        if not ((self.host[0] == 77).all() and (self.host[1] == 7.5).all() and (self.host[2] == 77).all()):
            return False
        self.ctx.sync()
        for d, a in zip(self.dev, self.host):
            x = np.empty(a.nbytes, np.uint8)
            self.ctx.d2h(x, d)
            if not (x == 0xA5).all():
                return False
        return True

    def close(self):
        for d in self.dev:
            self.ctx.free(d)
        self.models.clear()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(tiny.ENTRIES))
def test_refusals(world, entry):
    wrong = []
    for label, change in CASES:
        if not applies(entry, change):
            continue
        got, want = world.answer(entry, change), expected(entry, label)
        print("%-32s %-50s -> %r" % (entry, label, got))
        if want is None or got != tuple(want):
            wrong.append((label, got, want))
    assert not wrong, wrong
    assert world.untouched()
    # the index still answers, and the good request is one: the refusals above were refusals of what they changed
    assert world.answer(entry, {})[0] == _native.GZ_OK
    world.ctx.sync()
    world.fill()


def test_every_expectation_is_asked():
    asked = {(e, label) for label, change in CASES for e in tiny.ENTRIES if applies(e, change)}
    assert all(sum(len(members(r[2])) for r in rows) == len(set().union(*(members(r[2]) for r in rows))) for rows in EXPECT.values())
    held = {(e, label) for label, rows in EXPECT.items() for _, _, entries in rows for e in members(entries)}
    assert asked == held
