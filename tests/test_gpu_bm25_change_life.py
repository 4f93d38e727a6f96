"""One scripted life of a tiny BM25 index, plain and positional: build, appends that find room, that re-hash the term table, that
re-hash the pair table and grow the entries, a removal that leaves dead terms, an append that revives one, a compaction and an
append behind it.  After every step the index answers like a fresh build of the same documents and like a plain Python count, and
its gz_bm25_footprint equals FOOT: the triples the library gave before its three staging helpers became one function with a
three-valued size rule.  The footprint is a function of the buffers' capacities alone, so the equality is exact: the staging sizes
did not move.  SWEEP_K holds, for three of the steps, the first inject_bad_alloc count at which the call succeeds: its allocation
sites + 1.

Every device buffer is a multiple of 4 KiB (ensure() in gz_api.cpp adds 256 bytes and rounds up), so on an index this small most
buffers have room for an append although the build sized them exactly: test_the_footprints_show_the_branches says which step takes
which branch of the staging rule, by the same arithmetic."""
import numpy as np
import pytest

import bm25_restate as R
import bm25_tiny as tiny
from genz_tokenize import _native
from genz_tokenize._packing import pack

KINDS = ["plain", "pos"]
QUERIES = ["w0 w3", "n3 w11 absent", "f1 w5 w5", "n0 n21"]
ABSENT = "absent"


def bm_pow2(x):
    p = 16
    while p < x:
        p <<= 1
    return p


def remaining(docs, ids):
    gone = set(ids)
    return [d for i, d in enumerate(docs) if i not in gone]


def script():
    """[(what, "append" | "remove" | "compact", documents or ids)] behind the build of tiny.documents()"""
    new_words = [["n%d" % (8 * j + k) for k in range(8 if j < 2 else 6)] for j in range(3)]              # 22 new words
    wide = [" ".join(tiny.VOCAB[(j * (k + 1) + k) % 12] for k in range(5)) for j in range(70)]           # 350 known words
    n = tiny.N_DOCS + 1 + 1 + 3 + 70
    gone = sorted(set(range(0, n, 3)) | {tiny.N_DOCS + 2, tiny.N_DOCS + 3, tiny.N_DOCS + 4})             # a third, and all of step 4
    return [("2 append", "append", ["w0 w1 w2"]),
            ("3 append", "append", ["w3 w4"]),
            ("4 term table re-hash", "append", [" ".join(w) for w in new_words]),
            ("5 pair table re-hash", "append", wide),
            ("6 remove", "remove", gone),
            ("7 revive", "append", ["n3 w0 n3"]),
            ("8 compact", "compact", None),
            ("9 append", "append", ["w5 f1", "", "f1 f2 w0"])]


def py_vocab(docs):
    """(words in the order of their first occurrence, documents that contain each)"""
    df = {}
    for d in docs:
        for w in dict.fromkeys(d.split()):
            df[w] = df.get(w, 0) + 1
    return list(df), list(df.values())


ALL_WORDS = sorted({w for d in tiny.documents() for w in d.split()} |
                   {w for _, op, arg in script() if op == "append" for d in arg for w in d.split()}) + [ABSENT]

# gz_bm25_footprint (text bytes, terms held, device bytes) after the build and after every step of script()
FOOT = {
    "plain": [(1720, 12, 61440), (1728, 12, 61440), (1733, 12, 61440), (1808, 34, 65536), (2860, 34, 122880), (2860, 34, 122880),
              (2868, 34, 122880), (28, 13, 61440), (41, 15, 61440)],
    "pos": [(26, 12, 65536), (34, 12, 65536), (39, 12, 65536), (114, 34, 69632), (1166, 34, 126976), (1166, 34, 126976),
            (1174, 34, 126976), (28, 13, 65536), (41, 15, 65536)],
}
# the first inject_bad_alloc count at which the step succeeds
SWEEP_K = {
    "plain": {"4 term table re-hash": 26, "6 remove": 14, "8 compact": 20},
    "pos": {"4 term table re-hash": 26, "6 remove": 18, "8 compact": 21},
}


def test_the_script_crosses_every_threshold():
    """the arithmetic of bm25_build_core / bm25_append_core on the host: which step re-hashes which table"""
    docs = tiny.documents()
    T, W, E = len(py_vocab(docs)[0]), sum(len(d.split()) for d in docs), sum(len(set(d.split())) for d in docs)
    assert (T, W, E) == (12, 583, 410)
    tslots, pslots = bm_pow2(2 * T + 16), bm_pow2(W + W // 3 + 16)
    assert (tslots, pslots) == (64, 1024)
    table = set(py_vocab(docs)[0])                                                      # the term table: dead terms stay in it
    rehashed, revived = [], []
    for what, op, arg in script():
        if op == "append":
            words = {w for d in arg for w in d.split()}
            revived += [(what, w) for w in sorted(words & table - set(py_vocab(docs)[0]))]
            table |= words
            T1, P1 = len(table), E + sum(len(d.split()) for d in arg)
            if 2 * T1 > tslots:
                tslots = bm_pow2(4 * T1 + 16)
                rehashed.append((what, "terms"))
            if P1 + P1 // 3 + 16 > pslots:
                pslots = bm_pow2(2 * (P1 + P1 // 3) + 16)
                rehashed.append((what, "pairs"))
            docs = docs + arg
        elif op == "remove":
            assert len(arg) > len(docs) // 3 and all(0 <= i < len(docs) for i in arg)
            docs = remaining(docs, arg)
            assert len(table - set(py_vocab(docs)[0])) == 22                            # the whole new-word batch went: dead terms
        else:
            table, W = set(py_vocab(docs)[0]), sum(len(d.split()) for d in docs)
            tslots, pslots = bm_pow2(2 * len(table) + 16), bm_pow2(W + W // 3 + 16)
        E = sum(len(set(d.split())) for d in docs)
    assert rehashed == [("4 term table re-hash", "terms"), ("5 pair table re-hash", "pairs")]
    assert revived == [("7 revive", "n3")]


def cap(need):
    """ensure(): the capacity of a buffer allocated for `need` bytes"""
    return (max(need, 16) + 256 + 4095) // 4096 * 4096


def test_the_footprints_show_the_branches():
    for kind in KINDS:
        f = [x[2] for x in FOOT[kind]]
        # 2, 3 -- room: the live buffers have it, nothing is staged
        assert f[2] == f[1] == f[0] and FOOT[kind][2][0] > FOOT[kind][1][0] > FOOT[kind][0][0]
        # 4 -- exact: the term table from 64 to bm_pow2(4 * 34 + 16) slots of 16 bytes
        assert f[3] - f[2] == cap(256 * 16) - cap(64 * 16)
        # 5 -- exact: the pair table from 1024 to bm_pow2(2 * (P1 + P1 / 3) + 16) = 4096 slots; grow: the entries, 410 + 27 of them
        # in one 4 KiB buffer, need P1 = 787 of 8 bytes and get twice the capacity
        P1 = 410 + 3 + 2 + 22 + 350
        assert bm_pow2(2 * (P1 + P1 // 3) + 16) == 4096 and cap(P1 * 8) > cap(437 * 8) == 4096
        assert f[4] - f[3] == cap(4096 * 16) - cap(1024 * 16) + cap(max(P1 * 8, 2 * 4096)) - 4096
        # 6 -- same capacity: a removal keeps every capacity, the text and the dead terms; 7 -- room again
        assert f[6] == f[5] == f[4] and FOOT[kind][5][:2] == FOOT[kind][4][:2]
        # 8 -- exact: a compaction gives everything back, the 21 dead terms included; 9 -- room
        assert f[8] == f[7] == f[0] and FOOT[kind][7][1] == FOOT[kind][6][1] - 21


class Life:
    def __init__(self, kind, ctx=None):
        self.kind, self.pos = kind, kind == "pos"
        self.ctx = ctx or _native.Context()
        self.docs = tiny.documents()
        self.index = self.build(self.docs)
        self.canonical = True                                               # term ids equal a fresh build's

    def build(self, docs):
        buf, off = pack(docs)
        return self.ctx.bm25_build(buf, off, positions=self.pos)

    def call(self, op, arg):
        """the C call of a step; the documents follow only when it returns"""
        if op == "append":
            buf, off = pack(arg)
            self.ctx.bm25_append(self.index, buf, off)
            self.docs = self.docs + arg
        elif op == "remove":
            self.ctx.bm25_remove(self.index, np.array(arg, np.int64))
            self.docs, self.canonical = remaining(self.docs, arg), False
        else:
            self.ctx.bm25_compact(self.index)
            self.canonical = True

    def footprint(self):
        return tuple(self.ctx.bm25_footprint(self.index))

    def answers(self, index, full=True):
        """what the C face answers, term ids left out: info, fieldLens, per word (absent, df), the vocabulary, score bits and top-k
        of QUERIES; full: one search and -- a positional index -- the sequence as words, both of which leave derived buffers behind"""
        ctx = self.ctx
        wb, wo = pack(ALL_WORDS)
        ids, df = ctx.bm25_lookup(index, wb, wo)
        qw = [w for q in QUERIES for w in q.split()]
        qoff = np.array([0] + list(np.cumsum([len(q.split()) for q in QUERIES])), np.int64)
        qb, qo = pack(qw)
        terms, qdf = ctx.bm25_lookup(index, qb, qo)
        n = ctx.bm25_info(index)[0]
        idf = np.array([R.idf(n, int(x)) for x in qdf])
        lens = ctx.bm25_field_lengths(index)
        params = [2.2, 1.2, 0.25, 0.75, float(np.mean(lens)), 0.0]
        scores = ctx.bm25_score(index, terms, idf, qoff, params, False)
        topk = ctx.bm25_topk(index, terms, idf, qoff, params, False, 7)
        off, data, vdf = ctx.bm25_terms(index)
        raw = data.tobytes()
        vocab = [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]
        out = [ctx.bm25_info(index), lens.tolist(), (ids == -1).tolist(), df.tolist(), (vocab, vdf.tolist()),
               scores.view(np.uint64).tolist(), topk[0].tolist(), topk[1].view(np.uint64).tolist()]
        if full:
            found = ctx.bm25_search(index, terms, idf, qoff, params, False, 5)
            out += [found[0].tolist(), found[1].view(np.uint64).tolist(), found[2].tolist()]
            if self.pos:
                word = {int(t): w for t, w in zip(ids, ALL_WORDS) if t >= 0}
                seq, soff = ctx.bm25_sequence(index)
                out += [[word[int(t)] for t in seq], soff.tolist()]
        return out, ids.tolist()

    def check(self, what):
        docs, ctx = self.docs, self.ctx
        got, ids = self.answers(self.index)
        fresh = self.build(docs)
        want, want_ids = self.answers(fresh)
        ctx.bm25_destroy(fresh)
        assert got == want, what
        if self.canonical:
            assert ids == want_ids, what
        # and a plain count
        vocab = py_vocab(docs)
        lens = [len(d.split()) for d in docs]
        assert got[0] == (len(docs), len(vocab[0]), sum(lens)) and got[1] == lens and got[4] == vocab, what
        df = dict(zip(*vocab))
        assert got[2] == [w not in df for w in ALL_WORDS] and got[3] == [df.get(w, 0) for w in ALL_WORDS], what
        if self.pos:
            assert got[-2] == [w for d in docs for w in d.split()] and got[-1] == [0] + list(np.cumsum(lens)), what
        return got

    def close(self):
        self.ctx.bm25_destroy(self.index)
        self.ctx.close()


def live(kind, sweep=""):
    """the life: (the footprint after the build and after every step, the first inject_bad_alloc count at which each step whose
    number is in `sweep` succeeds).  Such a step fails at every allocation site in turn first, and leaves the index as it was."""
    life = Life(kind)
    ctx = life.ctx
    feet, ks = [life.footprint()], {}
    life.check("1 build")
    for what, op, arg in script():
        if what[0] in sweep:
            before = (life.answers(life.index, full=False), life.footprint())
            for k in range(1, 200):
                _native.debug_set("inject_bad_alloc", k, ctx)
                try:
                    life.call(op, arg)
                except _native.GzError as e:
                    _native.debug_set("inject_bad_alloc", 0, ctx)
                    assert e.code == _native.GZ_E_NOMEM, (what, k, e)
                    assert (life.answers(life.index, full=False), life.footprint()) == before, (what, k)
                    continue
                _native.debug_set("inject_bad_alloc", 0, ctx)
                ks[what] = k
                break
            assert what in ks, what
        else:
            life.call(op, arg)
        feet.append(life.footprint())                                       # (before the checks derive postings and word offsets)
        life.check(what)
    life.close()
    return feet, ks


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_life(kind):
    feet, _ = live(kind)
    print("FOOT[%r] = %r" % (kind, feet))
    assert feet == FOOT.get(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_life_under_allocation_failures(kind):
    feet, ks = live(kind, sweep="468")
    print("SWEEP_K[%r] = %r" % (kind, ks))
    assert feet == FOOT.get(kind)                                           # the first success is the un-injected step
    assert ks == SWEEP_K.get(kind)
