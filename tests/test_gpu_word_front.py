"""GPU: the word front that the BM25 build, the BM25 append and the word set share (count, scan, words, hash, de-duplication
rounds, first, scan), from outside.  One corpus whose word lengths sit on the tile edges of the count kernel goes through all three
under forced hash collisions: the word set in its host, device and counts forms against tests/learn_oracle.py, the index against
the word set, and an append of known and of new words behind it.  A sweep of inject_bad_alloc pins the number of allocation sites
of the two builds that no other test pins."""
import random

import numpy as np
import pytest

import learn_oracle as LO
from genz_tokenize import _native, learn
from genz_tokenize._packing import pack

gpu = pytest.mark.gpu

HASH_BITS = (1, 4, 0)           # 1 bit: two hash values, so about distinct / 2 de-duplication rounds; 0: the whole hash, one round


def _words():
    """60 distinct words: 1, 63, 64, 65 and 130 bytes in ASCII and in multi-byte code points, and short ones of both kinds"""
    w = list("abcdefghijklmn")                                                       # 14 of one byte
    for n in (63, 64, 65, 130):
        w += [(("%c%d-" % (c, n)) * n)[:n] for c in "pqrstu"]                        # 24, each of n bytes
    w += ["ệ" * 21, "😀" * 16, "ệ" * 21 + "ab", "😀" * 32 + "ab"]                    # 63, 64, 65 and 130 bytes
    w += ["ệ", "😀", "é", "éệ", "a😀"]
    w += ["ab", "ba", "abc", "sinh_viên", "công_nghệ", "x" * 7, "y" * 10, "<s>", "</w>", "@@", "1", "22", "333"]
    assert len(set(w)) == len(w) == 60
    assert {len(x.encode()) for x in w} >= {1, 63, 64, 65, 130}
    return w


def _corpus():
    """ten documents: eight of words (every word occurs, most of them more than once, within and across documents; every kind of
    separator), an empty one and one of whitespace only"""
    r = random.Random(17)
    words = _words()
    seps = [" ", "\n", "\t ", "　", "  "]
    docs = []
    for d in range(8):
        mine = words[d::8] + [r.choice(words) for _ in range(12)] + words[d::8][:3]
        r.shuffle(mine)
        docs.append("".join(x + r.choice(seps) for x in mine).rstrip(" ") if d % 2 else " " + " ".join(mine))
    docs.insert(3, "")
    docs.insert(7, " \n\t　 ")
    return docs


DOCS = _corpus()
WORDS, COUNTS = LO.word_counts(DOCS)                                                 # the reference: computed once, never changed


def test_the_corpus_is_what_the_tests_assume():
    assert len(DOCS) == 10 and len(WORDS) == 60 and set(WORDS) == set(_words())
    assert sum(COUNTS) == sum(len(d.split()) for d in DOCS) and max(COUNTS) > 1
    assert any(len(d.split()) != len(set(d.split())) for d in DOCS)                 # repeats within a document
    assert DOCS[3] == "" and DOCS[7] and DOCS[7].split() == []


class Switched:
    """a context of its own with bm25_hash_bits set; the switch is reset on the context and globally on the way out"""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        self.ctx = _native.Context()
        _native.debug_set("bm25_hash_bits", self.bits, self.ctx)
        return self.ctx

    def __exit__(self, *exc):
        try:
            _native.debug_set("bm25_hash_bits", 0, self.ctx)
            self.ctx.close()
        finally:
            _native.debug_set("bm25_hash_bits", 0)
        return False


def _read(ctx, ws):
    try:
        data, off, cnt = ctx.wordset_words(ws)
    finally:
        ctx.wordset_destroy(ws)
    raw = data.tobytes()
    return [raw[off[i]:off[i + 1]].decode("utf-8") for i in range(len(cnt))], cnt.tolist()


# ---- 1: the word set under forced collisions ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bits", HASH_BITS)
def test_word_set_host_form(bits):
    with Switched(bits) as ctx:
        w, c = learn.word_counts(DOCS, ctx=ctx)
        assert (w, c.tolist()) == (WORDS, COUNTS)


@gpu
@pytest.mark.parametrize("bits", HASH_BITS)
def test_word_set_device_form(bits):
    buf, off = pack(DOCS)
    with Switched(bits) as ctx:
        d_text, d_off = ctx.alloc(len(buf)), ctx.alloc(8 * len(off))
        try:
            ctx.h2d(d_text, buf)
            ctx.h2d(d_off, off)
            assert _read(ctx, ctx.wordset_build_device(d_text, d_off, len(DOCS), len(buf))) == (WORDS, COUNTS)
        finally:
            ctx.free(d_text)
            ctx.free(d_off)


@gpu
@pytest.mark.parametrize("bits", HASH_BITS)
def test_word_set_counts_form(bits):
    """every word given twice, the second time in reverse order and with another count: equal words add up"""
    words = WORDS + WORDS[::-1]
    counts = COUNTS + [3 * c + 1 for c in COUNTS[::-1]]
    want = [4 * c + 1 for c in COUNTS]
    buf, off = pack(words)
    with Switched(bits) as ctx:
        assert _read(ctx, ctx.wordset_from_counts(buf, off, np.array(counts, np.int64))) == (WORDS, want)
        t = learn.learn_bpe(words=words, counts=counts, n_merges=0, ctx=ctx)
        assert t.n_words == len(WORDS) and t.merges == []
        assert t.vocab == LO.learn(WORDS, want, 0).vocab


# ---- 2: one front, one answer ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bits", HASH_BITS)
def test_build_and_append_count_what_the_word_set_counts(bits):
    # 20 new words: more than the 2 or 16 hash values that 1 or 4 bits leave, so at least two of them share a hash in the append's
    # rounds; the first document repeats some of them, the second repeats some of the first's
    new = ["new%d" % i + "z" * (i % 3) for i in range(20)]
    more = [" ".join(new[:12] + new[:4]), " ".join(new[8:] + [new[0], new[19]])]
    assert not set(new) & set(WORDS) and len(set(new)) == 20
    with Switched(bits) as ctx:
        ix = ctx.bm25_build(*pack(DOCS))
        try:
            assert ctx.bm25_info(ix) == (len(DOCS), len(WORDS), sum(COUNTS))
            ctx.bm25_append(ix, *pack(DOCS))                                        # every word is known
            assert ctx.bm25_info(ix) == (2 * len(DOCS), len(WORDS), 2 * sum(COUNTS))
            ctx.bm25_append(ix, *pack(more))
            assert ctx.bm25_info(ix) == (2 * len(DOCS) + 2, len(WORDS) + 20, 2 * sum(COUNTS) + sum(len(d.split()) for d in more))
            # ... and the index names them as the word set of all of it does
            w, c = learn.word_counts(DOCS + DOCS + more, ctx=ctx)
            assert (w, c.tolist()) == LO.word_counts(DOCS + DOCS + more) and w == WORDS + new[:12] + new[12:]
            toff, data, _ = ctx.bm25_terms(ix)
            raw = data.tobytes()
            assert [raw[toff[i]:toff[i + 1]].decode() for i in range(len(toff) - 1)] == w
        finally:
            ctx.bm25_destroy(ix)


# ---- 3: allocation sites did not move ----------------------------------------------------------------------------------------------------
# The first inject_bad_alloc count at which the call succeeds on DOCS: its allocation sites + 1.  Recorded from the library as it
# was before the three copies of the word front became one (commit 3b3b1fc); the same test passes there.
SITES_K = {"bm25_build": 30, "bm25_build_positions": 50, "wordset_build": 25}


def _sweep(ctx, call):
    for k in range(1, 200):
        _native.debug_set("inject_bad_alloc", k, ctx)
        try:
            got = call()
        except _native.GzError as e:
            _native.debug_set("inject_bad_alloc", 0, ctx)
            assert e.code == _native.GZ_E_NOMEM, (k, e)
            # the context still works
            assert learn.word_counts(["b a b"], ctx=ctx)[1].tolist() == [2, 1], k
            continue
        _native.debug_set("inject_bad_alloc", 0, ctx)
        return k, got
    raise AssertionError("no success below 200 allocation sites")


@gpu
@pytest.mark.parametrize("what", sorted(SITES_K))
def test_allocation_sites_of_the_builds(what):
    buf, off = pack(DOCS)
    ctx = _native.Context()
    try:
        if what == "wordset_build":
            k, ws = _sweep(ctx, lambda: ctx.wordset_build(buf, off))
            assert _read(ctx, ws) == (WORDS, COUNTS)
        else:
            k, ix = _sweep(ctx, lambda: ctx.bm25_build(buf, off, positions=what.endswith("positions")))
            assert ctx.bm25_info(ix) == (len(DOCS), len(WORDS), sum(COUNTS))
            ctx.bm25_destroy(ix)
        print("SITES_K[%r] = %d" % (what, k))
        assert k == SITES_K[what]
    finally:
        _native.debug_set("inject_bad_alloc", 0, ctx)
        ctx.close()
