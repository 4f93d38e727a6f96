"""GPU: genz_tokenize.learn_bpe / word_counts against tests/learn_oracle.py, byte for byte -- the stop rules, self-overlapping pairs,
the interning of a merged string that exists already, ties, code points of every width, every whitespace code point, words on the
lane path, the wave path and their boundary, counts beyond 2^32, a forced tiny pair table and a table that grows, and the closure
of the learnt files under the tokenizer itself."""
import collections
import random

import numpy as np
import pytest

import learn_oracle as LO

pytestmark = pytest.mark.gpu

KNOWN = {"aaaa": 1, "aaaaa": 2, "ab": 3, "abab": 1, "b": 5}
INTERNING = {'/a<w/w//>/w': 1, '</>w</w>w/>>>aa': 2, 'a//<w>/<w': 3}


@pytest.fixture(scope="module")
def L():
    from genz_tokenize import learn                              # (no skip: without the module every test here fails)
    return learn


def _docs(counts):
    """documents whose word multiset is `counts`"""
    return [" ".join([w] * c) for w, c in counts.items()]


def _same(t, want):
    assert t.codes == want.codes
    assert t.vocab == want.vocab
    assert t.merges == want.merges
    assert t.n_symbols == want.n_symbols and t.n_words == len(want.words)


def _check(L, docs, n_merges, min_frequency=2, **kw):
    t = L.learn_bpe(docs, n_merges=n_merges, min_frequency=min_frequency, **kw)
    want = LO.learn_documents(docs, n_merges, min_frequency)
    _same(t, want)
    return t, want


# ---- stop rules and trivial corpora -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("docs", [[], [""], ["  \n\t 　 "], ["a"], ["a", "a a"]], ids=["none", "empty", "whitespace", "one", "no_pairs"])
def test_nothing_to_merge(L, docs):
    t, _ = _check(L, docs, 10, 1)
    assert t.merges == [] and t.codes == b"#version: 0.2\n"
    w, c = L.word_counts(docs)
    assert (w, c.tolist()) == LO.word_counts(docs) and c.dtype == np.int64


def test_stop_rules(L):
    docs = _docs(KNOWN)
    t, _ = _check(L, docs, 0)
    assert t.merges == [] and t.vocab == LO.learn_documents(docs, 0).vocab != b""
    full, _ = _check(L, docs, 1000, 1)                           # beyond what exists: until no pair is left
    assert 0 < len(full.merges) < 1000
    for n in range(1, len(full.merges) + 1):
        _check(L, docs, n, 1)
    stopped, _ = _check(L, docs, 1000, 3)                        # min_frequency ends the run mid-way
    assert 0 < len(stopped.merges) < len(full.merges)
    assert len(_check(L, docs, 1000, 8)[0].merges) == 1          # n(a, a) = 2 + 2 * 3 = 8 is the largest count there is
    assert len(_check(L, docs, 1000, 9)[0].merges) == 0
    assert len(_check(L, docs, 1000, 2 ** 40)[0].merges) == 0


# ---- merge behaviour --------------------------------------------------------------------------------------------------------------
def test_known_answer(L):
    t = L.learn_bpe(_docs(KNOWN), n_merges=10, min_frequency=2)
    assert t.codes == b"#version: 0.2\na a\na b</w>\naa a</w>\naa aaa</w>\n"
    assert t.vocab == b"b 5\nab 4\na@@ 2\naaaaa 2\na 1\naa@@ 1\nb@@ 1\n"
    assert t.merges == [("a", "a"), ("a", "b</w>"), ("aa", "a</w>"), ("aa", "aaa</w>")]
    assert t.n_words == 5


@pytest.mark.parametrize("word", ["aaa", "aaaa", "aaaaa", "ababab", "abababa", "aaaaaaaaaaaaaaaaa"])
def test_self_overlaps(L, word):
    for extra in ([], ["aa ab ba"], ["a b"]):
        _check(L, [word, word] + extra, 20, 1)


def test_interning_reuses_the_existing_symbol(L):
    words, counts = list(INTERNING), list(INTERNING.values())
    want = LO.learn(words, counts, 30, 1)
    assert want.merges[16] == ("w</w>", "w/>")
    _same(L.learn_bpe(words=words, counts=counts, n_merges=30, min_frequency=1), want)
    _same(L.learn_bpe(_docs(INTERNING), n_merges=30, min_frequency=1), want)


def test_pieces_that_collide_and_special_pieces(L):
    # "a@@" is the non-final piece of a and the final piece of the word a@@: one vocab line; the five special strings get none
    t, want = _check(L, ["ab ab ab a@@ a@@ a@@ a@@"], 10, 4)
    assert want.segs == [["a", "b</w>"], ["a@@</w>"]] and t.vocab == b"a@@ 7\nb 3\n"
    t, _ = _check(L, ["<s> <s> <pad> </s> <mask> <unk> <unk> <s>x ab"], 200, 1)
    assert t.vocab == b"<s>x 1\nab 1\n"
    assert t.tokenizer()._special_ids() == [0, 1, 2, 3, 4]


def test_ties_everywhere(L):
    r = random.Random(3)
    letters = "abcdefghijklmnopqrstuvwxyz"
    words = [a + r.choice(letters) for a in letters]
    r.shuffle(words)
    t, _ = _check(L, [" ".join(words)], 100, 1)
    assert len(t.merges) == 26


# ---- code points and whitespace ---------------------------------------------------------------------------------------------------
def test_code_points_of_every_width(L):
    r = random.Random(5)
    alphabet = ["a", "b", "\x7f", "\x80", "é", "߿", "ࠀ", "ệ", "￿", "\U00010000", "😀", "\U0010ffff", "<", "/", "w", ">", "@", "_"]
    docs = [" ".join("".join(r.choice(alphabet) for _ in range(r.randint(1, 7))) for _ in range(r.randint(0, 9))) for _ in range(60)]
    _check(L, docs, 80, 1)
    _check(L, docs, 25, 2)


def test_every_whitespace_code_point_separates(L):
    import gz_oracle as O
    assert len(O.WHITESPACE) == 29
    for cp in sorted(O.WHITESPACE):
        ws = chr(cp)
        docs = [ws.join(["ab", "abc", "ab", "ệ😀"]), ws + "ab" + ws + ws + "b" + ws]
        assert docs[0].split() == ["ab", "abc", "ab", "ệ😀"], hex(cp)
        w, c = L.word_counts(docs)
        assert (w, c.tolist()) == (["ab", "abc", "ệ😀", "b"], [3, 1, 1, 1]), hex(cp)
        _check(L, docs, 10, 1)


def test_word_counts_is_a_counter_over_split(L):
    r = random.Random(7)
    alphabet = "ab ệ\n\t😀c 　 "
    docs = ["".join(r.choice(alphabet) for _ in range(r.choice([0, 1, 5, 63, 64, 65, 300]))) for _ in range(400)]
    want = collections.Counter(w for d in docs for w in d.split())
    w, c = L.word_counts(docs)
    assert w == list(want) and c.tolist() == list(want.values())
    packed = "".join(docs).encode("utf-8")
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d.encode("utf-8")) for d in docs], out=off[1:])
    data, woff, cnt = L.word_counts_packed(np.frombuffer(packed, np.uint8), off)
    assert [data.tobytes()[woff[i]:woff[i + 1]].decode() for i in range(len(cnt))] == w and cnt.tolist() == c.tolist()


# ---- sizes and edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 4096])
def test_word_lengths_on_the_lane_and_wave_paths(L, n):
    r = random.Random(n)
    shapes = ["a" * n, ("ab" * n)[:n], ("aab" * n)[:n], "".join(r.choice("abc") for _ in range(n)), "".join(r.choice("aệ😀") for _ in range(n))]
    docs = [" ".join(shapes), shapes[0] + " " + shapes[3], "ab ba aa abc"]
    _check(L, docs, 40 if n > 200 else 120, 1)


def test_counts_beyond_32_bits(L):
    words, counts = ["abab", "abb", "ba", "b"], [3 * 10 ** 9, 3 * 10 ** 9, 5, 2 ** 40]
    t = L.learn_bpe(words=words, counts=counts, n_merges=10, min_frequency=2 ** 31)
    _same(t, LO.learn(words, counts, 10, 2 ** 31))               # n(a, b) = 6 * 10^9 to begin with
    assert len(t.merges) >= 2
    # equal words add up
    t2 = L.learn_bpe(words=words + ["abab"], counts=counts + [1], n_merges=10, min_frequency=1)
    _same(t2, LO.learn(words, [counts[0] + 1] + counts[1:], 10, 1))


def _spread_corpus():
    """24 565 words of three symbols whose 49 130 adjacent pairs are all distinct: the table of 65 536 slots starts just under its
    load rule, and every merge adds a key"""
    words = []
    for n in range(24565):
        i, j = divmod(n, 157)
        words.append(chr(0x100 + i) + chr(0x400 + j) + chr(0x800 + i))
    return words


def test_the_table_grows(L):
    words = _spread_corpus()
    counts = [1] * len(words)
    t = L.learn_bpe(words=words, counts=counts, n_merges=30, min_frequency=1)
    assert t.info["table_growths"] >= 1 and t.info["table_slots"] > 65536
    _same(t, LO.learn_incremental(words, counts, 30, 1))


def test_tiny_forced_table_equals_the_normal_one(L):
    from genz_tokenize import _native
    r = random.Random(11)
    docs = [" ".join("".join(r.choice("abcdeệ😀") for _ in range(r.randint(1, 70))) for _ in range(8)) for _ in range(40)]
    normal, want = _check(L, docs, 150, 1)
    assert normal.info["table_growths"] == 0
    for bits in (1, 4, 7):
        ctx = _native.Context()
        try:
            _native.debug_set("learn_table_bits", bits, ctx)
            tiny = L.learn_bpe(docs, n_merges=150, min_frequency=1, ctx=ctx)
        finally:
            ctx.close()
        _same(tiny, want)
        assert tiny.info["table_growths"] >= 1 and tiny.info["table_slots"] < normal.info["table_slots"]
        assert tiny.info["table_keys"] == normal.info["table_keys"]


# ---- whole-call properties --------------------------------------------------------------------------------------------------------
def _seeded(seed, n_docs=120):
    r = random.Random(seed)
    alphabet = "aabbcệô😀</w>@_"
    return [" ".join("".join(r.choice(alphabet) for _ in range(r.randint(1, 9))) for _ in range(r.randint(0, 12))) for _ in range(n_docs)]


def test_same_call_same_bytes_and_document_order_does_not_matter(L):
    docs = _seeded(1)
    a, _ = _check(L, docs, 60)
    b = L.learn_bpe(docs, n_merges=60)
    assert (a.codes, a.vocab) == (b.codes, b.vocab)
    r = random.Random(2)
    shuffled = docs[:]
    r.shuffle(shuffled)
    c = L.learn_bpe(shuffled, n_merges=60)
    whole = " ".join(docs)
    recut = [whole[:len(whole) // 3].rsplit(" ", 1)[0]]
    recut.append(whole[len(recut[0]):])
    d = L.learn_bpe(recut, n_merges=60)
    assert (a.codes, a.vocab) == (c.codes, c.vocab) == (d.codes, d.vocab)


def test_shard_counts_added_on_the_host(L):
    docs = _seeded(4)
    total = collections.Counter()
    for lo in range(0, len(docs), 37):
        w, c = L.word_counts(docs[lo:lo + 37])
        total.update(dict(zip(w, c.tolist())))
    t = L.learn_bpe(words=list(total), counts=list(total.values()), n_merges=60)
    whole = L.learn_bpe(docs, n_merges=60)
    assert (t.codes, t.vocab, t.merges) == (whole.codes, whole.vocab, whole.merges)


def test_closure_on_the_device(L):
    """the tokenizer loaded with the learnt files cuts the corpus into exactly the pieces the vocab file counts"""
    r = random.Random(9)
    alphabet = "abcdeệô_"
    docs = [" ".join("".join(r.choice(alphabet) for _ in range(r.randint(1, 8))) for _ in range(r.randint(1, 15))) for _ in range(300)]
    t = L.learn_bpe(docs, n_merges=200)
    lines = t.vocab.decode().splitlines()
    want = {5 + i: int(line.rsplit(" ", 1)[1]) for i, line in enumerate(lines)}
    tok = t.tokenizer()
    out = tok.encode_batch(docs, max_len=None, padding=False, truncation=False)
    ids = np.asarray(out["input_ids"]).reshape(-1)
    got = collections.Counter(ids.tolist())
    for special in (0, 1, 2):
        got.pop(special, None)
    assert dict(got) == want
    # ... and word for word: bpe() of a training word is the learner's own segmentation of it
    o = LO.learn_documents(docs, 200)
    for w in o.words[:50]:
        seg = o.segmentation(w)
        assert tok.bpe(w).split(" ") == [s + "@@" for s in seg[:-1]] + [seg[-1][:-4]], w
