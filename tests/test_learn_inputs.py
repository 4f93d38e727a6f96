"""CPU-only: the BPE learner's rule as tests/learn_oracle.py states it -- the worked answer, the corpus on which reusing an existing
symbol's id changes a merge, a second restatement with incremental counts, the order of the vocab lines, the special pieces left
out, and CLOSURE: the tokenizer's loader and merge loop (oracle/gz_oracle.py, imported and not edited; the reference itself where
GZ_REFERENCE_CHECKOUT names its checkout) applied to the learnt files reproduce the learner's final segmentation of every training
word.  tests/test_gpu_learn.py holds the device to this oracle byte for byte."""
import importlib.util
import os
import random

import pytest

import gz_oracle as O
import learn_oracle as LO

KNOWN = {"aaaa": 1, "aaaaa": 2, "ab": 3, "abab": 1, "b": 5}
INTERNING = {'/a<w/w//>/w': 1, '</>w</w>w/>>>aa': 2, 'a//<w>/<w': 3}
ALPHABET = ["a", "b", "c", "ệ", "ô", "😀", "<", "/", "w", ">", "@", "_"]


def _corpus(seed):
    r = random.Random(seed)
    n_words = r.randint(1, 14)
    words = {}
    while len(words) < n_words:
        words["".join(r.choice(ALPHABET[:r.choice([2, 4, 12])]) for _ in range(r.randint(1, 9)))] = r.randint(1, 6)
    return list(words), list(words.values()), r.randint(0, 40), r.choice([1, 1, 2, 3])


def test_known_answer():
    t = LO.learn(list(KNOWN), list(KNOWN.values()), 10, 2)
    assert t.codes == b"#version: 0.2\na a\na b</w>\naa a</w>\naa aaa</w>\n"
    assert t.vocab == b"b 5\nab 4\na@@ 2\naaaaa 2\na 1\naa@@ 1\nb@@ 1\n"
    # step 3 is a tie at count 2 between (aa, aa) and (aa, a</w>): a</w> has id 1, aa has id 4
    assert t.merges[2] == ("aa", "a</w>")
    assert t.segmentation("aaaa") == ["aa", "a", "a</w>"] and t.segmentation("aaaaa") == ["aaaaa</w>"]
    assert t.n_symbols == 4 + 4                                  # a, a</w>, b, b</w> and four merged symbols


def test_self_overlaps_merge_left_to_right():
    # (the last code point is the symbol a</w>: a word of k letters holds k - 1 symbols a)
    assert LO.learn(["aaaa"], [1], 1, 1).segs == [["aa", "a", "a</w>"]]
    assert LO.learn(["aaaaa"], [1], 1, 1).segs == [["aa", "aa", "a</w>"]]
    assert LO.learn(["aaaaaa"], [1], 1, 1).segs == [["aa", "aa", "a", "a</w>"]]
    assert LO.learn(["aaa", "aaaa"], [1, 1], 1, 1).merges == [("a", "a")]          # n(a, a) = 1 + 2: "a a a" counts it twice
    assert LO.learn(["ababa"], [1], 1, 1).segs == [["ab", "ab", "a</w>"]]


def test_interning_corpus_differs_at_merge_17():
    words, counts = list(INTERNING), list(INTERNING.values())
    with_reuse = LO.learn(words, counts, 30, 1)
    without = LO.learn(words, counts, 30, 1, reuse=False)
    assert with_reuse.merges[:16] == without.merges[:16]
    assert with_reuse.merges[16] == ("w</w>", "w/>")
    assert without.merges[16] == ("</>", "w</w>")


@pytest.mark.parametrize("seed", range(40))
def test_incremental_counts_equal_the_full_recount(seed):
    words, counts, n, f = _corpus(seed)
    a, b = LO.learn(words, counts, n, f), LO.learn_incremental(words, counts, n, f)
    assert (a.codes, a.vocab, a.merges, a.segs, a.n_symbols) == (b.codes, b.vocab, b.merges, b.segs, b.n_symbols)
    c = LO.learn_indexed(words, counts, n, f)                    # (the restatement tools/learn_bench.py times)
    assert (a.codes, a.vocab, a.merges, a.segs, a.n_symbols) == (c.codes, c.vocab, c.merges, c.segs, c.n_symbols)


def _pieces(seg):
    return [s + "@@" for s in seg[:-1]] + [seg[-1][:-4]]


@pytest.mark.parametrize("seed", range(60))
def test_closure_under_the_oracles_loader_and_bpe(seed):
    words, counts, n, f = _corpus(1000 + seed)
    t = LO.learn(words, counts, n, f)
    tables = O.Tables(t.vocab, t.codes)
    for w, seg in zip(t.words, t.segs):
        assert O.bpe_pieces(w, tables.ranks) == _pieces(seg), (w, t.merges)
        if len(w) > 1:
            assert O.bpe_string(w, tables) == " ".join(_pieces(seg))
    # every piece of the final segmentation has an id of its own, unless it is a special string
    for seg in t.segs:
        for p in _pieces(seg):
            assert p in tables.encoder
            assert (tables.encoder[p] >= 5) == (p not in LO.SPECIALS)


def _reference():
    root = os.environ.get("GZ_REFERENCE_CHECKOUT")
    path = os.path.join(root, "genz_tokenize", "tokenize.py") if root else None
    if not path or not os.path.exists(path):
        pytest.skip("GZ_REFERENCE_CHECKOUT does not name a checkout of the reference")
    spec = importlib.util.spec_from_file_location("gz_reference_tokenize", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_closure_under_the_reference_itself(tmp_path):
    ref = _reference()
    for seed in range(60):
        words, counts, n, f = _corpus(2000 + seed)
        t = LO.learn(words, counts, n, f)
        v, c = tmp_path / ("vocab%d.txt" % seed), tmp_path / ("codes%d.txt" % seed)
        v.write_bytes(t.vocab)
        c.write_bytes(t.codes)
        tok = ref.Tokenize.fromFile(str(v), str(c))
        for w, seg in zip(t.words, t.segs):
            assert tok.bpe(w) == " ".join(_pieces(seg)), (seed, w)


def test_vocab_lines_largest_count_first_then_bytes():
    t = LO.learn(["ba", "ab", "é", "z", "ệ", "😀"], [2, 2, 2, 2, 2, 3], 0, 1)
    assert t.vocab.decode() == "😀 3\na 2\na@@ 2\nb 2\nb@@ 2\nz 2\né 2\nệ 2\n"
    for seed in range(20):
        words, counts, n, f = _corpus(3000 + seed)
        lines = LO.learn(words, counts, n, f).vocab.decode().splitlines()
        keys = [(-int(line.rsplit(" ", 1)[1]), line.rsplit(" ", 1)[0].encode()) for line in lines]
        assert keys == sorted(keys) and len(set(k[1] for k in keys)) == len(keys)
        assert t.codes.endswith(b"\n")


def test_finality_belongs_to_the_position():
    # "a@@" is the non-final piece of a, and the final piece of the word a@@ : one line, the counts added
    t = LO.learn(["ab", "a@@"], [3, 4], 10, 4)
    assert t.segs == [["a", "b</w>"], ["a@@</w>"]] and t.vocab == b"a@@ 7\nb 3\n"


def test_special_pieces_are_left_out():
    words = ["<s>", "<pad>", "</s>", "<mask>", "<unk>", "<s>x", "ab"]
    t = LO.learn(words, [9, 8, 7, 6, 5, 4, 3], 200, 1)
    assert t.vocab == b"<s>x 4\nab 3\n"
    tables = O.Tables(t.vocab, t.codes)
    assert [tables.encoder[s] for s in ("<pad>", "<s>", "</s>", "<mask>", "<unk>")] == [0, 1, 2, 3, 4]
    for w, seg in zip(t.words, t.segs):
        assert O.bpe_pieces(w, tables.ranks) == _pieces(seg)


def test_word_counts_is_first_occurrence_order():
    assert LO.word_counts(["b a b", "", " c\na　b "]) == (["b", "a", "c"], [3, 2, 1])
