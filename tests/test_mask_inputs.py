"""CPU-only: the masked-LM rule of tests/mask_oracle.py against the Philox4x32-10 known answers, the bundled vocabulary, a
cell-by-cell restatement written a second way, its own slicing identity and end cases, and -- through the reference's restatement
(oracle/gz_oracle.py) with offsets -- against the words of real texts."""
import numpy as np
import pytest

import mask_oracle as MO
from conftest import DATA

PAD, BOS, EOS, MASK, UNK = 0, 1, 2, 3, 4
ONE = 2 ** 32


def test_philox_known_answers():
    f = 0xFFFFFFFF
    for counter, key, want in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                               ((f, f, f, f), (f, f), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                               ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join("%08x" % int(x) for x in MO.philox4x32_10(counter, key)) == want
    # the cell form: counter (g lo, g hi, 0, 0), key (seed lo, seed hi), on arrays
    g, seed = (0x85A308D3 << 32) | 0x243F6A88, (0x299F31D0 << 32) | 0xA4093822
    x = MO.draw(np.array([g, 0], dtype=np.uint64), seed)
    y = MO.philox4x32_10((0x243F6A88, 0x85A308D3, 0, 0), (0xA4093822, 0x299F31D0))
    assert [int(v[0]) for v in x] == [int(v) for v in y]


@pytest.fixture(scope="module")
def cont():
    return MO.continuation_ids(DATA + "/vocab.txt")


def test_bundled_vocabulary_has_11281_continuation_ids(cont, oracle_tables):
    assert len(cont) == 11281 and cont.min() >= 5
    enc = oracle_tables.encoder
    assert sorted(i for w, i in enc.items() if w.endswith("@@")) == cont.tolist()        # the reference's numbering, line i -> 5 + i
    assert (enc["<pad>"], enc["<s>"], enc["</s>"], enc["<mask>"], enc["<unk>"]) == (PAD, BOS, EOS, MASK, UNK)


def mulhi(a, b):
    return (a * b) >> 32


def philox_scalar(g, seed):
    """Philox4x32-10 with Python ints, written apart from mask_oracle"""
    c = [g & 0xFFFFFFFF, g >> 32, 0, 0]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        lo0, hi0 = (0xD2511F53 * c[0]) & 0xFFFFFFFF, mulhi(0xD2511F53, c[0])
        lo1, hi1 = (0xCD9E8D57 * c[2]) & 0xFFFFFFFF, mulhi(0xCD9E8D57, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def mask_by_cells(ids, cont, mask_id, seed, t_sel, t1, t2, lo, hi, whole_word, row_base, ignore):
    """the rule cell by cell, walking each row once with the open word's decision in hand"""
    cont = set(int(x) for x in cont)
    prot_ids = {PAD, BOS, EOS, mask_id}
    R, L = len(ids), len(ids[0]) if len(ids) else 0
    out, lab, cnt = [], [], []
    for r in range(R):
        o, l, n = [], [], 0
        word_open, decision = False, False                           # the cell before continues a word; that word is chosen
        for c in range(L):
            v = int(ids[r][c])
            if v in prot_ids:
                o.append(v); l.append(ignore)
                word_open = False
                continue
            x = philox_scalar((row_base + r) * L + c, seed)
            if not (whole_word and word_open):
                decision = x[0] < t_sel
            word_open = v in cont
            if decision:
                n += 1
                l.append(v)
                o.append(mask_id if x[1] < t1 else lo + mulhi(x[2], hi - lo) if x[1] < t2 else v)
            else:
                o.append(v); l.append(ignore)
        out.append(o); lab.append(l); cnt.append(n)
    return out, lab, cnt


def random_rows(rng, cont, R, L):
    pick = rng.random((R, L))
    ids = np.where(pick < 0.45, rng.choice(cont, (R, L)), rng.integers(5, 48000, (R, L)))
    ids = np.where(pick > 0.9, rng.choice([PAD, BOS, EOS, MASK, -1, 60000, 2 ** 31 - 1], (R, L)), ids)
    return ids.astype(np.int64)


@pytest.mark.parametrize("whole_word", [True, False])
def test_oracle_against_a_cell_by_cell_loop(cont, whole_word):
    rng = np.random.default_rng(3)
    for R, L, base, seed in ((7, 33, 0, 0), (3, 5, 2 ** 32 // 5 - 1, 0xDEADBEEF12345678), (4, 64, 2 ** 62 // 64, 9), (1, 1, 5, 1), (20, 2, 0, 2)):
        ids = random_rows(rng, cont, R, L)
        for (p, mp, rp, lo, hi) in ((0.5, 0.8, 0.1, 5, 48423), (0.15, 0.3, 0.3, -40, -3), (1.0, 0.0, 1.0, 0, 2 ** 31 - 1)):
            t_sel, t1, t2 = MO.thresholds(p, mp, rp)
            got = MO.mask(ids, cont, PAD, BOS, EOS, MASK, seed=seed, t_sel=t_sel, t1=t1, t2=t2, rand_lo=lo, rand_hi=hi,
                          whole_word=whole_word, row_base=base, ignore_index=-100)
            out, lab, cnt = mask_by_cells(ids.tolist(), cont, MASK, seed, t_sel, t1, t2, lo, hi, whole_word, base, -100)
            assert got["input_ids"].tolist() == out and got["labels"].tolist() == lab and got["n_chosen"].tolist() == cnt


def test_slices_with_row_base_are_the_slices_of_the_batch(cont):
    rng = np.random.default_rng(4)
    ids = random_rows(rng, cont, 30, 17)
    kw = dict(seed=77, t_sel=ONE // 3, t1=ONE // 2, t2=ONE // 4 * 3, rand_lo=5, rand_hi=900)
    whole = MO.mask(ids, cont, PAD, BOS, EOS, MASK, row_base=11, **kw)
    for a, b in ((0, 1), (1, 7), (7, 30), (30, 30)):
        part = MO.mask(ids[a:b], cont, PAD, BOS, EOS, MASK, row_base=11 + a, **kw)
        for k in whole:
            assert np.array_equal(part[k], whole[k][a:b]), (k, a, b)
    other = MO.mask(ids, cont, PAD, BOS, EOS, MASK, row_base=12, **kw)
    assert not np.array_equal(other["labels"], whole["labels"])


def test_end_cases_of_the_thresholds(cont):
    rng = np.random.default_rng(5)
    ids = random_rows(rng, cont, 12, 40)
    real = ~np.isin(ids, [PAD, BOS, EOS, MASK])
    run = lambda p, mp, rp, **kw: MO.mask(ids, cont, PAD, BOS, EOS, MASK, seed=6, rand_lo=5, rand_hi=48423,          # noqa: E731
                                          **dict(zip(("t_sel", "t1", "t2"), MO.thresholds(p, mp, rp))), **kw)
    assert MO.thresholds(0.0, 1.0, 0.0) == (0, ONE, ONE) and MO.thresholds(1.0, 0.0, 1.0) == (ONE, 0, ONE)
    assert MO.thresholds(0.15, 0.8, 0.1) == (644245094, 3435973836, 3865470566)
    none = run(0.0, 0.8, 0.1)
    assert np.array_equal(none["input_ids"], ids) and (none["labels"] == -100).all() and not none["n_chosen"].any()
    for ww in (True, False):
        every = run(1.0, 0.8, 0.1, whole_word=ww)
        assert np.array_equal(every["labels"] != -100, real) and np.array_equal(every["labels"][real], ids[real])
        assert np.array_equal(every["n_chosen"], real.sum(axis=1)) and np.array_equal(every["input_ids"][~real], ids[~real])
    masks = run(1.0, 1.0, 0.0)
    assert (masks["input_ids"][real] == MASK).all()
    rand = run(1.0, 0.0, 1.0)
    assert ((rand["input_ids"][real] >= 5) & (rand["input_ids"][real] < 48423)).all() and len(np.unique(rand["input_ids"][real])) > 100
    keep = run(1.0, 0.0, 0.0)
    assert np.array_equal(keep["input_ids"], ids)
    other = run(0.5, 0.8, 0.1, ignore_index=-7)
    assert (other["labels"][~real] == -7).all()


# split words, a word whose last piece is unknown, unknown single tokens, texts of one word, an empty text
TEXTS = ["công nghệ thông tin và truyền thông", "internationalization antidisestablishmentarianism", "trăm中 phần trăm 中", "xin chào thế giới", "",
         "một hai ba bốn năm sáu bảy tám chín mười", "a", "hà nội là thủ đô của nước cộng hòa xã hội chủ nghĩa việt nam",
         "học máy và trí tuệ nhân tạo đang thay đổi thế giới", "tokenization subword segmentation"]
N_TEXTS, SEED = 60, 1                                                # chosen here, on the CPU: see test_chosen_share_of_words


@pytest.fixture(scope="module")
def encoded(oracle_tables):
    """[(ids with frame, word spans as (first, last) columns)] for N_TEXTS texts: TEXTS and rotations of their words"""
    import gz_oracle as O
    texts = list(TEXTS)
    k = 0
    while len(texts) < N_TEXTS:
        w = TEXTS[k % len(TEXTS)].split() + TEXTS[(k + 3) % len(TEXTS)].split()
        texts.append(" ".join(w[k % 5:] + w[:k % 5]))
        k += 1
    out = []
    for t in texts:
        r = O.call(oracle_tables, t, None, None, True, True, True)
        out.append((r["input_ids"], r["offset"][1:-1]))
    return out


def test_texts_hold_split_words_an_unknown_word_and_single_tokens(encoded, cont):
    spans = [b - a + 1 for _, sp in encoded for a, b in sp]
    assert max(spans) >= 5 and spans.count(1) > 50 and sum(n > 1 for n in spans) > 50
    ids = encoded[2][0]
    assert ids.count(UNK) == 2 and ids[ids.index(UNK) - 1] in set(cont.tolist())       # "trăm中": tr@@ ăm@@ <unk>
    for row, sp in encoded:                                          # the spans are the rule's words: starts at first, continuation up to last
        prot, head = MO.heads(np.array([row]), cont, (PAD, BOS, EOS, MASK), True)
        for a, b in sp:
            assert (head[0, a:b + 1] == a).all(), (row, a, b)


def words_of(encoded, cont, p, whole_word, seed, joined=False):
    """per word of every text: the chosen flags of its cells"""
    t_sel, t1, t2 = MO.thresholds(p)
    flags = []
    if joined:                                                       # all texts back to back in ONE row: eos bos separates them
        row, spans, at = [], [], 0
        for ids, sp in encoded:
            row += ids
            spans += [(a + at, b + at) for a, b in sp]
            at += len(ids)
        rows = [(row, spans)]
    else:
        rows = encoded
    for r, (ids, sp) in enumerate(rows):
        got = MO.mask(np.array([ids]), cont, PAD, BOS, EOS, MASK, seed=seed, t_sel=t_sel, t1=t1, t2=t2, rand_lo=5, rand_hi=48423,
                      whole_word=whole_word, row_base=r)
        picked = got["labels"][0] != -100
        assert not picked[np.isin(ids, [PAD, BOS, EOS, MASK])].any()
        flags += [picked[a:b + 1] for a, b in sp]
    return flags


@pytest.mark.parametrize("joined", [False, True])
def test_words_are_chosen_whole(encoded, cont, joined):
    for seed in range(3):
        flags = words_of(encoded, cont, 0.5, True, seed, joined)
        assert all(f.all() or not f.any() for f in flags)
        assert any(f.all() for f in flags) and any(not f.any() for f in flags)
        loose = words_of(encoded, cont, 0.5, False, seed, joined)
        assert any(f.any() and not f.all() for f in loose)           # without whole_word some word is split


def test_chosen_share_of_words(encoded, cont):
    """p = 0.15, one fixed seed: the chosen share of words within four binomial standard deviations of 0.15"""
    flags = words_of(encoded, cont, 0.15, True, SEED)
    n = len(flags)
    k = sum(bool(f[0]) for f in flags)
    sd = (0.15 * 0.85 / n) ** 0.5
    assert n > 500 and abs(k / n - 0.15) <= 4 * sd, (k, n, sd)


def test_product_thresholds_are_the_oracles():
    """Tokenize._mask_rule (a static method, no native call): the integers the library is given are the ones the oracle is given"""
    from genz_tokenize.tokenize import Tokenize
    for p, mp, rp in ((0.15, 0.8, 0.1), (0.0, 1.0, 0.0), (1.0, 0.0, 1.0), (0.5, 0.5, 0.5), (1 / 3, 0.7, 0.3), (1, 0, 0), (np.float32(0.25), 0.1, 0.2)):
        rule = Tokenize._mask_rule(p, 2 ** 64 - 1, True, mp, rp, None, 2 ** 63 - 1, -100)
        assert rule[1:4] == MO.thresholds(p, mp, rp) and all(type(v) is int for v in rule[:4])
        assert rule == (2 ** 64 - 1, *MO.thresholds(p, mp, rp), None, None, 1, -100, 2 ** 63 - 1)
    assert Tokenize._mask_rule(0.15, 0, False, 0.8, 0.1, (7, 8), 0, 5)[4:] == (7, 8, 0, 5, 0)
