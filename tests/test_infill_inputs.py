"""CPU-only: the span-corruption rule of tests/infill_oracle.py against a cell-by-cell restatement written a second way (the "some
start begins a span that covers my word" form, Philox with Python ints), its slicing identity, its counting identities, the way back
from (E, T) to the row, its end cases, and the realised share of chosen cells against the exact expectation per word ordinal."""
import numpy as np
import pytest

import infill_oracle as IO
import mask_oracle as MO
from conftest import DATA

PAD, BOS, EOS, MASK, UNK = 0, 1, 2, 3, 4
ONE = 2 ** 32


@pytest.fixture(scope="module")
def cont():
    return MO.continuation_ids(DATA + "/vocab.txt")


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


def infill_by_cells(ids, cont, mask_id, seed, t_start, len_t, n_len, whole_word, row_base, ignore, W):
    """the rule cell by cell: the spans of a row as (first ordinal, one past the last), a cell chosen when its word's ordinal lies
    in one of them; then E and T written into padded lists"""
    cont = set(int(x) for x in cont)
    prot_ids = {PAD, BOS, EOS, mask_id}
    out = {k: [] for k in IO.KEYS}
    for r, row in enumerate(ids):
        L = len(row)
        spans, ordinal, word_open, ordinals = [], 0, False, []
        for c, v in enumerate(row):
            if v in prot_ids:
                word_open = False
                ordinals.append(None)
                continue
            if not (whole_word and word_open):                       # a start
                ordinal += 1
                x = philox_scalar((row_base + r) * L + c, seed)
                if x[0] < t_start:
                    spans.append((ordinal, ordinal + 1 + sum(1 for k in range(n_len - 1) if x[1] >= len_t[k])))
            word_open = v in cont
            ordinals.append(ordinal)
        chosen = [o is not None and any(a <= o < b for a, b in spans) for o in ordinals]
        E, T, runs = [], [], 0
        for c, v in enumerate(row):
            if chosen[c]:
                if c == 0 or not chosen[c - 1]:
                    runs += 1
                    E.append(mask_id)
                    T.append(mask_id)
                T.append(v)
            elif v != PAD:
                E.append(v)
        T.append(EOS)
        D = [BOS] + T[:-1]
        out["input_ids"].append(E + [PAD] * (L - len(E)))
        out["attention_mask"].append([1] * len(E) + [0] * (L - len(E)))
        out["labels"].append((T + [ignore] * W)[:W])
        out["decoder_input_ids"].append((D + [PAD] * W)[:W])
        out["enc_len"].append(len(E)); out["dec_len"].append(len(T)); out["n_spans"].append(runs)
    return out


def random_rows(rng, cont, R, L, specials=(PAD, BOS, EOS, MASK, -1, 60000, 2 ** 31 - 1)):
    pick = rng.random((R, L))
    ids = np.where(pick < 0.45, rng.choice(cont, (R, L)), rng.integers(5, 48000, (R, L)))
    ids = np.where(pick > 0.9, rng.choice(list(specials), (R, L)), ids)
    return ids.astype(np.int64)


RULES = ((ONE // 3, [ONE // 4, ONE // 2, ONE // 2, ONE - 1], 5), (ONE // 10, [0] * 15, 16), (ONE, [], 1), (0, [5], 2), (ONE // 2, [ONE, ONE], 3))


@pytest.mark.parametrize("whole_word", [True, False])
def test_oracle_against_a_cell_by_cell_loop(cont, whole_word):
    rng = np.random.default_rng(3)
    for R, L, base, seed in ((7, 33, 0, 0), (3, 5, 2 ** 32 // 5 - 1, 0xDEADBEEF12345678), (4, 64, 2 ** 62 // 64, 9), (1, 1, 5, 1), (20, 2, 0, 2)):
        ids = random_rows(rng, cont, R, L)
        for (t_start, len_t, n_len), W in zip(RULES, (L, 1, L + 2, max(1, L // 2), 3)):
            got = IO.infill(ids, cont, PAD, BOS, EOS, MASK, seed=seed, t_start=t_start, len_t=len_t, n_len=n_len, whole_word=whole_word,
                            row_base=base, ignore_index=-7, dec_width=W)
            want = infill_by_cells(ids.tolist(), cont, MASK, seed, t_start, len_t, n_len, whole_word, base, -7, W)
            for k in IO.KEYS:
                assert got[k].dtype == np.int32 and got[k].tolist() == want[k], (k, R, L, n_len)


def test_slices_with_row_base_are_the_slices_of_the_batch(cont):
    rng = np.random.default_rng(4)
    ids = random_rows(rng, cont, 30, 17)
    kw = dict(seed=77, t_start=ONE // 4, len_t=[ONE // 3, ONE // 3 * 2], n_len=3, dec_width=9)
    whole = IO.infill(ids, cont, PAD, BOS, EOS, MASK, row_base=11, **kw)
    for a, b in ((0, 1), (1, 7), (7, 30), (30, 30)):
        part = IO.infill(ids[a:b], cont, PAD, BOS, EOS, MASK, row_base=11 + a, **kw)
        for k in IO.KEYS:
            assert np.array_equal(part[k], whole[k][a:b]), (k, a, b)
    other = IO.infill(ids, cont, PAD, BOS, EOS, MASK, row_base=12, **kw)
    assert not np.array_equal(other["labels"], whole["labels"])


@pytest.mark.parametrize("whole_word", [True, False])
def test_counts_and_the_way_back_to_the_row(cont, whole_word):
    """dec_len == n_chosen + n_spans + 1; enc_len + n_chosen - n_spans == non-pad cells; E with every <mask> replaced by the
    matching piece of T is the row without its pads (rows without a <mask> of their own, so that every <mask> of E is a run's)"""
    rng = np.random.default_rng(5)
    ids = random_rows(rng, cont, 40, 50, specials=(PAD, BOS, EOS, -1, 60000))
    for t_start, len_t, n_len in RULES:
        kw = dict(seed=8, t_start=t_start, len_t=len_t, n_len=n_len, whole_word=whole_word, row_base=3)
        _, _, _, chosen = IO.chosen_cells(ids, cont, (PAD, BOS, EOS, MASK), 8, t_start, len_t, n_len, whole_word, 3)
        got = IO.infill(ids, cont, PAD, BOS, EOS, MASK, dec_width=52, **kw)
        n_chosen = chosen.sum(axis=1)
        assert np.array_equal(got["dec_len"], n_chosen + got["n_spans"] + 1)
        assert np.array_equal(got["enc_len"] + n_chosen - got["n_spans"], (ids != PAD).sum(axis=1))
        assert (got["dec_len"] <= 52).all()
        for r in range(len(ids)):
            E = got["input_ids"][r, :got["enc_len"][r]].tolist()
            T = got["labels"][r, :got["dec_len"][r]].tolist()
            assert T[-1] == EOS and got["decoder_input_ids"][r, :got["dec_len"][r]].tolist() == [BOS] + T[:-1]
            assert (got["labels"][r, got["dec_len"][r]:] == -100).all() and (got["decoder_input_ids"][r, got["dec_len"][r]:] == PAD).all()
            assert got["attention_mask"][r].tolist() == [1] * len(E) + [0] * (50 - len(E))
            pieces, body = [], T[:-1]
            for v in body:
                if v == MASK:
                    pieces.append([])
                else:
                    pieces[-1].append(v)
            assert len(pieces) == got["n_spans"][r] and all(pieces)
            back, k = [], 0
            for v in E:
                if v == MASK:
                    back += pieces[k]
                    k += 1
                else:
                    back.append(v)
            assert k == len(pieces) and back == [v for v in ids[r].tolist() if v != PAD]
    if whole_word:                                                   # all of a word or nothing of it
        prot, head = MO.heads(ids, cont, (PAD, BOS, EOS, MASK), True)
        _, _, _, chosen = IO.chosen_cells(ids, cont, (PAD, BOS, EOS, MASK), 8, ONE // 3, [ONE // 2], 2, True, 3)
        assert np.array_equal(chosen[~prot], np.take_along_axis(chosen, np.maximum(head, 0), axis=1)[~prot]) and chosen.any() and not chosen[~prot].all()


def test_end_cases(cont):
    c, d = (int(v) for v in cont[:2])
    x, y = (int(v) for v in np.setdiff1d(np.arange(5, 48000), cont)[:2])
    run = lambda ids, **kw: IO.infill(np.array(ids, dtype=np.int64), cont, PAD, BOS, EOS, MASK, **kw)    # noqa: E731
    row = [BOS, x, c, d, y, EOS, PAD, PAD]
    got = run([row], t_start=0, len_t=[5], n_len=2)                  # nothing chosen: the row, T = eos
    assert got["input_ids"].tolist() == [row] and got["labels"][0].tolist() == [EOS] + [-100] * 7
    assert got["decoder_input_ids"][0].tolist() == [BOS] + [PAD] * 7
    assert (got["enc_len"][0], got["dec_len"][0], got["n_spans"][0]) == (6, 1, 0)
    got = run([row], t_start=ONE, n_len=1)                           # every word begins a span of one word: one run
    assert got["input_ids"][0].tolist() == [BOS, MASK, EOS] + [PAD] * 5 and got["attention_mask"][0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert got["labels"][0].tolist() == [MASK, x, c, d, y, EOS, -100, -100]
    assert got["decoder_input_ids"][0].tolist() == [BOS, MASK, x, c, d, y, PAD, PAD]
    assert (got["enc_len"][0], got["dec_len"][0], got["n_spans"][0]) == (3, 6, 1)
    got = run([[PAD] * 5], t_start=ONE, n_len=1)                     # an all-pad row
    assert got["input_ids"].tolist() == [[PAD] * 5] and not got["attention_mask"].any()
    assert got["labels"][0].tolist() == [EOS, -100, -100, -100, -100] and got["decoder_input_ids"][0].tolist() == [BOS, PAD, PAD, PAD, PAD]
    assert (got["enc_len"][0], got["dec_len"][0], got["n_spans"][0]) == (0, 1, 0)
    got = run([[x, PAD, y, PAD, PAD, x]], t_start=0, n_len=1)        # a pad in mid-row drops out and the row closes up
    assert got["input_ids"][0].tolist() == [x, y, x, PAD, PAD, PAD] and got["enc_len"][0] == 3
    got = run([[x, PAD, y, c, PAD, x]], t_start=ONE, n_len=1)        # ... and splits runs
    assert got["input_ids"][0].tolist() == [MASK, MASK, MASK, PAD, PAD, PAD] and got["n_spans"][0] == 3
    assert got["labels"][0].tolist() == [MASK, x, MASK, y, c, MASK] and got["dec_len"][0] == 8
    for v, e, t in ((x, [MASK], [MASK]), (PAD, [PAD], [EOS]), (EOS, [EOS], [EOS])):      # row_len = 1
        got = run([[v]], t_start=ONE, n_len=1)
        assert got["input_ids"].tolist() == [e] and got["labels"].tolist() == [t] and got["decoder_input_ids"].tolist() == [[BOS]]
    # a span counts across a protected cell: two words, <mask> between them, one span of two words -> two runs
    seed = next(s for s in range(64) if int(MO.draw(0, s)[0]) < ONE // 2 <= int(MO.draw(2, s)[0]))
    got = run([[x, MASK, y, x]], seed=seed, t_start=ONE // 2, len_t=[0], n_len=2)
    assert got["input_ids"][0].tolist()[:3] == [MASK, MASK, MASK] and got["n_spans"][0] == 2 and got["labels"][0].tolist()[:4] == [MASK, x, MASK, y]


@pytest.mark.parametrize("W", [9, 10, 11])
def test_nine_cells_overflow_the_decoder_width(cont, W):
    """nine unprotected cells, whole_word = 0, t_start = 2^32: len(T) = 11 = row_len + 2"""
    ids = np.arange(100, 109, dtype=np.int64)[None, :]
    got = IO.infill(ids, cont, PAD, BOS, EOS, MASK, t_start=ONE, n_len=1, whole_word=False, dec_width=W)
    T = [MASK] + list(range(100, 109)) + [EOS]
    assert got["dec_len"].tolist() == [11] and got["n_spans"].tolist() == [1] and got["enc_len"].tolist() == [1]
    assert got["labels"].shape == (1, W) and got["labels"][0].tolist() == T[:W]
    assert got["decoder_input_ids"][0].tolist() == ([BOS] + T[:-1])[:W]
    assert got["input_ids"][0].tolist() == [MASK] + [PAD] * 8


def word_rows(rng, cont, R, L):
    """framed rows of real-looking words: bos, words of 1 .. 4 pieces, eos, pad"""
    ids = np.full((R, L), PAD, dtype=np.int64)
    plain = np.setdiff1d(np.arange(5, 48000), cont)
    for r in range(R):
        n = int(rng.integers(L // 2, L - 1))
        body = np.where(rng.random(n) < 0.4, rng.choice(cont, n), rng.choice(plain, n))
        ids[r, 0], ids[r, 1:n + 1], ids[r, n + 1] = BOS, body, EOS
    return ids


def share_and_expectation(ids, cont, seed, t_start, len_t, n_len):
    prot, _, n, chosen = IO.chosen_cells(ids, cont, (PAD, BOS, EOS, MASK), seed, t_start, len_t, n_len, True, 0)
    q = t_start / ONE
    tail = [1.0] + [1.0 - t / ONE for t in len_t[:n_len - 1]]        # P(len > k) as the integers give it
    cov = np.array([0.0] + [IO.coverage(q, tail, m) for m in range(1, n_len + 1)])
    want = cov[np.minimum(n[~prot], n_len)].mean()
    return chosen[~prot].mean(), want


@pytest.mark.parametrize("lengths,mean_span,max_span", [("geometric", 3.0, 10), ("poisson", 3.0, 10), ("fixed", 3, 3)])
def test_realised_share_of_the_oracle(cont, lengths, mean_span, max_span):
    """2000 rows of 128 cells at p = 0.15: the chosen share of unprotected cells against the exact expectation, the coverage product
    with min(n, n_len) factors summed per word ordinal (0.1458 / 0.1462 / 0.1474 on these rows for the three laws: the first words of
    a row pull it below p).  Coverage of neighbouring words is correlated, so the margin is not binomial: over 20 seeds of the oracle
    the share's deviation from the expectation had mean 0.0002 / -0.0002 / -0.0006 and standard deviation 0.0022 / 0.0021 / 0.0019
    (largest deviation 0.0053 / 0.0056 / 0.0047; the shares ran from 0.143 to 0.152).  The margin is 0.011: five times the largest of
    the three standard deviations."""
    rng = np.random.default_rng(6)
    ids = word_rows(rng, cont, 2000, 128)
    t_start, len_t, n_len = IO.rule_ints(0.15, mean_span, max_span, lengths)
    devs = []
    for seed in range(20):
        got, want = share_and_expectation(ids, cont, seed, t_start, len_t, n_len)
        devs.append(got - want)
        assert abs(got - want) < 0.011, (seed, got, want)
    print("share: expectation %.4f, deviations over 20 seeds: std %.4f, max %.4f" % (want, np.std(devs), np.abs(devs).max()))
    assert 0.14 < want < 0.15 and abs(np.mean(devs)) < 0.011 / 4                     # (the mean of 20: a fifth of the spread and more)
