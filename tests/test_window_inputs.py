"""CPU-only: the window rule of tests/window_oracle.py against the reference's restatement (oracle/gz_oracle.py) on the
bundled tables, its window count against a count by hand, and the shape lists of the GPU tests against the cases they are
named for.  The three facts that tie the rule to the reference:
  1. window 0 of a text is Tokenize.__call__(text, max_len=L)'s row and mask (tokenize.py:141-152);
  2. chunk_0 ++ chunk_1[s:] ++ chunk_2[s:] ++ ... is encode(text)[1:-1];
  3. every window after the first adds at least one new token."""
import random

import pytest

import window_oracle as W

LS = [(L, s) for L in (3, 4, 5, 7, 10, 16) for s in sorted({0, min(1, L - 3), L - 3})]


@pytest.fixture(scope="module")
def encoded(oracle_tables):
    import gz_oracle as O
    r = random.Random(11)
    vocab = [w for w in list(oracle_tables.encoder)[5:4000:7] if " " not in w and w]
    texts = W.texts(200, 40, 3)
    for _ in range(200):                                             # vocabulary words, pieces of them, strings outside the tables
        words = []
        for _ in range(r.randint(0, 40)):
            w = r.choice(vocab).replace("@@", "")
            words.append(w if r.random() < 0.7 else w[:r.randint(1, len(w))] + r.choice(["", "x", "Q9", "中"]))
        texts.append(" ".join(words))
    return texts, [O.encode(t, oracle_tables) for t in texts]


def test_texts_cover_empty_short_and_long_bodies(encoded):
    _, enc = encoded
    lens = [len(e) - 2 for e in enc]
    assert min(lens) == 0 and max(lens) > 3 * 14 and len(enc) == 400


@pytest.mark.parametrize("L,s", LS)
def test_window_zero_is_the_reference_row(encoded, oracle_tables, L, s):
    import gz_oracle as O
    t = oracle_tables
    for text, enc in zip(*encoded):
        want = O.call(t, text, None, L, True, True)
        row, mask, start, n_real = W.windows(enc[1:-1], L, s, t.bos_id, t.eos_id, t.pad_id)[0]
        assert row == want["input_ids"] and mask == want["attention_mask"] and start == 0, text
        assert n_real == min(len(enc), L)


@pytest.mark.parametrize("L,s", LS)
def test_chunks_join_to_the_body_and_each_adds_a_token(encoded, oracle_tables, L, s):
    t = oracle_tables
    for text, enc in zip(*encoded):
        body = enc[1:-1]
        ws = W.windows(body, L, s, t.bos_id, t.eos_id, t.pad_id)
        joined = []
        for j, (row, mask, start, n_real) in enumerate(ws):
            chunk = row[1:n_real - 1]
            assert len(row) == L and row[0] == t.bos_id and row[n_real - 1] == t.eos_id and row[n_real:] == [t.pad_id] * (L - n_real)
            assert chunk == body[start:start + len(chunk)]
            if j:
                assert len(chunk) > s, (text, j)                     # fact 3
            joined += chunk if j == 0 else chunk[s:]
        assert joined == body, text                                  # fact 2


def test_window_count_against_a_count_by_hand():
    """Windows are laid until the body is covered: window j covers body[: j * step + room]."""
    for L, s in W.RULE_CASES + LS + W.ALIGN_CASES:
        room, step = L - 2, L - 2 - s
        for T in sorted(set(range(0, 70)) | set(W.edge_lengths(L, s)) | {5000}):
            n = 1
            while (n - 1) * step + room < T:
                n += 1
            ws = W.windows(list(range(T)), L, s, -1, -2, -3)
            assert len(ws) == n, (L, s, T)
            assert [w[2] for w in ws] == [j * step for j in range(n)]


def test_batch_form_matches_the_list_form():
    bodies = [list(range(100, 100 + T)) for T in (0, 7, 1, 30, 0)]
    b = W.batch(bodies, 8, 2, 1, 2, 0)
    per = [W.windows(x, 8, 2, 1, 2, 0) for x in bodies]
    assert b["win_off"].tolist() == [0, 1, 3, 4, 11, 12]
    assert b["input_ids"].tolist() == [w[0] for ws in per for w in ws]
    assert b["attention_mask"].tolist() == [w[1] for ws in per for w in ws]
    assert b["doc"].tolist() == [0, 1, 1, 2] + [3] * 7 + [4]
    assert b["start"].tolist() == [w[2] for ws in per for w in ws] and b["n_real"].tolist() == [w[3] for ws in per for w in ws]
    e = W.batch([], 8, 2, 1, 2, 0)
    assert e["input_ids"].shape == (0, 8) and e["win_off"].tolist() == [0] and e["doc"].shape == (0,)


def test_rule_cases_are_legal_and_hold_their_edges():
    assert {L % 4 for L, _ in W.RULE_CASES} == {0, 1, 2, 3}
    assert (3, 0) in W.RULE_CASES and any(s == L - 3 and L > 4 for L, s in W.RULE_CASES) and any(L > 256 for L, _ in W.RULE_CASES)
    for L, s in W.RULE_CASES + W.ALIGN_CASES:
        assert L >= 3 and 0 <= s <= L - 3
        room, step = L - 2, L - 2 - s
        Ts = W.edge_lengths(L, s)
        assert Ts[0] == 0 and 1 in Ts and room in Ts and room + 1 in Ts and all(T >= 0 for T in Ts)
        n = {T: len(W.windows([0] * T, L, s, 1, 2, 3)) for T in Ts}
        assert n[room] == 1 and n[room + 1] == 2                     # "T == room" still fits, one more token does not
        assert n[room + step] == 2 and n[room + step + 1] == 3 and n[room + 3 * step] == 4
        last = W.windows(list(range(room + step + 1)), L, s, -1, -2, -3)[-1]
        assert last[3] - 2 - s == 1                                  # "the last chunk has one new token"


def test_alignment_batch_starts_chunks_at_every_residue():
    """Rows of 0 .. 40 tokens back to back: the windows' first source cells fall on every residue mod 4 and mod 16."""
    starts = [0]
    for T in W.ALIGN_LENGTHS:
        starts.append(starts[-1] + T)
    assert {a % 16 for a in starts[:-1]} == set(range(16))           # "rows start at every residue"
    for L, s in W.ALIGN_CASES:
        src = [a + w[2] for a, T in zip(starts, W.ALIGN_LENGTHS) for w in W.windows([0] * T, L, s, 1, 2, 3) if w[3] > 2]
        assert {x % 4 for x in src} == {0, 1, 2, 3} and {x % 16 for x in src} == set(range(16))
    assert any(T > 2 * (L - 2) for T in W.ALIGN_LENGTHS for L, _ in W.ALIGN_CASES)


def test_word_list_has_split_words_and_an_unknown_one(oracle_tables):
    import gz_oracle as O
    t = oracle_tables
    pieces = {w: O.encode(w, t)[1:-1] for w in W.WORDS}
    assert all(len(p) >= 1 for p in pieces.values())
    assert sum(len(p) == 1 for p in pieces.values()) >= 5            # whole words
    assert sum(len(p) >= 3 for p in pieces.values()) >= 2            # words in several pieces
    assert any(t.unk_id in p for p in pieces.values())               # a piece outside the vocabulary
    texts = W.texts(300, 60, 5)
    lens = [len(O.encode(x, t)) - 2 for x in texts[:60]]
    assert "" in texts and max(lens) > 64
