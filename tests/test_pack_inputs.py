"""CPU-only: the packing rule of tests/pack_oracle.py against the reference's restatement (oracle/gz_oracle.py) on the bundled
tables, its placement against the two properties that define next-fit, `Tokenize.unpack_rows` (numpy only) as its inverse, and
the shape lists of the GPU tests against the cases they are named for."""
import random

import numpy as np
import pytest

import pack_oracle as P

LS = (3, 4, 5, 7, 10, 16)


@pytest.fixture(scope="module")
def encoded(oracle_tables):
    import gz_oracle as O
    r = random.Random(11)
    vocab = [w for w in list(oracle_tables.encoder)[5:4000:7] if " " not in w and w]
    texts = P.texts(200, 12, 3)
    for _ in range(200):                                             # vocabulary words, pieces of them, strings outside the tables
        words = []
        for _ in range(r.randint(0, 12)):
            w = r.choice(vocab).replace("@@", "")
            words.append(w if r.random() < 0.7 else w[:r.randint(1, len(w))] + r.choice(["", "x", "Q9", "中"]))
        texts.append(" ".join(words))
    return texts, [O.encode(t, oracle_tables) for t in texts]


def test_texts_cover_empty_short_and_long_bodies(encoded):
    _, enc = encoded
    lens = [len(e) - 2 for e in enc]
    assert min(lens) == 0 and max(lens) > 16 and sum(1 <= n <= 3 for n in lens) > 10 and len(enc) == 400


@pytest.mark.parametrize("L", LS)
def test_segment_is_the_reference_row_without_its_padding(encoded, oracle_tables, L):
    import gz_oracle as O
    t = oracle_tables
    for text, enc in zip(*encoded):
        want = O.call(t, text, None, L, True, True)["input_ids"]
        n_real = min(len(enc), L)
        seg = P.segment(enc[1:-1], L, t.bos_id, t.eos_id)
        assert seg == want[:n_real] and want[n_real:] == [t.pad_id] * (L - n_real), text
        assert 2 <= len(seg) <= L


@pytest.mark.parametrize("L", LS)
def test_rows_hold_what_fits_and_not_one_document_more(encoded, oracle_tables, L):
    t = oracle_tables
    bodies = [e[1:-1] for e in encoded[1]]
    b = P.batch(bodies, L, t.bos_id, t.eos_id, t.pad_id)
    ro, ln = b["row_off"], b["doc_len"]
    R = len(ro) - 1
    assert ro[0] == 0 and ro[R] == len(bodies) and (np.diff(ro) >= 1).all()
    for i in range(R):
        used = int(ln[ro[i]:ro[i + 1]].sum())
        assert used <= L                                             # no row's lengths sum past L
        if i + 1 < R:
            assert used + int(ln[ro[i + 1]]) > L                     # the next row's first document would not have fitted
    # order kept: documents lie in the rows in their order, each behind the one before it
    assert (np.diff(b["doc_row"]) >= 0).all() and (np.diff(b["doc_row"]) <= 1).all()
    same_row = np.diff(b["doc_row"]) == 0
    assert (b["doc_col"][1:][same_row] == (b["doc_col"][:-1] + ln[:-1])[same_row]).all() and (b["doc_col"][1:][~same_row] == 0).all()
    assert b["seg_off"].tolist() == [0] + np.cumsum(ln).tolist()
    # cell arrays against the maps
    for r in (0, 1, len(bodies) // 2, len(bodies) - 1):
        i, c, n = b["doc_row"][r], b["doc_col"][r], ln[r]
        assert b["input_ids"][i, c:c + n].tolist() == P.segment(bodies[r], L, t.bos_id, t.eos_id)
        assert b["position_ids"][i, c:c + n].tolist() == list(range(n)) and (b["segment_ids"][i, c:c + n] == r - ro[i] + 1).all()
    tail = np.arange(L)[None, :] >= np.add.reduceat(ln, ro[:-1])[:, None]
    assert (b["segment_ids"][tail] == 0).all() and (b["segment_ids"][~tail] > 0).all() and (b["input_ids"][tail] == t.pad_id).all()
    assert np.array_equal(b["attention_mask"], (b["input_ids"] != t.pad_id).astype(np.int32))


def unpack_rows():
    """Tokenize.unpack_rows without the native library (a static method, numpy only)."""
    from genz_tokenize.tokenize import Tokenize
    return Tokenize.unpack_rows


@pytest.mark.parametrize("L", LS)
def test_unpack_rows_inverts_the_batch(encoded, oracle_tables, L):
    t = oracle_tables
    bodies = [e[1:-1] for e in encoded[1]]
    for bs in (bodies, bodies[:1], [], [[t.pad_id, t.pad_id, 7], [], [t.pad_id]]):
        b = P.batch(bs, L, t.bos_id, t.eos_id, t.pad_id)
        flat, off = unpack_rows()(b)
        assert flat.dtype == np.int32 and off.dtype == np.int64 and off.tolist() == b["seg_off"].tolist()
        assert [flat[off[r]:off[r + 1]].tolist() for r in range(len(bs))] == [P.segment(x, L, t.bos_id, t.eos_id) for x in bs]


def test_place_by_hand():
    assert P.place([], 8) == ([], [], 0)
    assert P.place([2, 2, 2, 2, 2], 8) == ([0, 0, 0, 0, 1], [0, 2, 4, 6, 0], 2)                  # four fill the row exactly
    assert P.place([5, 3, 4, 5, 8, 2], 8) == ([0, 0, 1, 2, 3, 4], [0, 5, 0, 0, 0, 0], 5)         # 4 + 5 = L + 1 does not fit
    b = P.batch([[7], [], [8, 9, 10, 11, 12, 13, 14], [5]], 6, 1, 2, 0)
    assert b["input_ids"].tolist() == [[1, 7, 2, 1, 2, 0], [1, 8, 9, 10, 11, 2], [1, 5, 2, 0, 0, 0]]
    assert b["segment_ids"].tolist() == [[1, 1, 1, 2, 2, 0], [1] * 6, [1, 1, 1, 0, 0, 0]]
    assert b["position_ids"].tolist() == [[0, 1, 2, 0, 1, 0], [0, 1, 2, 3, 4, 5], [0, 1, 2, 0, 0, 0]]
    assert b["row_off"].tolist() == [0, 2, 3, 4] and b["seg_off"].tolist() == [0, 3, 5, 11, 14] and b["doc_len"].tolist() == [3, 2, 6, 3]
    e = P.batch([], 6, 1, 2, 0)
    assert e["input_ids"].shape == (0, 6) and e["row_off"].tolist() == [0] and e["seg_off"].tolist() == [0] and e["doc_row"].shape == (0,)


def test_shape_lists_hold_the_cases_they_are_named_for():
    assert {L % 4 for L in P.RULE_LS} == {0, 1, 2, 3} and min(P.RULE_LS) == 3 and max(P.RULE_LS) > 256
    for L in P.RULE_LS + P.ALIGN_LS + P.BLOCK_EDGE_LS:
        Ts = P.edge_lengths(L)
        assert all(T >= 0 for T in Ts) and 0 in Ts and L - 2 in Ts and L - 1 in Ts
        lens = [len(P.segment([0] * T, L, 1, 2)) for T in Ts]
        assert min(lens) == 2 and max(lens) == L and lens[Ts.index(L - 2)] == L and lens[Ts.index(L - 1)] == L
    for L in P.RULE_LS:
        if L < 4:
            continue
        lens = [T + 2 for T in P.exact_fill(L)]
        assert all(2 <= n <= L for n in lens)
        row, col, R = P.place(lens, L)
        used = [sum(n for n, r in zip(lens, row) if r == i) for i in range(R)]
        assert L in used                                             # "a row that fills exactly"
        assert any(col[k] == 0 and col[k - 1] + lens[k - 1] + lens[k] == L + 1 for k in range(1, len(lens)))   # "... and to L + 1"
    for lead in (False, True):                                       # two chains that never meet
        lens = [T + 2 for T in P.never_merge(lead)]
        assert len(lens) == 2 * P.TILE + 3
        row, col, R = P.place(lens, 10)
        heads = [k for k in range(len(lens)) if col[k] == 0]
        assert {h % 2 for h in heads[1:]} == ({1} if lead else {0}) and len(heads) > P.TILE
        other = list(range(2 if lead else 1, len(lens), 2))          # the chain one document further on
        assert not set(other) & set(heads[1:])
    L, Ts = P.long_row()
    row, col, R = P.place([T + 2 for T in Ts], L)
    assert R == 3 and row.count(0) == P.TILE + 3 and [k for k in range(len(Ts)) if col[k] == 0] == [0, P.TILE + 3, 2 * P.TILE + 6]
    L, Ts = P.skipped_tile()
    row, col, R = P.place([T + 2 for T in Ts], L)
    assert R == 2 and not [k for k in range(P.TILE, 2 * P.TILE) if col[k] == 0]                  # no head in tile 1
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097} <= set(P.BLOCK_EDGE_NS)
    for B in (P.TILE, P.GROUP, P.FILL_DOCS):
        assert {B - 1, B, B + 1} <= set(P.BLOCK_EDGE_NS)
    starts = np.cumsum([0] + P.ALIGN_LENGTHS[:-1])
    assert {int(a) % 16 for a in starts} == set(range(16))           # "bodies start at every residue"
