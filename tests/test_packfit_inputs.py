"""CPU-only: tests/packfit_oracle.py tied to what exists -- its segments are pack_oracle's, its arrays are consistent with one
another, unpack_rows inverts it -- and the shape lists of tests/test_gpu_packfit.py hold the cases they are named for."""
import random

import numpy as np
import pytest

import pack_oracle as PO
import packfit_oracle as FO

SP = dict(bos=1, eos=2, pad=0)


def counters(lengths, base=1000):
    out, at = [], base
    for T in lengths:
        out.append(list(range(at, at + T)))
        at += T
    return out


def batches():
    rng = random.Random(9)
    out = []
    for _ in range(40):
        L = rng.randint(3, 40)
        out.append((L, counters([rng.randint(0, L + 4) for _ in range(rng.randint(0, 120))])))
    for L in FO.EVENT_LS[:-1]:
        out.append((L, counters(FO.event_edges(L))))
    return out


@pytest.mark.parametrize("k", range(len(batches())))
def test_the_oracles_arrays_agree_with_one_another(k):
    L, bodies = batches()[k]
    r = FO.batch(bodies, L, **SP)
    n, R = len(bodies), r["input_ids"].shape[0]
    kept = PO.batch(bodies, L, **SP)
    assert np.array_equal(r["doc_len"], kept["doc_len"]) and R <= kept["input_ids"].shape[0]
    assert sorted(r["row_docs"].tolist()) == list(range(n))                       # a permutation
    used = np.zeros(R, dtype=np.int64)
    np.add.at(used, r["doc_row"], r["doc_len"])
    assert (used <= L).all() and (used >= 2).all()
    for d in range(n):                                                             # a segment is pack_oracle's, where the maps say
        i, c, ln = r["doc_row"][d], r["doc_col"][d], r["doc_len"][d]
        assert r["input_ids"][i, c:c + ln].tolist() == PO.segment(bodies[d], L, SP["bos"], SP["eos"])
        assert r["position_ids"][i, c:c + ln].tolist() == list(range(ln)) and len(set(r["segment_ids"][i, c:c + ln].tolist())) == 1
    real = np.arange(L)[None, :] < used[:, None]
    assert (r["segment_ids"][real] > 0).all() and (r["segment_ids"][~real] == 0).all() and (r["input_ids"][~real] == SP["pad"]).all()
    # the packed order: rows ascending, columns ascending inside a row; row_off and seg_off index it
    key = [(int(r["doc_row"][d]), int(r["doc_col"][d])) for d in r["row_docs"]]
    assert key == sorted(key)
    assert r["row_off"][0] == 0 and r["row_off"][-1] == n
    for i in range(R):
        docs = r["row_docs"][r["row_off"][i]:r["row_off"][i + 1]]
        assert len(docs) >= 1 and (r["doc_row"][docs] == i).all()
        assert r["segment_ids"][i, r["doc_col"][docs]].tolist() == list(range(1, len(docs) + 1))
    assert np.array_equal(np.diff(r["seg_off"]), r["doc_len"][r["row_docs"]])
    # the segments back, in document order
    flat, off = FO.unpack(r)
    assert off.tolist() == kept["seg_off"].tolist()
    assert flat.tolist() == [v for b in bodies for v in PO.segment(b, L, SP["bos"], SP["eos"])]


def test_unpack_rows_inverts_the_oracle():
    from genz_tokenize import tokenize as tokenize
    for L, bodies in batches()[:12]:
        r = FO.batch(bodies, L, **SP)
        flat, off = tokenize.Tokenize.unpack_rows(r)
        want_flat, want_off = FO.unpack(r)
        assert flat.dtype == np.int32 and off.dtype == np.int64
        assert np.array_equal(flat, want_flat) and np.array_equal(off, want_off)
        kept = PO.batch(bodies, L, **SP)                                           # without row_docs: untouched
        kf, ko = tokenize.Tokenize.unpack_rows(kept)
        assert np.array_equal(kf, want_flat) and np.array_equal(ko, kept["seg_off"])


def test_the_rule_is_order_dependent_only_through_ties():
    """Documents of one length are placed in index order; the row numbers follow the longest documents."""
    doc_row, doc_col, R = FO.place([3, 7, 3, 7, 3], 10)
    assert (doc_row, doc_col, R) == ([0, 0, 1, 1, 2], [7, 0, 7, 0, 0], 3)


# ---- the shapes of the GPU tests -------------------------------------------------------------------------------------------------
def test_rank_shapes_sit_on_their_edges():
    ns = set(FO.RANK_NS)
    for edge in (64, FO.WAVE_DOCS, FO.TILE, FO.SCAN_SWITCH):
        assert {edge - 1, edge, edge + 1} <= ns
    assert 2 * FO.TILE + 1 in ns and FO.TILE == 4 * FO.WAVE_DOCS and FO.SCAN_SWITCH == 8 * 2048
    assert set(FO.one_length(5, 10)) == {1} and set(FO.one_length(5, 3)) == {0}
    two = FO.two_lengths(2 * FO.TILE + 1)
    assert len(two) == 2 * FO.TILE + 1 and two[:4] == [0, 3, 0, 3]
    for L in (10, 130, 4096):
        for times in (1, 2):
            lens = [min(T, L - 2) + 2 for T in FO.every_length(L, times)]
            assert sorted(set(lens)) == list(range(2, L + 1)) and len(lens) == times * (L - 1)
    assert FO.MAX_LEN == 4096 and FO.EVENT_LS[-1] == FO.MAX_LEN
    assert {L % 4 for L in FO.EVENT_LS} == {0, 1, 2, 3}                           # four cells a store, and one


@pytest.mark.parametrize("L", [127, 128, 130, 4096])
def test_event_shapes_hold_every_kind_of_event(L):
    """In event_edges(L) the middle length fills old rows (column > 0) -- several to a row, so that documents stand at the first
    and the last rank of an event -- and ends in a partial row; the shortest fills old rows, then opens new ones (column 0 in a row
    that no longer document opened) and ends in a partial new row."""
    Ts = FO.event_edges(L)
    lens = [min(T, L - 2) + 2 for T in Ts]
    doc_row, doc_col, R = FO.place_fast(lens, L)
    a, c = max(lens), 2
    rows_a = {doc_row[d] for d in range(len(lens)) if lens[d] == a}
    short = [d for d in range(len(lens)) if lens[d] == c]
    in_old = [d for d in short if doc_row[d] in rows_a]
    in_new = [d for d in short if doc_row[d] not in rows_a]
    assert in_old and in_new and all(doc_col[d] > 0 for d in in_old)
    heads = [d for d in in_new if doc_col[d] == 0]
    per_row = {}
    for d in in_new:
        per_row[doc_row[d]] = per_row.get(doc_row[d], 0) + 1
    assert len(heads) >= 2 and len(set(per_row.values())) == 2                   # full new rows and one partial new row
    b = sorted(set(lens))[1]
    mid = [d for d in range(len(lens)) if lens[d] == b]
    per = {}
    for d in mid:
        assert doc_row[d] in rows_a and doc_col[d] >= a
        per[doc_row[d]] = per.get(doc_row[d], 0) + 1
    assert max(per.values()) >= 2 and min(per.values()) < max(per.values())        # k a row, then the one partial row
    # documents of one length are interleaved with the others: the rank is by index, not by position in a run
    assert lens[:3] == [c, a, b]


@pytest.mark.parametrize("L", [3, 4, 5, 10])
def test_small_event_shapes_hold_what_they_can(L):
    """Too short for three lengths: one length (L = 3, 4: new rows only, L // 2 a row) or two (L = 5, 10: the
    len 2 documents go behind the long ones; at L = 5 they also open new rows)."""
    lens = [min(T, L - 2) + 2 for T in FO.event_edges(L)]
    doc_row, doc_col, R = FO.place(lens, L)
    kinds = sorted(set(lens))
    assert kinds == ([2] if L < 5 else [2, max(2, (3 * L) // 5)])
    per_row = [doc_row.count(i) for i in range(R)]
    if L < 5:
        assert per_row[:-1] == [L // 2] * (R - 1) and 1 <= per_row[-1] <= L // 2 and R >= 2
    else:
        long_rows = {doc_row[d] for d in range(len(lens)) if lens[d] == kinds[1]}
        behind = [d for d in range(len(lens)) if lens[d] == 2 and doc_row[d] in long_rows]
        fresh = [d for d in range(len(lens)) if lens[d] == 2 and doc_row[d] not in long_rows]
        assert behind and all(doc_col[d] >= kinds[1] for d in behind) and bool(fresh) == (L == 5)


def test_fill_shapes_sit_on_their_edges():
    for L in (6, 10, 127, 128, 130):
        lens = [T + 2 for T in FO.exact_rows(L, 7)]
        doc_row, doc_col, R = FO.place(lens, L)
        used = [0] * R
        for d, l in enumerate(lens):
            used[doc_row[d]] += l
        assert R == 7 and used == [L] * 7 and PO.place(lens, L)[2] > 7
    for L in (4, 7, 10, 128, 130):
        lens = [T + 2 for T in FO.one_cell_tail(L)]
        doc_row, doc_col, R = FO.place(lens, L)
        used = [0] * R
        for d, l in enumerate(lens):
            used[doc_row[d]] += l
        assert used == [L - 1] * R and R >= 3
    for L in (3, 4, 5, 10, 127, 128):
        n = 3 * (L // 2) + 1
        doc_row, doc_col, R = FO.place([2] * n, L)
        assert R == 4 and doc_row.count(0) == L // 2
