"""CPU-only: the table families of tests/row_tables.py against the reference's restatement of the loader (oracle/gz_oracle.py), the
properties each family is named for, the native host loader on them, and the conditions on the inputs of test_gpu_row_tables.py:
every (table, rows, p, seed) set of row_tables.cases and the custom tables' rows -- what that file runs with whole_word=True -- is
shown here, on the oracles alone, to choose and to leave cells, to choose a word of several cells, to replace a cell by a random
id, and to hold the ids the kernels could get wrong (the bitmap's last word, absent ids, ids past the snapshot).  The few hand-laid
rows of row_tables.word_rows are there for single words: of them it is shown that the cells named as one word are one, that those
named as two are two, and that the seeds the GPU file uses show both.  The rows that file makes from text are checked there, against
the reference's restatement of the encoder."""
import time

import numpy as np
import pytest

import gz_oracle as O
import infill_oracle as IO
import mask_oracle as MO
import pack_oracle as PO
import row_tables as RT

ALL = RT.SMALL_TABLES + RT.BIG_TABLES


@pytest.mark.parametrize("key", ALL + ("custom",))
def test_restated_loader_is_the_references(key):
    t = RT.custom() if key == "custom" else RT.table(key)
    ref = O.Tables(t.vocab, t.merges, t.specials)
    assert ref.encoder == t.snap_encoder and ref.decoder == t.decoder
    assert (ref.pad_id, ref.bos_id, ref.eos_id, ref.encoder[t.specials[3]]) == t.snap_ids
    assert t.n_ids == max(ref.decoder) + 1
    assert t.cont == sorted(i for i, w in ref.decoder.items() if w.endswith("@@"))
    if t.second is None:
        assert t.encoder is t.snap_encoder and t.ids == t.snap_ids and t.size == len(ref.encoder)
    else:
        # several vocab files behave like one file whose lines are the concatenation of theirs
        live = O.Tables(t.vocab + t.second, t.merges, t.specials)
        assert live.encoder == t.encoder and (live.pad_id, live.bos_id, live.eos_id, live.encoder[t.specials[3]]) == t.ids
        assert t.size == len(live.encoder)                           # the default random_ids of mask_rows: (5, len(encoder))


@pytest.mark.parametrize("key", RT.SMALL_TABLES)
def test_native_host_loader_agrees(key):
    """gz_host_tables (no GPU): the words and ids of the loader the device tables are built by, and the decoder the snapshot takes of
    them -- the last word of the list wins an id"""
    from genz_tokenize import _native
    t = RT.table(key)
    for vocab, enc in ((t.vocab, t.snap_encoder),) + (((t.vocab + t.second, t.encoder),) if t.second else ()):
        ht = _native.HostTables(vocab, t.merges, t.specials)
        items = ht.vocab_items()
        ht.close()
        assert dict(items) == enc and len(items) == len(enc)
        if enc is t.snap_encoder:
            assert {i: w for w, i in items} == t.decoder


def test_moved():
    t = RT.moved()
    assert len(set(t.ids)) == 4 and all(i > 4 for i in t.ids) and all(t.absent(i) for i in range(4)) and t.decoder[4] == "<unk>"
    assert all(abs(a - b) > 1 for a in t.ids for b in t.ids if a != b)
    words = [w for w in t.snap_encoder if w not in RT.SPECIALS]
    assert 300 <= len(words) <= 400 and abs(sum(w.endswith("@@") for w in words) - len(words) / 2) <= 2
    assert all(p in t.snap_encoder for p in RT.PIECES)
    # a moved special shares its id with the word behind it; behind <pad> and <mask> that word ends in "@@"
    assert t.decoder[t.pad].endswith("@@") and t.decoder[t.mask].endswith("@@") and t.pad in t.cont and t.mask in t.cont


def test_renamed():
    t, m = RT.renamed(), RT.moved()
    assert t.vocab == m.vocab and t.specials != m.specials
    assert len(set(t.ids)) == 4 and all(i > 4 for i in t.ids) and not set(t.ids) & set(m.ids)
    assert all(s.encode() + b" " in t.vocab for s in t.specials[:4]) and t.specials[3].endswith("@@")
    assert all(t.absent(i) for i in range(4)) and t.decoder[4] == "[UNK]"
    assert all(s in t.snap_encoder for s in RT.SPECIALS[:4])         # the usual strings are ordinary words here


def test_collide():
    t = RT.collide()
    e = t.snap_encoder
    # both directions of a won id
    assert e["p0"] == e["c1@@"] and t.decoder[e["p0"]] == "c1@@" and e["p0"] in t.cont
    assert e["c0@@"] == e["p3"] and t.decoder[e["p3"]] == "p3" and e["p3"] not in t.cont
    assert [i for i in range(5, t.n_ids) if t.absent(i)] == [5, 6, 7, 11]
    assert e[""] == t.n_ids - 1 == len(e) and e[""] not in t.cont and e["@@"] in t.cont
    assert e["p1"] == e["c30@@"] and e["p1"] in t.cont


@pytest.mark.parametrize("n", RT.EDGE_NS)
def test_edge(n):
    t = RT.edge(n)
    assert t.n_ids == n == t.size and t.ids == (0, 1, 2, 3) and sorted(t.decoder) == list(range(n))
    assert t.cont == sorted(i for i in {n - 1, n - 2, 31, 32, 5} if i < n)
    rows, one, two = RT.edge_rows(t, 64)
    ids = np.array(rows)
    _, head = MO.heads(ids, t.cont, t.ids, True)
    r, a, b = one
    assert (head[r, a:b + 1] == a).all() and head[r, b + 1] == b + 1 and ids[r, a] == n - 1
    (r, a, _), (_, c, d) = two
    assert head[r, a] == a and (head[r, c:d + 1] == c).all() and ids[r, a] == n
    out = np.arange(2, 14, 2)                                        # row 2: (n - 1, an id outside the snapshot) six times
    assert ids[2][out].tolist() == [n, n + 1, n + 31, n + 32, 2 ** 31 - 1, -7] and (ids[2][out - 1] == n - 1).all()
    assert (head[2][out] == out - 1).all() and (head[2][out + 1] == out + 1).all()   # each sits in the continuation's word, and ends it


@pytest.mark.parametrize("n", RT.BIG_NS)
def test_big(n):
    t = RT.big(n)
    assert t.n_ids == n == t.size and t.merges == RT.HEADER
    words = (n + 31) // 32
    assert (words * 4 <= 48 * 1024) == (n == RT.BIG_NS[0])           # GZ_MASK_LDS_MAX_BYTES lies between the two
    cont = set(t.cont)
    assert {5, 31, 32} <= cont and set(range(n - 40, n)) <= cont and abs(len(cont) / n - 0.5) < 0.01
    pool = RT.big_pool(t)
    assert len(pool) == 124 and 0.4 < sum(i in cont for i in pool) / len(pool) < 0.75
    assert max(len(w) for w in t.snap_encoder) <= 8


def test_grown():
    t = RT.grown()
    new = {w: i for w, i in t.encoder.items() if w not in t.snap_encoder}
    assert any(w.endswith("@@") and i >= t.n_ids for w, i in new.items())
    w = RT.GROWN_MOVED_WORD
    assert t.snap_encoder[w] in t.cont and t.encoder[w] >= t.n_ids and t.decoder[t.snap_encoder[w]] == w
    assert t.mask != t.snap_ids[3] and t.mask >= t.n_ids and t.ids[:2] == t.snap_ids[:2] and t.eos != t.snap_ids[2]
    assert t.snap_ids[3] in t.decoder and t.snap_ids[3] in t.cont      # the old <mask> id: a word of the snapshot, and it continues
    assert t.size > t.n_ids
    must = RT.must_ids(t)
    assert t.snap_ids[3] in must and t.encoder["g1@@"] in must and t.snap_encoder[w] in t.cont


def test_big_table_through_the_host_loader():
    """the figure in test_gpu_row_tables.py's docstring"""
    from genz_tokenize import _native
    t = RT.big(RT.BIG_NS[1])
    t0 = time.perf_counter()
    ht = _native.HostTables(t.vocab, t.merges, t.specials)
    dt = time.perf_counter() - t0
    items = ht.vocab_items()
    ht.close()
    print("HostTables(big(%d)): %.2f s" % (t.n_ids, dt))
    assert len(items) == t.size and items[-1] == ("w%x@@" % (t.n_ids - 1), t.n_ids - 1)
    assert dt < 30


# ---- conditions on the inputs of the GPU file ------------------------------------------------------------------------------------
def conditions(t, ids, p, seed):
    ids = np.asarray(ids, dtype=np.int64)
    L = ids.shape[1]
    cols = np.arange(L)[None, :]
    prot, head = MO.heads(ids, t.cont, t.ids, True)
    last = np.isin(ids, t.last_word_ids())
    assert last.any() and (last & ~prot).any(), "no id of the last bitmap word"
    assert any(t.absent(int(v)) for v in np.unique(ids)), "no absent id"
    if t.second is not None:
        assert ((ids >= t.n_ids) & (ids <= t.size) & ~prot).any(), "no id past the snapshot"
    # mask
    want = RT.mask_want(t, ids, p, seed)
    chosen = want["labels"] != -100
    assert chosen.any() and (~prot & ~chosen).any()
    assert (chosen & (head != cols)).any(), "no chosen word of several cells"
    assert (chosen & (want["input_ids"] != ids) & (want["input_ids"] != t.mask)).any(), "no random replacement"
    # infill
    t_start, len_t, n_len = IO.rule_ints(p)
    _, _, _, inside = IO.chosen_cells(ids, t.cont, t.ids, seed, t_start, len_t, n_len, True, 0)
    assert inside.any() and (~prot & ~inside).any()
    assert (inside & (head != cols)).any(), "no span word of several cells"


@pytest.mark.parametrize("key", ALL)
def test_conditions_on_the_gpu_files_row_sets(key):
    t = RT.table(key)
    for R, L, p, seed in RT.cases(key):
        ids = RT.rows_of(key, R, L, seed)
        assert len(ids) == R and all(len(r) == L for r in ids)
        conditions(t, ids, p, seed)
        if key in ("moved", "renamed", "grown"):                     # (their specials lie elsewhere)
            assert all(any(v in r[1:] for r in ids) for v in range(4)), "ids 0..3 as body tokens"


def test_long_rows_lay_a_word_across_trips():
    for key in RT.SMALL_TABLES:
        t = RT.table(key)
        R, L = RT.LONG
        ids = np.array(RT.rows_of(key, R, L, 1))
        _, head = MO.heads(ids, t.cont, t.ids, True)
        assert (head[1, 10:310] == 10).all() and head[1, 310] == 310      # one word over columns 64, 128, 192 and 256
        assert (head[0, 60:68] == 60).all() and (head[2, 200:290] == 200).all()


@pytest.mark.parametrize("key", RT.WORD_TABLES)
def test_hand_laid_rows_hold_the_words_they_name(key):
    """row_tables.word_rows: `together` lies in one word and `apart` in two by the oracle's heads, and at every row length the GPU file
    runs them at the seeds show each word of `together` chosen and left, and each pair of `apart` split"""
    t = RT.table(key)
    rows, together, apart, lengths = RT.word_rows(key)
    for L in lengths:
        ids = np.array(RT.pad_rows(t, rows, L), dtype=np.int64)
        prot, head = MO.heads(ids, t.cont, t.ids, True)
        assert all(len(set(head[r, a:b + 1])) == 1 and not prot[r, a:b + 1].any() for r, a, b in together)
        assert all(head[r, a] != head[r, b] and not prot[r, a] and not prot[r, b] for r, a, b in apart)
        picked = [RT.mask_want(t, ids, 0.5, seed)["labels"] != -100 for seed in RT.WORD_SEEDS]
        for r, a, b in together:
            assert {bool(q[r, a]) for q in picked} == {False, True}, (L, r, a, b)
        for r, a, b in apart:
            assert any(q[r, a] != q[r, b] for q in picked), (L, r, a, b)
    if key == "collide":
        e = t.snap_encoder
        assert rows[0][2] == e["p0"] and rows[0][5] == e["p3"] and rows[0][11] == e[""] and rows[0][14] == e["@@"]
        assert t.absent(rows[0][8]) and t.absent(rows[0][17])
    if key == "grown":
        e, s = t.encoder, t.snap_encoder
        assert rows[0][2] == e["g1@@"] >= t.n_ids and rows[0][5] == s[RT.GROWN_MOVED_WORD] and rows[0][11] == e[RT.GROWN_MOVED_WORD] >= t.n_ids
        assert rows[0][8] == t.snap_ids[3] and rows[0][14] == t.snap_ids[2] and rows[0][16] == t.mask and rows[0][18] == e["g5@@"]


def custom_packed(t):
    """the oracle's packed rows of the custom texts, with the extra rows behind them"""
    ref = O.Tables(t.vocab, t.merges, t.specials)
    bodies = [O.encode_words(s, ref)[0] for s in RT.custom_texts()]
    want = PO.batch(bodies, RT.CUSTOM_L, t.bos, t.eos, t.pad)
    return bodies, want, np.concatenate([want["input_ids"], np.array(RT.custom_extra_rows(), dtype=np.int32)])


def test_conditions_on_the_custom_tables_rows():
    t = RT.custom()
    assert t.n_ids == 100005 and t.ids == (0, 1, 2, 3) and len(t.cont) > 10000
    bodies, want, ids = custom_packed(t)
    assert len(bodies) == RT.CUSTOM_DOCS and want["input_ids"].shape[0] > 64 and (want["input_ids"] > 65535).any()
    assert np.isin(want["input_ids"], t.cont).any()
    conditions(t, ids, *RT.CUSTOM_CASE)
