"""The calls that shape rows -- window_rows, pack_rows, mask_rows, infill_rows, their encode_* and *_to_device forms -- on vocabularies
other than the bundled one (tests/row_tables.py): special ids that are not 0, 1, 2, 3, continuation bitmaps of every size around a
word's edge and around GZ_MASK_LDS_MAX_BYTES, id spaces with holes and collisions, and a vocabulary that grew after the decoder
snapshot was taken.  Every comparison with an oracle is exact, on every returned array, dtype and shape included; the oracles take
the table's ids from row_tables, which test_row_tables_inputs.py ties to the reference's restatement of the loader, and that file
also shows that every row set used here holds what it is meant to hold.

Load times of big(393 217), the table one id past the LDS threshold (393 212 words of at most 8 bytes, a merges file of one line):
  host loader alone (_native.HostTables, no GPU)          0.14 - 0.18 s  (test_row_tables_inputs.py prints it)
  Tokenize from the two files to the first vocab_size()   0.07 - 0.09 s on an MI355X host with the tables built and the table cache
                                                          written, 0.03 - 0.05 s on a cache hit; big(393 216) takes the same
Both are far below the 30 s a table may take; neither load was refused."""
import os
import time

import numpy as np
import pytest

import gz_oracle as O
import pack_oracle as PO
import row_tables as RT
import window_oracle as WO

pytestmark = pytest.mark.gpu

SEEDS = RT.WORD_SEEDS


def build(folder, t):
    """Tokenize over the table's files, the way fromFile does it, with the table's special strings"""
    from genz_tokenize import Tokenize
    vocab, merges = os.path.join(folder, t.name + ".vocab"), os.path.join(folder, t.name + ".codes")
    for path, data in ((vocab, t.vocab), (merges, t.merges)):
        if not os.path.exists(path):
            with open(path, "wb") as f:
                f.write(data)
    tok = Tokenize.__new__(Tokenize)
    tok.vocab_file, tok.bpe_file = vocab, merges
    pad, bos, eos, mask, unk = t.specials
    tok.__init__(pad_token=pad, bos_token=bos, eos_token=eos, mask_token=mask, unk_token=unk)
    return tok


def second_file(folder, t):
    path = os.path.join(folder, t.name + ".second")
    with open(path, "wb") as f:
        f.write(t.second)
    return path


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return str(tmp_path_factory.mktemp("row_tables"))


@pytest.fixture(scope="module")
def toks(folder):
    """one Tokenize a table, built on first use"""
    made = {}

    def get(key):
        if key not in made:
            t = RT.custom() if key == "custom" else RT.table(key)
            t0 = time.perf_counter()
            tok = build(folder, t)
            assert tok.vocab_size() == t.size and tuple(tok._special_ids()[:4]) == t.ids
            print("\n[load] %s: %.2f s" % (key, time.perf_counter() - t0))
            made[key] = (tok, t)
        return made[key]
    return get


def same(got, want):
    assert set(want) <= set(got)
    for k in want:
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        assert np.array_equal(g, want[k]), (k, np.argwhere(g != want[k])[:4].tolist())


def as_rows(ids):
    return np.array(ids, dtype=np.int64).astype(np.int32)


def check_mask(tok, t, ids, p, seed, **kw):
    want = RT.mask_want(t, ids, p, seed, **kw)
    same(tok.mask_rows(ids, p=p, seed=seed, **kw), want)
    return want


def check_infill(tok, t, ids, p, seed, **kw):
    want = RT.infill_want(t, ids, p, seed, **kw)
    same(tok.infill_rows(ids, p=p, seed=seed, **kw), want)
    return want


def check_cases(tok, t, key):
    """mask_rows and infill_rows over the table's row sets (row_tables.cases) against the oracles"""
    for R, L, p, seed in RT.cases(key):
        ids = as_rows(RT.rows_of(key, R, L, seed))
        for ww in (True, False):
            check_mask(tok, t, ids, p, seed, whole_word=ww)
            check_infill(tok, t, ids, p, seed, whole_word=ww, dec_len=None if ww else max(1, L // 2))


def check_words(tok, t, key):
    """The hand-laid rows of a table (row_tables.word_rows) at each of their row lengths: over SEEDS at p = 0.5, mask and infill equal
    the oracles; every (row, first, last) of `together` is chosen as a whole or not at all; the two cells (row, a, b) of every entry
    of `apart` lie in different words: some seed chooses one and not the other."""
    rows, together, apart, lengths = RT.word_rows(key)
    for L in lengths:
        check_words_at(tok, t, as_rows(RT.pad_rows(t, rows, L)), together, apart)


def check_words_at(tok, t, ids, together, apart):
    split = {x: False for x in apart}
    for seed in SEEDS:
        picked = check_mask(tok, t, ids, 0.5, seed)["labels"] != -100
        for r, a, b in together:
            assert picked[r, a:b + 1].all() or not picked[r, a:b + 1].any(), (seed, r, a, b)
        for r, a, b in apart:
            split[(r, a, b)] |= bool(picked[r, a] != picked[r, b])
        check_infill(tok, t, ids, 0.5, seed)
        check_infill(tok, t, ids, 0.3, seed, lengths="fixed", mean_span=1, max_span=1)       # spans of one word: the words show
    assert all(split.values()), split


def padded(t, cells, L):
    return cells + [t.pad] * (L - len(cells))


def bodies_of(t, rows):
    """the cells between bos and the first eos of rows made by row_tables.rows"""
    return [r[1:r.index(t.eos, 1)] for r in rows]


# ---- a. protected cells and framing follow the table's ids -------------------------------------------------------------------
@pytest.mark.parametrize("key", ["moved", "renamed"])
def test_mask_and_infill_protect_the_tables_ids_and_nothing_else(toks, key):
    tok, t = toks(key)
    assert not set(t.ids) & {0, 1, 2, 3, 4}
    check_cases(tok, t, key)
    # ids 0..3 are ordinary tokens: all chosen at p = 1, and the table's own ids are not
    L = 12
    ids = as_rows([padded(t, [t.bos, 0, 1, 2, 3, t.mask, 0, t.pad, 3, t.eos], L), [3, 2, 1, 0] * 3])
    got = tok.mask_rows(ids, p=1.0, mask_prob=1.0, random_prob=0.0)
    want = np.where(np.isin(ids, t.ids), -100, ids)
    assert np.array_equal(got["labels"], want) and got["n_chosen"].tolist() == [6, 12]
    assert np.array_equal(got["input_ids"], np.where(np.isin(ids, t.ids), ids, t.mask))
    inf = tok.infill_rows(ids, p=1.0)
    same(inf, RT.infill_want(t, ids, 1.0, 0))
    assert inf["input_ids"][1].tolist() == padded(t, [t.mask], L) and inf["labels"][1].tolist() == ([t.mask] + [3, 2, 1, 0] * 3)[:L]
    assert inf["decoder_input_ids"][1, 0] == t.bos and inf["dec_len"][1] == 14 and inf["labels"][0, :5].tolist() == [t.mask, 0, 1, 2, 3]


@pytest.mark.parametrize("key", ["moved", "renamed"])
def test_windows_and_packs_frame_and_pad_with_the_tables_ids(toks, key):
    tok, t = toks(key)
    sp = dict(bos=t.bos, eos=t.eos, pad=t.pad)
    bodies = bodies_of(t, RT.rows_of(key, 65, 130, 3)) + bodies_of(t, RT.rows_of(key, 2, 64, 4)) + [[0, 1, 2, 3], [], [3]]
    framed = [[t.bos] + b + [t.eos] for b in bodies]
    for L, s in ((16, 0), (16, 5), (7, 2), (64, 10)):
        want = WO.batch(bodies, L, s, **sp)
        for got in (tok.window_rows(bodies, L, s, framed=False), tok.window_rows(framed, L, s, framed=True)):
            same(got, want)
            ids, am = got["input_ids"], got["attention_mask"]
            assert np.array_equal(am, (ids != t.pad).astype(np.int32)) and (ids == t.pad).any() and (ids[:, 0] == t.bos).all()
            assert all(((ids == v) & (am == 1)).any() for v in range(4))
    for L in (16, 21, 64):
        want = PO.batch(bodies, L, **sp)
        for got in (tok.pack_rows(bodies, L, framed=False), tok.pack_rows(framed, L, framed=True)):
            same(got, want)
            ids, am = got["input_ids"], got["attention_mask"]
            assert np.array_equal(am, (ids != t.pad).astype(np.int32)) and (ids == t.pad).any() and (ids[:, 0] == t.bos).all()
            assert all(((ids == v) & (am == 1)).any() for v in range(4))
            assert np.array_equal(got["segment_ids"] == 0, ids == t.pad)


@pytest.mark.parametrize("key", ["moved", "renamed"])
def test_device_rows_of_the_same_object(toks, key):
    tok, t = toks(key)
    ref = O.Tables(t.vocab, t.merges, t.specials)
    texts = RT.texts(60, 11)
    bodies = [O.encode_words(s, ref)[0] for s in texts]
    for make, want in ((lambda: tok.encode_windows_to_device(texts, 16, 4), WO.batch(bodies, 16, 4, t.bos, t.eos, t.pad)),
                       (lambda: tok.encode_packs_to_device(texts, 24), PO.batch(bodies, 24, t.bos, t.eos, t.pad))):
        dev = make()
        same(dev, want)
        rows, host = dev["input_ids"], want["input_ids"]
        assert host.shape[0] > 8
        for ww in (True, False):
            got = tok.mask_rows_to_device(rows, p=0.4, seed=3, whole_word=ww, row_base=17)
            same(got, RT.mask_want(t, host, 0.4, 3, whole_word=ww, row_base=17))
            got = tok.infill_rows_to_device(rows, p=0.4, seed=3, whole_word=ww, row_base=17, dec_len=9)
            same(got, RT.infill_want(t, host, 0.4, 3, whole_word=ww, row_base=17, dec_len=9))
        assert np.array_equal(rows.numpy(), host)                    # the source rows are not changed


# ---- b. from text on such a table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["moved", "renamed"])
def test_from_text(toks, key):
    tok, t = toks(key)
    ref = O.Tables(t.vocab, t.merges, t.specials)
    texts = RT.texts(70, 5)
    enc = [O.encode_words(s, ref) for s in texts]
    bodies = [e[0] for e in enc]
    assert max(len(b) for b in bodies) > 40 and any(t.encoder[t.specials[4]] in b for b in bodies)
    for L, s in ((8, 2), (16, 0), (64, 5)):
        got = tok.encode_windows(texts, L, s)
        same(got, WO.batch(bodies, L, s, t.bos, t.eos, t.pad))
        first = got["input_ids"][got["win_off"][:-1]]
        batch = tok.encode_batch(texts, max_len=L)
        want_ids, want_am = O.call_batch(ref, texts, None, L)[:2]
        assert np.array_equal(first, batch["input_ids"]) and first.tolist() == want_ids
        assert batch["attention_mask"].tolist() == want_am
        same(tok.encode_packs(texts, L), PO.batch(bodies, L, t.bos, t.eos, t.pad))
    # whole words: the pieces "xx@@ yy@@ zz" of a word whose pieces the vocabulary holds go together
    L = 130
    ids = tok.encode_batch(texts, max_len=L)["input_ids"]
    assert ids.tolist() == O.call_batch(ref, texts, None, L)[0]
    unk = t.encoder[t.specials[4]]
    words = []
    for r, (body, per_word) in enumerate(enc):
        at = 1
        for n in per_word:
            if n > 1 and unk not in body[at - 1:at - 1 + n - 1]:
                words.append((r, at, at + n - 1))
            at += n
    assert len(words) > 30
    seen = set()
    for seed in SEEDS:
        picked = check_mask(tok, t, ids, 0.5, seed)["labels"] != -100
        for r, a, b in words:
            assert picked[r, a:b + 1].all() or not picked[r, a:b + 1].any(), (seed, texts[r], a, b)
            seen.add(bool(picked[r, a]))
        check_infill(tok, t, ids, 0.5, seed)
    assert seen == {False, True}
    loose = tok.mask_rows(ids, p=0.5, seed=1, whole_word=False)["labels"] != -100
    assert any(loose[r, a:b + 1].any() and not loose[r, a:b + 1].all() for r, a, b in words)


# ---- c. bitmap edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RT.EDGE_NS)
def test_bitmap_edges(toks, n):
    key = "edge%d" % n
    tok, t = toks(key)
    assert t.n_ids == n
    check_cases(tok, t, key)
    check_words(tok, t, key)


# ---- d. the size threshold ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RT.BIG_NS)
def test_bitmap_in_lds_and_in_memory_by_the_vocabularys_size(toks, n):
    """48 KB of bitmap is staged in LDS, one id more is read from memory; behind the switch both tables take the memory path.  The
    calls go through the ordinary entry: a launch that fails raises there, and fails this test."""
    from genz_tokenize import _native
    key = "big%d" % n
    tok, t = toks(key)
    assert t.n_ids == n and ((n + 31) // 32 * 4 <= 48 * 1024) == (n == RT.BIG_NS[0])
    sets = [(as_rows(RT.rows_of(key, R, L, seed)), p, seed) for R, L, p, seed in RT.cases(key)]
    assert [s[0].shape for s in sets] == [(65, 64), (65, 130)]
    first = [(tok.mask_rows(ids, p=p, seed=seed), tok.infill_rows(ids, p=p, seed=seed)) for ids, p, seed in sets]
    for (ids, p, seed), (m, f) in zip(sets, first):
        same(m, RT.mask_want(t, ids, p, seed))
        same(f, RT.infill_want(t, ids, p, seed))
    _native.debug_set("mask_lds", 0, tok._ctx)
    try:
        again = [(tok.mask_rows(ids, p=p, seed=seed), tok.infill_rows(ids, p=p, seed=seed)) for ids, p, seed in sets]
    finally:
        _native.debug_set("mask_lds", 1, tok._ctx)
    for (m, f), (m2, f2) in zip(first, again):
        same(m2, m)
        same(f2, f)
    check_words(tok, t, key)


# ---- e. holes and collisions ----------------------------------------------------------------------------------------------------
def test_holes_and_collisions(toks):
    tok, t = toks("collide")
    check_cases(tok, t, "collide")
    check_words(tok, t, "collide")       # a won id follows its winner, an absent id and the empty word's id are plain, "@@" continues


# ---- f. the snapshot against the live tables ------------------------------------------------------------------------------------
def check_grown(tok, t):
    assert tok.vocab_size() == t.size and tuple(tok._special_ids()[:4]) == t.ids and t.ids != t.snap_ids
    check_cases(tok, t, "grown")
    check_words(tok, t, "grown")         # a new "@@" word's id is plain, the moved word's old id and the old <mask> id continue
    cells = RT.word_rows("grown")[0][0]
    ids = as_rows([padded(t, cells, 24)])
    got = tok.mask_rows(ids, p=1.0)
    assert got["labels"][0, 8] == t.snap_ids[3] and got["labels"][0, 14] == t.snap_ids[2]      # the old ids are unprotected tokens
    assert got["labels"][0, 16] == -100 and got["input_ids"][0, 16] == t.mask and got["n_chosen"][0] == 18
    # windows and packs frame with the live ids
    bodies = bodies_of(t, RT.rows_of("grown", 65, 130, 3)) + [[t.snap_ids[2], t.snap_ids[3], 0, 1, 2, 3]]
    for L, s in ((16, 5), (64, 0)):
        got = tok.window_rows(bodies, L, s, framed=False)
        same(got, WO.batch(bodies, L, s, t.bos, t.eos, t.pad))
        assert (got["input_ids"][:, 0] == t.bos).all() and (got["input_ids"] == t.eos).sum() == len(got["doc"])
    same(tok.pack_rows(bodies, 64, framed=False), PO.batch(bodies, 64, t.bos, t.eos, t.pad))


def test_snapshot_taken_by_add_vocab_file(folder):
    """object A: the vocabulary grows before any call has touched the tables, and mask_rows is the first that does"""
    t, m = RT.grown(), RT.moved()
    tok = build(folder, m)
    tok.add_vocab_file(second_file(folder, t))
    R, L, p, seed = RT.cases("grown")[0]
    ids = as_rows(RT.rows_of("grown", R, L, seed))
    same(tok.mask_rows(ids, p=p, seed=seed), RT.mask_want(t, ids, p, seed))
    check_grown(tok, t)


def test_snapshot_taken_by_the_first_row_call(folder):
    """object B: infill_rows is the first call on a fresh object, then the vocabulary grows"""
    t, m = RT.grown(), RT.moved()
    tok = build(folder, m)
    R, L, p, seed = RT.cases("moved")[1]
    ids = as_rows(RT.rows_of("moved", R, L, seed))
    same(tok.infill_rows(ids, p=p, seed=seed), RT.infill_want(m, ids, p, seed))
    cells = RT.word_rows("grown")[0][0]
    before = tok.mask_rows(as_rows([padded(m, cells, 24)]), p=1.0)["labels"][0]
    assert before[8] == -100 and before[14] == -100 and before[16] == t.mask           # <mask> and </s> have not moved yet
    tok.add_vocab_file(second_file(folder, t))
    check_grown(tok, t)


# ---- g. the 100 k custom tables end to end ---------------------------------------------------------------------------------------
def test_custom_tables_end_to_end(toks):
    tok, t = toks("custom")
    ref = O.Tables(t.vocab, t.merges, t.specials)
    texts = RT.custom_texts()
    bodies = [O.encode_words(s, ref)[0] for s in texts]
    L = RT.CUSTOM_L
    want = PO.batch(bodies, L, t.bos, t.eos, t.pad)
    got = tok.encode_packs(texts, L)
    same(got, want)
    assert (got["input_ids"] > 65535).any()
    ids = np.concatenate([got["input_ids"], as_rows(RT.custom_extra_rows())])
    p, seed = RT.CUSTOM_CASE
    for ww in (True, False):
        check_mask(tok, t, ids, p, seed, whole_word=ww)
        check_infill(tok, t, ids, p, seed, whole_word=ww)
    flat, off = tok.unpack_rows(got)
    segs = [flat[off[i]:off[i + 1]].tolist() for i in range(len(texts))]
    assert segs == [PO.segment(b, L, t.bos, t.eos) for b in bodies]
    assert tok.decode_batch(segs) == [O.decode(s, ref) for s in segs]
