"""GPU: what `return_offset=True` rests on -- gz_word_token_counts over the word records a GZ_KEEP_WORDS call leaves behind --
against the Python oracle, on every kernel path that writes such a record and through every branch of the host code that reads
them.  Integer work: every comparison is ==.  The inputs and what the oracle says about them come from offset_oracle.py (built once
per process; test_offset_inputs.py says on the CPU that they are what these tests assume).

  raw counts     counts[] and doc_first[] after ctx.encode(..., GZ_KEEP_WORDS): words of 1 .. 2 500 symbols placed five ways, document
                 boundaries at tile and block edges, a corpus of 132 369 words; single texts and pairs, four layouts, whole-word
                 tables on and off
  offsets        encode_batch(..., return_offset=True) against O.call(...)["offset"], pair rule included
  g3 rows        the reference's own return_offset rows through the batch call
  other kernels  far records beside near ones, the merge kernel's two instances, one stream, the chained scan, two sub-batches
  the law        documents that are not UTF-8: counts add up to the row, runs agree, the neighbours are untouched
  the ABI        capacity, refusals, stale records after a CSR call, empty inputs
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gz_oracle as O
import offset_oracle as X

pytestmark = pytest.mark.gpu

DEFAULTS = dict(near_limit=1 << 25, m2_split_min=65536, m2_split_always=0, side=1, brk_side=1, scan_multi=8192, sub_batches=1)


@pytest.fixture(scope="module")
def native():
    from genz_tokenize import _native
    return _native


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    t = Tokenize()
    t._sync_tables()
    return t


@pytest.fixture(scope="module")
def tok_sw():
    """A tokenizer of its own for the tests that set switches on their context."""
    from genz_tokenize import Tokenize
    t = Tokenize()
    t._sync_tables()
    return t


def _group(name):
    return {"ladder": (X.ladder(),), "edges": X.edges(), "corpus": (X.corpus(),)}[name]


def _keep_call(native, ctx, batch, pair, layout=(None, True, True), word_table=True):
    ml, pad, tr = layout
    ta, oa = batch.packed(0)
    tb, ob = batch.packed(1) if pair else (None, None)
    flags = native.GZ_KEEP_WORDS | (0 if word_table else native.GZ_NO_WORD_TABLE)
    return ctx.encode(ta, oa, tb, ob, ml, pad, tr, flags)


def _check_raw(native, ctx, batch, pair, layouts=X.LAYOUTS, tables=(True, False)):
    n = len(batch.docs)
    for layout in layouts:
        for wt in tables:
            _keep_call(native, ctx, batch, pair, layout, wt)
            for which in ((0, 1) if pair else (0,)):
                want_counts, want_first = batch.words(which)
                counts, first = ctx.word_token_counts(which, n, 1 << 16)
                what = (batch.name, pair, layout, wt, which)
                assert counts.dtype == np.int32 and first.dtype == np.int64
                assert np.array_equal(first, want_first), (what, np.flatnonzero(first != want_first)[:5])
                assert len(counts) == len(want_counts), what
                bad = np.flatnonzero(counts != want_counts)
                assert bad.size == 0, (what, bad[:5], counts[bad[:5]], want_counts[bad[:5]])


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("name", ["ladder", "edges", "corpus"])
def test_counts_and_first_words_equal_the_oracle(native, tok, name, pair):
    """gz_word_token_counts after a GZ_KEEP_WORDS call: counts element for element, doc_first whole."""
    for batch in _group(name):
        _check_raw(native, tok._ctx, batch, pair)


def _flat_offsets(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return np.array([e for x in lists for e in x], dtype=np.int64).reshape(-1, 2), off


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("name", ["ladder", "edges", "corpus"])
def test_encode_batch_offsets_equal_the_oracle_call(tok, name, pair):
    """encode_batch(..., return_offset=True): every document's list is O.call(...)["offset"]; pairs get the entry-count shift."""
    for batch in _group(name):
        want = batch.offsets(pair)
        flat, off = _flat_offsets(want)
        for ml, pad, tr in X.LAYOUTS:
            for wt in (True, False):
                r = tok.encode_batch(batch.docs, batch.pair_docs if pair else None, max_len=ml, padding=pad, truncation=tr,
                                     word_table=wt, return_offset=True)
                what = (batch.name, pair, ml, pad, tr, wt)
                assert r["offset"].dtype == np.int32 and r["offset"].shape == (int(off[-1]), 2), what
                assert np.array_equal(r["offset_off"], off), what
                bad = np.flatnonzero((r["offset"] != flat).any(axis=1))
                assert bad.size == 0, (what, bad[:5], r["offset"][bad[:5]], flat[bad[:5]])
                for i in (0, len(want) // 2, len(want) - 1):              # ... and in the list form offsets_of hands out
                    assert tok.offsets_of(r, i) == want[i], (what, i)


def test_reference_rows_with_offsets_through_the_batch_call(tok):
    """The g3 rows the reference made with return_offset=True, grouped by keyword arguments, through encode_batch."""
    compared = raised = 0
    for (nargs, ml, pad, tr), rows in X.g3_offset_groups().items():
        texts = [r["args"][0] for r in rows]
        pairs = [r["args"][1] for r in rows] if nargs == 2 else None
        out = tok.encode_batch(texts, pairs, max_len=ml, padding=pad, truncation=tr, return_offset=True)
        assert out["offset"].dtype == np.int32 and len(out["offset_off"]) == len(rows) + 1
        assert out["offset"].shape == (int(out["offset_off"][-1]), 2) and out["offset_off"][0] == 0
        for i, r in enumerate(rows):
            if "raises" in r:
                assert out["status"][i] == 1
                raised += 1
                continue
            assert out["status"][i] == 0
            assert [list(e) for e in tok.offsets_of(out, i)] == r["result"]["offset"], (nargs, ml, pad, tr, i)
            compared += 1
    assert compared >= 300 and raised == 40


@pytest.fixture()
def switches(native, tok_sw):
    """set(**kv) on tok_sw's context; every switch is back at its default when the test ends."""
    def set_(**kv):
        for k, v in kv.items():
            native.debug_set(k, v, tok_sw._ctx)
    try:
        yield set_
    finally:
        set_(**DEFAULTS)


@pytest.mark.parametrize("sw", [dict(near_limit=300), dict(m2_split_min=1, m2_split_always=1), dict(side=0, brk_side=0), dict(scan_multi=0)],
                         ids=["far_records", "merge_two_instances", "one_stream", "chained_scan"])
def test_other_kernels_leave_the_same_records(native, tok_sw, switches, sw):
    switches(**sw)
    for pair in (False, True):
        _check_raw(native, tok_sw._ctx, X.ladder(), pair)
        _check_raw(native, tok_sw._ctx, X.corpus(), pair, layouts=X.LAYOUTS[:1])


def _raw(native, ctx, which, n_docs, capacity):
    """gz_word_token_counts itself, into arrays filled with a mark: (rc, *n_words, counts, doc_first)."""
    counts = np.full(max(capacity, 0) + 8, -7, dtype=np.int32)
    first = np.full(n_docs + 1, -7, dtype=np.int64)
    nw = C.c_int64(-7)
    rc = ctx.lib.gz_word_token_counts(ctx.handle, which, C.c_void_p(counts.ctypes.data), capacity, C.c_void_p(first.ctypes.data), C.byref(nw))
    return rc, nw.value, counts, first


def test_two_sub_batches_report_the_whole_word_total(native, tok_sw, switches):
    """sub_batches = 2 on the dense corpus: word indices of the second half start behind the first half's words, and a capacity
    error names the words of BOTH halves, so that the shim's one retry fits (132 369 words: more than its first 65 536)."""
    b = X.corpus()
    ctx = tok_sw._ctx
    switches(sub_batches=2)
    for pair in (False, True):
        _check_raw(native, ctx, b, pair, layouts=X.LAYOUTS[:1])
        for which in ((0, 1) if pair else (0,)):
            total = len(b.words(which)[0])
            for cap in (0, 1 << 16, total - 1):
                rc, nw, counts, first = _raw(native, ctx, which, len(b.docs), cap)
                assert (rc, nw) == (native.GZ_E_CAPACITY, total), (pair, which, cap)
    r = tok_sw.encode_batch(b.docs, max_len=48, return_offset=True)
    flat, off = _flat_offsets(b.offsets(False))
    assert np.array_equal(r["offset_off"], off) and np.array_equal(r["offset"], flat)


def test_three_sub_batches_are_refused_and_the_context_goes_on(native, tok_sw, switches):
    b = X.corpus()
    ctx = tok_sw._ctx
    switches(sub_batches=3)
    _keep_call(native, ctx, b, False, X.LAYOUTS[0])
    rc, nw, counts, first = _raw(native, ctx, 0, len(b.docs), 1 << 18)
    assert rc == native.GZ_E_INVALID and nw == -7 and np.all(counts == -7) and np.all(first == -7)
    with pytest.raises(native.GzError) as e:
        ctx.word_token_counts(0, len(b.docs), 1 << 16)
    assert e.value.code == native.GZ_E_INVALID and "sub-batches" in str(e.value)
    switches(sub_batches=1)
    _check_raw(native, ctx, b, False, layouts=X.LAYOUTS[:1], tables=(True,))
    _plain_call_matches(tok_sw)


def test_counts_of_documents_that_are_not_utf8(native, tok):
    """Where the oracle is silent (bytes that are no UTF-8) the law still holds: a document's counts add up to its row without
    bos and eos, two runs agree, and the well-formed documents between them count as the oracle says."""
    docs, good, well = X.not_utf8()
    text, offs = X.pack(docs)
    n = len(docs)
    ctx = tok._ctx
    want_counts, want_first = well.words(0)
    for wt in (True, False):
        flags = native.GZ_KEEP_WORDS | (0 if wt else native.GZ_NO_WORD_TABLE)
        runs = []
        for _ in range(2):
            r = ctx.encode(text, offs, None, None, None, True, True, flags)
            counts, first = ctx.word_token_counts(0, n, 1 << 16)
            runs.append((counts, first, r["row_off"].copy()))
        (counts, first, row_off), (counts2, first2, row_off2) = runs
        assert np.array_equal(counts, counts2) and np.array_equal(first, first2) and np.array_equal(row_off, row_off2)
        # (a "word" of nothing but stray continuation bytes has no symbol and so no piece: counts of 0 occur here, and only here)
        assert first[0] == 0 and first[-1] == len(counts) and np.all(np.diff(first) >= 0) and counts.min() >= 0
        cs = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        per_doc = cs[first[1:]] - cs[first[:-1]]
        bad = np.flatnonzero(per_doc != np.diff(row_off) - 2)
        assert bad.size == 0, (wt, bad[:5], per_doc[bad[:5]], np.diff(row_off)[bad[:5]])
        nw = np.diff(first)
        assert np.array_equal(nw[good], np.diff(want_first)), wt
        is_good = np.zeros(n, dtype=bool)
        is_good[good] = True
        assert np.array_equal(counts[np.repeat(is_good, nw)], want_counts), wt


@functools.lru_cache(maxsize=None)
def _plain():
    docs = X.edges()[0].docs + ["", "xin chào việt nam", "x" * 70 + " y"]
    return docs, O.call_batch(X.tables(), docs, None, 32, True, True)


def _plain_call_matches(t):
    """A call that keeps nothing, against the oracle: the context is as good as before."""
    docs, (I, M, _, _, _) = _plain()
    out = t.encode_batch(docs, max_len=32)
    assert out["input_ids"].tolist() == I and out["attention_mask"].tolist() == M


def test_capacity_is_reported_exactly(native, tok):
    b = X.ladder()
    ctx, n = tok._ctx, len(b.docs)
    want_counts, want_first = b.words(0)
    total = len(want_counts)
    _keep_call(native, ctx, b, False)
    rc, nw, counts, first = _raw(native, ctx, 0, n, total - 1)
    assert (rc, nw) == (native.GZ_E_CAPACITY, total) and np.all(counts == -7)
    rc, nw, counts, first = _raw(native, ctx, 0, n, 0)
    assert (rc, nw) == (native.GZ_E_CAPACITY, total) and np.all(counts == -7)
    rc, nw, counts, first = _raw(native, ctx, 0, n, total)
    assert (rc, nw) == (native.GZ_OK, total)
    assert np.array_equal(counts[:total], want_counts) and np.all(counts[total:] == -7) and np.array_equal(first, want_first)
    # a batch without a word: capacity 0 is enough
    ws = X.Batch("spaces", list(X.WS_DOCS) + [""])
    _keep_call(native, ctx, ws, False)
    rc, nw, counts, first = _raw(native, ctx, 0, len(ws.docs), 0)
    assert (rc, nw) == (native.GZ_OK, 0) and np.all(first == 0) and np.all(counts == -7)


def _refused(native, ctx, which, n_docs):
    rc, nw, counts, first = _raw(native, ctx, which, n_docs, 1 << 16)
    assert rc == native.GZ_E_INVALID and nw == -7 and np.all(counts == -7) and np.all(first == -7)


def test_refusals_leave_the_context_usable(native, tok):
    b = X.edges()[4]
    ctx, n = tok._ctx, len(b.docs)
    _keep_call(native, ctx, b, False)
    _refused(native, ctx, 1, n)                                   # text B of a call that had none
    _plain_call_matches(tok)
    _refused(native, ctx, 0, n)                                   # the last call kept nothing
    ta, oa = b.packed(0)
    ctx.encode(ta, oa, None, None, 16, True, True, 0)
    _refused(native, ctx, 0, n)
    _plain_call_matches(tok)
    _check_raw(native, ctx, b, True, layouts=X.LAYOUTS[:2])


def test_records_do_not_outlive_a_csr_call(native, tok):
    """The CSR host path and the large dense host call run their sub-batches through the same per-text workspace: after them the
    records of an earlier GZ_KEEP_WORDS call are gone, and gz_word_token_counts says so."""
    small, big = X.edges()[4], X.corpus()
    ctx = tok._ctx
    ta, oa = big.packed(0)
    _keep_call(native, ctx, small, False)
    csr = tok.encode_packed_csr(ta, oa, 48)
    _refused(native, ctx, 0, len(small.docs))
    _plain_call_matches(tok)
    _keep_call(native, ctx, small, True)
    dense = tok.encode_packed(ta, oa, max_len=48)                 # more than 1 MiB: the dense host call that pads on the host
    _refused(native, ctx, 0, len(small.docs))
    _refused(native, ctx, 1, len(small.docs))
    _plain_call_matches(tok)
    # both calls computed what they should have
    I = O.call_batch(X.tables(), big.docs[:50], None, 48, True, True)[0]
    assert dense["input_ids"][:50].tolist() == I
    lens = np.asarray(csr["n_real"][:50], dtype=np.int64)
    got = np.asarray(csr["tokens"][:int(lens.sum())], dtype=np.int64).tolist()
    assert got == [v for row, k in zip(I, lens) for v in row[:k]]
    _check_raw(native, ctx, small, False, layouts=X.LAYOUTS[:1])


def test_empty_inputs(native, tok):
    big = X.ladder()
    ctx = tok._ctx
    for pairs in (None, []):
        _keep_call(native, ctx, big, pairs is not None)           # records of many documents are around ...
        r = tok.encode_batch([], pairs, return_offset=True)      # ... and a call without texts must not ask for them
        assert r["offset"].dtype == np.int32 and r["offset"].shape == (0, 2)
        assert r["offset_off"].dtype == np.int64 and r["offset_off"].tolist() == [0]
        _refused(native, ctx, 0, len(big.docs))                   # the empty call was an encode call too
        r = tok.encode_batch([], pairs, max_len=8, return_offset=True)
        assert r["offset"].shape == (0, 2) and r["offset_off"].tolist() == [0] and r["input_ids"].shape == (0, 8)
        _plain_call_matches(tok)
    assert tok("", return_offset=True)["offset"] == [(0, 0), (1, 1)]
    assert tok.encode("", True) == O.encode("", X.tables(), True)
    r = tok.encode_batch(["", " ", ""], ["", "", "\n"], return_offset=True)
    assert [tok.offsets_of(r, i) for i in range(3)] == [[(0, 0), (1, 1), (2, 2), (3, 3)]] * 3
    _plain_call_matches(tok)
