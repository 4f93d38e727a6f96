"""GPU: word spans, word ids and aligned labels (gz_word_spans, gz_align_rows, gz_span_labels, each with its _device form;
Tokenize.word_spans, align_rows, span_labels, encode_aligned) against the plain-Python oracle of align_oracle.py.  Integer work: every
comparison is ==.  test_align_inputs.py says on the CPU that the inputs hold the cases these tests assume.

  spans          both units: document boundaries at tile and block edges, words of 1 .. 2 500 symbols, runs of empty documents, two- and
                 three-byte spaces, 2-, 3- and 4-byte characters across a tile edge, lone surrogates, line feeds, N = 0, the sizing pass,
                 GZ_E_CAPACITY at W - 1, a device call whose offsets do not start at 0; word_off == doc_first of gz_word_token_counts
  align          documents of 1 .. 2 500 words, max_len 3 .. 48, T around room, cuts at and inside a word, empty documents, rows repeated
                 and out of order, starts mid-word and past the end, every continuation mode, R = 0, each output left out; the law that
                 ties word_ids to the reference's return_offset; windows against encode_windows and join_windows
  span labels    touching, empty, reversed, whitespace-only, past-the-end, nested, overlapping and unsorted marks; both schemes; S = 0
  encode_aligned end to end on 300 noisy documents, dense and in windows
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import align_oracle as A
import gz_oracle as O
import offset_oracle as X

pytestmark = pytest.mark.gpu

UNITS = {"char": 0, "byte": 1}
MARK = -77                                                             # what an untouched output cell holds


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


@functools.lru_cache(maxsize=None)
def _want_spans(name, unit):
    return A.batch_spans(A.span_batches()[name], unit)


@functools.lru_cache(maxsize=None)
def _corpus_words():
    """(counts per document, spans per document) of the noisy corpus, by the oracle"""
    docs = A.noisy_corpus()
    with X._bpe_once():
        counts = [A.piece_counts(d, X.tables()) for d in docs]
    return counts, [A.spans(d) for d in docs]


def _err(ctx):
    return ctx.lib.gz_last_error(ctx.handle).decode("utf-8", "replace")


class Dev:
    """device copies of host arrays, freed together"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def up(self, arr, pad=0):
        arr = np.ascontiguousarray(arr)
        d = self.ctx.alloc(arr.nbytes + pad + 64)
        self.bufs.append(d)
        if arr.nbytes:
            self.ctx.h2d(d + pad, arr)
        return d

    def new(self, nbytes):
        d = self.ctx.alloc(nbytes + 64)
        self.bufs.append(d)
        return d

    def down(self, d, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            self.ctx.d2h(out, d)
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.bufs:
            self.ctx.free(d)


# ---- spans -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", ["char", "byte"])
def test_spans_equal_the_oracle(tok, unit):
    for name, docs in A.span_batches().items():
        text, off = A.pack(docs)
        span, word_off = tok._ctx.word_spans(text, off, UNITS[unit])
        want, want_off = _want_spans(name, unit)
        assert span.dtype == np.int32 and word_off.dtype == np.int64
        assert np.array_equal(word_off, want_off), (name, np.flatnonzero(word_off != want_off)[:5])
        assert span.shape == want.shape, name
        bad = np.flatnonzero((span != want).any(axis=1))
        assert bad.size == 0, (name, unit, bad[:5], span[bad[:5]], want[bad[:5]])


def test_python_word_spans(tok):
    docs = list(A.SMALL_DOCS)
    for unit in UNITS:
        span, word_off = tok.word_spans(docs, unit=unit)
        want, want_off = A.batch_spans(docs, unit)
        assert np.array_equal(span, want) and np.array_equal(word_off, want_off), unit
    span, word_off = tok.word_spans([])
    assert span.shape == (0, 2) and word_off.tolist() == [0]
    for stride in (None, 2):                                             # no texts at all: empty rows, not an error
        none = tok.encode_aligned([], 8, stride=stride)
        assert none["word_ids"].shape == (0, 8) and none["input_ids"].shape == (0, 8) and none["word_off"].tolist() == [0]


def test_word_off_equals_doc_first_of_the_piece_counts(native, tok):
    for name, docs in A.span_batches().items():
        if not docs:
            continue
        text, off = A.pack(docs)
        tok._ctx.encode(text, off, None, None, None, False, False, native.GZ_KEEP_WORDS)
        counts, first = tok._ctx.word_token_counts(0, len(docs), 1 << 16)
        _, word_off = tok._ctx.word_spans(text, off, 0)
        assert np.array_equal(word_off, first), name
        assert len(counts) == int(word_off[-1]), name


def test_sizing_pass_and_capacity(native, tok):
    ctx = tok._ctx
    docs = A.span_batches()["edges[+0,cut]"]
    text, off = A.pack(docs)
    want, want_off = _want_spans("edges[+0,cut]", "char")
    W, n = len(want), len(docs)
    total = C.c_int64(-1)
    word_off = np.full(n + 1, MARK, dtype=np.int64)
    head = (ctx.handle, native._ptr(text), native._ptr(off), n, 0)
    assert ctx.lib.gz_word_spans(*head, None, native._ptr(word_off), 0, C.byref(total)) == native.GZ_OK
    assert total.value == W and np.array_equal(word_off, want_off)
    span = np.full((W, 2), MARK, dtype=np.int32)
    word_off[:] = MARK
    total = C.c_int64(-1)
    assert ctx.lib.gz_word_spans(*head, native._ptr(span), native._ptr(word_off), W - 1, C.byref(total)) == native.GZ_E_CAPACITY
    assert "capacity is %d" % (W - 1) in _err(ctx)
    assert total.value == W and np.array_equal(word_off, want_off) and bool((span == MARK).all())
    assert ctx.lib.gz_word_spans(*head, native._ptr(span), native._ptr(word_off), W, C.byref(total)) == native.GZ_OK
    assert np.array_equal(span, want)
    with Dev(ctx) as D:                                                  # the device form says the same
        d_text, d_off, d_woff, d_span = D.up(text), D.up(off), D.new(8 * (n + 1)), D.up(np.full((W, 2), MARK, dtype=np.int32))
        assert ctx.word_spans_device(d_text, d_off, n, len(text), 0, 0, d_woff, 0) == W
        with pytest.raises(native.GzError) as e:
            ctx.word_spans_device(d_text, d_off, n, len(text), 0, d_span, d_woff, W - 1)
        assert e.value.code == native.GZ_E_CAPACITY and e.value.total == W
        assert bool((D.down(d_span, (W, 2), np.int32) == MARK).all())
        assert np.array_equal(D.down(d_woff, n + 1, np.int64), want_off)


@pytest.mark.parametrize("unit", ["char", "byte"])
def test_device_form_with_offsets_that_do_not_start_at_0(tok, unit):
    ctx = tok._ctx
    for name in ("straddle", "small", "edges[-1,space]"):
        docs = A.span_batches()[name]
        text, off = A.pack(docs)
        want, want_off = _want_spans(name, unit)
        W, n, shift = len(want), len(docs), 37
        junk = np.frombuffer(b"\xe2\x80 kh\xc3\xb4ng \xf0\x9f\x98" * 3, dtype=np.uint8)[:shift]          # ends inside a character
        with Dev(ctx) as D:
            d_text = D.up(np.concatenate([junk, text, junk]))
            d_off, d_woff, d_span = D.up(off + shift), D.new(8 * (n + 1)), D.new(8 * W)
            assert ctx.word_spans_device(d_text, d_off, n, len(text), UNITS[unit], d_span, d_woff, W) == W
            assert np.array_equal(D.down(d_woff, n + 1, np.int64), want_off), name
            assert np.array_equal(D.down(d_span, (W, 2), np.int32), want), name


def test_span_refusals(native, tok):
    ctx = tok._ctx
    text, off = A.pack(["xin chao", "a"])
    woff, total = np.zeros(3, dtype=np.int64), C.c_int64()
    p = native._ptr

    def call(text=text, off=off, n=2, unit=0, cap=0):
        return ctx.lib.gz_word_spans(ctx.handle, p(text), p(off), n, unit, None, p(woff), cap, C.byref(total))
    said = []
    for kw, want in ((dict(n=-1), "word spans need n_docs >= 0"), (dict(unit=2), "word spans need unit 0 (code points) or 1 (bytes)"),
                     (dict(cap=-1), "word spans need capacity_words >= 0"), (dict(off=np.array([0, 9, 8], dtype=np.int64)), "text offsets must not decrease"),
                     (dict(off=np.array([5, 5, 1], dtype=np.int64)), "bad text offsets")):
        assert call(**kw) == native.GZ_E_INVALID, kw
        assert want in _err(ctx), kw
        said.append(want)
    assert len(set(said)) == len(said)
    assert call() == native.GZ_OK and total.value == 3


# ---- align -----------------------------------------------------------------------------------------------------------------------
def _flat(per_doc, dtype=np.int32):
    off = np.zeros(len(per_doc) + 1, dtype=np.int64)
    for i, c in enumerate(per_doc):
        off[i + 1] = off[i] + len(c)
    return np.array([x for c in per_doc for x in c], dtype=dtype), off


@functools.lru_cache(maxsize=None)
def _align_case():
    """counts, labels per document and the rows of the align tests: every document at start 0 in order, then rows repeated and out of
    order with starts mid-word, at the last token, at T and past it"""
    r = random.Random(7)
    counts = A.synthetic_counts()
    labels = [[r.choice((-100, -1, 0, 1, 2, 3, 4, 5, 9, 1000)) for _ in c] for c in counts]
    rows = []
    for d, c in enumerate(counts):
        T = sum(c)
        for s in {1, T // 2, max(T - 1, 0), T, T + 5}:
            rows.append((d, s))
    for d, c in enumerate(counts):
        if len(c) == 2500:
            rows += [(d, s) for s in r.sample(range(sum(c)), 12)]
    r.shuffle(rows)
    rows = [(d, 0) for d in range(len(counts))] + rows + rows[:7]
    return counts, labels, tuple(rows)


@pytest.mark.parametrize("max_len", A.ALIGN_LENS)
def test_align_rows_equal_the_oracle(tok, max_len):
    counts, labels, rows = _align_case()
    flat, off = _flat(counts)
    flat_l, _ = _flat(labels)
    row_doc = np.array([d for d, _ in rows], dtype=np.int32)
    row_start = np.array([s for _, s in rows], dtype=np.int32)
    cont_map = np.array([7, -100, 2, 11, 0, 6], dtype=np.int32)
    for mode, name in ((0, "ignore"), (1, "same"), (2, "map")):
        want_w, want_l, want_n = A.rows(counts, row_doc.tolist(), row_start.tolist(), max_len, labels, name, cont_map.tolist(), -100)
        got = tok._ctx.align_rows(flat, off, max_len, flat_l, row_doc, row_start, mode, cont_map if mode == 2 else None, -100)
        assert np.array_equal(got["n_real"], np.array(want_n, dtype=np.int32)), name
        for key, want in (("word_ids", want_w), ("labels", want_l)):
            want = np.array(want, dtype=np.int32)
            bad = np.flatnonzero((got[key] != want).any(axis=1))
            assert bad.size == 0, (name, key, bad[:3], rows[bad[0]], got[key][bad[0]], want[bad[0]])
    # another ignore value, and the rows in their own order with no row arrays at all
    n = len(counts)
    want_w, want_l, want_n = A.rows(counts, range(n), [0] * n, max_len, labels, "ignore", None, 12345)
    got = tok._ctx.align_rows(flat, off, max_len, flat_l, None, None, 0, None, 12345)
    assert np.array_equal(got["word_ids"], np.array(want_w, dtype=np.int32)) and np.array_equal(got["labels"], np.array(want_l, dtype=np.int32))
    assert got["n_real"].tolist() == want_n
    # row_start alone: row r is document r
    starts = np.array([i % 3 for i in range(n)], dtype=np.int32)
    want_w, _, want_n = A.rows(counts, range(n), starts.tolist(), max_len)
    got = tok._ctx.align_rows(flat, off, max_len, None, None, starts, 0, None, -100)
    assert "labels" not in got and np.array_equal(got["word_ids"], np.array(want_w, dtype=np.int32)) and got["n_real"].tolist() == want_n


@pytest.mark.parametrize("max_len", [32, 33, 64, 65, 128, 257, 1024, 1025])
def test_align_rows_at_the_kernel_edges(tok, max_len):
    """the bitmap of a row grows a word at every 32 cells, the rows a block takes change with max_len, and rows of more than 1 024
    cells take the kernel that searches: the same rows through each"""
    counts, labels, rows = _align_case()
    rows = rows[::3]
    flat, off = _flat(counts)
    flat_l, _ = _flat(labels)
    row_doc = np.array([d for d, _ in rows], dtype=np.int32)
    row_start = np.array([s for _, s in rows], dtype=np.int32)
    cont_map = np.array([7, -100, 2, 11, 0, 6], dtype=np.int32)
    want_w, want_l, want_n = A.rows(counts, row_doc.tolist(), row_start.tolist(), max_len, labels, "map", cont_map.tolist(), -100)
    got = tok._ctx.align_rows(flat, off, max_len, flat_l, row_doc, row_start, 2, cont_map, -100)
    assert got["n_real"].tolist() == want_n
    assert np.array_equal(got["word_ids"], np.array(want_w, dtype=np.int32))
    assert np.array_equal(got["labels"], np.array(want_l, dtype=np.int32))


def test_align_outputs_left_out_and_no_rows(native, tok):
    counts, labels, rows = _align_case()
    flat, off = _flat(counts)
    flat_l, _ = _flat(labels)
    row_doc = np.array([d for d, _ in rows[:40]], dtype=np.int32)
    row_start = np.array([s for _, s in rows[:40]], dtype=np.int32)
    full = tok._ctx.align_rows(flat, off, 16, flat_l, row_doc, row_start, 1, None, -100)
    for k, key in enumerate(("word_ids", "labels", "n_real")):
        want = [True, True, True]
        want[k] = False
        got = tok._ctx.align_rows(flat, off, 16, flat_l, row_doc, row_start, 1, None, -100, want=tuple(want))
        assert key not in got and sorted(got) == sorted(set(full) - {key})
        for other in got:
            assert np.array_equal(got[other], full[other]), (key, other)
    assert tok._ctx.align_rows(flat, off, 16, flat_l, row_doc, row_start, 1, None, -100, want=(False, False, False)) == {}
    none = tok._ctx.align_rows(flat, off, 16, flat_l, row_doc[:0], row_start[:0], 0, None, -100)
    assert none["word_ids"].shape == (0, 16) and none["labels"].shape == (0, 16) and none["n_real"].shape == (0,)
    empty = tok._ctx.align_rows(flat[:0], off[:1], 16, None, None, None, 0, None, -100)                  # no documents at all
    assert empty["word_ids"].shape == (0, 16)
    got = tok.align_rows(flat, off, 16, word_labels=flat_l, row_doc=row_doc, row_start=row_start, continuation="same")
    assert all(np.array_equal(got[k], full[k]) for k in full)


def test_align_device_form(tok):
    ctx = tok._ctx
    counts, labels, rows = _align_case()
    flat, off = _flat(counts)
    flat_l, _ = _flat(labels)
    row_doc = np.array([d for d, _ in rows], dtype=np.int32)
    row_start = np.array([s for _, s in rows], dtype=np.int32)
    cont_map = np.array([3, 2, 1], dtype=np.int32)
    R, L, lead = len(rows), 16, 5
    want = ctx.align_rows(flat, off, L, flat_l, row_doc, row_start, 2, cont_map, -100)
    with Dev(ctx) as D:                                                  # the counts behind five foreign words: absolute offsets
        d_counts, d_labels = D.up(np.concatenate([np.full(lead, 99, dtype=np.int32), flat])), D.up(np.concatenate([np.full(lead, 99, dtype=np.int32), flat_l]))
        d_off, d_doc, d_start, d_map = D.up(off + lead), D.up(row_doc), D.up(row_start), D.up(cont_map)
        d_w, d_l, d_n = D.new(4 * R * L), D.new(4 * R * L), D.new(4 * R)
        ctx.align_rows_device(d_counts, d_off, len(counts), len(flat), d_doc, d_start, R, L, d_labels, 2, d_map, len(cont_map), -100, d_w, d_l, d_n)
        assert np.array_equal(D.down(d_w, (R, L), np.int32), want["word_ids"])
        assert np.array_equal(D.down(d_l, (R, L), np.int32), want["labels"])
        assert np.array_equal(D.down(d_n, R, np.int32), want["n_real"])
        # outputs that do not start on a 16-byte boundary: one cell a lane, the same cells
        d_w, d_l = D.new(4 * R * L + 16), D.new(4 * R * L + 16)
        ctx.align_rows_device(d_counts, d_off, len(counts), len(flat), d_doc, d_start, R, L, d_labels, 2, d_map, len(cont_map), -100, d_w + 4, d_l + 8, 0)
        assert np.array_equal(D.down(d_w + 4, (R, L), np.int32), want["word_ids"])
        assert np.array_equal(D.down(d_l + 8, (R, L), np.int32), want["labels"])


def test_align_refusals(native, tok):
    ctx, p = tok._ctx, native._ptr
    counts, off = np.array([1, 2, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64)
    labels, cmap = np.array([1, 2, 3], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    out, out_l = np.zeros((4, 8), dtype=np.int32), np.zeros((4, 8), dtype=np.int32)

    def call(counts=counts, off=off, n=2, doc=None, start=None, R=2, L=8, wl=labels, cont=0, cm=None, n_map=0, lab=out_l):
        return ctx.lib.gz_align_rows(ctx.handle, p(counts), p(off), n, p(doc), p(start), R, L, p(wl), cont, p(cm), n_map, -100, p(out), p(lab), None)
    i32 = lambda *a: np.array(a, dtype=np.int32)                         # noqa: E731
    said = []
    for kw, want in ((dict(counts=i32(1, 0, 1)), "a word's piece count is below 1"),
                     (dict(off=np.array([0, 3, 2], dtype=np.int64)), "word offsets must not decrease"),
                     (dict(off=np.array([4, 4, 3], dtype=np.int64)), "bad word offsets"),
                     (dict(doc=i32(0, 2)), "a row_doc lies outside [0, n_docs)"), (dict(doc=i32(-1, 0)), "a row_doc lies outside [0, n_docs)"),
                     (dict(start=i32(0, -1)), "a row_start is negative"), (dict(L=2), "aligned rows need max_len >= 3"),
                     (dict(wl=None), "aligned rows need word_labels where labels are asked for"),
                     (dict(cont=2), "aligned rows in map mode need a cont_map of at least one entry"),
                     (dict(cont=2, cm=cmap, n_map=0), "aligned rows in map mode need a cont_map of at least one entry"),
                     (dict(cont=3), "aligned rows need continuation 0 (ignore), 1 (same) or 2 (map)"),
                     (dict(R=3), "aligned rows without row_doc need n_rows == n_docs"), (dict(R=-1, doc=i32(0)), "aligned rows need n_docs >= 0 and n_rows >= 0")):
        assert call(**kw) == native.GZ_E_INVALID, kw
        assert want in _err(ctx), (kw, _err(ctx))
        said.append(want)
    assert len(set(said)) == 11
    assert call() == native.GZ_OK and call(cont=2, cm=cmap, n_map=2) == native.GZ_OK and call(wl=None, lab=None) == native.GZ_OK


def test_word_ids_are_the_columns_of_return_offset(tok):
    """on rows long enough to hold a document whole, the columns where word_ids == j are exactly offset[j + 1] of return_offset"""
    docs = list(A.noisy_corpus()[:60]) + ["", "a\n b", "xin"]
    ref = tok.encode_batch(docs, return_offset=True)
    L = int(np.diff(ref["row_off"]).max())
    got = tok.encode_aligned(docs, L)
    assert np.array_equal(got["input_ids"], tok.encode_batch(docs, max_len=L)["input_ids"])
    for i in range(len(docs)):
        off = tok.offsets_of(ref, i)
        assert len(off) - 2 == int(got["word_off"][i + 1] - got["word_off"][i])
        for j, (first, last) in enumerate(off[1:-1]):
            assert np.flatnonzero(got["word_ids"][i] == j).tolist() == list(range(first, last + 1)), (i, j)
        assert int((got["word_ids"][i] >= 0).sum()) == off[-1][0] - 1


@pytest.mark.parametrize("max_len,stride", [(16, 3), (3, 0), (48, 45), (4, 1)])
def test_windows_equal_encode_windows_and_stitch(tok, max_len, stride):
    docs = list(A.noisy_corpus()[:40]) + ["", "xin"]
    counts = _corpus_words()[0][:40] + [[], [1]]
    got = tok.encode_aligned(docs, max_len, stride=stride)
    win = tok.encode_windows(docs, max_len, stride)
    for a, b in (("input_ids", "input_ids"), ("attention_mask", "attention_mask"), ("n_real", "n_real"), ("doc", "doc"), ("start", "start"),
                 ("win_off", "win_off")):
        assert np.array_equal(got[a], win[b]), a
    assert got["word_tokens"].tolist() == [c for d in counts for c in d]
    flat, row_off = tok.join_windows(dict(input_ids=got["word_ids"], n_real=got["n_real"], win_off=got["win_off"]), stride)
    for i, c in enumerate(counts):
        assert flat[row_off[i]:row_off[i + 1]].tolist() == [j for j, k in enumerate(c) for _ in range(k)], i
    want_w, _, want_n = A.rows(counts, got["doc"].tolist(), got["start"].tolist(), max_len)
    assert np.array_equal(got["word_ids"], np.array(want_w, dtype=np.int32)) and got["n_real"].tolist() == want_n


# ---- span labels -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _label_case():
    r = random.Random(13)
    docs = list(A.noisy_corpus()[:40])
    spans = [A.spans(d) for d in docs]
    marks = [A.random_marks(sp, len(d), r) for sp, d in zip(spans, docs)]
    # by hand: a document without words but with marks; one without marks; nested and overlapping marks given out of order
    spans += [[], [(0, 3), (4, 8)], [(0, 2), (3, 5), (6, 9), (10, 12), (14, 15)]]
    marks += [[(0, 4, 1), (2, 3, 2)], [], [(0, 5, 1), (3, 9, 4), (4, 4, 2), (9, 10, 3), (12, 14, 3), (5, 6, 2), (14, 99, 0), (2, 3, 6), (11, 15, 4)]]
    return spans, marks


@pytest.mark.parametrize("scheme", ["plain", "bio"])
def test_span_labels_equal_the_oracle(tok, scheme):
    spans, marks = _label_case()
    want_l, want_m = A.span_labels(spans, marks, scheme, outside=-5)
    flat_s, word_off = _flat(spans)
    flat_s = flat_s.reshape(-1, 2)
    flat_m, mark_off = _flat(marks)
    flat_m = flat_m.reshape(-1, 3)
    got_l, got_m = tok._ctx.span_labels(flat_s, word_off, flat_m, mark_off, 1 if scheme == "bio" else 0, -5)
    assert got_l.tolist() == [x for d in want_l for x in d]
    assert got_m.tolist() == [list(x) for d in want_m for x in d]
    py_l, py_m = tok.span_labels(flat_s, word_off, [list(m) for m in marks], scheme=scheme, outside=-5)
    assert np.array_equal(py_l, got_l) and np.array_equal(py_m, got_m)
    py_l, py_m = tok.span_labels(flat_s, word_off, (flat_m, mark_off), scheme=scheme, outside=-5)
    assert np.array_equal(py_l, got_l) and np.array_equal(py_m, got_m)
    # the smallest index wins, and B follows a stolen first word (the hand-made document)
    if scheme == "bio":
        assert want_l[-1] == [2 * 1 + 1, 2 * 1 + 2, 2 * 4 + 1, 2 * 4 + 1, 2 * 0 + 1]
    # no marks at all, no words at all
    l0, m0 = tok._ctx.span_labels(flat_s, word_off, flat_m[:0], np.zeros(len(word_off), dtype=np.int64), 1 if scheme == "bio" else 0, -5)
    assert m0.shape == (0, 2) and l0.tolist() == [0 if scheme == "bio" else -5] * len(flat_s)
    l1, m1 = tok._ctx.span_labels(flat_s[:0], np.zeros(len(word_off), dtype=np.int64), flat_m, mark_off, 0, -5)
    assert l1.shape == (0,) and bool((m1 == -1).all())
    # the device form, the spans and marks behind foreign entries
    ctx = tok._ctx
    with Dev(ctx) as D:
        d_span, d_marks = D.up(np.concatenate([np.full((3, 2), 5, dtype=np.int32), flat_s])), D.up(np.concatenate([np.full((2, 3), 1, dtype=np.int32), flat_m]))
        d_woff, d_moff = D.up(word_off + 3), D.up(mark_off + 2)
        d_l, d_m = D.up(np.full(len(flat_s) + 3, MARK, dtype=np.int32)), D.new(8 * len(flat_m))
        ctx.span_labels_device(d_span, d_woff, len(spans), len(flat_s), d_marks, d_moff, len(flat_m), 1 if scheme == "bio" else 0, -5, d_l, d_m)
        dl = D.down(d_l, len(flat_s) + 3, np.int32)
        assert dl[:3].tolist() == [MARK] * 3 and np.array_equal(dl[3:], got_l)
        assert np.array_equal(D.down(d_m, (len(flat_m), 2), np.int32), got_m)


def test_span_label_refusals(native, tok):
    ctx, p = tok._ctx, native._ptr
    span, woff = np.array([[0, 1], [2, 3], [0, 4]], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64)
    marks, moff = np.array([[0, 1, 1], [0, 9, 2]], dtype=np.int32), np.array([0, 1, 2], dtype=np.int64)
    wl, mw = np.zeros(3, dtype=np.int32), np.zeros((2, 2), dtype=np.int32)
    i64 = lambda *a: np.array(a, dtype=np.int64)                         # noqa: E731

    def call(woff=woff, marks=marks, moff=moff, n=2, scheme=1):
        return ctx.lib.gz_span_labels(ctx.handle, p(span), p(woff), n, p(marks), p(moff), scheme, 0, p(wl), p(mw))
    said = []
    for kw, want in ((dict(marks=np.array([[0, 1, 1], [0, 9, -2]], dtype=np.int32)), "span labels under BIO need labels >= 0"),
                     (dict(woff=i64(0, 3, 2)), "word offsets must not decrease"), (dict(woff=i64(3, 3, 2)), "bad word offsets"),
                     (dict(moff=i64(0, 2, 1)), "mark offsets must not decrease"), (dict(moff=i64(2, 2, 1)), "bad mark offsets"),
                     (dict(scheme=2), "span labels need scheme 0 (plain) or 1 (BIO)"), (dict(n=-1), "span labels need n_docs >= 0")):
        assert call(**kw) == native.GZ_E_INVALID, kw
        assert want in _err(ctx), (kw, _err(ctx))
        said.append(want)
    assert len(set(said)) == len(said)
    assert call(marks=np.array([[0, 1, 1], [0, 9, -2]], dtype=np.int32), scheme=0) == native.GZ_OK and wl.tolist() == [1, 0, -2]
    assert call() == native.GZ_OK and wl.tolist() == [3, 0, 5] and mw.tolist() == [[0, 1], [0, 1]]


# ---- encode_aligned --------------------------------------------------------------------------------------------------------------
BIO_MAP = [v + 1 if v % 2 else v for v in range(64)]


@pytest.mark.parametrize("stride", [None, 5])
def test_encode_aligned_end_to_end(tok, stride):
    docs = list(A.noisy_corpus())
    counts, spans = _corpus_words()
    assert len(docs) == 300
    r = random.Random(29)
    marks = [A.random_marks(sp, len(d), r) for sp, d in zip(spans, docs)]
    L = 32
    got = tok.encode_aligned(docs, L, marks=marks, stride=stride, continuation="bio", scheme="bio")
    want_labels, want_mw = A.span_labels(spans, marks, "bio")
    t = X.tables()
    if stride is None:
        row_doc, row_start = list(range(len(docs))), [0] * len(docs)
        with X._bpe_once():
            for i in range(0, len(docs), 7):
                assert got["input_ids"][i].tolist() == O.call(t, docs[i], max_len=L)["input_ids"], i
    else:
        win = tok.encode_windows(docs, L, stride)
        assert np.array_equal(got["input_ids"], win["input_ids"]) and np.array_equal(got["win_off"], win["win_off"])
        row_doc, row_start = win["doc"].tolist(), win["start"].tolist()
    want_w, want_l, want_n = A.rows(counts, row_doc, row_start, L, want_labels, "map", BIO_MAP, -100)
    assert got["word_tokens"].tolist() == [c for d in counts for c in d]
    assert got["word_span"].tolist() == [list(s) for d in spans for s in d]
    assert got["word_off"].tolist() == np.cumsum([0] + [len(c) for c in counts]).tolist()
    assert got["word_labels"].tolist() == [x for d in want_labels for x in d]
    assert got["mark_words"].tolist() == [list(x) for d in want_mw for x in d]
    assert got["n_real"].tolist() == want_n
    assert np.array_equal(got["word_ids"], np.array(want_w, dtype=np.int32))
    assert np.array_equal(got["labels"], np.array(want_l, dtype=np.int32))
    assert np.array_equal(got["attention_mask"], (got["input_ids"] != t.pad_id).astype(np.int32))
    # word labels given directly, byte spans, another ignore value
    flat_labels = [x for d in want_labels for x in d]
    again = tok.encode_aligned(docs, L, word_labels=flat_labels, stride=stride, continuation="same", ignore_index=-1, unit="byte", word_table=False)
    want_w2, want_l2, _ = A.rows(counts, row_doc, row_start, L, want_labels, "same", None, -1)
    assert np.array_equal(again["word_ids"], got["word_ids"]) and np.array_equal(again["labels"], np.array(want_l2, dtype=np.int32))
    assert again["word_span"].tolist() == [list(s) for d in docs for s in A.spans(d, "byte")]
    assert "labels" not in tok.encode_aligned(docs[:5], L, stride=stride)
    with pytest.raises(ValueError):
        tok.encode_aligned(docs[:5], L, word_labels=[1, 2, 3], stride=stride)
