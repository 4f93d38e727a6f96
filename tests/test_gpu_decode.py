"""Batch decode on the GPU (Tokenize.decode_batch, gz_decode_batch, gz_decode_batch_device; csrc/gz_decode.inc) against
gz_oracle.decode and the reference's recorded results (g6b_decode_shapes.jsonl.gz) on the synthetic table of decode_tables.py:
every inline piece size at every output alignment, rows around multiples of the 64 tokens a wave takes per trip with chosen words on
both sides of the edge, rows of ids with little or no text, ids outside the table, the unk string in its inline / arena / filtered
forms replacing each other in the one table slot, exact capacities with guard bytes around the device output, and the decoder
snapshot that add_vocab_file must not move.  Every comparison is ==: decoded bytes and offsets, no tolerance.
test_decode_inputs.py (CPU) checks that the rows are what they claim and that the oracle agrees with the reference on them."""
import base64
import ctypes as C
import random
import types

import numpy as np
import pytest

import decode_tables as T
import gz_oracle as O
from conftest import read_jsonl

pytestmark = pytest.mark.gpu

GROUPS = ("align", "trips", "nothing", "ids", "unk_rows")


@pytest.fixture(scope="module")
def s():
    return T.Shapes()


@pytest.fixture(scope="module")
def fx():
    return T.fixture(read_jsonl("g6b_decode_shapes.jsonl.gz"))


@pytest.fixture(scope="module")
def files(fx, tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_shapes")
    for name, key in (("vocab", "vocab_b64"), ("bpe", "bpe_b64"), ("vocab2", "second_vocab_b64")):
        (d / name).write_bytes(base64.b64decode(fx[0][key]))
    return str(d / "vocab"), str(d / "bpe"), str(d / "vocab2")


@pytest.fixture(scope="module")
def tables(fx):
    return O.Tables(base64.b64decode(fx[0]["vocab_b64"]), base64.b64decode(fx[0]["bpe_b64"]))


@pytest.fixture(scope="module")
def want(s, tables):
    """The oracle's text of every row of every group: computed once, read by all tests."""
    return {g: [O.decode(r, tables) for r in getattr(s, g)] for g in GROUPS}


@pytest.fixture(scope="module")
def tok(files):
    from genz_tokenize import Tokenize
    t = Tokenize.fromFile(files[0], files[1])
    assert t.decode_batch([[1, 2]]) == ["<s> </s>"]                     # (tables and decoder snapshot are on the device from here on)
    return t


def _where(s, g, k, row):
    return "%s[%d]%s: %d tokens, trip edges %s" % (g, k, " (%s)" % s.trip_notes[k] if g == "trips" else "", len(row), T.edges(s, row))


def _with_unk(tables, u):
    """The table as it is, another string for the ids it does not hold (what Context.decode's `unk` argument is)."""
    return types.SimpleNamespace(decoder=tables.decoder, specials=tuple(tables.specials[:4]) + (u,))


def _pack(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        np.cumsum([len(r) for r in rows], out=off[1:])
    flat = np.asarray([i for r in rows for i in r], dtype=np.int64).astype(np.int32)
    return flat, off


def _texts(data, off):
    raw = data.tobytes()
    return [raw[off[i]:off[i + 1]].decode("utf-8") for i in range(len(off) - 1)]


def _bytes_and_offsets(texts):
    parts = [t.encode("utf-8") for t in texts]
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    if parts:
        np.cumsum([len(p) for p in parts], out=off[1:])
    return np.frombuffer(b"".join(parts), dtype=np.uint8), off


# ---- the row groups, one call each ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GROUPS)
def test_row_group_in_one_call(tok, s, fx, want, g):
    rows = getattr(s, g)
    got = tok.decode_batch(rows)
    assert len(got) == len(rows)
    for k, row in enumerate(rows):
        assert got[k] == want[g][k], _where(s, g, k, row)
        assert T.same(got[k], fx[1][g]["result"][k]), _where(s, g, k, row)


def test_batches_of_little_or_no_text(tok, s, want):
    for b, picks in enumerate(s.nothing_batches):
        assert tok.decode_batch([s.nothing[i] for i in picks]) == [want["nothing"][i] for i in picks], b
    zero = [s.nothing[i] for i in s.nothing_batches[s.ZERO_BATCH]]
    assert sum(map(len, zero)) > 0 and tok.decode_batch(zero) == [""] * len(zero)


def test_ids_outside_int32_decode_to_unk(tok, s, tables):
    assert tok.decode_batch(s.ids_wide) == [O.decode(r, tables) for r in s.ids_wide]
    for r in s.ids_wide:
        assert tok.decode(r) == O.decode(r, tables)


# ---- the same rows alone, and four to a workgroup ---------------------------------------------------------------------------
def test_trips_as_single_row_calls(tok, s, want):
    for k, row in enumerate(s.trips):
        assert tok.decode_batch([row]) == [want["trips"][k]], _where(s, "trips", k, row)


@pytest.mark.parametrize("b", range(1, 10))
def test_trips_in_batches_between_empty_rows(tok, s, want, b):
    """b rows of `trips` at a time with an empty row before, between and behind them: a workgroup holds four rows, so every row
    meets every wave of the workgroup and empty neighbours."""
    n = len(s.trips)
    for lo in range(0, n, b):
        ks = list(range(lo, min(n, lo + b)))
        batch, exp = [[]], [""]
        for k in ks:
            batch += [s.trips[k], []]
            exp += [want["trips"][k], ""]
        got = tok.decode_batch(batch)
        for j, k in enumerate(ks):
            assert got[1 + 2 * j] == exp[1 + 2 * j], _where(s, "trips", k, s.trips[k])
        assert got == exp


# ---- array inputs -------------------------------------------------------------------------------------------------------------
ODD = {"int64": (2 ** 40, -2 ** 40, 2 ** 31, -2 ** 31 - 1), "uint32": (2 ** 31, 2 ** 32 - 1), "int16": (-1, -2 ** 15),
       "uint64": (2 ** 63 + 5, 2 ** 64 - 1, 2 ** 32), "int32": (-1, 2 ** 31 - 1, -2 ** 31)}


@pytest.mark.parametrize("L", [63, 64, 65])
@pytest.mark.parametrize("dtype", sorted(ODD))
def test_two_dimensional_arrays(tok, s, tables, L, dtype):
    r = random.Random(L)
    pool = [s.id[n] for n in s.pool_names()]
    rows = [[pool[int(r.random() * len(pool))] for _ in range(L)] for _ in range(9)]
    rows[1][L - 1] = s.id["ends:8"]                                   # kept: the row ends there
    rows[2][62], rows[2][L - 1] = s.id["ends:15"], s.id["inner:6:xends"]
    for k, v in enumerate(ODD[dtype]):                                # values that no int32 holds, or that no word has
        rows[3 + k][0] = rows[3 + k][L - 1] = rows[3 + k][31 + k] = v
    arr = np.array(rows, dtype=dtype)
    assert arr.shape == (9, L) and arr.tolist() == rows
    got = tok.decode_batch(arr)
    for k, row in enumerate(rows):
        assert got[k] == O.decode(row, tables), (dtype, L, k)
    assert tok.decode_batch([np.array(x, dtype=dtype) for x in rows]) == got          # a list of 1-D arrays


def test_float_ids_are_refused(tok):
    with pytest.raises(TypeError):
        tok.decode_batch(np.zeros((2, 64), dtype=np.float32))
    with pytest.raises(TypeError):
        tok.decode_batch(np.zeros((2, 3), dtype=np.float64))


# ---- the unk string -------------------------------------------------------------------------------------------------------------
def test_unk_strings_replace_each_other_on_one_context(tok, s, tables):
    """The unk string of a call sits in ONE table slot (and, past 12 bytes or with an inner '@@ ', behind the arena): each form
    after each other form, the same string twice (dec_set_unk keeps the last one), and the 4096-byte limit."""
    from genz_tokenize import _native
    ctx = tok._ctx
    rows = s.unk_rows + s.ids
    flat, off = _pack(rows)
    u12, u13, e12, big = T.UNKS[2], T.UNKS[3], T.UNKS[4], T.UNKS[7]
    order = ["", "u", u12, u13, e12, "@@", "a@@ b", big, "u", "u"]
    assert [T.nbytes(u) for u in order] == [0, 1, 12, 13, 12, 2, 5, 4096, 1, 1] and e12.endswith("@@")

    def check(u, step):
        data, out_off = ctx.decode(flat, off, u.encode("utf-8"))
        got, tu = _texts(data, out_off), _with_unk(tables, u)
        for k, row in enumerate(rows):
            assert got[k] == O.decode(row, tu), ("step %d, unk of %d bytes %r" % (step, T.nbytes(u), u[:16]), k, row[:8])
    for step, u in enumerate(order):
        check(u, step)
    with pytest.raises(_native.GzError) as ei:
        ctx.decode(flat, off, b"x" * 4097)
    assert ei.value.code == _native.GZ_E_LIMIT
    check("u", 10)                                                    # (the refused call changed nothing)
    check(u13, 11)
    with pytest.raises(_native.GzError):
        ctx.decode(flat, off, b"x" * 4097)
    check("a@@ b", 12)
    # another string of the SAME length right after: other bytes ("v" after "u"), other flags (12 bytes, then 12 ending in "@@"; an
    # inner "@@ " in 13 bytes after 13 plain ones), a prefix of the last one in the arena
    for step, u in enumerate(["u", "v", u12, e12, u12[:10] + "@ ", u13, u13[:5] + "@@ " + u13[8:], big, big[:4095] + "@", big[:4090]], 13):
        check(u, step)
    assert tok.decode_batch(s.unk_rows) == [O.decode(r, tables) for r in s.unk_rows]          # and back to the object's own


def test_unk_token_of_the_constructor(files, s, fx, tables):
    """Tokenize(unk_token=u) on the synthetic table, built the way the fixture's reference objects were: u is word 4 of the
    table as well (and moves the ids where it is one of the file's words)."""
    from genz_tokenize import Tokenize
    vocab = open(files[0], "rb").read()
    for line in fx[2]:
        u = line["unk_token"]
        t = Tokenize.__new__(Tokenize)
        t.vocab_file, t.bpe_file = files[0], files[1]
        t.__init__(unk_token=u)
        tu = O.Tables(vocab, b"", O.DEFAULT_SPECIALS[:4] + (u,))
        for g, res in line["result"].items():
            rows = getattr(s, g)
            got = t.decode_batch(rows)
            for k, row in enumerate(rows):
                assert got[k] == O.decode(row, tu), (u[:16], g, k)
                assert T.same(got[k], res[k]), (u[:16], g, k)
        assert t.decode(s.unk_rows[6]) == O.decode(s.unk_rows[6], tu)
        t._ctx.close()                                                # (one native context per unk string: released here)


# ---- the device form ----------------------------------------------------------------------------------------------------------
GUARD = 64


class _Dev:
    """Device buffers of one test; every one is freed at the end."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.alloc(max(int(nbytes), 1))
        self.bufs.append(p)
        return p

    def up(self, arr):
        p = self.alloc(arr.nbytes + 64)
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def free(self):
        for p in self.bufs:
            self.ctx.free(p)
        self.bufs = []


def _device_case(dev, rows, texts, shifts, unk=b"<unk>"):
    """Size query, then the text into exactly `need` bytes at buf + GUARD + s of a buffer of 0xA5: the bytes before and behind stay;
    one byte less of capacity is refused and writes nothing."""
    from genz_tokenize import _native
    ctx, n = dev.ctx, len(rows)
    flat, off = _pack(rows)
    exp, exp_off = _bytes_and_offsets(texts)
    need = int(exp_off[-1])
    d_ids, d_ro = dev.up(flat), dev.up(off)
    d_oo = dev.up(np.full(n + 1, -7, dtype=np.int64))
    assert ctx.decode_device(d_ids, d_ro, n, unk, 0, 0, d_oo) == need
    oo = np.empty(n + 1, dtype=np.int64); ctx.d2h(oo, d_oo)
    assert np.array_equal(oo, exp_off)
    size = GUARD + 8 + need + GUARD
    fill = np.full(size, 0xA5, dtype=np.uint8)
    d_buf = dev.alloc(size)
    got = np.empty(size, dtype=np.uint8)
    for sh in shifts:
        base = GUARD + sh
        ctx.h2d(d_buf, fill)
        ctx.h2d(d_oo, np.full(n + 1, -7, dtype=np.int64))
        assert ctx.decode_device(d_ids, d_ro, n, unk, d_buf + base, need, d_oo) == need
        ctx.d2h(got, d_buf); ctx.d2h(oo, d_oo)
        assert np.array_equal(oo, exp_off), sh
        assert np.all(got[:base] == 0xA5), ("bytes in front of the output", sh, np.flatnonzero(got[:base] != 0xA5)[:8])
        assert np.all(got[base + need:] == 0xA5), ("bytes behind the output", sh, np.flatnonzero(got[base + need:] != 0xA5)[:8])
        if not np.array_equal(got[base:base + need], exp):
            at = int(np.flatnonzero(got[base:base + need] != exp)[0])
            row = int(np.searchsorted(exp_off, at, side="right")) - 1
            raise AssertionError("shift %d: byte %d differs, row %d %r" % (sh, at, row, rows[row][:8]))
    if need:
        ctx.h2d(d_buf, fill)
        with pytest.raises(_native.GzError) as ei:
            ctx.decode_device(d_ids, d_ro, n, unk, d_buf + GUARD, need - 1, d_oo)
        assert ei.value.code == _native.GZ_E_CAPACITY
        ctx.d2h(got, d_buf)
        assert np.all(got == 0xA5)
    return need


def test_device_form_fills_its_capacity_and_no_more(tok, s, want):
    dev = _Dev(tok._ctx)
    try:
        need = _device_case(dev, s.align + s.trips, want["align"] + want["trips"], range(8))
        assert need > 100_000
    finally:
        dev.free()


def test_device_form_by_the_last_token(tok, s, tables):
    """Batches whose last bytes are an inline token of every length, plain and ending in '@@' (kept: nothing follows)."""
    names = ["empty:0"] + ["plain:%d" % n for n in range(1, 13)] + ["ends:%d" % n for n in range(2, 13)] + ["ends:3:at", "ends:4:at"]
    dev = _Dev(tok._ctx)
    try:
        for j, name in enumerate(names):
            rows = [[s.id["plain:3"], s.id["ends:8"]], [s.id["plain:%d" % (1 + j % 8)], s.id[name]]]
            _device_case(dev, rows, [O.decode(r, tables) for r in rows], [(3 * j) % 8, (3 * j + 5) % 8])
            dev.free()
    finally:
        dev.free()


def test_device_form_without_rows(tok):
    dev = _Dev(tok._ctx)
    try:
        d_oo = dev.up(np.full(2, -7, dtype=np.int64))
        d_ro = dev.up(np.zeros(1, dtype=np.int64))
        d_out = dev.up(np.full(64, 0xA5, dtype=np.uint8))
        for out, cap in ((0, 0), (d_out, 64)):
            tok._ctx.h2d(d_oo, np.full(2, -7, dtype=np.int64))
            assert tok._ctx.decode_device(0, d_ro, 0, b"<unk>", out, cap, d_oo) == 0
            oo = np.empty(2, dtype=np.int64); tok._ctx.d2h(oo, d_oo)
            assert oo.tolist() == [0, -7]
        got = np.empty(64, dtype=np.uint8); tok._ctx.d2h(got, d_out)
        assert np.all(got == 0xA5)
    finally:
        dev.free()


# ---- the host form --------------------------------------------------------------------------------------------------------------
def _host_call(ctx, rows, unk, cap):
    from genz_tokenize._native import _ptr
    flat, off = _pack(rows)
    n = len(rows)
    out_off = np.full(n + 1, -7, dtype=np.int64)
    out = np.full(max(cap, 1) + GUARD, 0xA5, dtype=np.uint8)
    ub = C.create_string_buffer(unk, len(unk))
    rc = ctx.lib.gz_decode_batch(ctx.handle, _ptr(flat) if len(flat) else None, _ptr(off), n, C.cast(ub, C.c_void_p), len(unk),
                                 _ptr(out), cap, _ptr(out_off))
    return rc, out, out_off


def test_host_form_reports_the_size_it_needs(tok, s, want):
    from genz_tokenize import _native
    rows, texts = s.trips[:40], want["trips"][:40]
    exp, exp_off = _bytes_and_offsets(texts)
    need = int(exp_off[-1])
    for cap in (need - 1, 0):
        rc, out, out_off = _host_call(tok._ctx, rows, b"<unk>", cap)
        assert rc == _native.GZ_E_CAPACITY and np.array_equal(out_off, exp_off) and np.all(out == 0xA5), cap
    rc, out, out_off = _host_call(tok._ctx, rows, b"<unk>", need)
    assert rc == _native.GZ_OK
    assert np.array_equal(out_off, exp_off) and np.array_equal(out[:need], exp) and np.all(out[need:] == 0xA5)


def test_host_form_with_ids_and_no_text(tok, s):
    from genz_tokenize import _native
    zero = [s.nothing[i] for i in s.nothing_batches[s.ZERO_BATCH]]
    flat, off = _pack(zero)
    assert len(flat) == 2
    data, out_off = tok._ctx.decode(flat, off, b"<unk>")
    assert len(data) == 0 and out_off.tolist() == [0] * (len(zero) + 1)
    rc, out, out_off = _host_call(tok._ctx, zero, b"<unk>", 0)
    assert rc == _native.GZ_OK and out_off.tolist() == [0] * (len(zero) + 1) and np.all(out == 0xA5)


# ---- the decoder snapshot ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode_first", [False, True])
def test_add_vocab_file_leaves_the_decoder_alone(files, fx, decode_first):
    """tokenize.py:40: `decoder` is made once, by __init__.  Words of a later add_vocab_file get ids that encode() returns and that
    decode() and decode_batch() do not know.  Without `decode_first` NOTHING touches the tables between fromFile and
    add_vocab_file (no encode, no vocab_size, no `encoder`): add_vocab_file itself has to take the device decoder snapshot before
    the vocabulary grows -- the sequence the fixture's reference object went through."""
    from genz_tokenize import Tokenize
    added = fx[3]
    t = Tokenize.fromFile(files[0], files[1])
    try:
        if decode_first:
            assert t.decode_batch(added["ids"]) == added["before"]
            assert {w: t.encode(w, False) for w in added["encode_before"]} == added["encode_before"]
            assert t.vocab_size() == added["vocab_size"][0]
        t.add_vocab_file(files[2])
        assert t.decode_batch(added["ids"]) == added["after"]
        assert [t.decode(r) for r in added["ids"]] == added["after"]
        assert t.vocab_size() == added["vocab_size"][1]
        assert {w: t.encode(w, False) for w in added["encode_after"]} == added["encode_after"]
        assert {w: t.encoder[w] for w in added["new_word_ids"]} == added["new_word_ids"]
        assert t.decode_batch(added["ids"]) == added["after"]
    finally:
        t._ctx.close()


def test_words_before_add_vocab_file_on_an_object_of_their_own(files, fx):
    """What encode() and vocab_size() give before the second file, without a decode before them."""
    from genz_tokenize import Tokenize
    added = fx[3]
    t = Tokenize.fromFile(files[0], files[1])
    try:
        assert {w: t.encode(w, False) for w in added["encode_before"]} == added["encode_before"]
        assert t.vocab_size() == added["vocab_size"][0]
        t.add_vocab_file(files[2])
        assert t.decode_batch(added["ids"]) == added["after"]
    finally:
        t._ctx.close()
