"""Text quality signals on the GPU (gz_text_signals / _device; genz_tokenize.quality): all 14 signals and all six optional arrays,
exactly, against the plain-Python rule of quality_oracle.py -- at the edges of the walk's trips (T bytes) and lanes, of the
workgroup, of the table, and through every form of the call."""
import ctypes as C
import functools

import numpy as np
import pytest

import quality_oracle as Q

pytestmark = pytest.mark.gpu
KEYS = Q.NAMES + ("line_off", "line_span", "line_first", "para_off", "para_span", "para_first")


@pytest.fixture(scope="module")
def env():
    from genz_tokenize import _native, quality
    ctx = _native.Context()
    yield _native, quality, ctx
    ctx.close()


def fill(n):
    return ("ab cd\nefg " * (n // 10 + 1))[:n].encode()


def edge_docs(T):
    """every item so that it ends at, straddles and begins at a trip edge (and, one byte on, a lane edge)"""
    items = ["\u2028", "\u3000", "\n\n", "\n \n", ".......", "\u2026", "\n- b", "\n\u2022 b", "\u00e9", "x\u2026\ny"]
    docs = []
    for it in items:
        b = it.encode()
        for p in (T - len(b), T - 1, T, T + 1, 2 * T - 2):
            docs.append(fill(p) + b + b"tail ab\nab")
            docs.append(fill(p) + b)
    return docs


@functools.lru_cache(maxsize=None)
def case(name, T, WPB, LONG=512):
    long_line = fill(3 * T + 7).replace(b"\n", b" ")
    many = [b"same line"] * 4000 + [b"line %d" % k for k in range(1000)]
    return {
        "lengths": [fill(n) for n in (0, 1, T - 1, T, T + 1, 3 * T + 1)],
        "edges": edge_docs(T),
        "spans": [long_line + b"\nother\n" + long_line, b" a b \n\ta b\n\na b", b"a  b\na b\na\tb", b"a b\r\nc\r\na b\r\n\r\nc", " \n\t\u3000\u2028 ".encode(),
                  "\u2028\u2028\n".encode(), b"ends in a word\nends in a word", b"ends in a newline\nends in a newline\n", b"...\n...\n\n..."],
        "tables": [b"x y\nz\nx y", b"x y\nz\nx y"] + [fill(40 + k) for k in range(9)] + [b"x y\nz\nx y", b"ab\nba\nab\nba\nabc\nab", b"x y\n\nx y\nz\n\nz\n\nx y\nz",
                   b"q\n\nq", b"\n\n".join([b"p q"] * 5)],
        "lines63": [b"\n".join(b"l%d" % (k % 50) for k in range(n)) for n in (63, 64, 65)],
        "docs-1": [b"a\na"] * (WPB - 1), "docs+0": [b"a\na"] * WPB, "docs+1": [b"a\n\na"] * (WPB + 1), "none": [],
        "contention": [b"\n".join(many[k * 7 % 5000] for k in range(5000))],
        "long": [b"w" * 20000 + b"\n\n" + b"w" * 19999 + b"v\n\n" + b"w" * 20000, b"z " * 10000 + b"\n" + b"z " * 10000,
                 b"\n".join([b"k" * LONG, b"m" * (LONG + 1), b"k" * LONG, b"m" * (LONG + 1), b"m" * LONG + b"k"])],
        "pow2-1": [b"\n".join(b"u%d" % k for k in range(62))], "pow2": [b"\n".join(b"u%d" % k for k in range(63))],
    }[name]


NAMES = ("lengths", "edges", "spans", "tables", "lines63", "docs-1", "docs+0", "docs+1", "none", "contention", "long", "pow2-1", "pow2")


def packed(docs):
    return np.frombuffer(b"".join(docs), np.uint8), np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)


def same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("bits", [0, 1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_signals_and_spans_equal_the_oracle(env, name, bits):
    _native, quality, ctx = env
    docs = case(name, _native.GZ_QUALITY_TRIP, _native.GZ_QUALITY_WPB)
    _native.debug_set("quality_hash_bits", bits, ctx)
    try:
        got = quality.text_signals_packed(*packed(docs), return_lines=True, return_paragraphs=True, ctx=ctx)
    finally:
        _native.debug_set("quality_hash_bits", 0, ctx)
    same(got, Q.signals(docs))


def test_hash_bits_out_of_range_are_refused(env):
    _native, _, ctx = env
    with pytest.raises(ValueError):
        _native.debug_set("quality_hash_bits", 33, ctx)


def test_slices_equal_the_whole(env):
    _native, quality, ctx = env
    docs = case("tables", _native.GZ_QUALITY_TRIP, _native.GZ_QUALITY_WPB)
    whole = quality.text_signals_packed(*packed(docs), ctx=ctx)
    part = quality.text_signals_packed(*packed(docs[3:12]), ctx=ctx)
    for k in Q.NAMES:
        assert np.array_equal(part[k], whole[k][3:12]), k


GUARD = 64
SHAPES = lambda n, L, P: {"signals": ((14, n), np.int32), "line_off": ((n + 1,), np.uint32), "line_span": ((L, 2), np.int64), "line_first": ((L,), np.int32),  # noqa: E731
                          "para_off": ((n + 1,), np.uint32), "para_span": ((P, 2), np.int64), "para_first": ((P,), np.int32)}


@pytest.mark.parametrize("omit", [(), ("signals",), ("line_span",), ("line_first",), ("line_off", "line_span", "line_first"), ("para_span",), ("para_first",),
                                  ("para_off", "para_span", "para_first")])
def test_device_form_behind_junk_with_guard_cells(env, omit):
    _native, quality, ctx = env
    docs = case("spans", _native.GZ_QUALITY_TRIP, _native.GZ_QUALITY_WPB)
    want = Q.signals(docs)
    want["signals"] = np.stack([want[k] for k in Q.NAMES])
    text, off = packed(docs)
    junk = np.frombuffer(b"junk\n\n...#" * 4, np.uint8)[:37]
    shapes = SHAPES(len(docs), len(want["line_first"]), len(want["para_first"]))
    held = []
    try:
        d_text, d_off = ctx.alloc(len(text) + 2 * len(junk)), ctx.alloc(8 * len(off))
        held += [d_text, d_off]
        ctx.h2d(d_text, np.concatenate([junk, text, junk]))
        ctx.h2d(d_off, off + len(junk))
        ptr = {}
        for k, (shape, dtype) in shapes.items():
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            d = ctx.alloc(nbytes + 2 * GUARD)
            held.append(d)
            ctx.h2d(d, np.full(nbytes + 2 * GUARD, 0xA5, np.uint8))
            ptr[k] = (d, nbytes)
        ctx.text_signals_device(d_text, d_off, len(docs), *[0 if k in omit else ptr[k][0] + GUARD for k in shapes])
        for k, (shape, dtype) in shapes.items():
            raw = np.empty(ptr[k][1] + 2 * GUARD, np.uint8)
            ctx.d2h(raw, ptr[k][0])
            assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + ptr[k][1]:] == 0xA5).all(), k
            body = raw[GUARD:GUARD + ptr[k][1]]
            if k in omit:
                assert (body == 0xA5).all(), k
            else:
                assert np.array_equal(body.view(dtype).reshape(shape), want[k]), k
    finally:
        for d in held:
            ctx.free(d)


def test_texts_end_to_end_through_gopher_filter(env):
    _native, quality, ctx = env
    good = " ".join("word%d and" % k for k in range(40))
    texts = [good, good + "\n" + "\n".join(["menu home about"] * 30), "# # # " * 30, "", "- " + good.replace(" and", " ...\n-")]
    out = quality.gopher_filter(texts, ctx=ctx)
    want = Q.signals([t.encode() for t in texts])
    same(out, want, Q.NAMES)
    assert out["keep"].tolist() == [True, False, False, False, False]
    assert np.array_equal(quality.text_signals_to_device(texts, ctx=ctx).numpy(), np.stack([want[k] for k in Q.NAMES]))


def test_c_refusals_leave_canaries(env):
    _native, _, ctx = env
    lib, h, INV = ctx.lib, ctx.handle, _native.GZ_E_INVALID
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    text, off = packed([b"a\na", b"b\n\nb c"])
    text = text.copy()
    out = {k: np.full(int(np.prod(s)) * np.dtype(t).itemsize + 64, 0xC3, np.uint8) for k, (s, t) in SHAPES(2, 4, 3).items()}
    o = {k: P(v) for k, v in out.items()}
    args = lambda **kw: [kw.get(k, o[k]) for k in out]  # noqa: E731
    bad_off = np.array([0, 5, 3], np.int64)
    inside = C.c_void_p(out["signals"].ctypes.data + 8)
    d_text, d_off = ctx.alloc(64), ctx.alloc(64)
    try:
        ctx.h2d(d_text, text)
        ctx.h2d(d_off, bad_off)
        for call, sentence in [
            (lambda: lib.gz_text_signals(h, P(text), P(off), -1, *args()), "n_docs >= 0"),
            (lambda: lib.gz_text_signals(h, None, P(off), 2, *args()), "text and offsets"),
            (lambda: lib.gz_text_signals(h, P(text), None, 2, *args()), "text and offsets"),
            (lambda: lib.gz_text_signals(h, P(text), P(bad_off), 2, *args()), "do not decrease"),
            (lambda: lib.gz_text_signals(h, P(text), P(off), 2, *args(line_off=None)), "beside line_off"),
            (lambda: lib.gz_text_signals(h, P(text), P(off), 2, *args(para_off=None, para_span=None)), "beside para_off"),
            (lambda: lib.gz_text_signals(h, P(text), P(off), 2, *args(line_first=inside)), "overlap"),
            (lambda: lib.gz_text_signals(h, P(text), P(off), 2, *args(para_off=P(off))), "overlap"),
            (lambda: lib.gz_text_signals_device(h, C.c_void_p(d_text), C.c_void_p(d_off), 2, *[None] * 7), "do not decrease"),
            (lambda: lib.gz_text_signals_device(h, None, C.c_void_p(d_off), 2, *[None] * 7), "text and offsets"),
        ]:
            assert call() == INV and sentence in lib.gz_last_error(h).decode(), sentence
        assert lib.gz_text_signals(None, P(text), P(off), 2, *args()) == INV
        assert lib.gz_text_signals(h, None, None, 0, *args()) == _native.GZ_OK and lib.gz_text_signals_device(h, None, None, 0, *[None] * 7) == _native.GZ_OK
        assert all((v == 0xC3).all() for v in out.values()) and off.tolist() == [0, 3, 9] and text.tobytes() == b"a\nab\n\nb c"
        assert lib.gz_text_signals(h, P(text), P(off), 2, *[None] * 7) == _native.GZ_OK
    finally:
        ctx.free(d_text)
        ctx.free(d_off)
