"""CPU-only: span-corruption rows exist on every layer -- the two C entry points are declared with their argument lists, documented
in the header's own section, exported and bound; _native.Context routes to them; Tokenize has infill_rows / infill_rows_to_device
with their defaults; every bad argument is refused before any native call; and Tokenize._infill_rule makes the integers the oracle
makes.  Nothing is computed on a device here (tests/test_gpu_infill.py does that)."""
import inspect
import os
import re

import numpy as np
import pytest

import infill_oracle as IO
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_infill_rows": 20, "gz_infill_rows_device": 20}
OLD = {"gz_mask_rows": 17, "gz_mask_rows_device": 17, "gz_window_rows": 16, "gz_pack_rows": 18}      # (what the neighbours take stays)
TYPES = ["gz_ctx *", "const int32_t *", "int64_t", "int32_t", "int64_t", "uint64_t", "uint64_t", "const uint64_t *", "int32_t", "int32_t",
         "int32_t", "int32_t", "int32_t"] + ["int32_t *"] * 7
ORDER = ["ctx", "ids", "n_rows", "row_len", "row_base", "seed", "t_start", "len_t", "n_len", "mask_id", "whole_word", "ignore_index",
         "dec_width", "input_ids", "attention_mask", "labels", "decoder_input_ids", "enc_len", "dec_len", "n_spans"]
ONE = 2 ** 32


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in dict(NAMES, **OLD).items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == argc, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc, n
        if n in NAMES:
            assert [re.sub(r"\w+$", "", a).strip() for a in args] == TYPES, n
            assert [re.sub(r"_dev$", "", re.search(r"\w+$", a).group(0)) for a in args] == ORDER, n
    assert lib.gz_version() == 0x010100
    C = native.C
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert lib.gz_infill_rows.argtypes == [vp, vp, i64, i32, i64, u64, u64, vp, i32, i32, i32, i32, i32] + [vp] * 7
    assert lib.gz_infill_rows_device.argtypes == lib.gz_infill_rows.argtypes
    assert lib.gz_infill_rows.restype is C.c_int and lib.gz_infill_rows_device.restype is C.c_int
    for m in ("infill_rows", "infill_rows_device"):
        assert callable(getattr(native.Context, m)), m


def test_header_documents_the_rule():
    src = open(HEADER).read()
    block = src[src.index("span-corruption inputs and targets"):]
    comment = block[:block.index("int  gz_infill_rows(")]
    for word in ("PROTECTED", "CONTINUATION", "start(r, c)", "head(r, c)", "g(r, c)", "Philox4x32-10", "x0 and x1", "correlated", "n(r, c)",
                 "t_start", "len_t", "n_len", "chosen(r, c)", "reach(s)", "far(", "run ", "E(r)", "T(r)", "n_chosen + n_spans + 1", "dec_width",
                 "UNCLIPPED", "ignore_index", "decoder_input_ids", "attention_mask", "enc_len", "dec_len", "n_spans", "row_base",
                 "row_len + 2", "GZ_E_INVALID", "GZ_E_NOTABLES", "gz_decoder_snapshot", "overlapping", "HOST pointer", "gz_infill_rows_device:",
                 "gz_infill_rows:", "2^63", "2^32", "BART"):
        assert word in comment, word
    assert src.index("gz_mask_rows_device(") < src.index("span-corruption inputs and targets") < src.index("---- text pre-pass")


def test_tokenize_signatures():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    want = [("input_ids", inspect.Parameter.empty), ("p", 0.15), ("mean_span", 3.0), ("max_span", 10), ("lengths", "geometric"), ("seed", 0),
            ("whole_word", True), ("dec_len", None), ("row_base", 0), ("ignore_index", -100)]
    for name in ("infill_rows", "infill_rows_to_device"):
        p = inspect.signature(getattr(tokenize.Tokenize, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in want], name
        for k, d in want:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
    # the neighbour is what it was
    p = inspect.signature(tokenize.Tokenize.mask_rows).parameters
    assert list(p) == ["self", "input_ids", "p", "seed", "whole_word", "mask_prob", "random_prob", "random_ids", "row_base", "ignore_index"]


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = _NoNative()
    t._dirty = True                                                   # (so that any table use would reach the context)
    return t


IDS = np.zeros((2, 4), dtype=np.int32)
BAD = [
    (IDS, dict(p=-0.1), ValueError), (IDS, dict(p=1.0001), ValueError), (IDS, dict(p=float("nan")), ValueError), (IDS, dict(p=True), TypeError),
    (IDS, dict(p="0.1"), TypeError), (IDS, dict(p=None), TypeError),
    (IDS, dict(mean_span=0.5), ValueError), (IDS, dict(mean_span=11.0), ValueError), (IDS, dict(mean_span=float("nan")), ValueError),
    (IDS, dict(mean_span=float("inf")), ValueError), (IDS, dict(mean_span="3"), TypeError), (IDS, dict(mean_span=True), TypeError),
    (IDS, dict(mean_span=None), TypeError), (IDS, dict(mean_span=2.5, lengths="fixed"), ValueError),
    (IDS, dict(max_span=0), ValueError), (IDS, dict(max_span=17), ValueError), (IDS, dict(max_span=10.0), TypeError),
    (IDS, dict(max_span=True), TypeError), (IDS, dict(max_span=2), ValueError),                        # (mean_span 3 > max_span 2)
    (IDS, dict(lengths="uniform"), ValueError), (IDS, dict(lengths=None), TypeError), (IDS, dict(lengths=3), TypeError),
    (IDS, dict(seed=-1), ValueError), (IDS, dict(seed=2 ** 64), ValueError), (IDS, dict(seed=1.0), TypeError), (IDS, dict(seed=True), TypeError),
    (IDS, dict(seed=None), TypeError),
    (IDS, dict(whole_word=1), TypeError), (IDS, dict(whole_word=None), TypeError), (IDS, dict(whole_word="yes"), TypeError),
    (IDS, dict(dec_len=0), ValueError), (IDS, dict(dec_len=-3), ValueError), (IDS, dict(dec_len=2 ** 31), ValueError),
    (IDS, dict(dec_len=4.0), TypeError), (IDS, dict(dec_len=True), TypeError),
    (IDS, dict(row_base=-1), ValueError), (IDS, dict(row_base=2 ** 63), ValueError), (IDS, dict(row_base=True), TypeError),
    (IDS, dict(row_base=0.0), TypeError), (IDS, dict(row_base=2 ** 63 // 4 - 1), ValueError),
    (IDS, dict(ignore_index=2 ** 31), ValueError), (IDS, dict(ignore_index=-2 ** 31 - 1), ValueError), (IDS, dict(ignore_index=False), TypeError),
    (IDS, dict(ignore_index=1.5), TypeError),
    (IDS.astype(np.float64), {}, TypeError), (IDS.astype(bool), {}, TypeError), ([["a", "b"]], {}, TypeError),
    (IDS[0], {}, ValueError), (IDS.reshape(2, 2, 2), {}, ValueError), (np.zeros((3, 0), dtype=np.int32), {}, ValueError), (7, {}, ValueError),
    (np.array([[2 ** 31]]), {}, ValueError), (np.array([[-2 ** 31 - 1]]), {}, ValueError), (np.array([[2 ** 63]], dtype=np.uint64), {}, ValueError),
]
N_RULE = 44                                                           # the entries of BAD that the rule itself refuses


def test_refusals_before_any_native_call():
    t = _bare()
    assert all(ids is IDS for ids, _, _ in BAD[:N_RULE]) and BAD[N_RULE][0] is not IDS
    for ids, kw, exc in BAD:
        with pytest.raises(exc):
            t.infill_rows(ids, **kw)
    handoff = pytest.importorskip("genz_tokenize.handoff")
    for rows in (IDS, IDS.tolist(), None):
        with pytest.raises(TypeError):
            t.infill_rows_to_device(rows)
    fake = handoff.DeviceArray.__new__(handoff.DeviceArray)           # (no allocation behind it: only its shape and dtype are looked at)
    fake._ctx, fake.ptr, fake._block = t._ctx, 0, None
    for shape, dtype, exc in (((2, 4), np.int64, TypeError), ((8,), np.int32, ValueError), ((2, 0), np.int32, ValueError), ((2, 2, 2), np.int32, ValueError)):
        fake.shape, fake.dtype = shape, np.dtype(dtype)
        with pytest.raises(exc):
            t.infill_rows_to_device(fake)
    fake.shape, fake.dtype = (2, 4), np.dtype(np.int32)
    for _, kw, exc in BAD[:N_RULE]:                                   # the rule's own refusals are the same ones
        with pytest.raises(exc):
            t.infill_rows_to_device(fake, **kw)
    fake._ctx = _NoNative()                                           # rows of another context
    with pytest.raises(ValueError):
        t.infill_rows_to_device(fake)


LAWS = [("geometric", 3.0, 10), ("geometric", 1.0, 16), ("geometric", 16.0, 16), ("geometric", 2.5, 3), ("poisson", 3.0, 10),
        ("poisson", 1.0, 1), ("poisson", 7.5, 16), ("fixed", 3.0, 10), ("fixed", 1, 1), ("fixed", 16, 16)]


def test_rule_integers():
    """thresholds non-decreasing and in [0, 2^32]; n_len is max_span (the fixed law: its length); q reproduces p through the product
    formula to 1e-9 -- on q itself: t_start is q cut to 32 bits, and a step of 2^-32 in q moves the coverage by up to
    n_len * 2^-32 = 3.7e-9 --; and the integers are the ones tests/infill_oracle.py makes on its own"""
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    T = tokenize.Tokenize
    for law, mean, mx in LAWS:
        pmf = T._infill_lengths(law, mean, mx)
        n_len = int(mean) if law == "fixed" else mx
        assert len(pmf) == n_len and abs(sum(pmf) - 1) < 1e-12 and all(x >= 0 for x in pmf)
        assert pmf == IO.length_law(law, mean, mx)
        tail = IO.tail_of(pmf)
        assert tail[0] == 1.0 and all(a >= b for a, b in zip(tail, tail[1:]))
        for p in (0.0, 1e-6, 0.05, 0.15, 0.5, 0.9, 0.999999, 1.0):
            q = T._infill_start_share(p, tail)
            assert 0 <= q <= 1
            prod = 1.0
            for k in range(n_len):
                prod *= 1.0 - q * tail[k]
            assert abs((1.0 - prod) - p) < 1e-9, (law, mean, mx, p)
            seed, t_start, len_t, got_n, ww, ignore, dec_len, base = T._infill_rule(p, mean, mx, law, 5, False, None, 9, -1)
            assert (seed, got_n, ww, ignore, dec_len, base) == (5, n_len, 0, -1, None, 9)
            assert t_start == int(q * ONE) and 0 <= t_start <= ONE and (t_start == ONE) == (p == 1.0) and (t_start == 0) == (p == 0.0)
            assert len(len_t) == n_len - 1 and all(isinstance(v, int) and 0 <= v <= ONE for v in len_t)
            assert all(a <= b for a, b in zip(len_t, len_t[1:]))
            assert (t_start, len_t, n_len) == IO.rule_ints(p, mean, mx, law)
            if law == "fixed":
                assert len_t == [0] * (n_len - 1)                     # every span n_len words
    _, t_start, len_t, n_len, _, _, dec_len, _ = T._infill_rule(0.15, 3.0, 10, "geometric", 0, True, 64, 0, -100)
    assert dec_len == 64 and n_len == 10
    # the geometric law before truncation: P(len <= k) = 1 - (2/3)^k, renormalised by 1 - (2/3)^10
    z = 1 - (2 / 3) ** 10
    assert all(abs(v / ONE - (1 - (2 / 3) ** (k + 1)) / z) < 1e-9 for k, v in enumerate(len_t))
    assert 0.04 < t_start / ONE < 0.07                                # about p / the mean length
