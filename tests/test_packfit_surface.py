"""CPU-only: best-fit packing exists on every layer -- the two C entry points are declared with their argument lists, documented in
the header's own section (the rule written out), exported and bound; _native.Context routes to them; Tokenize.pack_rows and
encode_packs_to_device take `order`, encode_packs_fit exists, unpack_rows is static; the kernels are their own file and the host
plan is a HIP-free header; the refusals come before any native call.  Nothing is computed on a GPU here (tests/test_gpu_packfit.py
does that)."""
import inspect
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
CSRC = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
I32, CI32, CI64 = "int32_t *", "const int32_t *", "const int64_t *"
FIT = ["gz_ctx *", CI32, CI64, "int64_t", "int32_t", "int32_t", "int32_t"] + [I32] * 8 + ["int64_t *", "int64_t *", "int64_t", "int64_t *"]
NAMES = {"gz_pack_rows_fit": FIT, "gz_pack_rows_fit_device": FIT}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_pack_rows": 18, "gz_pack_rows_device": 18, "gz_window_rows": 16, "gz_mask_rows": 17, "gz_infill_rows": 20, "gz_debug_set": 3}


def test_symbols_declared_exported_and_bound():
    from genz_tokenize import _native as native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, types in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        args = [a.strip() for a in decl.group(1).split(",")]
        assert [re.sub(r"\w+$", "", a).strip() for a in args] == types, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == len(types) == 19, n
        assert getattr(lib, n).restype is native.C.c_int, n
    # gz_pack_rows' arguments plus row_docs in front of pack_off
    kept = re.search(r"\bint\s+gz_pack_rows\s*\(([^;]*?)\)\s*;", src, flags=re.S).group(1).split(",")
    fit = re.search(r"\bint\s+gz_pack_rows_fit\s*\(([^;]*?)\)\s*;", src, flags=re.S).group(1).split(",")
    names = lambda xs: [re.search(r"(\w+)\s*$", a).group(1) for a in xs]
    assert names(fit) == names(kept)[:14] + ["row_docs"] + names(kept)[14:] and names(fit)[15] == "pack_off"
    for n, argc in OLD.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == argc, n
        assert len(getattr(lib, n).argtypes) == argc, n
    assert lib.gz_version() == 0x010100
    assert re.search(r"#define\s+GZ_PACK_FIT_MAX_LEN\s+4096\b", src)
    C = native.C
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.gz_pack_rows_fit.argtypes == [vp, vp, vp, i64, i32, i32, i32] + [vp] * 10 + [i64, C.POINTER(i64)]
    assert lib.gz_pack_rows_fit_device.argtypes == lib.gz_pack_rows_fit.argtypes
    for m in ("pack_rows_fit", "pack_rows_fit_device"):
        assert callable(getattr(native.Context, m)), m
    assert re.search(r"\bint\s+gz_pack_rows_fit_info\s*\(\s*gz_ctx \*ctx, double \*plan_ms, int64_t \*events, int64_t \*segments\s*\)\s*;", src)
    assert "gz_pack_rows_fit_info" in native.SYMBOLS and lib.gz_pack_rows_fit_info.argtypes == [vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64)]
    assert lib.gz_pack_rows_fit_info(None, None, None, None) == native.GZ_E_INVALID
    p = list(inspect.signature(native.Context.pack_rows_fit_device).parameters)
    assert p[p.index("d_doc_len") + 1:] == ["d_row_docs", "d_pack_off", "d_seg_off", "capacity"]


RULE = """Take the documents in the order (len descending, index ascending).
Rows are numbered in the order they are opened.  A row carries free (L at first) and stamp (the time of its last
A document of length l goes into the row with the smallest (free, stamp) among the rows with free >= l; if there is none
it opens row R, and R += 1.
Then doc_row = row, doc_col = L - free, free -= l, stamp = ++t."""


def test_header_states_the_rule():
    src = open(HEADER).read()
    block = src[src.index("---- best-fit packing: short documents packed into FULL rows of max_len"):]
    comment = block[:block.index("int  gz_pack_rows_fit(")]
    lines = [re.sub(r"^ \*\s*", "", l).rstrip() for l in comment.splitlines()]
    for want in RULE.splitlines():
        assert want in lines, want
    flat = " ".join(" ".join(lines).split())
    for word in ("best-fit-decreasing", "Krell et al., 2021", "len_r = min(T, L-2) + 2", "L = max_len in [3, GZ_PACK_FIT_MAX_LEN]",
                 "never on timing", "rank among the documents of its length, by index", "from the longest documents to the shortest",
                 "row_docs [n_rows]", "sorted by (doc_row, doc_col)", "row_docs[pack_off[i] .. pack_off[i+1])", "R + 1 entries are written",
                 "the exclusive scan of doc_len[row_docs[.]]", "*total_host = R on GZ_OK and on GZ_E_CAPACITY", "input_ids == NULL sizes only",
                 "the maps are valid and nothing is written to the four cell arrays", "may each be NULL", "max_len > GZ_PACK_FIT_MAX_LEN",
                 "refused, not handled slowly", "DEVICE pointer", "ABSOLUTE", "context's stream", "waits for the device twice",
                 "pinned staging", "Not here", "pair texts", "16-bit outputs"):
        assert word in flat, word
    # a section of its own, right behind the pack section and before the masked rows
    assert src.index("gz_pack_rows_device(") < src.index("---- best-fit packing") < src.index("int  gz_pack_rows_fit_device(") < \
        src.index("masked-LM inputs and labels")


def test_kernels_and_plan_are_their_own_files():
    hip = open(os.path.join(CSRC, "gz_kernels.hip")).read()
    assert hip.index('#include "gz_packrows.inc"') < hip.index('#include "gz_packfit.inc"') < hip.index('#include "gz_mask.inc"')
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "gz_packfit.inc" in make and "gz_packfit.h" in make                 # the build identity covers them
    inc = open(os.path.join(CSRC, "gz_packfit.inc")).read()
    for word in ("gz_packfit_rank_kernel", "gz_packfit_cols_kernel", "gz_packfit_rows_kernel", "gz_packfit_place_kernel", "gz_packfit_seglen_kernel",
                 "wballot(", "below(", "PF_T = GZ_FIT_TILE", "WORKSPACE", "every dependency is a kernel boundary"):
        assert word in inc, word
    assert "atomic" not in inc and "hipMemset" not in inc                      # the rank does not depend on the order anything lands in
    rows = open(os.path.join(CSRC, "gz_packrows.inc")).read()
    assert "template <int U, bool FIT = false>" in rows and "if constexpr (FIT)" in rows       # one fill body for both orders
    kh = open(os.path.join(CSRC, "gz_kernels.h")).read()
    assert "struct GzFitArgs" in kh and re.search(r"GZ_FIT_TILE = 1024\b", kh) and re.search(r"GZ_FIT_MAX_LEN = 4096\b", kh)
    plan = open(os.path.join(CSRC, "gz_packfit.h")).read()
    assert "hip" not in plan.lower().replace("no hip", "") and "inline void gz_packfit_plan(" in plan
    for word in ("struct GzFitEvent", "struct GzFitSeg", "struct GzFitPlan", "__builtin_ctzll"):
        assert word in plan, word
    api = open(os.path.join(CSRC, "gz_rows_api.inc")).read()
    tail = api[api.index("int fit_maps_locked("):api.index("// ---- masked-LM inputs and labels over dense rows")]
    for word in ("gz_packfit_plan(", "pin->fit_hist", "copy_in(", "rows_check(", "rows_stage(", "StagedOut S;", "staged_copy_out(c, S)",
                 "max_len > GZ_PACK_FIT_MAX_LEN", "GZ_E_CAPACITY"):
        assert word in tail, word
    assert tail.count("hipStreamSynchronize") == 3                             # the histogram and the end; the third is the empty batch's
    import packfit_oracle as FO
    assert FO.TILE == 1024 and FO.MAX_LEN == 4096


def test_tokenize_signatures():
    from genz_tokenize import tokenize as tokenize
    T = tokenize.Tokenize
    empty = inspect.Parameter.empty
    want = {
        "pack_rows": [("rows", empty), ("max_len", empty), ("framed", True), ("order", "kept")],
        "encode_packs_fit": [("texts", empty), ("max_len", empty), ("word_table", True)],
        "encode_packs_to_device": [("texts", empty), ("max_len", empty), ("order", "kept")],
    }
    for name, params in want.items():
        p = inspect.signature(getattr(T, name)).parameters
        assert list(p) == ["self"] + [k for k, _ in params], name
        for k, d in params:
            assert p[k].default == d and type(p[k].default) is type(d), (name, k)
    assert isinstance(inspect.getattr_static(T, "unpack_rows"), staticmethod)
    assert list(inspect.signature(T.unpack_rows).parameters) == ["result"]
    assert T.PACK_FIT_MAX_LEN == 4096
    for word in ("best-fit-decreasing", "row_docs", "from the longest documents to the shortest", "shuffles rows"):
        assert word in T.pack_rows.__doc__, word
    assert "row_docs" in T.unpack_rows.__doc__ and "document r" in T.unpack_rows.__doc__
    # the neighbour is what it was
    assert list(inspect.signature(T.encode_packs).parameters) == ["self", "texts", "max_len", "word_table"]


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def test_refusals_come_before_any_native_call():
    from genz_tokenize import tokenize as tokenize
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = _NoNative()
    t._dirty = True
    for order in ("best", "", None, "Fit", 0):
        with pytest.raises(ValueError):
            t.pack_rows([[1, 2, 3]], 8, order=order)
        with pytest.raises(ValueError):
            t.encode_packs_to_device(["a"], 8, order=order)
    for L in (2, 4097, 2 ** 31):
        with pytest.raises(ValueError):
            t.pack_rows([[1, 2, 3]], L, order="fit")
        with pytest.raises(ValueError):
            t.encode_packs_fit(["a"], L)
        with pytest.raises(ValueError):
            t.encode_packs_to_device(["a"], L, order="fit")
    with pytest.raises(TypeError):
        t.pack_rows([[1, 2, 3]], 8.0, order="fit")
    assert tokenize.Tokenize._pack_order("fit", 4096) is True and tokenize.Tokenize._pack_order("kept", 2 ** 20) is False
