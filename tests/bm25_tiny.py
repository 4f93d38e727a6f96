"""A tiny corpus and one ctypes caller for the fifteen search entry points of the BM25 index (gz_bm25_search, _bool, _phrase, _near
and _groups, each with a _device form and a gz_bm25_match_count* form): what test_gpu_bm25_search_refusals.py and
test_gpu_bm25_search_doors.py share.  130 one-line documents over twelve words: a row's bitmap takes three 64-bit words.
CHANGES / change() are the same for the nine entry points that make or change an index (test_gpu_bm25_change_refusals.py,
test_gpu_bm25_change_life.py)."""
import ctypes

import numpy as np

VOCAB = ["w%d" % i for i in range(12)]
N_DOCS = 130
W64 = (N_DOCS + 63) // 64


def documents():
    """document i: 3 to 6 words, every word of VOCAB in many documents, neighbouring documents different"""
    return [" ".join(VOCAB[(i * (j + 1) + j * j + i // 12) % 12] for j in range(3 + i % 4)) for i in range(N_DOCS)]


_Q = ["terms", "idf", "qoff", "nq", "params", "plus", "k"]
_C = ["terms", "qoff", "nq"]
_BOOL = ["mode", "ex_terms", "ex_off"]
_PH = ["ph_terms", "ph_off"]
_NR = ["nr_terms", "nr_off", "nr_win"]
_OUT = ["doc", "score", "cnt"]
_G = ["alt_terms", "alt_off", "group_idf", "group_off", "nq", "params", "plus", "k"]

# entry point -> its arguments behind the index, in the order of include/genz_tokenize.h
ENTRIES = {
    "gz_bm25_search": _Q + _OUT,
    "gz_bm25_search_device": _Q + _OUT,
    "gz_bm25_match_count": _C + ["cnt"],
    "gz_bm25_search_bool": _Q + _BOOL + _OUT,
    "gz_bm25_search_bool_device": _Q + _BOOL + _OUT,
    "gz_bm25_match_count_bool": _C + _BOOL + ["cnt"],
    "gz_bm25_search_phrase": _Q + _BOOL + _PH + _OUT,
    "gz_bm25_search_phrase_device": _Q + _BOOL + _PH + _OUT,
    "gz_bm25_match_count_phrase": _C + _BOOL + _PH + ["cnt"],
    "gz_bm25_search_near": _Q + _BOOL + _PH + _NR + _OUT,
    "gz_bm25_search_near_device": _Q + _BOOL + _PH + _NR + _OUT,
    "gz_bm25_match_count_near": _C + _BOOL + _PH + _NR + ["cnt"],
    "gz_bm25_search_groups": _G + _BOOL + _OUT,
    "gz_bm25_search_groups_device": _G + _BOOL + _OUT,
    "gz_bm25_match_count_groups": ["alt_terms", "alt_off", "group_off", "nq"] + _BOOL + ["cnt"],
}
assert len(ENTRIES) == 15

_DTYPE = {"terms": np.int32, "idf": np.float64, "qoff": np.int64, "params": np.float64, "ex_terms": np.int32, "ex_off": np.int64,
          "ph_terms": np.int32, "ph_off": np.int64, "nr_terms": np.int32, "nr_off": np.int64, "nr_win": np.int64,
          "alt_terms": np.int32, "alt_off": np.int64, "group_idf": np.float64, "group_off": np.int64}
_SCALAR = ("nq", "plus", "k", "mode")


def is_device(entry):
    return entry.endswith("_device")


def is_count(entry):
    return "match_count" in entry


def call(lib, index, entry, req):
    """lib.<entry>(index, ...) with the arguments taken from req by name: arrays (None: a null pointer) are converted to the entry
    point's dtype; doc / score / cnt are addresses (int, host or device as the entry point wants them) or None."""
    keep, args = [], [ctypes.c_void_p(index)]
    for f in ENTRIES[entry]:
        v = req[f]
        if f in _SCALAR:
            args.append(int(v))
        elif v is None:
            args.append(None)
        elif f in _OUT:
            args.append(ctypes.c_void_p(int(v)))
        else:
            a = np.ascontiguousarray(v, dtype=_DTYPE[f])
            keep.append(a)
            args.append(ctypes.c_void_p(a.ctypes.data))
    return getattr(lib, entry)(*args)


# ---- the nine entry points that make or change an index -------------------------------------------------------------------------
# entry point -> all its arguments, in the order of include/genz_tokenize.h
CHANGES = {
    "gz_bm25_build": ["ctx", "text", "text_off", "n_docs", "out"],
    "gz_bm25_build_device": ["ctx", "text", "text_off", "n_docs", "text_bytes", "out"],
    "gz_bm25_build_ex": ["ctx", "text", "text_off", "n_docs", "flags", "out"],
    "gz_bm25_build_device_ex": ["ctx", "text", "text_off", "n_docs", "text_bytes", "flags", "out"],
    "gz_bm25_append": ["index", "text", "text_off", "n_docs"],
    "gz_bm25_append_device": ["index", "text", "text_off", "n_docs", "text_bytes"],
    "gz_bm25_remove": ["index", "ids", "n_ids"],
    "gz_bm25_remove_device": ["index", "ids", "n_ids"],
    "gz_bm25_compact": ["index"],
}
assert len(CHANGES) == 9
_CH_SCALAR = ("n_docs", "text_bytes", "flags", "n_ids")


def is_build(entry):
    return "build" in entry


def change(lib, entry, req):
    """lib.<entry>(...) with the arguments taken from req by name: the scalars are ints, every pointer is an address (int, host or
    device as the entry point wants it) or None; `out` of a build is a ctypes.c_void_p to receive the handle, or None."""
    args = []
    for f in CHANGES[entry]:
        v = req[f]
        if f in _CH_SCALAR:
            args.append(int(v))
        elif v is None:
            args.append(None)
        elif f == "out":
            args.append(ctypes.byref(v))
        else:
            args.append(ctypes.c_void_p(int(v)))
    return getattr(lib, entry)(*args)
