"""The refusal matrix of the five BM25 entry points that change a live index (gz_bm25_append, gz_bm25_remove, their _device forms,
and gz_bm25_compact), called through ctypes on a tiny index: every bad call answers one exact (return code, gz_last_error text), and
of two faults at once the one that the entry point checks first.  EXPECT holds what the library answered before these entry points
shared their prologue; nothing here is derived from the code under test.  A refused call leaves the live indexes bit-identical:
info, fieldLens, footprint, a score row.

Bad VALUES live in valid buffers, host or device.  The address 16 ("dangling") stands only in calls that are refused before anything
is read: the 2^32 limit, which gz_bm25_append_device answers before it looks at its pointers.

The four build entry points (bm25_tiny.CHANGES lists them) are not asked: a device build refused for its offsets faulted on the GPU
when this matrix was first run, against the library as it was before any change, and the cause is not known."""
import ctypes

import numpy as np
import pytest

import bm25_tiny as tiny
from genz_tokenize import _native
from genz_tokenize._packing import pack

ENTRIES = [e for e in tiny.CHANGES if not tiny.is_build(e)]
PAD = 7                                               # the device batch lies behind 7 bytes: offsets need not start at 0
BATCH = ["w0 w1", "w2 zz"]                            # 10 bytes
# offsets of two documents, by name
OFFS = {
    "good": [0, 5, 10],
    "dec": [0, 6, 4],                                 # decrease
    "end<start": [5, 6, 3],                           # text_off[n] < text_off[0]
    "leave": [0, 4, 11],                              # leave the 10 bytes a device form announces
    "neg": [-PAD - 1, 2, 3],                          # a negative first offset (the device form: -1 once PAD is added)
    "huge": [0, 1 << 31, 1 << 32],                    # 2^32 bytes: the limit, answered before the text is read
}
IDS = {"ids": [1, 5], "n_docs": [1, tiny.N_DOCS], "-1": [1, -1]}
HOST_ONLY, DEVICE_ONLY = "host", "device"

# (label, what the call changes in the good request, None or the forms it is asked of)
CASES = [
    ("null index", dict(index=None), None),
    ("n_docs -1", dict(n_docs=-1), None),
    ("n_ids -1", dict(n_ids=-1), None),
    ("text_bytes -1", dict(text_bytes=-1), None),
    ("null offsets", dict(text_off=None), None),
    ("null ids", dict(ids=None), None),
    ("null text", dict(text=None), None),
    ("decreasing offsets", dict(text_off="dec"), None),
    ("text_off[n] < text_off[0]", dict(text_off="end<start"), HOST_ONLY),
    ("offsets leave the text", dict(text_off="leave"), DEVICE_ONLY),
    ("negative first offset", dict(text_off="neg"), DEVICE_ONLY),
    ("id n_docs", dict(ids="n_docs"), None),
    ("id -1", dict(ids="-1"), None),
    ("2^32 bytes", dict(text_off="huge"), HOST_ONLY),
    ("2^32 bytes, nothing behind the call", dict(text="dangling", text_off="dangling", n_docs=5, text_bytes=1 << 32), None),
    ("n_docs 0", dict(n_docs=0, text=None, text_off=None), None),
    ("n_docs 0, text_bytes 0", dict(n_docs=0, text=None, text_off=None, text_bytes=0), None),
    ("n_ids 0", dict(n_ids=0, ids=None), None),
    # two faults at once: the order of the checks
    ("2^32 bytes + null pointers", dict(text=None, text_off=None, n_docs=1, text_bytes=(1 << 32) - 200), None),
    ("n_docs 0 + null offsets + text_bytes -1", dict(n_docs=0, text=None, text_off=None, text_bytes=-1), None),
    ("n_docs -1 + null index", dict(n_docs=-1, index=None), None),
    ("null text + decreasing offsets", dict(text=None, text_off="dec"), None),
    ("null text + text_off[n] < text_off[0]", dict(text=None, text_off="end<start"), HOST_ONLY),
    ("null ids + n_ids -1", dict(ids=None, n_ids=-1), None),
    ("n_ids 0 + null index", dict(n_ids=0, ids=None, index=None), None),
    ("text_bytes -1 + 2^32 documents", dict(text_bytes=-1, n_docs=1 << 32, text="dangling", text_off="dangling"), None),
]

_A, _AD, _R, _RD, _C = ("gz_bm25_" + n for n in ("append", "append_device", "remove", "remove_device", "compact"))

BAD, OFFSETS, TEXT_OFF = "bad arguments", "text offsets must not decrease", "bad text offsets"
LEAVE = "BM25 append: document offsets decrease or leave the 10 bytes of text"
OUTSIDE = "BM25 remove: a document id outside [0, 130)"
LIMIT = "BM25 index: %d bytes + %d documents; the index takes fewer than 2^32"

# label -> [return code, gz_last_error text (None: the call leaves the text as it was), the entry points that answer so, and -- where
# the answer depends on the bytes the index holds (1720 the plain one, 26 the positional one: its terms) -- the index]
EXPECT = {
    "null index": [[-1, None, (_A, _AD, _R, _RD, _C)]],
    "n_docs -1": [[-1, BAD, (_A, _AD)]],
    "n_ids -1": [[-1, BAD, (_R, _RD)]],
    "text_bytes -1": [[-1, BAD, (_AD,)]],
    "null offsets": [[-1, BAD, (_A, _AD)]],
    "null ids": [[-1, BAD, (_R, _RD)]],
    "null text": [[-1, TEXT_OFF, (_A,)], [-1, BAD, (_AD,)]],
    "decreasing offsets": [[-1, OFFSETS, (_A,)], [-1, LEAVE, (_AD,)]],
    "text_off[n] < text_off[0]": [[-1, TEXT_OFF, (_A,)]],
    "offsets leave the text": [[-1, LEAVE, (_AD,)]],
    "negative first offset": [[-1, "negative text offset", (_AD,)]],
    "id n_docs": [[-1, OUTSIDE, (_R, _RD)]],
    "id -1": [[-1, OUTSIDE, (_R, _RD)]],
    "2^32 bytes": [[-6, LIMIT % (4294969016, 132), (_A,), "plain"], [-6, LIMIT % (4294967322, 132), (_A,), "pos"]],
    "2^32 bytes, nothing behind the call": [[-6, LIMIT % (4294969016, 135), (_AD,), "plain"], [-6, LIMIT % (4294967322, 135), (_AD,), "pos"]],
    "n_docs 0": [[0, None, (_A, _AD)]],
    "n_docs 0, text_bytes 0": [[0, None, (_AD,)]],
    "n_ids 0": [[0, None, (_R, _RD)]],
    # (2^32 - 200 bytes: over the limit behind the plain index's 1720 bytes, not behind the positional index's 26)
    "2^32 bytes + null pointers": [[-6, LIMIT % (4294968816, 131), (_AD,), "plain"], [-1, BAD, (_AD,), "pos"]],
    "n_docs 0 + null offsets + text_bytes -1": [[-1, BAD, (_AD,)]],
    "n_docs -1 + null index": [[-1, None, (_A, _AD)]],
    "null text + decreasing offsets": [[-1, TEXT_OFF, (_A,)], [-1, BAD, (_AD,)]],
    "null text + text_off[n] < text_off[0]": [[-1, TEXT_OFF, (_A,)]],
    "null ids + n_ids -1": [[-1, BAD, (_R, _RD)]],
    "n_ids 0 + null index": [[-1, None, (_R, _RD)]],
    "text_bytes -1 + 2^32 documents": [[-1, BAD, (_AD,)]],
}


def applies(entry, change, forms):
    if forms is not None and (forms == DEVICE_ONLY) != tiny.is_device(entry):
        return False
    return all(f in tiny.CHANGES[entry] for f in change)


def expected(entry, label, kind):
    for rc, text, entries, *which in EXPECT.get(label, ()):
        if entry in entries and which in ([], [kind]):
            return rc, text
    return None


class World:
    MARK = "width = 0; a snippet takes width >= 1"

    def __init__(self):
        self.ctx = ctx = _native.Context()
        self.lib = ctx.lib
        self.live = {"plain": self.build(False), "pos": self.build(True)}
        assert ctx.bm25_info(self.live["pos"])[:2] == (tiny.N_DOCS, len(tiny.VOCAB))
        self.text, good = pack(BATCH)
        assert good.tolist() == OFFS["good"] and not set(OFFS) & set(IDS)
        self.host = {k: np.array(v, np.int64) for k, v in list(OFFS.items()) + list(IDS.items())}
        self.dev = {}
        for k, v in self.host.items():                                   # (the device form's offsets count from the padded buffer)
            self.dev[k] = ctx.alloc(v.nbytes)
            ctx.h2d(self.dev[k], v + PAD if k in OFFS else v)
        self.dev_text = ctx.alloc(64)
        ctx.h2d(self.dev_text, np.concatenate([np.full(PAD, 32, np.uint8), self.text, np.full(64 - PAD - len(self.text), 32, np.uint8)]))

    def build(self, positions):
        buf, off = pack(tiny.documents())
        return self.ctx.bm25_build(buf, off, positions=positions)

    def request(self, entry, change, index):
        dev = tiny.is_device(entry)
        req = dict(index=index, text=self.dev_text if dev else self.text.ctypes.data, text_off="good", n_docs=2, text_bytes=len(self.text),
                   ids="ids", n_ids=2)
        req.update(change)
        for f in ("text", "text_off", "ids"):
            if req[f] == "dangling":
                req[f] = 16
            elif isinstance(req[f], str):
                req[f] = self.dev[req[f]] if dev else self.host[req[f]].ctypes.data
        return req

    def last_error(self):
        return self.lib.gz_last_error(self.ctx.handle).decode("utf-8", "replace")

    def answer(self, entry, change, index):
        """(return code, text) of the good request on `index` with `change` applied; text None when the call left the text alone"""
        req = self.request(entry, change, index)
        # a refusal of another entry point with a text no changing call has: whether the call under test wrote a text shows
        q = np.array([0, 0], np.int64)
        assert self.lib.gz_bm25_snippets(ctypes.c_void_p(self.live["pos"]), None, ctypes.c_void_p(q.ctypes.data), 1, None, 0, 0, None,
                                         None) == _native.GZ_E_INVALID
        assert self.last_error() == self.MARK
        rc = tiny.change(self.lib, entry, req)
        text = self.last_error()
        return rc, (None if text == self.MARK else text)

    def state(self):
        """of both live indexes: info, fieldLens, footprint and one score row, as bits"""
        ctx, out = self.ctx, []
        for index in self.live.values():
            lens = ctx.bm25_field_lengths(index)
            row = ctx.bm25_score(index, [0, 1], [1.0, 1.5], [0, 2], [2.2, 1.2, 0.25, 0.75, float(np.mean(lens)), 0.0], False)
            out.append((ctx.bm25_info(index), lens.tolist(), ctx.bm25_footprint(index), row.view(np.uint64).tolist()))
        return out

    def close(self):
        for d in list(self.dev.values()) + [self.dev_text]:
            self.ctx.free(d)
        for ix in self.live.values():
            self.ctx.bm25_destroy(ix)
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "pos"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals(world, entry, kind):
    before = world.state()
    wrong = []
    for label, change, forms in CASES:
        if not applies(entry, change, forms):
            continue
        got, want = world.answer(entry, change, world.live[kind]), expected(entry, label, kind)
        print("%-5s %-24s %-42s -> %r" % (kind, entry, label, got))
        if want is None or got != tuple(want):
            wrong.append((label, got, want))
        if world.state() != before:
            wrong.append((label, "a live index changed"))
            break
    assert not wrong, wrong
    # the good request is one: the refusals above were refusals of what they changed.  (On an index of its own.)
    scratch = world.build(kind == "pos")
    assert world.answer(entry, {}, scratch) == (_native.GZ_OK, None)
    want_docs = {"append": tiny.N_DOCS + 2, "remove": tiny.N_DOCS - 2, "compact": tiny.N_DOCS}[entry.split("_")[2]]
    assert world.ctx.bm25_info(scratch)[0] == want_docs
    world.ctx.bm25_destroy(scratch)
    assert world.state() == before


def test_every_expectation_is_asked():
    asked = {(e, label) for label, change, forms in CASES for e in ENTRIES if applies(e, change, forms)}
    held = [(e, label, k) for label, rows in EXPECT.items() for _, _, entries, *which in rows for e in entries for k in which or ["plain", "pos"]]
    assert len(held) == len(set(held)) and {(e, label, k) for e, label in asked for k in ("plain", "pos")} == set(held)
