"""Best-fit packing over lists of ints, stated once and on its own (nothing of the product is imported), document by document,
and the shape lists the fit tests share.  tests/test_packfit_inputs.py ties `batch` to pack_oracle's segment and checks that the
lists hold the cases they are named for; tests/test_packfit_plan.py compares the host plan of csrc/gz_packfit.h with `place`;
tests/test_gpu_packfit.py compares the GPU with `batch`.

The rule.  L = max_len, len_r = min(T_r, L - 2) + 2.  The documents are taken in the order (len descending, index ascending).
Rows are numbered in the order they are opened; a row carries `free` (L at first) and `stamp` (the time of its last placement, a
counter that goes up by one per placed document).  A document of length l goes into the row with the smallest (free, stamp) among
the rows with free >= l; if there is none it opens row R, and R += 1.  Then doc_row = row, doc_col = L - free, free -= l,
stamp = ++t."""
import numpy as np

from pack_oracle import segment

# the constants of csrc/gz_packfit.inc and csrc/gz_kernels.hip the shapes below were written for: documents per tile of the rank
# pass (= 4 waves of 256 consecutive documents each), documents per workgroup of the fill, where the 64-bit scan switches kernels
TILE, WAVE_DOCS, FILL_DOCS, SCAN_SWITCH = 1024, 256, 256, 8 * 2048
MAX_LEN = 4096


def place(lens, L):
    """Best-fit-decreasing, sequentially: (doc_row, doc_col, R)."""
    order = sorted(range(len(lens)), key=lambda d: (-lens[d], d))
    free, stamp, t = [], [], 0
    doc_row, doc_col = [0] * len(lens), [0] * len(lens)
    for d in order:
        l = lens[d]
        best = None
        for row in range(len(free)):
            if free[row] >= l and (best is None or (free[row], stamp[row]) < (free[best], stamp[best])):
                best = row
        if best is None:
            best = len(free)
            free.append(L)
            stamp.append(0)
        doc_row[d], doc_col[d] = best, L - free[best]
        free[best] -= l
        t += 1
        stamp[best] = t
    return doc_row, doc_col, len(free)


def place_fast(lens, L):
    """`place` with the candidate rows kept by free space (the same decisions, for batches of thousands of documents)."""
    import bisect
    order = sorted(range(len(lens)), key=lambda d: (-lens[d], d))
    keys, R, t = [], 0, 0                                            # sorted (free, stamp, row) of every open row
    doc_row, doc_col = [0] * len(lens), [0] * len(lens)
    for d in order:
        l = lens[d]
        at = bisect.bisect_left(keys, (l, -1, -1))
        if at < len(keys):
            free, _, row = keys.pop(at)
        else:
            free, row, R = L, R, R + 1
        doc_row[d], doc_col[d] = row, L - free
        t += 1
        bisect.insort(keys, (free - l, t, row))
    return doc_row, doc_col, R


def batch(bodies, L, bos, eos, pad, fast=False):
    """The rule over many bodies, in the arrays the product returns for order="fit"."""
    segs = [segment(b, L, bos, eos) for b in bodies]
    lens = [len(s) for s in segs]
    doc_row, doc_col, R = (place_fast if fast else place)(lens, L)
    n = len(segs)
    row_docs = sorted(range(n), key=lambda d: (doc_row[d], doc_col[d]))
    ids = np.full((R, L), pad, dtype=np.int64)
    seg_ids, pos = np.zeros((R, L), dtype=np.int32), np.zeros((R, L), dtype=np.int32)
    row_off = np.zeros(R + 1, dtype=np.int64)
    in_row = 0
    for p, d in enumerate(row_docs):
        i, c, s = doc_row[d], doc_col[d], segs[d]
        in_row = 0 if c == 0 else in_row + 1
        ids[i, c:c + len(s)] = s
        seg_ids[i, c:c + len(s)] = in_row + 1
        pos[i, c:c + len(s)] = np.arange(len(s))
        row_off[i + 1] = p + 1
    seg_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        np.cumsum([lens[d] for d in row_docs], out=seg_off[1:])
    ids = ids.astype(np.int32)
    return dict(input_ids=ids, attention_mask=(ids != pad).astype(np.int32), segment_ids=seg_ids, position_ids=pos,
                doc_row=np.array(doc_row, dtype=np.int32), doc_col=np.array(doc_col, dtype=np.int32), doc_len=np.array(lens, dtype=np.int32),
                row_docs=np.array(row_docs, dtype=np.int32), row_off=row_off, seg_off=seg_off)


def unpack(result):
    """The segments of a fit result back in DOCUMENT order: (flat, row_off [N + 1])."""
    L = result["input_ids"].shape[1] if result["input_ids"].ndim == 2 else 0
    flat, off = [], [0]
    for d in range(len(result["doc_len"])):
        i, c, n = int(result["doc_row"][d]), int(result["doc_col"][d]), int(result["doc_len"][d])
        assert c + n <= L
        flat += result["input_ids"][i, c:c + n].tolist()
        off.append(off[-1] + n)
    return np.array(flat, dtype=np.int32), np.array(off, dtype=np.int64)


# ---- the shapes of tests/test_gpu_packfit.py: body lengths T (len = min(T, L - 2) + 2) -------------------------------------------
# max_len of the event and fill cases: the smallest rows, L % 4 of 0, 1, 2 and 3 (one cell a store and four), the largest row
EVENT_LS = (3, 4, 5, 10, 127, 128, 130, 4096)

# document counts at the rank pass's edges: a wave, a wave's run of documents, a tile, two tiles, the scan's switch
RANK_NS = sorted({63, 64, 65, WAVE_DOCS - 1, WAVE_DOCS, WAVE_DOCS + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, SCAN_SWITCH - 1, SCAN_SWITCH,
                  SCAN_SWITCH + 1})


def one_length(n, L):
    """Every document the same length (3 cells, or 2 where a row is 3): the rank runs across every wave and tile."""
    return [1 if L > 3 else 0] * n


def two_lengths(n):
    """Lengths 2 and 5 alternating: two ranks interleaved through every wave."""
    return [0, 3] * (n // 2) + [0] * (n % 2)


def every_length(L, times):
    """Every len 2 .. L `times` times, document order ascending by length (the reverse of the order they are placed in)."""
    return [T for T in range(0, L - 1) for _ in range(times)]


def event_edges(L):
    """A batch whose plan has events of every kind for one length: rows opened k a row with a partial last row, then a shorter
    length that fills old rows first (first and last rank of an event), ends in one partial row, and a third that opens new rows
    behind old ones.  Lengths a > b > c with a ~ 0.6 L.  That needs room for three lengths: it holds for L >= 127
    (tests/test_packfit_inputs.py checks each kind there).  At L = 3 and 4 every document has len 2 and at L = 5 and 10 there are two
    lengths, the shorter of which fills the old rows' free space and, at L = 5, opens new rows: those cases are there for the tiny rows
    of the fill (one cell a store at L = 3, 5, 10, four at L = 4), not for the events."""
    a = max(2, (3 * L) // 5)
    b = max(2, (L - a) // 2)
    c = 2
    la = [a - 2] * 5
    lb = [b - 2] * 7 if b != a else []
    lc = [c - 2] * (3 * (L // 2) + 3) if c not in (a, b) else [0] * 3
    out = []
    for k in range(max(len(la), len(lb), len(lc))):                 # interleaved: the rank is by index, not by position in a run
        for x in (lc, la, lb):
            if k < len(x):
                out.append(max(x[k], 0))
    return out


def exact_rows(L, k):
    """[2] * k + [L - 2] * k: exactly k full rows, where next-fit makes more."""
    return [0] * k + [L - 4] * k if L >= 6 else [0] * k


def one_cell_tail(L):
    """Rows that end one cell short: len L - 1 alone (L >= 3), and len L - 3 with a len 2 behind it."""
    return [L - 3] * 3 + ([L - 5, 0] * 2 if L >= 7 else [])
