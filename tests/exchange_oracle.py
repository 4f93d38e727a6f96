"""The exchange step's rule in numpy, stated once and on its own: dense rows <-> their leading entries, the block
[n_real | first | entries] a rank sends, and what the receiving side accepts of a block.  Nothing of the product is imported but
`distributed.block_words` (host arithmetic only).  tests/test_exchange_inputs.py ties the functions to answers written out by hand
and checks that the shape lists hold the cases they are named for; tests/test_gpu_exchange.py compares the GPU with them."""
import numpy as np

from genz_tokenize.distributed import block_words

# the constants the shapes below were written for
WAVE = 64                    # lanes of a wave: gz_kernels.hip, `constexpr int WAVE = 64`
ROWS_PER_WAVE = 8            # rows a wave of gz_compact_kernel takes side by side: gz_pipeline.inc, `#define GZ_CK 8`
WAVES = 4                    # waves per workgroup of the compact and expand kernels: gz_pipeline.inc, `#define GZ_PWPB 4`
SCAN_TRIP = 4096             # elements per trip of gz_scan32_kernel (`base += 4096`) = per workgroup of gz_scan32x_local_kernel (`SC32`)
SCAN_SWITCH = 8 * 4096       # gz_launch_row_offsets: `n_rows >= 8 * SC32` takes the three-kernel scan
BASES_TRIP = 1024            # blocks per trip of gz_scan32x_bases_kernel (`base += 1024`)

U32 = 0xFFFFFFFF


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def scan(n_real):
    """Exclusive sum of uint32(n_real) modulo 2^32, n + 1 values."""
    t = np.asarray(n_real, dtype=np.int64) & U32
    first = np.zeros(len(t) + 1, dtype=np.int64)
    np.cumsum(t, out=first[1:])
    return (first & U32).astype(np.uint32)


def compact(ids, n_real):
    """(entries, first, total): the rows' leading n_real[r] cells back to back, where each row starts (n + 1 values), how many."""
    ids = np.asarray(ids)
    n_real = np.asarray(n_real, dtype=np.int64)
    n, L = ids.shape
    assert n_real.shape == (n,) and ((n_real >= 0) & (n_real <= L)).all()
    keep = np.arange(L)[None, :] < n_real[:, None]
    return ids[keep].astype(np.int32), scan(n_real), int(n_real.sum())


def layout(n_real, first, entries, bits):
    """(words, defined): the int32 words [n_real | first | entries] of a block, entries of 16 bits little-endian and two to a word;
    `defined`: how many bytes of the last word the block defines (2 behind an odd number of 16-bit entries, else 4)."""
    n_real = np.asarray(n_real, dtype=np.int64)
    first = np.asarray(first, dtype=np.int64)
    entries = np.asarray(entries, dtype=np.int64)
    assert bits in (16, 32) and n_real.shape == first.shape
    head = np.concatenate([n_real & U32, first & U32]).astype("<u4").tobytes()
    if bits == 32:
        body, defined = (entries & U32).astype("<u4").tobytes(), 4
    else:
        assert ((entries >= 0) & (entries <= 0xFFFF)).all()
        odd = len(entries) % 2
        body, defined = entries.astype("<u2").tobytes() + b"\0\0" * odd, 2 if odd else 4
    words = np.frombuffer(head + body, dtype="<i4").astype(np.int32)
    assert len(words) == block_words(len(n_real), len(entries), bits)
    return words, defined


def block(ids, n_real, bits):
    """(words, defined) of the block gz_compact_block writes from dense rows."""
    entries, first, _ = compact(ids, n_real)
    return layout(n_real, first[:-1], entries, bits)


def split(words, n, total, bits):
    """(n_real, first, entries) of a block's words."""
    words = np.ascontiguousarray(words, dtype=np.int32)
    body = words[2 * n:]
    entries = body.copy() if bits == 32 else body.view(np.uint16)
    return words[:n].copy(), words[n:2 * n].view(np.uint32).copy(), entries[:total]


class Expanded:
    def __init__(self, ids, mask, bad, max_read):
        self.ids, self.mask, self.bad, self.max_read = ids, mask, bad, max_read


def expand(entries, first, n_real, L, pad, total):
    """What the receiving side makes of a block: with t = uint32(n_real[r]), row r is refused when t > L or uint64(first[r]) + t >
    total and is then all `pad`; an accepted row is entries[first[r] : first[r] + t], then `pad`.  mask = ids != pad.  `bad`: a row
    was refused; `max_read`: the largest entry index an accepted row reads (-1: none).  uint16 entries are values 0 .. 65535."""
    entries = np.asarray(entries)
    t = np.asarray(n_real, dtype=np.int64) & U32
    o = np.asarray(first, dtype=np.int64)[:len(t)] & U32
    refused = (t > L) | (o + t > int(total))
    t = np.where(refused, 0, t)
    cols = np.arange(L, dtype=np.int64)
    keep = cols[None, :] < t[:, None]
    src = (o[:, None] + cols[None, :])[keep]
    ids = np.full((len(t), L), pad, dtype=np.int32)
    ids[keep] = entries.astype(np.int64)[src].astype(np.int32)       # (an index past the entries raises: nothing is made up)
    return Expanded(ids, (ids != pad).astype(np.int32), bool(refused.any()), int(src.max()) if src.size else -1)


def expand_scanned(entries, n_real, L, pad):
    """gz_expand_rows: no `first` travels, the receiver scans n_real again; every entry index below 2^32 counts as announced."""
    return expand(entries, scan(n_real), n_real, L, pad, U32)


def dense(ids, n_real, pad):
    """The rows with everything behind their real entries set to `pad`: what a round trip has to give back."""
    ids = np.asarray(ids, dtype=np.int32)
    keep = np.arange(ids.shape[1])[None, :] < np.asarray(n_real, dtype=np.int64)[:, None]
    return np.where(keep, ids, np.int32(pad)).astype(np.int32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def counting_rows(n_real, L, base=1000):
    """int32 [n, L]: every real cell holds its own value, counting up from `base` across the batch (below 65536 for the batches of
    the 16-bit tests), so an entry taken from the wrong place shows; every cell behind a row's real entries holds its own NEGATIVE
    value -- junk that must never come out of a compact call."""
    n_real = np.asarray(n_real, dtype=np.int64)
    cell = np.arange(len(n_real) * L, dtype=np.int64).reshape(len(n_real), L)
    keep = np.arange(L)[None, :] < n_real[:, None]
    return np.where(keep, base + cell, -1 - cell).astype(np.int32)


# a. row lengths around the wave: the first 64 entries of a row are read side by side, what lies beyond in a loop of its own
ROW_LS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200)
AROUND_WAVE = (WAVE - 2, WAVE - 1, WAVE, WAVE + 1, WAVE + 2, 2 * WAVE - 2, 2 * WAVE - 1, 2 * WAVE, 2 * WAVE + 1, 2 * WAVE + 2)


def edge_counts(L):
    """The n_real values a batch of row length L has to hold."""
    return sorted({0, 1, L - 1, L} | {v for v in AROUND_WAVE if v <= L})


def edge_batch(L, times=3, seed=0):
    """n_real of one batch: every value of edge_counts(L) `times` times in shuffled order; an empty row first and last, and one
    between two full rows."""
    rng = np.random.default_rng(1000 * L + seed)
    body = np.array(edge_counts(L) * times, dtype=np.int32)
    rng.shuffle(body)
    h = len(body) // 2
    return np.concatenate([[0], body[:h], [L, 0, L], body[h:], [0]]).astype(np.int32)


# b. row counts around a wave's 8 rows and a workgroup's 32
ROW_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257)
ROW_COUNT_L = 5


def count_batch(n, seed=0):
    """Random n_real in [0, ROW_COUNT_L]; the first wave's eighth row is never empty."""
    b = np.random.default_rng(77 * n + seed).integers(0, ROW_COUNT_L + 1, size=n).astype(np.int32)
    if n >= ROWS_PER_WAVE:
        b[ROWS_PER_WAVE - 1] = max(int(b[ROWS_PER_WAVE - 1]), 1)
    return b


# c. the scan: trips of 4 096, the switch to three kernels at 8 * 4 096, blocks above it, a second trip of the bases
SCAN_NS = (4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 36863, 36864, 36865)
SCAN_L = 2
SCAN_BIG_N, SCAN_BIG_L = BASES_TRIP * SCAN_TRIP + 1, 1
SCAN_BIG_NS = (SCAN_BIG_N - 1, SCAN_BIG_N)       # 1 025 blocks both; at the smaller one the last block holds out[n] alone


def scan_batch(n, L, seed=0):
    """Random n_real in [0, L]; the last row is never empty, so a lost tail of the scan shows in the entries as well."""
    nr = np.random.default_rng(n + seed).integers(0, L + 1, size=n).astype(np.int32)
    nr[-1] = L
    return nr


# g. tiny batches of gz_encode_emit_block: a document that any of the row lengths cuts, an empty one, whitespace only, then others
EMIT_NS = (1, 7, 8, 9, 33)
EMIT_LS = (4, 6, 8)
EMIT_TEXTS = ["sinh_viên công_nghệ hello xin chào Việt_Nam học máy và là của", "", " \t\n  ", "a", "xin chào", "hello",
              "tokenization internationalization", " học máy ", "GPU 2024 !", "zzqxj中q", "một người"]


def emit_texts(n):
    return [EMIT_TEXTS[k % len(EMIT_TEXTS)] + (" a" * (k // len(EMIT_TEXTS))) for k in range(n)]
