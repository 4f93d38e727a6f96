"""The packing rule over lists of ints, stated once and on its own (nothing of the product is imported), and the shape lists the
pack tests share.  tests/test_pack_inputs.py ties `segment` to the reference's restatement and checks that the lists hold the
cases they are named for; tests/test_gpu_packs.py compares the GPU with `batch`."""
import numpy as np

# the constants of csrc/gz_packrows.inc the shapes below were written for: documents per tile of the break chain, documents
# per group of tiles, documents per workgroup of the fill
TILE, GROUP, FILL_DOCS = 1024, 16 * 1024, 256


def segment(body, L, bos, eos):
    """Document -> its segment: the frame around at most L - 2 body tokens (len in [2, L])."""
    return [bos] + list(body[:L - 2]) + [eos]


def place(lens, L):
    """Next-fit, order kept: (doc_row, doc_col, R)."""
    used, row, doc_row, doc_col = 0, 0, [], []
    for n in lens:
        if used + n > L:
            row, used = row + 1, 0
        doc_row.append(row)
        doc_col.append(used)
        used += n
    return doc_row, doc_col, (row + 1 if lens else 0)


def batch(bodies, L, bos, eos, pad):
    """The rule over many bodies, in the arrays the product returns."""
    segs = [segment(b, L, bos, eos) for b in bodies]
    lens = [len(s) for s in segs]
    doc_row, doc_col, R = place(lens, L)
    ids = np.full((R, L), pad, dtype=np.int64)
    seg_ids, pos = np.zeros((R, L), dtype=np.int32), np.zeros((R, L), dtype=np.int32)
    row_off = np.zeros(R + 1, dtype=np.int64)
    in_row = 0
    for r, s in enumerate(segs):
        i, c = doc_row[r], doc_col[r]
        in_row = 0 if c == 0 else in_row + 1
        ids[i, c:c + len(s)] = s
        seg_ids[i, c:c + len(s)] = in_row + 1
        pos[i, c:c + len(s)] = np.arange(len(s))
        row_off[i + 1] = r + 1
    seg_off = np.zeros(len(segs) + 1, dtype=np.int64)
    if segs:
        np.cumsum(lens, out=seg_off[1:])
    ids = ids.astype(np.int32)
    return dict(input_ids=ids, attention_mask=(ids != pad).astype(np.int32), segment_ids=seg_ids, position_ids=pos,
                doc_row=np.array(doc_row, dtype=np.int32), doc_col=np.array(doc_col, dtype=np.int32), doc_len=np.array(lens, dtype=np.int32),
                row_off=row_off, seg_off=seg_off)


# max_len: the smallest row, L % 4 of 0, 1, 2 and 3, rows of one store, of a wave's width and beyond
RULE_LS = (3, 4, 5, 7, 10, 64, 65, 256, 257)


def edge_lengths(L):
    """Body lengths at the rule's edges: nothing, one token, one short of / exactly / one past what a row takes, two rows' worth."""
    return [0, 1, L - 3, L - 2, L - 1, 2 * L]


def exact_fill(L):
    """Bodies whose rows fill to exactly L (two documents), and to L + 1 (the second opens a row), alternating."""
    a = (L - 4) // 2
    b = L - 4 - a
    return [a, b, a, b + 1, b, a, a + 1, b, 0, L - 4, 1, L - 4] if L >= 4 else [1, 1, 0, 1]


def never_merge(lead):
    """L = 10, every len 5: two documents a row.  The chain from an even document visits the even ones, the chain from an odd one
    the odd ones, and the two never meet.  lead=True puts one document of len 10 in front, which makes the heads odd."""
    n = 2 * TILE + 3
    return ([8] if lead else []) + [3] * (n - (1 if lead else 0))


def long_row():
    """(L, body lengths): empty bodies, L = 2 TILE + 6 -> TILE + 3 documents a row, N = 3 TILE + 5: a row is longer than a tile, a
    tile's only head lies 3 and 6 documents into it, and most documents' heads lie in the tile before their own."""
    return 2 * TILE + 6, [0] * (3 * TILE + 5)


def skipped_tile():
    """(L, body lengths): empty bodies, L = 4 TILE + 6 -> 2 TILE + 3 documents a row, N = 3 TILE + 5: two rows, heads 0 and
    2 TILE + 3; the chain passes over tile 1 entirely (a row has to span two tiles' worth of documents for that)."""
    return 4 * TILE + 6, [0] * (3 * TILE + 5)


BLOCK_EDGE_NS = sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097,
                        FILL_DOCS - 1, FILL_DOCS, FILL_DOCS + 1, TILE - 1, TILE, TILE + 1, GROUP - 1, GROUP, GROUP + 1})
BLOCK_EDGE_LS = (7, 12)

ALIGN_LENGTHS = list(range(41))          # successive rows of 0 .. 40 tokens: the rows start at the triangular numbers
ALIGN_LS = (10, 16)

# words of the end-to-end texts: whole-word hits, words that split into several pieces, one word outside the vocabulary
WORDS = ["sinh_viên", "công_nghệ", "hello", "xin", "chào", "Việt_Nam", "học", "máy", "a", "và", "là", "của", "tokenization",
         "internationalization", "GPU", "2024", "thế_giới", "không", "một", "người", "trường_đại_học", "zzqxj中q", "nghiên_cứu", "!"]


def texts(n, max_words, seed):
    import random
    r = random.Random(seed)
    return [" ".join(r.choice(WORDS) for _ in range(r.randint(0, max_words))) for _ in range(n)]
