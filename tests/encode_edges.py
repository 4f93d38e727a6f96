"""Document builders for the encode pipeline's edge suite (tests/test_gpu_encode_edges.py runs them on the GPU against the oracles,
tests/test_encode_edges_inputs.py proves on the CPU that every built case sits on the edge it is meant for).

The constants restate what the kernels are built around (gz_pipeline.inc, gz_hot.inc); nothing here computes an expected row.

  A  classification   1 024-byte tiles, 16 bytes a lane, 4 096-byte blocks: whitespace, line feeds, document starts and the end of
                      the text at those edges, beside tiles that take the fast form and tiles that take the general one
  B  word kernel      word lengths around the 16-byte key, the long-key table, the 32-bit end search and the 48 bytes of look-ahead;
                      word starts per tile around the rounds of 64
  C  miss lists       miss totals around the groups of 64 and the pre-pass tiles of 3 072, by symbol count
  D  dense rows       rounds of gz_rows1_kernel: CAP words and tokens, MLCAP merged words, documents per wave, the max_len classes
"""
import os
import random

import numpy as np

import gz_oracle as O

TILE, LANE, BLOCK = 1024, 16, 4096
DOC = 4096                       # a document of family A: one block of the pipeline, one workgroup of the one-launch kernel
LEAD = 2048                      # the leading document of the shifted batches: local offset 2 048 lands on block edges
SMALL_DOC, SMALL_TOTAL = 4096, 2 << 20      # the one-launch kernel takes batches of documents up to / a total up to
MPRE_TILE, MISS_GROUP = 3072, 64
MLCAP, RMAX = 96, 16

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genz-tokenize_amd", "genz_tokenize", "data")
WS = sorted(O.WHITESPACE)


class Batch:
    """One call: documents (bytes), what to call it with, and the marks the host-only test checks."""

    def __init__(self, name, docs, max_lens=(None, 1024), marks=(), **info):
        self.name, self.docs, self.max_lens, self.marks, self.info = name, list(docs), tuple(max_lens), list(marks), info
        self.off = np.zeros(len(self.docs) + 1, np.int64)
        np.cumsum([len(d) for d in self.docs], out=self.off[1:])
        raw = b"".join(self.docs)
        self.raw = raw
        self.text = np.frombuffer(raw + b"\0" * 16, np.uint8)[:len(raw)]        # (a view with readable bytes behind it, as _pack gives)

    @property
    def nbytes(self):
        return int(self.off[-1])

    def takes_one_launch(self):
        return len(self.docs) > 0 and max(len(d) for d in self.docs) <= SMALL_DOC and self.nbytes <= SMALL_TOTAL

    def strings(self, idx):
        return [self.docs[i].decode("utf-8") for i in idx]

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------------------------
# the fast-form rule of gz_classify_kernel, as DESIGN.md documents it
def plain_tile(tile: bytes) -> bool:
    """No control character, no byte that can lead a multi-byte whitespace character (C2, E2 and above), no 9A."""
    return not any(b < 0x20 or b >= 0xE2 or b == 0xC2 or b == 0x9A for b in tile)


def fast_tile(text: bytes, k: int) -> bool:
    """... and the tile does not end in E1 with 9A behind it (U+1680 cut 1|2 by the tile edge)."""
    tile = text[k * TILE:(k + 1) * TILE]
    cut = len(tile) == TILE and tile[-1] == 0xE1 and text[(k + 1) * TILE:(k + 1) * TILE + 1] == b"\x9a"
    return plain_tile(tile) and not cut


def vocab_words():
    """The bundled vocabulary's whole words (entries without the continuation suffix), in file order."""
    out = []
    for line in open(os.path.join(DATA, "vocab.txt"), "rb").read().decode("utf-8").split("\n"):
        line = line.strip()
        if line and " " in line:
            w = line[:line.rfind(" ")]
            if w and not w.endswith(O.CONT) and not any(ord(c) in O.WHITESPACE for c in w):
                out.append(w)
    return out


_VOCAB = None
_TABLES = None


def tables():
    """The oracle's tables of the bundled files (the builders use them to count pieces, never to make an expected row)."""
    global _TABLES
    if _TABLES is None:
        _TABLES = O.Tables(open(os.path.join(DATA, "vocab.txt"), "rb").read(), open(os.path.join(DATA, "bpe.codes"), "rb").read())
    return _TABLES


def vocab():
    global _VOCAB
    if _VOCAB is None:
        _VOCAB = vocab_words()
    return _VOCAB


_FILLER = None


def filler_words():
    """Short plain ASCII words of the vocabulary: running text whose tiles are eligible for the fast form."""
    global _FILLER
    if _FILLER is None:
        t = tables()
        _FILLER = []
        for w in vocab():
            if w.isascii() and w.isalpha() and w.islower() and 2 <= len(w) <= 6 and O.bpe_pieces(w, t.ranks) == [w]:
                _FILLER.append(w)
                if len(_FILLER) == 200:
                    break
        assert len(_FILLER) == 200
    return _FILLER


def filler(n, salt=0):
    """Exactly n bytes of filler words with single spaces between them."""
    ws = filler_words()
    out, size, i = [], 0, salt
    while size < n + 8:
        w = ws[(i * 7 + salt) % len(ws)]
        out.append(w); size += len(w) + 1; i += 1
    return bytearray(" ".join(out).encode("ascii")[:n])


def put(doc, at, item, guard=True):
    """item at doc[at ...], with letters on both sides of it."""
    assert 2 <= at and at + len(item) + 2 <= len(doc), (at, len(item), len(doc))
    doc[at:at + len(item)] = item
    if guard:
        doc[at - 2:at] = b"qz"
        doc[at + len(item):at + len(item) + 2] = b"zq"


# ---------------------------------------------------------------------------------------------------------------------------------
# A. classification
EDGES_P = (1024, 3072)           # documents of kind P carry their item at these local offsets (tiles 0|1 and 2|3) ...
EDGES_Q = (528, 2048)            # ... of kind Q at a lane edge inside tile 0 and at the edge of tiles 1|2: no two items share a tile
VARIANTS = ("plain", "before", "after", "both")     # where a general-form neighbour stands: a \t in the tile before, U+2003 in the tile behind


def ws_items():
    """(name, bytes, k, code point): each whitespace code point with k of its bytes in front of the edge, k = 0 .. its length (0 and
    the length: whole behind / whole in front of the edge), and the line-feed cases of the glue rule."""
    items = []
    for cp in WS:
        e = chr(cp).encode("utf-8")
        for k in range(len(e) + 1):
            items.append(("U+%04X %d|%d" % (cp, k, len(e) - k), e, k, cp))
    # "\S+\n?": a word that ends on the tile's last byte, its line feed the next tile's first
    items.append(("glue \\n", b"\n", 0, None))
    items.append(("glue \\n\\n", b"\n\n", 0, None))
    items.append(("glue \\r\\n", b"\r\n", 0, None))
    for cp in (0x85, 0x1680, 0x2003, 0x3000):       # a line feed directly behind a multi-byte whitespace character is not glued to anything
        e = chr(cp).encode("utf-8")
        items.append(("U+%04X then \\n" % cp, e + b"\n", len(e), None))
    return items


def neighbour_offsets(kind, variant):
    """Local offsets of the general-form neighbours: (\\t offsets, U+2003 offsets)."""
    # the tiles in front of / behind the document's edges (kind Q: the lane edge's tile is both)
    front = (100, 2148) if kind == "P" else (100, 1124)
    behind = (1124, 3172) if kind == "P" else (300, 2148)
    return (front if variant in ("before", "both") else ()), (behind if variant in ("after", "both") else ())


def a_document(kind, item, k, variant, salt):
    doc = filler(DOC, salt)
    doc[0:2] = b"qz"; doc[-2:] = b"zq"            # letters at both ends: only the document start separates it from its neighbours
    tabs, ems = neighbour_offsets(kind, variant)
    for at in tabs:
        put(doc, at, b"\t")
    for at in ems:
        put(doc, at, "\u2003".encode("utf-8"))
    for edge in (EDGES_P if kind == "P" else EDGES_Q):
        put(doc, edge - k, item)
    assert len(doc) == DOC
    return bytes(doc)


def family_a(variant, shifted):
    """All items at all edges, beside the neighbours of `variant`; `shifted`: behind one leading document of 2 048 bytes."""
    docs, marks = [], []
    if shifted:
        lead = filler(LEAD, 99); lead[-2:] = b"zq"
        docs.append(bytes(lead))
    for n, (name, item, k, cp) in enumerate(ws_items()):
        for kind in ("P", "Q"):
            for edge in (EDGES_P if kind == "P" else EDGES_Q):
                marks.append(dict(doc=len(docs), edge=edge, item=item, k=k, cp=cp, name=name, kind=kind, variant=variant))
            docs.append(a_document(kind, item, k, variant, n))
    return Batch("A-%s%s" % (variant, "-shifted" if shifted else ""), docs, marks=marks, shifted=shifted)


def family_a_boundaries():
    """Document starts on tile and block edges with letters on both sides (only the start bit separates the words), with one, two
    and 70 empty documents at such an edge, at a lane edge and inside a lane."""
    batches = []
    for empties in (0, 1, 2, 70):
        docs, marks = [], []
        for size in (1024, 3072, 4096, 4096, 2048, 1008, 16, 1024, 7, 1017, 4096):
            d = filler(size, size + empties)
            d[0:2] = b"qz"; d[-2:] = b"zq"
            docs.append(bytes(d))
            pos = sum(len(x) for x in docs)
            marks.append(dict(pos=pos, empties=empties))
            docs += [b""] * empties
        last = filler(500, 3); last[0:2] = b"qz"
        docs.append(bytes(last))
        batches.append(Batch("A-boundaries-%d-empty" % empties, docs, max_lens=(None, 1024, 8), marks=marks))
    # "\S+\n?" does not reach into the next document: a line feed as a document's first byte, behind a document that ends in a letter
    docs, marks = [], []
    for size in (1024, 3072, 4096, 2048, 1008, 16, 1024, 7, 1017, 4096):
        d = filler(size, size + 5)
        d[0:2] = b"\nq"; d[-2:] = b"zq"
        docs.append(bytes(d))
        marks.append(dict(pos=sum(len(x) for x in docs), empties=0, newline=True))
    docs.append(b"\nqz")
    batches.append(Batch("A-boundaries-line-feed", docs, max_lens=(None, 1024, 8), marks=marks))
    return batches


END_SIZES = (8192, 8193, 8192 + 15, 8192 + 16, 8192 + 17, 5120, 5121, 4096, 4097)
END_KINDS = ("word", "glued", "U+0085", "U+1680", "U+2003")


def family_a_text_end():
    """The end of the text: total sizes B = 0, 1, 15, 16, 17 (mod 16) and 0, 1 (mod 1 024 and mod 4 096); the last word ends exactly at
    B, or has a glued line feed at B - 1, or the last character is a multi-byte whitespace."""
    batches = []
    for B in END_SIZES:
        for kind in END_KINDS:
            body = filler(B, B % 97)
            tail = {"word": b"qzqz", "glued": b"qzq\n"}.get(kind) or b"qz" + chr(int(kind[2:], 16)).encode("utf-8")
            body[B - len(tail):] = tail
            body[B - len(tail) - 1:B - len(tail)] = b"z"
            raw = bytes(body)
            docs = [raw[:B % DOC]] * (B % DOC != 0) + [raw[i:i + DOC] for i in range(B % DOC, B, DOC)]      # (the short document first: the tail stays whole)
            batches.append(Batch("A-end-%d-%s" % (B, kind), docs, max_lens=(None, 1024), end=kind, size=B, tail=tail))
    return batches


TAIL_CASES = ((1026, (1024,)), (2050, (1024, 2048)), (4098, (1024, 3072, 4096)), (4096 + 15, (4096,)), (4096 + 16, (4096,)),
              (8192 + 5, (4096, 5120, 8192)), (3 * 4096, (8192, 9216, 11264)), (4 * 4096, (1024, 3072, 5120, 8192)))


def inner_block(p0, B):
    """gz_classify_kernel requests a block's four tiles at once when 16 bytes behind the block are still text; the last one or two
    blocks of a text are loaded tile by tile, with the careful load."""
    return p0 + BLOCK + 16 <= B


def family_a_tail_blocks():
    """U+1680 cut 1|2 by the tile edges of a text's last blocks, one case a batch (the tile in front stays plain): the byte behind the
    tile comes from the next tile's registers inside a block, from one byte loaded with the block for its last tile, and from a guarded
    load in the last blocks -- down to a text that ends with the character."""
    batches = []
    item = "\u1680".encode("utf-8")
    for B, edges in TAIL_CASES:
        for e in edges:
            body = filler(B, e % 89)
            body[e - 3:e - 1] = b"qz"
            body[e - 1:e + 2] = item
            if e + 4 <= B:
                body[e + 2:e + 4] = b"zq"
            raw = bytes(body)
            cuts = [0] + list(range(100, B, DOC)) + [B]            # (documents of at most 4 096 bytes, cut away from the tile edges)
            docs = [raw[a:b] for a, b in zip(cuts, cuts[1:])]
            batches.append(Batch("A-tail-%d-%d" % (B, e), docs, size=B, edge=e))
    return batches


# ---------------------------------------------------------------------------------------------------------------------------------
# B. word kernel
WORD_BYTES = (1, 12, 13, 16, 17, 32, 33, 48, 49, 80)
LOOKAHEAD = 48
TILE_WORDS = (63, 64, 65, 129, 512)


def hit_word(nbytes):
    """A whole word of the vocabulary of this many bytes that the merge loop leaves in one piece -- what the whole-word tables hold,
    up to 32 bytes (None: the bundled vocabulary has none: 48, 49 and 80)."""
    for w in vocab():
        if len(w.encode("utf-8")) == nbytes and O.bpe_pieces(w, tables().ranks) == [w]:
            return w
    return None


def invented_word(nbytes):
    """A word of this many bytes that is no entry of the vocabulary."""
    known = set(vocab())
    if nbytes == 1:                                  # (every letter is an entry: a printable ASCII character that is none)
        return next(chr(c) for c in range(0x7E, 0x20, -1) if chr(c) not in known)
    for salt in range(50):
        r = random.Random(1000 * nbytes + salt)
        w = "".join(r.choice("qxzwkjfvbp") for _ in range(nbytes))
        if w not in known:
            return w
    raise AssertionError(nbytes)


def straddles(nbytes):
    """Bytes of the word that lie in front of the edge: it starts in the last 1..48 bytes of a tile and ends in the next.  (A word
    of one byte cannot straddle: it stands on the tile's last byte, s = 1, and on the next tile's first, s = 0.)"""
    return (1, 0) if nbytes == 1 else tuple(range(1, min(LOOKAHEAD, nbytes - 1) + 1))


def family_b_words(kind):
    """Every word length, each start in the last 1..48 bytes of a tile, at the local offsets 1 024, 2 048 and 3 072 of 4 096-byte
    documents behind a leading document of 2 048 bytes: tile edges and a block edge of the pipeline."""
    lead = filler(LEAD, 98); lead[-2:] = b"zq"
    docs, marks = [bytes(lead)], []
    for nb in WORD_BYTES:
        w = hit_word(nb) if kind == "hit" else invented_word(nb)
        if w is None:
            continue
        wb = w.encode("utf-8")
        for s in straddles(nb):
            doc = filler(DOC, nb + s)
            doc[0:2] = b"qz"; doc[-2:] = b"zq"
            for edge in (1024, 2048, 3072):
                at = edge - s
                doc[at - 1:at] = b" "
                doc[at:at + nb] = wb
                doc[at + nb:at + nb + 1] = b" "
                marks.append(dict(doc=len(docs), edge=edge, at=at, word=w, nbytes=nb, s=s))
            docs.append(bytes(doc))
    return Batch("B-words-%s" % kind, docs, marks=marks, kind=kind)


def family_b_text_end():
    """The same words as the last word of the text: started in the last s bytes of a tile, ended exactly at the text's last byte."""
    batches = []
    for kind in ("hit", "invented"):
        for nb in WORD_BYTES:
            w = hit_word(nb) if kind == "hit" else invented_word(nb)
            if w is None:
                continue
            for s in sorted({straddles(nb)[0], straddles(nb)[-1]}):
                body = filler(DOC + 1024 - s - 1, nb) + b" " + w.encode("utf-8")
                raw = bytes(body)
                docs = [raw[:DOC], raw[DOC:]]
                batches.append(Batch("B-end-%s-%d-s%d" % (kind, nb, s), docs, word=w, at=DOC + 1024 - s, s=s, nbytes=nb))
    return batches


def tile_of_words(n):
    """1 024 bytes with exactly n word starts: n words, a space behind each (the tile starts with a letter and ends with a space)."""
    letters, base, extra = TILE - n, (TILE - n) // n, (TILE - n) % n
    assert base >= 1
    out = bytearray()
    for i in range(n):
        ln = base + (1 if i < extra else 0)
        out += bytes(97 + (i + j) % 26 for j in range(ln)) + b" "
    assert len(out) == TILE and letters == TILE - n
    return bytes(out)


def family_b_tiles():
    """Tiles of 63, 64, 65, 129 and 512 word starts (the last: "a a a ...", eight starts in a lane's 16 bytes, past the unrolled four),
    and a tile whose only word start is its last byte."""
    one = b" " * (TILE - 1) + b"a"                   # ... the word goes on in the next tile
    docs, marks = [], []
    order = [(63, 64, 65, 129), (512, 63, 512, 64), (129, 512, 65, 63)]
    for row in order:
        docs.append(b"".join(tile_of_words(n) for n in row))
        marks.append(dict(doc=len(docs) - 1, starts=row))
    docs.append(one + b"bcd " + filler(TILE - 4, 1) + one + b"bcd " + filler(TILE - 4, 2))
    marks.append(dict(doc=len(docs) - 1, starts=None, single=(0, 2)))
    docs.append(tile_of_words(512) * 4)
    marks.append(dict(doc=len(docs) - 1, starts=(512,) * 4))
    return Batch("B-tiles", docs, marks=marks, max_lens=(None, 1024, 64))


# ---------------------------------------------------------------------------------------------------------------------------------
# C. miss lists
MISS_TOTALS = (0, 1, 63, 64, 65, 3071, 3072, 3073, 6145)
MISS_FORMS = (1, 2, 8, 9, 16, "spread")
SYMBOLS = "abcdeghiklmnopqrstuvxyàáâãèéêìíòóôõùúýăđĩũơưạảấầẩẫậắằẳẵặẹẻẽếềểễệỉịọỏốồổỗộớờởỡợụủứừửữựỳỵỷỹ"


def miss_word(r, nsym):
    return "".join(r.choice(SYMBOLS) for _ in range(nsym))


def docs_of_words(words, limit=DOC):
    """The words, one space between them, cut into documents of at most `limit` bytes at spaces."""
    docs, cur, size = [], [], 0
    for w in words:
        b = len(w.encode("utf-8"))
        if cur and size + 1 + b > limit:
            docs.append(" ".join(cur).encode("utf-8")); cur, size = [], 0
        size += b + (1 if cur else 0)
        cur.append(w)
    docs.append(" ".join(cur).encode("utf-8"))
    return docs


def miss_counts(total, form):
    """Symbol counts of the batch's words."""
    if form != "spread":
        return [form] * total
    counts = [1 + i % 16 for i in range(total)]
    for at, c in ((total // 5, 17), (total // 3, 64), (total // 2, 65), (total - 1, 17)):      # the hand-over to the wide and long kernels
        if total >= 64:
            counts[at] = c
    return counts


def family_c(total, form):
    """`total` words, every one a miss with word_table=False."""
    r = random.Random(7 * total + (form if form != "spread" else 5))
    counts = miss_counts(total, form)
    words = [miss_word(r, c) for c in counts]
    docs = docs_of_words(words) if total else [b" " * 100, b"", b"   "]
    return Batch("C-%d-%s" % (total, form), docs, max_lens=(None, 256), counts=counts, words=words)


def family_c_blocks(tables_on):
    """Blocks without a miss between blocks full of them: 4 096 bytes of spaces (tables off), or of table hits only (tables on, where
    the misses are invented words); and one block with the most misses a block can hold: 2 048 one-letter words."""
    r = random.Random(31 + tables_on)
    known = set(vocab())
    hit = filler_words()[0]

    def full():
        ws = []
        while sum(len(w.encode("utf-8")) + 1 for w in ws) < DOC - 40:
            w = miss_word(r, r.choice((3, 5, 9, 12)))
            if w not in known:
                ws.append(w)
        b = " ".join(ws).encode("utf-8")
        return b + b" " * (DOC - len(b)), len(ws)

    def empty():
        if not tables_on:
            return b" " * DOC
        b = ((hit + " ") * (DOC // (len(hit) + 1) + 1)).encode("ascii")[:DOC - 1]
        return b[:b.rfind(b" ")].ljust(DOC, b" ")

    docs, misses = [], []
    for kind in "FEFEEEFFEEEEEEEEEF":
        if kind == "F":
            d, n = full()
            docs.append(d); misses.append(n)
        else:
            docs.append(empty()); misses.append(0)
    if not tables_on:
        docs.append(b" ".join(bytes([97 + i % 26]) for i in range(2048)) + b" "); misses.append(2048)
        docs.append(empty()); misses.append(0)
        d, n = full()
        docs.append(d); misses.append(n)
    return Batch("C-blocks-%s" % ("hits" if tables_on else "spaces"), docs, max_lens=(None, 256), misses=misses, tables_on=tables_on, hit=hit)


# ---------------------------------------------------------------------------------------------------------------------------------
# D. dense rows
def rows_class(max_len):
    """(CAP, documents per wave) of gz_rows1_kernel for this max_len (a multiple of 4 up to 1 024)."""
    assert max_len % 4 == 0 and 4 <= max_len <= 1024
    return (512, 8) if max_len <= 256 else (1024, 4) if max_len <= 512 else (1024, 1)


def rounds(words, tokens, max_len, merged=None):
    """The rounds of gz_rows1_kernel as its header comment and walk give them, for documents of words[d] words whose word w has
    tokens[d][w] tokens (merged[d][w]: a merged word, on the round's list).  A wave takes `documents per wave` consecutive documents
    and works in rounds: up to RMAX documents whose words, cut to max_len - 1 each, fit CAP; a document whose row (bos, tokens up to
    position max_len - 2, eos -- max_len - 1 entries when it is cut) does not fit what is left of CAP rolls back and opens the next
    round.  Returns one dict per round: wave, docs, words, entries, merged, rolled_back, overflow (more than MLCAP merged words)."""
    cap, dpw = rows_class(max_len)
    limit = max_len - 1
    out = []
    n = len(words)
    for wave, dbeg in enumerate(range(0, n, dpw)):
        dend = min(n, dbeg + dpw)
        da = dbeg
        while da < dend:
            nd, used = 0, 0
            while da + nd < dend and nd < RMAX and used + min(words[da + nd], limit) <= cap:
                used += min(words[da + nd], limit); nd += 1
            tb, nml, rolled, taken = 0, 0, False, 0
            for j in range(nd):
                d = da + j
                run, nml0 = 1, nml
                for w in range(min(words[d], limit)):
                    if run >= limit:
                        break
                    if tb + run < cap and merged is not None and merged[d][w]:
                        nml += 1
                    run += tokens[d][w]
                first = limit if run + 1 >= max_len else run + 1
                if tb + first > cap:
                    nml, rolled = nml0, True
                    break
                tb += first; taken += 1
            # (the kernel walks chunks of 64 words and ends a document's walk between chunks; a word at or behind position
            # max_len - 1 has no room and is not listed, so the count above ends at the same word)
            out.append(dict(wave=wave, docs=taken, words=sum(min(words[da + j], limit) for j in range(taken)), entries=tb, merged=nml,
                            rolled_back=rolled, overflow=nml > MLCAP))
            da += taken
    return out


def pieces_of(word):
    return len(O.bpe_pieces(word, tables().ranks))


def word_with_pieces(n, lo=2, hi=400):
    """An invented word the merge loop leaves in exactly n pieces (searched among consonant strings, which have few merges)."""
    known = set(vocab())
    for salt in range(4000):
        r = random.Random(salt * 131 + n)
        w = "".join(r.choice("qxzwkjfvbp") for _ in range(r.randint(max(lo, n), min(hi, n + 6))))
        if w not in known and pieces_of(w) == n:
            return w
    raise AssertionError("no word of %d pieces" % n)


def wide_word():
    """An invented word of 300 symbols: a far record of some 300 pieces."""
    r = random.Random(300)
    return "".join(r.choice("qxzwkjfvbp") for _ in range(300))


def hits(n, salt=0):
    ws = filler_words()
    return [ws[(salt + 3 * i) % len(ws)] for i in range(n)]


def d_doc(words):
    return " ".join(words).encode("utf-8")


D_SHAPES = ((4, 1), (4, 65), (8, 7), (12, 8), (16, 9), (252, 31), (256, 32), (256, 8), (260, 33), (512, 65), (516, 9), (1024, 8), (1024, 1))


def family_d_shapes(max_len, n_docs):
    """n_docs documents with word counts around max_len: 0, 1, max_len - 2, max_len - 1, max_len, many more, and in between."""
    sizes = (max_len - 2, 0, max_len - 1, 1, max_len, 3, 3 * max_len + 5, max_len // 2, 2, max_len - 3, 5 * max_len, max_len + 1)
    docs = [d_doc(hits(sizes[i % len(sizes)], i)) for i in range(n_docs)]
    return Batch("D-shape-%d-%d" % (max_len, n_docs), docs, max_lens=(max_len,), words=[sizes[i % len(sizes)] for i in range(n_docs)])


def family_d_cap(max_len, delta):
    """One wave's documents whose words, cut to max_len - 1 each, add up to CAP + delta."""
    cap, dpw = rows_class(max_len)
    limit = max_len - 1
    sizes = [limit + 40] + [0] * (dpw - 1)                      # the first is cut to max_len - 1
    left = cap + delta - limit
    for i in range(1, dpw):
        sizes[i] = min(left, (cap - limit) // (dpw - 1) + (9 if i % 2 else -9)) if i < dpw - 1 else left
        left -= sizes[i]
    assert left == 0 and all(0 < s <= limit for s in sizes[1:]), sizes
    docs = [d_doc(hits(s, i)) for i, s in enumerate(sizes)]
    return Batch("D-cap-%d%+d" % (max_len, delta), docs, max_lens=(max_len,), words=sizes)


def family_d_cap_rows(max_len, delta):
    """One round whose row entries add up to CAP + delta: two documents cut to max_len - 1 entries each and a third of 2 or 3 (or,
    for CAP - 1, a second document one entry short of the cut)."""
    cap, dpw = rows_class(max_len)
    assert dpw >= 3 and cap == 2 * (max_len - 1) + 2
    sizes = {-1: [max_len + 44, max_len - 4, 0], 0: [max_len + 44, max_len + 44, 0], 1: [max_len + 44, max_len + 44, 1]}[delta]
    return Batch("D-cap-rows-%d%+d" % (max_len, delta), [d_doc(hits(s, i)) for i, s in enumerate(sizes)], max_lens=(max_len,), words=sizes)


def family_d_rollback():
    """Two documents of 255 words and one of two at max_len 256: 512 words fit the round, 510 + 4 row entries do not."""
    sizes = [255, 255, 2, 9, 0, 30, 1, 255]
    return Batch("D-rollback", [d_doc(hits(s, i)) for i, s in enumerate(sizes)], max_lens=(256,), words=sizes)


def family_d_straddle(max_len, wide):
    """A merged word whose pieces straddle position max_len - 1: 2 of its pieces fit (5 pieces, or a wide word of some 300)."""
    w = wide_word() if wide else word_with_pieces(5)
    docs, toks = [], []
    for fit in (2, 1, 0, 5):                                     # pieces that fit in front of position max_len - 1
        pre = max(0, max_len - 2 - fit)
        docs.append(d_doc(hits(pre, fit) + [w] + hits(3, 1)))
        toks.append([1] * pre + [pieces_of(w)] + [1] * 3)
    return Batch("D-straddle-%d-%s" % (max_len, "wide" if wide else "5"), docs, max_lens=(max_len,), word=w, tokens=toks,
                 merged=[[t > 1 for t in row] for row in toks])


def family_d_merged(n_merged):
    """One wave of eight documents of 30 words at max_len 256 with n_merged merged words among table hits: two-piece words (near
    records) and, in two documents, a word of more than 16 pieces (a far record)."""
    two, far = word_with_pieces(2), word_with_pieces(17, lo=17)
    per = [n_merged // 8 + (1 if d < n_merged % 8 else 0) for d in range(8)]
    docs, toks, mrg = [], [], []
    for d in range(8):
        ws, tk, mg = [], [], []
        for i in range(30):
            m = i < per[d]
            word = (far if (d in (0, 5) and i == 0) else two) if m else hits(1, d * 30 + i)[0]
            ws.append(word); tk.append(pieces_of(word) if m else 1); mg.append(m)
        # (merged words and hits interleaved: the list index and the position walk disagree about order otherwise)
        order = sorted(range(30), key=lambda i: (i * 7) % 30)
        docs.append(d_doc([ws[i] for i in order])); toks.append([tk[i] for i in order]); mrg.append([mg[i] for i in order])
    return Batch("D-merged-%d" % n_merged, docs, max_lens=(256,), tokens=toks, merged=mrg, words=[30] * 8, two=two, far=far)


def family_d_empty():
    """Rounds that hold only empty documents, and empty documents around full ones."""
    docs = [b""] * 65 + [d_doc(hits(300, 1))] + [b""] * 9 + [d_doc(hits(5, 2))] + [b"", b" ", b"\n"]
    return Batch("D-empty", docs, max_lens=(8, 256, 1024), words=[0] * 65 + [300] + [0] * 9 + [5, 0, 0, 0])
