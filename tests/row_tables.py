"""Vocabularies other than the bundled one for the calls that shape rows (window_rows, pack_rows, mask_rows, infill_rows and their
encode_* / *_to_device forms), and what the kernels should see of each: test_row_tables_inputs.py checks them on the CPU,
test_gpu_row_tables.py runs the GPU on them.  Nothing here imports the library, the oracle or numpy: a table is the bytes of a vocab
file and of a merges file, and its numbers come from `decode_tables.load`, the ten-line restatement of the loader rule
(tokenize.py:31-51) that test_row_tables_inputs.py holds against gz_oracle.Tables on every family.

What the row calls read of a table (include/genz_tokenize.h, the mask rule):
  the special ids    pad, bos, eos and <mask>, looked up in the LIVE encoder at call time
  n_ids, cont        the decoder SNAPSHOT of the first vocab load: largest id + 1, and the ids whose word ends in "@@", where on an
                     id collision the last word wins; an id outside the snapshot or absent from it continues nothing
  size               len(encoder) of the live table: the default random_ids of mask_rows is (5, size)

How ids move (tokenize.py:51 takes the size BEFORE the insert): a word the encoder holds already takes the id len(encoder) and leaves
its old id without a word; the size has not grown, so the next NEW word takes that id as well and, being later in the dict, wins it
in the decoder.  A moved word therefore shares its id with the next new word unless it is the file's last line.

Families:
  moved()      300 filler words, half of them ending in "@@", the pieces a small merges file makes, and <pad>, <s>, </s>, <mask>
               listed again between them: the four ids become large, different and far apart, ids 0..3 keep no word
  renamed()    the same file under other special strings, four of them words of the file (one ends in "@@")
  collide()    repeated words: an id won by a "@@" word over a plain one and one won the other way, holes, the empty word, "@@"
  edge(n)      n_ids = n exactly, no repeats: the words with ids n - 1, n - 2, 31, 32 and 5 end in "@@" and no other word does
  big(n)       n_ids = n exactly, short words "w<hex>", a seeded half ending in "@@"; ids 5, 31, 32 and the top 40 always do
  grown()      moved(), then a second file: new words (some "@@"), a continuation word of the first file moved, <mask> and </s>
               moved again (the ids they held stay with the "@@" words that shared them: ordinary tokens now)

Everything is deterministic; seeded choices use random.Random(seed).random() alone."""
import random

from decode_tables import SPECIALS, load

HEADER = b"#version: 0.2\n"
# merges over the letters a .. e: "ab", "cd" and "abcd" anywhere in a word, "ba" and "de" at its end
BPE = HEADER + b"a b\nc d\nab cd\nb a</w>\nd e</w>\n"
# every piece those merges can make of a word over "abcde" (a piece that is not the word's last is written "piece@@")
PIECES = [x + t for x in ("a", "b", "c", "d", "e", "ab", "cd", "abcd") for t in ("", "@@")] + ["ba", "de"]
TEXT_LETTERS = "abcdez"                                  # 'z' is in no word: it becomes <unk>

RENAMED = ("m200", "m150", "m250", "m101@@", "[UNK]")    # pad, bos, eos, mask, unk
EDGE_NS = (32, 33, 63, 64, 65, 96)
BIG_NS = (393216, 393217)                                # 48 KB of bitmap and one id more (GZ_MASK_LDS_MAX_BYTES)


def _filler(k):
    return "m%03d" % k + ("@@" if k % 2 else "")


def moved_vocab():
    lines = []
    again = {41: "<pad>", 120: "<s>", 201: "</s>", 271: "<mask>"}      # behind <pad> and <mask> comes a "@@" word, which shares the id
    for k in range(300):
        if k in again:
            lines.append(again[k] + " 1")
        lines.append("%s %d" % (_filler(k), 1 + k % 7))
        if k % 11 == 0 and k // 11 < len(PIECES):
            lines.append(PIECES[k // 11] + " 2")
    assert 11 * len(PIECES) < 300
    return ("\n".join(lines) + "\n").encode("utf-8")


def collide_vocab():
    lines = ["p0 1", "c0@@ 1", "p1 1",
             "p0 2", "c1@@ 1",                           # p0 moves to 8 and c1@@ takes 8 too: a "@@" word wins the id over a plain one
             "p2 1",
             "c0@@ 2", "p3 1",                           # c0@@ moves to 10 and p3 takes 10: a plain word wins it over a "@@" one
             " 1", "@@ 1"]                               # the empty word, and the word that is "@@" and nothing else
    for k in range(4, 30):
        lines.append(("c%d@@ 1" if k % 3 else "p%d 1") % k)
    lines += ["p1 3", "p1 4", "c30@@ 1",                 # moved twice before the next new word comes
              "p31 1", "c32@@ 1", "p33 1", ""]           # the blank last line moves the empty word to the largest id, alone
    return ("\n".join(lines) + "\n").encode("utf-8")


def edge_vocab(n):
    ends = {n - 1, n - 2, 31, 32, 5}
    return "".join("e%d%s 1\n" % (i, "@@" if i in ends else "") for i in range(5, n)).encode("utf-8")


def big_ends(n):
    """the ids of big(n) whose word ends in "@@" """
    r = random.Random(n)
    always = {5, 31, 32} | set(range(n - 40, n))
    return [i for i in range(5, n) if (r.random() < 0.5) | (i in always)]


def big_vocab(n):
    ends = set(big_ends(n))
    return "".join("w%x%s 1\n" % (i, "@@" if i in ends else "") for i in range(5, n)).encode("utf-8")


GROWN_MOVED_WORD = "m051@@"


def grown_second():
    return ("g0 1\ng1@@ 1\ng2@@ 1\n%s 1\ng3 1\n<mask> 1\ng4 1\ng5@@ 1\n</s> 1\n" % GROWN_MOVED_WORD).encode("utf-8")


class Table:
    """A family member: the files' bytes, the snapshot's numbers and the live table's (the same unless a second file came)."""

    def __init__(self, name, vocab, merges=HEADER, specials=SPECIALS, second=None):
        self.name, self.vocab, self.merges, self.specials, self.second = name, vocab, merges, tuple(specials), second
        self.snap_encoder, self.decoder = load(vocab, self.specials)
        self.n_ids = max(self.decoder) + 1
        self.cont = sorted(i for i, w in self.decoder.items() if w.endswith("@@"))
        self.snap_ids = tuple(self.snap_encoder[s] for s in self.specials[:4])
        self.encoder = self.snap_encoder if second is None else load(second, encoder=self.snap_encoder)[0]
        self.size = len(self.encoder)
        self.pad, self.bos, self.eos, self.mask = self.ids = tuple(self.encoder[s] for s in self.specials[:4])
        self.protected = set(self.ids)

    def absent(self, i):
        return i not in self.decoder

    def last_word_ids(self):
        """the snapshot's ids that lie in the last word of its bitmap"""
        return [i for i in range((self.n_ids - 1) & ~31, self.n_ids) if i in self.decoder]


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def moved():
    return _once("moved", lambda: Table("moved", moved_vocab(), BPE))


def renamed():
    return _once("renamed", lambda: Table("renamed", moved_vocab(), BPE, RENAMED))


def collide():
    return _once("collide", lambda: Table("collide", collide_vocab()))


def edge(n):
    return _once("edge%d" % n, lambda: Table("edge%d" % n, edge_vocab(n)))


def big(n):
    return _once("big%d" % n, lambda: Table("big%d" % n, big_vocab(n)))


def grown():
    return _once("grown", lambda: Table("grown", moved_vocab(), BPE, second=grown_second()))


def table(key):
    """'moved', 'renamed', 'collide', 'grown', 'edge64', 'big393216', ..."""
    for prefix, make in (("edge", edge), ("big", big)):
        if key.startswith(prefix):
            return make(int(key[len(prefix):]))
    return {"moved": moved, "renamed": renamed, "collide": collide, "grown": grown}[key]()


# ---- rows ------------------------------------------------------------------------------------------------------------------
def rows(t, R, L, seed, pool=None, must=(), words=()):
    """[R][L] ids, each row [bos] body [eos] pad* with the table's live ids.  The body's cells are drawn from `pool` (default: the
    snapshot's continuation ids and its other words' ids, half and half); every id of `must` is then written into a body cell of its
    own, and every (row, col, ids) of `words` is laid over the row from column `col` on, frame or not."""
    r = random.Random(seed)
    if pool is None:
        plain = [i for i in sorted(t.decoder) if i not in t.protected and not t.decoder[i].endswith("@@")]
        cont = [i for i in t.cont if i not in t.protected]
        pool = (cont, plain)

    def pick():
        side = pool[int(r.random() * 2)] if isinstance(pool, tuple) else pool
        return side[int(r.random() * len(side))]
    out, cells = [], []
    for i in range(R):
        n = L - 2 if (i == 0 or L < 3) else int(r.random() * (L - 1))          # body length 0 .. L - 2; row 0 is full
        if L < 3:
            out.append([pick() for _ in range(L)])
            cells += [(i, c) for c in range(L)]
            continue
        out.append([t.bos] + [pick() for _ in range(n)] + [t.eos] + [t.pad] * (L - 2 - n))
        cells += [(i, c) for c in range(1, n + 1)]
    taken = {(i, c + k) for i, c, ids in words for k in range(len(ids))}
    free = [x for x in cells if x not in taken]
    assert len(must) <= len(free), "more ids to place than body cells"
    for v in must:
        i, c = free.pop(int(r.random() * len(free)))
        out[i][c] = v
    for i, c, ids in words:
        assert c + len(ids) <= L
        out[i][c:c + len(ids)] = ids
    return out


def must_ids(t):
    """What every row set of a table holds: ids of the bitmap's last word (a continuation and a plain one where both exist), ids
    that keep no word (holes, ids past the snapshot, a negative one and the largest int32), the ids 0..3 where they are no specials,
    and for a grown table the ids its second file brought."""
    last = t.last_word_ids()
    pick = [i for i in last if i in t.cont and i not in t.protected][-2:] + [i for i in last if i not in t.cont and i not in t.protected][-1:]
    holes = [i for i in range(t.n_ids) if t.absent(i) and i not in t.protected][:4]
    out = pick + holes + [t.n_ids, t.n_ids + 1, t.n_ids + 31, t.n_ids + 32, 2 ** 31 - 1, -7]
    out += [i for i in range(4) if i not in t.protected and i not in out]
    if t.second is not None:
        out += [i for i in range(t.n_ids, t.size + 1) if i not in t.protected]
        out += [i for i in t.snap_ids if i not in t.protected]                  # the old <mask> id: an ordinary token now
    return out


def word_cells(t, n):
    """n ids that make ONE word under the snapshot: n - 1 continuation ids and a plain one"""
    cont = [i for i in t.cont if i not in t.protected]
    plain = [i for i in sorted(t.decoder) if i not in t.protected and i not in t.cont]
    return [cont[k % len(cont)] for k in range(n - 1)] + [plain[0]]


# (R, L) of the row sets: one cell a lane (L % 4 != 0) and four (L % 4 == 0), rows that share a trip and rows of several trips
SHAPES = ((65, 5), (2, 64), (1, 130), (65, 130))
LONG = (3, 400)                                          # a word laid across the trip edges of both kernels


def case_rows(t, R, L, seed):
    """The row set of a table at one shape: `rows` with must_ids, a word over columns 60 .. 67 where the row is long enough, and at
    L = 400 a word over columns 10 .. 309 (the trip edges at 64, 128, 192 and 256) and one over 200 .. 289."""
    words, x = [], word_cells(t, 1)                       # (a plain id in front: the word starts where it is laid)
    if L >= 130:
        words.append((0, 59, x + word_cells(t, 8)))
    if L >= 400:
        words.append((1, 9, x + word_cells(t, 300)))
        words.append((2, 199, x + word_cells(t, 90)))
    return rows(t, R, L, seed, must=must_ids(t), words=words)


# The (table, R, L, p, seed) sets of the GPU file's mask and infill comparisons with whole_word=True.  test_row_tables_inputs.py
# asserts on the oracle alone that each of them chooses and leaves cells, chooses a word of several cells, holds ids of the last
# bitmap word, absent ids, (grown) ids past the snapshot, and that mask_rows replaces a cell by a random id.
SMALL_TABLES = ("moved", "renamed", "collide", "grown") + tuple("edge%d" % n for n in EDGE_NS)
BIG_TABLES = tuple("big%d" % n for n in BIG_NS)
P = 0.45


def cases(key):
    """[(R, L, p, seed)] of one table"""
    shapes = (SHAPES + (LONG,)) if key in SMALL_TABLES else ((65, 64), (65, 130))
    return [(R, L, P, 1000 * k + L + R) for k, (R, L) in enumerate(shapes)]


def big_pool(t):
    """ids 5..64 and the top 64 ids of a big table"""
    return list(range(5, 65)) + list(range(t.n_ids - 64, t.n_ids))


def big_rows(t, R, L, seed):
    return rows(t, R, L, seed, pool=big_pool(t), must=[t.n_ids - 1, t.n_ids - 2, t.n_ids, t.n_ids + 31, -7],
                words=[(0, 59, [t.n_ids, t.n_ids - 1, t.n_ids - 2, t.n_ids - 3, t.n_ids + 31])] if L >= 130 else [])


def rows_of(key, R, L, seed):
    t = table(key)
    return big_rows(t, R, L, seed) if key in BIG_TABLES else case_rows(t, R, L, seed)


# ---- the bitmap-edge rows of edge(n) -----------------------------------------------------------------------------------------
def edge_rows(t, L):
    """Rows for edge(n): ids that are plain in every table, the word (n - 1, n - 2, plain), and the same cells with n_ids in place of
    n - 1, which makes two words.  Returns (rows, one_word (row, first, last), two_words ((row, a, a), (row, a + 1, a + 2)))."""
    n = t.n_ids
    outside = [n, n + 1, n + 31, n + 32, 2 ** 31 - 1, -7]
    x = 6                                                # a plain word of every edge table
    a = [t.bos, x] + outside + [n - 1, n - 2, x, x, t.eos]
    b = [t.bos, x] + outside + [n, n - 2, x, x, t.eos]
    c = [t.bos] + [v for o in outside for v in (n - 1, o)] + [31, 32, 5, x, t.eos]      # a continuation before each of them
    assert max(len(a), len(c)) <= L
    out = [row + [t.pad] * (L - len(row)) for row in (a, b, c)]
    return out, (0, 8, 10), ((1, 8, 8), (1, 9, 10))


# ---- hand-laid rows: which cells are one word, which are not -------------------------------------------------------------------
WORD_SEEDS = tuple(range(12))                            # at p = 0.5 they show every pair of `apart` split (asserted on the CPU)
WORD_TABLES = ("collide", "grown") + tuple("edge%d" % n for n in EDGE_NS) + BIG_TABLES


def pad_rows(t, rows_, L):
    assert all(len(r) <= L for r in rows_)
    return [list(r) + [t.pad] * (L - len(r)) for r in rows_]


def word_rows(key):
    """(rows without their padding, together, apart, row lengths to run them at) of one table: every (row, first, last) of
    `together` is one word, or the tail of one, under the snapshot; the cells (row, a) and (row, b) of every entry of `apart` belong
    to different words."""
    t = table(key)
    n = t.n_ids
    if key.startswith("edge"):
        out, one, two = edge_rows(t, 18)
        out = [r[:r.index(t.eos) + 1] for r in out]
        together = [one, two[1]] + [(2, c - 1, c) for c in range(2, 14, 2)]      # row 2: (n - 1, an id outside the snapshot) six times
        apart = [(0, 7, 8), (0, 10, 11), (1, 8, 9), (1, 7, 8)] + [(2, c, c + 1) for c in range(2, 14, 2)]
        return out, together, apart, (64, 130, 19)
    if key in BIG_TABLES:
        cells = [t.bos, 6, n, n - 1, n - 2, n - 3, n + 31, n - 1, n, n - 1, n + 1, t.eos]
        return [cells], [(0, 3, 6), (0, 7, 8), (0, 9, 10)], [(0, 2, 3), (0, 6, 7), (0, 8, 9)], (64, 13)
    if key == "collide":
        e = t.snap_encoder
        x, won, lost, hole, empty, at = e["p2"], e["p0"], e["p3"], 5, e[""], e["@@"]
        cells = [t.bos, x, won, x, x, lost, x, x, hole, x, x, empty, x, x, at, x, x, 6, x, t.eos]
        # the id a "@@" word won continues, so does the word "@@"; the id a plain word won, a hole, the empty word, the hole a "@@"
        # word left behind do not
        return [cells], [(0, 2, 3), (0, 14, 15)], [(0, 5, 6), (0, 8, 9), (0, 11, 12), (0, 17, 18)], (20, 64, 21)
    if key == "grown":
        e, s = t.encoder, t.snap_encoder
        x, new_at, old, old_mask, old_eos = s["m010"], e["g1@@"], s[GROWN_MOVED_WORD], t.snap_ids[3], t.snap_ids[2]
        cells = [t.bos, x, new_at, x, x, old, x, x, old_mask, x, x, e[GROWN_MOVED_WORD], x, x, old_eos, x, t.mask, x, e["g5@@"], x, t.eos]
        # the moved word's old id and the ids <mask> and </s> held continue (the snapshot's words there end in "@@"); a new "@@"
        # word's id and the moved word's new id do not
        return [cells], [(0, 5, 6), (0, 8, 9), (0, 14, 15)], [(0, 2, 3), (0, 11, 12), (0, 18, 19)], (21, 64)
    raise KeyError(key)


# ---- texts for the tables with merges ----------------------------------------------------------------------------------------
def texts(n, seed, max_words=12):
    r = random.Random(seed)

    def word():
        return "".join(TEXT_LETTERS[int(r.random() * len(TEXT_LETTERS))] for _ in range(1 + int(r.random() * 6)))
    out = [" ".join(word() for _ in range(int(r.random() * (max_words + 1)))) for _ in range(n)]
    out[1], out[2] = "", "abcd abcde ba de z"
    return out


# ---- the 100 k custom tables of the encode tests (corpus.custom_tables: ids above 65 535, a bitmap of about 12.5 KB) -------------
CUSTOM_DOCS, CUSTOM_L, CUSTOM_SEED = 300, 64, 77


def custom():
    def make():
        import corpus
        vocab, merges = corpus.custom_tables()
        return Table("custom", vocab, merges)
    return _once("custom", make)


def custom_texts():
    def make():
        import corpus
        text, offs, _ = corpus.config_corpus(2, n_docs=CUSTOM_DOCS, seed=CUSTOM_SEED)
        raw = text.tobytes()
        return [raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(CUSTOM_DOCS)]
    return _once("custom_texts", make)


def custom_extra_rows():
    """two rows behind the packed ones: they bring the ids no text gives (absent ids, the bitmap's last word)"""
    return case_rows(custom(), 2, CUSTOM_L, 5)


CUSTOM_CASE = (P, 9)                                     # (p, seed) of the mask and infill calls over the packed rows


# ---- what the oracles say of a row set (numpy and the oracle modules are imported here, on use) ---------------------------------
def mask_want(t, ids, p, seed, whole_word=True, random_ids=None, mask_prob=0.8, random_prob=0.1, **kw):
    """mask_oracle.mask with the table's snapshot and live ids, thresholds as Tokenize.mask_rows makes them, and the default
    random_ids = (5, len(encoder)) of the live table"""
    import mask_oracle as MO
    t_sel, t1, t2 = MO.thresholds(p, mask_prob, random_prob)
    lo, hi = random_ids if random_ids is not None else (5, t.size)
    return MO.mask(ids, t.cont, t.pad, t.bos, t.eos, t.mask, seed=seed, t_sel=t_sel, t1=t1, t2=t2, rand_lo=lo, rand_hi=hi,
                   whole_word=whole_word, **kw)


def infill_want(t, ids, p, seed, whole_word=True, dec_len=None, mean_span=3.0, max_span=10, lengths="geometric", **kw):
    import infill_oracle as IO
    t_start, len_t, n_len = IO.rule_ints(p, mean_span, max_span, lengths)
    return IO.infill(ids, t.cont, t.pad, t.bos, t.eos, t.mask, seed=seed, t_start=t_start, len_t=len_t, n_len=n_len, whole_word=whole_word,
                     dec_width=dec_len, **kw)
