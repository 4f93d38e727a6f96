"""The synthetic decoder table and the id rows of the batch-decode tests (test_decode_inputs.py on the CPU, test_gpu_decode.py on
the GPU) and of the `g6b` fixture (tests/golden/make_golden.py).  Nothing here imports the library, the oracle or numpy: the vocab
file is text, the loader rule that turns it into ids (tokenize.py:31-51) is restated in `load()` in ten lines, and
test_decode_inputs.py holds that restatement against gz_oracle.Tables.

The table has one word of every kind the decode kernel tells apart (csrc/gz_decode.inc): a word of at most 12 bytes sits in its
16-byte table entry and leaves in up to four stores of 8 / 4 / 2 / 1 bytes, a longer one is copied from the byte arena; a word that
ends in "@@" loses those two bytes when a separator follows; a word with "@@ " inside is always an arena word and is filtered byte
by byte.  Classes (every name is `<class>:<bytes>[:<tag>]`):

  plain   no '@', no space: every length of LENGTHS, and multi-byte UTF-8 at 12 and 13 bytes
  ends    ends in "@@": every length >= 2 of LENGTHS, with "@@" itself, "@@@" and "@@@@"
  inner   holds "@@ ": at the start, in the middle, twice, with a trailing "@@" as well ("x@@ @@"), and "@@@ y", whose leftmost
          occurrence starts at the second '@'; 4 to 20 bytes and one of 300
  space   an inner space without "@@ "
  empty   the empty word (a line " 1")
and the id space has holes: the blank line that ends the file re-assigns the empty word, a duplicated word takes a new id, and
either way the earlier id keeps no word (tokenize.py:51 takes the size before the insert, :40 lets the last word win).

Everything is deterministic; the seeded choices use random.Random(seed).random() alone, which does not change between Python
versions."""
import random

LENGTHS = tuple(range(17)) + (20, 33, 300, 5000)
SPECIALS = ("<pad>", "<s>", "</s>", "<mask>", "<unk>")
TRIP = 64                                                # tokens one wave takes per trip
TRIP_LENGTHS = (0, 1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 257)
PLACED_LENGTHS = (64, 65, 128, 129)
_ALPHA = "abcdefghijklmnopqrstuvwxyz0123456789"


def plain(n, salt=0):
    """n bytes of ASCII without '@' or space; neighbouring bytes differ, so a byte stored one place off shows."""
    return "".join(_ALPHA[(i + 3 * n + 7 * salt + 3) % 36] for i in range(n))


def nbytes(w):
    return len(w.encode("utf-8"))


def _words():
    """[(name, word)] in file order, without the lines that make holes."""
    out = []
    for n in LENGTHS:
        if n:
            out.append(("plain:%d" % n, plain(n)))
    out += [("plain:12:u3", "ệ" * 4), ("plain:12:u4", "\U0001F600" * 3), ("plain:12:u123", "a" + "ô" * 4 + "ệ"),
            ("plain:13:u3", "ệ" * 4 + "a"), ("plain:13:u4", "a" + "\U0001F600" * 3), ("plain:13:u23", "ô" * 5 + "ệ")]
    for n in LENGTHS:
        if n >= 2:
            out.append(("ends:%d" % n, plain(n - 2, 1) + "@@"))
    out += [("ends:3:at", "@@@"), ("ends:4:at", "@@@@")]
    for n in range(4, 21):
        out.append(("inner:%d:start" % n, "@@ " + plain(n - 3, 2)))
        if n >= 5:
            a = (n - 3) // 2
            out.append(("inner:%d:mid" % n, plain(a, 3) + "@@ " + plain(n - 3 - a, 4)))
        if n >= 9:
            a = (n - 6) // 3
            b = (n - 6 - a) // 2
            out.append(("inner:%d:twice" % n, plain(a, 5) + "@@ " + plain(b, 6) + "@@ " + plain(n - 6 - a - b, 7)))
        if n >= 8:
            a = (n - 5) // 2
            out.append(("inner:%d:ends" % n, plain(a, 8) + "@@ " + plain(n - 5 - a, 9) + "@@"))
    out += [("inner:6:xends", "x@@ @@"), ("inner:5:at3", "@@@ y"), ("inner:7:adjacent", "@@ @@ z"),
            ("inner:300", plain(100, 2) + "@@ " + plain(150, 3) + "@@ " + plain(42, 4) + "@@")]
    out += [("space:3", "a b"), ("space:3:at", "@ @"), ("space:4:two", "a  b"), ("space:7:ends", "ab cd@@"), ("space:5:at", "x @@y"),
            ("space:12", "hello wor ld"), ("space:13", "hello worl dz"), ("space:19", "hello world foo bar")]
    return out


def shapes_vocab():
    """The bytes of the synthetic vocab file."""
    lines = []
    for k, (name, w) in enumerate(_words()):
        lines.append("%s %d" % (w, 1 + k % 9))
        if name == "plain:3":
            lines.append(" 1")                          # the empty word
    # holes.  A re-assigned word takes the id the next NEW word will take as well, and that word wins it: `fill0` is gone after
    # `fill1`, its first id keeps no word.  The blank line is the file's last, so the empty word keeps the new id and leaves a hole
    lines += ["fill0 1", "fill0 2", "fill1 1", ""]
    return ("\n".join(lines) + "\n").encode("utf-8")


def second_vocab():
    """A small second vocab file for add_vocab_file: new words, and one word the first file has."""
    return ("new0 1\nnew1@@ 1\n" + plain(7) + " 3\nnew2 long enough for the arena 1\n").encode("utf-8")


# merges that make one piece of the second vocab's word "new0", so that encode() can return its id
BPE = b"#v\nn e\nne w\nnew 0</w>\n"


def load(vocab, specials=SPECIALS, encoder=None):
    """tokenize.py:31-51 for a file without '\\r' and of plain spaces: (encoder, decoder)."""
    enc = {} if encoder is None else dict(encoder)
    if encoder is None:
        for i, s in enumerate(specials):
            enc[s] = i
    for line in vocab.decode("utf-8").split("\n")[:-1]:
        line = line.strip()
        enc[line[:line.rfind(" ")]] = len(enc)
    return enc, {v: k for k, v in enc.items()}


class Shapes:
    """The table by class, and the named row lists."""

    def __init__(self):
        self.vocab = shapes_vocab()
        self.encoder, self.decoder = load(self.vocab)
        self.n_ids = max(self.decoder) + 1
        self.holes = [i for i in range(self.n_ids) if i not in self.decoder]
        self.names = dict(_words())                      # name -> word
        self.names["empty:0"] = ""
        self.id = {name: self.encoder[w] for name, w in self.names.items()}          # name -> id
        self.name_of = {i: name for name, i in self.id.items()}
        assert len(self.id) == len(set(self.id.values())) == len(self.names), "two class words share an id"
        assert all(self.decoder[i] == self.names[name] for name, i in self.id.items()), "a class word lost its id"
        self.small = [name for name, w in self.names.items() if nbytes(w) <= 16]
        self.align = self._align()
        self.trips, self.trip_notes = self._trips()
        self.nothing, self.nothing_batches = self._nothing()
        self.ids, self.ids_wide = self._ids()
        self.unk_rows = self._unk_rows()

    def cls(self, i):
        """The class name of an id, for failure messages."""
        return self.name_of.get(i, "hole" if i in self.holes else "special" if 0 <= i < 5 else "fill" if 0 <= i < self.n_ids else "unknown")

    # every small word behind P_k, k = 1..8: every inline piece size at every output alignment, followed and last
    def _align(self):
        q = self.id["plain:2"]
        rows = []
        for name in self.small:
            for k in range(1, 9):
                p = self.id["plain:%d" % k]
                rows.append([p, self.id[name]])
                rows.append([p, self.id[name], q])
        return rows

    def pool_names(self):
        return [name for name, w in self.names.items() if nbytes(w) <= 33]

    def _trips(self):
        r = random.Random(6464)
        pool = self.pool_names()
        short = [name for name in pool if nbytes(self.names[name]) <= 8]
        I = self.id

        def fill(n, names):
            return [I[names[int(r.random() * len(names))]] for _ in range(n)]
        rows, notes = [], []
        for n in TRIP_LENGTHS:
            rows.append(fill(n, pool)); notes.append("random:%d" % n)
        # the long words, in a handful of rows
        for n, at, name in ((3, 1, "inner:300"), (66, 0, "plain:5000"), (66, 63, "plain:300"), (130, 64, "ends:5000"), (130, 63, "ends:300"),
                            (193, 127, "ends:300"), (193, 128, "plain:5000"), (65, 64, "ends:5000")):
            row = fill(n, pool)
            row[at] = I[name]
            rows.append(row); notes.append("long:%d:%s@%d" % (n, name, at))
        # placed rows: the token at index 63 (and 127) and the one at index 64 (and 128) by kind
        at63 = ("ends:8", "ends:15", "ends:2", "empty:0", "inner:6:xends", "ends:300", "inner:300")
        at64 = ("plain:5", "empty:0", "ends:2")
        for n in PLACED_LENGTHS:
            base = fill(n, short)
            for a in at63:
                for b in (at64 if n > 64 else (None,)):
                    row = list(base)
                    row[63] = I[a]
                    if b is not None:
                        row[64] = I[b]
                    if n >= 128:
                        row[127] = I[a]
                    if n > 128 and b is not None:
                        row[128] = I[b]
                    rows.append(row); notes.append("placed:%d:%s|%s" % (n, a, b))
        # the last token ends in "@@": it is kept
        for n in (1, 2, 64, 65, 128):
            for a in ("ends:8", "ends:15", "ends:2", "inner:6:xends", "ends:300", "ends:4:at"):
                row = fill(n, short)
                row[-1] = I[a]
                rows.append(row); notes.append("last:%d:%s" % (n, a))
        return rows, notes

    def _nothing(self):
        e, at = self.id["empty:0"], self.id["ends:2"]
        rows = [[e], [e] * 64, [e] * 65, [at], [at] * 2, [at] * 64, [at] * 65, [e, at], [at, e], [e] * 63 + [at], [at] * 63 + [e] + [at],
                [e] * 64 + [at], [at] * 64 + [e], [], [e, e]]
        batches = [list(range(len(rows))), [0], [0, 13, 0], [3, 4], [1, 2, 5, 6], [13, 13, 13]]        # indices into rows
        return rows, batches

    ZERO_BATCH = 2                                       # nothing_batches[2]: [empty], [], [empty] -- ids, and 0 bytes of text

    def _ids(self):
        I, n = self.id, self.n_ids
        odd = [-1, -2 ** 31, 2 ** 31 - 1, n, n + 1] + self.holes
        k5, e8, x = I["plain:5"], I["ends:8"], I["inner:6:xends"]
        rows = [[v] for v in odd] + [[k5, v, e8] for v in odd] + [[e8, v] for v in odd] + [[x, v, x] for v in odd]
        rows += [odd, odd * 13, [4], [0, 1, 2, 3, 4], list(range(n)), list(range(n - 1, -1, -1))]
        wide = [[2 ** 40], [-2 ** 40], [k5, 2 ** 40, e8, -2 ** 40], [2 ** 40] * 65, [2 ** 31, -2 ** 31 - 1, 2 ** 63 - 1, -2 ** 63]]
        return rows, wide

    def added_rows(self):
        """Rows for the add_vocab_file sequence: the ids that the words of second_vocab() take (and the two behind them) alone, in a
        row, between old words and across a trip.  The first new word takes id len(encoder), which is n_ids - 1 here: the id the
        moved empty word holds in the decoder, so it decodes to "" before and after; the larger ones decode to unk."""
        enc2, _ = load(second_vocab(), encoder=self.encoder)
        new_ids = list(range(len(self.encoder), len(enc2) + 2))
        I = self.id
        return [[i] for i in new_ids] + [new_ids, [I["plain:5"]] + new_ids + [I["ends:8"]], [I["ends:8"], new_ids[0], I["ends:15"], new_ids[-1]],
                                         [I["plain:7"], I["plain:5"], I["empty:0"]], (new_ids * 65)[:65]]

    def _unk_rows(self):
        """All-unknown rows of 1, 64 and 65 tokens, and rows mixed with known words."""
        I, n = self.id, self.n_ids
        u = n + 7
        k5, e8, e15, x, p13 = I["plain:5"], I["ends:8"], I["ends:15"], I["inner:6:xends"], I["plain:13"]
        return [[u], [u] * 64, [u] * 65, [k5, u], [u, k5], [e8, u, e8, u], [u, e15, u, x, u, p13, u], [u, I["empty:0"], u],
                [self.holes[0], k5, -1, e8, 2 ** 31 - 1], ([k5, u, e8] * 22)[:64] + [u], [u] * 63 + [e8, u]]


def same(text, recorded):
    """A decoded text against the fixture's record of it: the text itself, or {"sha256", "len"} of its UTF-8 bytes for a long one
    (tests/golden/make_golden.py, g6b)."""
    if isinstance(recorded, str):
        return text == recorded
    import hashlib
    raw = text.encode("utf-8", "surrogatepass")
    return len(raw) == recorded["len"] and hashlib.sha256(raw).hexdigest() == recorded["sha256"]


def fixture(rows):
    """The lines of g6b_decode_shapes.jsonl.gz by what they hold: (table, {group: line}, [unk lines], add_vocab_file line)."""
    return (rows[0], {r["group"]: r for r in rows if r["name"] == "default"}, [r for r in rows if r["name"] == "unk"],
            [r for r in rows if r["name"] == "add_vocab_file"][0])


def edges(s, row):
    """The classes of the tokens on both sides of every trip edge of a row, for failure messages."""
    return ["%d:%s|%s" % (c, s.cls(row[c - 1]), s.cls(row[c])) for c in range(TRIP, len(row), TRIP)]


# the unk strings of the tests, in the order one context sees them (inline, arena and inner forms replace each other)
UNKS = ("", "u", plain(12, 11), plain(13, 11), plain(10, 12) + "@@", "@@", "a@@ b", plain(4096, 13))
