"""Inputs and expected values of the `return_offset` tests (test_offset_inputs.py on the CPU, test_gpu_offsets.py on the GPU).

What `return_offset=True` reports rests on two things the device leaves behind after a call made with GZ_KEEP_WORDS: the number of
pieces of every word and the index of every document's first word.  Both are integers, and the Python oracle (oracle/gz_oracle.py,
itself pinned to the reference by test_oracle_golden.py) gives both: `O.encode_words(text, t)[1]` is the piece count of every word
of one document, `O.call(..., return_offset=True)["offset"]` the list the reference returns, pair rule included.  Neither depends
on max_len, padding or truncation, so one oracle pass per batch serves every layout; the batches are built once per process.

Three batches:
  ladder()   words of chosen symbol counts -- the edges of the merge kernel's 8 / 16-symbol instances, of W_LONG (> 16), W_HUGE (> 64),
             PLONG (256) and of the arena pass (> 1024) -- and real vocabulary words, each placed five ways;
  edges()    nine small batches with document boundaries at chosen bytes of the PACKED text: the tile (1 KiB) and scan-block (4 KiB)
             edges and their neighbours, a word ending there / cut there / whitespace there, runs of empty documents, documents of
             nothing but two- and three-byte spaces;
  corpus()   3 000 noisy cfg-3 documents: more than one 65 536-word capacity step of gz_word_token_counts.
"""
import contextlib
import functools
import os
import random

import numpy as np

import corpus as corpus_mod
import gz_oracle as O
from conftest import DATA, read_jsonl

TILE, PBLK = 1024, 4096                     # bytes per tile of the word kernels, per block of the scans (gz_docw0_kernel)
ALPHA = "nghiêngtrườngkhôngaaaabđ_.😀"      # the alphabet of test_long_and_huge_words: words drawn from it barely merge
LADDER = (1, 2, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)
# whole words of the bundled vocabulary that bpe() turns into ONE piece: by byte length on both sides of the whole-word tables'
# key sizes (<= 16 bytes, 17 .. 32 bytes); the 33-byte word is in no table and becomes one piece only through the merge loop
VOCAB_WORDS = ("xin", "việt", "đột_nhiên", "lệnh_hồ_xung", "báo_điện_tử", "đảng_cộng_sản_việt_nam", "nghiêng_nước_nghiêng_thành",
               "đường_đường_chính_chính")
POSITIONS = (1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)
VARIANTS = ("ends", "cut", "space")
EMPTY_RUNS = {"ends": 1, "cut": 2, "space": 65}
WS_DOCS = ("\u00a0", "\u0085\u2003\u00a0", "\u3000\u2028\n", " ", "\u2000\u200a\u205f\u1680\u202f\u2029")      # is_ws2 / is_ws3 of gz_pipeline.inc
ROTATE = 7                                  # text B of the pair form: text A rotated by this many documents
LAYOUTS = ((48, True, True), (None, True, True), (16, False, True), (1, True, True))
_SYLLABLES = ("xin", "chào", "việt", "nam", "không", "được", "người", "a", "và", "sinh_viên", "công_nghệ", "hà_nội", "ng", "x.y", "1975")


@functools.lru_cache(maxsize=None)
def tables():
    return O.Tables(open(os.path.join(DATA, "vocab.txt"), "rb").read(), open(os.path.join(DATA, "bpe.codes"), "rb").read())


@contextlib.contextmanager
def _bpe_once():
    """O.bpe_pieces with a memory for the length of the block: the same word costs one merge loop however many documents hold it."""
    plain, seen = O.bpe_pieces, {}

    def cached(word, ranks):
        got = seen.get(word)
        if got is None:
            got = seen[word] = plain(word, ranks)
        return got
    O.bpe_pieces = cached
    try:
        yield
    finally:
        O.bpe_pieces = plain


def pack(docs):
    """Documents (str or bytes) -> (uint8 text, int64 offsets[N + 1]) as the C ABI takes them."""
    raw = [d if isinstance(d, bytes) else d.encode("utf-8") for d in docs]
    offs = np.zeros(len(raw) + 1, dtype=np.int64)
    if raw:
        np.cumsum([len(b) for b in raw], out=offs[1:])
    return np.frombuffer(b"".join(raw), dtype=np.uint8), offs


def rotate(docs, k=ROTATE):
    k %= max(len(docs), 1)
    return list(docs[k:]) + list(docs[:k])


class Batch:
    """One list of documents with what the oracle says about it (computed on first use, then kept)."""

    def __init__(self, name, docs):
        self.name, self.docs, self.pair_docs = name, list(docs), rotate(docs)
        self._words, self._offsets = {}, {}

    def packed(self, which=0):
        return pack(self.pair_docs if which else self.docs)

    def words(self, which=0):
        """(counts int32 [words of all documents], doc_first int64 [N + 1]) of text A (0) or B (1)."""
        if which not in self._words:
            with _bpe_once():
                per = [O.encode_words(d, tables())[1] for d in (self.pair_docs if which else self.docs)]
            first = np.zeros(len(per) + 1, dtype=np.int64)
            if per:
                np.cumsum([len(p) for p in per], out=first[1:])
            self._words[which] = (np.array([c for p in per for c in p], dtype=np.int32), first)
        return self._words[which]

    def offsets(self, pair):
        """The reference's 'offset' list of every document: O.call(..., return_offset=True)["offset"]."""
        if pair not in self._offsets:
            with _bpe_once():
                self._offsets[pair] = [O.call(tables(), a, b if pair else None, return_offset=True)["offset"]
                                       for a, b in zip(self.docs, self.pair_docs)]
        return self._offsets[pair]


def _fill(n, r, lead="", tail=""):
    """Exactly n bytes of short words with single spaces between them, behind `lead` and in front of `tail`."""
    budget = n - len(lead.encode()) - len(tail.encode())
    assert budget >= 1, n
    parts, used = [], 0
    while True:
        w = r.choice(_SYLLABLES)
        b = len(w.encode())
        if used + b + 1 >= budget:
            break
        parts.append(w); used += b + 1
    out = lead + " ".join(parts + ["a" * (budget - used)]) + tail
    assert len(out.encode()) == n
    return out


def ladder_words():
    r = random.Random(9)
    return [(n, "".join(r.choice(ALPHA) for _ in range(n))) for n in LADDER] + [(len(w), w) for w in VOCAB_WORDS]


@functools.lru_cache(maxsize=None)
def ladder():
    """Every word alone in its document; between two short words; followed by a glued line feed and another word; as the last
    bytes of its document with the next one starting on a non-space byte (the packed text shows no separator); and behind
    1000 - n % 7 spaces in a document that starts on a tile edge of the packed text, so that the word straddles the next edge."""
    r = random.Random(19)
    docs, at = [], 0

    def add(d):
        nonlocal at
        docs.append(d); at += len(d.encode())
    for n, w in ladder_words():
        add(w)
        add("xin " + w + " nam")
        add(w + "\nhết")
        add("chào " + w)
        add("việt nam")
        if at % TILE:
            add(_fill(TILE - at % TILE, r))
        add(" " * (1000 - n % 7) + w)
    return Batch("ladder", docs)


def ladder_straddlers():
    """(packed start, packed end) of the words placed behind spaces, for the inputs test."""
    b = ladder()
    offs = pack(b.docs)[1]
    out = []
    for i, d in enumerate(b.docs):
        if d.startswith(" " * 900):
            out.append((int(offs[i]) + len(d) - len(d.lstrip(" ")), int(offs[i + 1])))
    return out


def _edge_docs(delta, variant):
    r = random.Random(100 * (delta + 2) + VARIANTS.index(variant))
    lead = "" if variant == "cut" else " "
    docs, at, here = [], 0, ""
    for k, p in enumerate(q for q in POSITIONS if (q - delta) % TILE == 0):
        tail = "" if variant != "space" else "\n" if k == 1 else " "
        docs.append(_fill(p - at, r, here, tail)); at = p
        if p == PBLK:
            docs += [""] * EMPTY_RUNS[variant]
        here = lead
    docs.append(_fill(150, r, here))
    docs += list(WS_DOCS) + ["hết"] + [""] * EMPTY_RUNS[variant]
    return docs


@functools.lru_cache(maxsize=None)
def edges():
    """Nine batches: the positions that are a tile edge - 1, a tile edge, a tile edge + 1, each with a word ending at the boundary
    (the next document starts with a space), a word cut by it (non-space bytes on both sides) and whitespace on both sides (once
    a glued line feed); 1, 2 and 65 empty documents at 4 096 and at the very end; whitespace-only documents."""
    return tuple(Batch("edges[%+d,%s]" % (d, v), _edge_docs(d, v)) for d in (-1, 0, 1) for v in VARIANTS)


@functools.lru_cache(maxsize=None)
def corpus():
    text, offs, _ = corpus_mod.config_corpus(3, n_docs=3000, seed=5)
    text, offs = corpus_mod.add_noise(text, offs, seed=5, rate=0.05)
    raw = text.tobytes()
    return Batch("corpus", [raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(len(offs) - 1)])


def batches():
    return (ladder(),) + edges() + (corpus(),)


@functools.lru_cache(maxsize=None)
def g3_offset_groups():
    """The reference's own rows with return_offset (g3_random.jsonl.gz), grouped by their keyword arguments as
    test_g3_random_batched groups the others: {(n_args, max_len, padding, truncation): rows}."""
    groups = {}
    for r in read_jsonl("g3_random.jsonl.gz"):
        kw = r["kwargs"]
        if kw.get("return_offset"):
            groups.setdefault((len(r["args"]), kw.get("max_len"), kw.get("padding", True), kw.get("truncation", True)), []).append(r)
    return groups


@functools.lru_cache(maxsize=None)
def not_utf8():
    """The documents of test_bytes_that_are_not_utf8_stay_inside_their_document: runs of stray continuation bytes, truncated and
    over-long sequences between well-formed documents.  -> (docs as bytes, indices of the well-formed ones, those as a Batch)."""
    text, offs, _ = corpus_mod.config_corpus(3, n_docs=3000, seed=91)
    raw = text.tobytes()
    r = random.Random(17)

    def junk():
        n = r.choice([1, 2, 3, 5, 8, 13, 16, 17, 31, 40, 70, 200])
        pool = [b"\x80", b"\xbf", b"\x9a", b"a", b"\xe1", b"\xe1\xba", b"\xf0\x9f", b"\xc3", b"\xc2\xa0", b" ", b"\n", b"ng", b"\xe1\xbb\x87", b"\xff", b"\xc0\x80"]
        return b"".join(r.choice(pool) for _ in range(n))
    docs, good = [], []
    for i in range(len(offs) - 1):
        if r.random() < 0.3:
            docs.append(junk())
        good.append(len(docs))
        docs.append(raw[offs[i]:offs[i + 1]])
    docs.append(junk())
    return docs, good, Batch("well-formed", [docs[g].decode("utf-8") for g in good])
