"""Host-only: every case of tests/encode_edges.py sits on the edge it is built for.  Positions are taken in the PACKED text (what
the kernels see), tiles are judged by the documented fast-form rule of gz_classify_kernel, splits by the oracle; miss totals, symbol
classes and the rounds of the dense row kernel by counting.  Nothing here computes an expected row, and nothing runs on a GPU."""
import collections

import pytest

import encode_edges as E
import gz_oracle as O

MB = 1 << 20
LIMIT = int(1.1 * MB)            # "about 1 MB" a batch


def split(doc: bytes):
    return O.split_words(doc.decode("utf-8"))


def plain_bytes(cp, k):
    """(front, behind): do the character's bytes in front of / behind the edge leave a tile plain -- stated by the character's class,
    not by the tile rule: the space always; a control character never; of a multi-byte character the lead byte never, except E1, and
    its continuation bytes always, except 9A."""
    e = chr(cp).encode("utf-8")
    def part(b):
        if not b or cp == 0x20:
            return True
        if len(e) == 1:
            return False
        lead_ok = b[0] != e[0] or e[0] == 0xE1
        return lead_ok and 0x9A not in b
    return part(e[:k]), part(e[k:])


# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_fast_form_rule_has_exactly_one_hole_and_the_fix_closes_it():
    """Of all 29 whitespace code points at all byte splits over a tile edge, only U+1680 cut 1|2 leaves the tile that holds its lead
    byte plain; the rule with the E1|9A test (fast_tile) does not."""
    holes = []
    for cp in E.WS:
        e = chr(cp).encode("utf-8")
        for k in range(1, len(e)):
            text = b"x" * (E.TILE - k) + e + b"y" * (E.TILE - (len(e) - k))
            assert len(text) == 2 * E.TILE
            if E.plain_tile(text[:E.TILE]):
                holes.append((cp, k))
                assert not E.fast_tile(text, 0)
            assert E.plain_tile(text[:E.TILE]) == plain_bytes(cp, k)[0]
    assert holes == [(0x1680, 1)]
    assert len(E.WS) == 29 and sum(len(chr(c).encode("utf-8")) + 1 for c in E.WS) == 10 * 2 + 2 * 3 + 17 * 4


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("variant", E.VARIANTS)
def test_family_a_items_sit_on_their_edges(variant, shifted):
    b = E.family_a(variant, shifted)
    assert b.nbytes <= LIMIT and b.takes_one_launch()
    raw, off = b.raw, b.off
    first = 1 if shifted else 0
    assert all(len(d) == E.DOC for d in b.docs[first:])
    seen = collections.Counter()
    holes = 0
    for m in b.marks:
        d, edge, item, k, cp = m["doc"], m["edge"], m["item"], m["k"], m["cp"]
        g = int(off[d]) + edge                                   # the edge in the packed text
        assert raw[g - k:g - k + len(item)] == item, m["name"]
        if edge == 528:
            assert g % E.LANE == 0 and g % E.TILE != 0
        else:
            assert g % E.TILE == 0
            assert (g % E.BLOCK == 0) == (shifted and edge == 2048)      # local 2 048 is a block edge behind the leading document only
        assert int(off[d]) % E.BLOCK == (E.LEAD if shifted else 0)
        seen[(m["name"], edge)] += 1
        # the tiles in front of and behind the edge: plain or not, by the item's class and the variant's neighbours
        tf, tb = (g - 1) // E.TILE, g // E.TILE
        if cp is not None:
            pf, pb = plain_bytes(cp, k)
            if edge == 528:
                pf = pb = pf and pb
                want_f = want_b = pf and variant == "plain"
            else:
                want_f = pf and variant in ("plain", "after")
                want_b = pb and variant in ("plain", "before")
            assert E.plain_tile(raw[tf * E.TILE:(tf + 1) * E.TILE]) == want_f, (m["name"], edge, variant)
            assert E.plain_tile(raw[tb * E.TILE:(tb + 1) * E.TILE]) == want_b, (m["name"], edge, variant)
            if cp == 0x1680 and k == 1 and edge != 528 and variant in ("plain", "after"):
                holes += 1
                assert E.plain_tile(raw[tf * E.TILE:(tf + 1) * E.TILE]) and not E.fast_tile(raw, tf)
            # the oracle splits the document at the character: one word more than with a letter in its place
            doc = b.docs[d]
            at = edge - k
            assert len(split(doc)) == len(split(doc[:at] + b"x" * len(item) + doc[at + len(item):])) + 1, (m["name"], edge)
        else:
            assert not E.plain_tile(raw[tb * E.TILE:(tb + 1) * E.TILE])        # the line feed's tile
    # the hole, where a plain tile stands in front: at local 1 024, 2 048 and 3 072 (behind the leading document the middle one is a block edge)
    assert holes == (3 if variant in ("plain", "after") else 0)
    assert len(seen) == len(E.ws_items()) * 4 and set(seen.values()) == {1}
    # the glue rule, by the oracle: the word that ends on the tile's last byte takes "\n" along, and only then
    for m in b.marks:
        if m["cp"] is None:
            doc, at = b.docs[m["doc"]], m["edge"] - m["k"]
            words = split(doc[:at + len(m["item"])])
            glued = m["item"][:1] == b"\n"
            assert words[-1].endswith("qz\n") == glued and (glued or words[-1].endswith("qz")), m["name"]


def test_family_a_document_starts_and_empty_documents():
    for b in E.family_a_boundaries():
        assert b.nbytes <= LIMIT and b.takes_one_launch()
        kinds = collections.Counter()
        for m in b.marks:
            p = m["pos"]
            if m.get("newline"):                                 # a line feed opens the next document: not glued across the document start
                assert b.raw[p - 1:p].isalpha() and b.raw[p:p + 2] == b"\nq" and p in b.off
            else:
                assert b.raw[p - 1:p + 1].isalpha()               # letters on both sides: only the start bit separates the words
            assert list(b.off).count(p) == m["empties"] + 1      # that many empty documents stand at the edge
            kinds["block" if p % E.BLOCK == 0 else "tile" if p % E.TILE == 0 else "lane" if p % E.LANE == 0 else "inside"] += 1
        assert kinds["block"] >= 3 and kinds["tile"] >= 3 and kinds["lane"] >= 1 and kinds["inside"] >= 1
        # the oracle: every document's first word starts at its first byte
        assert all(not d or split(d)[0][0] == chr(d.lstrip(b"\n")[0]) for d in b.docs)


def test_family_a_end_of_the_text():
    got = set()
    for b in E.family_a_text_end():
        B, kind = b.info["size"], b.info["end"]
        assert b.nbytes == B and b.takes_one_launch() and b.raw.endswith(b.info["tail"])
        got.add((B % 16, B % E.TILE, B % E.BLOCK, kind))
        words = split(b.docs[-1])
        assert len(b.docs[-1]) >= len(b.info["tail"])
        if kind == "word":
            assert words[-1].endswith("qzqz")
        elif kind == "glued":
            assert words[-1].endswith("qzq\n") and b.raw[B - 1:B] == b"\n"
        else:
            assert words[-1].endswith("qz") and ord(b.raw.decode("utf-8")[-1]) in O.WHITESPACE and b.raw[-1] >= 0x80
    for kind in E.END_KINDS:
        assert {m for (m, _, _, k) in got if k == kind} >= {0, 1, 15}
        assert {(t, blk) for (_, t, blk, k) in got if k == kind} >= {(0, 0), (1, 1), (0, 1024), (1, 1025)}
    assert {B % 16 for B in E.END_SIZES} == {0, 1, 15} and {B % 32 for B in E.END_SIZES} >= {0, 1, 15, 16, 17}


def test_family_a_u1680_in_the_last_blocks():
    paths = collections.Counter()
    for b in E.family_a_tail_blocks():
        B, e = b.info["size"], b.info["edge"]
        assert b.nbytes == B and b.takes_one_launch() and e % E.TILE == 0 and e + 2 <= B
        assert b.raw[e - 1:e + 2] == b"\xe1\x9a\x80" and b.raw[e - 3:e - 1].isalpha()
        k = e // E.TILE - 1                                           # the tile in front: plain, and not fast
        assert E.plain_tile(b.raw[k * E.TILE:e]) and not E.fast_tile(b.raw, k)
        inner = E.inner_block(k * E.TILE // E.BLOCK * E.BLOCK, B)
        paths[(inner, "last tile of its block" if e % E.BLOCK == 0 else "inside its block", "ends the text" if e + 2 == B else "")] += 1
        text = b.raw.decode("utf-8")
        at = len(b.raw[:e - 1].decode("utf-8"))
        assert text[at] == "\u1680" and sum(len(d) for d in b.docs[:1]) == 100
        assert len(O.split_words(text)) == len(O.split_words(text[:at] + "x" + text[at + 1:])) + (1 if e + 2 < B else 0)
        assert all(d.decode("utf-8") is not None for d in b.docs)   # no document boundary inside the character
    assert paths[(True, "last tile of its block", "")] >= 2 and paths[(True, "inside its block", "")] >= 2
    assert paths[(False, "last tile of its block", "")] >= 2 and paths[(False, "inside its block", "")] >= 2
    assert paths[(False, "last tile of its block", "ends the text")] >= 1 and paths[(False, "inside its block", "ends the text")] >= 1
    # the bound of the inner path itself: 16 bytes behind the block, and one fewer
    assert E.inner_block(0, 4096 + 16) and not E.inner_block(0, 4096 + 15) and (4096 + 15, (4096,)) in E.TAIL_CASES and (4096 + 16, (4096,)) in E.TAIL_CASES


# ---------------------------------------------------------------------------------------------------------------------------------
def test_family_b_word_lengths_and_starts():
    """The bundled vocabulary has whole words of 1, 12, 13, 16, 17, 32 and 33 bytes and none of 48, 49 or 80."""
    assert [nb for nb in E.WORD_BYTES if E.hit_word(nb) is None] == [48, 49, 80]
    known = set(E.vocab())
    for kind in ("hit", "invented"):
        b = E.family_b_words(kind)
        assert b.nbytes <= LIMIT and b.takes_one_launch()
        seen = set()
        for m in b.marks:
            w, nb, s = m["word"], m["nbytes"], m["s"]
            assert (w in known) == (kind == "hit") and len(w.encode("utf-8")) == nb
            g = int(b.off[m["doc"]]) + m["at"]                     # the word's first byte in the packed text
            assert b.raw[g:g + nb] == w.encode("utf-8") and b.raw[g - 1:g] == b" " and b.raw[g + nb:g + nb + 1] == b" "
            edge = g + s
            assert edge % E.TILE == 0 and (edge % E.BLOCK == 0) == (m["edge"] == 2048)
            assert 0 <= s <= E.LOOKAHEAD and (nb == 1 or (1 <= s < nb))    # starts in the last 1..48 bytes of a tile, ends in the next
            assert w in split(b.docs[m["doc"]])
            seen.add((nb, s, m["edge"]))
        lengths = [nb for nb in E.WORD_BYTES if kind == "invented" or nb <= 33]
        assert seen == {(nb, s, e) for nb in lengths for s in E.straddles(nb) for e in (1024, 2048, 3072)}
    assert E.straddles(80) == tuple(range(1, 49)) and E.straddles(13) == tuple(range(1, 13))
    n = 0
    for b in E.family_b_text_end():
        w, at = b.info["word"].encode("utf-8"), b.info["at"]
        assert b.raw[at:] == w and b.raw[at - 1:at] == b" " and (at + b.info["s"]) % E.TILE == 0 and b.takes_one_launch()
        assert split(b.docs[-1])[-1] == b.info["word"]
        n += 1
    assert n == 2 * (7 + 10)


def test_family_b_word_starts_per_tile():
    b = E.family_b_tiles()
    assert all(len(d) == E.DOC for d in b.docs) and b.takes_one_launch()
    def starts(tile, before):
        prev = before + tile[:-1]
        return [i for i in range(len(tile)) if tile[i] != 0x20 and prev[i] == 0x20]
    counts = set()
    for m in b.marks:
        g = int(b.off[m["doc"]])
        assert g % E.BLOCK == 0
        for t in range(4):
            tile = b.raw[g + t * E.TILE:g + (t + 1) * E.TILE]
            st = starts(tile, b.raw[g + t * E.TILE - 1:g + t * E.TILE] if t else b" ")      # (a document start is a word start)
            if m["starts"] is not None:
                assert len(st) == m["starts"][t]
                counts.add(len(st))
                if len(st) == 512:
                    assert max(sum(1 for i in st if i // E.LANE == lane) for lane in range(64)) == 8     # more than the unrolled four
            elif t in m["single"]:
                assert st == [E.TILE - 1]                             # one word start, in the tile's last byte
        assert len(split(b.docs[m["doc"]])) > 0
    assert counts == set(E.TILE_WORDS)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", E.MISS_FORMS)
def test_family_c_miss_totals_and_classes(form):
    for total in E.MISS_TOTALS:
        b = E.family_c(total, form)
        assert b.nbytes <= LIMIT and b.takes_one_launch()
        words = [w for d in b.docs for w in split(d)]
        assert len(words) == total                                    # with the tables off every word is a miss
        hist = collections.Counter(len(w) for w in words)             # symbols = code points
        if form == "spread":
            assert all(abs(hist[c] - total / 16) <= 5 for c in range(1, 17))       # (four words at most were made longer)
            assert (hist[17] >= 1 and hist[64] == 1 and hist[65] == 1) == (total >= 64)
        else:
            assert hist == ({form: total} if total else {})
    assert {t % E.MISS_GROUP for t in E.MISS_TOTALS} >= {0, 1, 63} and {t - E.MPRE_TILE for t in E.MISS_TOTALS} >= {-1, 0, 1}
    assert 2 * E.MPRE_TILE + 1 in E.MISS_TOTALS


def test_family_c_blocks_without_a_miss():
    known = set(E.vocab())
    for on in (False, True):
        b = E.family_c_blocks(on)
        assert all(len(d) == E.DOC for d in b.docs) and b.nbytes <= LIMIT and b.takes_one_launch()
        for d, n in zip(b.docs, b.info["misses"]):
            words = split(d)
            if n:
                assert len(words) == n and (n == 2048 or not on or not (set(words) & known))
            elif on:
                assert words and set(words) == {b.info["hit"]} and O.bpe_pieces(words[0], E.tables().ranks) == words[:1]
            else:
                assert not words and d == b" " * E.DOC
        runs = "".join("F" if n else "E" for n in b.info["misses"])
        assert "FEF" in runs and "FEEEF" in runs and "FEEEEEEEEEF" in runs and "FF" in runs
        if not on:
            assert 2048 in b.info["misses"] and E.BLOCK // 2 == 2048     # a word and a space every two bytes: no block holds more


# ---------------------------------------------------------------------------------------------------------------------------------
def plan(b, max_len):
    toks = b.info.get("tokens") or [[1] * w for w in b.info["words"]]
    words = b.info.get("words") or [len(t) for t in toks]
    for d, doc in zip(range(len(b.docs)), b.docs):
        ws = split(doc)
        assert len(ws) == words[d]
        if "tokens" in b.info:
            assert [len(O.bpe_pieces(w, E.tables().ranks)) for w in ws] == toks[d]
    return E.rounds(words, toks, max_len, b.info.get("merged"))


def test_family_d_classes_and_shapes():
    assert [E.rows_class(m) for m in (4, 256, 260, 512, 516, 1024)] == [(512, 8), (512, 8), (1024, 4), (1024, 4), (1024, 1), (1024, 1)]
    assert {m for m, _ in E.D_SHAPES} == {4, 8, 12, 16, 252, 256, 260, 512, 516, 1024}
    assert {n for _, n in E.D_SHAPES} == {1, 7, 8, 9, 31, 32, 33, 65}
    for max_len, n in E.D_SHAPES:
        b = E.family_d_shapes(max_len, n)
        assert b.nbytes <= LIMIT and len(b.docs) == n
        r = plan(b, max_len)
        cap, dpw = E.rows_class(max_len)
        assert sum(x["docs"] for x in r) == n and all(x["words"] <= cap and x["entries"] <= cap and x["docs"] >= 1 for x in r)
        assert len({x["wave"] for x in r}) == (n + dpw - 1) // dpw
        if n >= 12:
            assert {max_len - 2, max_len - 1, max_len, 5 * max_len} <= set(b.info["words"])


def test_family_d_rounds_at_cap():
    for max_len in (256, 512):
        cap, dpw = E.rows_class(max_len)
        for delta in (-1, 0, 1):
            b = E.family_d_cap(max_len, delta)
            assert len(b.docs) == dpw and sum(min(w, max_len - 1) for w in b.info["words"]) == cap + delta
            r = plan(b, max_len)
            # CAP - 1 and CAP words: all documents enter the round and the last rolls back on its row; CAP + 1: it never enters
            assert [(x["docs"], x["rolled_back"]) for x in r] == [(dpw - 1, delta <= 0), (1, False)]
            b = E.family_d_cap_rows(max_len, delta)
            r = plan(b, max_len)
            assert r[0]["entries"] == (cap + delta if delta <= 0 else cap - 2)
            assert [(x["docs"], x["rolled_back"]) for x in r] == ([(3, False)] if delta <= 0 else [(2, True), (1, False)])
    r = plan(E.family_d_rollback(), 256)
    assert (r[0]["docs"], r[0]["words"], r[0]["entries"], r[0]["rolled_back"]) == (2, 510, 510, True) and len(r) == 2


def test_family_d_merged_words_and_cuts():
    for n in (95, 96, 97, 200):
        b = E.family_d_merged(n)
        r = plan(b, 256)
        assert len(r) == 1 and r[0]["merged"] == n and r[0]["overflow"] == (n > E.MLCAP) and r[0]["docs"] == 8
        assert E.pieces_of(b.info["two"]) == 2 and E.pieces_of(b.info["far"]) > 16        # near and far records side by side
        assert not ({b.info["two"], b.info["far"]} & set(E.vocab()))
    for max_len in (4, 16, 256, 260, 1024):
        for wide in (False, True):
            b = E.family_d_straddle(max_len, wide)
            n = E.pieces_of(b.info["word"])
            assert n == 5 if not wide else n > 64 and n > 250
            plan(b, max_len)
            for toks, fit in zip(b.info["tokens"], (2, 1, 0, 5)):
                at = toks.index(n)                               # position of the word's first piece: bos + the hits in front of it
                assert max_len - 1 - (1 + at) == (fit if max_len - 2 - fit >= 0 else max_len - 2)
    b = E.family_d_empty()
    r = plan(b, 8)
    assert [x["entries"] for x in r[:8]] == [16] * 8 and all(x["words"] == 0 for x in r[:8])      # rounds of empty documents only
