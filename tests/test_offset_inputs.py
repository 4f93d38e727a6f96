"""CPU only: the inputs of test_gpu_offsets.py keep their point.  offset_oracle.py builds words of chosen symbol counts, document
boundaries at chosen bytes of the packed text and a corpus of more than 65 536 words; here the oracle alone says that the ladder
reaches every record form and kernel of the miss path, that the boundaries sit where they are meant to, that the corpus crosses
the capacity step of gz_word_token_counts in both texts, and that enough of the reference's own rows are left to compare."""
import numpy as np

import gz_oracle as O
import offset_oracle as X


def _is_ws(ch):
    return ord(ch) in O.WHITESPACE


def test_ladder_words_have_their_symbol_counts_and_reach_every_piece_class():
    t = X.tables()
    words = X.ladder_words()
    assert [n for n, _ in words[:len(X.LADDER)]] == list(X.LADDER) and all(len(w) == n for n, w in words)
    assert all(set(w) <= set(X.ALPHA) for _, w in words[:len(X.LADDER)])
    pieces = {w: len(O.bpe_pieces(w, t.ranks)) for _, w in words}
    got = sorted(pieces.values())
    for lo, hi in ((1, 1), (2, 16), (17, 64), (65, 1024), (1025, 1 << 30)):
        assert any(lo <= p <= hi for p in got), (lo, hi)
    # "barely merge": a word of n >= 16 symbols keeps at least n / 2 pieces, so the symbol classes are piece classes too
    assert all(pieces[w] * 2 >= n for n, w in words[:len(X.LADDER)] if n >= 16)
    # the real words are ONE piece: short and long keys of the whole-word tables, and one past them (merge loop only)
    sizes = [len(w.encode()) for w in X.VOCAB_WORDS]
    assert all(pieces[w] == 1 and w in t.encoder for w in X.VOCAB_WORDS)
    assert min(sizes) <= 4 and 16 in sizes and 17 in sizes and 32 in sizes and max(sizes) == 33


def test_ladder_places_every_word_five_ways():
    b = X.ladder()
    text, offs = b.packed()
    raw = text.tobytes()
    for n, w in X.ladder_words():
        docs = [i for i, d in enumerate(b.docs) if w in d]
        alone = [i for i in docs if b.docs[i] == w]
        assert alone and any(b.docs[i] == "xin " + w + " nam" for i in docs) and any(b.docs[i].startswith(w + "\n") and len(b.docs[i]) > n + 1 for i in docs)
        # last bytes of its document, the next one starts on a non-space byte: the packed text shows no separator
        glued = [i for i in docs if b.docs[i].endswith(w) and b.docs[i] != w and i + 1 < len(b.docs) and b.docs[i + 1] and not _is_ws(b.docs[i + 1][0])]
        assert glued, n
        behind = [i for i in docs if b.docs[i] == " " * (1000 - n % 7) + w]
        assert len(behind) == 1 and int(offs[behind[0]]) % X.TILE == 0, n
    st = X.ladder_straddlers()
    assert len(st) == len(X.ladder_words())
    assert all(a % X.TILE >= 994 for a, _ in st)
    assert all((e - 1) // X.TILE > a // X.TILE for a, e in st if e - a > 30)           # every word of more than 30 bytes crosses a tile edge
    assert max((e - 1) // X.TILE - a // X.TILE for a, e in st) >= 3                     # ... the longest one three of them
    assert raw[st[0][0]:st[0][1]].decode() == X.ladder_words()[0][1]
    counts, first = b.words(0)
    assert counts.max() > 1024 and len(first) == len(b.docs) + 1 and first[-1] == len(counts)


def test_edge_batches_put_the_boundaries_at_the_named_bytes():
    seen = {}
    for b in X.edges():
        delta, variant = b.name[6:-1].split(",")
        text, offs = b.packed()
        raw = text.tobytes()
        inner = set(offs[1:-1].tolist())
        here = [p for p in X.POSITIONS if (p - int(delta)) % X.TILE == 0]
        assert set(here) <= inner, b.name
        for k, p in enumerate(here):
            i = int(np.searchsorted(offs, p, side="left"))                # the document that ends at p ...
            j = int(np.searchsorted(offs, p, side="right"))               # ... and the first one with bytes behind p
            left, right = b.docs[i - 1], b.docs[j - 1]
            assert offs[i] == p and offs[j - 1] == p and left and right
            lw, rw = _is_ws(left[-1]), _is_ws(right[0])
            assert (lw, rw) == {"ends": (False, True), "cut": (False, False), "space": (True, True)}[variant], (b.name, p)
            if variant == "space" and k == 1:
                assert left[-1] == "\n" and not _is_ws(left[-2])             # a glued line feed as the last byte in front of the edge
            seen.setdefault(p, set()).add(variant)
        # runs of empty documents at the block edge and at the very end
        run = X.EMPTY_RUNS[variant]
        lens = np.diff(offs)
        if X.PBLK in here:
            assert int(np.sum((offs[:-1] == X.PBLK) & (lens == 0))) == run, b.name
        assert np.all(lens[-run:] == 0) and lens[-run - 1] > 0, b.name
        # whitespace-only documents, in one-, two- and three-byte spaces: no words
        counts, first = b.words(0)
        nw = np.diff(first)
        ws = [i for i, d in enumerate(b.docs) if d and all(_is_ws(c) for c in d)]
        assert len(ws) == len(X.WS_DOCS) and all(nw[i] == 0 for i in ws)
        assert {len(c.encode()) for i in ws for c in b.docs[i]} == {1, 2, 3}
    assert seen == {p: set(X.VARIANTS) for p in X.POSITIONS}
    assert sorted(X.EMPTY_RUNS.values()) == [1, 2, 65]


def test_corpus_crosses_the_capacity_step_in_both_texts():
    b = X.corpus()
    text, offs = b.packed()
    assert len(b.docs) == 3000 and len(text) > 256 * X.PBLK
    for which in (0, 1):
        counts, first = b.words(which)
        assert len(counts) > 65536 and first[-1] == len(counts)
        assert first[len(b.docs) // 2] > 65536 // 2                         # two sub-batches: words on both sides
        assert counts.min() == 1 and counts.max() > 64
        assert {int(c) for c in counts} >= set(range(1, 15))
    assert int(np.sum(np.diff(b.words(0)[1]) == 0)) > 0                       # documents without words
    assert b.pair_docs[0] == b.docs[X.ROTATE] and b.pair_docs != b.docs
    # pair rule: B's entries are shifted by A's ENTRY count
    off = b.offsets(True)[0]
    na = int(np.diff(b.words(0)[1])[0]) + 2
    assert off[na] == (na, na) and len(off) == na + int(np.diff(b.words(1)[1])[0]) + 2


def test_g3_selection_keeps_at_least_300_usable_rows():
    groups = X.g3_offset_groups()
    rows = [r for rs in groups.values() for r in rs]
    usable = [r for r in rows if "raises" not in r]
    assert len(usable) >= 300 and all("offset" in r["result"] for r in usable)
    assert all(r["raises"] == "ValueError" for r in rows if "raises" in r)
    assert {k[0] for k in groups} == {1, 2}


def test_not_utf8_batch_mixes_bad_and_well_formed_documents():
    docs, good, well = X.not_utf8()
    assert len(good) == len(well.docs) == 3000 and len(docs) > len(good) + 500
    bad = sorted(set(range(len(docs))) - set(good))
    n_bad = 0
    for i in bad:
        try:
            docs[i].decode("utf-8")
        except UnicodeDecodeError:
            n_bad += 1
    assert n_bad > len(bad) // 2
