"""CPU only: the inputs of test_gpu_decode.py keep their point.  decode_tables.Shapes is meant to hold one word of every kind the
decode kernel tells apart and to put those words at every output alignment and on both sides of the 64-token trips of a wave; the
fixture g6b_decode_shapes.jsonl.gz holds what the reference decodes from them.  Here the table is read back through
gz_oracle.Tables, the row lists are counted, the fixture is held against the builder (it cannot go stale) and the oracle against
the fixture (so the GPU is compared with an oracle that is pinned to the reference on these very rows)."""
import base64

import pytest

import decode_tables as T
import gz_oracle as O
from conftest import read_jsonl


@pytest.fixture(scope="module")
def s():
    return T.Shapes()


@pytest.fixture(scope="module")
def tables(s):
    return O.Tables(s.vocab, b"")


@pytest.fixture(scope="module")
def fx():
    return T.fixture(read_jsonl("g6b_decode_shapes.jsonl.gz"))


def _by_class(tables):
    dec = {i: w for i, w in tables.decoder.items() if i >= 5 and not w.startswith("fill")}
    inner = {w for w in dec.values() if "@@ " in w}
    space = {w for w in dec.values() if " " in w and w not in inner}
    ends = {w for w in dec.values() if w.endswith("@@") and w not in inner and w not in space}
    plain = {w for w in dec.values() if w and w not in inner | space | ends}
    return dec, plain, ends, inner, space


def test_the_builder_restates_the_loader(s, tables):
    assert (s.encoder, s.decoder) == (tables.encoder, tables.decoder)
    assert s.n_ids == max(tables.decoder) + 1 and all(s.decoder[i] == s.names[n] for n, i in s.id.items())


def test_the_table_holds_every_class(s, tables):
    dec, plain, ends, inner, space = _by_class(tables)
    L = lambda ws: sorted(set(T.nbytes(w) for w in ws))                          # noqa: E731
    assert L(plain) == [n for n in T.LENGTHS if n] and all("@" not in w for w in plain)
    for n in (12, 13):                                                          # multi-byte characters across the inline limit
        multi = [w for w in plain if T.nbytes(w) == n and len(w) < n]
        assert {max(len(c.encode()) for c in w) for w in multi} >= {3, 4} and any(len(w[0].encode()) == 1 for w in multi), n
        assert any(len(w[-1].encode()) > 1 for w in multi) and any(len(w[0].encode()) > 1 for w in multi), n
    assert L(ends) == [n for n in T.LENGTHS if n >= 2] and {"@@", "@@@", "@@@@"} <= ends
    assert set(range(4, 21)) | {300} == set(L(inner))
    assert all(any(w.startswith("@@ ") and T.nbytes(w) == n for w in inner) for n in range(4, 21))
    assert all(any(w.find("@@ ") > 0 and T.nbytes(w) == n for w in inner) for n in range(5, 21))
    assert all(any(w.count("@@ ") == 2 and T.nbytes(w) == n for w in inner) for n in range(9, 21))
    assert {"x@@ @@", "@@@ y"} <= inner and "@@@ y".find("@@ ") == 1
    assert any(w.endswith("@@") for w in inner) and any(T.nbytes(w) <= 12 for w in inner)
    assert {"a b", "@ @"} <= space and any(T.nbytes(w) > 12 for w in space) and any(w.endswith("@@") for w in space)
    assert "" in dec.values() and s.id["empty:0"] == tables.encoder[""]
    assert len(s.holes) >= 2 and all(h not in tables.decoder and 5 <= h < s.n_ids for h in s.holes)
    assert tables.decoder[s.n_ids - 1] == ""                                    # the blank line moved the empty word: its first id is a hole
    assert "fill0" in tables.encoder and "fill0" not in tables.decoder.values()  # the duplicated word: its first id is a hole
    assert [tables.decoder[i] for i in range(5)] == list(O.DEFAULT_SPECIALS)


def test_align_puts_every_piece_at_every_alignment(s, tables):
    seen = set()
    for row in s.align:
        assert len(row) in (2, 3) and s.decoder[row[0]] == T.plain(T.nbytes(s.decoder[row[0]]))
        k, w = T.nbytes(s.decoder[row[0]]), s.decoder[row[1]]
        seen.add((s.name_of[row[1]], k, len(row) == 3))
        if "@@ " not in w and T.nbytes(w) <= 12:
            seen.add(("inline", T.nbytes(w), w.endswith("@@"), len(row) == 3, k))
    for name, w in s.names.items():
        if T.nbytes(w) <= 16:
            assert all((name, k, f) in seen for k in range(1, 9) for f in (False, True)), name
    want = [("inline", n, e, f, k) for n in range(13) for e in (False, True) if n >= 2 or not e for f in (False, True) for k in range(1, 9)]
    assert all(x in seen for x in want), [x for x in want if x not in seen][:5]
    # the piece sizes that reach the stores: 0 .. 13 bytes with the separator
    sizes = {T.nbytes(s.decoder[r[1]]) + 1 for r in s.align if len(r) == 3 and "@" not in s.decoder[r[1]] and T.nbytes(s.decoder[r[1]]) <= 12}
    sizes |= {T.nbytes(s.decoder[r[1]]) - 2 for r in s.align if len(r) == 3 and s.decoder[r[1]].endswith("@@") and " " not in s.decoder[r[1]]}
    assert sizes >= set(range(14)), sizes


def test_trips_have_their_lengths_and_placed_tokens(s):
    lens = [len(r) for r in s.trips]
    assert lens[:len(T.TRIP_LENGTHS)] == list(T.TRIP_LENGTHS)
    assert len(s.trips) == len(s.trip_notes) and max(lens) == 257
    kind = {"ends": lambda w: w.endswith("@@") and "@@ " not in w and len(w) > 2, "@@": lambda w: w == "@@", "empty": lambda w: w == "",
            "x@@ @@": lambda w: w == "x@@ @@", "300": lambda w: T.nbytes(w) == 300, "plain": lambda w: w != "" and "@" not in w and " " not in w}
    for n in T.PLACED_LENGTHS:
        rows = [r for r in s.trips if len(r) == n]
        for a in ("ends", "@@", "empty", "x@@ @@", "300"):
            if n == 64:
                assert any(kind[a](s.decoder[r[63]]) for r in rows), (n, a)
                continue
            for b in ("plain", "empty", "@@"):
                assert any(kind[a](s.decoder[r[63]]) and kind[b](s.decoder[r[64]]) for r in rows), (n, a, b)
                if n == 129:
                    assert any(kind[a](s.decoder[r[127]]) and kind[b](s.decoder[r[128]]) for r in rows), (n, a, b)
    big = [r for r in s.trips + s.align + s.nothing + s.ids + s.unk_rows if any(T.nbytes(s.decoder.get(i, "")) == 5000 for i in r)]
    assert 1 <= len(big) <= 8                                                    # the 5000-byte words stay in a handful of rows
    last = [r for r in s.trips if r and s.decoder[r[-1]].endswith("@@")]
    assert {len(r) for r in last} >= {1, 2, 64, 65, 128}
    pool = {s.cls(i).split(":")[0] for r in s.trips[:len(T.TRIP_LENGTHS)] for i in r}
    assert pool == {"plain", "ends", "inner", "space", "empty"}


def test_trip_edges_carry_cuts_and_inner_words(s, tables):
    cut = inner = 0
    for r in s.trips:
        words = [tables.decoder[i] for i in r]
        cut += any(words[c - 1].endswith("@@") for c in range(T.TRIP, len(r), T.TRIP))
        inner += any("@@ " in words[c - 1] or "@@ " in words[c] for c in range(T.TRIP, len(r), T.TRIP))
    n = len(s.trips)
    assert cut >= n // 4 and inner >= n // 10, \
        "%d of %d rows cut an '@@' whose next token is in the next trip, %d have an inner '@@ ' at a trip edge" % (cut, n, inner)


def test_nothing_and_ids_are_what_they_claim(s, tables):
    e, at = s.id["empty:0"], s.id["ends:2"]
    for k in (1, 64, 65):
        assert [e] * k in s.nothing
    for k in (1, 2, 64, 65):
        assert [at] * k in s.nothing
    assert any(e in r and at in r for r in s.nothing)
    assert all(set(r) <= {e, at} for r in s.nothing)
    zero = [s.nothing[i] for i in s.nothing_batches[s.ZERO_BATCH]]
    assert sum(len(r) for r in zero) > 0 and all(O.decode(r, tables) == "" for r in zero)
    assert s.nothing_batches[0] == list(range(len(s.nothing)))
    flat = {i for r in s.ids for i in r}
    assert flat >= {-1, -2 ** 31, 2 ** 31 - 1, s.n_ids, s.n_ids + 1} | set(s.holes)
    assert all(-2 ** 31 <= i < 2 ** 31 for r in s.ids + s.align + s.trips + s.nothing + s.unk_rows for i in r)
    assert {2 ** 40, -2 ** 40} <= {i for r in s.ids_wide for i in r}
    assert [len(r) for r in s.unk_rows[:3]] == [1, 64, 65] and all(i not in tables.decoder for r in s.unk_rows[:3] for i in r)
    assert any(any(i in tables.decoder for i in r) and any(i not in tables.decoder for i in r) for r in s.unk_rows)


def test_unk_strings_are_the_forms(s):
    assert [T.nbytes(u) for u in T.UNKS] == [0, 1, 12, 13, 12, 2, 5, 4096]
    assert T.UNKS[4].endswith("@@") and T.UNKS[5] == "@@" and "@@ " in T.UNKS[6]
    assert not set(T.UNKS[1:]) & set(s.decoder.values()) - {"@@"}               # (only "@@" is a word of the table as well)


def test_fixture_is_what_the_builder_makes_today(s, fx):
    table, groups, unks, added = fx
    assert base64.b64decode(table["vocab_b64"]) == s.vocab
    assert base64.b64decode(table["second_vocab_b64"]) == T.second_vocab() and base64.b64decode(table["bpe_b64"]) == T.BPE
    assert added["ids"] == s.added_rows() and len(added["before"]) == len(added["after"]) == len(added["ids"])
    assert set(groups) == {"align", "trips", "nothing", "ids", "unk_rows"}
    for g, line in groups.items():
        assert line["ids"] == getattr(s, g), g
        assert len(line["result"]) == len(line["ids"])
    assert [u["unk_token"] for u in unks] == list(T.UNKS) and not any("raises" in u for u in unks)


def test_oracle_decodes_what_the_reference_decoded(s, fx):
    table, groups, unks, added = fx
    vocab, bpe = base64.b64decode(table["vocab_b64"]), base64.b64decode(table["bpe_b64"])
    t = O.Tables(vocab, bpe)
    n = 0
    for g, line in groups.items():
        for k, (ids, want) in enumerate(zip(line["ids"], line["result"])):
            assert T.same(O.decode(ids, t), want), (g, k, T.edges(s, ids))
            n += 1
    for u in unks:
        tu = O.Tables(vocab, bpe, O.DEFAULT_SPECIALS[:4] + (u["unk_token"],))
        for g, res in u["result"].items():
            for k, (ids, want) in enumerate(zip(getattr(s, g), res)):
                assert T.same(O.decode(ids, tu), want), (u["unk_token"][:16], g, k)
                n += 1
    # add_vocab_file leaves `decoder` alone (tokenize.py:40): before == after == the first file's table
    assert added["before"] == added["after"]
    for ids, want in zip(added["ids"], added["after"]):
        assert T.same(O.decode(ids, t), want), ids
    both = O.Tables(vocab + T.second_vocab(), bpe)
    # the first new word lands on the id the moved empty word holds in the decoder and decodes to "" before and after; the
    # larger new ids are past the table and decode to unk, although words have them now
    new = added["new_word_ids"]
    assert new["new0"] == s.n_ids - 1 == len(t.encoder) and t.decoder[new["new0"]] == "" and [new["new0"]] in added["ids"]
    late = [i for i in new.values() if i >= s.n_ids]
    assert len(set(late)) >= 2 and all([i] in added["ids"] and i in both.decoder and i not in t.decoder for i in late)
    assert all(added["after"][added["ids"].index([i])] == "<unk>" for i in late)
    assert {w: both.encoder[w] for w in added["new_word_ids"]} == added["new_word_ids"]
    assert added["vocab_size"] == [len(t.encoder), len(both.encoder)]
    for w, ids in added["encode_after"].items():
        assert O.encode(w, both) == ids and O.encode(w, t) == added["encode_before"][w], w
    assert added["encode_after"]["new0"] == [1, added["new_word_ids"]["new0"], 2] != added["encode_before"]["new0"]
    assert n > 1700
