"""CPU only: the inputs of test_gpu_bm25_doc_shapes.py keep their point.  bm25_oracles.WS, NEAR and sweep_docs() are meant to put every
whitespace code point of str.split(), and every non-whitespace neighbour of one in the UTF-8 byte space, at every byte offset around the
edges of the 64-byte tiles in which the index walks a document.  Nothing here touches the GPU: the offsets are read from the encoded
bytes, the whitespace from str."""
import pytest

from bm25_oracles import NEAR, SWEEP_K, WS, encoded, sweep_docs, vocab_oracle

EDGES = (62, 63, 64, 126, 127, 128)              # a 3-byte character from 62 / 126 and a 2-byte one from 63 / 127 straddle a tile edge


@pytest.fixture(scope="module")
def sweep():
    return sweep_docs()


def test_the_whitespace_is_all_of_it():
    assert len(WS) == 29 and len(set(WS)) == 29
    assert sorted(len(encoded(c)) for c in WS) == [1] * 10 + [2] * 2 + [3] * 17
    assert all(len("a" + c + "b") == 3 and ("a" + c + "b").split() == ["a", "b"] for c in WS)


def test_no_near_miss_is_whitespace():
    assert len(set(NEAR)) == len(NEAR) >= 32 and not set(NEAR) & set(WS)
    for c in NEAR:
        assert not c.isspace(), hex(ord(c))
        assert ("x" * 5 + c + "y").split() == ["x" * 5 + c + "y"], hex(ord(c))
    assert sorted(set(len(encoded(c)) for c in NEAR)) == [1, 2, 3, 4]
    assert encoded("\ud800") == b"\xed\xa0\x80"                          # the lone surrogate, as the packer writes it
    # the neighbours share their lead bytes with whitespace, and 85 / A0 follow another lead byte
    leads = {encoded(c)[:-1] for c in WS if len(encoded(c)) > 1}
    assert all(any(encoded(c)[:-1] == l for c in NEAR) for l in leads), leads
    assert encoded("\u0485") == b"\xd2\x85" and encoded("\u04a0") == b"\xd2\xa0"


def test_the_sweep_has_its_size(sweep):
    assert len(sweep) == len(WS + NEAR) * len(SWEEP_K) * 3 and len(sweep) <= 25_000
    assert len(set(sweep)) == len(sweep)
    assert list(SWEEP_K) == list(range(131))


@pytest.mark.parametrize("group", ["WS", "NEAR"])
def test_every_multi_byte_character_starts_at_every_edge(sweep, group):
    chars = [c for c in (WS if group == "WS" else NEAR) if len(encoded(c)) > 1]
    assert len(chars) == (19 if group == "WS" else 26)
    raw = [encoded(d) for d in sweep]
    for c in chars:
        e = encoded(c)
        for at in EDGES:
            hits = [r for r in raw if r[at:at + len(e)] == e and r[:at] == b"x" * at]
            # followed by a word, ending the document, and doubled
            assert any(r[at + len(e):] == b"y" for r in hits), (hex(ord(c)), at)
            assert any(len(r) == at + len(e) for r in hits), (hex(ord(c)), at)
            assert any(r[at + len(e):] == e + b"z" for r in hits), (hex(ord(c)), at)


def test_every_character_starts_at_every_lane_of_two_tiles(sweep):
    raw = set(encoded(d) for d in sweep)
    for c in WS + NEAR:
        e = encoded(c)
        assert all(b"x" * at + e in raw for at in range(129)), hex(ord(c))


def test_the_oracles_tell_whitespace_from_its_neighbours(sweep):
    lens = [len(d.split()) for d in sweep]
    n = len(SWEEP_K)
    assert lens[:3] == [1, 0, 1] and lens[3:6] == [2, 1, 2]              # "\ty", "\t", "\t\tz"; "x\ty", "x\t", "x\t\tz"
    assert set(lens[len(WS) * n * 3:]) == {1}                            # a near miss never cuts
    words, df = vocab_oracle(sweep)
    assert len(words) == len(set(words)) == len(df) and words[:2] == ["y", "z"] and sum(df) == sum(len(set(d.split())) for d in sweep)
    assert df[words.index("z")] == len(WS) * n and df[words.index("x" * 64)] == 3 * len(WS)
