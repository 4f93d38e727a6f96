"""The encode pipeline at the constants its kernels are built around, against the oracles, exactly: ids, mask, row_off and n_real.

The documents come from tests/encode_edges.py (tests/test_encode_edges_inputs.py proves on the CPU that each sits on its edge); the
expected rows come from the plain-C restatement (gz_oracle_c.COracle.call_packed) for whole batches, tied to the Python oracle
(gz_oracle.call_batch) on a sample of every batch.  Every batch runs through the kernel pipeline (small = 0) with the whole-word
tables on and off and through the one-launch kernel where it qualifies; switches are set on the context and put back.

  A  gz_classify_kernel     whitespace, line feeds, document starts and the end of the text at tile, lane and block edges
  B  gz_words2_kernel       word lengths at the key, table, end-search and look-ahead boundaries; 63 .. 512 word starts a tile
  C  gz_mpre_kernel & co.   miss totals around the groups of 64 and the tiles of 3 072, by symbol count; blocks without a miss
  D  gz_rows1_kernel        rounds at CAP words and entries, MLCAP merged words, documents per wave, the max_len classes
"""
import contextlib

import numpy as np
import pytest

import encode_edges as E
import gz_oracle as O

pytestmark = pytest.mark.gpu

DEFAULTS = dict(small=1, scan_multi=8192, m2_split_always=0, m2_split_min=65536, hot_miss_wgs=0, near_limit=1 << 25)
# (label, switches, whole-word tables)
PIPELINE = [("pipeline", dict(small=0), True), ("pipeline, tables off", dict(small=0), False)]
ONE_LAUNCH = [("one launch", dict(small=1), True), ("one launch, tables off", dict(small=1), False)]
CHAINED = [("pipeline, chained scans", dict(small=0, scan_multi=0), True)]
MISS_SWITCHES = [("merge instances share a launch", dict(small=0, m2_split_always=1, m2_split_min=1)),
                 ("one merge workgroup", dict(small=0, hot_miss_wgs=1)),
                 ("far records", dict(small=0, near_limit=300))]


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


@pytest.fixture(scope="module")
def co():
    import gz_oracle_c as OC
    import corpus
    return OC.COracle(open(corpus.VOCAB_PATH, "rb").read(), open(corpus.BPE_PATH, "rb").read())


@contextlib.contextmanager
def switches(tok, **kv):
    from genz_tokenize import _native
    try:
        for k, v in kv.items():
            _native.debug_set(k, v, tok._ctx)
        yield
    finally:
        for k in kv:
            _native.debug_set(k, DEFAULTS[k], tok._ctx)


def expected(co, tables, b, max_len, pair=False):
    """The C oracle's rows of the batch (computed once per call shape), tied to the Python oracle on a sample of its documents: the
    first, the last and up to six spread between them."""
    text, off = np.ascontiguousarray(b.text), b.off
    ids, mask, tt, sq, row, pl, st = co.call_packed(text, off, text if pair else None, off if pair else None, max_len=max_len)
    lens = np.diff(row)
    n = len(b.docs)
    sample = sorted({0, n - 1} | {(n * k) // 7 for k in range(1, 7)})
    docs = b.strings(sample)
    I, M, _, _, _ = O.call_batch(tables, docs, docs if pair else None, max_len)
    for k, d in enumerate(sample):
        assert ids[row[d]:row[d + 1]].tolist() == I[k] and mask[row[d]:row[d + 1]].tolist() == M[k], (b, max_len, d)
    if max_len is None:
        n_real = lens.astype(np.int32)
    else:
        full = np.diff(co.call_packed(text, off, max_len=None)[4])
        n_real = np.minimum(full, max_len).astype(np.int32)
    return ids[:row[-1]], mask[:row[-1]], row, n_real


def run(tok, co, tables, b, routes):
    """The batch through every route at each of its max_len; every comparison exact."""
    text = np.ascontiguousarray(b.text)
    for max_len in b.max_lens:
        ids, mask, row, n_real = expected(co, tables, b, max_len)
        for label, sw, word_table in routes:
            with switches(tok, **sw):
                got = tok.encode_packed(text, b.off, max_len=max_len, word_table=word_table)
            what = (b.name, max_len, label)
            assert np.array_equal(np.asarray(got["row_off"], np.int64), row), what
            assert np.array_equal(np.asarray(got["input_ids"]).reshape(-1), ids), what
            assert np.array_equal(np.asarray(got["attention_mask"]).reshape(-1), mask), what
            assert np.array_equal(np.asarray(got["n_real"]), n_real), what


def routes_for(b, extra=()):
    assert b.takes_one_launch() or max(len(d) for d in b.docs) > E.SMALL_DOC
    return PIPELINE + (ONE_LAUNCH if b.takes_one_launch() else []) + list(extra)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True], ids=["tile-edges", "block-edges"])
@pytest.mark.parametrize("variant", E.VARIANTS)
def test_classification_at_tile_lane_and_block_edges(tok, co, oracle_tables, variant, shifted):
    """Each of the 29 whitespace code points at every byte split over a tile edge, a lane edge and (behind a leading document of 2 048
    bytes) a block edge, whole on either side of it, and the glue rule's line feeds as the next tile's first byte -- beside tiles that
    take the fast form and beside tiles that take the general one (a \\t in front, U+2003 behind, both).

    The parent commit gets U+1680 cut 1|2 wrong, at tile edges and at block edges, wherever the tile in front is plain (the variants
    "plain" and "after"): E1 as a tile's last byte with 9A 80 opening the next left the first tile in the fast form, which sees a letter
    and carries nothing over, so the word was not split there -- and at a block edge the next block's look-back set a start bit behind
    the character whose end bit the block before never wrote.  By reading, and by the CPU restatement of the fast-form test
    (tests/test_encode_edges_inputs.py); the parent's library was not run on these cases."""
    b = E.family_a(variant, shifted)
    run(tok, co, oracle_tables, b, routes_for(b, CHAINED))


def test_classification_of_pairs(tok, co, oracle_tables):
    """One paired run of the plain documents against themselves (pair mode has its own row kernels: a smoke check)."""
    b = E.family_a("plain", True)
    text = np.ascontiguousarray(b.text)
    ids, mask, tt, sq, row, pl, st = co.call_packed(text, b.off, text, b.off, max_len=None)
    with switches(tok, small=0):
        got = tok.encode_packed(text, b.off, text, b.off, max_len=None)
    k = int(row[-1])
    assert np.array_equal(np.asarray(got["row_off"], np.int64), row)
    assert np.array_equal(np.asarray(got["input_ids"]).reshape(-1), ids[:k])
    assert np.array_equal(np.asarray(got["attention_mask"]).reshape(-1), mask[:k])
    assert np.array_equal(np.asarray(got["n_real"]), np.diff(row))


def test_document_starts_and_empty_documents_at_edges(tok, co, oracle_tables):
    """Document boundaries exactly on tile, lane and block edges with letters on both sides -- only the start bit separates the two
    words -- one, two and 70 empty documents at each of them, and a line feed as the next document's first byte (not glued across)."""
    for b in E.family_a_boundaries():
        run(tok, co, oracle_tables, b, routes_for(b, CHAINED))


@pytest.mark.parametrize("kind", E.END_KINDS)
def test_the_end_of_the_text(tok, co, oracle_tables, kind):
    """Total sizes of 0, 1, 15, 16 and 17 bytes past a multiple of 32 and 0 and 1 past a multiple of 1 024 and of 4 096: the last word ends
    exactly at the last byte, has a glued line feed as the last byte, or the text ends in a multi-byte whitespace character."""
    n = 0
    for b in E.family_a_text_end():
        if b.info["end"] == kind:
            run(tok, co, oracle_tables, b, routes_for(b, CHAINED))
            n += 1
    assert n == len(E.END_SIZES)


def test_u1680_cut_by_tile_edges_of_the_last_blocks(tok, co, oracle_tables):
    """U+1680 cut 1|2 by tile edges where gz_classify_kernel takes the byte behind the tile from each of its three sources: the next
    tile's registers, the byte loaded with a block inside the text, and the guarded load of the last blocks (with the text ending 16,
    15 and 0 bytes behind the character's block, and with the character as the text's last).  The parent commit gets all of them wrong."""
    for b in E.family_a_tail_blocks():
        run(tok, co, oracle_tables, b, routes_for(b, CHAINED))


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hit", "invented"])
def test_word_lengths_across_tile_and_block_edges(tok, co, oracle_tables, kind):
    """Words of 1, 12, 13, 16, 17, 32, 33, 48, 49 and 80 bytes -- the 16-byte key, the extra dword of 13..16-byte keys, the long-key table
    of 17..32 bytes, the 32-bit end search, the 48 bytes of look-ahead -- each started in every one of the last 1..48 bytes of a tile
    that lets it end in the next, at tile edges and at a block edge; once as entries of the bundled vocabulary, once invented.  (The
    bundled vocabulary has no whole word of 48, 49 or 80 bytes: those lengths run invented only.)"""
    b = E.family_b_words(kind)
    run(tok, co, oracle_tables, b, routes_for(b))


def test_word_lengths_at_the_end_of_the_text(tok, co, oracle_tables):
    """The same words as the text's last word: started in the last bytes of a tile, ended at the text's last byte."""
    for b in E.family_b_text_end():
        run(tok, co, oracle_tables, b, routes_for(b))


def test_word_starts_per_tile(tok, co, oracle_tables):
    """Tiles of 63, 64, 65, 129 and 512 word starts (512: "a a a ...", eight starts in a lane's 16 bytes, the loop behind the unrolled
    four) and a tile whose only word start is its last byte."""
    b = E.family_b_tiles()
    run(tok, co, oracle_tables, b, routes_for(b))


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", E.MISS_FORMS)
def test_miss_totals(tok, co, oracle_tables, form):
    """0, 1, 63, 64, 65, 3 071, 3 072, 3 073 and 6 145 misses (tables off: every word), all of one symbol count -- one class takes a whole
    pre-pass tile -- or spread over 1..16 symbols with words of 17, 64 and 65 among them (the wide and long kernels); with the merge
    kernel's two instances in one launch, with one merge workgroup, and with far records from place 300 on."""
    for total in E.MISS_TOTALS:
        b = E.family_c(total, form)
        run(tok, co, oracle_tables, b, routes_for(b, [(label, sw, False) for label, sw in MISS_SWITCHES]))


@pytest.mark.parametrize("tables_on", [False, True], ids=["spaces", "hits"])
def test_blocks_without_a_miss(tok, co, oracle_tables, tables_on):
    """The group look-up of the miss lists across one, three and nine blocks without a miss (4 096 spaces; with the tables on, table hits
    only), and a block of 2 048 one-letter words: the most misses a block can hold."""
    b = E.family_c_blocks(tables_on)
    run(tok, co, oracle_tables, b, routes_for(b, [(label, sw, tables_on) for label, sw in MISS_SWITCHES]))


# ---------------------------------------------------------------------------------------------------------------------------------
def dense_routes(b, far=False):
    return routes_for(b, [("far records", dict(small=0, near_limit=300), True)] if far else [])


@pytest.mark.parametrize("max_len,n_docs", E.D_SHAPES)
def test_dense_rows_shapes(tok, co, oracle_tables, max_len, n_docs):
    """max_len on both sides of the classes of gz_rows1_kernel (CAP 512 and eight documents a wave up to 256, CAP 1 024 and four up to
    512, one above), powers of two and not; document counts around the wave and workgroup sizes; documents of max_len - 2,
    max_len - 1, max_len and many more words."""
    b = E.family_d_shapes(max_len, n_docs)
    run(tok, co, oracle_tables, b, dense_routes(b))


def test_dense_rows_rounds_at_cap(tok, co, oracle_tables):
    """A wave's documents whose words add up to CAP - 1, CAP and CAP + 1; rounds whose row entries do; the round whose words fit and
    whose rows do not (the roll-back); rounds of empty documents."""
    for max_len in (256, 512):
        for delta in (-1, 0, 1):
            for b in (E.family_d_cap(max_len, delta), E.family_d_cap_rows(max_len, delta)):
                run(tok, co, oracle_tables, b, dense_routes(b))
    for b in (E.family_d_rollback(), E.family_d_empty()):
        run(tok, co, oracle_tables, b, dense_routes(b))


def test_dense_rows_merged_words(tok, co, oracle_tables):
    """95, 96, 97 and 200 merged words in one round among table hits (the list holds 96), near and far records mixed, and all far; a
    merged word of 5 pieces and a wide one of some 270 cut at position max_len - 1 with 2, 1, 0 and 5 pieces in front of it."""
    for n in (95, 96, 97, 200):
        b = E.family_d_merged(n)
        run(tok, co, oracle_tables, b, dense_routes(b, far=True))
    for max_len in (4, 16, 256, 260, 1024):
        for wide in (False, True):
            b = E.family_d_straddle(max_len, wide)
            run(tok, co, oracle_tables, b, dense_routes(b, far=True))
