"""CPU: the BM25 fixtures (tests/golden/g8_bm25.jsonl.gz, written by make_bm25_golden.py from the reference's ranking.py) against
the numpy restatement in tests/bm25_restate.py -- word statistics, df, idf and every score, compared as bit patterns."""
import numpy as np
import pytest

import bm25_restate as R
from conftest import read_jsonl
from genz_tokenize import _native, ranking

CASES = read_jsonl("g8_bm25.jsonl.gz")


def val(x):
    return int(x["v"]) if x["t"] == "int" else float.fromhex(x["v"])


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    """Bit patterns equal; a nan only has to meet a nan (float.hex, the fixture's form, keeps no sign or payload of a nan)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def test_fixture_covers_the_edge_cases():
    assert len(CASES) >= 20
    assert any(c["num_doc"] == 0 for c in CASES)
    assert any(c["num_doc"] and not any(c["fieldLens"]) for c in CASES)
    assert any(c["num_doc"] >= 300 for c in CASES)
    assert any(c["b"]["t"] == "int" and c["k1"]["t"] == "int" for c in CASES)
    assert any(c["cls"] == "BM25Plus" and np.signbit(val(c["delta"])) for c in CASES)
    assert any(s == "int:0" for c in CASES for r in c["results"] for s in r["scores"])


@pytest.mark.parametrize("i", range(len(CASES)))
def test_word_statistics(i):
    c = CASES[i]
    lens, freq = R.stats(c["documents"])
    assert c["num_doc"] == len(c["documents"])
    assert lens == c["fieldLens"]
    assert [[[w, n] for w, n in f.items()] for f in freq] == c["frequency_word_in_doc"]
    assert same([R.avg_field_len(lens)], [float.fromhex(c["avgFieldLen"])])
    for r in c["results"]:
        assert r["words"] == c["queries"][c["results"].index(r)].split()
        assert [R.doc_freq(freq, w) for w in r["words"]] == r["df"]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_scores_bit_for_bit(i):
    """Scores from the RECORDED idf (so this host's np.log plays no part): every float64 of the reference, nan and -0.0 included."""
    c = CASES[i]
    lens, freq = R.stats(c["documents"])
    avg = R.avg_field_len(lens)
    b, k1 = val(c["b"]), val(c["k1"])
    delta = val(c["delta"]) if c["cls"] == "BM25Plus" else None
    for r in c["results"]:
        if not c["num_doc"]:
            assert r["scores"] == []
        elif not r["words"]:
            assert r["scores"] == ["int:0"] * c["num_doc"]
        else:
            got = R.scores(lens, freq, avg, r["words"], [float.fromhex(v) for v in r["idf"]], b, k1, delta)
            want = np.array([float.fromhex(s) for s in r["scores"]])
            assert same(got, want), (i, r["words"])


def test_idf_expression_reproduces_the_recorded_idf():
    """ranking.py:31 evaluated here, scalar np.log, against the reference's recorded idf.  A difference here is this host's
    np.log (not correctly rounded, it may differ by an ulp between machines), not a kernel mismatch."""
    diff = []
    for c in CASES:
        for r in c["results"]:
            for w, d, v in zip(r["words"], r["df"], r["idf"]):
                if float(R.idf(c["num_doc"], d)).hex() != v:
                    diff.append((c["num_doc"], d, v, float(R.idf(c["num_doc"], d)).hex()))
    assert not diff, "this host's np.log differs from the one the fixtures were recorded with (not a kernel mismatch): %r" % diff[:5]


def test_ranking_surface_without_a_device():
    """The module's face and its C ABI are there; non-str documents and queries are refused before any device work (a stated
    deviation: the reference takes anything with .split())."""
    assert {"gz_bm25_build", "gz_bm25_build_device", "gz_bm25_info", "gz_bm25_field_lengths", "gz_bm25_lookup", "gz_bm25_score",
            "gz_bm25_score_device", "gz_bm25_destroy"} <= set(_native.SYMBOLS)
    assert issubclass(ranking.BM25Plus, ranking.BM25)
    for bad in (["a b", 3], ["a", b"b"], [None]):
        with pytest.raises(TypeError):
            ranking.BM25(bad)
    with pytest.raises(TypeError):
        ranking.BM25Plus(("x", 1.5))
