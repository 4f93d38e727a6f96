"""CPU-only: search over word groups exists on every layer -- the three C entry points are declared with their argument counts,
documented in the header's ranking block, exported and bound; _native.Context routes to them; genz_tokenize.ranking has
search_groups / count_groups / group_df / expand / search_fuzzy with their defaults on both classes; search / count_matches are what
they were; and every bad argument is refused before any native call.  Nothing is computed here (tests/test_gpu_bm25_groups.py does
that)."""
import inspect
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "genz_tokenize.h")
NAMES = {"gz_bm25_search_groups": 15, "gz_bm25_search_groups_device": 15, "gz_bm25_match_count_groups": 9}
# (the issue adds functions only: what the neighbours take stays)
OLD = {"gz_bm25_search_bool": 14, "gz_bm25_search_bool_device": 14, "gz_bm25_match_count_bool": 8, "gz_bm25_search": 11,
       "gz_bm25_match_count": 5, "gz_bm25_search_near": 19, "gz_bm25_similar": 10}


def test_symbols_declared_exported_and_bound():
    native = pytest.importorskip("genz_tokenize._native")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for n, argc in dict(NAMES, **OLD).items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S)
        assert decl, n
        assert len(decl.group(1).split(",")) == argc, n
        assert hasattr(lib, n), "missing export: " + n
        assert n in native.SYMBOLS
        assert len(getattr(lib, n).argtypes) == argc, n
    assert lib.gz_version() == 0x010100
    assert native.GZ_BM25_GROUP_MAX == 64
    vp = native.C.c_void_p
    # the boolean form's arguments with (alt_terms, alt_off, group_idf, group_off) where (terms, idf, query_off) stand
    b = lib.gz_bm25_search_bool.argtypes
    assert lib.gz_bm25_search_groups.argtypes == [b[0], vp, vp, vp, vp] + b[4:]
    assert lib.gz_bm25_search_groups_device.argtypes == lib.gz_bm25_search_groups.argtypes
    c = lib.gz_bm25_match_count_bool.argtypes
    assert lib.gz_bm25_match_count_groups.argtypes == [c[0], vp, vp, vp] + c[3:]
    p = inspect.signature(native.Context.bm25_search_groups).parameters
    assert list(p)[:9] == ["self", "index", "alt_terms", "alt_off", "group_idf", "group_off", "params", "plus", "k"]
    for name in ("mode", "ex_terms", "ex_off", "d_ids", "d_scores", "d_counts"):
        assert p[name].default == (0 if name == "mode" else None), name
    p = inspect.signature(native.Context.bm25_match_count_groups).parameters
    assert list(p) == ["self", "index", "alt_terms", "alt_off", "group_off", "mode", "ex_terms", "ex_off"]
    # the plain bindings are what they were
    for m in ("bm25_search", "bm25_match_count"):
        assert list(inspect.signature(getattr(native.Context, m)).parameters)[-3:] == ["nr_terms", "nr_off", "nr_window"], m


def test_header_documents_the_functions():
    src = open(HEADER).read()
    assert re.search(r"^#define GZ_VERSION\s+0x010100\b", src, flags=re.M)
    assert re.search(r"^#define GZ_BM25_GROUP_MAX\s+64\b", src, flags=re.M)
    block = src[src.index("BM25 / BM25Plus ranking"):]
    comment = block[:block.index("#define GZ_BM25_TOPK_MAX")]
    for n in NAMES:
        assert re.search(r"^ \*   %s\s" % n, comment, flags=re.M), n
    for word in ("GZ_BM25_GROUP_MAX", "GZ_E_LIMIT", "GZ_E_INVALID", "alt_off", "group_idf", "group_off", "gz_groups.inc", "bit for bit"):
        assert word in comment[comment.index(" *   gz_bm25_search_groups"):], word


def test_sources_and_documents_name_the_feature():
    csrc = os.path.join(ROOT, "genz-tokenize_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "gz_groups.inc"))
    hip = open(os.path.join(csrc, "gz_kernels.hip")).read()
    assert hip.index('#include "gz_search.inc"') < hip.index('#include "gz_groups.inc"')
    assert "gz_groups.inc" in open(os.path.join(csrc, "Makefile")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "search_fuzzy(" in readme and "search_groups(" in readme and "word group" in readme.lower()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Word groups" in design and "gz_groups.inc" in design


def test_ranking_signatures():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    p = inspect.signature(ranking.BM25.search_groups).parameters
    assert list(p) == ["self", "groups", "k", "match", "exclude"]
    assert p["match"].default == "any" and p["exclude"].default is None
    p = inspect.signature(ranking.BM25.count_groups).parameters
    assert list(p) == ["self", "groups", "match", "exclude"]
    assert p["match"].default == "any" and p["exclude"].default is None
    assert list(inspect.signature(ranking.BM25.group_df).parameters) == ["self", "groups"]
    p = inspect.signature(ranking.BM25.expand).parameters
    assert list(p) == ["self", "queries", "max_edits", "limit", "only_unknown", "prefix_last"]
    assert [p[n].default for n in list(p)[2:]] == [1, 8, True, False]
    p = inspect.signature(ranking.BM25.search_fuzzy).parameters
    assert list(p) == ["self", "queries", "k", "max_edits", "limit", "only_unknown", "prefix_last", "match", "exclude"]
    assert [p[n].default for n in list(p)[3:]] == [1, 8, True, False, "any", None]
    for name in ("search_groups", "count_groups", "group_df", "expand", "search_fuzzy"):
        assert getattr(ranking.BM25Plus, name) is getattr(ranking.BM25, name), name
        # phrase= / near are not offered together with groups
        assert not {"phrase", "near", "window"} & set(inspect.signature(getattr(ranking.BM25, name)).parameters), name
    # search / count_matches / similar_words are what they were
    assert list(inspect.signature(ranking.BM25.search).parameters) == ["self", "queries", "k", "match", "exclude", "phrase"]
    assert list(inspect.signature(ranking.BM25.count_matches).parameters) == ["self", "queries", "match", "exclude", "phrase"]
    assert list(inspect.signature(ranking.BM25.similar_words).parameters) == ["self", "words", "max_edits", "k"]
    doc = ranking.__doc__
    assert "Word groups:" in doc and "search_groups(" in doc and "search_fuzzy(" in doc and "expand(" in doc and "gz_groups.inc" in doc


class _NoNative:
    """stands in for the context: any native call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare(cls):
    m = cls.__new__(cls)
    m._ctx = _NoNative()
    m._index = 0
    m.num_doc = 3
    m._texts = ["a b", "b", ""]
    m._idf = {}
    return m


G2 = [[["a", "b"]], [["b"], ["a"]]]
# (groups, keywords) -> the exception
BAD_GROUPS = [
    ("ab", {}, TypeError),                              # a str where the list of queries is due
    (["a b", "b"], {}, TypeError),                      # a str where a query's list of groups is due
    ([["a", "b"], [["b"]]], {}, TypeError),             # a str where a group's list of alternatives is due
    ([[["a", 3]], [["b"]]], {}, TypeError),
    ([[["a", b"b"]], [["b"]]], {}, TypeError),
    ([[["a", None]], [["b"]]], {}, TypeError),
    ([[["a"]], [[["b"]]]], {}, TypeError),              # one level too many
    ([[["a"]], 5], {}, TypeError),
    ([[["a"]], [7]], {}, TypeError),
    (G2, {"match": "some"}, ValueError),
    (G2, {"match": 1}, TypeError),
    (G2, {"exclude": ["a"]}, ValueError),
    (G2, {"exclude": ["a", "b", "c"]}, ValueError),
    (G2, {"exclude": ["a", 1]}, TypeError),
]


def test_group_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls)
        for groups, kw, exc in BAD_GROUPS:
            with pytest.raises(exc):
                m.search_groups(groups, 3, **kw)
            with pytest.raises(exc):
                m.count_groups(groups, **kw)
            if not kw:
                with pytest.raises(exc):
                    m.group_df(groups)
        for k, exc in ((0, ValueError), (-1, ValueError), (True, TypeError), (2.0, TypeError), ("3", TypeError)):
            with pytest.raises(exc):
                m.search_groups(G2, k)
            with pytest.raises(exc):
                m.search_fuzzy(["a", "b"], k)


Q2 = ["a b", "b"]
# (queries, keywords) -> the exception
BAD_FUZZY = [
    (["a", 3], {}, TypeError),
    ([b"a", "b"], {}, TypeError),
    (Q2, {"max_edits": -1}, ValueError),
    (Q2, {"max_edits": 65}, ValueError),
    (Q2, {"max_edits": 1.0}, TypeError),
    (Q2, {"max_edits": True}, TypeError),
    (Q2, {"limit": 0}, ValueError),
    (Q2, {"limit": 65}, ValueError),
    (Q2, {"limit": -3}, ValueError),
    (Q2, {"limit": 2.0}, TypeError),
    (Q2, {"limit": True}, TypeError),
    (Q2, {"limit": "8"}, TypeError),
]
BAD_SEARCH_FUZZY = BAD_FUZZY + [
    (Q2, {"match": "some"}, ValueError),
    (Q2, {"match": 0}, TypeError),
    (Q2, {"exclude": ["a"]}, ValueError),
    (Q2, {"exclude": ["a", 2]}, TypeError),
]


def test_fuzzy_validation_before_any_native_call():
    ranking = pytest.importorskip("genz_tokenize.ranking")
    for cls in (ranking.BM25, ranking.BM25Plus):
        m = _bare(cls)
        for queries, kw, exc in BAD_FUZZY:
            with pytest.raises(exc):
                m.expand(queries, **kw)
        for queries, kw, exc in BAD_SEARCH_FUZZY:
            with pytest.raises(exc):
                m.search_fuzzy(queries, 3, **kw)
        # queries without words need no native call to expand
        assert m.expand([]) == [] and m.expand(["", "  "], prefix_last=True) == [[], []]
