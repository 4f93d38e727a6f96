"""Word segmentation by lexicon on the GPU against tests/segment_oracle.py: text, offsets, stats and join compare exactly.  The edges
are named from the constants the kernels are built around: gz_lexicon_info's `tile` (GZ_SEG_TILE token starts a trip of the candidate
kernel) and `wave` (the lanes of one ballot of the stretch compaction)."""
import numpy as np
import pytest

import segment_oracle as SO

pytestmark = pytest.mark.gpu
TOP = 2 ** 24 - 1


@pytest.fixture(scope="module")
def ctx():
    from genz_tokenize import _native
    c = _native.Context()
    yield c
    c.close()


def run(ctx, docs, words, costs=None, K=8, unk=1, split=True, fold=True, off0=b"", **switches):
    """the call against the oracle, document by document; returns (texts, stats, the lexicon's info after the call)"""
    from genz_tokenize import _native, segment as S
    for k, v in switches.items():
        _native.debug_set(k, v, ctx)
    try:
        lex = S.Lexicon.from_words(words, costs=costs, max_syllables=K, fold_case=fold, ctx=ctx)
        raw = [d.encode("utf-8") for d in docs]
        buf = np.frombuffer(off0 + b"".join(raw), dtype=np.uint8)
        off = len(off0) + np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
        r = S.segment_packed(buf, off, lex, split_punct=split, unk_cost=unk, return_tokens=True)
        info = lex.info()
        lex.close()
    finally:
        for k in switches:
            _native.debug_set(k, {"seg_lds": 1}.get(k, 0), ctx)
    table = dict(zip(lex.words, lex.costs))
    want = [SO.segment(d, table, K, unk, split, fold) for d in docs]
    text, oo = r["text"].tobytes(), r["offsets"]
    got = [text[oo[i]:oo[i + 1]].decode("utf-8") for i in range(len(docs))]
    assert oo[0] == 0 and got == [w[0] for w in want]
    assert r["stats"].tolist() == [w[1] for w in want]
    assert r["join"].tolist() == [j for w in want for j in w[2]]
    starts = [int(off[i]) + len(d[:p].encode()) for i, d in enumerate(docs) for p in token_positions(d, split)]
    assert r["tok_off"].tolist() == starts
    return got, r["stats"], info


def token_positions(doc, split):
    """character positions of the oracle's tokens in doc, by finding each in turn"""
    at, out = 0, []
    for t in SO.tokens(doc, split):
        at = doc.index(t, at)
        out.append(at)
        at += len(t)
    return out


SYL = ["s%d" % i for i in range(1, 10)]


@pytest.mark.parametrize("K", [2, 4, 8])
def test_spans_up_to_max_syllables_and_never_across_documents(ctx, K):
    words = ["_".join(SYL[:k]) for k in range(1, K + 1)] + ["s8_s9"]
    # s8 | s9: the entry s8_s9 would need the next document's first token -- after the bytes before text_off[0], between two
    # documents, and at the last document's end
    docs = ["s9", " ".join(SYL[:8]), " ".join(SYL[:K]), "s8", "s9 s8", "", "s1 s2 s8"]
    got, _, _ = run(ctx, docs, words, K=K, off0=b"s8 ")
    assert got[0] == "s9" and got[2] == "_".join(SYL[:K]) and got[3] == "s8" and got[4] == "s9 s8" and got[6].endswith(" s8")


def test_a_nine_syllable_entry_is_refused(ctx):
    from genz_tokenize import _native, segment as S
    with pytest.raises(_native.GzError, match="s1_s2_s3_s4_s5_s6_s7_s8_s9.*9 syllables") as e:
        S.Lexicon.from_words(["a", "_".join(SYL)], ctx=ctx)
    assert e.value.code == _native.GZ_E_INVALID


@pytest.mark.parametrize("unk", [1, TOP])
def test_choice_ties_greedy_and_unk_cost(ctx, unk):
    docs = ["a b c", "a b c d", "q a b q", "x"]
    got, stats, _ = run(ctx, docs, ["a_b", "b_c", "b_c_d", "a", "c"], costs=[2, 2, 1, 2, 2], K=3, unk=unk)
    assert got[0] == "a b_c"                                                             # a_b + c == a + b_c: the largest last word
    assert got[1] == "a b_c_d" and SO.leftmost_longest(docs[1], {"a_b": 2, "b_c": 2, "b_c_d": 1, "a": 2, "c": 2}, 3, unk)[0] == "a_b c d"
    assert stats[3].tolist() == [1, 1, 0, unk] and stats[2, 3] == 2 * unk + 2


def chain(n, first=0):
    """n tokens that are ONE stretch: every neighbouring pair is an entry"""
    return ["w%d" % i for i in range(first, first + n)]


def test_stretch_lengths_and_words_across_the_tile_and_wave_edges(ctx):
    from genz_tokenize import segment as S
    probe = S.Lexicon.from_words(["a"], ctx=ctx)
    tile, wave = probe.info()["tile"], probe.info()["wave"]
    probe.close()
    assert (tile, wave) == (1024, 64)
    K = 8
    pairs = ["w%d_w%d" % (i, i + 1) for i in range(40)]
    lens = [1, 2, K, K + 1]
    docs = [" ".join(chain(n)) for n in lens]
    _, _, info = run(ctx, docs, pairs + ["_".join(SYL[:8]), "a_b"], K=K)
    assert (info["stretches_1"], info["stretches_2_8"], info["stretches_longer"], info["longest_stretch"]) == (1, 2, 1, K + 1)
    # one token stream with a word across every edge: a_b over the first wave edge, s1..s8 over the tile edge (its first syllable 5
    # tokens before it), a_b over the wave edge at two tiles; cut into documents of 1000 tokens, then at the tile edge itself
    stream = ["x"] * (2 * tile + 100)
    stream[wave - 1:wave + 1] = ["a", "b"]
    stream[tile - 5:tile + 3] = SYL[:8]
    stream[2 * tile - 1:2 * tile + 1] = ["a", "b"]
    for cut in (1000, tile):
        docs = [" ".join(stream[i:i + cut]) for i in range(0, len(stream), cut)]
        got, stats, _ = run(ctx, docs, pairs + ["_".join(SYL[:8]), "a_b"], K=K)
        joined = " ".join(got)
        assert joined.count("a_b") == (2 if cut == 1000 else 1) and ("_".join(SYL[:8]) in joined) == (cut == 1000)


def test_one_stretch_of_5000_tokens_at_the_largest_cost(ctx):
    got, stats, info = run(ctx, [" ".join(["a"] * 5000), "a a"], ["a_a", "a_a_a"], costs=[TOP, TOP], K=3, unk=TOP)
    assert info["longest_stretch"] == 5000 and stats[0].tolist() == [5000, 1667, 1667, 1667 * TOP]


@pytest.mark.parametrize("split", [True, False])
def test_tokens_whitespace_punctuation_and_underscores(ctx, split):
    docs = ["", " \t\n", " sinh viên　\x1c công nghệ\x85", "(Hà Nội), ... 3.5", "sinh_viên công nghệ _ (_)", "!!", "a.b. .a"]
    got, stats, _ = run(ctx, docs, ["sinh_viên", "công_nghệ", "hà_nội", "3.5", "."], K=2, unk=3, split=split)
    assert got[2] == "sinh_viên công_nghệ" and got[4].startswith("sinh_viên công_nghệ")
    assert got[3] == ("( Hà_Nội ) , . . . 3.5" if split else "(Hà Nội), ... 3.5") and stats[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("fold", [True, False])
def test_case_folding_matches_and_keeps_the_bytes(ctx, fold):
    got, stats, _ = run(ctx, ["Sinh Viên ĐẠI HỌC Ứng DỤNG"], ["sinh_viên", "đại_học", "ứng_dụng"], K=2, fold=fold)
    assert got == (["Sinh_Viên ĐẠI_HỌC Ứng_DỤNG"] if fold else ["Sinh Viên ĐẠI HỌC Ứng DỤNG"]) and stats[0, 2] == (3 if fold else 0)


@pytest.mark.parametrize("switches", [dict(seg_hash_bits=3), dict(seg_lds=0), dict(seg_hash_bits=1, seg_lds=0)])
def test_hash_collisions_and_the_filter_do_not_change_the_result(ctx, switches):
    words = ["w%d_w%d" % (i, i + 1) for i in range(0, 60, 3)] + ["w%d" % i for i in range(60)]        # 80 keys in at most 8 hashes
    docs = [" ".join(chain(60)), " ".join(chain(7, 20)), "w1 w0 w3 w4 zz"]
    a = run(ctx, docs, words, K=2, unk=5)
    b = run(ctx, docs, words, K=2, unk=5, **switches)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_end_to_end_corpus_encode_vncore_and_device_route(ctx):
    import corpus
    from genz_tokenize import Tokenize, preprocess, segment as S
    text, offs, _ = corpus.config_corpus(2, n_docs=300, seed=3)
    raw = text.tobytes()
    seg = [raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(300)]
    plain = [d.replace("_", " ") for d in seg]
    tok = Tokenize()
    lex = S.Lexicon.from_corpus(seg, ctx=tok._ctx)
    table = dict(zip(lex.words, lex.costs))
    want = [SO.segment(d, table, 8, lex.unk_cost)[0] for d in plain]
    got = S.segment_batch(plain, lex)
    assert got == want
    a, b = tok.encode_batch(got, max_len=32), tok.encode_batch(want, max_len=32)
    assert np.array_equal(a["input_ids"], b["input_ids"])
    assert preprocess.vncore_tokenize(plain[7], lex) == got[7]
    with pytest.raises(TypeError, match="Lexicon"):
        preprocess.vncore_tokenize(plain[7], type("Client", (), {"tokenize": lambda self, t: t})())
    dev = S.segment_to_device(plain, lex)
    assert dev["text"].numpy()[:dev["n_bytes"]].tobytes() == "".join(got).encode()
    c, n, L = tok._ctx, 300, 32
    d_ids, d_mask, d_nr = c.alloc(4 * n * L), c.alloc(4 * n * L), c.alloc(4 * n)
    try:
        tok._sync_tables()
        c.encode_device(dev["text"].ptr, dev["offsets"].ptr, 0, 0, n, L, 3, n * L, d_ids, d_mask, d_n_real=d_nr)
        c.sync()
        ids = np.zeros((n, L), np.int32)
        c.d2h(ids, d_ids)
    finally:
        for d in (d_ids, d_mask, d_nr):
            c.free(d)
    assert np.array_equal(ids, a["input_ids"]) and dev["offsets"].numpy().tolist() == np.concatenate([[0], np.cumsum([len(g.encode()) for g in got])]).tolist()
    lex.close()


@pytest.mark.parametrize("words,costs,match", [
    (["a", "b"], [1, 2 ** 24], "cost 16777216 of entry 1 \"b\""), (["a", "b"], [0, 1], "cost 0 of entry 0 \"a\""),
    (["sinh_viên", "a", "sinh_viên"], [1, 1, 1], "entry 2 \"sinh_viên\" is given twice"), (["a", "b c"], [1, 1], "entry 1 \"b c\" holds whitespace"),
    (["a", ""], [1, 1], "entry 1 is empty"),
])
def test_lexicon_refusals_name_the_entry(ctx, words, costs, match):
    from genz_tokenize import _native
    from genz_tokenize._packing import pack
    with pytest.raises(_native.GzError, match=match) as e:
        ctx.lexicon_create(*pack(words), np.asarray(costs, np.int32), 8, 1)
    assert e.value.code == _native.GZ_E_INVALID


def test_capacity_too_small_leaves_valid_offsets(ctx):
    from genz_tokenize import _native, segment as S
    from genz_tokenize._packing import pack
    lex = S.Lexicon.from_words(["a_b"], ctx=ctx)
    buf, off = pack(["a b (c)", "a"])
    with pytest.raises(_native.GzError) as e:
        ctx.segment(lex.handle, buf, off, 1, 1, capacity=8)
    assert e.value.code == _native.GZ_E_CAPACITY and e.value.out_off.tolist() == [0, 9, 10]
    assert ctx.segment(lex.handle, buf, off, 1, 1, capacity=10)[0].tobytes() == b"a_b ( c )a"
    lex.close()
