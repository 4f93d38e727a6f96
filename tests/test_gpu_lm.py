"""The token n-gram language model and perplexity on the GPU against tests/lm_oracle.py.  Integers compare exactly.  bits_fx compares
per row with abs(device - oracle) <= n_tokens, a bound that is derived, not measured: a float64 log2 of a value below 2^32 is within
a few ulp, below 2^-46 absolute, which is 2^-22 of a grid step, so a position's grid value differs from the oracle's by at most 1,
and only when its cost lies within 2^-22 of a half step.  Device against device is exact."""
import ctypes

import numpy as np
import pytest

import lm_oracle as LO
from test_gpu_ngram import FILL, PIECE, Guarded, mixture, reference, tok  # noqa: F401  (tok: the module's Tokenize fixture)

pytestmark = pytest.mark.gpu
INTS = ("n_tokens", "n_order", "token_order", "token_num", "token_den", "row_off")


def same(got, want, keys=INTS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    diff = np.abs(got["bits_fx"].astype(np.int64) - want["bits_fx"].astype(np.int64))
    assert got["bits_fx"].dtype == np.uint64 and (diff <= want["n_tokens"]).all(), diff.max()


def check(tok, ref, N, rows, alpha=0.4, framed=False):
    """model, slot count and scores against the oracle; every order 0..N occurs and some gram has a count above 1 -- asserted on the
    ORACLE's output, before any device call"""
    model = LO.train(ref, N, framed)
    want = LO.score(model, N, rows, alpha, framed)
    assert (want["n_order"].sum(axis=1) > 0).all() and max(model[0][N].values()) > 1
    with tok.ngram_lm(ref, N, framed=framed) as lm:
        assert (lm.order, lm.n_rows, lm.n_ids, lm.n_tokens) == (N, len(ref), sum(len(r) for r in ref), model[1])
        assert (lm.n_grams, lm.n_distinct) == LO.grams(model, N)
        info = tok._ctx.ngram_lm_info(lm._handle)                         # the smallest power of two that is at least twice the positions
        assert info["slots"] == 1 << (2 * sum(lm.n_grams[1:]) - 1).bit_length() and lm.device_bytes >= 16 * info["slots"] + 4 * lm.n_ids
        got = tok.perplexity_rows(rows, lm, alpha, framed=framed, return_tokens=True)
        same(got, want)
        bare = tok.perplexity_rows(rows, lm, alpha, framed=framed)
        assert len(bare) == 5 and all(np.array_equal(bare[k], got[k]) for k in bare)
    bpt = got["bits_fx"] / 2.0 ** 24 / np.maximum(got["n_tokens"], 1)
    assert np.array_equal(got["bits_per_token"], bpt) and np.array_equal(got["perplexity"], np.where(got["n_tokens"] > 0, 2.0 ** bpt, np.inf))
    return want, got


def queries(rng, ref, N, lengths):                                        # copies out of the training bodies between runs over 0..8 (7, 8: never trained)
    return [mixture(rng, ref, max(N, 2), T) for T in lengths]


@pytest.mark.parametrize("N,alpha", [(1, 2.0 ** -8), (2, 1), (5, 0.4), (8, 0.4)])
def test_body_lengths_at_the_rules_and_the_trips_edges(tok, N, alpha):
    """nothing, one id, around the order; around one and two trips of 64 positions (the carried predecessor ids) -- on both sides"""
    rng = np.random.default_rng(N)
    lengths = sorted({0, 1, max(N - 1, 0), N, N + 1, 63, 64, 65, 64 + N - 2, 64 + N - 1, 64 + N, 127, 128, 129})
    ref = reference(rng, lengths, max(N, 2))
    want, _ = check(tok, ref, N, queries(rng, ref, N, lengths) + [list(b) for b in ref[-3:]], alpha)
    assert want["n_tokens"].tolist()[:len(lengths)] == lengths and (want["n_order"][0, -3:] == 0).all()      # (a training body: no token unseen)


@pytest.mark.parametrize("N", [2, 8])
def test_pieces(tok, N):
    """one below, at and above one piece and a body of five pieces, on BOTH sides, the long bodies with one gram planted across, before
    and behind a piece boundary: long rows meet by atomics, and a later piece fetches the ids (score: and the counts) before its start"""
    rng = np.random.default_rng(50 + N)
    g = [3, 1, 4, 1, 5, 2, 6, 5][:N]
    planted = (PIECE - N // 2, 2 * PIECE - N, 3 * PIECE, 4 * PIECE - 1)   # across, before, behind, across by one id
    ref = reference(rng, [50, 300, PIECE - 1, PIECE, PIECE + 1, 4 * PIECE + 300], max(N, 2))
    long = mixture(rng, ref, max(N, 2), 4 * PIECE + 300)
    for p in planted:
        ref[-1][p:p + N] = long[p:p + N] = g
    want, _ = check(tok, ref, N, queries(rng, ref, N, [PIECE - 1, PIECE, PIECE + 1]) + [long, [], [7, 8, 1]])
    ends = want["row_off"][3] + np.array(planted) + N - 1
    assert (want["token_order"][ends] == N).all() and (want["token_num"][ends] >= 4).all()


@pytest.mark.parametrize("key,values", [("lm_combine", (1, 0)), ("lm_hash_bits", (0, 1, 4, 32))])
def test_switches_change_nothing(tok, key, values):
    """lm_combine over 5000 equal ids (one hot slot: the counts reach 5000, N - k + 1 below that per order), with and without the
    combining of a trip's equal grams; lm_hash_bits over more than 300 distinct grams: with 1 bit every probe of every order starts in
    one of two slots with the same tag"""
    from genz_tokenize import _native
    rng, hot = np.random.default_rng(13), key == "lm_combine"
    N, ref = (5, [[3] * 5000]) if hot else (4, reference(rng, [70, 0, 140, 3, 170], 4))
    rows = [[3] * 40, [3] * 3 + [4], [4] * 20, [2] + [3] * 13, [8, 3, 3]] if hot else queries(rng, ref, N, (0, 3, 4, 70, 200, 64))
    n_grams, n_distinct = LO.grams(LO.train(ref, N), N)
    assert (n_grams, n_distinct) == ((5000, 5000, 4999, 4998, 4997, 4996), (1,) * 6) if hot else sum(n_distinct) > 300
    results = []
    try:
        for v in values:
            _native.debug_set(key, v, tok._ctx)
            results.append(check(tok, ref, N, rows)[1])
    finally:
        _native.debug_set(key, values[0], tok._ctx)                       # (the default)
    assert all(np.array_equal(r[k], results[0][k]) for r in results for k in r)
    got = results[0]
    assert not hot or (got["token_num"][39] == 4996 and got["token_den"][39] == 4997 and got["token_num"][0] == got["token_den"][0] == 5000)


@pytest.mark.parametrize("P", [255, 256, 257])
def test_gram_totals_at_table_sizes(tok, P):
    """the gram positions of both orders together just below, at and above a power of two: the slot count, which `check` asserts"""
    rng = np.random.default_rng(P)
    ref = [rng.integers(0, 7, size=(P + 1) // 2).tolist(), rng.integers(0, 7, size=P // 2 + 1).tolist()]      # m1 + m2 + (m1 - 1) + (m2 - 1) = 2 P
    assert sum(LO.grams(LO.train(ref, 2), 2)[0][1:]) == 2 * P
    check(tok, ref, 2, queries(rng, ref, 2, (0, 2, 50, 130)))


@pytest.mark.parametrize("R", [1, 255, 256, 257])
def test_row_counts_at_block_edges(tok, R):
    rng = np.random.default_rng(100 + R)
    ref = [rng.integers(0, 7, size=int(T)).tolist() for T in rng.integers(0, 12, size=R)] + reference(rng, [40, 60, 5], 3)
    want, _ = check(tok, ref, 3, queries(rng, ref, 3, [60] + rng.integers(0, 40, size=R - 1).tolist()))
    assert want["n_order"].shape == (4, R)


def test_framed_against_bare_bodies(tok):
    N = 4
    rng = np.random.default_rng(31)
    ref = reference(rng, [0, 1, 3, 4, 5, 70], N)
    bodies = queries(rng, ref, N, (0, 1, 3, 4, 5, 70, 130))
    bare, _ = check(tok, ref, N, bodies)
    framed = [[-7] + b + [-9] for b in bodies] + [[], [5]]                # the frame is dropped whatever it holds; rows shorter than it
    want, _ = check(tok, [[-7] + b + [-9] for b in ref], N, framed, framed=True)      # (the oracle's frame cells are 0: `same` compares them)
    assert all(np.array_equal(want[k][..., :len(bodies)], bare[k]) for k in ("n_tokens", "n_order", "bits_fx"))


def test_slices_and_single_rows_equal_the_whole(tok):
    N = 5
    rng = np.random.default_rng(12)
    ref = reference(rng, [30, 100, 200], N)
    rows = queries(rng, ref, N, rng.integers(0, 150, size=60)) + queries(rng, ref, N, [PIECE + 300])
    with tok.ngram_lm(ref, N, framed=False) as lm:
        whole = tok.perplexity_rows(rows, lm, framed=False, return_tokens=True)
        same(whole, LO.score(LO.train(ref, N), N, rows))
        for a, b in ((0, 61), (0, 1), (17, 60), (60, 61), (5, 5)):
            part = tok.perplexity_rows(rows[a:b], lm, framed=False, return_tokens=True)
            assert all(np.array_equal(part[k], whole[k][a:b]) for k in ("n_tokens", "bits_fx", "bits_per_token", "perplexity")), (a, b)
            assert np.array_equal(part["n_order"], whole["n_order"][:, a:b])
        assert [tok.perplexity_rows([r], lm, framed=False)["bits_fx"][0] for r in rows[50:]] == whole["bits_fx"][50:].tolist()


def test_device_form_behind_junk(tok):
    """rows behind a prefix of junk (row_off_dev[0] != 0) and before a tail of it, on both sides; nothing outside the outputs is written"""
    ctx, N, junk, R = tok._ctx, 4, 37, 7
    rng = np.random.default_rng(41)
    ref = reference(rng, [0, 30, 7, 90], N)
    bodies = queries(rng, ref, N, (0, 3, 70, PIECE + 9, 0, 1, 130))
    want = LO.score(LO.train(ref, N), N, bodies)
    assert (want["n_order"].sum(axis=1) > 0).all()

    def up(rows):
        flat = np.array([-77] * junk + [v for b in rows for v in b] + [-88] * 5, dtype=np.int32)
        ro = junk + np.cumsum([0] + [len(b) for b in rows], dtype=np.int64)
        d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
        ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
        return d_ids, d_ro, flat, ro
    r_ids, r_ro, r_flat, _ = up(ref)
    q_ids, q_ro, q_flat, ro = up(bodies)
    g = [Guarded(ctx, R), Guarded(ctx, 2 * R), Guarded(ctx, (N + 1) * R)]                   # (bits_fx: two 32-bit cells a row)
    g_tok = [Guarded(ctx, len(q_flat), dtype=t) for _, t in ctx.LM_TOKEN_OUT]
    lm = ctx.ngram_lm_build_device(r_ids, r_ro, len(ref), 0, 0, N)
    try:
        ctx.h2d(r_ids, np.full(len(r_flat), 3, dtype=np.int32))           # the model owns a copy: the caller's ids may change
        ctx.ngram_lm_score_device(lm, q_ids, q_ro, R, 0, 0, 0.4, *[x.ptr for x in g + g_tok])
        host = ctx.ngram_lm_score(lm, N, q_flat[junk:-5], ro - junk, False, 0.4, True)
        assert np.array_equal(g[0].read(), want["n_tokens"]) and np.array_equal(g[2].read().reshape(N + 1, R), want["n_order"])
        assert np.array_equal(g[1].read().view(np.uint64), host["bits_fx"])      # device against device: exact
        for x, (k, _) in zip(g_tok, ctx.LM_TOKEN_OUT):
            cells = x.read()
            assert (cells[:junk] == x.fill).all() and (cells[int(ro[-1]):] == x.fill).all()       # the junk's cells are nobody's
            assert np.array_equal(cells[junk:int(ro[-1])], want[k]) and np.array_equal(host[k], want[k]), k
    finally:
        ctx.ngram_lm_destroy(lm)
        for x in g + g_tok:
            x.free()
        for d in (r_ids, r_ro, q_ids, q_ro):
            ctx.free(d)


def test_refusals(tok):
    from genz_tokenize import _native
    ctx, lib, P, vp, h, INV = tok._ctx, tok._ctx.lib, _native._ptr, ctypes.c_void_p, tok._ctx.handle, _native.GZ_E_INVALID
    ids, ro = np.arange(10, dtype=np.int32), np.array([0, 4, 10], dtype=np.int64)
    out = vp(0xDEAD)
    for bad_ro, skip, order in ((ro, 0, 0), (ro, 0, 9), (np.array([3, 3, 3], dtype=np.int64), 0, 5), (np.array([0, 1, 2], dtype=np.int64), 1, 5)):
        assert lib.gz_ngram_lm_build(h, P(ids), P(bad_ro), 2, skip, skip, order, ctypes.byref(out)) == INV       # orders outside 1..8; T = 0
    assert lib.gz_ngram_lm_build(h, None, None, 0, 0, 0, 5, ctypes.byref(out)) == INV and out.value == 0xDEAD      # no rows: T = 0
    lm = vp(ctx.ngram_lm_build(ids, ro, 3, False))
    other = _native.Context()
    gone, foreign = vp(other.ngram_lm_build(ids, ro, 3, False)), vp(other.ngram_lm_build(ids, ro, 3, False))
    other.ngram_lm_destroy(gone.value)
    try:
        for model, alpha, c in [(lm, a, h) for a in (0.0, 1.5, float("nan"), 2.0 ** -9)] + [(None, 0.4, h), (foreign, 0.4, h), (gone, 0.4, other.handle)]:
            outs = [np.full(2, FILL, dtype=np.int32), np.full(2, FILL, dtype=np.uint64), np.full(8, FILL, dtype=np.int32), np.full(10, 0x5A, dtype=np.uint8),
                    np.full(10, FILL, dtype=np.uint32), np.full(10, FILL, dtype=np.uint32)]
            canary = [a.copy() for a in outs]
            assert lib.gz_ngram_lm_score(c, model, P(ids), P(ro), 2, 0, 0, alpha, *[P(a) for a in outs]) == INV
            assert all(np.array_equal(a, b) for a, b in zip(outs, canary))
        assert lib.gz_ngram_lm_score(h, lm, None, None, 0, 0, 0, 0.4, None, None, None, None, None, None) == _native.GZ_OK
    finally:
        ctx.ngram_lm_destroy(lm.value)
        other.close()
    check(tok, [[1, 2, 3, 4, 1, 2]], 2, [[1, 2], [9]])                    # the context is usable afterwards


def test_text_end_to_end(tok):
    train = ["the cat sat on the mat", "the dog sat on the log", "a cat and a dog sat on the mat", "the mat is on the log", "a dog is a dog"]
    texts = ["the dog sat on the log", "log the on sat dog the", "zqx vvk jjq qzx kkv", ""]           # a copy, its words shuffled, unseen letters, nothing
    enc = tok.encode_batch(train + texts, max_len=None)
    rows = [enc["input_ids"][enc["row_off"][i]:enc["row_off"][i + 1]].tolist() for i in range(len(train) + len(texts))]
    want = LO.score(LO.train(rows[:5], 3, framed=True), 3, rows[5:], 0.4, framed=True)
    with tok.encode_ngram_lm(train, order=3) as lm:
        got = tok.encode_perplexity(texts, lm)
        same(got, want, keys=("n_tokens", "n_order"))
        ppl = got["perplexity"]
        assert ppl[0] < ppl[1] < ppl[2] < ppl[3] == np.inf
        cut = float((ppl[0] + ppl[1]) / 2)
        flt = tok.perplexity_filter(texts, lm, cut)
        assert flt["keep"].tolist() == [True, False, False, False] and flt["keep"].dtype == bool
        assert tok.perplexity_filter(texts, lm, 1e300)["keep"].tolist() == [True, True, True, False]
        assert tok.perplexity_filter(texts, lm, float(ppl[2]), min_perplexity=cut)["keep"].tolist() == [False, True, True, False]
        dev = tok.perplexity_to_device(texts, lm)
        assert all(np.array_equal(dev[k].numpy(), got[k]) for k in ("n_tokens", "bits_fx", "n_order"))
