"""Modified Kneser-Ney perplexity on the GPU against tests/kn_oracle.py (exact fractions).  Every integer compares exactly: n_tokens,
n_order, token_order, the counts of counts, V and the empty context's A and F.  token_bits_fx is within 1 of the oracle and bits_fx
within n_tokens, a bound that is derived, not measured: p is a sum of non-negative terms built with about 6 roundings an order plus
the discounts' own, so its relative error is far below 2^-40 and the cost is off by far less than the 2^-24 grid step: a position's
grid value differs by at most 1, and only beside a half step.  Device against device is exact."""
import ctypes

import numpy as np
import pytest

import kn_oracle as KO
import lm_oracle as LO
from test_gpu_ngram import FILL, PIECE, Guarded, mixture, reference, tok  # noqa: F401  (tok: the module's Tokenize fixture)

pytestmark = pytest.mark.gpu
KN = dict(smoothing="kneser_ney")


def same(got, want):
    for k in ("n_tokens", "n_order", "token_order", "row_off"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    off = {k: np.abs(got[k].astype(np.int64) - want[k].astype(np.int64)) for k in ("token_bits_fx", "bits_fx")}
    assert got["token_bits_fx"].dtype == np.uint32 and got["bits_fx"].dtype == np.uint64 and (off["token_bits_fx"] <= 1).all() and (off["bits_fx"] <= want["n_tokens"]).all()


def check(tok, ref, N, rows, D=None, framed=False, occur=()):
    """statistics and scores against the oracle, a second score call against the first; every order 0..N and `occur` occur in the ORACLE's output"""
    kn = KO.derive(LO.train(ref, N, framed), N)
    want = KO.score(kn, N, rows, D, framed)
    rule, fallback = KO.discounts(kn["n"])
    seen = want["flags"] | ({"L0"} if kn["L0"] else set()) | ({"computed"} if False in fallback else set()) | ({"fallback"} if True in fallback else set())
    assert (want["n_order"].sum(axis=1) > 0).all() and set(occur) <= seen, (want["n_order"].sum(axis=1), seen)
    with tok.ngram_lm(ref, N, framed=framed) as lm:
        before = tok._ctx.ngram_lm_kn_info(lm._handle)
        assert (before["prepared"], before["V"], before["sidecar_bytes"]) == (False, kn["V"], 0)                  # never prepared: no sidecar
        info = lm.kneser_ney()
        assert (info["prepared"], info["V"], info["A"], list(info["F"])) == (True, kn["V"], kn["ctx"][1][()][0], kn["ctx"][1][()][1:])
        assert np.array_equal(info["counts_of_counts"], kn["n"]) and info["fallback"].tolist() == fallback and info["sidecar_bytes"] >= 20 * tok._ctx.ngram_lm_info(lm._handle)["slots"]
        assert np.allclose(info["discounts"], np.array(rule, dtype=np.float64), rtol=1e-13, atol=0)
        got = tok.perplexity_rows(rows, lm, framed=framed, return_tokens=True, discounts=D, **KN)
        same(got, want)
        again = tok.perplexity_rows(rows, lm, framed=framed, return_tokens=True, discounts=D, **KN)
        assert sorted(again) == sorted(got) and all(np.array_equal(again[k], got[k]) for k in got)
    return want, got, kn


def queries(rng, ref, N, lengths):                                        # copies out of the training bodies between runs over 0..8 (7, 8: never trained)
    return [mixture(rng, ref, max(N, 2), T) for T in lengths]


@pytest.mark.parametrize("N", [1, 2, 5, 8])
def test_body_lengths_at_the_rules_and_the_trips_edges(tok, N):
    """both sides around the order and one trip of 64; 50 only ends a body (a held context with A = 0), 60 only starts one (L = 0)"""
    rng = np.random.default_rng(N + 10)
    lengths = sorted({0, 1, max(N - 1, 0), N, 63, 64, 65})
    ref = reference(rng, lengths, max(N, 2)) + [[3, 1, 50], [60, 3]]
    rows = queries(rng, ref, N, lengths) + [[50, 2, 50, 7], [60, 3, 60], list(ref[-3])]
    want, _, _ = check(tok, ref, N, rows, occur=("A0", "L0", "computed", "fallback") if N > 1 else ())
    assert want["n_tokens"].tolist()[:len(lengths)] == lengths


@pytest.mark.parametrize("N,hi", [(3, 7), (8, 2)])
def test_pieces(tok, N, hi):
    """a body of 4097 and one of five pieces on BOTH sides, a gram planted across, before and behind a piece boundary (N = 8 over two
    ids: few distinct histories for the oracle)"""
    rng = np.random.default_rng(50 + N)
    g = [1, 0, 1, 1, 0, 0, 0, 1][:N]
    planted = (PIECE - N // 2, 2 * PIECE - N, 3 * PIECE, 4 * PIECE - 1)   # across, before, behind, across by one id
    ref = reference(rng, [50, 300], N) + [rng.integers(0, hi, size=T).tolist() for T in (PIECE + 1, 4 * PIECE + 300)]
    rows = [rng.integers(0, hi + 1, size=T).tolist() for T in (PIECE + 1, 4 * PIECE + 300)] + queries(rng, ref[:2], N, [70]) + [[], [7, 8, 1]]
    for body in (ref[-1], rows[1]):
        for p in planted:
            body[p:p + N] = g
    ref[-2][PIECE + 1 - N:] = rows[0][PIECE + 1 - N:] = g                  # (ends on the second piece's only position)
    want, _, _ = check(tok, ref, N, rows)
    ends = np.array([PIECE + 1 - N] + [PIECE + 1 + p for p in planted]) + N - 1
    assert (want["token_order"][ends] == N).all()


@pytest.mark.parametrize("N,ref,rows", [(3, [[v for i in range(350) for v in (5, 100 + i)]], [[5, 100, 5], [5, 7], [449, 5, 200, 5]]),
                                        (5, [[3] * 5000], [[3] * 40, [3] * 3 + [4], [8, 3, 3]])])
def test_hot_cells(tok, N, ref, rows):
    """a context with 350 distinct followers that share their one left neighbour (one A, F_1 and L cell for all); 5 000 equal ids"""
    _, _, kn = check(tok, ref, N, rows)
    assert max(s[1] + s[2] + s[3] for s in kn["ctx"][2].values()) == (350 if N == 3 else 1)


@pytest.mark.parametrize("P", [255, 256, 257])
def test_gram_totals_at_table_sizes(tok, P):
    """gram positions of both orders just below, at and above a power of two: the derivation's lane-a-slot grids"""
    rng = np.random.default_rng(P)
    ref = [rng.integers(0, 7, size=(P + 1) // 2).tolist(), rng.integers(0, 7, size=P // 2 + 1).tolist()]      # m1 + m2 + (m1 - 1) + (m2 - 1) = 2 P
    assert sum(LO.grams(LO.train(ref, 2), 2)[0][1:]) == 2 * P
    check(tok, ref, 2, queries(rng, ref, 2, (0, 2, 50, 130)))


def test_hash_bits_discounts_frames_and_slices(tok):
    """1, 4 and 32 hash bits over 300 distinct grams change nothing; the caller's discounts, D_j = j among them; frames; slices"""
    from genz_tokenize import _native
    N, rng = 4, np.random.default_rng(13)
    ref = reference(rng, [70, 0, 140, 3, 170], N)
    rows = queries(rng, ref, N, (0, 3, 4, 70, 200, 64))
    own = [[1.0, 2.0, 3.0], [0.25, 1.5, 0.125], [0.9, 0.1, 2.75], [0.5, 1.0, 1.5]]
    assert sum(LO.grams(LO.train(ref, N), N)[1][1:]) > 300
    try:
        results = [(_native.debug_set("lm_hash_bits", bits, tok._ctx), check(tok, ref, N, rows)[1])[1] for bits in (0, 1, 4, 32)]
    finally:
        _native.debug_set("lm_hash_bits", 0, tok._ctx)
    assert all(np.array_equal(r[k], results[0][k]) for r in results for k in r)
    want, _, _ = check(tok, ref, N, rows, D=own)
    assert not np.array_equal(want["bits_fx"], results[0]["bits_fx"])
    framed, _, _ = check(tok, [[-7] + b + [-9] for b in ref], N, [[-7] + b + [-9] for b in rows] + [[], [5]], D=own, framed=True)
    assert all(np.array_equal(framed[k][..., :len(rows)], want[k]) for k in ("n_tokens", "n_order", "bits_fx"))
    with tok.ngram_lm(ref, N, framed=False) as lm:
        whole = tok.perplexity_rows(rows, lm, framed=False, **KN)
        for a, b in ((0, 6), (0, 1), (2, 5), (5, 6), (3, 3)):
            part = tok.perplexity_rows(rows[a:b], lm, framed=False, **KN)
            assert all(np.array_equal(part[k], whole[k][..., a:b]) for k in ("n_tokens", "bits_fx", "n_order", "perplexity")), (a, b)


def test_the_ps_of_a_context_sum_to_one_on_the_device(tok):
    """x.w for every seen w and one unseen id at the last position: the sum of 2^(-fx / 2^24) is 1 within (V + 1) 2^-24"""
    N, rng = 3, np.random.default_rng(3)
    ref = reference(rng, [40, 90, 7], N)
    with tok.ngram_lm(ref, N, framed=False) as lm:
        for x in ([], [8], [2, 3], [7, 1], ref[1][4:7], ref[0][-3:], [1, 8, 8]):
            got = tok.perplexity_rows([list(x) + [w] for w in list(range(7)) + [99]], lm, framed=False, return_tokens=True, **KN)
            last = got["token_bits_fx"][got["row_off"][1:] - 1].astype(np.float64)
            assert lm.kneser_ney()["V"] == 7 and abs(np.sum(2.0 ** (-last / 2.0 ** 24)) - 1.0) <= 8 * 2.0 ** -24, x


def test_device_form_behind_junk_and_refusals(tok):
    """rows between junk: the device form equals the host form and writes nothing else; then every C refusal over canary-filled outputs"""
    from genz_tokenize import _native
    ctx, N, junk = tok._ctx, 4, 37
    rng = np.random.default_rng(41)
    ref = reference(rng, [0, 30, 7, 90], N)
    bodies = queries(rng, ref, N, (0, 3, 70, PIECE + 9, 0, 1, 130))
    R, flat = len(bodies), np.array([-77] * junk + [v for b in bodies for v in b] + [-88] * 5, dtype=np.int32)
    ro = junk + np.cumsum([0] + [len(b) for b in bodies], dtype=np.int64)
    d_ids, d_ro = ctx.alloc(flat.nbytes), ctx.alloc(ro.nbytes)
    ctx.h2d(d_ids, flat); ctx.h2d(d_ro, ro)
    g = [Guarded(ctx, R), Guarded(ctx, 2 * R), Guarded(ctx, (N + 1) * R)] + [Guarded(ctx, len(flat), dtype=t) for _, t in ctx.LM_KN_TOKEN_OUT]
    lm = ctx.ngram_lm_build(np.array([v for b in ref for v in b], dtype=np.int32), np.cumsum([0] + [len(b) for b in ref], dtype=np.int64), N, False)
    other = _native.Context()
    foreign = other.ngram_lm_build(np.arange(5, dtype=np.int32), np.array([0, 5], dtype=np.int64), 2, False)
    try:
        ctx.ngram_lm_score_kn_device(lm, d_ids, d_ro, R, 0, 0, None, *[x.ptr for x in g])
        host = ctx.ngram_lm_score_kn(lm, N, flat[junk:-5], ro - junk, False, None, True)
        assert np.array_equal(g[0].read(), host["n_tokens"]) and np.array_equal(g[1].read().view(np.uint64), host["bits_fx"])
        assert np.array_equal(g[2].read().reshape(N + 1, R), host["n_order"]) and (host["n_order"].sum(axis=1) > 0).all()
        for x, (k, _) in zip(g[3:], ctx.LM_KN_TOKEN_OUT):
            cells = x.read()
            assert (cells[:junk] == x.fill).all() and (cells[int(ro[-1]):] == x.fill).all() and np.array_equal(cells[junk:int(ro[-1])], host[k]), k
        P, vp, ok = _native._ptr, ctypes.c_void_p, np.array([[0.5, 1.0, 1.5]] * N)
        ids, r2 = np.arange(10, dtype=np.int32), np.array([0, 4, 10], dtype=np.int64)
        bad = [(ctx.handle, vp(lm), 2, 0, d) for d in (ok * 0, ok * 2.5, ok * np.nan, -ok, np.vstack([ok[:3], [[0.5, 2.0, 3.5]]]))]
        bad += [(ctx.handle, vp(lm), -1, 0, ok), (ctx.handle, vp(lm), 2, 2, ok), (ctx.handle, None, 2, 0, ok), (ctx.handle, vp(foreign), 2, 0, ok), (other.handle, vp(lm), 2, 0, ok)]
        for c, model, n_rows, skip, d in bad:
            outs = [np.full(2, FILL, dtype=np.int32), np.full(2, FILL, dtype=np.uint64), np.full(2 * (N + 1), FILL, dtype=np.int32), np.full(10, 0x5A, dtype=np.uint8),
                    np.full(10, FILL, dtype=np.uint32)]
            canary = [a.copy() for a in outs]
            assert ctx.lib.gz_ngram_lm_score_kn(c, model, P(ids), P(r2), n_rows, skip, skip, P(np.ascontiguousarray(d)), *[P(a) for a in outs]) == _native.GZ_E_INVALID
            assert all(np.array_equal(a, b) for a, b in zip(outs, canary))
        assert ctx.lib.gz_ngram_lm_score_kn(ctx.handle, vp(lm), P(ids), P(r2), 2, 0, 0, None, P(outs[0]), P(outs[1]), None, None, P(outs[0])) == _native.GZ_E_INVALID      # overlap
        assert ctx.lib.gz_ngram_lm_score_kn(ctx.handle, vp(lm), None, None, 0, 0, 0, None, None, None, None, None, None) == _native.GZ_OK
    finally:
        ctx.ngram_lm_destroy(lm)
        other.close()
        [x.free() for x in g]
        ctx.free(d_ids); ctx.free(d_ro)


def test_text_end_to_end(tok):
    train = ["the cat sat on the mat", "the dog sat on the log", "a cat and a dog sat on the mat", "the mat is on the log", "a dog is a dog"]
    texts = ["the dog sat on the log", "log the on sat dog the", "zqx vvk jjq qzx kkv", ""]           # a copy, its words shuffled, unseen letters, nothing
    enc = tok.encode_batch(train + texts, max_len=None)
    rows = [enc["input_ids"][enc["row_off"][i]:enc["row_off"][i + 1]].tolist() for i in range(len(train) + len(texts))]
    want = KO.score(KO.derive(LO.train(rows[:5], 3, framed=True), 3), 3, rows[5:], framed=True)
    with tok.encode_ngram_lm(train, order=3) as lm:
        got = tok.encode_perplexity(texts, lm, **KN)
        assert all(np.array_equal(got[k], want[k]) for k in ("n_tokens", "n_order")) and (np.abs(got["bits_fx"].astype(np.int64) - want["bits_fx"].astype(np.int64)) <= want["n_tokens"]).all()
        ppl = got["perplexity"]
        assert ppl[0] < ppl[1] < ppl[2] < ppl[3] == np.inf and not np.array_equal(got["bits_fx"], tok.encode_perplexity(texts, lm)["bits_fx"])
        assert tok.perplexity_filter(texts, lm, float((ppl[0] + ppl[1]) / 2), **KN)["keep"].tolist() == [True, False, False, False]
        dev = tok.perplexity_to_device(texts, lm, **KN)
        assert all(np.array_equal(dev[k].numpy(), got[k]) for k in ("n_tokens", "bits_fx", "n_order"))
