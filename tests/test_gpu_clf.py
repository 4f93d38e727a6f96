"""Hashed n-gram class models on the GPU against tests/clf_oracle.py.  Counts, totals, n_features and best compare exactly.  Weights
compare with abs(device - oracle) <= 1, a bound that is derived, not measured: a float64 log2 of a value below 2^49 is within a few
ulp, below 2^-45 absolute, which is 2^-21 of a grid step.  bits_fx compares EXACTLY against the numpy sum of the DEVICE's weight table
gathered at the ORACLE's buckets.  best is compared on the rows whose two smallest oracle sums differ by more than 2 n_features (a
weight off by one a feature cannot turn them); that they are nine tenths of a case is asserted on the oracle's output first."""
import ctypes

import numpy as np
import pytest

import clf_oracle as CO
from test_gpu_ngram import FILL, PIECE, Guarded, mixture, reference, tok  # noqa: F401  (tok: the module's Tokenize fixture)

pytestmark = pytest.mark.gpu
LDS_BYTES = 128 << 10                                                     # csrc/gz_kernels.h: GZ_CLF_LDS_BYTES, of gz_clf.inc's two LDS paths


def labels_of(ref, C):
    return [r % max(C - 1, 1) for r in range(len(ref))]                   # class C - 1 (of more than one) has no rows at all


def scored(tok, clf, want, rows, N, framed=False):
    """a score call against the oracle's buckets and the device's own weights"""
    dw = clf.weights().astype(np.int64)
    got = tok.class_bits_rows(rows, clf, framed=framed)
    assert got["n_features"].dtype == np.int32 and np.array_equal(got["n_features"], want["n_features"])
    sums = np.stack([dw[b].sum(axis=0) if len(b) else np.zeros(dw.shape[1], np.int64) for b in want["buckets"]], axis=1)
    assert got["bits_fx"].dtype == np.int64 and np.array_equal(got["bits_fx"], sums), np.argwhere(got["bits_fx"] != sums)[:4].tolist()
    ok = CO.decided(want)
    assert np.array_equal(got["best"][ok], want["best"][ok]) and np.array_equal(got["bits"], got["bits_fx"] / 2.0 ** 24)
    return got


def check(tok, N, C, bits, ref, rows, labels=None, framed=False, a=1.0):
    labels = labels_of(ref, C) if labels is None else labels
    count, grams = CO.fit(ref, labels, N, bits, C, framed)
    w = CO.weights(count, a)
    want = CO.score(w, N, bits, rows, framed)
    assert CO.decided(want).mean() >= 0.9 and count.sum() > 0            # asserted on the ORACLE's output, before any device call
    with tok.ngram_classifier(C, order=N, bits=bits, smoothing=a) as clf:
        clf.fit_rows(ref, labels, framed=framed)
        assert (clf.order, clf.bits, clf.n_classes, clf.n_rows, clf.n_features) == (N, bits, C, len(ref), count.sum())
        assert np.array_equal(clf.counts(), count) and clf.totals.tolist() == count.sum(axis=0).tolist()
        dw = clf.weights()
        assert dw.dtype == np.int32 and np.abs(dw - w).max() <= 1 and dw.min() >= 0 and dw.max() <= 2 ** 30
        got = scored(tok, clf, want, rows, N, framed)
    return want, got, count, grams


@pytest.mark.parametrize("N,C,bits", [(1, 1, 8), (2, 2, 14), (4, 3, 10), (4, 8, 8)])
def test_rule_at_the_trip_edges(tok, N, C, bits):
    """nothing, one id, around the order; around one and two trips of 64 positions (the carried predecessor ids) -- on both sides"""
    rng = np.random.default_rng(N + C)
    lengths = sorted({0, 1, max(N - 1, 0), N, N + 1, 63, 64, 65, 64 + N - 2, 64 + N - 1, 64 + N, 127, 128, 129})
    ref = reference(rng, lengths, max(N, 2))
    rows = [mixture(rng, ref, max(N, 2), T) for T in lengths] + [list(b) for b in ref[-3:]] + [list(range(1000, 1600, 3))]
    want, _, _, grams = check(tok, N, C, bits, ref + [list(range(1000, 1600))], rows)      # (600 ids: more unigrams than 2^8 buckets)
    assert want["n_features"].tolist()[:len(lengths)] == [sum(max(T - k + 1, 0) for k in range(1, N + 1)) for T in lengths]
    assert bits != 8 or max(len(g) for g in grams.values()) > 1           # buckets that hold several distinct grams


@pytest.mark.parametrize("N", [2, 4])
def test_pieces(tok, N):
    """one below, at and above one piece and a body of five pieces, on BOTH sides, one gram planted across, before and behind a piece
    boundary; long rows of different classes between short ones: the class-ordered piece list"""
    rng = np.random.default_rng(50 + N)
    g = [3, 1, 4, 1][:N]
    planted = (PIECE - N // 2, 2 * PIECE - N, 3 * PIECE, 4 * PIECE - 1)   # across, before, behind, across by one id
    ref = reference(rng, [50, PIECE - 1, 300, 4 * PIECE + 300, 7, PIECE, PIECE + 1, 4 * PIECE + 300], N)
    labels = [0, 1, 2, 0, 1, 2, 0, 1]
    long = mixture(rng, ref, N, 4 * PIECE + 300)
    for p in planted:
        ref[3][p:p + N] = ref[7][p:p + N] = long[p:p + N] = g
    rows = [mixture(rng, ref, N, T) for T in (PIECE - 1, 20, PIECE, PIECE + 1)] + [long, [], [7, 8, 1]]
    _, got, count, _ = check(tok, N, 3, 12, ref, rows, labels)
    assert (count[CO.features(g, N, 12)[-1][0]][:2] >= 4).all()           # the planted gram's bucket, in both long rows' classes


HOT = [[3] * 5000]


@pytest.mark.parametrize("N,C,bits,fit_lds,score_lds", [(2, 1, 15, True, True), (2, 1, 16, False, False), (2, 4, 13, True, True), (2, 5, 13, True, False)])
def test_lds_edges_and_the_switch(tok, N, C, bits, fit_lds, score_lds):
    """the fit's histogram at the largest B that fits LDS and the smallest that does not; the score's table at the largest (bits, C)
    that fits and the smallest that does not; each with clf_lds 1 and 0: not a bit differs.  One row of 5000 equal ids: one hot bin"""
    from genz_tokenize import _native
    assert (4 << bits <= LDS_BYTES, 4 * _native.Context.CLF_CP[C] << bits <= LDS_BYTES) == (fit_lds, score_lds)
    rng = np.random.default_rng(bits + C)
    ref = HOT + reference(rng, [70, 0, 140, 3, 170, 900], N)
    rows = [mixture(rng, ref[1:], N, T) for T in (0, 3, 70, 200, 64)] + [[3] * 40]
    results = []
    try:
        for v in (1, 0):
            _native.debug_set("clf_lds", v, tok._ctx)
            with tok.ngram_classifier(C, order=N, bits=bits) as clf:
                info = tok._ctx.ngram_clf_info(clf._handle)
                assert (info["fit_lds"], info["score_lds"], info["lds_bytes"]) == (bool(v) and fit_lds, bool(v) and score_lds, LDS_BYTES)
            _, got, count, _ = check(tok, N, C, bits, ref, rows)
            results.append((got, count))
    finally:
        _native.debug_set("clf_lds", 1, tok._ctx)                         # (the default)
    assert all(np.array_equal(results[0][0][k], results[1][0][k]) for k in results[0][0])
    one, two = CO.features([3, 3], 2, bits)[1][0], CO.features([3, 3], 2, bits)[2][0]
    assert results[0][1][one, 0] >= 5000 and results[0][1][two, 0] >= 4999      # (`check` compared every count with the oracle's)


def test_adding_up(tok):
    """one fit; three fits of the rows permuted; two shard models summed on the host and uploaded: the same counts.  Slices of the
    query rows and single rows equal the whole"""
    N, C, bits = 3, 2, 10
    rng = np.random.default_rng(12)
    ref = reference(rng, [30, 100, 200, 0, 5, PIECE + 40, 64], N)
    labels = [0, 1, 0, 1, 1, 0, 1]
    rows = [mixture(rng, ref, N, int(T)) for T in rng.integers(0, 150, size=40)] + [mixture(rng, ref, N, PIECE + 300)]
    want, whole, count, _ = check(tok, N, C, bits, ref, rows, labels)
    perm = rng.permutation(len(ref)).tolist()
    with tok.ngram_classifier(C, order=N, bits=bits) as a, tok.ngram_classifier(C, order=N, bits=bits) as b, tok.ngram_classifier(C, order=N, bits=bits) as s:
        for part in (perm[:2], perm[2:3], perm[3:]):
            a.fit_rows([ref[i] for i in part], [labels[i] for i in part], framed=False)
        b.fit_rows(ref[:3], labels[:3], framed=False)
        s.fit_rows(ref[3:], labels[3:], framed=False)
        assert np.array_equal(a.counts(), count) and a.n_rows == len(ref)
        b.set_counts(b.counts().astype(np.int64) + s.counts())
        assert np.array_equal(b.counts(), count) and b.totals.tolist() == count.sum(axis=0).tolist() and b.n_features == count.sum()
        for clf in (a, b):
            scored(tok, clf, want, rows, N)
        for lo, hi in ((0, 41), (0, 1), (17, 40), (40, 41), (5, 5)):
            part = tok.class_bits_rows(rows[lo:hi], a, framed=False)
            assert all(np.array_equal(part[k], whole[k][..., lo:hi]) for k in whole), (lo, hi)
        assert [tok.class_bits_rows([r], a, framed=False)["bits_fx"][1, 0] for r in rows[35:]] == whole["bits_fx"][1, 35:].tolist()


@pytest.mark.parametrize("R", [1, 255, 256, 257])
def test_row_counts_at_block_edges(tok, R):
    rng = np.random.default_rng(100 + R)
    ref = [rng.integers(0, 7, size=int(T)).tolist() for T in rng.integers(0, 12, size=R)] + reference(rng, [40, 60, 5], 3)
    want, _, _, _ = check(tok, 3, 3, 9, ref, [mixture(rng, ref, 3, int(T)) for T in [60] + rng.integers(0, 40, size=R - 1).tolist()])
    assert want["bits_fx"].shape == (3, R)


def test_framed_against_bare_bodies(tok):
    rng = np.random.default_rng(31)
    ref = reference(rng, [0, 1, 3, 4, 5, 70], 4)
    bodies = [mixture(rng, ref, 4, T) for T in (0, 1, 3, 4, 5, 70, 130)]
    _, bare, count, _ = check(tok, 4, 2, 11, ref, bodies)
    framed = [[-7] + b + [-9] for b in bodies] + [[], [5]]                # the frame is dropped whatever it holds; rows shorter than it
    _, got, count2, _ = check(tok, 4, 2, 11, [[-7] + b + [-9] for b in ref], framed, framed=True)
    assert np.array_equal(count, count2) and all(np.array_equal(got[k][..., :len(bodies)], bare[k]) for k in bare)


def test_device_form_behind_junk(tok):
    """rows behind a prefix of junk (row_off_dev[0] != 0) and before a tail of it, on both sides; every output left out in turn;
    nothing outside the outputs is written"""
    ctx, N, C, bits, junk = tok._ctx, 3, 3, 9, 37
    rng = np.random.default_rng(41)
    ref = reference(rng, [0, 30, 7, 90, PIECE + 5], N)
    labels = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    bodies = [mixture(rng, ref, N, T) for T in (0, 3, 70, PIECE + 9, 0, 1, 130)]
    R = len(bodies)
    count, _ = CO.fit(ref, labels, N, bits, C)
    want = CO.score(CO.weights(count), N, bits, bodies)
    bufs = []

    def up(a):
        bufs.append(ctx.alloc(a.nbytes))
        ctx.h2d(bufs[-1], a)
        return bufs[-1]

    def rows_up(rows):
        flat = np.array([-77] * junk + [v for b in rows for v in b] + [-88] * 5, dtype=np.int32)
        return up(flat), up(junk + np.cumsum([0] + [len(b) for b in rows], dtype=np.int64))
    r_ids, r_ro = rows_up(ref)
    q_ids, q_ro = rows_up(bodies)
    clf = ctx.ngram_clf_create(N, bits, C, 1.0)
    guards = []
    try:
        ctx.ngram_clf_fit_device(clf, r_ids, r_ro, up(labels), len(ref), 0, 0)
        assert np.array_equal(ctx.ngram_clf_counts(clf, bits, C), count)
        host = ctx.ngram_clf_score(clf, C, np.array([v for b in bodies for v in b], dtype=np.int32), np.cumsum([0] + [len(b) for b in bodies]), False)
        for out in (None, 0, 1, 2):                                       # all three outputs, then each left out in turn
            g = [Guarded(ctx, R), Guarded(ctx, 2 * C * R), Guarded(ctx, R)]                     # (bits_fx: two 32-bit cells a sum)
            guards += g
            ctx.ngram_clf_score_device(clf, q_ids, q_ro, R, 0, 0, *[0 if k == out else x.ptr for k, x in enumerate(g)])
            for k, (x, key) in enumerate(zip(g, ("n_features", "bits_fx", "best"))):
                assert x.untouched() if k == out else np.array_equal(x.read().view(host[key].dtype).reshape(host[key].shape), host[key]), (out, key)
        assert np.array_equal(host["n_features"], want["n_features"])
    finally:
        ctx.ngram_clf_destroy(clf)
        for x in guards:
            x.free()
        for d in bufs:
            ctx.free(d)


def test_refusals(tok):
    from genz_tokenize import NgramClassifier, _native
    ctx, lib, P, vp, h, INV = tok._ctx, tok._ctx.lib, _native._ptr, ctypes.c_void_p, tok._ctx.handle, _native.GZ_E_INVALID
    ids, ro, lab = np.arange(10, dtype=np.int32), np.array([0, 4, 10], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    out = vp(0xDEAD)
    for order, bits, C, a in ((0, 14, 2, 1.0), (5, 14, 2, 1.0), (2, 7, 2, 1.0), (2, 23, 2, 1.0), (2, 14, 0, 1.0), (2, 14, 9, 1.0), (2, 14, 2, 0.0),
                              (2, 14, 2, float("nan")), (2, 14, 2, 2.0 ** 17)):
        assert lib.gz_ngram_clf_create(h, order, bits, C, a, ctypes.byref(out)) == INV and out.value == 0xDEAD
    other = _native.Context()
    clf, gone, foreign = vp(ctx.ngram_clf_create(2, 8, 2, 1.0)), vp(other.ngram_clf_create(2, 8, 2, 1.0)), vp(other.ngram_clf_create(2, 8, 2, 1.0))
    other.ngram_clf_destroy(gone.value)
    given = NgramClassifier.from_weights(tok, np.arange(-256, 256, dtype=np.int64).reshape(256, 2) * 1000, 2)
    try:
        bad = [(clf, ro, np.array([0, 2], dtype=np.int32), h), (clf, ro, np.array([-1, 0], dtype=np.int32), h), (clf, np.array([0, 5, 4], dtype=np.int64), lab, h),
               (vp(given._handle), ro, lab, h), (None, ro, lab, h), (foreign, ro, lab, h), (gone, ro, lab, other.handle)]
        for model, offs, labels, c in bad:
            assert lib.gz_ngram_clf_fit(c, model, P(ids), P(offs), P(labels), 2, 0, 0) == INV
        assert lib.gz_ngram_clf_fit(h, clf, P(ids), P(ro), P(lab), 2, 2, 0) == INV and ctx.ngram_clf_info(clf.value)["n_features"] == 0
        assert not ctx.ngram_clf_counts(clf.value, 8, 2).any()            # every refused fit left the model as it was
        for model, offs, c in [(m, ro, c) for m, _, _, c in bad[4:]] + [(clf, np.array([0, 5, 4], dtype=np.int64), h)]:
            outs = [np.full(2, FILL, dtype=np.int32), np.full(4, FILL, dtype=np.int64), np.full(2, FILL, dtype=np.int32)]
            assert lib.gz_ngram_clf_score(c, model, P(ids), P(offs), 2, 0, 0, *[P(a) for a in outs]) == INV
            assert all((a == a.dtype.type(FILL)).all() for a in outs)
        assert lib.gz_ngram_clf_score(h, clf, None, None, 0, 0, 0, None, None, None) == _native.GZ_OK
        rows = [[1, 2, 3], [], [9]]                                       # negative weights, scored exactly; a model without fitted rows scores too
        w = given.weights().astype(np.int64)
        want = CO.score(w, 2, 8, rows)
        got = tok.class_bits_rows(rows, given, framed=False)
        assert w.min() < 0 and all(np.array_equal(got[k], want[k]) for k in ("n_features", "bits_fx", "best"))
        empty = ctx.ngram_clf_score(clf.value, 2, np.array([1, 2, 3], dtype=np.int32), np.array([0, 3]), False)
        assert empty["bits_fx"].tolist() == [[5 * 8 * 2 ** 24]] * 2 and empty["best"].tolist() == [0]      # log2(0 + 256) - log2(0 + 1) a feature
    finally:
        given.close()
        ctx.ngram_clf_destroy(clf.value)
        other.close()
    check(tok, 2, 2, 8, [[1, 2, 3, 4, 1, 2], [5, 5, 6]], [[1, 2], [9], [5, 6, 5]], [0, 1])      # the context is usable afterwards


def test_text_end_to_end(tok):
    raw = ["buy cheap pills now click here", "click here to win a free prize now", "cheap cheap pills buy now", "win win win click"]
    target = ["the cat sat on the mat", "the dog sat on the log", "a cat and a dog sat on the mat", "the mat is on the log"]
    texts = ["the dog sat on the mat", "click here buy cheap pills", "zqx vvk jjq qzx kkv", ""]      # target-like, raw-like, unseen letters, nothing
    with tok.ngram_classifier(2, order=2, bits=12) as clf:
        clf.fit(raw + target, [0] * 4 + [1] * 4)
        enc = tok.encode_batch(raw + target + texts, max_len=None)
        rows = [enc["input_ids"][enc["row_off"][i]:enc["row_off"][i + 1]].tolist() for i in range(12)]
        count, _ = CO.fit(rows[:8], [0] * 4 + [1] * 4, 2, 12, 2, framed=True)
        assert np.array_equal(clf.counts(), count) and clf.n_rows == 8
        got = tok.importance_weights(texts, clf)
        assert np.array_equal(got["n_features"], CO.score(CO.weights(count), 2, 12, rows[8:], framed=True)["n_features"])
        lw = got["log_weight_per_feature"]
        assert lw[0] > lw[1] and lw[0] > lw[2] and lw[0] > 0 > lw[1] and got["log_weight"][3] == 0 and got["best"].tolist()[:2] + [got["best"][3]] == [1, 0, -1]
        assert np.array_equal(got["log_weight"], got["bits"][0] - got["bits"][1])
        flt = tok.classifier_filter(texts, clf)
        assert flt["keep"].dtype == bool and flt["keep"].tolist() == [bool(lw[i] >= 0) and i != 3 for i in range(4)] and flt["keep"].tolist()[:2] == [True, False]
        assert tok.classifier_filter(texts, clf, min_log_weight=-1e9, per_feature=False)["keep"].tolist() == [True, True, True, False]
        dev = tok.class_bits_to_device(texts, clf)
        assert all(np.array_equal(dev[k].numpy(), got[k]) for k in ("n_features", "bits_fx", "best"))
