"""CPU-only: the modified Kneser-Ney calls are declared, documented, exported and bound on every layer; the Python refusals come before
any native call; tests/kn_oracle.py agrees with the cases its docstring works by hand and its p sum to one exactly; and the new rules
of csrc/gz_rowrules.h hold in a stand-alone program under ASan + UBSan.  Nothing is computed on a GPU here (tests/test_gpu_lm_kn.py)."""
from fractions import Fraction

import numpy as np
import pytest

import kn_oracle as KO
import lm_oracle as LO
import test_lm_surface as S

NAMES = {"gz_ngram_lm_kn_prepare": 2, "gz_ngram_lm_kn_info": 2, "gz_ngram_lm_kn_discounts": 2, "gz_ngram_lm_score_kn": 13, "gz_ngram_lm_score_kn_device": 13}


def test_symbols_declared_documented_exported_and_bound(monkeypatch):
    monkeypatch.setattr(S, "NAMES", NAMES)                               # (the same checks, over the new names)
    S.test_symbols_declared_documented_exported_and_bound()
    assert callable(__import__("genz_tokenize").NgramLM.kneser_ney)


def test_python_refusals_come_before_any_native_call():
    from genz_tokenize import tokenize
    t, live = tokenize.Tokenize.__new__(tokenize.Tokenize), tokenize.NgramLM.__new__(tokenize.NgramLM)
    live._handle, live._ctx, live._info, t._ctx = 1, None, {"order": 2}, None       # no context: a native call would raise AttributeError
    ok = [[0.5, 1.0, 1.5]] * 2
    bad = [dict(smoothing="kn"), dict(smoothing=None), dict(discounts=ok), dict(smoothing="stupid_backoff", discounts=ok)]
    bad += [dict(smoothing="kneser_ney", discounts=d) for d in (ok[:1], [0.5, 1.0, 1.5], [[0.5, 1.0]] * 2, [[0.0, 1.0, 1.5]] * 2, [[0.5, 2.5, 1.5]] * 2,
                                                                 [[0.5, 1.0, float("nan")]] * 2, [[-0.5, 1.0, 1.5]] * 2)]
    for kw in bad:
        for call in (lambda: t.perplexity_rows([[1]], live, **kw), lambda: t.encode_perplexity(["a"], live, **kw),
                     lambda: t.perplexity_to_device(["a"], live, **kw), lambda: t.perplexity_filter(["a"], live, 10.0, **kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(TypeError):
        t.perplexity_rows([[1]], live, 0.4, True, False, "kneser_ney")    # keyword-only


def test_oracle_agrees_with_the_cases_worked_by_hand():
    kn = KO.derive(LO.train([[1, 2, 1, 2, 3], [2]], 2), 2)
    assert (kn["V"], kn["ctx"][1][()], kn["ctx"][2], kn["n"].tolist()) == (3, [3, 3, 0, 0], {(1,): [2, 0, 1, 0], (2,): [2, 2, 0, 0]}, [[3, 0, 0, 0], [2, 1, 0, 0]])
    D, fallback = KO.discounts(kn["n"])
    assert D == [KO.FALLBACK] * 2 and fallback == [True, True] and not kn["L0"]
    assert [KO.prob(kn, D, 2, c, w) for c, w in (([], 1), ([1], 2))] == [(1, Fraction(7, 24)), (2, Fraction(31, 48))]
    flags = set()
    assert [KO.prob(kn, D, 2, c, w, flags) for c, w in (([3], 1), ([3, 1], 9))] == [(1, Fraction(7, 24)), (0, Fraction(1, 16))] and flags == {"A0"}
    a = KO.score(kn, 2, [[1, 2], [3, 1, 9], []])
    f = KO.fx_of
    assert a["token_bits_fx"].tolist() == [f(Fraction(7, 24)), f(Fraction(31, 48)), f(Fraction(7, 24)), f(Fraction(7, 24)), 4 << 24]
    assert a["n_order"].T.tolist() == [[0, 1, 1], [1, 2, 0], [0, 0, 0]] and a["bits_fx"][1] == a["token_bits_fx"][2:].sum() and a["n_tokens"].tolist() == [2, 3, 0]
    assert KO.discounts([[8, 4, 2, 1]]) == ([(Fraction(1, 2), Fraction(5, 4), Fraction(2))], [False]) and KO.discounts([[1, 1, 3, 1]])[1] == [True]


@pytest.mark.parametrize("N,R,own", [(1, 40, False), (2, 8, False), (5, 40, False), (5, 40, True)])
def test_the_ps_of_a_context_sum_to_one_exactly(N, R, own):
    """over the V seen tokens and one unseen token, behind seen, unseen and empty contexts; computed and fallback discounts both occur"""
    rng = np.random.default_rng(N)
    ref = [rng.integers(0, 7, size=int(T)).tolist() for T in rng.integers(0, 60, size=R)]
    kn = KO.derive(LO.train(ref, N), N)
    D, fallback = KO.discounts(kn["n"])
    assert N == 1 or (True in fallback and False in fallback)
    D = [[Fraction(1, 3), Fraction(2), Fraction(5, 2)]] * N if own else D
    for _ in range(30):
        c = rng.integers(0, 9, size=int(rng.integers(0, N + 2))).tolist()
        assert sum(KO.prob(kn, D, N, c, w)[1] for w in list(range(7)) + [99]) == 1 and kn["V"] == 7


MAIN = S.MAIN[:S.MAIN.index("int main()")] + r"""
int main()
{
    const char* disc = "perplexity needs discounts D[k][j] in (0, j]";
    double D[6] = {0.5, 1.0, 1.5, 1.0, 2.0, 3.0};
    OK(is(lm_kn_score_fault(5, 1, 1, nullptr, 8), 0)); OK(is(lm_kn_score_fault(0, 0, 0, D, 2), 0)); OK(is(lm_kn_score_fault(INT64_MAX, 1, 0, D, 1), 0));
    OK(is(lm_kn_score_fault(-1, 0, 0, D, 2), "perplexity needs n_rows >= 0")); OK(is(lm_kn_score_fault(1, 0, 2, D, 2), "perplexity needs skips of 0 or 1"));
    D[4] = std::nextafter(2.0, 3.0); OK(is(lm_kn_score_fault(1, 0, 0, D, 2), disc)); OK(is(lm_kn_score_fault(1, 0, 0, D, 1), 0));
    D[4] = 2.0; D[0] = 0.0; OK(is(lm_kn_score_fault(1, 0, 0, D, 2), disc)); D[0] = std::nan(""); OK(is(lm_kn_score_fault(1, 0, 0, D, 1), disc));
    D[0] = -0.5; OK(is(lm_kn_score_fault(1, 0, 0, D, 2), disc)); D[0] = 5e-324; OK(is(lm_kn_score_fault(1, 0, 0, D, 2), 0));
    const int64_t a[4] = {8, 4, 2, 1}, b[4] = {3, 0, 0, 0}, c[4] = {1, 1, 3, 1}, d[4] = {3, 1, 1, 3}, e[4] = {4, 1, 1, 0};
    const int64_t big[4] = {(int64_t)1 << 32, (int64_t)1 << 32, (int64_t)1 << 32, (int64_t)1 << 32};
    OK(!lm_kn_discounts(a, D) && D[0] == 0.5 && D[1] == 1.25 && D[2] == 2.0);             // Y = 1/2
    OK(lm_kn_discounts(b, D) && D[0] == 0.5 && D[1] == 1.0 && D[2] == 1.5);               // a zero count
    OK(lm_kn_discounts(c, D)); OK(lm_kn_discounts(d, D)); OK(lm_kn_discounts(e, D));    // D_2 = 2 - 9 * (1/3) < 0; D_3 = 3 - 12 * (3/5) < 0; n4 = 0
    OK(!lm_kn_discounts(big, D) && D[0] > 0.333 && D[0] < 0.334 && D[1] == 1.0 && D[2] > 1.66 && D[2] < 1.67);      // (products above 2^64)
    return bad != 0;
}
"""


def test_kn_rules_alone_under_asan_and_ubsan(tmp_path, monkeypatch):
    monkeypatch.setattr(S, "MAIN", MAIN)
    S.test_lm_rules_alone_under_asan_and_ubsan(tmp_path)
