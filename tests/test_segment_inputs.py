"""CPU-only: the segmentation oracle against answers written out by hand, the fold map against `str.lower()`, and the costs
`Lexicon.from_words` derives from counts against the formula."""
import math

import pytest

import segment_oracle as SO


@pytest.mark.parametrize("doc,lex,K,unk,want,stats", [
    ("sinh viên công nghệ", {"sinh_viên": 1, "công_nghệ": 1, "viên": 1}, 2, 1, "sinh_viên công_nghệ", [4, 2, 2, 2]),
    # equal minima: a_b + c and a + b_c both cost 2; the largest LAST word wins
    ("a b c", {"a_b": 1, "b_c": 1, "a": 1, "c": 1}, 2, 1, "a b_c", [3, 2, 2, 2]),
    # leftmost-longest takes a_b, then pays for c and d apart (cost 1 + 5 + 5); the best path is a + b_c_d (2 + 1)
    ("a b c d", {"a_b": 1, "b_c_d": 1, "a": 2}, 3, 5, "a b_c_d", [4, 2, 2, 3]),
    ("(Hà Nội), ... 3.5 x_y", {"hà_nội": 1, "x_y": 1}, 2, 7, "( Hà_Nội ) , . . . 3.5 x_y", [10, 9, 2, 51]),     # 7 unknown words at 7, 2 entries at 1
    ("  ", {"a": 1}, 1, 1, "", [0, 0, 0, 0]),
])
def test_oracle_against_hand_answers(doc, lex, K, unk, want, stats):
    text, st, join = SO.segment(doc, lex, K, unk)
    assert (text, st) == (want, stats) and sum(join) == st[0] - st[1]


def test_dynamic_programme_beats_leftmost_longest():
    lex = {"a_b": 1, "b_c_d": 1, "a": 2}
    greedy, gcost = SO.leftmost_longest("a b c d", lex, 3, 5)
    text, st, _ = SO.segment("a b c d", lex, 3, 5)
    assert (greedy, gcost) == ("a_b c d", 11) and (text, st[3]) == ("a b_c_d", 3)


def test_fold_map_is_str_lower_on_its_code_points_and_keeps_the_length():
    from genz_tokenize.segment import FOLD_MAP, fold_case
    assert set(FOLD_MAP) == SO.FOLDED and len(FOLD_MAP) == 26 + 30 + 6 + 45
    for c, v in FOLD_MAP.items():
        assert chr(c).lower() == chr(v) and len(chr(c).encode()) == len(chr(v).encode()), hex(c)
    assert fold_case("ĐẠI HỌC × İ Ω") == "đại học × İ Ω" == SO.fold("ĐẠI HỌC × İ Ω")       # (outside the map: left alone)


@pytest.mark.parametrize("count", [0, 1, 90])
def test_costs_from_counts_follow_the_formula(count):
    from genz_tokenize.segment import cost_of_count
    total, V = 90, 3
    want = min(max(round(65536 * (math.log2(total + V) - math.log2(count + 1))), 1), 2 ** 24 - 1)
    assert cost_of_count(count, total, V) == want
    assert cost_of_count(0, 2 ** 62, 1) == 62 * 65536 and cost_of_count(10 ** 6, 10, 1) == 1       # (a count above the total clips at 1)
