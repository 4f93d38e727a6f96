"""CPU-only: the pair window rule of tests/pairwin_oracle.py against the reference's restatement (oracle/gz_oracle.py) on the bundled
tables, a table worked by hand, the case lists of the GPU tests against the edges they are named for, every refusal of the Python
layer before any native call, and pair_window_spans (host numpy) against its law.  The four laws that tie the rule to the reference:
  1. a pair with T >= 1, Tq <= mq and q + 4 + T <= L has one window whose row and mask are Tokenize.__call__(question, context,
     max_len=L)'s; its type row is the reference's token_type_ids where n_real < L, and where n_real == L the reference's last cell
     holds the eos id (its token-type row is cut like a row of ids) while the rule's holds 1 -- the ONE deviation, asserted both ways;
  2. chunk_0 ++ chunk_1[s:] ++ ... is the context body, and every later window adds a token;
  3. columns 1 .. q of every window are Q[:q];
  4. an answer of at most s + 1 tokens is held by a window, one longer than room by none, and a held answer is
     row[start_pos : end_pos + 1]."""
import random

import numpy as np
import pytest

import pairwin_oracle as P

SP = dict(bos=-1, eos=-2, pad=-3)


@pytest.fixture(scope="module")
def encoded(oracle_tables):
    """(questions, contexts, question bodies, context bodies) over the bundled tables"""
    import gz_oracle as O
    qs, cs = P.texts(120, 0, 9, 21), P.texts(120, 0, 40, 22)
    cs[5] = ""
    return qs, cs, [O.encode(x, oracle_tables)[1:-1] for x in qs], [O.encode(x, oracle_tables)[1:-1] for x in cs]


def test_texts_cover_empty_short_and_long(encoded):
    _, _, qb, cb = encoded
    assert min(map(len, qb)) == 0 and max(map(len, qb)) >= 9 and min(map(len, cb)) == 0 and max(map(len, cb)) > 60


def test_law_1_one_window_is_the_reference_pair_row(encoded, oracle_tables):
    import gz_oracle as O
    t = oracle_tables
    sp = dict(bos=t.bos_id, eos=t.eos_id, pad=t.pad_id)
    seen = {"below": 0, "full": 0}
    for question, context, Q, body in zip(*encoded):
        if not body:
            continue                                                  # T == 0: the reference leaves None cells, outside the law
        for extra in (0, 1, 3):                                       # n_real == L, and n_real < L
            L = len(Q) + 4 + len(body) + extra
            want = O.call(t, question, context, L, True, True)
            for s, mq in ((0, L - 5), (L - 5 - len(Q), len(Q))):
                ws = P.windows(Q, body, L, s, mq, **sp)
                assert len(ws) == 1
                w = ws[0]
                assert w["row"] == want["input_ids"] and w["mask"] == want["attention_mask"], (question, context)
                assert w["n_real"] == L - extra and w["q_len"] == len(Q) and w["start"] == 0
                if extra:
                    assert w["type"] == want["token_type_ids"]
                    seen["below"] += 1
                else:
                    assert w["type"][:-1] == want["token_type_ids"][:-1]
                    assert want["token_type_ids"][-1] == t.eos_id and w["type"][-1] == 1      # the one deviation
                    seen["full"] += 1
    assert seen["below"] > 100 and seen["full"] > 50


LSM = [(5, 0, 0), (8, 1, 1), (8, 0, 3), (9, 4, 0), (12, 3, 2), (16, 3, 3), (16, 11, 0), (16, 0, 11), (33, 10, 5)]


@pytest.mark.parametrize("L,s,mq", LSM)
def test_laws_2_and_3_chunks_rejoin_behind_the_question(encoded, L, s, mq):
    _, _, qb, cb = encoded
    for Q, body in zip(qb, cb):
        q, room, step = P.geometry(len(Q), L, s, mq)
        assert room >= s + 1 and step >= 1
        ws = P.windows(Q, body, L, s, mq, **SP)
        joined = []
        for j, w in enumerate(ws):
            row, n_real = w["row"], w["n_real"]
            n = n_real - q - 4
            assert len(row) == L == len(w["mask"]) == len(w["type"]) and w["q_len"] == q and w["start"] == j * step
            assert row[0] == SP["bos"] and row[1:q + 1] == Q[:q]                                  # law 3
            assert row[q + 1:q + 3] == [SP["eos"]] * 2 and row[n_real - 1] == SP["eos"] and row[n_real:] == [SP["pad"]] * (L - n_real)
            chunk = row[q + 3:q + 3 + n]
            assert chunk == body[w["start"]:w["start"] + n] and 0 <= n <= room
            assert w["type"] == [0] * (q + 2) + [1] * (n + 2) + [SP["pad"]] * (L - n_real)
            assert w["mask"] == [1] * n_real + [0] * (L - n_real)
            if j:
                assert n > s
            joined += chunk if j == 0 else chunk[s:]
        assert joined == body                                                                     # law 2


@pytest.mark.parametrize("L,s,mq", LSM)
def test_law_4_answers(L, s, mq):
    r = random.Random(L * 100 + s)
    for Tq in P.question_lengths(mq):
        q, room, step = P.geometry(Tq, L, s, mq)
        for T in sorted(set(P.context_lengths(room, step)) | {3 * room + 1, 40}):
            body = list(range(500, 500 + T))
            spans = [(a0, a1) for a0 in range(T) for a1 in range(a0 + 1, T + 1)]
            for a0, a1 in (spans if len(spans) < 300 else r.sample(spans, 300)):
                ws = P.windows(list(range(Tq)), body, L, s, mq, answer=(a0, a1), **SP)
                held = [w for w in ws if w["has_answer"]]
                if a1 - a0 <= s + 1:
                    assert held, (Tq, T, a0, a1)
                if a1 - a0 > room:
                    assert not held
                for w in ws:
                    if w["has_answer"]:
                        assert w["row"][w["start_pos"]:w["end_pos"] + 1] == body[a0:a1]
                        assert w["start_pos"] >= q + 3 and w["end_pos"] <= w["n_real"] - 2
                    else:
                        assert w["start_pos"] == 0 and w["end_pos"] == 0
            for bad in ((-1, -1), (2, 2), (3, 1), (0, T + 1), (-1, 2), (T, T + 1)):
                assert not any(w["has_answer"] or w["start_pos"] or w["end_pos"] for w in P.windows([], body, L, s, mq, answer=bad, **SP))


def test_table_worked_by_hand():
    """L = 8, mq = 1, s = 1, a question of 2 tokens, T = 5: q = 1, room = 3, step = 2, 2 windows."""
    ws = P.windows([70, 71], [10, 11, 12, 13, 14], 8, 1, 1, bos=1, eos=2, pad=0, answer=(2, 4))
    assert P.geometry(2, 8, 1, 1) == (1, 3, 2) and len(ws) == 2
    assert ws[0] == dict(row=[1, 70, 2, 2, 10, 11, 12, 2], mask=[1] * 8, type=[0, 0, 0, 1, 1, 1, 1, 1], start=0, n_real=8, q_len=1,
                         start_pos=0, end_pos=0, has_answer=0)
    assert ws[1] == dict(row=[1, 70, 2, 2, 12, 13, 14, 2], mask=[1] * 8, type=[0, 0, 0, 1, 1, 1, 1, 1], start=2, n_real=8, q_len=1,
                         start_pos=4, end_pos=5, has_answer=1)
    # a third token: the last window is shorter, not shifted back; the pad id stands in the type row too
    ws = P.windows([70], [10, 11, 12, 13, 14, 15], 8, 1, 1, bos=1, eos=2, pad=9)
    assert [w["row"] for w in ws] == [[1, 70, 2, 2, 10, 11, 12, 2], [1, 70, 2, 2, 12, 13, 14, 2], [1, 70, 2, 2, 14, 15, 2, 9]]
    assert ws[2]["type"] == [0, 0, 0, 1, 1, 1, 1, 9] and ws[2]["mask"] == [1] * 7 + [0] and ws[2]["n_real"] == 7
    # no question, no context
    ws = P.windows([], [], 5, 0, 0, bos=1, eos=2, pad=0)
    assert len(ws) == 1 and ws[0]["row"] == [1, 2, 2, 2, 0] and ws[0]["type"] == [0, 0, 1, 1, 0] and ws[0]["n_real"] == 4


def test_window_count_against_a_count_by_hand():
    for L, mq, s in P.rule_cases():
        for Tq in P.question_lengths(mq):
            q, room, step = P.geometry(Tq, L, s, mq)
            for T in sorted(set(range(0, 40)) | set(P.context_lengths(room, step)) | {3000}):
                n = 1
                while (n - 1) * step + room < T:
                    n += 1
                assert P.n_windows(T, room, step) == n, (L, mq, s, Tq, T)


def test_batch_form_matches_the_list_form():
    qs, bodies = [[7, 8, 9], [], [5]], P.counters([0, 7, 1, 30])
    q_row, answers = [2, 0, 1, 0], [(-1, -1), (2, 4), (0, 1), (10, 12)]
    b = P.batch(qs, bodies, 12, 2, 2, 1, 2, 0, q_row=q_row, answers=answers)
    per = [P.windows(qs[q_row[r]], bodies[r], 12, 2, 2, 1, 2, 0, answers[r]) for r in range(4)]
    flat = [w for ws in per for w in ws]
    assert b["win_off"].tolist() == [0] + np.cumsum([len(ws) for ws in per]).tolist() and len(flat) == b["win_off"][-1]
    assert b["input_ids"].tolist() == [w["row"] for w in flat] and b["token_type_ids"].tolist() == [w["type"] for w in flat]
    assert b["pair"].tolist() == [r for r, ws in enumerate(per) for _ in ws] and b["q_len"].tolist() == [w["q_len"] for w in flat]
    assert b["start_positions"].tolist() == [w["start_pos"] for w in flat] and b["has_answer"].sum() >= 3
    assert set(b) == set(P.KEYS + P.ANSWER_KEYS) and set(P.batch(qs[:2], bodies[:2], 12, 2, 2, 1, 2, 0)) == set(P.KEYS)
    # a q_row entry outside the questions is an empty question
    out = P.batch(qs, bodies[:2], 12, 2, 2, 1, 2, 0, q_row=[-1, 3])
    assert out["q_len"].tolist() == [0] * len(out["q_len"])
    e = P.batch([], [], 8, 0, 1, 1, 2, 0, answers=[])
    assert e["input_ids"].shape == (0, 8) and e["win_off"].tolist() == [0] and e["has_answer"].shape == (0,)


# ---- the GPU cases sit on their edges -------------------------------------------------------------------------------------------------
def test_rule_cases_are_legal_and_hold_their_edges():
    cases = P.rule_cases()
    assert {L for L, _, _ in cases} == set(P.RULE_LS) and (5, 0, 0) in cases
    assert {L % 4 for L in P.RULE_LS} >= {0, 1} and 128 in P.RULE_LS
    for L in P.RULE_LS:
        mine = [(mq, s) for l, mq, s in cases if l == L]
        assert {mq for mq, _ in mine} >= {0, L - 5} | ({1} if L >= 6 else set())              # mq in {0, 1, L - 5 - s}
        assert all(s in (0, L - 5 - mq) for mq, s in mine)                                    # s in {0, L - 5 - mq}
        assert (0, L - 5) in mine and any(mq >= 1 and s >= 1 and s == L - 5 - mq for mq, s in mine) == (L >= 8)      # a question AND an overlap at step 1
    total = 0
    for L, mq, s in cases:
        assert L >= 5 and 0 <= mq <= L - 5 and 0 <= s <= L - 5 - mq
        tqs, ts = P.rule_pairs(L, mq, s)
        assert set(tqs) == set(P.question_lengths(mq)) and {0, mq, mq + 1} <= set(tqs)
        for Tq in set(tqs):
            q, room, step = P.geometry(Tq, L, s, mq)
            assert q == min(Tq, mq) and room == L - 4 - q >= s + 1 and step >= 1
            mine = {T for a, T in zip(tqs, ts) if a == Tq}
            assert {0, 1, room, room + 1, room + step, room + step + 1} <= mine
            n = {T: P.n_windows(T, room, step) for T in mine}
            assert n[room] == 1 and n[room + 1] == 2 and n[room + step] == 2 and n[room + step + 1] == 3
        total += sum(P.n_windows(T, *P.geometry(Tq, L, s, mq)[1:]) for Tq, T in zip(tqs, ts))
    assert total < 5000                                                                       # seconds on the GPU, not minutes


def test_work_division_cases_make_exactly_their_windows():
    q, room, step = P.geometry(2, P.WORK_L, P.WORK_S, P.WORK_MQ)
    assert (q, room, step) == (2, 6, 5)
    for W in P.WORK_WS:
        lengths = P.work_lengths(W)
        n = [P.n_windows(T, room, step) for T in lengths]
        assert sum(n) == W and {1, 2, 3} <= set(n) and 0 in lengths
    assert set(P.WORK_WS) == {63, 64, 65, 128, 129}
    assert P.n_windows(P.LONG_T, room, step) > 40 * 64                                        # one pair's windows span many waves


def test_answer_cases_sit_where_they_are_named():
    q, room, step = P.geometry(P.ANSWER_TQ, P.ANSWER_L, P.ANSWER_S, P.ANSWER_MQ)
    assert (q, room, step) == (3, 9, 6) and P.n_windows(P.ANSWER_T, room, step) == 5
    body = list(range(100, 100 + P.ANSWER_T))

    def holders(name):
        ws = P.windows([1, 2, 3], body, P.ANSWER_L, P.ANSWER_S, P.ANSWER_MQ, answer=P.ANSWERS[name], **SP)
        assert [w["start"] for w in ws] == [0, 6, 12, 18, 24] and [w["n_real"] - q - 4 for w in ws] == [9, 9, 9, 9, 6]
        return [j for j, w in enumerate(ws) if w["has_answer"]]
    assert holders("a0_at_start") == [0, 1] and P.ANSWERS["a0_at_start"][0] == 6
    assert holders("a1_at_end") == [1, 2] and P.ANSWERS["a1_at_end"][1] == 6 + 9
    assert holders("straddles_end") == [1]
    assert holders("in_overlap") == [0, 1]
    assert holders("longer_than_room") == [] and P.ANSWERS["longer_than_room"][1] - P.ANSWERS["longer_than_room"][0] > room
    assert holders("none") == holders("empty") == holders("past_end") == []
    assert holders("whole_tail") == [4] and holders("first_token") == [0]


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
class _NoNative:
    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were validated" % name)


def _bare():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    t = tokenize.Tokenize.__new__(tokenize.Tokenize)
    t._ctx = _NoNative()

    def no_tables():
        raise AssertionError("tables synchronised before the arguments were validated")
    t._sync_tables = no_tables
    return t


def test_pair_window_rule():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    rule = tokenize.Tokenize._pair_window_rule
    assert rule(128, 32) == (128, 32, 64) and rule(128, 0) == (128, 0, 64) and rule(384, 128, None) == (384, 128, 64)
    assert rule(16, 4) == (16, 4, 7) and rule(5, 0) == (5, 0, 0) and rule(16, 11) == (16, 11, 0)      # min(64, L - 5 - s)
    assert rule(16, 0, 11) == (16, 0, 11) and rule(16, 3, 8) == (16, 3, 8) and rule(np.int64(16), np.int32(3), np.int16(0)) == (16, 3, 0)
    for L, mq, s in P.rule_cases():
        assert rule(L, s, mq) == (L, s, mq)
    for bad in ((4, 0), (0, 0), (-3, 0), (2 ** 31, 0), (16, -1), (16, 12), (16, 0, 12), (16, 0, -1), (16, 4, 8), (16, 11, 1), (5, 1), (5, 0, 1)):
        with pytest.raises(ValueError):
            rule(*bad)
    for bad in ((16.0, 0), (None, 0), ("16", 0), (True, 0), (16, 1.5), (16, None), (16, 0, 2.0), (16, 0, "2"), (16, 0, False)):
        with pytest.raises(TypeError):
            rule(*bad)


def test_python_refusals_come_before_any_native_call():
    t = _bare()
    qs, cs = [[1, 5, 2], [1, 2]], [[1, 7, 8, 9, 2], [1, 2]]
    for call in (lambda **k: t.pair_window_rows(qs, cs, **k), lambda **k: t.encode_pair_windows(["a", "b"], ["c d", "e"], **k),
                 lambda **k: t.encode_pair_windows_to_device(["a", "b"], ["c d", "e"], **k)):
        for kw, exc in ((dict(max_len=4), ValueError), (dict(max_len=16, stride=12), ValueError), (dict(max_len=16, stride=-1), ValueError),
                        (dict(max_len=16, max_query_len=12), ValueError), (dict(max_len=16, max_query_len=-1), ValueError),
                        (dict(max_len=16, stride=6, max_query_len=6), ValueError), (dict(max_len=16.0), TypeError), (dict(max_len=True), TypeError),
                        (dict(max_len=16, stride=1.0), TypeError), (dict(max_len=16, max_query_len="4"), TypeError),
                        (dict(max_len=16, q_row=[0]), ValueError), (dict(max_len=16, q_row=[0, 2]), ValueError), (dict(max_len=16, q_row=[-1, 0]), ValueError),
                        (dict(max_len=16, q_row=[[0, 1]]), ValueError), (dict(max_len=16, q_row=[0.0, 1.0]), TypeError),
                        (dict(max_len=16, answers=[(0, 1)]), ValueError), (dict(max_len=16, answers=[(0, 1), (0, 1, 2)]), ValueError),
                        (dict(max_len=16, answers=[(0, 1.5), None]), TypeError), (dict(max_len=16, answers=[(0, 2 ** 31), None]), ValueError),
                        (dict(max_len=16, answers=np.zeros((2, 3), dtype=np.int32)), ValueError), (dict(max_len=16, answers=np.zeros((2, 2))), TypeError),
                        (dict(max_len=16, answers=np.zeros((3, 2), dtype=np.int64)), ValueError)):
            with pytest.raises(exc):
                call(**kw)
    with pytest.raises(ValueError):
        t.pair_window_rows(qs[:1], cs, 16)                                 # no q_row: one question per context
    with pytest.raises(ValueError):
        t.encode_pair_windows(["a"], ["b", "c"], 16)
    with pytest.raises(TypeError):
        t.pair_window_rows(np.zeros((2, 4)), cs, 16)
    with pytest.raises(TypeError):
        t.pair_window_rows(qs, np.zeros((1, 4)), 16, q_row=[0])
    for bad in ((["a", 3], ["b", "c"]), ([b"a", "b"], ["b", "c"]), (["a", "b"], ["b", None])):
        with pytest.raises(TypeError):
            t.encode_pair_windows(*bad, 16)
    with pytest.raises(ValueError):
        t.encode_pair_windows(["a", "b"], ["c d", "e"], 16, unit="word")
    with pytest.raises(TypeError):
        t.encode_pair_windows(["a", "b"], ["c d", "e"], 16, unit=0)
    counts, woff = np.array([1, 2, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64)
    mw, moff = np.array([[0, 2], [-1, -1]], dtype=np.int32), np.array([0, 1, 2], dtype=np.int64)
    for a, exc in (((np.array([1, 0, 1]), woff, mw, moff), ValueError), ((counts, np.array([0, 2, 4]), mw, moff), ValueError),
                   ((counts, woff, mw[:, :1], moff), ValueError), ((counts, woff, mw, np.array([0, 1, 3])), ValueError),
                   ((counts, woff, mw, np.array([0, 2])), ValueError), ((counts, woff, mw.astype(np.float64), moff), TypeError),
                   ((counts, woff, np.array([[0, 3], [-1, -1]]), moff), ValueError),          # beyond the document's 2 words
                   ((counts, woff, np.array([[0, 2], [1, 2]]), moff), ValueError),            # document 1 has one word
                   ((counts, woff, np.array([[2, 1], [-1, -1]]), moff), ValueError), ((counts, woff, np.array([[-1, 1], [-1, -1]]), moff), ValueError),
                   ((counts, np.array([0.0, 3.0]), mw, moff), TypeError)):
        with pytest.raises(exc):
            t.span_tokens(*a)


# ---- pair_window_spans ------------------------------------------------------------------------------------------------------------------
def _result(contexts, counts_per_doc, questions_q, L, s, answers_words):
    """A result as encode_pair_windows lays it out, made by the oracle: words are \\S+ runs, word j of a context has counts[j] tokens."""
    import re
    span, counts, word_off, bodies, answers = [], [], [0], [], []
    for text, cnt, aw in zip(contexts, counts_per_doc, answers_words):
        ms = list(re.finditer(r"\S+", text))
        assert len(ms) == len(cnt)
        span += [[m.start(), m.end()] for m in ms]
        counts += cnt
        word_off.append(len(counts))
        bodies.append(list(range(sum(cnt))))
        C = [0] + np.cumsum(cnt).tolist()
        answers.append((-1, -1) if aw is None else (C[aw[0]], C[aw[1] + 1]))
    out = P.batch([list(range(q)) for q in questions_q], bodies, L, s, max(questions_q), 1, 2, 0, answers=answers)
    out.update(word_off=np.array(word_off, dtype=np.int64), word_span=np.array(span, dtype=np.int32).reshape(-1, 2),
               word_tokens=np.array(counts, dtype=np.int32))
    return out, span, word_off


def test_pair_window_spans_law_and_junk_columns():
    tokenize = pytest.importorskip("genz_tokenize.tokenize")
    spans_of = tokenize.Tokenize.pair_window_spans
    contexts = ["xin chao  cac ban\nhoc   may", "mot", "", "a b c d e f g h i j k l"]
    counts = [[1, 3, 1, 2, 1, 4], [2], [], [1, 2, 1, 1, 3, 1, 1, 1, 2, 1, 1, 1]]
    aw = [(1, 3), (0, 0), None, (4, 5)]
    res, span, word_off = _result(contexts, counts, [2, 0, 3, 1], 16, 3, aw)
    W = len(res["pair"])
    assert W >= 6 and res["has_answer"].sum() == 3 and (res["has_answer"] == 0).any()      # every answer is held once
    got = spans_of(res, res["start_positions"], res["end_positions"])
    assert got.dtype == np.int32 and got.shape == (W, 2)
    for w in range(W):
        r = int(res["pair"][w])
        if res["has_answer"][w]:
            f, l = aw[r]
            assert got[w].tolist() == [span[word_off[r] + f][0], span[word_off[r] + l][1]], w      # the words the answer overlaps
        else:
            assert got[w].tolist() == [-1, -1]                                                    # column 0 is bos: outside the chunk
    # a column inside a word gives the whole word; every chunk column maps to its word
    for w in range(W):
        r, q, n, start = int(res["pair"][w]), int(res["q_len"][w]), int(res["n_real"][w]) - int(res["q_len"][w]) - 4, int(res["start"][w])
        ends = np.cumsum(counts[r]).tolist()
        for k in range(n):
            word = next(j for j, e in enumerate(ends) if start + k < e)
            one = spans_of(res, np.where(np.arange(W) == w, q + 3 + k, 0), np.where(np.arange(W) == w, q + 3 + k, 0))
            assert one[w].tolist() == span[word_off[r] + word] and (np.delete(one, w, axis=0) == -1).all()
        # junk: the separators, the last eos, padding, negative and huge columns, end < start
        for a, b in ((q + 2, q + 3), (q + 3, q + 3 + n), (0, 0), (-1, q + 3), (q + 3, 10 ** 9), (q + 4, q + 3), (15, 15)):
            if n == 0 or not (q + 3 <= a <= b < q + 3 + n):
                assert spans_of(res, np.full(W, a), np.full(W, b))[w].tolist() == [-1, -1], (w, a, b)
    with pytest.raises(ValueError):
        spans_of(res, res["start_positions"][:-1], res["end_positions"])
    empty = P.batch([], [], 8, 0, 1, 1, 2, 0, answers=[])
    empty.update(word_off=np.zeros(1, dtype=np.int64), word_span=np.zeros((0, 2), dtype=np.int32), word_tokens=np.zeros(0, dtype=np.int32))
    assert spans_of(empty, [], []).shape == (0, 2)


def test_word_list_has_split_words_and_an_unknown_one(oracle_tables):
    import gz_oracle as O
    t = oracle_tables
    pieces = {w: O.encode(w, t)[1:-1] for w in P.WORDS}
    assert sum(len(p) == 1 for p in pieces.values()) >= 5 and sum(len(p) >= 3 for p in pieces.values()) >= 2
    assert any(t.unk_id in p for p in pieces.values())
    contexts = P.texts(48, 1, 60, 7)
    spans, words = P.word_answers(contexts, 3)
    assert sum(s is None for s in spans) >= 10 and sum(s is not None for s in spans) >= 30
    assert any(w is not None and w[1] > w[0] for w in words)
    assert max(len(O.encode(x, t)) - 2 for x in contexts) > 3 * 24                # several windows at L = 32
