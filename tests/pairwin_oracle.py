"""The pair window rule over lists of ints, stated once and on its own (nothing of the product is imported), and the case lists the
pair window tests share.  tests/test_pairwin_inputs.py ties `windows` to the reference's pair row (oracle/gz_oracle.py) and checks that
the lists hold the cases they are named for; tests/test_gpu_pairwin.py compares the GPU with it."""
import numpy as np

KEYS = ("input_ids", "attention_mask", "token_type_ids", "pair", "start", "n_real", "q_len", "win_off")
ANSWER_KEYS = ("start_positions", "end_positions", "has_answer")


def geometry(Tq, L, s, mq):
    """(q, room, step) of a pair whose question body has Tq tokens"""
    q = min(Tq, mq)
    room = L - 4 - q
    return q, room, room - s


def n_windows(T, room, step):
    return 1 if T <= room else 1 + -(-(T - room) // step)


def windows(question, body, L, s, mq, bos, eos, pad, answer=None):
    """The windows of one pair as dicts of plain lists and ints: row, mask, type, start, n_real, q_len, start_pos, end_pos, has_answer."""
    q, room, step = geometry(len(question), L, s, mq)
    T = len(body)
    present = False
    if answer is not None:
        a0, a1 = answer
        present = 0 <= a0 < a1 <= T
    out = []
    for j in range(n_windows(T, room, step)):
        start = j * step
        chunk = list(body[start:min(start + room, T)])
        n = len(chunk)
        row = [bos] + list(question[:q]) + [eos, eos] + chunk + [eos] + [pad] * (room - n)
        n_real = q + 4 + n
        typ = [0 if k < q + 2 else 1 if k < n_real else pad for k in range(L)]
        held = present and start <= a0 and a1 <= start + n
        out.append(dict(row=row, mask=[int(v != pad) for v in row], type=typ, start=start, n_real=n_real, q_len=q,
                        start_pos=q + 3 + a0 - start if held else 0, end_pos=q + 3 + a1 - 1 - start if held else 0, has_answer=int(held)))
    return out


def batch(questions, bodies, L, s, mq, bos, eos, pad, q_row=None, answers=None):
    """`windows` over many pairs, in the arrays the product returns.  A q_row entry outside the questions is an empty question (what the
    device form makes of it)."""
    per = []
    for r, body in enumerate(bodies):
        qi = r if q_row is None else q_row[r]
        question = questions[qi] if 0 <= qi < len(questions) else []
        per.append(windows(question, body, L, s, mq, bos, eos, pad, None if answers is None else answers[r]))
    flat = [(w, r) for r, ws in enumerate(per) for w in ws]
    W = len(flat)
    win_off = np.zeros(len(bodies) + 1, dtype=np.int64)
    if bodies:
        np.cumsum([len(ws) for ws in per], out=win_off[1:])

    def cells(k):
        return np.array([w[k] for w, _ in flat], dtype=np.int32).reshape(W, L)

    def column(k):
        return np.array([w[k] for w, _ in flat], dtype=np.int32).reshape(W)
    out = dict(input_ids=cells("row"), attention_mask=cells("mask"), token_type_ids=cells("type"), pair=np.array([r for _, r in flat], dtype=np.int32),
               start=column("start"), n_real=column("n_real"), q_len=column("q_len"), win_off=win_off)
    if answers is not None:
        out.update(start_positions=column("start_pos"), end_positions=column("end_pos"), has_answer=column("has_answer"))
    return out


def counters(lengths, base=1000):
    """Bodies whose ids count up across the batch: a cell taken from the wrong place shows."""
    out, at = [], base
    for T in lengths:
        out.append(list(range(at, at + T)))
        at += T
    return out


# ---- the cell rule: (L, mq, s) and, for each, the question and context lengths at the rule's edges ------------------------------------
RULE_LS = (5, 8, 12, 13, 128)                 # the minimum, the 4-cell path (8, 12, 128), the 1-cell path (5, 13)


def rule_cases():
    """[(L, mq, s)]: mq in {0, 1, L - 5 - s} and s in {0, L - 5 - mq}, every pair of them that is a valid call"""
    out = []
    for L in RULE_LS:
        for s_kind in ("zero", "most"):
            for mq_kind in (0, 1, "most"):
                if s_kind == "zero":
                    s, mq = 0, (L - 5 if mq_kind == "most" else mq_kind)
                    if mq > L - 5:
                        continue
                else:
                    if mq_kind == "most":
                        continue                          # (mq = L - 5 - s and s = L - 5 - mq together: every split, below)
                    mq = mq_kind
                    if mq > L - 5:
                        continue
                    s = L - 5 - mq
                if (L, mq, s) not in out:
                    out.append((L, mq, s))
        for mq in sorted({(L - 5) // 2, (L - 5) // 3}):    # both at once, mq = L - 5 - s and s = L - 5 - mq: step 1 where q = mq
            if (L, mq, L - 5 - mq) not in out:
                out.append((L, mq, L - 5 - mq))
    return out


def question_lengths(mq):
    return sorted({t for t in (0, 1, mq - 1, mq, mq + 1) if t >= 0})


def context_lengths(room, step):
    return sorted({t for t in (0, 1, room - 1, room, room + 1, room + step, room + step + 1) if t >= 0})


def rule_pairs(L, mq, s):
    """(question lengths, context lengths) of one batch: every Tq of the rule with every T at ITS room's edges, pair by pair"""
    tqs, ts = [], []
    for Tq in question_lengths(mq):
        q, room, step = geometry(Tq, L, s, mq)
        for T in context_lengths(room, step):
            tqs.append(Tq)
            ts.append(T)
    return tqs, ts


# ---- work division: W at the wave's edges ------------------------------------------------------------------------------------------
WORK_L, WORK_MQ, WORK_S = 12, 2, 1              # q = 2: room = 6, step = 5
WORK_WS = (63, 64, 65, 128, 129)


def work_lengths(W):
    """Context lengths of a batch with exactly W windows under (WORK_L, WORK_MQ, WORK_S) and questions of 2 tokens: rows of 1, 2 and 3
    windows in turn, then rows of one window"""
    room, step = WORK_L - 4 - WORK_MQ, WORK_L - 4 - WORK_MQ - WORK_S
    out, have, k = [], 0, 0
    while have < W:
        nw = min(1 + k % 3, W - have)
        out.append(0 if nw == 1 and k % 2 else room + (nw - 1) * step - (k % 2 if nw > 1 else 0))
        have += nw
        k += 1
    return out


LONG_T = 20000                                 # one context among short ones whose windows span many waves

# ---- answers: (a0, a1) against a context of ANSWER_T tokens under (ANSWER_L, ANSWER_MQ, ANSWER_S) with a question of 3 tokens -------------
ANSWER_L, ANSWER_MQ, ANSWER_S, ANSWER_TQ, ANSWER_T = 16, 3, 3, 3, 30      # q = 3: room = 9, step = 6: starts 0, 6, 12, 18, 24 -> n = 9, 9, 9, 9, 6
ANSWERS = {
    "a0_at_start": (6, 8),                     # a0 == start of window 1
    "a1_at_end": (13, 15),                     # a1 == start + n of window 1 (6 + 9)
    "straddles_end": (8, 10),                  # crosses window 0's end (9): window 1 holds it, window 0 does not
    "in_overlap": (7, 9),                      # inside [6, 9): held by windows 0 and 1
    "longer_than_room": (2, 12),               # 10 tokens > room: held by none
    "none": (-1, -1),
    "empty": (5, 5),                           # a0 == a1
    "past_end": (28, 31),                      # a1 > T
    "whole_tail": (24, 30),                    # the last, shorter window, all of it
    "first_token": (0, 1),
}

# words of the end-to-end texts: whole-word hits, words that split into several pieces, one word outside the vocabulary
WORDS = ["sinh_viên", "công_nghệ", "hello", "xin", "chào", "Việt_Nam", "học", "máy", "a", "và", "là", "của", "tokenization",
         "internationalization", "GPU", "2024", "thế_giới", "không", "một", "người", "trường_đại_học", "zzqxj中q", "nghiên_cứu", "!"]


def texts(n, lo_words, max_words, seed):
    import random
    r = random.Random(seed)
    return [" ".join(r.choice(WORDS) for _ in range(r.randint(lo_words, max_words))) for _ in range(n)]


def word_answers(contexts, seed):
    """One character span per context that covers whole words first..last (or None for every fourth context): (spans, [(first, last)])"""
    import random
    import re
    r = random.Random(seed)
    spans, words = [], []
    for i, t in enumerate(contexts):
        ms = list(re.finditer(r"\S+", t))
        if not ms or i % 4 == 3:
            spans.append(None)
            words.append(None)
            continue
        f = r.randrange(len(ms))
        l = min(len(ms) - 1, f + r.randrange(3))
        spans.append((ms[f].start(), ms[l].end()))
        words.append((f, l))
    return spans, words
