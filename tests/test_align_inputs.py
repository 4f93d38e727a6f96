"""CPU-only: the oracle and the inputs of the align tests are what test_gpu_align.py assumes.  The oracle's spans cut out exactly the
words of O.split_words; its rows for start = 0 have -1 exactly where O.call(...) holds bos, eos or pad at the cut; and the generators
produce the edge cases they claim."""
import random

import numpy as np
import pytest

import align_oracle as A
import gz_oracle as O
import offset_oracle as X


def _all_docs():
    for name, docs in A.span_batches().items():
        for d in docs:
            yield name, d
    for d in A.noisy_corpus():
        yield "corpus", d


def test_spans_cut_out_the_words_of_split_words():
    n = 0
    for name, d in _all_docs():
        words = O.split_words(d)
        sp = A.spans(d)
        assert len(sp) == len(words), (name, d[:40])
        raw = A.enc(d)
        for (b, e), (bb, be), w in zip(sp, A.spans(d, "byte"), words):
            bare = w[:-1] if w.endswith("\n") else w
            assert d[b:e] == bare, (name, b, e)
            assert raw[bb:be] == A.enc(bare), (name, bb, be)
            assert (w.endswith("\n")) == (e < len(d) and d[e] == "\n"), (name, b, e)
            n += 1
    assert n > 20000


def test_spans_equal_finditer_on_random_whitespace_heavy_strings():
    r = random.Random(5)
    alphabet = "ab\u00e9\u1ec7\U0001F600 \n\r\t\u00a0\u0085\u2003\u2028\u3000\u1680\x1c\ud800"
    for _ in range(2000):
        s = "".join(r.choice(alphabet) for _ in range(r.randrange(0, 40)))
        words = O.split_words(s)
        assert [s[b:e] for b, e in A.spans(s)] == [w[:-1] if w.endswith("\n") else w for w in words], repr(s)


def test_rows_for_start_0_frame_where_the_call_does(oracle_tables):
    t = oracle_tables
    docs = list(A.noisy_corpus()[:60]) + ["", "xin", "a\n b", "sinh_viên công_nghệ " * 30]
    counts = [A.piece_counts(d, t) for d in docs]
    for L in (3, 4, 16, 48):
        wid, _, n_real = A.rows(counts, range(len(docs)), [0] * len(docs), L)
        for i, d in enumerate(docs):
            got = O.call(t, d, max_len=L, padding=True, truncation=True)["input_ids"]
            special = [k == 0 or k >= n_real[i] - 1 for k in range(L)]                   # bos | eos and pad
            assert [w == -1 for w in wid[i]] == special, (L, i)
            assert [x == t.pad_id for x in got] == [k >= n_real[i] for k in range(L)], (L, i)
            assert got[0] == t.bos_id and got[n_real[i] - 1] == t.eos_id, (L, i)
            # the words of the cells: every word's run of cells is as long as its piece count, up to the cut
            body = [w for w in wid[i] if w >= 0]
            want = [j for j, c in enumerate(counts[i]) for _ in range(c)][:L - 2]
            assert body == want, (L, i)


def test_straddlers_straddle():
    docs, claims = A.straddle_docs()
    raw = A.pack(docs)[0].tobytes()
    assert {w for _, _, w in claims} == {2, 3, 4}
    assert {(b, w) for _, b, w in claims} >= {(1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4)}
    for edge, before, w in claims:
        assert edge % X.TILE == 0 and edge < len(raw)
        ch = raw[edge - before:edge - before + w]
        assert (ch[0] & 0xC0) != 0x80 and all((c & 0xC0) == 0x80 for c in ch[1:]), (edge, ch)
        assert len(ch.decode("utf-8", "surrogatepass")) == 1
    assert any(raw[e - b:e - b + w] in (b"\xc2\xa0", b"\xe2\x80\x83") for e, b, w in claims)       # two- and three-byte spaces too
    assert any(raw[e - b:e - b + w] == b"\xed\xa0\x80" for e, b, w in claims)                       # and a lone surrogate


def test_small_docs_hold_what_they_claim():
    s = A.SMALL_DOCS
    for d in ("a\n b", "a\n\nb", "\n", "a\r\n", ""):
        assert d in s
    assert any(d.endswith("\n") and len(O.split_words(d)) == 2 for d in s)
    assert any(any(0xD800 <= ord(c) < 0xE000 for c in d) for d in s)
    assert A.spans("a\n b") == [(0, 1), (3, 4)] and A.spans("a\n\nb") == [(0, 1), (3, 4)] and A.spans("\n") == [] and A.spans("a\r\n") == [(0, 1)]
    b = A.span_batches()
    assert b["none"] == [] and b["one_empty"] == [""]
    runs = set()
    for batch in X.edges():
        run = 0
        for d in batch.docs + ["x"]:
            if d == "":
                run += 1
            else:
                if run:
                    runs.add(run)
                run = 0
    assert runs >= {1, 2, 65}
    assert max(len(w) for _, w in X.ladder_words()) == 2500


def test_synthetic_counts_hold_the_align_cases():
    docs = A.synthetic_counts()
    assert {len(d) for d in docs} >= {0, 1, 2, 16, 17, 2500}
    for L in A.ALIGN_LENS:
        room = L - 2
        totals = {sum(d) for d in docs}
        assert {room, room + 1} <= totals and (room == 1 or room - 1 in totals)
        at_boundary = [d for d in docs if sum(d) > room and room in np.cumsum(d).tolist()]
        inside = [d for d in docs if sum(d) > room and room not in np.cumsum(d).tolist()]
        assert at_boundary and inside, L


def test_marks_hold_the_span_label_cases():
    r = random.Random(1)
    seen = set()
    for d in A.noisy_corpus()[:40]:
        sp = A.spans(d)
        marks = A.random_marks(sp, len(d), r)
        labels, mw = A.span_labels([sp], [marks], "bio")
        for (b, e, _), (f, l) in zip(marks, mw[0]):
            if e <= b:
                seen.add("reversed" if e < b else "empty")
                assert (f, l) == (-1, -1)
            elif b >= len(d):
                seen.add("past")
                assert (f, l) == (-1, -1)
            elif (f, l) == (-1, -1):
                seen.add("touching")                                  # a non-empty mark inside the text that overlaps no word
                assert all(e <= wb or we <= b for wb, we in sp)
            elif l - f > 1:
                seen.add("many")
        # B follows a stolen first word: some mark's first overlapped word belongs to an earlier mark, and its first OWNED word is a B
        owner = [None] * len(sp)
        for m, (f, l) in enumerate(mw[0]):
            for j in range(max(f, 0), max(l, 0)):
                if owner[j] is None:
                    owner[j] = m
        for m, (f, l) in enumerate(mw[0]):
            mine = [j for j in range(max(f, 0), max(l, 0)) if owner[j] == m]
            if f >= 0 and mine and mine[0] != f:
                seen.add("stolen")
                assert labels[0][mine[0]] == 2 * marks[m][2] + 1
    assert seen >= {"reversed", "empty", "past", "touching", "many", "stolen"}, seen
    assert A.span_labels([[]], [[(0, 5, 1)]], "plain", 7) == ([[]], [[(-1, -1)]])
    assert A.span_labels([[(0, 2), (3, 5)]], [[]], "plain", 7) == ([[7, 7]], [[]])
