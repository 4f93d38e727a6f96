"""BPE-dropout on the GPU against the plain-Python oracle (tests/dropout_oracle.py), byte for byte: the known answers, single words at
the boundaries of the lane / wave / chunked forms, p = 0 against the plain encode in every single-text shape, p = 1 against the code
points, a batch of about 300 documents and 6 000 words on every kernel path and through every door, reproducibility across calls and
batch splits, a table other than the bundled one, and the composition with window_rows and decode_batch.  The oracle's rows of the
batch are computed once per p and shared."""
import contextlib
import json
import os
import random

import numpy as np
import pytest

import dropout_oracle as DO
import gz_oracle as O
import row_tables as RT
import window_oracle as WO
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

PS = (0.0, 0.1, 0.5, 1.0)
LETTERS = "abcdefghijklmnopqrstuvwxyz_áàảãạâấầăđêếềệôốồơớờưứừíìúùýABCXYZ0123456789"
BASE = "sinhviêncôngnghệthôngtinhelloworld_họcmáytrườngđạihọcnghiêncứu"


@pytest.fixture(scope="module")
def tok():
    from genz_tokenize import Tokenize
    return Tokenize()


@pytest.fixture(scope="module")
def known():
    with open(os.path.join(GOLDEN, "dropout_known.json"), encoding="ascii") as f:
        return json.load(f)


DEFAULTS = dict(sub_batches=1, m2_split_always=0, hot_miss_wgs=0, assemble=3)


@contextlib.contextmanager
def switches(tok, **kv):
    from genz_tokenize import _native
    try:
        for k, v in kv.items():
            _native.debug_set(k, v, tok._ctx)
        yield
    finally:
        for k in kv:
            _native.debug_set(k, DEFAULTS[k], tok._ctx)


def ragged_rows(r):
    ro = r["row_off"]
    assert r["input_ids"].dtype == np.int32 and r["attention_mask"].dtype == np.int32 and ro.dtype == np.int64
    return [r["input_ids"][ro[i]:ro[i + 1]].tolist() for i in range(len(ro) - 1)]


def check(got, t, framed, max_len=None, padding=True, truncation=True):
    """a result of encode_dropout* against the oracle's framed rows in the same shape, every array"""
    want = DO.shaped(t, framed, max_len, padding, truncation)
    dense = max_len is not None and padding and truncation
    if dense:
        ids = got["input_ids"] if isinstance(got["input_ids"], np.ndarray) else got["input_ids"].numpy()
        am = got["attention_mask"] if isinstance(got["attention_mask"], np.ndarray) else got["attention_mask"].numpy()
        assert ids.dtype == np.int32 and ids.shape == (len(framed), max_len) == am.shape
        bad = [i for i in range(len(want)) if ids[i].tolist() != want[i]]
        assert bad == [], (bad[:5], ids[bad[0]].tolist(), want[bad[0]])
    else:
        rows = ragged_rows(got)
        bad = [i for i in range(len(want)) if rows[i] != want[i]]
        assert bad == [], (bad[:5], rows[bad[0]][:40], want[bad[0]][:40])
        ids, am = got["input_ids"], got["attention_mask"]
        assert got["row_off"].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert np.array_equal(am, (ids != t.pad_id).astype(np.int32))
    assert got["n_real"].tolist() == [sum(1 for v in w if v != t.pad_id) for w in want]


# ---- the golden text ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
def test_golden_text(tok, oracle_tables, known, p):
    case = [c for c in known["cases"] if c["p"] == p][0]
    r = tok.encode_dropout([known["text"]], p=p, seed=known["seed"], doc_base=known["doc"])
    assert ragged_rows(r) == [case["ids"]]
    for j, (w, pieces) in enumerate(zip(O.split_words(known["text"]), case["pieces"])):
        assert tok.bpe_dropout(w, p, seed=known["seed"], doc=known["doc"], word=j) == pieces


# ---- single words ---------------------------------------------------------------------------------------------------------------
def single_words():
    out = [(BASE * 4)[:n] for n in (1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 200)]
    out += ["a" * n for n in list(range(2, 10)) + [63, 64, 65, 66, 127, 128, 129, 130]]
    out += ["ôêđưă", "ệấầứừ", "中文字符", "\U0001F600\U0001F601\U0001F602", "aô中\U0001F600b", "đ\U0001F600" * 9, "ệ" * 17]
    out += ["中文字", "☃☄", "hello\n", "thông_tin\n", "a\n"]
    return out


@pytest.mark.parametrize("p", PS)
def test_single_words(tok, oracle_tables, p):
    t, thr = oracle_tables, DO.threshold(p)
    assert [len(w) for w in single_words()[:11]] == [1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 200]
    for k, w in enumerate(single_words()):
        for seed, doc, j in ((0, 0, 0), (7, 3, k), (2 ** 64 - 1, 2 ** 40 + 5, 2 ** 32 - 1)):
            assert tok.bpe_dropout(w, p, seed=seed, doc=doc, word=j) == DO.bpe_string(w, t, thr, seed, doc, j), (w, seed, doc, j)
    if p == 1.0:
        assert tok.bpe_dropout("中文字", 0.0) == "中@@ 文@@ 字"      # code points in no table never merge
        assert ragged_rows(tok.encode_dropout(["☃☄"], p=0.0)) == [[t.bos_id, t.unk_id, t.unk_id, t.eos_id]]
    if p == 0.0:
        for w in single_words():
            assert tok.bpe_dropout(w, 0.0) == tok.bpe(w), w


def test_words_in_a_batch_take_the_same_path_as_alone(tok, oracle_tables):
    """every single word as a document of its own and all of them as one document: the lane, wide and chunked kernels of the pipeline"""
    t = oracle_tables
    docs = [w for w in single_words() if not w.endswith("\n")] + ["hello\nworld a\n\nb", " ".join(w for w in single_words() if not w.endswith("\n"))]
    for p in (0.1, 0.5):
        framed = DO.rows(t, docs, DO.threshold(p), seed=11, doc_base=5)
        check(tok.encode_dropout(docs, p=p, seed=11, doc_base=5), t, framed)


# ---- p = 0 and p = 1 --------------------------------------------------------------------------------------------------------------
SHAPES = [dict(max_len=8), dict(max_len=10), dict(max_len=None), dict(max_len=8, padding=False), dict(max_len=8, truncation=False)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
def test_p_zero_is_the_plain_encode(tok, shape):
    texts = WO.texts(120, 14, 3) + ["", " \n ", "hello\nworld", "x" * 40, "a"]
    got = tok.encode_dropout(texts, p=0, seed=5, doc_base=9, **shape)
    for word_table in (True, False):
        want = tok.encode_batch(texts, word_table=word_table, **shape)
        for k in ("input_ids", "attention_mask", "row_off", "n_real"):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, word_table)
            assert np.array_equal(got[k], want[k]), (k, word_table)
        assert got["dense"] == want["dense"]


def test_p_one_is_the_code_points(tok, oracle_tables):
    t = oracle_tables
    texts = WO.texts(60, 10, 8) + ["", "hello\nworld", "☃ a"]
    unk = t.unk_id
    want = []
    for x in texts:
        row = [t.bos_id]
        for w in O.split_words(x):
            row += [t.encoder.get(c + "@@", unk) for c in w[:-1]] + [t.encoder.get(w[-1], unk)]
        want.append(row + [t.eos_id])
    assert ragged_rows(tok.encode_dropout(texts, p=1, seed=3)) == want
    assert ragged_rows(tok.encode_dropout(texts, p=1.0, seed=4, doc_base=77)) == want


# ---- the batch ------------------------------------------------------------------------------------------------------------------------
def make_batch():
    import corpus
    n = 318
    text, offs, _ = corpus.config_corpus(2, n_docs=n, seed=21)
    raw = text.tobytes()
    r = random.Random(3)

    def letters(lo, hi):
        return "".join(r.choice(LETTERS) for _ in range(r.randint(lo, hi)))
    docs = []
    for i in range(n):
        ws = raw[offs[i]:offs[i + 1]].decode("utf-8").split(" ")
        docs.append(" ".join(letters(1, 24) if r.random() < 0.2 else w for w in ws))
    docs[5], docs[6], docs[7], docs[8], docs[9] = "", " \t \n ", "hello", "", "　"
    docs[40] = "".join(r.choice(WO.WORDS[:20]) for _ in range(800))[:3000]                      # ONE word of 3 000 symbols
    docs[41] = "".join("w%d" % k + chr(c) for k, c in enumerate(sorted(O.WHITESPACE)))          # every whitespace code point
    docs[42] = "hello\nworld\n\nxin chào\n" + letters(17, 17) + "\n " + letters(16, 16) + "\n"  # glued line feeds, at the lane form's edge too
    docs[43] = letters(64, 64) + " " + letters(65, 65) + " " + letters(300, 300) + " \U0001F600\U0001F601 " + "ệ" * 16
    docs += ["", "một"]
    return docs


@pytest.fixture(scope="module")
def batch(oracle_tables):
    docs = make_batch()
    words = [w for d in docs for w in O.split_words(d)]
    assert 295 <= len(docs) <= 325 and 5000 <= len(words) <= 7000 and len(words) > 3072
    assert len(docs[40]) == 3000 and O.split_words(docs[40]) == [docs[40]]
    assert len(O.split_words(docs[41])) == len(O.WHITESPACE)
    assert 0.01 < sum(1 for w in words if len(w) > 16) / len(words) < 0.25                      # wide words are there, and are few
    return docs, {p: DO.rows(oracle_tables, docs, DO.threshold(p), seed=13, doc_base=1000) for p in (0.1, 0.5)}


KW = dict(seed=13, doc_base=1000)


@pytest.mark.parametrize("p", (0.1, 0.5))
def test_batch_ragged_and_dense(tok, oracle_tables, batch, p):
    docs, framed = batch
    t = oracle_tables
    assert framed[0.1] != framed[0.5]
    check(tok.encode_dropout(docs, p=p, **KW), t, framed[p])
    check(tok.encode_dropout(docs, p=p, max_len=32, **KW), t, framed[p], 32)
    check(tok.encode_dropout(docs, p=p, max_len=30, **KW), t, framed[p], 30)
    check(tok.encode_dropout(docs, p=p, max_len=24, padding=False, **KW), t, framed[p], 24, padding=False)
    check(tok.encode_dropout(docs, p=p, max_len=24, truncation=False, **KW), t, framed[p], 24, truncation=False)


@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("sw", [dict(sub_batches=1), dict(sub_batches=3), dict(m2_split_always=1), dict(hot_miss_wgs=1), dict(assemble=1),
                                dict(assemble=3), dict(sub_batches=3, hot_miss_wgs=1, assemble=1)],
                         ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
def test_batch_under_the_switches(tok, oracle_tables, batch, p, sw):
    docs, framed = batch
    with switches(tok, **sw):
        check(tok.encode_dropout(docs, p=p, max_len=32, **KW), oracle_tables, framed[p], 32)
        check(tok.encode_dropout(docs, p=p, **KW), oracle_tables, framed[p])


@pytest.mark.parametrize("p", (0.1, 0.5))
def test_batch_through_every_door(tok, oracle_tables, batch, p):
    docs, framed = batch
    t = oracle_tables
    enc = [d.encode("utf-8") for d in docs]
    text = np.frombuffer(b"".join(enc), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)
    check(tok.encode_dropout_packed(text, offs, p=p, **KW), t, framed[p])
    check(tok.encode_dropout_packed(text, offs, p=p, max_len=32, **KW), t, framed[p], 32)
    dev = tok.encode_dropout_to_device(docs, p, 13, 32, doc_base=1000)
    check(dev, t, framed[p], 32)
    with switches(tok, sub_batches=3):
        check(tok.encode_dropout_to_device(docs, p, 13, 32, doc_base=1000), t, framed[p], 32)


# ---- reproducibility --------------------------------------------------------------------------------------------------------------
def test_reproducible(tok, batch):
    docs, _ = batch
    a = tok.encode_dropout(docs, p=0.3, seed=21, doc_base=50)
    b = tok.encode_dropout(docs, p=0.3, seed=21, doc_base=50)
    for k in ("input_ids", "attention_mask", "row_off", "n_real"):
        assert np.array_equal(a[k], b[k]), k
    h = len(docs) // 2
    first, second = tok.encode_dropout(docs[:h], p=0.3, seed=21, doc_base=50), tok.encode_dropout(docs[h:], p=0.3, seed=21, doc_base=50 + h)
    assert ragged_rows(first) + ragged_rows(second) == ragged_rows(a)
    assert ragged_rows(tok.encode_dropout(docs, p=0.3, seed=22, doc_base=50)) != ragged_rows(a)
    assert ragged_rows(tok.encode_dropout(docs, p=0.3, seed=21, doc_base=51)) != ragged_rows(a)
    # a dropout call is an encode call that keeps no word records
    from genz_tokenize import _native
    with pytest.raises(_native.GzError):
        tok._ctx.word_token_counts(0, len(docs), 16)


# ---- the C entry points' refusals ----------------------------------------------------------------------------------------------------
def test_invalid_arguments(tok):
    from genz_tokenize import _native
    tok._sync_tables()
    ctx, lib = tok._ctx, tok._ctx.lib
    text = np.frombuffer(b"a b", dtype=np.uint8)
    off = np.array([0, 3], dtype=np.int64)
    ids, am, ro, nr = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(2, np.int64), np.zeros(1, np.int32)
    ptr = _native._ptr

    def call(fn, flags=_native.GZ_MAX_LEN_NONE, thr=0, doc_base=0, n=1):
        return fn(ctx.handle, ptr(text), ptr(off), n, 0, flags, 16, thr, 0, doc_base, ptr(ids), ptr(am), ptr(ro), ptr(nr))
    for fn in (lib.gz_encode_dropout, lib.gz_encode_dropout_device):
        assert call(fn, flags=_native.GZ_MAX_LEN_NONE | _native.GZ_KEEP_WORDS) == _native.GZ_E_INVALID
        assert call(fn, thr=2 ** 32 + 1) == _native.GZ_E_INVALID
        assert call(fn, doc_base=-1) == _native.GZ_E_INVALID
        assert call(fn, doc_base=2 ** 63 - 1) == _native.GZ_E_INVALID
    assert call(lib.gz_encode_dropout, thr=2 ** 32, doc_base=2 ** 63 - 2) == _native.GZ_OK
    assert call(lib.gz_encode_dropout, flags=_native.GZ_MAX_LEN_NONE | _native.GZ_NO_WORD_TABLE) == _native.GZ_OK
    w = np.frombuffer(b"hello", dtype=np.uint8)
    out = np.zeros(8, np.int32)
    for thr, doc, j in ((2 ** 32 + 1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 2 ** 32)):
        assert lib.gz_bpe_word_dropout(ctx.handle, ptr(w), 5, thr, 0, doc, j, ptr(out), 8) == _native.GZ_E_INVALID
    assert lib.gz_bpe_word_dropout(ctx.handle, ptr(w), 5, 2 ** 32, 0, 2 ** 63 - 1, 2 ** 32 - 1, ptr(out), 8) == 5


# ---- other tables ---------------------------------------------------------------------------------------------------------------------
def test_on_another_table(tmp_path):
    """the table `moved` of tests/row_tables.py: special ids that are not 0 .. 4, a small merges file, a letter that is in no word"""
    from genz_tokenize import Tokenize
    t = RT.table("moved")
    vocab, merges = os.path.join(str(tmp_path), "moved.vocab"), os.path.join(str(tmp_path), "moved.codes")
    for path, data in ((vocab, t.vocab), (merges, t.merges)):
        with open(path, "wb") as f:
            f.write(data)
    tk = Tokenize.__new__(Tokenize)
    tk.vocab_file, tk.bpe_file = vocab, merges
    pad, bos, eos, mask, unk = t.specials
    tk.__init__(pad_token=pad, bos_token=bos, eos_token=eos, mask_token=mask, unk_token=unk)
    ref = O.Tables(t.vocab, t.merges, t.specials)
    texts = RT.texts(70, 5) + ["abcdabcdabcdabcdabcde " + "abcd" * 40 + " ba"]
    for p in (0.0, 0.3, 1.0):
        framed = DO.rows(ref, texts, DO.threshold(p), seed=4, doc_base=2)
        check(tk.encode_dropout(texts, p=p, seed=4, doc_base=2), ref, framed)
        check(tk.encode_dropout(texts, p=p, seed=4, doc_base=2, max_len=12), ref, framed, 12)
    assert ragged_rows(tk.encode_dropout(texts, p=0.0)) == ragged_rows(tk.encode_batch(texts, max_len=None))


# ---- composition ------------------------------------------------------------------------------------------------------------------------
def test_composes_with_windows_and_decode(tok, oracle_tables):
    t = oracle_tables
    r = random.Random(12)
    words = [w for w in WO.WORDS if w not in ("zzqxj中q", "GPU", "Việt_Nam")]      # (the vocabulary has no single capital letters)
    texts = [" ".join(r.choice(words) for _ in range(r.randint(0, 40))) for _ in range(150)]
    framed = DO.rows(t, texts, DO.threshold(0.5), seed=6)
    assert all(t.unk_id not in row for row in framed)                 # no piece fell to unk: the text survives
    got = tok.encode_dropout(texts, p=0.5, seed=6, max_len=None)
    check(got, t, framed)
    rows = ragged_rows(got)
    assert rows != ragged_rows(tok.encode_batch(texts, max_len=None))
    pad, bos, eos = t.pad_id, t.bos_id, t.eos_id
    want = WO.batch([row[1:-1] for row in framed], 16, 4, bos, eos, pad)
    win = tok.window_rows(rows, 16, 4)
    for k in want:
        assert win[k].dtype == want[k].dtype and np.array_equal(win[k], want[k]), k
    assert tok.decode_batch(rows) == [" ".join(["<s>"] + x.split() + ["</s>"]) for x in texts]
