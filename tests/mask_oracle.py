"""The masked-LM rule of include/genz_tokenize.h ("masked-LM inputs and labels") in plain Python / numpy, for the tests.  Imports
nothing of the product: the continuation ids come in as an argument, and `continuation_ids` reads them from a vocab file the way the
reference numbers its lines (tokenize.py:31-51).

  protected cell   id in {pad, bos, eos, mask_id}: never chosen, passes through, label = ignore_index
  continuation     an id whose word ends in "@@"
  start(r, c)      unprotected, and c == 0 or cell c-1 protected or cell c-1 no continuation
  head(r, c)       the largest c' <= c with start(r, c'); c itself without whole_word
  g(r, c)          (row_base + r) * L + c
  D(g)             Philox4x32-10, counter (g lo, g hi, 0, 0), key (seed lo, seed hi)
  chosen           unprotected and D(g(head)).x0 < t_sel
  chosen cell      a = D(g).x1: a < t1 -> mask_id; a < t2 -> rand_lo + ((D(g).x2 * (rand_hi - rand_lo)) >> 32); else the id stays
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
ONE = 2 ** 32


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two -- ints or arrays of one shape.  Returns the four output words as uint64 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k = [np.asarray(x, dtype=np.uint64) for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64: no overflow
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & LOW, (p0 >> S32) ^ c[3] ^ k[1], p0 & LOW]
        k = [(k[0] + np.uint64(W0)) & LOW, (k[1] + np.uint64(W1)) & LOW]
    return c


def draw(g, seed):
    """D(g) for an array (or int) of global cell indices < 2^64: (x0, x1, x2, x3) as uint64 arrays"""
    g = np.asarray(g, dtype=np.uint64)
    zero = np.zeros_like(g)
    return philox4x32_10((g & LOW, g >> S32, zero, zero), (seed & 0xFFFFFFFF, seed >> 32))


def thresholds(p=0.15, mask_prob=0.8, random_prob=0.1):
    """(t_sel, t1, t2) the way Tokenize.mask_rows makes them: floor(x * 2**32), exact for a float"""
    return int(p * ONE), int(mask_prob * ONE), min(int((mask_prob + random_prob) * ONE), ONE)


def continuation_ids(vocab_path, n_special=5):
    """Sorted ids of the words of a vocab file that end in "@@", numbered as add_vocab_file numbers them (tokenize.py:44-51): the
    word is the stripped line up to its last space, and it gets the next free id -- line i gets id 5 + i in a file without
    repeated words, as the bundled one."""
    enc = {}
    with open(vocab_path, "r", encoding="utf-8") as f:
        for line in f.readlines():
            line = line.strip()
            word = line[:line.rfind(" ")]
            enc[word] = n_special + len(enc)
    return np.array(sorted(i for w, i in enc.items() if w.endswith("@@")), dtype=np.int64)


def heads(ids, cont_ids, protected, whole_word):
    """(prot bool [R, L], head int64 [R, L]: the column of each unprotected cell's head, -1 in protected cells)"""
    ids = np.asarray(ids, dtype=np.int64)
    R, L = ids.shape
    prot = np.isin(ids, np.asarray(sorted(set(int(x) for x in protected)), dtype=np.int64))
    cols = np.broadcast_to(np.arange(L, dtype=np.int64), (R, L))
    if not whole_word:
        return prot, np.where(prot, -1, cols)
    cont = np.isin(ids, np.asarray(cont_ids, dtype=np.int64)) & ~prot
    before = np.zeros((R, L), dtype=bool)
    before[:, 1:] = cont[:, :-1]                                     # cell c-1 is an unprotected continuation
    start = ~prot & ~before
    head = np.maximum.accumulate(np.where(start, cols, -1), axis=1)
    return prot, np.where(prot, -1, head)


def mask(ids, cont_ids, pad_id, bos_id, eos_id, mask_id, seed=0, t_sel=0, t1=0, t2=0, rand_lo=5, rand_hi=6, whole_word=True,
         row_base=0, ignore_index=-100):
    """dict(input_ids int32 [R, L], labels int32 [R, L], n_chosen int32 [R])"""
    ids = np.asarray(ids, dtype=np.int64)
    R, L = ids.shape
    assert 0 <= t_sel <= ONE and 0 <= t1 <= t2 <= ONE and rand_lo < rand_hi and row_base >= 0 and (row_base + R) * L < 2 ** 63
    prot, head = heads(ids, cont_ids, (pad_id, bos_id, eos_id, mask_id), whole_word)
    g = (np.uint64(row_base * L) + (np.arange(R, dtype=np.uint64) * np.uint64(L))[:, None] + np.arange(L, dtype=np.uint64)[None, :]) \
        if R else np.zeros((0, L), dtype=np.uint64)
    x0, x1, x2, _ = draw(g, seed)
    x0_head = np.take_along_axis(x0, np.maximum(head, 0), axis=1) if R else x0
    chosen = ~prot & (x0_head < np.uint64(t_sel))
    rand = (rand_lo + ((x2 * np.uint64(rand_hi - rand_lo)) >> S32).astype(np.int64))
    out = np.where(chosen & (x1 < np.uint64(t1)), mask_id, np.where(chosen & (x1 < np.uint64(t2)), rand, ids))
    labels = np.where(chosen, ids, ignore_index)
    return dict(input_ids=out.astype(np.int32), labels=labels.astype(np.int32), n_chosen=chosen.sum(axis=1).astype(np.int32))
