"""The BPE learner's rule in plain Python strings (include/genz_tokenize.h "learn"): what
genz_tokenize.learn_bpe must give, byte for byte.  `learn` recounts every pair in every step; `learn_incremental` keeps the counts
and, for a word that holds the best pair, takes its old pairs off and puts its new ones on -- the shape of the device's step.
Nothing here is fast and nothing here imports the package."""
from collections import Counter

END = "</w>"
CONT = "@@"
SPECIALS = ("<pad>", "<s>", "</s>", "<mask>", "<unk>")
HEADER = "#version: 0.2\n"


def word_counts(documents):
    """distinct str.split() words in first-occurrence order, and their counts"""
    c = Counter()
    for d in documents:
        c.update(d.split())
    return list(c), list(c.values())


def _key(s):
    return s.encode("utf-8", "surrogatepass")


def _initial(words):
    segs = []
    for w in words:
        s = list(w)
        s[-1] += END
        segs.append(s)
    ids = {s: i for i, s in enumerate(sorted({x for seg in segs for x in seg}, key=_key))}
    return segs, ids


def _merge_word(seg, l, r):
    out, k = [], 0
    while k < len(seg):
        if k + 1 < len(seg) and seg[k] == l and seg[k + 1] == r:
            out.append(l + r)
            k += 2
        else:
            out.append(seg[k])
            k += 1
    return out


def _best(n, ids):
    """largest count, then smallest (id_l, id_r); None when no pair has a count above 0"""
    best = None
    for (l, r), c in n.items():
        if c > 0 and (best is None or (-c, ids[l], ids[r]) < best[0]):
            best = ((-c, ids[l], ids[r]), (l, r), c)
    return best


def _files(segs, counts, merges):
    pieces = Counter()
    for seg, c in zip(segs, counts):
        for i, s in enumerate(seg):
            pieces[s[:-4] if i == len(seg) - 1 else s + CONT] += c
    for sp in SPECIALS:
        pieces.pop(sp, None)
    order = sorted(pieces.items(), key=lambda kv: (-kv[1], _key(kv[0])))
    vocab = "".join("%s %d\n" % kv for kv in order)
    codes = HEADER + "".join("%s %s\n" % m for m in merges)
    return _key(codes), _key(vocab)


class Learnt:
    def __init__(self, words, counts, segs, merges, n_symbols):
        self.words, self.counts, self.segs, self.merges, self.n_symbols = words, counts, segs, merges, n_symbols
        self.codes, self.vocab = _files(segs, counts, merges)

    def segmentation(self, word):
        return self.segs[self.words.index(word)]


def learn(words, counts, n_merges, min_frequency=2, reuse=True):
    """words: distinct strings without whitespace; counts: ints >= 1.  reuse=False gives a merged symbol a fresh id even when its
    string exists -- NOT the rule; the interning test shows the two differ."""
    segs, ids = _initial(words)
    merges = []
    fresh = len(ids)
    for _ in range(n_merges):
        n = Counter()
        for seg, c in zip(segs, counts):
            for a, b in zip(seg, seg[1:]):
                n[(a, b)] += c
        best = _best(n, ids)
        if best is None or best[2] < min_frequency:
            break
        l, r = best[1]
        merges.append((l, r))
        if not reuse or l + r not in ids:
            ids[l + r] = fresh
            fresh += 1
        segs = [_merge_word(seg, l, r) for seg in segs]
    return Learnt(list(words), list(counts), segs, merges, fresh)


def learn_incremental(words, counts, n_merges, min_frequency=2):
    segs, ids = _initial(words)
    merges = []
    n = Counter()
    for seg, c in zip(segs, counts):
        for a, b in zip(seg, seg[1:]):
            n[(a, b)] += c
    for _ in range(n_merges):
        best = _best(n, ids)
        if best is None or best[2] < min_frequency:
            break
        l, r = best[1]
        merges.append((l, r))
        ids.setdefault(l + r, len(ids))
        for k, (seg, c) in enumerate(zip(segs, counts)):
            if not any(a == l and b == r for a, b in zip(seg, seg[1:])):
                continue
            for a, b in zip(seg, seg[1:]):
                n[(a, b)] -= c
            seg = segs[k] = _merge_word(seg, l, r)
            for a, b in zip(seg, seg[1:]):
                n[(a, b)] += c
    return Learnt(list(words), list(counts), segs, merges, len(ids))


def learn_documents(documents, n_merges, min_frequency=2):
    w, c = word_counts(documents)
    return learn(w, c, n_merges, min_frequency)


def learn_indexed(words, counts, n_merges, min_frequency=2):
    """`learn_incremental` with an index from each pair to the words that hold it: the same files, fast enough to be timed on
    thousands of words and merges (tools/learn_bench.py)."""
    segs, ids = _initial(words)
    merges = []
    n = Counter()
    where = {}
    for k, (seg, c) in enumerate(zip(segs, counts)):
        for p in zip(seg, seg[1:]):
            n[p] += c
            where.setdefault(p, set()).add(k)
    for _ in range(n_merges):
        if not n:
            break
        (l, r), best = max(n.items(), key=lambda kv: (kv[1], -ids[kv[0][0]], -ids[kv[0][1]]))
        if best < 1 or best < min_frequency:
            break
        merges.append((l, r))
        ids.setdefault(l + r, len(ids))
        for k in sorted(where.get((l, r), ())):
            seg, c = segs[k], counts[k]
            if not any(a == l and b == r for a, b in zip(seg, seg[1:])):
                continue                                         # (an index entry may outlive the pair in that word)
            for p in zip(seg, seg[1:]):
                n[p] -= c
            seg = segs[k] = _merge_word(seg, l, r)
            for p in zip(seg, seg[1:]):
                n[p] += c
                where.setdefault(p, set()).add(k)
    return Learnt(list(words), list(counts), segs, merges, len(ids))
