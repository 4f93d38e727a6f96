"""The segmentation rule of include/genz_tokenize.h ("segment") in plain Python: `str.split`, the punctuation rule, a dict lexicon and
the recurrence over Python integers.  Nothing of the product is imported."""
import string

PUNCT = set(string.punctuation) - {"_"}
FOLDED = (set(range(0x41, 0x5B)) | (set(range(0xC0, 0xDF)) - {0xD7}) | {0x0102, 0x0110, 0x0128, 0x0168, 0x01A0, 0x01AF} | set(range(0x1EA0, 0x1EF9, 2)))


def fold(s):
    return "".join(c.lower() if ord(c) in FOLDED else c for c in s)


def tokens(doc, split_punct=True):
    out = []
    for piece in doc.split():
        if not split_punct:
            out.append(piece)
            continue
        lead = 0
        while lead < len(piece) and piece[lead] in PUNCT:
            lead += 1
        if lead == len(piece):
            out += list(piece)
            continue
        trail = 0
        while piece[len(piece) - 1 - trail] in PUNCT:
            trail += 1
        out += list(piece[:lead]) + [piece[lead:len(piece) - trail]] + list(piece[len(piece) - trail:])
    return out


def segment(doc, lex, K, unk, split_punct=True, fold_case=True):
    """lex: {entry (folded where fold_case): cost} -> (text, [n_tokens, n_words, n_known, cost], join list)"""
    tk = tokens(doc, split_punct)
    T = len(tk)
    best, pick = [0] + [None] * T, [None] * (T + 1)
    for i in range(1, T + 1):
        for k in range(1, min(K, i) + 1):
            key = "_".join(tk[i - k:i])
            cost = lex.get(fold(key) if fold_case else key)
            known = cost is not None
            if not known:
                if k > 1:
                    continue
                cost = unk
            v = best[i - k] + cost
            if best[i] is None or v <= best[i]:
                best[i], pick[i] = v, (k, known)
    join, words, n_known, i = [0] * T, [], 0, T
    while i > 0:
        k, known = pick[i]
        words.append("_".join(tk[i - k:i]))
        for j in range(i - k, i - 1):
            join[j] = 1
        n_known += known
        i -= k
    return " ".join(reversed(words)), [T, len(words), n_known, best[T]], join


def leftmost_longest(doc, lex, K, unk, split_punct=True):
    """greedy maximal matching, what the dynamic programme is compared with: (text, cost)"""
    tk, i, words, cost = tokens(doc, split_punct), 0, [], 0
    while i < len(tk):
        for k in range(min(K, len(tk) - i), 0, -1):
            c = lex.get(fold("_".join(tk[i:i + k])))
            if c is not None or k == 1:
                words.append("_".join(tk[i:i + k])); cost += unk if c is None else c; i += k
                break
    return " ".join(words), cost
