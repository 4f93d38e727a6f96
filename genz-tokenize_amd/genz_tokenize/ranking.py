"""Drop-in for genz_tokenize/ranking.py: BM25 and BM25Plus with the index built and the scores computed on the GPU.

Same attributes, methods and results as the reference, to the bit: `b`, `k1`, `delta`, `num_doc`, `fieldLens`, `avgFieldLen`,
`cal_idf`, `get_score`.  The constructor packs the documents and builds a device index (csrc/gz_bm25.inc): words by str.split(),
term ids by exact bytes, document frequencies, per-document term counts.  Scoring is one launch for a whole batch of queries
(`get_scores`, the form meant for real work); `get_score` is a batch of one.  There is no CPU fallback.

Retrieval: `top_k(queries, k)` returns the ids and scores of every query's k best documents and `get_top_n(query, documents, n)`
those documents (rank_bm25's form).  The score rows are computed and searched on the GPU (csrc/gz_topk.inc): only [Q, k] ids and
scores come back.  The order is total: higher scores first, ties to the lower document index, NaN last.

Search: `search(queries, k)` ranks only the documents that MATCH a query -- those that hold at least one of its words -- and
tells how many match; `count_matches(queries)` only counts.  The matching documents come from term-major postings on the GPU
(csrc/gz_search.inc), built by the first search and again after the index changes; only they are scored and ranked, so a query of
rare words does not pay for the whole corpus.  The ranked documents are exactly `top_k`'s order with the other documents left
out; unlike `top_k`, a row is never filled up with documents that hold none of the query's words (with BM25Plus those have positive
scores too): unfilled positions hold id -1 and NaN.

Boolean search: `search(queries, k, match="all")` keeps only the documents that hold EVERY word of the query, and
`exclude=[...]` (one string of words per query, with either match) drops the documents that hold any of those words; both also on
`count_matches`.  The device marks only the postings of each query's rarest word and a filter kernel clears, from those documents,
the ones that lack a word or hold an excluded one (gz_bm25_search_bool).  Scores, order and padding are those of `search`; excluded
words never enter a score.  With the defaults the call is the plain search, unchanged.

Phrase search: an index built with `positions=True` additionally keeps, on the GPU, the term id of every word of every document
in order (`seq`, uint32 [all words]; document d is seq[woff[d]:woff[d+1]] with woff the scan of fieldLens, derived on the device
when first needed; `term_sequences()` reads both back), and `add_documents`, `remove_documents` and `compact` maintain it like
every other array of the index.  Such an index never needs the documents' text again, so its build ends in the form `compact()`
gives (the text copy holds the terms' bytes only): a compacted positional index equals a fresh positional build of its documents,
`footprint()` included.  `search(queries, k, phrase=[...])` (one string per query, with either match and with exclude; also
on `count_matches`) then keeps only the documents in which the phrase's words stand next to each other in this order:
`documents[d].split()[i:i+len(P)] == P` for some i.  One more kernel behind the marking and the filter (gz_bm25_sr_phrase_kernel)
rejects a marked document that lacks a phrase word, else walks its slice of seq.  The phrase is a filter only: its words enter no
score.  An index built without positions is the same index as before, buffer for buffer, and refuses `phrase=` with ValueError.

Snippets: a positional index also tells where INSIDE a document the query's words stand -- the second reader of `seq`, and what
a result page needs.  `snippets(queries, ids, width)` takes the ids `search` or `top_k` returned ([Q, k]; -1 is the padding) and
gives, for every (query, document) pair, the window of `width` words that holds the most query words: the smallest start among the
best windows, and that count.  `occurrences(queries, ids)` lists every position of a query word in those documents, with the word's
first place in the query, pair after pair.  Both walk the documents' slices of seq on the GPU (csrc/gz_snippet.inc), a wave per
pair; nothing but the word offsets is derived for them -- no postings -- and the index may be in any state.
`snippet_texts(queries, ids, width, mark)` joins the windows' words on the host, splitting only the texts of the ids it was given,
and wraps the query's words in `mark`.  An index built without positions refuses all three with ValueError.

Proximity: the third reader of `seq` answers "these words close to each other, in any order" and its dual, "the shortest passage
that holds them".  `search_near(queries, k, near, window)` is `search` (with match, exclude and phrase as there) restricted to the
documents in which some `window[q]` consecutive words hold every word of `near[q]`; `count_near(queries, near, window)` only counts.
The near words are a set and a filter only -- they enter no score; a window never reaches into a neighbouring document, and a
window as long as the document means "holds all of them".  One more kernel behind the phrase stage (gz_bm25_sr_near_kernel,
csrc/gz_near.inc) rejects a marked document that lacks a near word, else walks its slice of seq with the near terms in the lanes:
per term a ballot of its occurrences and a carry across trips give every position the shortest window that ends there.
`cover(queries, ids)` runs the same walk per (query, document) pair, a wave each, and gives the shortest window that holds every
distinct query word the document holds at all -- the smallest start among the shortest -- with the number of those words.  At most
64 distinct words per near set or cover query; an index built without positions refuses all three with ValueError.

Growth: `add_documents(more)` appends to the live index on the GPU (gz_bm25_append): afterwards the object behaves exactly like
one constructed over the old and the new documents together, without the old documents being packed, copied or indexed again.

Deletion: `remove_documents(ids)` takes documents out of the live index on the GPU (gz_bm25_remove): afterwards the object behaves
exactly like one constructed over the remaining documents, which are renumbered in their old order.  An update is a removal
followed by an `add_documents`.

Compaction: a removal leaves the index's copy of the text, its term table (terms no document has any more) and its buffers'
capacities as they were, and every append adds its whole batch to the text copy.  `compact()` rebuilds text and term table on the
GPU from the index itself (gz_bm25_compact): afterwards the index is the one a fresh build of the current documents gives -- term
ids and device memory included -- without any string being packed, tokenised or hashed again.  `footprint()` tells when that is
worth it, and `vocabulary()` reads the current words and their document frequencies (gz_bm25_terms) in any state of the index.

Vocabulary lookup: everything above starts from an exact, byte-for-byte lookup of the query's words, so a word that is one letter
off -- `cong nghe` for `công nghệ`, a dropped tone mark, half a word -- matches nothing.  `similar_words(words, max_edits, k)`
gives, for every word, the terms of the index within `max_edits` edits of it (Levenshtein distance over code points), the closest
first, the more frequent first among equally close ones, with distances, document frequencies and the number of such terms;
`prefix_words(prefixes, k)` the most frequent terms that start with a prefix.  Both compare every word with every live term on the
GPU (csrc/gz_vocab.inc: a bit-parallel distance recurrence with the query word as the pattern, a lane per term, hence at most 64
code points a word) and select the k best with `top_k`'s selection; the ids are `vocabulary()`'s in any state of the index, which
is not modified.  `term_texts(ids)` reads back the words of given ids only.  `suggest`, `complete` and `correct(queries)` compose
them on the host: (word, distance, df) lists, (word, df) lists, and the queries with every unknown word replaced by its best match.
`search` itself stays exact: pass it `correct(queries)` to search for what was meant.

Word groups: `correct` replaces a word by ONE guess.  `search_groups(groups, k, match, exclude)` searches for a word "in some
spelling" instead: a query is a list of groups, a group a list of alternative words that count as one query word -- a document
holds the group when it holds any alternative, the group's f is the sum of their counts and its df the number of documents that
hold any of them, so the variants share one idf (`group_df`, cached per group on the host) and a misspelling that is rare in the
corpus does not outrank the correct word by its idf.  match="all" is an AND of ORs.  On the GPU (csrc/gz_groups.inc) the flat
alternative list is marked like a word list; with match="all" only the group with the smallest sum of postings-list lengths (an
upper bound of its union), and a filter and a score kernel add up a group's alternatives per document behind a 256-bit mask of the
group's signature bits (gz_bm25_search_groups); everything behind the bitmap is `search`'s.  With singleton groups the result is
`search`'s, bit for bit.  `count_groups` only counts.  `expand(queries, max_edits, limit, only_unknown, prefix_last)` builds the
groups from `similar_words` / `prefix_words` (fuzzy words; the last word as a prefix), and `search_fuzzy(queries, k, ...)` is
`search_groups(expand(...))`: `cong nghe` retrieves the documents with `công nghệ`, `cộng nghệ`, ... ranked together.  At most
64 distinct alternatives a group; `phrase=` and `near` do not combine with groups.

What stays on the host, as in the reference: `avgFieldLen = np.mean(fieldLens)` and every idf, computed per query word by the
reference's scalar expression `np.log(1+(N-df+0.5)/(df+0.5))` (np.log is not correctly rounded, and its scalar and array loops may
differ by an ulp: the device never computes a logarithm).  `documents` (the word lists) and `frequency_word_in_doc` (dicts in
first-occurrence order) are built on the host on first access only: they are not on the hot path.

Deviation: documents and queries must be `str` (TypeError otherwise); the reference takes anything with `.split()`.
"""
import itertools
import numbers
import weakref
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from ._packing import pack as _pack

_ctx: Optional[_native.Context] = None


def _context() -> _native.Context:
    global _ctx
    if _ctx is None:
        _ctx = _native.Context()
    return _ctx


def _strings(items, what: str) -> list:
    items = list(items)
    for x in items:
        if not isinstance(x, str):
            raise TypeError("%s must be str, not %s" % (what, type(x).__name__))
    return items


class BM25:
    def __init__(self, documents: List, b: float = 0.75, k1: float = 1.2, ctx: Optional[_native.Context] = None,
                 positions: bool = False) -> None:
        self.b = b
        self.k1 = k1
        self._texts = _strings(documents, "documents")
        self._ctx = ctx or _context()
        self._positions = bool(positions)
        buf, off = _pack(self._texts)
        self._index = self._ctx.bm25_build(buf, off, positions=True) if self._positions else self._ctx.bm25_build(buf, off)
        # (the finalizer holds the context: the index is freed before it)
        self._finalizer = weakref.finalize(self, self._ctx.bm25_destroy, self._index)
        self.num_doc = len(self._texts)
        lens = self._ctx.bm25_field_lengths(self._index)
        self.fieldLens = lens.tolist()
        self.avgFieldLen = np.mean(lens)                         # ranking.py:27 (nan and a RuntimeWarning for no documents)
        self._idf = {}
        self._documents = None
        self._freq = None

    # ---- growth -----------------------------------------------------------------------------------------------------
    def add_documents(self, documents: Sequence[str]) -> None:
        """Append documents: afterwards self equals type(self)(old documents + list(documents), ...) built fresh -- num_doc,
        fieldLens, avgFieldLen, idf, scores and top-k to the bit.  TypeError (an item that is no str) and _native.GzError leave the
        object as it was."""
        more = _strings(documents, "documents")
        if not more:
            return
        buf, off = _pack(more)
        self._ctx.bm25_append(self._index, buf, off)
        old = self.num_doc
        self._texts.extend(more)
        self.num_doc = len(self._texts)
        lens = self._ctx.bm25_field_lengths(self._index)
        self.fieldLens.extend(lens[old:].tolist())
        self.avgFieldLen = np.mean(lens)                         # (the constructor's expression over all the lengths)
        self._idf.clear()                                        # N and df changed
        self.__dict__.pop("_group_idf", None)                    # (the word groups' df and idf: search_groups)
        if self._documents is not None:
            self._documents.extend(t.split() for t in more)
        self._freq = None                                        # (rebuilt on the next access)

    def remove_documents(self, ids) -> None:
        """Remove the documents with these ids (any iterable of ints; any order, duplicates allowed): afterwards self equals
        type(self)(remaining documents, ...) built fresh -- num_doc, fieldLens, avgFieldLen, idf, scores and top-k to the bit.  The
        remaining documents keep their order; new id = old id - the number of removed documents before it.  TypeError (an item
        that is no int), IndexError (an id outside [0, num_doc)) and _native.GzError leave the object as it was."""
        gone = set()
        for i in ids:
            if isinstance(i, bool) or not isinstance(i, numbers.Integral):
                raise TypeError("document ids must be int, not %s" % type(i).__name__)
            gone.add(int(i))
        for i in gone:
            if not 0 <= i < self.num_doc:
                raise IndexError("document id %d is out of range for %d documents" % (i, self.num_doc))
        if not gone:
            return
        ids = np.fromiter(sorted(gone), dtype=np.int64, count=len(gone))
        self._ctx.bm25_remove(self._index, ids)
        keep = np.ones(self.num_doc, dtype=bool)
        keep[ids] = False
        keep = keep.tolist()
        self._texts = list(itertools.compress(self._texts, keep))
        self.num_doc = len(self._texts)
        lens = self._ctx.bm25_field_lengths(self._index)
        self.fieldLens = lens.tolist()
        self.avgFieldLen = np.mean(lens)                         # (nan and a RuntimeWarning when nothing is left, as BM25([]))
        self._idf.clear()                                        # N and df changed
        self.__dict__.pop("_group_idf", None)                    # (the word groups' df and idf: search_groups)
        if self._documents is not None:
            self._documents = list(itertools.compress(self._documents, keep))
        self._freq = None                                        # (rebuilt on the next access)

    # ---- upkeep and the vocabulary -----------------------------------------------------------------------------------
    def compact(self) -> None:
        """Rebuild text copy and term table on the GPU: afterwards the index equals a fresh build of the current documents, term ids
        and buffer sizes included.  Nothing observable through this object changes: N and every df stay, so do fieldLens,
        avgFieldLen and the idf cache.  _native.GzError leaves the index as it was."""
        self._ctx.bm25_compact(self._index)

    def vocabulary(self):
        """(words, df): the distinct words of the current documents as a list of str, in the order of their first occurrence, and
        an int32 array of their document frequencies.  words[i] is the term that has id i once the index is compacted.  The index
        is not modified."""
        off, data, df = self._ctx.bm25_terms(self._index)
        raw = data.tobytes()
        off = off.tolist()
        return [raw[off[i]:off[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(off) - 1)], df

    def term_sequences(self):
        """(terms int32 [all words], offsets int64 [num_doc + 1]) of an index built with positions=True: the term id of every word,
        documents in id order, words in str.split() order; document d is terms[offsets[d]:offsets[d + 1]].  The ids are those
        `_lookup` answers; on a compacted (or freshly built) index vocabulary()[0][terms[i]] is the i-th word.  ValueError on an
        index without positions."""
        if not getattr(self, "_positions", False):
            raise ValueError("the index was built without positions=True")
        return self._ctx.bm25_sequence(self._index)

    def footprint(self) -> dict:
        """{"text_bytes": bytes of the index's text copy (what the 2^32 limit of add_documents counts), "table_terms": terms held in
        the term table, dead ones included, "device_bytes": device memory allocated to the index}"""
        t, n, d = self._ctx.bm25_footprint(self._index)
        return {"text_bytes": t, "table_terms": n, "device_bytes": d}

    # ---- words that look like a given one: typo-tolerant and prefix lookup over the vocabulary --------------------------
    @staticmethod
    def _edits(max_edits) -> int:
        if isinstance(max_edits, bool) or not isinstance(max_edits, numbers.Integral):
            raise TypeError("max_edits must be int, not %s" % type(max_edits).__name__)
        max_edits = int(max_edits)
        if not 0 <= max_edits <= _native.GZ_BM25_EDIT_MAX:
            raise ValueError("max_edits must lie in [0, %d], not %d" % (_native.GZ_BM25_EDIT_MAX, max_edits))
        return max_edits

    def _n_terms(self) -> int:
        """T = len(vocabulary()[0]): host bookkeeping of the index, no device work"""
        return self._ctx.bm25_info(self._index)[1]

    def similar_words(self, words: Sequence[str], max_edits: int = 2, k: int = 10):
        """(ids int64 [W, k'], dist int32 [W, k'], df int32 [W, k'], counts int64 [W]), k' = min(k, T) with V, DF = vocabulary() and
        T = len(V).  With ed(a, b) the Levenshtein distance of two str as sequences of code points (unit-cost insertion, deletion,
        substitution; no transposition; a lone surrogate is one code point): the matching terms of words[w] are
        {i : ed(words[w], V[i]) <= max_edits}, counts[w] is their number (it may exceed k') and row w holds the first k' of
        sorted(matching, key=lambda i: (ed(words[w], V[i]), -DF[i], i)) with their distances and document frequencies; positions from
        counts[w] on hold id -1, dist -1, df 0.  A word of the vocabulary comes first with distance 0; "" is a word like any other
        (its distance to a term is the term's length); the words are not split.  The ids index vocabulary() in any state of the
        index -- after appends and removals too -- and are `_lookup`'s once it is compacted.  Every word is compared with every
        live term on the GPU and the rows are selected there; the index is not modified.  TypeError: a word that is no str, k or
        max_edits that is bool or no int; ValueError: k < 1, max_edits outside [0, 64]; _native.GzError (GZ_E_LIMIT): a word of
        more than 64 code points, k' above 1024."""
        words = _strings(words, "words")
        max_edits = self._edits(max_edits)
        k = self._k(k)
        kk = min(k, self._n_terms())
        if not words:
            return (np.zeros((0, kk), dtype=np.int64), np.zeros((0, kk), dtype=np.int32), np.zeros((0, kk), dtype=np.int32),
                    np.zeros(0, dtype=np.int64))
        buf, off = _pack(words)
        return self._ctx.bm25_similar(self._index, buf, off, max_edits, k)

    def prefix_words(self, prefixes: Sequence[str], k: int = 10):
        """(ids int64 [W, k'], df int32 [W, k'], counts int64 [W]): as `similar_words` for the terms with
        V[i].startswith(prefixes[w]), in the order (-DF[i], i) -- the most frequent completions first.  "" matches every term."""
        prefixes = _strings(prefixes, "prefixes")
        k = self._k(k)
        kk = min(k, self._n_terms())
        if not prefixes:
            return np.zeros((0, kk), dtype=np.int64), np.zeros((0, kk), dtype=np.int32), np.zeros(0, dtype=np.int64)
        buf, off = _pack(prefixes)
        return self._ctx.bm25_prefix(self._index, buf, off, k)

    def term_texts(self, ids) -> list:
        """The words with these ids of vocabulary()'s numbering (what similar_words / prefix_words return): any integer array or
        nesting of lists of ids gives the same nesting of str, id -1 gives "".  Only the requested terms' bytes are gathered on the
        GPU and copied back; the vocabulary is not read.  TypeError: ids that are no integers; IndexError: an id outside [-1, T)."""
        if isinstance(ids, np.ndarray):
            if ids.dtype == np.bool_ or not np.issubdtype(ids.dtype, np.integer):
                raise TypeError("ids must be integers, not %s" % ids.dtype)
            ids = ids.tolist()
        flat = []

        def walk(x):
            if isinstance(x, (list, tuple)):
                return [walk(y) for y in x]
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise TypeError("ids must be integers, not %s" % type(x).__name__)
            flat.append(int(x))
            return len(flat) - 1

        nest = walk(ids)
        if flat:
            n_terms = self._n_terms()
            if min(flat) < -1 or max(flat) >= n_terms:
                raise IndexError("term ids must lie in [-1, %d)" % n_terms)
            off, data = self._ctx.bm25_term_bytes(self._index, np.array(flat, dtype=np.int64))
            raw, off = data.tobytes(), off.tolist()
            texts = [raw[off[i]:off[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(flat))]

        def fill(x):
            return [fill(y) for y in x] if isinstance(x, list) else texts[x]

        return fill(nest)

    def suggest(self, words: Sequence[str], max_edits: int = 2, k: int = 10) -> list:
        """A list of W lists of (word, distance, df): `similar_words` with the ids as `term_texts` spells them, without the padding."""
        ids, dist, df, counts = self.similar_words(words, max_edits, k)
        texts = self.term_texts(ids)
        return [list(zip(t[:c], d[:c], f[:c])) for t, d, f, c in zip(texts, dist.tolist(), df.tolist(), counts.tolist())]

    def complete(self, prefixes: Sequence[str], k: int = 10) -> list:
        """A list of W lists of (word, df): `prefix_words` with the ids as `term_texts` spells them, without the padding."""
        ids, df, counts = self.prefix_words(prefixes, k)
        texts = self.term_texts(ids)
        return [list(zip(t[:c], f[:c])) for t, f, c in zip(texts, df.tolist(), counts.tolist())]

    def correct(self, queries: Sequence[str], max_edits: int = 2) -> list:
        """A list of str: " ".join over q.split() of every query, a word the index holds kept, any other replaced by its best
        `similar_words` match (the smallest (distance, -df, id) within max_edits) when there is one, else kept.  One lookup and one
        similar_words call for the whole batch."""
        split = [q.split() for q in _strings(queries, "queries")]
        max_edits = self._edits(max_edits)
        words = [w for ws in split for w in ws]
        fixed = {}
        if words:
            terms = self._lookup(words)[0].tolist()
            unknown = list(dict.fromkeys(w for w, t in zip(words, terms) if t < 0))
            ids, _, _, counts = self.similar_words(unknown, max_edits, 1)
            if unknown and ids.shape[1]:
                best = self.term_texts(ids[:, 0])
                fixed = {w: b for w, b, c in zip(unknown, best, counts.tolist()) if c}
        return [" ".join(fixed.get(w, w) for w in ws) for ws in split]

    # ---- the reference's per-document lists, built lazily on the host -------------------------------------------------
    @property
    def documents(self):
        """document.split() of every document (ranking.py:17-18)."""
        if self._documents is None:
            self._documents = [t.split() for t in self._texts]
        return self._documents

    @property
    def frequency_word_in_doc(self):
        """{word: count} per document, in first-occurrence order (ranking.py:22-26)."""
        if self._freq is None:
            out = []
            for words in self.documents:
                f = {}
                for w in words:
                    f[w] = f.get(w, 0) + 1
                out.append(f)
            self._freq = out
        return self._freq

    # ---- scoring ----------------------------------------------------------------------------------------------------
    def _params(self):
        delta = getattr(self, "delta", 0.0)
        return [float(self.k1 + 1), float(self.k1), float(1 - self.b), float(self.b), float(self.avgFieldLen), float(delta)]

    def _idf_of(self, q: str, df: int):
        v = self._idf.get(q)
        if v is None:
            v = self._idf[q] = np.log(1+(self.num_doc-df+0.5)/(df+0.5))          # ranking.py:31, a scalar np.log
        return v

    def _lookup(self, words: Sequence[str]):
        buf, off = _pack(list(words))
        return self._ctx.bm25_lookup(self._index, buf, off)

    def cal_idf(self, q: str) -> float:
        if not isinstance(q, str):
            raise TypeError("q must be str, not %s" % type(q).__name__)
        _, df = self._lookup([q])
        return self._idf_of(q, int(df[0]))

    def _queries(self, queries: Sequence[str]):
        """str.split() of every query -> (query count, term ids, host idf of every word, int64 query offsets)."""
        split = [q.split() for q in _strings(queries, "queries")]
        qoff = np.zeros(len(split) + 1, dtype=np.int64)
        if split:
            np.cumsum([len(w) for w in split], out=qoff[1:])
        words = [w for ws in split for w in ws]
        terms, df = self._lookup(words) if words else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        idf = np.array([self._idf_of(w, int(d)) for w, d in zip(words, df.tolist())], dtype=np.float64)
        return len(split), terms, idf, qoff

    def get_scores(self, queries: Sequence[str]) -> np.ndarray:
        """float64 [len(queries), num_doc]: row q is get_score(queries[q]) (0.0 for a query without words)."""
        nq, terms, idf, qoff = self._queries(queries)
        if not nq or self.num_doc == 0:
            return np.zeros((nq, self.num_doc), dtype=np.float64)
        plus = isinstance(self, BM25Plus)
        return self._ctx.bm25_score(self._index, terms, idf, qoff, self._params(), plus)

    def top_k(self, queries: Sequence[str], k: int):
        """(ids int64 [len(queries), k'], scores float64 [len(queries), k']), k' = min(k, num_doc): row q holds the k' best documents
        of queries[q], np.argsort(-get_scores(queries)[q], kind="stable")[:k'] and their scores (original bits).  Higher scores first,
        +0.0 and -0.0 tie, NaN below every number, ties to the lower document index.  Selected on the GPU: the score rows never
        leave device memory.  k' above 1024 raises _native.GzError (GZ_E_LIMIT)."""
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise TypeError("k must be int, not %s" % type(k).__name__)
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1, not %d" % k)
        nq, terms, idf, qoff = self._queries(queries)
        plus = isinstance(self, BM25Plus)
        return self._ctx.bm25_topk(self._index, terms, idf, qoff, self._params(), plus, k)

    @staticmethod
    def _k(k) -> int:
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise TypeError("k must be int, not %s" % type(k).__name__)
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1, not %d" % k)
        return k

    @staticmethod
    def _match(match) -> int:
        if not isinstance(match, str):
            raise TypeError("match must be str, not %s" % type(match).__name__)
        if match not in ("any", "all"):
            raise ValueError('match must be "any" or "all", not %r' % match)
        return 1 if match == "all" else 0

    def _exclusions(self, exclude, nq: int):
        """str.split() of every exclude[q] -> (term ids, int64 offsets); (None, None) for exclude=None.  A word no document holds
        has term -1, which the search ignores."""
        split = [x.split() for x in exclude]
        xoff = np.zeros(nq + 1, dtype=np.int64)
        if split:
            np.cumsum([len(w) for w in split], out=xoff[1:])
        words = [w for ws in split for w in ws]
        terms = self._lookup(words)[0] if words else np.zeros(0, np.int32)
        return terms, xoff

    def _bool_args(self, queries, match, exclude, phrase=None):
        """validation of search / count_matches, all of it before any native call -> (queries, mode, exclude, phrase)"""
        mode = self._match(match)
        queries = _strings(queries, "queries")
        if exclude is not None:
            exclude = _strings(exclude, "exclude")
            if len(exclude) != len(queries):
                raise ValueError("exclude has %d items for %d queries" % (len(exclude), len(queries)))
        if phrase is not None:
            phrase = _strings(phrase, "phrase")
            if len(phrase) != len(queries):
                raise ValueError("phrase has %d items for %d queries" % (len(phrase), len(queries)))
            if not getattr(self, "_positions", False):
                raise ValueError("phrase needs an index built with positions=True")
        return queries, mode, exclude, phrase

    def search(self, queries: Sequence[str], k: int, match: str = "any", exclude: Optional[Sequence[str]] = None,
               phrase: Optional[Sequence[str]] = None):
        """(ids int64 [len(queries), k'], scores float64 [len(queries), k'], counts int64 [len(queries)]), k' = min(k, num_doc).
        With R = set(queries[q].split()), X = set(exclude[q].split()) (empty for exclude=None) and W(d) the words of document d:
        match="any": d matches q iff R & W(d) and not X & W(d); match="all": d matches iff R and R <= W(d) and not X & W(d) (a query
        without words, or with a word that no document holds, matches nothing).  A word both in R and in X excludes every document
        that holds it.  Excluded words never enter a score or an idf.  counts[q] is the number of matching documents
        (it may exceed k; a repeated query word counts once).  Row q holds the best matching documents in top_k's order:
        [i for i in np.argsort(-get_scores(queries)[q], kind="stable") if d_i matches][:k'] and their scores (original bits);
        positions from counts[q] on hold id -1 and NaN (bits 0x7FF8000000000000).  Only the matching documents are scored, on the
        GPU; with match="all" only the documents of each query's rarest word are looked at.  k' above 1024 raises
        _native.GzError (GZ_E_LIMIT).  exclude: None or one str per query (ValueError for another length).
        phrase: None or one str per query (ValueError for another length, or on an index built without positions=True).  With
        P = phrase[q].split(), d matches iff it matches as above AND (P is empty or documents[d].split()[i:i+len(P)] == P for some
        i): a phrase word that no document holds matches nothing, a one-word phrase means "holds this word", a phrase never
        matches across two documents.  The phrase is a filter only -- its words enter no score and no idf; put them into the
        query to have them scored.  More than 64 words in a phrase raise _native.GzError (GZ_E_LIMIT)."""
        k = self._k(k)
        queries, mode, exclude, phrase = self._bool_args(queries, match, exclude, phrase)
        nq, terms, idf, qoff = self._queries(queries)
        plus = isinstance(self, BM25Plus)
        xterms, xoff = self._exclusions(exclude, nq) if exclude is not None else (None, None)
        # (the same packing for a phrase: term -1 for a word no document holds)
        pterms, poff = self._exclusions(phrase, nq) if phrase is not None else (None, None)
        return self._ctx.bm25_search(self._index, terms, idf, qoff, self._params(), plus, k, mode=mode, ex_terms=xterms, ex_off=xoff,
                                     ph_terms=pterms, ph_off=poff)

    def count_matches(self, queries: Sequence[str], match: str = "any", exclude: Optional[Sequence[str]] = None,
                      phrase: Optional[Sequence[str]] = None) -> np.ndarray:
        """int64 [len(queries)]: counts of search(queries, k, match, exclude, phrase) alone.  With the defaults: the documents that
        hold at least one word of each query; for a query of one word, its df."""
        queries, mode, exclude, phrase = self._bool_args(queries, match, exclude, phrase)
        nq, terms, _, qoff = self._queries(queries)
        xterms, xoff = self._exclusions(exclude, nq) if exclude is not None else (None, None)
        pterms, poff = self._exclusions(phrase, nq) if phrase is not None else (None, None)
        return self._ctx.bm25_match_count(self._index, terms, qoff, mode=mode, ex_terms=xterms, ex_off=xoff, ph_terms=pterms, ph_off=poff)

    # ---- word groups: alternatives that count as one query word; fuzzy and prefix search over them -----------------------
    def _group_args(self, groups, match, exclude):
        """validation of search_groups / count_groups / group_df, all of it before any native call -> (groups as lists of lists of
        lists of str, mode, exclude)"""
        mode = self._match(match)
        if isinstance(groups, (str, bytes)):
            raise TypeError("groups must be a list of queries, not %s" % type(groups).__name__)
        out = []
        for query in groups:
            if isinstance(query, (str, bytes)) or not isinstance(query, (list, tuple)):
                raise TypeError("a query must be a list of groups, not %s" % type(query).__name__)
            gs = []
            for group in query:
                if isinstance(group, (str, bytes)) or not isinstance(group, (list, tuple)):
                    raise TypeError("a group must be a list of str, not %s" % type(group).__name__)
                gs.append(_strings(group, "alternatives"))
            out.append(gs)
        if exclude is not None:
            exclude = _strings(exclude, "exclude")
            if len(exclude) != len(out):
                raise ValueError("exclude has %d items for %d queries" % (len(exclude), len(out)))
        return out, mode, exclude

    def _group_arrays(self, groups):
        """validated groups -> ({alternative: (term id, df)}, the groups one after the other, alt_terms int32, alt_off int64 [G + 1],
        group_off int64 [Q + 1]): one lookup of the distinct alternatives; -1 and repeats stay in alt_terms, the library drops them"""
        words = list(dict.fromkeys(a for q in groups for g in q for a in g))
        if words:
            terms, dfs = self._lookup(words)
            known = {w: (t, d) for w, t, d in zip(words, terms.tolist(), dfs.tolist())}
        else:
            known = {}
        flat = [g for q in groups for g in q]
        alt_terms = np.array([known[a][0] for g in flat for a in g], dtype=np.int32)
        alt_off = np.zeros(len(flat) + 1, dtype=np.int64)
        if flat:
            np.cumsum([len(g) for g in flat], out=alt_off[1:])
        group_off = np.zeros(len(groups) + 1, dtype=np.int64)
        if groups:
            np.cumsum([len(q) for q in groups], out=group_off[1:])
        return known, flat, alt_terms, alt_off, group_off

    def _group_pack(self, groups):
        """validated groups -> (alt_terms int32, alt_off int64 [G + 1], group_off int64 [Q + 1], df list [G], idf float64 [G]).
        The df of a group with several known alternatives is a match count ("any") of them as a query, one call for all such
        groups that the cache does not hold; a group with one known alternative has its df."""
        known, flat, alt_terms, alt_off, group_off = self._group_arrays(groups)
        cache = self.__dict__.setdefault("_group_idf", {})
        keys, pending = [], {}
        for g in flat:
            key = frozenset(a for a in g if known[a][0] >= 0)
            keys.append(key)
            if key not in cache and key not in pending:
                if len(key) == 0:
                    pending[key] = 0
                elif len(key) == 1:
                    pending[key] = known[next(iter(key))][1]
                else:
                    pending[key] = None
        multi = [key for key, v in pending.items() if v is None]
        if multi:
            lists = [[known[a][0] for a in key] for key in multi]
            moff = np.zeros(len(lists) + 1, dtype=np.int64)
            np.cumsum([len(x) for x in lists], out=moff[1:])
            counts = self._ctx.bm25_match_count(self._index, np.array([t for x in lists for t in x], dtype=np.int32), moff)
            for key, c in zip(multi, counts.tolist()):
                pending[key] = c
        for key, df in pending.items():
            cache[key] = (df, np.log(1+(self.num_doc-df+0.5)/(df+0.5)))            # ranking.py:31 with the group's df
        df = [cache[key][0] for key in keys]
        idf = np.array([cache[key][1] for key in keys], dtype=np.float64)
        return alt_terms, alt_off, group_off, df, idf

    def search_groups(self, groups, k: int, match: str = "any", exclude: Optional[Sequence[str]] = None):
        """`search` over WORD GROUPS: groups[q] is a list of groups and a group a list of alternative words (str, looked up as given,
        never split) that count as ONE query word.  With A_g the distinct alternatives of group g that the index holds and c(a, d)
        the count of word a in document d: f_g(d) = sum(c(a, d) for a in A_g), df_g = #{d : f_g(d) > 0} and
        idf_g = np.log(1+(N-df_g+0.5)/(df_g+0.5)); the score is get_score's sum with group g where a word stands (f_g, idf_g; groups
        in order, a group listed twice summed twice).  match="any": d matches iff some f_g(d) > 0; match="all": iff there is a group
        and every f_g(d) > 0.  A group without a known alternative is a word that no document holds.  exclude, the outputs
        (ids, scores, counts), their order and padding are `search`'s; with every group a single word the result equals
        search(queries, k, match, exclude) bit for bit.  A misspelling that is rare in the corpus therefore does not outrank the
        correct spelling by its idf: the variants share one df.  At most 64 distinct known alternatives a group (_native.GzError,
        GZ_E_LIMIT).  TypeError: an alternative that is no str, a str where a list is due; ValueError: a bad match, an exclude of
        another length -- all before any native call."""
        k = self._k(k)
        groups, mode, exclude = self._group_args(groups, match, exclude)
        alt_terms, alt_off, group_off, _, idf = self._group_pack(groups)
        xterms, xoff = self._exclusions(exclude, len(groups)) if exclude is not None else (None, None)
        plus = isinstance(self, BM25Plus)
        return self._ctx.bm25_search_groups(self._index, alt_terms, alt_off, idf, group_off, self._params(), plus, k, mode=mode,
                                            ex_terms=xterms, ex_off=xoff)

    def count_groups(self, groups, match: str = "any", exclude: Optional[Sequence[str]] = None) -> np.ndarray:
        """int64 [len(groups)]: counts of search_groups(groups, k, match, exclude) alone."""
        groups, mode, exclude = self._group_args(groups, match, exclude)
        _, _, alt_terms, alt_off, group_off = self._group_arrays(groups)
        xterms, xoff = self._exclusions(exclude, len(groups)) if exclude is not None else (None, None)
        return self._ctx.bm25_match_count_groups(self._index, alt_terms, alt_off, group_off, mode=mode, ex_terms=xterms, ex_off=xoff)

    def group_df(self, groups) -> list:
        """df_g of every group, in the nesting of `groups` without the innermost level: the documents that hold at least one of
        the group's alternatives."""
        groups, _, _ = self._group_args(groups, "any", None)
        df = self._group_pack(groups)[3]
        it = iter(df)
        return [[next(it) for _ in q] for q in groups]

    @staticmethod
    def _limit(limit) -> int:
        if isinstance(limit, bool) or not isinstance(limit, numbers.Integral):
            raise TypeError("limit must be int, not %s" % type(limit).__name__)
        limit = int(limit)
        if not 1 <= limit <= _native.GZ_BM25_GROUP_MAX:
            raise ValueError("limit must lie in [1, %d], not %d" % (_native.GZ_BM25_GROUP_MAX, limit))
        return limit

    def _expand(self, split, max_edits: int, limit: int, only_unknown: bool, prefix_last: bool) -> list:
        """expand() behind its validation: split = the queries' words"""
        words = list(dict.fromkeys(w for ws in split for w in ws))
        if not words:
            return [[] for _ in split]
        held = {w: t >= 0 for w, t in zip(words, self._lookup(words)[0].tolist())}
        last = set(ws[-1] for ws in split if ws) if prefix_last else set()
        inner = set(w for ws in split for w in (ws[:-1] if prefix_last else ws))
        fuzzy = [w for w in words if w in inner and max_edits > 0 and not (only_unknown and held[w])]
        similar, completions = {}, {}
        if self._n_terms() > 0:
            if fuzzy:
                ids, _, _, counts = self.similar_words(fuzzy, max_edits, limit)
                for w, t, c in zip(fuzzy, self.term_texts(ids), counts.tolist()):
                    similar[w] = t[:c]
            if last:
                tails = [w for w in words if w in last]
                ids, _, counts = self.prefix_words(tails, limit)
                for w, t, c in zip(tails, self.term_texts(ids), counts.tolist()):
                    completions[w] = t[:c]
        out = []
        for ws in split:
            gs = []
            for i, w in enumerate(ws):
                if prefix_last and i == len(ws) - 1:
                    g = ([w] if held[w] else []) + [v for v in completions.get(w, []) if v != w]
                    g = g[:limit]
                else:
                    g = list(similar.get(w, []))
                gs.append(g if g else [w])
            out.append(gs)
        return out

    def expand(self, queries: Sequence[str], max_edits: int = 1, limit: int = 8, only_unknown: bool = True, prefix_last: bool = False) -> list:
        """The groups that `search_groups` takes, for a typo-tolerant search of `queries`: one group per word of q.split(), in order,
        repeats kept.  The group of a word w is [w] if max_edits == 0, or only_unknown and the index holds w; else the words of
        similar_words([w], max_edits, limit) in its order (distance, more frequent first) -- w itself first where the index holds
        it -- or [w] if no term is within reach.  prefix_last=True handles the LAST word of every query as half-typed instead: [w]
        first if the index holds w, then the words of prefix_words([w], limit) in its order other than w, cut at limit entries; [w]
        if nothing results.  limit lies in [1, 64].  Composed on the host of one lookup, one similar_words, one prefix_words call
        and term_texts, over the distinct words of the batch; right in every state of the index."""
        split = [q.split() for q in _strings(queries, "queries")]
        return self._expand(split, self._edits(max_edits), self._limit(limit), bool(only_unknown), bool(prefix_last))

    def search_fuzzy(self, queries: Sequence[str], k: int, max_edits: int = 1, limit: int = 8, only_unknown: bool = True,
                     prefix_last: bool = False, match: str = "any", exclude: Optional[Sequence[str]] = None):
        """search_groups(expand(queries, max_edits, limit, only_unknown, prefix_last), k, match, exclude): `cong nghe` finds the
        documents with `công nghệ` and its other spellings, ranked together as one word each; with prefix_last the last word matches
        its completions.  With max_edits=0 and prefix_last=False it equals search(queries, k, match, exclude) bit for bit."""
        k = self._k(k)
        self._match(match)
        split = [q.split() for q in _strings(queries, "queries")]
        max_edits, limit = self._edits(max_edits), self._limit(limit)
        if exclude is not None:
            exclude = _strings(exclude, "exclude")
            if len(exclude) != len(split):
                raise ValueError("exclude has %d items for %d queries" % (len(exclude), len(split)))
        return self.search_groups(self._expand(split, max_edits, limit, bool(only_unknown), bool(prefix_last)), k, match, exclude)

    # ---- inside a document: snippets and the positions of the query's words ---------------------------------------------
    def _snippet_args(self, queries, ids, width=1):
        """validation of snippets / occurrences / snippet_texts, all of it before any native call -> (queries, ids int64 [Q, k])"""
        queries = _strings(queries, "queries")
        if isinstance(width, bool) or not isinstance(width, numbers.Integral):
            raise TypeError("width must be int, not %s" % type(width).__name__)
        ids = np.asarray(ids)
        if ids.dtype == np.bool_ or not np.issubdtype(ids.dtype, np.integer):
            raise TypeError("ids must be integers, not %s" % ids.dtype)
        if ids.ndim != 2:
            raise ValueError("ids must be 2-D [queries, k], not %d-D" % ids.ndim)
        if ids.shape[0] != len(queries):
            raise ValueError("ids has %d rows for %d queries" % (ids.shape[0], len(queries)))
        if int(width) < 1:
            raise ValueError("width must be >= 1, not %d" % width)
        if not getattr(self, "_positions", False):
            raise ValueError("snippets need an index built with positions=True")
        if ids.size and (int(ids.min()) < -1 or int(ids.max()) >= self.num_doc):
            raise IndexError("document ids must lie in [-1, %d)" % self.num_doc)
        return queries, np.ascontiguousarray(ids, dtype=np.int64)

    def _query_terms(self, queries):
        """str.split() of every query -> (term ids, int64 query offsets): _queries without the idf"""
        split = [q.split() for q in queries]
        qoff = np.zeros(len(split) + 1, dtype=np.int64)
        if split:
            np.cumsum([len(w) for w in split], out=qoff[1:])
        words = [w for ws in split for w in ws]
        return (self._lookup(words)[0] if words else np.zeros(0, np.int32)), qoff

    def snippets(self, queries: Sequence[str], ids, width: int = 32):
        """(starts int32 [Q, k], hits int32 [Q, k]) for ids [Q, k] (what search / top_k returned; anything np.asarray makes a 2-D
        integer array of).  With W = documents[d].split(), n = len(W), R = set(queries[q].split()) and h[p] = W[p] in R: over the
        starts s in range(max(1, n - width + 1)), hits(s) = sum(h[s:s + width]); starts[q, j] is the SMALLEST s with the largest
        hits(s) for d = ids[q, j], hits[q, j] that count.  A document without words gives (0, 0), n <= width start 0 and all of the
        document's hits, a query without (known) words hits 0; id -1 gives start -1, hits 0.  Computed on the GPU from the positional
        store.  TypeError: a query that is no str, ids that are no integers, a width that is no int; ValueError: ids not 2-D or
        with another row count than queries, width < 1, an index built without positions=True; IndexError: an id outside
        [-1, num_doc)."""
        queries, ids = self._snippet_args(queries, ids, width)
        if ids.size == 0:
            return np.zeros(ids.shape, dtype=np.int32), np.zeros(ids.shape, dtype=np.int32)
        terms, qoff = self._query_terms(queries)
        return self._ctx.bm25_snippets(self._index, terms, qoff, ids, int(width))

    def occurrences(self, queries: Sequence[str], ids):
        """(positions int32 [T], words int32 [T], offsets int64 [Q * k + 1]) for ids [Q, k]: pair r = q * k + j owns
        [offsets[r], offsets[r + 1]).  With W and Rl = queries[q].split() as in `snippets`: its positions are the p with W[p] in Rl,
        ascending, and words holds Rl.index(W[p]) -- the first place of that word in the query.  Id -1 owns nothing.  Computed on
        the GPU (count, scan, fill).  Errors as `snippets`."""
        queries, ids = self._snippet_args(queries, ids)
        if ids.size == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
        terms, qoff = self._query_terms(queries)
        return self._ctx.bm25_occurrences(self._index, terms, qoff, ids)

    def snippet_texts(self, queries: Sequence[str], ids, width: int = 32, mark=None) -> list:
        """A list of Q lists of k str: " ".join(W[s:s + width]) of every pair's snippet (`snippets`), "" for id -1.  With
        mark=(open, close) every word of the window that is an occurrence (`occurrences`) is wrapped: open + word + close.  Only the
        texts of the given ids are split, each once."""
        queries, ids = self._snippet_args(queries, ids, width)
        if mark is not None:
            mark = tuple(_strings(mark, "mark"))
            if len(mark) != 2:
                raise ValueError("mark must be (open, close), not %d items" % len(mark))
        width = int(width)
        starts, _ = self.snippets(queries, ids, width)
        if mark is not None:
            pos, _, off = self.occurrences(queries, ids)
            pos, off = pos.tolist(), off.tolist()
        words = {}
        out = []
        k = ids.shape[1]
        for q, (row, srow) in enumerate(zip(ids.tolist(), starts.tolist())):
            texts = []
            for j, (d, s) in enumerate(zip(row, srow)):
                if d < 0:
                    texts.append("")
                    continue
                W = words.get(d)
                if W is None:
                    W = words[d] = self._texts[d].split()
                win = W[s:s + width]
                if mark is not None:
                    r = q * k + j
                    for p in pos[off[r]:off[r + 1]]:
                        if s <= p < s + width:
                            win[p - s] = mark[0] + win[p - s] + mark[1]
                texts.append(" ".join(win))
            out.append(texts)
        return out

    # ---- proximity: words within a window of each other, and the smallest window that holds them ----------------------
    def _near_args(self, queries, near, window, match, exclude, phrase):
        """validation of search_near / count_near, all of it before any native call -> (queries, mode, exclude, phrase, near,
        windows int64 [Q])"""
        mode = self._match(match)
        queries = _strings(queries, "queries")
        near = _strings(near, "near")
        if isinstance(window, numbers.Integral):
            windows = [window] * len(queries)
        else:
            try:
                windows = [] if isinstance(window, (str, bytes)) else list(window)
            except TypeError:
                windows = []
            if not windows and not isinstance(window, (list, tuple, np.ndarray)):
                raise TypeError("window must be int or one int per query, not %s" % type(window).__name__)
        for w in windows:
            if isinstance(w, bool) or not isinstance(w, numbers.Integral):
                raise TypeError("window must be int, not %s" % type(w).__name__)
        queries, mode, exclude, phrase = self._bool_args(queries, match, exclude, phrase)
        if len(near) != len(queries):
            raise ValueError("near has %d items for %d queries" % (len(near), len(queries)))
        if len(windows) != len(queries):
            raise ValueError("window has %d items for %d queries" % (len(windows), len(queries)))
        for w in windows:
            if int(w) < 1:
                raise ValueError("window must be >= 1, not %d" % w)
        if not getattr(self, "_positions", False):
            raise ValueError("near needs an index built with positions=True")
        return queries, mode, exclude, phrase, near, np.array([min(int(w), 1 << 62) for w in windows], dtype=np.int64)

    def _sets(self, strings):
        """the DISTINCT words of every string, in the order of their first occurrence -> (term ids, int64 offsets); a word no
        document holds has term -1"""
        split = [list(dict.fromkeys(x.split())) for x in strings]
        off = np.zeros(len(split) + 1, dtype=np.int64)
        if split:
            np.cumsum([len(w) for w in split], out=off[1:])
        words = [w for ws in split for w in ws]
        return (self._lookup(words)[0] if words else np.zeros(0, np.int32)), off

    def _near_native(self, queries, exclude, phrase, near):
        nq, terms, idf, qoff = self._queries(queries)
        xterms, xoff = self._exclusions(exclude, nq) if exclude is not None else (None, None)
        pterms, poff = self._exclusions(phrase, nq) if phrase is not None else (None, None)
        nterms, noff = self._sets(near)
        return terms, idf, qoff, dict(ex_terms=xterms, ex_off=xoff, ph_terms=pterms, ph_off=poff, nr_terms=nterms, nr_off=noff)

    def search_near(self, queries: Sequence[str], k: int, near: Sequence[str], window, match: str = "any",
                    exclude: Optional[Sequence[str]] = None, phrase: Optional[Sequence[str]] = None):
        """(ids, scores, counts) with the dtypes, shapes, order and padding of `search`, restricted to the documents that ALSO hold
        the words of near[q] close to each other.  With W = documents[d].split(), S = set(near[q].split()) and w = window[q] (an int
        for every query, or one int per query; >= 1): d matches iff it matches under match / exclude / phrase exactly as `search`
        defines it AND (S is empty or S <= set(W[i:i + w]) for some i in range(max(1, len(W) - w + 1))) -- the words in any order,
        repeated words counting once.  A near word that no document holds matches nothing, an empty near[q] is no constraint,
        w < len(S) can match nothing, w >= len(W) means "holds all of them", and a window never reaches into a neighbouring
        document.  Near is a filter only: its words enter no score and no idf.  With near=[""] * len(queries) the result is
        `search`'s, bit for bit.  More than 64 distinct words in a near[q] raise _native.GzError (GZ_E_LIMIT).  TypeError: a near
        item that is no str, a window that is bool or no int; ValueError: near or window of another length than queries, a window
        < 1, an index built without positions=True; everything else as `search`."""
        k = self._k(k)
        queries, mode, exclude, phrase, near, windows = self._near_args(queries, near, window, match, exclude, phrase)
        terms, idf, qoff, kw = self._near_native(queries, exclude, phrase, near)
        plus = isinstance(self, BM25Plus)
        return self._ctx.bm25_search(self._index, terms, idf, qoff, self._params(), plus, k, mode=mode, nr_window=windows, **kw)

    def count_near(self, queries: Sequence[str], near: Sequence[str], window, match: str = "any",
                   exclude: Optional[Sequence[str]] = None, phrase: Optional[Sequence[str]] = None) -> np.ndarray:
        """int64 [len(queries)]: counts of search_near(queries, k, near, window, match, exclude, phrase) alone."""
        queries, mode, exclude, phrase, near, windows = self._near_args(queries, near, window, match, exclude, phrase)
        terms, _, qoff, kw = self._near_native(queries, exclude, phrase, near)
        return self._ctx.bm25_match_count(self._index, terms, qoff, mode=mode, nr_window=windows, **kw)

    def cover(self, queries: Sequence[str], ids):
        """(starts, lengths, words), each int32 [Q, k], for ids [Q, k] (as `snippets` takes them): the shortest passage of document
        d = ids[q, j] that holds all the query words it has.  With W = documents[d].split() and R = set(queries[q].split()) &
        set(W): words[q, j] = len(R); over all windows W[i:i2] with R <= set(W[i:i2]), the one with the smallest (i2 - i, i):
        starts[q, j] = i, lengths[q, j] = i2 - i.  A document with none of the words gives (0, 0, 0), id -1 gives (-1, 0, 0);
        words unknown to the index are ignored, and words == len(set(queries[q].split())) says that the cover is complete.
        Computed on the GPU from the positional store, a wave per pair.  More than 64 distinct words in a query raise
        _native.GzError (GZ_E_LIMIT); every other error as `snippets` (no width)."""
        queries, ids = self._snippet_args(queries, ids)
        if ids.size == 0:
            return tuple(np.zeros(ids.shape, dtype=np.int32) for _ in range(3))
        terms, qoff = self._sets(queries)
        return self._ctx.bm25_cover(self._index, terms, qoff, ids)

    def get_top_n(self, query: str, documents: Optional[Sequence] = None, n: int = 5) -> list:
        """The n best documents for query, best first (rank_bm25's get_top_n): [documents[i] for i in top_k([query], n)[0][0]].
        documents defaults to the strings the index was built from; any sequence of num_doc objects may stand in for them."""
        if not isinstance(query, str):
            raise TypeError("query must be str, not %s" % type(query).__name__)
        if documents is None:
            documents = self._texts
        elif len(documents) != self.num_doc:
            raise ValueError("documents has %d items; the index has %d documents" % (len(documents), self.num_doc))
        ids, _ = self.top_k([query], n)
        return [documents[i] for i in ids[0].tolist()]

    def get_score(self, query: str) -> List:
        if not isinstance(query, str):
            raise TypeError("query must be str, not %s" % type(query).__name__)
        if self.num_doc == 0:
            return []
        if not query.split():
            return [0] * self.num_doc                           # ranking.py:37-38: the int 0 of an empty sum
        return list(self.get_scores([query])[0])                 # np.float64 items, like the reference's


class BM25Plus(BM25):
    def __init__(self, documents: List, b: float = 0.75, k1: float = 1.2, delta: float = 1.0,
                 ctx: Optional[_native.Context] = None, positions: bool = False) -> None:
        super().__init__(documents, b, k1, ctx, positions)
        self.delta = delta
