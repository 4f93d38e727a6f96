"""Drop-in `Tokenize` for DVNghiem/genz-tokenize v1.2.7, computed on an MI355X.

Same Python surface as the reference class (reference genz_tokenize/tokenize.py:6-278):
`Tokenize(...)`, `Tokenize.fromFile`, `__call__`, `encode`, `decode`, `bpe`, `vocab_size`,
`add_vocab_file`, `add_bpe_file`, the three `get_*` helpers and the module function
`get_pairs`, with the same results, key order, `None`s and exceptions.  Underneath, every
call that tokenizes goes through the C ABI of include/genz_tokenize.h into hand-written HIP
kernels; nothing here falls back to a CPU implementation.

On top of the reference surface there is a batch API (`encode_batch`, `encode_packed`)
that returns numpy arrays, which is what the GPU is for.
"""
from __future__ import annotations

import contextlib
import math
import os
import threading
import weakref
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native, _packing
from ._packing import pack as _pack            # list of str -> packed UTF-8 + offsets (C when built)

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def _read_text(path) -> str:
    # the reference opens both files with open(path, 'r', encoding='utf-8') (tokenize.py:45, :54):
    # FileNotFoundError / UnicodeDecodeError surface from here exactly as they do there
    with open(path, "r", encoding="utf-8") as f:
        return f.read()


def _require_str(x):
    # re.findall(r"\S+\n?", x) (tokenize.py:106) is what rejects non-str input in the reference
    if isinstance(x, str):
        return
    if isinstance(x, (bytes, bytearray, memoryview)):
        raise TypeError("cannot use a string pattern on a bytes-like object")
    raise TypeError("expected string or bytes-like object")


# ---- validators of the row-shaping calls (window_rows, pack_rows, mask_rows, infill_rows): the value, or the refusal ----
def _integer(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s must be an int" % name)
    if not lo <= int(v) < hi:
        raise ValueError("%s must lie in [%d, %d)" % (name, lo, hi))
    return int(v)


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError("%s must be a number" % name)
    return float(v)


def _share(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError("%s must be a number" % name)
    if not 0 <= v <= 1:                                                # (NaN fails here too)
        raise ValueError("%s must lie in [0, 1]" % name)
    return float(v)


def _int32_ids(name, a, dense=False):
    """ids as an int32 array, refused in the words of the call `name`; dense: they are rows [R, L], not flat"""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError("%s() expects integer ids" % name)
    if dense and (a.ndim != 2 or a.shape[1] < 1 or a.shape[1] >= 2 ** 31):
        raise ValueError("%s() expects a 2-D array of rows, [R, L] with 1 <= L < 2**31" % name)
    if a.dtype != np.int32:
        if a.size and (int(a.min()) < -(2 ** 31) or int(a.max()) >= 2 ** 31):
            raise ValueError("%s() expects ids that fit in int32" % name)
        a = a.astype(np.int32)
    return a


class NgramIndex(object):
    """The token n-grams of a held-out set, resident in HBM (`Tokenize.ngram_index`, `Tokenize.encode_ngram_index`): what
    `ngram_overlap_rows`, `encode_ngram_overlap` and `decontaminate` of the SAME Tokenize object query.  It owns a copy of the
    reference ids.  `close()` (or leaving a `with` block, or garbage collection) frees the device memory; a closed index is
    refused.  Properties: n, n_rows (reference rows), n_ids (reference ids), n_grams (n-gram positions), n_distinct (distinct
    n-grams) and device_bytes."""

    def __init__(self, ctx, handle):
        self._ctx = ctx
        self._handle = handle
        self._info = ctx.ngram_index_info(handle)
        # (the finalizer holds the context: the index is freed before it)
        self._finalizer = weakref.finalize(self, ctx.ngram_index_destroy, handle)

    n = property(lambda self: self._info["n"])
    n_rows = property(lambda self: self._info["n_rows"])
    n_ids = property(lambda self: self._info["n_ids"])
    n_grams = property(lambda self: self._info["n_grams"])
    n_distinct = property(lambda self: self._info["n_distinct"])
    device_bytes = property(lambda self: self._info["device_bytes"])

    @property
    def closed(self):
        return self._handle is None

    def close(self):
        if self._handle is not None:
            self._handle = None
            self._finalizer()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __repr__(self):
        return "NgramIndex(n=%d, n_rows=%d, n_distinct=%d%s)" % (self.n, self.n_rows, self.n_distinct, ", closed" if self.closed else "")


class Tokenize(object):
    def __init__(self, pad_token='<pad>', bos_token='<s>', eos_token='</s>', mask_token='<mask>',
                 unk_token='<unk>', device: Optional[int] = None) -> None:
        super().__init__()
        # tokenize.py:15-23 -- paths survive a second __init__ (that is how fromFile works)
        if not hasattr(self, "vocab_file"):
            self.vocab_file = os.path.join(_DATA, "vocab.txt")
        if not hasattr(self, "bpe_file"):
            self.bpe_file = os.path.join(_DATA, "bpe.codes")
        self.pad_token, self.bos_token, self.eos_token = pad_token, bos_token, eos_token
        self.mask_token, self.unk_token = mask_token, unk_token
        if not hasattr(self, "_ctx"):
            self._ctx = _native.Context(device)
            self._batch_lock = threading.Lock()      # the batch calls' pinned text arena (one per object): _packing.pack_pinned
        self._vocab_texts: List[str] = []
        self._bpe_text = ""
        self._dicts = {}
        self._dirty = True
        self._snapshot_pending = False
        self.add_vocab_file(self.vocab_file)
        # tokenize.py:40: `decoder` is built ONCE, here, from the first vocab load; a later add_vocab_file does not
        # change it.  Both snapshots are taken lazily: the host dict when `.decoder` / decode() is first used, the
        # device one with the first table build (the merges loaded next do not touch `encoder`).
        self._decoder_snapshot = None
        self._snapshot_source = (self._vocab_texts[0], (pad_token, bos_token, eos_token, mask_token, unk_token))
        self._snapshot_pending = True
        self.add_bpe_file(self.bpe_file)

    # ---- tables -------------------------------------------------------------------------------------------
    def add_vocab_file(self, vocab_file):
        """tokenize.py:44-51 -- appends words to `encoder`; the device tables are rebuilt lazily."""
        text = _read_text(vocab_file)
        if getattr(self, "_snapshot_pending", False):
            self._sync_tables()                 # take the device decoder snapshot before the vocabulary grows
        self._vocab_texts.append(text)
        self._dirty = True

    def add_bpe_file(self, bpe_file):
        """tokenize.py:53-57 -- replaces `bpe_ranks`."""
        self._bpe_text = _read_text(bpe_file)
        self._dirty = True

    def _sync_tables(self):
        if not self._dirty:
            return
        # several vocab files behave like one file whose lines are the concatenation of theirs
        chunks = []
        for t in self._vocab_texts:
            chunks.append(t if (t == "" or t.endswith("\n")) else t + "\n")
        vocab = "".join(chunks).encode("utf-8")
        self._ctx.load_tables(vocab, self._bpe_text.encode("utf-8"),
                              (self.pad_token, self.bos_token, self.eos_token, self.mask_token, self.unk_token))
        self._dicts = {}
        self._dirty = False
        if self._snapshot_pending:
            self._ctx.decoder_snapshot()
            self._snapshot_pending = False

    @property
    def encoder(self) -> Dict[str, int]:
        self._sync_tables()
        if "encoder" not in self._dicts:
            self._dicts["encoder"] = dict(self._ctx.vocab_items())
        return self._dicts["encoder"]

    @property
    def decoder(self) -> Dict[int, str]:
        if self._decoder_snapshot is None:
            text, specials = self._snapshot_source
            vocab = (text if (text == "" or text.endswith("\n")) else text + "\n").encode("utf-8")
            ht = _native.HostTables(vocab, b"", specials)
            self._decoder_snapshot = {v: k for k, v in ht.vocab_items()}
            ht.close()
        return self._decoder_snapshot

    @property
    def bpe_ranks(self):
        self._sync_tables()
        if "ranks" not in self._dicts:
            self._dicts["ranks"] = dict(self._ctx.merge_items())
        return self._dicts["ranks"]

    def vocab_size(self):
        self._sync_tables()
        return self._ctx.table_info()[0]

    def _special_ids(self):
        self._sync_tables()
        return self._ctx.table_info()[1]       # pad, bos, eos, mask, unk  (looked up at call time, rule L4)

    # ---- BPE of one word -----------------------------------------------------------------------------------
    def bpe(self, token):
        """tokenize.py:62-101: "piece@@ piece ..." for ONE word (no whitespace splitting here)."""
        if not isinstance(token, str):
            raise TypeError("bpe() expects str")
        if token == "":
            raise IndexError("tuple index out of range")         # word[-1] on an empty tuple (tokenize.py:64)
        self._sync_tables()
        pieces = self._ctx.bpe_word(token.encode("utf-8", "surrogatepass"))
        if len(pieces) == 1 and len(token) == 1:
            return token                                         # tokenize.py:66-67
        strs = []
        for k, p in enumerate(pieces):
            p = int(p)
            if p >= 0:
                strs.append(self._ctx.symbol(p))
            else:
                strs.append(chr(-p - 1) + ("</w>" if k == len(pieces) - 1 else ""))
        return "@@ ".join(strs)[:-4]

    # ---- encode / decode -------------------------------------------------------------------------------------
    def _run(self, texts, pairs, max_len, padding, truncation, word_table=True, keep_words=False):
        self._sync_tables()
        tb, to = _pack(texts)
        pb = po = None
        if pairs is not None:
            pb, po = _pack(pairs)
        return self._ctx.encode(tb, to, pb, po, max_len, bool(padding), bool(truncation),
                                (0 if word_table else _native.GZ_NO_WORD_TABLE) | (_native.GZ_KEEP_WORDS if keep_words else 0))

    def encode(self, sentence, return_offset) -> List[int]:
        """tokenize.py:126-135."""
        _require_str(sentence)
        r = self._run([sentence], None, None, False, False, keep_words=bool(return_offset))
        ids = r["input_ids"].tolist()
        if return_offset:
            return ids, self._offsets(0, len(sentence.encode("utf-8", "surrogatepass")))
        return ids

    def _offsets(self, which_text, nbytes):
        """tokenize.py:105, :111-117: [(0,0)] + one (first, last) 1-based token span per word + (T+1, T+1), from the
        per-word piece counts of the last device call."""
        counts, _ = self._ctx.word_token_counts(which_text, 1, nbytes // 1 + 2)
        off, seen = [(0, 0)], 0
        for c in counts.tolist():
            off.append((seen + 1, seen + c)); seen += c
        off.append((seen + 1, seen + 1))
        return off

    def decode(self, token):
        """tokenize.py:137-139 (host side: string assembly)."""
        dec, unk = self.decoder, self.unk_token
        return ' '.join(dec.get(i, unk) for i in token).replace('@@ ', '')

    def decode_batch(self, rows) -> List[str]:
        """`decode` for many id lists at once, on the GPU (the reference has no batch form).
        `rows` is a sequence of integer sequences or a 2-D integer array; ids outside the int32 range decode to the
        unk token like any other unknown id."""
        flat, off = self._flat_rows(rows)
        self._sync_tables()
        flat = np.asarray(flat)
        if flat.dtype != np.int32:
            if flat.dtype.kind not in "iu":
                raise TypeError("decode_batch() expects integer ids")
            flat = np.where((flat < -(2 ** 31)) | (flat >= 2 ** 31), -1, flat).astype(np.int32)
        data, out_off = self._ctx.decode(flat, off, self.unk_token.encode("utf-8", "surrogatepass"))
        raw = data.tobytes()
        return [raw[out_off[i]:out_off[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(off) - 1)]

    @staticmethod
    def _flat_rows(rows):
        """Sequences of ints, or a 2-D array -> (the rows back to back, int64 offsets [N+1])."""
        if isinstance(rows, np.ndarray) and rows.ndim == 2:
            n, L = rows.shape
            return rows.reshape(-1), np.arange(n + 1, dtype=np.int64) * L
        rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        if rows:
            np.cumsum([len(r) for r in rows], out=off[1:])
        return (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)), off

    def get_atttention_mask(self, token):
        pad = self._special_ids()[0]
        return [1 if i != pad else 0 for i in token]

    def get_token_type(self, token):
        """tokenize.py:154-161 (mutates and returns its argument; ValueError when < 2 None remain)."""
        token[0] = 0
        token[-1] = 1
        token[token.index(None)] = 0
        token[token.index(None)] = 1
        return token

    def get_sequence_id(self, token):
        """tokenize.py:163-182."""
        sp = self._special_ids()
        bos, eos = sp[1], sp[2]
        out = []
        for v in token:
            if v == eos:
                out.append(None)
                break
            out.append(None if v == bos else 0)
        for k in range(len(out), len(token)):
            if token[k] == eos:
                out.append(None)
                if out[k - 1] == 1:
                    break
            else:
                out.append(1)
        return out

    def __call__(self, text: str, pair_text: str = None, max_len: int = None, padding: bool = True,
                 truncation: bool = True, return_offset: bool = False) -> Dict:
        """tokenize.py:184-259.  Returns {'input_ids', 'attention_mask'[, 'sequence_id', 'token_type_ids']}."""
        _require_str(text)
        if pair_text is not None:
            _require_str(pair_text)
        if max_len is not None and not isinstance(max_len, (int, np.integer)):
            raise TypeError("max_len must be an int or None")
        r = self._run([text], None if pair_text is None else [pair_text], max_len, padding, truncation, keep_words=bool(return_offset))
        if pair_text is not None and int(r["status"][0]) != 0:
            raise ValueError("None is not in list")                 # tokenize.py:157-160, rule P3
        result = {}
        if return_offset:                                            # tokenize.py:225-234, :241-244 (first key, rule R1)
            off = self._offsets(0, len(text.encode("utf-8", "surrogatepass")))
            if pair_text is not None:
                shift = len(off)                                     # entries of A, not tokens (rule O2)
                off = off + [(a + shift, b + shift)
                             for a, b in self._offsets(1, len(pair_text.encode("utf-8", "surrogatepass")))]
            result['offset'] = off
        result['input_ids'] = r["input_ids"].tolist()
        result['attention_mask'] = r["attention_mask"].tolist()
        if pair_text is not None:
            ns, nt = (int(x) for x in r["pair_len"][0])
            seq = [None if v == _native.GZ_NONE else v for v in r["sequence_id"][:ns].tolist()]
            if max_len is not None and padding:
                tt = [None if v == _native.GZ_NONE else v for v in r["token_type_ids"][:nt].tolist()]
            else:
                tt = seq                                             # the same list object (tokenize.py:254-255)
            result['sequence_id'] = seq
            result['token_type_ids'] = tt
        return result

    # ---- batch API (new) -----------------------------------------------------------------------------------------
    def encode_batch(self, texts: Sequence[str], pair_texts: Optional[Sequence[str]] = None,
                     max_len: Optional[int] = None, padding: bool = True, truncation: bool = True,
                     word_table: bool = True, return_offset: bool = False):
        """`__call__` over many documents in one launch.  With max_len >= 1, padding and truncation the result
        arrays are [N, max_len] int32; otherwise they are flat with `row_off` [N+1].  `status[i] == 1` marks a
        document for which the single-call API raises ValueError.
        `return_offset=True` adds `__call__`'s 'offset' lists for every document (tokenize.py:105, :111-117, :225-234) as two
        arrays: `offset` int32 [E, 2] -- the (first, last) spans of all documents one after the other -- and `offset_off`
        int64 [N+1]: document i's list is offset[offset_off[i]:offset_off[i+1]] (`offsets_of(result, i)` gives it in the
        reference's list-of-tuples form)."""
        if pair_texts is not None and len(pair_texts) != len(texts):
            raise ValueError("texts and pair_texts differ in length")
        if (pair_texts is None and padding and truncation and max_len is not None and int(max_len) >= 1 and len(texts) >= 20000
                and _packing._gz_pack is not None and not return_offset):
            return self._shape(self._encode_batch_large(texts, int(max_len), word_table), len(texts))
        r = self._run(list(texts), None if pair_texts is None else list(pair_texts), max_len, padding, truncation,
                      word_table, keep_words=bool(return_offset))
        out = self._shape(r, len(texts))
        if return_offset:
            out["offset"], out["offset_off"] = self._batch_offsets(len(texts), pair_texts is not None)
        return out

    def _batch_offsets(self, n, is_pair):
        """The 'offset' lists of the last batch call, from the per-word piece counts the device kept (GZ_KEEP_WORDS): per text
        [(0, 0)] + one 1-based (first, last) token span per word + (T+1, T+1) (tokenize.py:105, :111-117); in pair mode B's
        entries follow A's, each shifted by the NUMBER OF ENTRIES of A (tokenize.py:231-234: `len(offset)`, not tokens)."""
        if n == 0:                                               # no texts: the device kept nothing, and is asked for nothing
            return np.zeros((0, 2), dtype=np.int32), np.zeros(1, dtype=np.int64)
        def spans(which):
            counts, first = self._ctx.word_token_counts(which, n, 1 << 16)
            first = first.astype(np.int64)
            nw = np.diff(first)
            eoff = first + 2 * np.arange(n + 1, dtype=np.int64)          # entries before document d: its words + 2 per document
            cs = np.zeros(len(counts) + 1, dtype=np.int64)
            np.cumsum(counts, out=cs[1:])
            base = cs[first[:-1]]
            out = np.zeros((int(eoff[-1]), 2), dtype=np.int64)
            doc = np.repeat(np.arange(n, dtype=np.int64), nw)
            w = np.arange(len(counts), dtype=np.int64)
            pos = w + 2 * doc + 1
            out[pos, 0] = cs[:-1] - base[doc] + 1
            out[pos, 1] = cs[1:] - base[doc]
            T = cs[first[1:]] - base
            out[eoff[1:] - 1] = (T + 1)[:, None]
            return out, eoff
        a, ea = spans(0)
        if not is_pair:
            return a.astype(np.int32), ea
        b, eb = spans(1)
        na, nb = np.diff(ea), np.diff(eb)
        b += np.repeat(na, nb)[:, None]                              # rule O2: shifted by A's entry count
        eoff = ea + eb
        out = np.empty((int(eoff[-1]), 2), dtype=np.int64)
        ia = np.arange(len(a), dtype=np.int64) + np.repeat(eb[:-1], na)          # A's entries of document d move up by B's earlier ones
        ib = np.arange(len(b), dtype=np.int64) + np.repeat(ea[1:], nb)           # B's follow A's of the same document
        out[ia] = a
        out[ib] = b
        return out.astype(np.int32), eoff

    @staticmethod
    def offsets_of(result, i):
        """Document i's 'offset' list of an `encode_batch(..., return_offset=True)` result, as `__call__` returns it."""
        lo, hi = int(result["offset_off"][i]), int(result["offset_off"][i + 1])
        return [(int(a), int(b)) for a, b in result["offset"][lo:hi]]

    def _encode_batch_large(self, texts, max_len, word_table):
        """Large dense single-text batches: the strings are packed on threads (csrc/gz_pack.c) straight into a pinned arena this
        object keeps, and the packed text goes through the library's dense host path (gz_encode_batch: sub-batches, only the text
        and the rows' real entries cross PCIe, the [N, max_len] arrays are padded into place by host threads inside the call).
        The arena is ONE buffer per object: the lock keeps a second thread's batch out of it until this call has consumed it."""
        self._sync_tables()
        with self._batch_lock:
            tb, to = _packing.pack_pinned(texts, self, self._ctx)
            return self._ctx.encode(tb, to, None, None, max_len, True, True, 0 if word_table else _native.GZ_NO_WORD_TABLE)

    def encode_packed(self, text_u8: np.ndarray, offsets: np.ndarray, pair_u8=None, pair_offsets=None,
                      max_len: Optional[int] = None, padding: bool = True, truncation: bool = True,
                      word_table: bool = True):
        """Batch call on already packed UTF-8 (uint8 array + int64 offsets[N+1]); skips Python string packing.
        `word_table=False` makes every word run the merge loop (same results; for tests and measurements)."""
        self._sync_tables()
        r = self._ctx.encode(text_u8, offsets, pair_u8, pair_offsets, max_len, bool(padding), bool(truncation),
                             0 if word_table else _native.GZ_NO_WORD_TABLE)
        return self._shape(r, len(offsets) - 1)

    def encode_packed_csr(self, text_u8: np.ndarray, offsets: np.ndarray, max_len: int, word_table: bool = True):
        """The fast host path for large batches: `__call__(text, max_len=max_len)` over packed UTF-8, with the result in
        CSR form -- dict(tokens [total] (uint16 when every id fits, else int32), n_real [N], row_off [N+1], max_len,
        pad_id).  Only the text and the rows' real entries cross PCIe (the copies overlap the kernels); `csr_to_dense`
        rebuilds the [N, max_len] input_ids / attention_mask of `encode_packed` on the host when they are wanted."""
        self._sync_tables()
        if max_len is None or int(max_len) < 1:
            raise ValueError("encode_packed_csr needs max_len >= 1 (rows are cut to max_len)")
        bits = 16 if self.vocab_size() <= 65536 and max(self._special_ids()) < 65536 and min(self._special_ids()) >= 0 else 32
        try:
            tokens, n_real = self._ctx.encode_csr(text_u8, offsets, int(max_len), bits, 0 if word_table else _native.GZ_NO_WORD_TABLE)
        except _native.GzError as e:
            if bits == 16 and e.code == _native.GZ_E_LIMIT:              # an id collision pushed an id past 65535
                tokens, n_real = self._ctx.encode_csr(text_u8, offsets, int(max_len), 32, 0 if word_table else _native.GZ_NO_WORD_TABLE)
            else:
                raise
        row_off = np.zeros(len(n_real) + 1, dtype=np.int64)
        np.cumsum(n_real, out=row_off[1:])
        return dict(tokens=tokens, n_real=n_real, row_off=row_off, max_len=int(max_len), pad_id=self._special_ids()[0])

    @staticmethod
    def csr_to_dense(csr):
        """(input_ids, attention_mask) [N, max_len] int32 of a `encode_packed_csr` result: rows padded with the pad id
        (tokenize.py:141-146), mask = ids != pad (:148-152)."""
        n, L = len(csr["n_real"]), csr["max_len"]
        ids = np.full((n, L), csr["pad_id"], dtype=np.int32)
        cols = np.arange(L, dtype=np.int64)[None, :]
        keep = cols < csr["n_real"][:, None]
        ids[keep] = csr["tokens"].astype(np.int32, copy=False)
        return ids, (ids != csr["pad_id"]).astype(np.int32)

    def encode_to_device(self, texts: Sequence[str], pair_texts: Optional[Sequence[str]] = None, max_len: int = 128):
        """Batch `__call__` (padding=True, truncation=True) whose [N, max_len] int32 outputs STAY in HBM: a dict with the field names
        of the reference's DataCollection (models/bert/dataset.py:7-28) -- input_ids, attention_mask and, with pair
        texts, token_type_ids / sequence_id -- as `handoff.DeviceArray`s (DLPack: `torch.from_dlpack(x)` is zero-copy),
        plus host arrays n_real [N] and status [N]."""
        from .handoff import DeviceArray
        if max_len is None or int(max_len) < 1:
            raise ValueError("encode_to_device needs max_len >= 1 (dense rows)")
        self._sync_tables()
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            return self._encode_to_device_locked(texts, pair_texts, int(max_len))

    def _encode_to_device_locked(self, texts, pair_texts, L):
        from .handoff import DeviceArray
        ctx = self._ctx
        t, to = _packing.pack_pinned(texts, self, ctx)                 # (a pinned arena this object keeps: the H2D copy is real DMA)
        n = len(to) - 1
        pair = pair_texts is not None
        if pair:
            if len(pair_texts) != n:
                raise ValueError("texts and pair_texts differ in length")
            p, po = _pack(pair_texts)
        bufs = []

        def up(a):
            d = ctx.alloc(max(a.nbytes, 1) + 64)
            bufs.append(d)
            if a.nbytes:
                ctx.h2d(d, np.ascontiguousarray(a))
            return d
        try:
            d_t, d_to = up(t), up(to)
            d_p, d_po = (up(p), up(po)) if pair else (0, 0)
            cells = max(n * L, 1)
            out = {k: DeviceArray(ctx, ctx.alloc(4 * cells), (n, L)) for k in
                   (("input_ids", "attention_mask", "token_type_ids", "sequence_id") if pair else ("input_ids", "attention_mask"))}
            d_nr, d_st, d_pl = ctx.alloc(4 * max(n, 1)), ctx.alloc(4 * max(n, 1)), ctx.alloc(8 * max(n, 1))
            bufs += [d_nr, d_st, d_pl]
            flags = _native.GZ_PADDING | _native.GZ_TRUNCATION
            ctx.encode_device(d_t, d_to, d_p, d_po, n, L, flags, n * L, out["input_ids"].ptr, out["attention_mask"].ptr,
                              out["token_type_ids"].ptr if pair else None, out["sequence_id"].ptr if pair else None,
                              None, d_pl if pair else None, d_nr, d_st if pair else None)
            ctx.sync()
            nr = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
            if n:
                ctx.d2h(nr, d_nr)
                if pair:
                    ctx.d2h(st, d_st)
            out["n_real"], out["status"] = nr, st
            return out
        finally:
            for d in bufs:
                ctx.free(d)

    # ---- BPE-dropout (Provilkov et al., 2020): seeded segmentation noise --------------------------------------------------
    @staticmethod
    def _dropout_rule(p, seed, doc_base=0, word=0):
        """(thr, seed, doc_base, word) of a dropout call, or the refusal.  thr = int(p * 2**32): a candidate merge is skipped when its
        32-bit draw is below it (p = 1.0 drops everything)."""
        thr = int(_share("p", p) * 2 ** 32)
        return thr, _integer("seed", seed, 0, 2 ** 64), _integer("doc_base", doc_base, 0, 2 ** 63), _integer("word", word, 0, 2 ** 32)

    def bpe_dropout(self, token, p, seed=0, doc=0, word=0):
        """`bpe(token)` under BPE-dropout: the segmentation that word number `word` of document `doc` gets in an
        `encode_dropout(..., p, seed)` call, in `bpe()`'s form."""
        if not isinstance(token, str):
            raise TypeError("bpe_dropout() expects str")
        thr, seed, doc, word = self._dropout_rule(p, seed, doc, word)
        if token == "":
            raise IndexError("tuple index out of range")         # as bpe()
        self._sync_tables()
        pieces = self._ctx.bpe_word_dropout(token.encode("utf-8", "surrogatepass"), thr, seed, doc, word)
        if len(pieces) == 1 and len(token) == 1:
            return token
        strs = []
        for k, q in enumerate(pieces):
            q = int(q)
            if q >= 0:
                strs.append(self._ctx.symbol(q))
            else:
                strs.append(chr(-q - 1) + ("</w>" if k == len(pieces) - 1 else ""))
        return "@@ ".join(strs)[:-4]

    def encode_dropout(self, texts: Sequence[str], p=0.1, seed=0, max_len: Optional[int] = None, padding: bool = True,
                       truncation: bool = True, doc_base=0):
        """`encode_batch` for single texts under BPE-dropout: while a word is segmented, each candidate merge is skipped with
        probability `p`.  The draws depend on (seed, doc_base + i, the word's index in text i, the merge iteration, the position)
        alone: the same call gives the same arrays, on any batch split, as long as `doc_base` says where the batch starts.
        p = 0 gives `encode_batch`'s result, p = 1 every word as its code points.  The result has `encode_batch`'s form: dense
        [N, max_len] with max_len, padding and truncation, else flat with `row_off` (which feeds window_rows / pack_rows /
        minhash_rows / decode_batch as an encode result does)."""
        thr, seed, doc_base, _ = self._dropout_rule(p, seed, doc_base)
        texts = list(texts)
        if doc_base + len(texts) > 2 ** 63 - 1:
            raise ValueError("doc_base + len(texts) must stay below 2**63")
        self._sync_tables()
        tb, to = _pack(texts)
        r = self._ctx.encode_dropout(tb, to, max_len, bool(padding), bool(truncation), thr, seed, doc_base)
        return self._shape(r, len(texts))

    def encode_dropout_packed(self, text_u8: np.ndarray, offsets: np.ndarray, p=0.1, seed=0, max_len: Optional[int] = None,
                              padding: bool = True, truncation: bool = True, doc_base=0):
        """`encode_dropout` on already packed UTF-8 (uint8 array + int64 offsets[N+1])."""
        thr, seed, doc_base, _ = self._dropout_rule(p, seed, doc_base)
        if doc_base + len(offsets) - 1 > 2 ** 63 - 1:
            raise ValueError("doc_base + the number of documents must stay below 2**63")
        self._sync_tables()
        r = self._ctx.encode_dropout(text_u8, offsets, max_len, bool(padding), bool(truncation), thr, seed, doc_base)
        return self._shape(r, len(offsets) - 1)

    def encode_dropout_to_device(self, texts: Sequence[str], p, seed, max_len, doc_base=0):
        """`encode_dropout` (padding=True, truncation=True) whose [N, max_len] int32 rows STAY in HBM, as `encode_to_device`:
        input_ids and attention_mask as `handoff.DeviceArray`s, plus the host array n_real [N]."""
        from .handoff import DeviceArray
        thr, seed, doc_base, _ = self._dropout_rule(p, seed, doc_base)
        if max_len is None or isinstance(max_len, bool) or int(max_len) < 1:
            raise ValueError("encode_dropout_to_device needs max_len >= 1 (dense rows)")
        L = int(max_len)
        texts = list(texts)
        if doc_base + len(texts) > 2 ** 63 - 1:
            raise ValueError("doc_base + len(texts) must stay below 2**63")
        self._sync_tables()
        ctx = self._ctx
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            t, to = _packing.pack_pinned(texts, self, ctx)
            n = len(to) - 1
            bufs = []
            try:
                for a in (t, to):
                    d = ctx.alloc(max(a.nbytes, 1) + 64)
                    bufs.append(d)
                    if a.nbytes:
                        ctx.h2d(d, np.ascontiguousarray(a))
                cells = max(n * L, 1)
                out = {k: DeviceArray(ctx, ctx.alloc(4 * cells), (n, L)) for k in ("input_ids", "attention_mask")}
                d_nr = ctx.alloc(4 * max(n, 1))
                bufs.append(d_nr)
                ctx.encode_dropout_device(bufs[0], bufs[1], n, L, _native.GZ_PADDING | _native.GZ_TRUNCATION, n * L, thr, seed, doc_base,
                                          out["input_ids"].ptr, out["attention_mask"].ptr, None, d_nr)
                ctx.sync()
                nr = np.zeros(n, dtype=np.int32)
                if n:
                    ctx.d2h(nr, d_nr)
                out["n_real"], out["status"] = nr, np.zeros(n, dtype=np.int32)
                return out
            finally:
                for d in bufs:
                    ctx.free(d)

    # ---- overlapping max_len windows (long documents) ---------------------------------------------------------------
    @staticmethod
    def _window_rule(max_len, stride):
        """(L, s) of a window call, or the refusal: L >= 3 (bos, a token, eos) and 0 <= s <= L - 3 (every window adds a token)."""
        for name, v in (("max_len", max_len), ("stride", stride)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an int" % name)
        L, s = int(max_len), int(stride)
        if L < 3 or L >= 2 ** 31:
            raise ValueError("windows need 3 <= max_len < 2**31 (bos, at least one token, eos)")
        if not 0 <= s <= L - 3:
            raise ValueError("stride must lie in [0, max_len - 3]: every window adds at least one new token")
        return L, s

    def window_rows(self, rows, max_len: int, stride: int = 0, framed: bool = True):
        """Cut token rows into overlapping rows of `max_len`, on the GPU.  `rows` as `decode_batch` takes them; `framed=True`:
        each row is an encode result and loses its first and last entry first, `False`: bare bodies.  With room = max_len - 2
        and step = room - stride, window j of a body is [bos] + body[j*step : j*step + room] + [eos], padded to max_len; a body
        that fits makes one window, the reference's own row (tokenize.py:141-152), and the last window is shorter, not shifted
        back.  Returns numpy arrays: input_ids [W, L], attention_mask [W, L] (ids != pad), doc [W] (the source row), start [W]
        (the window's first body position), n_real [W], win_off [N+1] (row r's windows are win_off[r]:win_off[r+1])."""
        L, s = self._window_rule(max_len, stride)
        flat, off = self._flat_rows(rows)
        flat = _int32_ids("window_rows", flat)
        self._sync_tables()
        return self._ctx.window_rows(flat, off, L, s, bool(framed))

    def encode_windows(self, texts: Sequence[str], max_len: int, stride: int = 0, word_table: bool = True):
        """`window_rows` over the whole token sequence of every text: the texts are encoded without a length limit on the
        device, cut into windows there, and only the windows come back.  Returns the dict of `window_rows`; window 0 of every
        text is `encode_batch(texts, max_len=max_len)`'s row.  Single texts only."""
        L, s = self._window_rule(max_len, stride)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        self._sync_tables()
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            return self._encode_windows_locked(texts, L, s, word_table, False)

    def encode_windows_to_device(self, texts: Sequence[str], max_len: int, stride: int = 0):
        """`encode_windows` whose [W, max_len] input_ids / attention_mask STAY in HBM as `handoff.DeviceArray`s
        (`torch.from_dlpack(x)` is zero-copy, as with `encode_to_device`); doc, start, n_real and win_off are host arrays."""
        L, s = self._window_rule(max_len, stride)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        self._sync_tables()
        with self._batch_lock:
            return self._encode_windows_locked(texts, L, s, True, True)

    @contextlib.contextmanager
    def _encode_ragged_to_device(self, texts, word_table):
        """The texts encoded without a length limit into HBM, enqueued on the context's stream and NOT synchronised, so that what
        shapes the rows goes right behind it: yields (d_ids, d_row_off, n, dev) -- dev(nbytes) allocates more -- and frees every
        allocation on exit."""
        ctx = self._ctx
        t, to = _packing.pack_pinned(texts, self, ctx)
        n = len(to) - 1
        cap = (int(to[n] - to[0]) if n else 0) + 2 * n                 # a token takes a byte of text at least, plus the frame
        bufs = []

        def dev(nbytes):
            d = ctx.alloc(max(int(nbytes), 1) + 64)
            bufs.append(d)
            return d
        try:
            d_t, d_to = dev(t.nbytes), dev(to.nbytes)
            if t.nbytes:
                ctx.h2d(d_t, np.ascontiguousarray(t))
            ctx.h2d(d_to, np.ascontiguousarray(to))
            d_ids, d_mask, d_ro = dev(4 * cap), dev(4 * cap), dev(8 * (n + 1))
            if n:
                ctx.encode_device(d_t, d_to, 0, 0, n, 0, _native.GZ_MAX_LEN_NONE | (0 if word_table else _native.GZ_NO_WORD_TABLE), cap,
                                  d_ids, d_mask, d_row_off=d_ro)
            else:
                ctx.h2d(d_ro, np.zeros(1, dtype=np.int64))
            yield d_ids, d_ro, n, dev
        finally:
            for d in bufs:
                ctx.free(d)

    def _encode_windows_locked(self, texts, L, s, word_table, to_device):
        from .handoff import DeviceArray
        ctx = self._ctx
        with self._encode_ragged_to_device(texts, word_table) as (d_ids, d_ro, n, dev):
            d_wo = dev(8 * (n + 1))
            W = ctx.window_rows_device(d_ids, d_ro, n, L, s, 1, 1, 0, 0, 0, 0, 0, d_wo, 0)
            ctx.sync()                                                 # (what the encode call deferred is reported here)
            cells = max(W * L, 1)
            out = {k: DeviceArray(ctx, ctx.alloc(4 * cells), (W, L)) for k in ("input_ids", "attention_mask")}
            d_meta = dev(12 * W)
            ctx.window_rows_device(d_ids, d_ro, n, L, s, 1, 1, out["input_ids"].ptr, out["attention_mask"].ptr, d_meta, d_meta + 4 * W,
                                   d_meta + 8 * W, d_wo, W)
            meta = np.empty((3, W), dtype=np.int32)
            win_off = np.zeros(n + 1, dtype=np.int64)
            if W:
                ctx.d2h(meta, d_meta)
            ctx.d2h(win_off, d_wo)
            if not to_device:
                out = {k: v.numpy() for k, v in out.items()}           # (the DeviceArrays go with this frame)
            out["doc"], out["start"], out["n_real"], out["win_off"] = meta[0], meta[1], meta[2], win_off
            return out

    @staticmethod
    def join_windows(result, stride: int):
        """The bodies back from a window result (numpy only): (flat int32, row_off int64 [N+1]), body r =
        flat[row_off[r]:row_off[r+1]].  Window 0 gives its whole chunk, every later window its chunk without the first
        `stride` tokens, which the window before it holds already.  The same selection stitches per-token model outputs."""
        ids, n_real, win_off = np.asarray(result["input_ids"]), np.asarray(result["n_real"]), np.asarray(result["win_off"])
        W, s = len(n_real), int(stride)
        first = np.zeros(W, dtype=bool)
        first[win_off[:-1][win_off[:-1] < W]] = True
        lo = np.where(first, 1, 1 + s)[:, None]                        # column of the window's first NEW token (column 0 is bos)
        cols = np.arange(ids.shape[1] if ids.ndim == 2 else 0)[None, :]
        keep = (cols >= lo) & (cols <= (n_real - 2)[:, None])          # the chunk is columns 1 .. n_real - 2
        new = keep.sum(axis=1)
        row_off = np.zeros(len(win_off), dtype=np.int64)
        per_win = np.zeros(W + 1, dtype=np.int64)
        np.cumsum(new, out=per_win[1:])
        row_off[:] = per_win[win_off]
        return ids[keep].astype(np.int32, copy=False), row_off

    # ---- align: word spans, word ids and token labels (token classification) ---------------------------------------------
    ALIGN_UNITS = {"char": 0, "byte": 1}
    ALIGN_SCHEMES = {"plain": 0, "bio": 1}
    ALIGN_CONTINUATIONS = {"ignore": 0, "same": 1, "bio": 2}

    @staticmethod
    def _align_choice(name, v, table):
        if not isinstance(v, str):
            raise TypeError("%s must be a str" % name)
        if v not in table:
            raise ValueError("%s must be one of %s" % (name, ", ".join(repr(k) for k in table)))
        return table[v]

    @staticmethod
    def _align_offsets(call, name, off, total=None):
        """int64 offsets [N+1] from 0, not decreasing (and ending at `total`), or the refusal in the words of `call`"""
        off = np.asarray(off)
        if off.dtype.kind not in "iu":
            raise TypeError("%s() expects integer %s" % (call, name))
        if off.ndim != 1 or len(off) < 1:
            raise ValueError("%s() expects %s as a 1-D array of N + 1 entries" % (call, name))
        off = off.astype(np.int64)
        if off[0] != 0 or (len(off) > 1 and bool(np.any(np.diff(off) < 0))):
            raise ValueError("%s() expects %s that start at 0 and do not decrease" % (call, name))
        if total is not None and int(off[-1]) != total:
            raise ValueError("%s() expects %s that end at %d, the number of entries they index" % (call, name, total))
        return np.ascontiguousarray(off)

    @staticmethod
    def _align_vector(call, name, a, length=None):
        a = _int32_ids(call, a)
        if a.ndim != 1 or (length is not None and len(a) != length):
            raise ValueError("%s() expects %s as a 1-D array%s" % (call, name, "" if length is None else " of %d entries" % length))
        return np.ascontiguousarray(a)

    @classmethod
    def _align_continuation(cls, continuation, word_labels):
        """(mode, map or None) of `continuation`: a name, or an integer array that is the map itself"""
        if isinstance(continuation, str):
            mode = cls._align_choice("continuation", continuation, cls.ALIGN_CONTINUATIONS)
            if mode != 2:
                return mode, None
            top = int(word_labels.max()) + 1 if word_labels is not None and len(word_labels) else 1
            v = np.arange(max(top, 1), dtype=np.int32)
            return 2, np.ascontiguousarray(np.where(v % 2 == 1, v + 1, v).astype(np.int32))      # B-x = 2l + 1 -> I-x = 2l + 2
        cont_map = cls._align_vector("align_rows", "a continuation map", continuation)
        if len(cont_map) < 1:
            raise ValueError("align_rows() expects a continuation map of at least one entry")
        return 2, cont_map

    def word_spans(self, texts: Sequence[str], unit: str = "char"):
        """Where every word of every text stands: (span int32 [W, 2], word_off int64 [N+1]).  span[j] is the [begin, end) of the
        `\\S+` part of word j in its own text -- `str` indices with unit="char", UTF-8 bytes with "byte" -- and text i's words are
        span[word_off[i]:word_off[i+1]], the words `encode_batch(..., return_offset=True)` reports on.  Computed on the GPU."""
        u = self._align_choice("unit", unit, self.ALIGN_UNITS)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        tb, to = _pack(texts)
        return self._ctx.word_spans(tb, to, u)

    def align_rows(self, counts, word_off, max_len: int, word_labels=None, row_doc=None, row_start=None, continuation="ignore",
                   ignore_index: int = -100):
        """The word of every cell of [R, max_len] rows, and its label, on the GPU.  counts [W] / word_off [N+1]: the per-word piece
        counts of an encode call.  Row r holds body tokens row_start[r] .. of document row_doc[r] behind a bos (row_doc None: row r
        is document r; row_start None: 0, the reference's own row; `doc` / `start` of `window_rows` give its windows).  Returns
        word_ids [R, L] (-1 on bos, eos, pad), n_real [R] and, with word_labels [W], labels [R, L]: a word's first piece carries its
        label, a later piece `ignore_index` ("ignore"), the same label ("same"), the I- label of a B- label 2l+1 -> 2l+2 ("bio"),
        or map[label] where `continuation` is an integer array; specials and padding carry `ignore_index`."""
        L = _integer("max_len", max_len, 3, 2 ** 31)
        ig = _integer("ignore_index", ignore_index, -(2 ** 31), 2 ** 31)
        counts = self._align_vector("align_rows", "counts", counts)
        word_off = self._align_offsets("align_rows", "word_off", word_off, len(counts))
        n = len(word_off) - 1
        if len(counts) and int(counts.min()) < 1:
            raise ValueError("align_rows() expects piece counts of at least 1")
        if word_labels is not None:
            word_labels = self._align_vector("align_rows", "word_labels", word_labels, len(counts))
        if row_doc is not None:
            row_doc = self._align_vector("align_rows", "row_doc", row_doc)
            if len(row_doc) and (int(row_doc.min()) < 0 or int(row_doc.max()) >= n):
                raise ValueError("align_rows() expects row_doc inside [0, %d)" % n)
        if row_start is not None:
            row_start = self._align_vector("align_rows", "row_start", row_start, n if row_doc is None else len(row_doc))
            if len(row_start) and int(row_start.min()) < 0:
                raise ValueError("align_rows() expects row_start >= 0")
        mode, cont_map = self._align_continuation(continuation, word_labels)
        return self._ctx.align_rows(counts, word_off, L, word_labels, row_doc, row_start, mode, cont_map, ig)

    @classmethod
    def _align_marks(cls, marks, n):
        """(marks int32 [S, 3], mark_off int64 [N+1]) of a list of (begin, end, label) lists per document, or of that pair itself"""
        if isinstance(marks, tuple) and len(marks) == 2 and isinstance(marks[0], np.ndarray) and marks[0].ndim == 2:
            arr = _int32_ids("span_labels", marks[0])
            if arr.ndim != 2 or arr.shape[1] != 3:
                raise ValueError("span_labels() expects marks as an [S, 3] array of (begin, end, label)")
            return np.ascontiguousarray(arr), cls._align_offsets("span_labels", "mark_off", marks[1], len(arr))
        per_doc = list(marks)
        if len(per_doc) != n:
            raise ValueError("span_labels() expects one list of marks per document: %d documents, %d lists" % (n, len(per_doc)))
        flat, off = [], np.zeros(n + 1, dtype=np.int64)
        for d, ms in enumerate(per_doc):
            for m in ms:
                if len(m) != 3:
                    raise ValueError("span_labels() expects marks of (begin, end, label)")
                flat.append([_integer("a mark's " + k, v, -(2 ** 31), 2 ** 31) for k, v in zip(("begin", "end", "label"), m)])
            off[d + 1] = len(flat)
        return np.asarray(flat, dtype=np.int32).reshape(len(flat), 3), off

    def span_labels(self, span, word_off, marks, scheme: str = "bio", outside: int = 0):
        """Word labels from annotated character spans, on the GPU.  span / word_off of `word_spans`; marks: per document a list of
        (begin, end, label) in the unit of the spans, in any order, or (array [S, 3], mark_off [N+1]).  A mark owns the words it
        overlaps (touching is not overlapping); where marks overlap the one given first wins.  scheme="plain": a word gets its
        mark's label, else `outside`; "bio" (labels >= 0): 0 outside, 2*label+1 on a mark's first owned word, 2*label+2 after it.
        Returns (word_labels int32 [W], mark_words int32 [S, 2]: the [first, last+1) words of its document a mark overlaps, or -1)."""
        sc = self._align_choice("scheme", scheme, self.ALIGN_SCHEMES)
        out = _integer("outside", outside, -(2 ** 31), 2 ** 31)
        span = _int32_ids("span_labels", span)
        if span.ndim != 2 or span.shape[1] != 2:
            raise ValueError("span_labels() expects span as a [W, 2] array")
        word_off = self._align_offsets("span_labels", "word_off", word_off, len(span))
        arr, mark_off = self._align_marks(marks, len(word_off) - 1)
        if len(mark_off) != len(word_off):
            raise ValueError("span_labels() expects mark_off and word_off over the same documents")
        if sc == 1 and len(arr) and (int(arr[:, 2].min()) < 0 or int(arr[:, 2].max()) >= 2 ** 30 - 1):
            raise ValueError("span_labels() with scheme='bio' expects labels in [0, 2**30 - 1)")
        return self._ctx.span_labels(np.ascontiguousarray(span), word_off, arr, mark_off, sc, out)

    def encode_aligned(self, texts: Sequence[str], max_len: int, word_labels=None, marks=None, stride: Optional[int] = None,
                       continuation="ignore", scheme: str = "bio", ignore_index: int = -100, unit: str = "char", word_table: bool = True):
        """Rows for token classification in one call: the texts encoded, and every cell's word and label beside them.
        stride None: one row a text, cut the reference's way (`encode_batch(texts, max_len=max_len)`'s rows); an int: every text
        whole, in `encode_windows`'s overlapping windows.  word_labels: one label per word of the batch (the words of
        `word_spans`), or marks: annotated spans as `span_labels` takes them (not both).  Returns input_ids, attention_mask,
        word_ids [R, L], labels [R, L] (when labels or marks are given), n_real [R], word_off [N+1], word_span [W, 2],
        word_tokens [W] (pieces per word) and, with a stride, doc, start, win_off of the windows.  Single texts only."""
        L = _integer("max_len", max_len, 3, 2 ** 31)
        s = None
        if stride is not None:
            L, s = self._window_rule(max_len, stride)
        if word_labels is not None and marks is not None:
            raise ValueError("encode_aligned() takes word_labels or marks, not both")
        u = self._align_choice("unit", unit, self.ALIGN_UNITS)
        sc = self._align_choice("scheme", scheme, self.ALIGN_SCHEMES)
        ig = _integer("ignore_index", ignore_index, -(2 ** 31), 2 ** 31)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        if word_labels is not None:
            word_labels = self._align_vector("encode_aligned", "word_labels", word_labels)
        if not isinstance(continuation, str):
            self._align_continuation(continuation, None)                  # (refused here, before any device call)
        else:
            self._align_choice("continuation", continuation, self.ALIGN_CONTINUATIONS)
        if marks is not None:
            marks = self._align_marks(marks, len(texts))
            if len(marks[1]) != len(texts) + 1:
                raise ValueError("encode_aligned() expects marks over the same documents as texts")
        n = len(texts)
        self._sync_tables()
        with self._batch_lock:
            tb, to = _pack(texts)
            flags = (0 if word_table else _native.GZ_NO_WORD_TABLE) | _native.GZ_KEEP_WORDS
            if s is None:
                r = self._shape(self._ctx.encode(tb, to, None, None, L, True, True, flags), n)
            else:
                r = self._ctx.encode(tb, to, None, None, None, False, False, flags)
            if n:
                counts, word_off = self._ctx.word_token_counts(0, n, 1 << 16)
            else:
                counts, word_off = np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
            counts = np.ascontiguousarray(counts)
            span, span_off = self._ctx.word_spans(tb, to, u)
            if not np.array_equal(span_off, word_off):
                raise RuntimeError("encode_aligned(): the word spans and the piece counts disagree on the words of the batch")
            if word_labels is not None and len(word_labels) != len(counts):
                raise ValueError("encode_aligned() expects one word label per word: %d words, %d labels" % (len(counts), len(word_labels)))
            out = {}
            if marks is not None:
                if sc == 1 and len(marks[0]) and (int(marks[0][:, 2].min()) < 0 or int(marks[0][:, 2].max()) >= 2 ** 30 - 1):
                    raise ValueError("encode_aligned() with scheme='bio' expects labels in [0, 2**30 - 1)")
                word_labels, out["mark_words"] = self._ctx.span_labels(span, word_off, marks[0], marks[1], sc, 0)
            mode, cont_map = self._align_continuation(continuation, word_labels)
            if s is None:
                out["input_ids"], out["attention_mask"] = r["input_ids"], r["attention_mask"]
                row_doc = row_start = None
            else:
                w = self._ctx.window_rows(r["input_ids"], r["row_off"], L, s, True)
                out["input_ids"], out["attention_mask"] = w["input_ids"], w["attention_mask"]
                out["doc"], out["start"], out["win_off"] = w["doc"], w["start"], w["win_off"]
                row_doc, row_start = w["doc"], w["start"]
            out.update(self._ctx.align_rows(counts, word_off, L, word_labels, row_doc, row_start, mode, cont_map, ig))
            out["word_off"], out["word_span"], out["word_tokens"] = word_off, span, counts
            if word_labels is not None:
                out["word_labels"] = word_labels
            return out

    # ---- pair windows: question-context windows with answer positions (extractive QA, reranking) --------------------------
    @staticmethod
    def _pair_window_rule(max_len, stride, max_query_len=None):
        """(L, s, mq) of a pair window call, or the refusal: L >= 5 (bos, eos, eos, a context token, eos), 0 <= mq <= L - 5 and
        0 <= s <= L - 5 - mq (room = L - 4 - q > s for every q <= mq: every window adds a token).  max_query_len None:
        min(64, L - 5 - s)."""
        for name, v in (("max_len", max_len), ("stride", stride)) + ((("max_query_len", max_query_len),) if max_query_len is not None else ()):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an int" % name)
        L, s = int(max_len), int(stride)
        if L < 5 or L >= 2 ** 31:
            raise ValueError("pair windows need 5 <= max_len < 2**31 (bos, eos, eos, at least one context token, eos)")
        if s < 0:
            raise ValueError("stride must not be negative")
        mq = min(64, L - 5 - s) if max_query_len is None else int(max_query_len)
        if max_query_len is None and mq < 0:
            raise ValueError("stride must lie in [0, max_len - 5]: it leaves no room for a context token")
        if not 0 <= mq <= L - 5:
            raise ValueError("max_query_len must lie in [0, max_len - 5]")
        if s > L - 5 - mq:
            raise ValueError("stride must lie in [0, max_len - 5 - max_query_len]: every window adds at least one new token")
        return L, s, mq

    @staticmethod
    def _pair_q_row(call, q_row, n, nq):
        """q_row as int32 [n] inside [0, nq), or None where pair r uses question r (then nq == n)"""
        if q_row is None:
            if nq != n:
                raise ValueError("%s() without q_row expects one question per context: %d questions, %d contexts" % (call, nq, n))
            return None
        q_row = _int32_ids(call, q_row)
        if q_row.ndim != 1 or len(q_row) != n:
            raise ValueError("%s() expects q_row as a 1-D array of %d entries, one per context" % (call, n))
        if n and (int(q_row.min()) < 0 or int(q_row.max()) >= nq):
            raise ValueError("%s() expects q_row inside [0, %d)" % (call, nq))
        return np.ascontiguousarray(q_row)

    @staticmethod
    def _pair_answers(call, answers, n):
        """answers as int32 [n, 2] (an entry that is None, or a pair with a -1, reads as no answer: (-1, -1)), or None"""
        if answers is None:
            return None
        if not isinstance(answers, np.ndarray):
            answers = list(answers)
            if len(answers) != n:
                raise ValueError("%s() expects one answer per context: %d contexts, %d answers" % (call, n, len(answers)))
            rows = []
            for a in answers:
                if a is None:
                    rows.append((-1, -1))
                    continue
                if len(a) != 2:
                    raise ValueError("%s() expects answers of (begin, end), or None" % call)
                rows.append(tuple(_integer("an answer's " + k, v, -(2 ** 31), 2 ** 31) for k, v in zip(("begin", "end"), a)))
            answers = np.asarray(rows, dtype=np.int32).reshape(n, 2)
        answers = _int32_ids(call, answers)
        if answers.shape != (n, 2):
            raise ValueError("%s() expects answers as an [N, 2] array of (begin, end), one row per context" % call)
        return np.ascontiguousarray(answers)

    def pair_window_rows(self, question_rows, context_rows, max_len: int, stride: int = 0, max_query_len: Optional[int] = None, q_row=None,
                         answers=None, framed: bool = True):
        """Question-context rows over whole contexts, on the GPU: the question stands in front of EVERY window of its context.
        Both row sets as `decode_batch` takes them; `framed=True`: encode results that lose their first and last entry first.
        Pair r is (question q_row[r], context r); q_row None: question r.  With q = min(len(question), max_query_len) (the question
        keeps its first q tokens; max_query_len None: min(64, max_len - 5 - stride)), room = max_len - 4 - q and step = room -
        stride, window j of a context body is [bos] + question[:q] + [eos, eos] + body[j*step : j*step + room] + [eos], padded to
        max_len; the last window is shorter, not shifted back.  A pair that fits makes one window, the reference's own pair row
        (`encode_batch(questions, pair_texts=contexts, max_len=max_len)`).  answers [N, 2]: the [a0, a1) body positions of each
        context's answer, anything else (such as (-1, -1)) for none.
        Returns numpy arrays: input_ids, attention_mask (ids != pad), token_type_ids (0 up to the first separator, 1 from the second
        to the last eos, the pad id behind) [W, L]; pair, start, n_real, q_len [W]; win_off [N+1] (pair r's windows are
        win_off[r]:win_off[r+1]); and, with answers, start_positions, end_positions, has_answer [W]: the columns of the answer's first
        and last token in a window that holds the whole answer, else 0, 0 (the bos column) and has_answer 0."""
        L, s, mq = self._pair_window_rule(max_len, stride, max_query_len)
        qf, qo = self._flat_rows(question_rows)
        cf, co = self._flat_rows(context_rows)
        qf, cf = _int32_ids("pair_window_rows", qf), _int32_ids("pair_window_rows", cf)
        n = len(co) - 1
        q_row = self._pair_q_row("pair_window_rows", q_row, n, len(qo) - 1)
        answers = self._pair_answers("pair_window_rows", answers, n)
        self._sync_tables()
        return self._ctx.pair_window_rows(qf, qo, cf, co, L, s, mq, q_row, answers, bool(framed))

    def span_tokens(self, word_tokens, word_off, mark_words, mark_off):
        """The word ranges `span_labels` returns as body-token ranges, on the GPU.  word_tokens [W] / word_off [N+1]: the per-word
        piece counts of an encode call; mark_words [S, 2] / mark_off [N+1]: per mark the [first, last + 1) words of its document, or
        (-1, -1).  Returns int32 [S, 2]: [first token of the first word, last token of the last word + 1) among the body tokens of
        the mark's document; (-1, -1) stays (-1, -1)."""
        counts = self._align_vector("span_tokens", "word_tokens", word_tokens)
        word_off = self._align_offsets("span_tokens", "word_off", word_off, len(counts))
        if len(counts) and int(counts.min()) < 1:
            raise ValueError("span_tokens() expects piece counts of at least 1")
        mark_words = _int32_ids("span_tokens", mark_words)
        if mark_words.ndim != 2 or mark_words.shape[1] != 2:
            raise ValueError("span_tokens() expects mark_words as an [S, 2] array")
        mark_off = self._align_offsets("span_tokens", "mark_off", mark_off, len(mark_words))
        if len(mark_off) != len(word_off):
            raise ValueError("span_tokens() expects mark_off and word_off over the same documents")
        if len(mark_words):
            doc = np.searchsorted(mark_off, np.arange(len(mark_words)), side="right") - 1
            words = np.diff(word_off)[doc]
            f, e = mark_words[:, 0].astype(np.int64), mark_words[:, 1].astype(np.int64)
            if not bool(np.all(((f == -1) & (e == -1)) | ((0 <= f) & (f <= e) & (e <= words)))):
                raise ValueError("span_tokens() expects word ranges that are (-1, -1) or 0 <= first <= last + 1 <= the document's words")
        return self._ctx.span_tokens(counts, word_off, np.ascontiguousarray(mark_words), mark_off)

    def encode_pair_windows(self, questions: Sequence[str], contexts: Sequence[str], max_len: int, stride: int = 0,
                            max_query_len: Optional[int] = None, q_row=None, answers=None, unit: str = "char", word_table: bool = True):
        """`pair_window_rows` over texts, with answers given as character spans: questions and contexts are encoded without a length
        limit, and every answer goes from characters to words (`word_spans`, `span_labels`: an answer owns the words it overlaps,
        so positions are word-granular), from words to body tokens (`span_tokens`) and from there into the columns of every window
        that holds it.  answers: one (begin, end) span of its context per context in `unit`s ("char": str indices, "byte"), or None
        for none, or an [N, 2] array with -1 for none.  Returns the dict of `pair_window_rows` and word_off [N+1], word_span [W, 2],
        word_tokens [W] of the contexts and, with answers, answer_tokens [N, 2] (the body positions, -1 for none);
        `pair_window_spans` maps predicted columns back to characters."""
        return self._encode_pair_windows(questions, contexts, max_len, stride, max_query_len, q_row, answers, unit, word_table, False)

    def encode_pair_windows_to_device(self, questions: Sequence[str], contexts: Sequence[str], max_len: int, stride: int = 0,
                                      max_query_len: Optional[int] = None, q_row=None, answers=None, unit: str = "char", word_table: bool = True):
        """`encode_pair_windows` whose [W, max_len] input_ids / attention_mask / token_type_ids STAY in HBM as `handoff.DeviceArray`s
        (`torch.from_dlpack(x)` is zero-copy, as with `encode_windows_to_device`); every other entry is a host array."""
        return self._encode_pair_windows(questions, contexts, max_len, stride, max_query_len, q_row, answers, unit, word_table, True)

    def _encode_pair_windows(self, questions, contexts, max_len, stride, max_query_len, q_row, answers, unit, word_table, to_device):
        L, s, mq = self._pair_window_rule(max_len, stride, max_query_len)
        u = self._align_choice("unit", unit, self.ALIGN_UNITS)
        questions, contexts = list(questions), list(contexts)
        for t in questions + contexts:
            _require_str(t)
        n, nq = len(contexts), len(questions)
        q_row = self._pair_q_row("encode_pair_windows", q_row, n, nq)
        answers = self._pair_answers("encode_pair_windows", answers, n)
        self._sync_tables()
        with self._batch_lock:
            flags = 0 if word_table else _native.GZ_NO_WORD_TABLE
            qb, qo = _pack(questions)
            rq = self._ctx.encode(qb, qo, None, None, None, False, False, flags)
            tb, to = _pack(contexts)
            rc = self._ctx.encode(tb, to, None, None, None, False, False, flags | _native.GZ_KEEP_WORDS)
            if n:
                counts, word_off = self._ctx.word_token_counts(0, n, 1 << 16)
            else:
                counts, word_off = np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
            counts = np.ascontiguousarray(counts)
            span, span_off = self._ctx.word_spans(tb, to, u)
            if not np.array_equal(span_off, word_off):
                raise RuntimeError("encode_pair_windows(): the word spans and the piece counts disagree on the words of the batch")
            answer_tokens = None
            if answers is not None:
                gone = (answers < 0).any(axis=1)
                marks = np.zeros((n, 3), dtype=np.int32)
                marks[:, :2] = np.where(gone[:, None], 0, answers)                # (a mark with end <= begin overlaps nothing)
                mark_off = np.arange(n + 1, dtype=np.int64)
                _, mark_words = self._ctx.span_labels(span, word_off, marks, mark_off, 0, 0)
                answer_tokens = self._ctx.span_tokens(counts, word_off, mark_words, mark_off)
            args = (rq["input_ids"], rq["row_off"], rc["input_ids"], rc["row_off"], L, s, mq, q_row, answer_tokens)
            out = self._pair_windows_to_device_locked(*args) if to_device else self._ctx.pair_window_rows(*args, True)
            out["word_off"], out["word_span"], out["word_tokens"] = word_off, span, counts
            if answer_tokens is not None:
                out["answer_tokens"] = answer_tokens
            return out

    def _pair_windows_to_device_locked(self, q_ids, q_off, ids, row_off, L, s, mq, q_row, answers):
        from .handoff import DeviceArray
        ctx = self._ctx
        n, nq = len(row_off) - 1, len(q_off) - 1
        bufs = []

        def up(a, dtype):
            if a is None:
                return 0
            a = np.ascontiguousarray(a, dtype=dtype)
            d = ctx.alloc(max(a.nbytes, 1) + 64)
            bufs.append(d)
            if a.nbytes:
                ctx.h2d(d, a)
            return d
        try:
            d_q, d_qo, d_c, d_co = up(q_ids, np.int32), up(q_off, np.int64), up(ids, np.int32), up(row_off, np.int64)
            d_qr, d_ans = up(q_row, np.int32), up(answers, np.int32)
            d_wo = up(np.zeros(n + 1, dtype=np.int64), np.int64)
            head = (d_q, d_qo, nq, d_c, d_co, n, d_qr, d_ans, L, s, mq, 1, 1)
            W = ctx.pair_window_rows_device(*head, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_wo, 0)
            names = _native.Context.PAIRWIN_META + (_native.Context.PAIRWIN_ANSWER if answers is not None else ())
            out = {k: DeviceArray(ctx, ctx.alloc(4 * max(W * L, 1)), (W, L)) for k in _native.Context.PAIRWIN_CELLS}
            d_meta = up(np.zeros((7, max(W, 1)), dtype=np.int32), np.int32)
            meta_ptrs = [d_meta + 4 * W * k if k < len(names) else 0 for k in range(7)]
            ctx.pair_window_rows_device(*head, out["input_ids"].ptr, out["attention_mask"].ptr, out["token_type_ids"].ptr, *meta_ptrs, d_wo, W)
            meta = np.empty((7, W), dtype=np.int32)
            win_off = np.zeros(n + 1, dtype=np.int64)
            if W:
                ctx.d2h(meta, d_meta)
            ctx.d2h(win_off, d_wo)
            for k, name in enumerate(names):
                out[name] = meta[k]
            out["win_off"] = win_off
            return out
        finally:
            for d in bufs:
                ctx.free(d)

    @staticmethod
    def pair_window_spans(result, start_cols, end_cols):
        """Predicted columns back to characters (host numpy): for every window w of an `encode_pair_windows` result the (begin, end)
        span of its context, in the result's unit, that runs from the begin of the word of column start_cols[w]'s token to the end of
        the word of column end_cols[w]'s token.  Returns int32 [W, 2]; a column outside the window's chunk, or end < start, gives
        (-1, -1).  Fed `start_positions` / `end_positions` of windows with `has_answer`, it returns the span of the words the answer
        overlaps."""
        pair, start = np.asarray(result["pair"], dtype=np.int64), np.asarray(result["start"], dtype=np.int64)
        n_real, q_len = np.asarray(result["n_real"], dtype=np.int64), np.asarray(result["q_len"], dtype=np.int64)
        word_off, span = np.asarray(result["word_off"], dtype=np.int64), np.asarray(result["word_span"])
        counts = np.asarray(result["word_tokens"], dtype=np.int64)
        sc, ec = np.asarray(start_cols, dtype=np.int64).reshape(-1), np.asarray(end_cols, dtype=np.int64).reshape(-1)
        W = len(pair)
        if len(sc) != W or len(ec) != W:
            raise ValueError("pair_window_spans() expects one start column and one end column per window: %d windows" % W)
        out = np.full((W, 2), -1, dtype=np.int32)
        if not W:
            return out
        ends = np.cumsum(counts)                                           # tokens of the batch up to and including word j
        doc_tok0 = np.concatenate(([0], ends))[word_off[:-1]]              # tokens of the batch before a document's first word
        ctx_col, n = q_len + 3, n_real - q_len - 4
        ok = (sc >= ctx_col) & (ec < ctx_col + n) & (sc <= ec)
        t0 = doc_tok0[pair] + start + sc - ctx_col                         # batch-wide token positions
        t1 = doc_tok0[pair] + start + ec - ctx_col
        w0 = np.searchsorted(ends, np.where(ok, t0, 0), side="right")
        w1 = np.searchsorted(ends, np.where(ok, t1, 0), side="right")
        ok &= (w1 < len(counts)) if len(counts) else False
        out[ok, 0] = span[w0[ok], 0]
        out[ok, 1] = span[w1[ok], 1]
        return out

    # ---- short documents packed into rows of max_len ("sequence packing") -------------------------------------------
    PACK_CELLS = ("input_ids", "attention_mask", "segment_ids", "position_ids")
    PACK_MAPS = ("doc_row", "doc_col", "doc_len")

    @staticmethod
    def _pack_rule(max_len):
        """L of a pack call, or the refusal: L >= 3 (bos, a token, eos)."""
        if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)):
            raise TypeError("max_len must be an int")
        L = int(max_len)
        if L < 3 or L >= 2 ** 31:
            raise ValueError("packed rows need 3 <= max_len < 2**31 (bos, at least one token, eos)")
        return L

    PACK_FIT_MAX_LEN = 4096                          # GZ_PACK_FIT_MAX_LEN: the longest row order="fit" takes

    @classmethod
    def _pack_order(cls, order, L):
        """True for order="fit", False for "kept", or the refusal."""
        if order not in ("kept", "fit"):
            raise ValueError('order must be "kept" or "fit"')
        if order == "fit" and L > cls.PACK_FIT_MAX_LEN:
            raise ValueError('order="fit" needs max_len <= %d' % cls.PACK_FIT_MAX_LEN)
        return order == "fit"

    def pack_rows(self, rows, max_len: int, framed: bool = True, order: str = "kept"):
        """Lay token rows back to back into rows of `max_len`, on the GPU.  `rows` as `window_rows` takes them (`framed=True`:
        each row is an encode result and loses its first and last entry first, `False`: bare bodies).  Document r becomes
        [bos] + body[:max_len-2] + [eos] -- the reference's own row without its padding (tokenize.py:141-146) -- and goes behind
        the documents before it, or opens the next row when it does not fit (next-fit: the order is kept).  Returns numpy
        arrays: input_ids, attention_mask (ids != pad), segment_ids (1 + the document's index within its row; 0 in the padding
        tail only), position_ids (column - doc_col; 0 in the tail), all [R, L]; doc_row, doc_col, doc_len [N]; row_off int64
        [R+1] (packed row i holds documents row_off[i]:row_off[i+1]); seg_off int64 [N+1] (the scan of doc_len: the cumulative
        sequence lengths variable-length attention kernels take).

        `order="fit"` (max_len <= 4096) places the same segments by best-fit-decreasing instead: the documents are taken from the
        longest to the shortest (ties by index) and each goes into the open row with the least free space that still takes it
        (ties: the row touched longest ago), or opens a new row.  Rows fill almost completely (0.997 full against next-fit's 0.79 on the
        1 M-document corpus at max_len 128: DESIGN.md, Packs) and come out ordered from the longest documents to the shortest: a trainer shuffles rows.
        The result has one more key, row_docs int32 [N]: the document indices in packed order, sorted by (doc_row, doc_col).
        row_off then indexes row_docs (row i holds documents row_docs[row_off[i]:row_off[i+1]], in column order), seg_off is the
        scan of doc_len[row_docs] (the segments' lengths in the order they lie in the rows), and doc_row, doc_col, doc_len stay
        indexed by document.  `unpack_rows` gives the segments back in document order either way."""
        L = self._pack_rule(max_len)
        fit = self._pack_order(order, L)
        flat, off = self._flat_rows(rows)
        flat = _int32_ids("pack_rows", flat)
        self._sync_tables()
        return (self._ctx.pack_rows_fit if fit else self._ctx.pack_rows)(flat, off, L, bool(framed))

    def _encode_packs_call(self, texts, max_len, word_table, to_device, order):
        """What the three text doors share: the rule, the texts, the tables, the lock."""
        L = self._pack_rule(max_len)
        fit = self._pack_order(order, L)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        self._sync_tables()
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            return self._encode_packs_locked(texts, L, word_table, to_device, fit)

    def encode_packs(self, texts: Sequence[str], max_len: int, word_table: bool = True):
        """`pack_rows` over the texts: they are encoded without a length limit on the device, packed there, and only the packed
        rows and the maps come back.  Segment r of the result is `tok(texts[r], max_len=max_len)["input_ids"]` without its
        padding.  Single texts only.  (`encode_packs_fit` is this call with `order="fit"`.)"""
        return self._encode_packs_call(texts, max_len, word_table, False, "kept")

    def encode_packs_fit(self, texts: Sequence[str], max_len: int, word_table: bool = True):
        """`encode_packs` in best-fit order: `pack_rows(..., order="fit")` over the texts, with row_docs among the maps.  Rows come out
        ordered from the longest documents to the shortest; a trainer shuffles rows."""
        return self._encode_packs_call(texts, max_len, word_table, False, "fit")

    def encode_packs_to_device(self, texts: Sequence[str], max_len: int, order: str = "kept"):
        """`encode_packs` whose four [R, max_len] arrays STAY in HBM as `handoff.DeviceArray`s (`torch.from_dlpack(x)` is
        zero-copy, as with `encode_to_device`); doc_row, doc_col, doc_len, row_off and seg_off are host arrays.  `order="fit"`
        packs by best-fit-decreasing as `pack_rows` describes it; row_docs is a host array too."""
        return self._encode_packs_call(texts, max_len, True, True, order)

    def _encode_packs_locked(self, texts, L, word_table, to_device, fit=False):
        from .handoff import DeviceArray
        ctx = self._ctx
        with self._encode_ragged_to_device(texts, word_table) as (d_ids, d_ro, n, dev):
            n_maps = 4 if fit else 3                                   # doc_row, doc_col, doc_len and, in best-fit order, row_docs
            d_maps, d_po, d_so = dev(4 * n_maps * n), dev(8 * (n + 1)), dev(8 * (n + 1))
            maps = tuple(d_maps + 4 * n * k for k in range(n_maps)) if n else (0,) * n_maps
            call = ctx.pack_rows_fit_device if fit else ctx.pack_rows_device
            R = call(d_ids, d_ro, n, L, 1, 1, 0, 0, 0, 0, *maps, d_po, d_so, 0)
            ctx.sync()                                                 # (what the encode call deferred is reported here)
            cells = max(R * L, 1)
            out = {k: DeviceArray(ctx, ctx.alloc(4 * cells), (R, L)) for k in self.PACK_CELLS}
            call(d_ids, d_ro, n, L, 1, 1, *[out[k].ptr for k in self.PACK_CELLS], *maps, d_po, d_so, R)
            meta = np.empty((n_maps, n), dtype=np.int32)
            row_off, seg_off = np.zeros(R + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
            if n:
                ctx.d2h(meta, d_maps)
            ctx.d2h(row_off, d_po)
            ctx.d2h(seg_off, d_so)
            if not to_device:
                out = {k: v.numpy() for k, v in out.items()}           # (the DeviceArrays go with this frame)
            out["doc_row"], out["doc_col"], out["doc_len"], out["row_off"], out["seg_off"] = meta[0], meta[1], meta[2], row_off, seg_off
            if fit:
                out["row_docs"] = meta[3]
            return out

    @staticmethod
    def unpack_rows(result):
        """The segments back from a pack result (numpy only): (flat int32, row_off int64 [N+1]), segment r =
        flat[row_off[r]:row_off[r+1]] = [bos] + body + [eos].  Segments lie in document order in the packed rows and the tail
        of a row has segment id 0, so one selection does it; the same selection un-packs per-token model outputs.  A result of
        `order="fit"` (it has row_docs) lies in packed order: the selection is gathered back so that segment r is still
        document r, and row_off is the scan of doc_len."""
        ids, seg = np.asarray(result["input_ids"]), np.asarray(result["segment_ids"])
        flat = ids[seg != 0].astype(np.int32, copy=False)
        if "row_docs" not in result:
            return flat, np.asarray(result["seg_off"], dtype=np.int64).copy()
        doc_len = np.asarray(result["doc_len"], dtype=np.int64)
        row_docs, seg_off = np.asarray(result["row_docs"], dtype=np.int64), np.asarray(result["seg_off"], dtype=np.int64)
        off = np.zeros(len(doc_len) + 1, dtype=np.int64)
        np.cumsum(doc_len, out=off[1:])
        src = np.empty(len(doc_len), dtype=np.int64)                  # where document d's segment starts in the packed selection
        src[row_docs] = seg_off[:-1]
        take = np.repeat(src - off[:-1], doc_len) + np.arange(off[-1], dtype=np.int64)
        return flat[take], off

    # ---- what the dense-row calls (mask_rows*, infill_rows*) share ----------------------------------------------------
    def _dense_prologue(self, base, R, L):
        """mask_id, once the cell indices are known to fit and the tables are on the device"""
        if (base + R) * L >= 2 ** 63:
            raise ValueError("(row_base + rows) * row length must stay below 2**63")
        self._sync_tables()
        mask_id = self._special_ids()[3]                               # encoder[mask_token], looked up at call time
        if mask_id < 0:
            raise KeyError(self.mask_token)
        return mask_id

    def _device_rows(self, name, x):
        """(R, L) of int32 rows in this object's HBM, refused in the words of the call `name`"""
        from .handoff import DeviceArray
        if not isinstance(x, DeviceArray):
            raise TypeError("%s() expects a handoff.DeviceArray" % name)
        if x.dtype != np.int32:
            raise TypeError("%s() expects int32 ids" % name)
        if len(x.shape) != 2 or x.shape[1] < 1 or x.shape[1] >= 2 ** 31:
            raise ValueError("%s() expects rows [R, L] with 1 <= L < 2**31" % name)
        if x._ctx is not self._ctx:
            raise ValueError("the rows belong to another Tokenize object's device context")
        return x.shape

    def _owned_rows(self, R, width):
        """a fresh [R, width] int32 DeviceArray (an allocation nothing owns yet is freed when its DeviceArray fails)"""
        from .handoff import DeviceArray
        d = self._ctx.alloc(4 * max(R * width, 1))
        try:
            return DeviceArray(self._ctx, d, (R, width))
        except BaseException:
            self._ctx.free(d)
            raise

    # ---- masked-LM inputs and labels, whole-word ---------------------------------------------------------------------
    @staticmethod
    def _mask_rule(p, seed, whole_word, mask_prob, random_prob, random_ids, row_base, ignore_index):
        """The arguments of a mask call as integers -- (seed, t_sel, t1, t2, rand_lo, rand_hi (None: the vocabulary), whole_word,
        ignore_index, row_base) -- or the refusal.  Thresholds are floor(x * 2**32): exact, a float times a power of two."""
        p, mp, rp = _share("p", p), _share("mask_prob", mask_prob), _share("random_prob", random_prob)
        if mp + rp > 1:
            raise ValueError("mask_prob + random_prob must not exceed 1")
        if not isinstance(whole_word, (bool, np.bool_)):
            raise TypeError("whole_word must be a bool")
        one = 2 ** 32
        t_sel, t1, t2 = int(p * one), int(mp * one), min(int((mp + rp) * one), one)
        lo = hi = None
        if random_ids is not None:
            if not isinstance(random_ids, (tuple, list)) or len(random_ids) != 2:
                raise TypeError("random_ids must be None or a pair (lo, hi)")
            lo = _integer("random_ids[0]", random_ids[0], -(2 ** 31), 2 ** 31)
            hi = _integer("random_ids[1]", random_ids[1], -(2 ** 31), 2 ** 31)
            if lo >= hi:
                raise ValueError("random_ids must be a non-empty range [lo, hi)")
        return (_integer("seed", seed, 0, 2 ** 64), t_sel, t1, t2, lo, hi, int(bool(whole_word)),
                _integer("ignore_index", ignore_index, -(2 ** 31), 2 ** 31), _integer("row_base", row_base, 0, 2 ** 63))

    def _mask_call(self, rule, R, L):
        """(the nine arguments of gz_mask_rows behind row_base, row_base) once the tables are known"""
        seed, t_sel, t1, t2, lo, hi, ww, ignore, base = rule
        mask_id = self._dense_prologue(base, R, L)
        if lo is None:
            lo, hi = 5, self.vocab_size()                              # (the five specials hold ids 0 .. 4, tokenize.py:31-37)
            if hi <= lo:
                raise ValueError("the vocabulary holds nothing but the specials: give random_ids")
        return (seed, t_sel, t1, t2, lo, hi, mask_id, ww, ignore), base

    def mask_rows(self, input_ids, p=0.15, seed=0, whole_word=True, mask_prob=0.8, random_prob=0.1, random_ids=None, row_base=0,
                  ignore_index=-100):
        """Masked-LM inputs and labels from dense [R, L] rows (the input_ids of `encode_batch`, `encode_windows`, `encode_packs`),
        on the GPU.  A cell that holds pad, bos, eos or <mask> is never touched.  Of the others a share `p` is chosen -- with
        `whole_word=True` word by word: the pieces "xx@@ yy@@ zz" of a word go together, and words end at protected cells and at
        the row's edge -- and a chosen cell becomes <mask> (share `mask_prob`), a random id from `random_ids` = (lo, hi), default
        (5, vocab_size()) (share `random_prob`), or stays.  The draw is Philox4x32-10 keyed by `seed` over the cell's global
        position (row_base + r) * L + c: the same seed gives the same cells whatever the batch is cut into
        (`mask_rows(rows[a:b], row_base=a)` is `mask_rows(rows)[a:b]`); a new epoch is a new seed.  Returns numpy arrays:
        input_ids [R, L], labels [R, L] (the original id where chosen, `ignore_index` elsewhere), n_chosen [R].  The attention
        mask is the caller's and does not change."""
        rule = self._mask_rule(p, seed, whole_word, mask_prob, random_prob, random_ids, row_base, ignore_index)
        ids = _int32_ids("mask_rows", input_ids, dense=True)
        args, base = self._mask_call(rule, *ids.shape)
        return self._ctx.mask_rows(ids, args, base)

    def mask_rows_to_device(self, input_ids, p=0.15, seed=0, whole_word=True, mask_prob=0.8, random_prob=0.1, random_ids=None,
                            row_base=0, ignore_index=-100):
        """`mask_rows` over rows that are in HBM already and stay there: `input_ids` is a `handoff.DeviceArray` -- the input_ids of
        `encode_to_device`, `encode_windows_to_device` or `encode_packs_to_device` -- and input_ids and labels come back as
        `DeviceArray`s (`torch.from_dlpack(x)` is zero-copy); n_chosen is a host array.  The source rows are not changed."""
        rule = self._mask_rule(p, seed, whole_word, mask_prob, random_prob, random_ids, row_base, ignore_index)
        R, L = self._device_rows("mask_rows_to_device", input_ids)
        args, base = self._mask_call(rule, R, L)
        ctx = self._ctx
        out = {"input_ids": self._owned_rows(R, L)}
        out["labels"] = self._owned_rows(R, L)
        n_chosen = np.zeros(R, dtype=np.int32)
        d_cnt = ctx.alloc(4 * max(R, 1))
        try:
            ctx.mask_rows_device(input_ids.ptr if R else 0, R, L, base, args, out["input_ids"].ptr if R else 0,
                                 out["labels"].ptr if R else 0, d_cnt if R else 0)
            if R:
                ctx.d2h(n_chosen, d_cnt)
        finally:
            ctx.free(d_cnt)
        out["n_chosen"] = n_chosen
        return out

    # ---- span-corruption inputs and targets for encoder-decoder models ----------------------------------------------
    @staticmethod
    def _infill_lengths(lengths, mean_span, max_span):
        """P(len = 1 .. n_len) of a span's length in words: the law truncated at max_span and renormalised"""
        if lengths == "fixed":
            return [0.0] * (int(mean_span) - 1) + [1.0]
        if lengths == "geometric":
            r = 1.0 / mean_span
            w = [r * (1.0 - r) ** (k - 1) for k in range(1, max_span + 1)]
        else:                                                          # "poisson", without the zero-length spans
            w = [math.exp(-mean_span) * mean_span ** k / math.factorial(k) for k in range(1, max_span + 1)]
        total = sum(w)
        return [x / total for x in w]

    @staticmethod
    def _infill_coverage(q, tail):
        """1 - prod_k (1 - q P(len > k)): the probability that a word with at least n_len - 1 words before it in its row lies in
        a span, when every word begins one with probability q"""
        prod = 1.0
        for t in tail:
            prod *= 1.0 - q * t
        return 1.0 - prod

    @staticmethod
    def _infill_start_share(p, tail):
        """q with _infill_coverage(q, tail) == p, by bisection (the coverage rises from 0 at q = 0 to 1 at q = 1)"""
        if p <= 0.0 or p >= 1.0:
            return float(p)
        lo, hi = 0.0, 1.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if Tokenize._infill_coverage(mid, tail) < p:
                lo = mid
            else:
                hi = mid
        return hi

    @staticmethod
    def _infill_rule(p, mean_span, max_span, lengths, seed, whole_word, dec_len, row_base, ignore_index):
        """The arguments of an infill call as integers -- (seed, t_start, len_t (n_len - 1 thresholds), n_len, whole_word,
        ignore_index, dec_len (None: the row length), row_base) -- or the refusal.  t_start = floor(q * 2**32) with q solved from
        the coverage formula; len_t[k] = floor(P(len <= k + 1) * 2**32), non-decreasing."""
        p = _number("p", p)
        if not 0 <= p <= 1:                                            # (NaN fails here too)
            raise ValueError("p must lie in [0, 1]")
        max_span = _integer("max_span", max_span, 1, 17)
        mean_span = _number("mean_span", mean_span)
        if not isinstance(lengths, str):
            raise TypeError("lengths must be a str")
        if lengths not in ("geometric", "poisson", "fixed"):
            raise ValueError('lengths must be "geometric", "poisson" or "fixed"')
        if not 1 <= mean_span <= max_span:                             # (NaN and infinities fail here)
            raise ValueError("mean_span must lie in [1, max_span]")
        if lengths == "fixed" and mean_span != int(mean_span):
            raise ValueError('lengths="fixed" needs a whole mean_span')
        if not isinstance(whole_word, (bool, np.bool_)):
            raise TypeError("whole_word must be a bool")
        if dec_len is not None:
            dec_len = _integer("dec_len", dec_len, 1, 2 ** 31)
        seed = _integer("seed", seed, 0, 2 ** 64)
        ignore_index = _integer("ignore_index", ignore_index, -(2 ** 31), 2 ** 31)
        row_base = _integer("row_base", row_base, 0, 2 ** 63)
        one = 2 ** 32
        pmf = Tokenize._infill_lengths(lengths, mean_span, max_span)
        tail = [max(0.0, 1.0 - sum(pmf[:k])) if k else 1.0 for k in range(len(pmf))]
        q = Tokenize._infill_start_share(p, tail)
        len_t, acc, last = [], 0.0, 0
        for k in range(len(pmf) - 1):
            acc += pmf[k]
            last = max(last, min(int(min(acc, 1.0) * one), one))
            len_t.append(last)
        return (seed, int(q * one), len_t, len(pmf), int(bool(whole_word)), ignore_index, dec_len, row_base)

    def _infill_call(self, rule, R, L):
        """(the rule of _native.Context.infill_rows, row_base) once the tables are known"""
        seed, t_start, len_t, n_len, ww, ignore, dec_len, base = rule
        mask_id = self._dense_prologue(base, R, L)
        return (seed, t_start, len_t, n_len, mask_id, ww, ignore, L if dec_len is None else dec_len), base

    def infill_rows(self, input_ids, p=0.15, mean_span=3.0, max_span=10, lengths="geometric", seed=0, whole_word=True, dec_len=None,
                    row_base=0, ignore_index=-100):
        """Span-corruption inputs and targets for an encoder-decoder model (the denoising objective of T5, MASS and
        BART-infilling) from dense [R, L] rows, on the GPU.  Spans of whole words are chosen so that about a share `p` of the
        tokens lies inside one: every word begins a span with probability q, and a span is 1 .. `max_span` (<= 16) words long
        -- `lengths` = "geometric" (mean `mean_span` before truncation), "poisson" (lambda `mean_span`, no empty spans) or
        "fixed" (`mean_span` words) --, the law truncated at `max_span` and renormalised; q is solved so that a word with
        max_span - 1 words before it in its row is covered with probability exactly p, hence the realised share near a row's
        start is lower.  Overlapping and touching spans merge.  Cells that hold pad, bos, eos or <mask> are never chosen and end
        a run.  Each run collapses to ONE <mask> in the encoder row, pads drop out and the row closes up; the target is, run by
        run, <mask> and the run's ids, closed by eos.  With `whole_word=False` every token is a word.  The draw is counter-based
        as in `mask_rows` (`infill_rows(rows[a:b], row_base=a)` is `infill_rows(rows)[a:b]`; the same seed gives draws
        correlated with `mask_rows`).  Returns numpy arrays: input_ids and attention_mask [R, L]; labels (target, then
        `ignore_index`) and decoder_input_ids (bos + target shifted, then pad) [R, `dec_len`] (None: L); enc_len, dec_len and
        n_spans [R] -- dec_len is the target's whole length, so `dec_len > labels.shape[1]` marks a clipped row.  BART's
        full-sequence target is the row you passed in."""
        rule = self._infill_rule(p, mean_span, max_span, lengths, seed, whole_word, dec_len, row_base, ignore_index)
        ids = _int32_ids("infill_rows", input_ids, dense=True)
        args, base = self._infill_call(rule, *ids.shape)
        return self._ctx.infill_rows(ids, args, base)

    def infill_rows_to_device(self, input_ids, p=0.15, mean_span=3.0, max_span=10, lengths="geometric", seed=0, whole_word=True,
                              dec_len=None, row_base=0, ignore_index=-100):
        """`infill_rows` over rows that are in HBM already and stay there: `input_ids` is a `handoff.DeviceArray` -- the
        input_ids of `encode_to_device`, `encode_windows_to_device` or `encode_packs_to_device` -- and input_ids,
        attention_mask, labels and decoder_input_ids come back as `DeviceArray`s (`torch.from_dlpack(x)` is zero-copy);
        enc_len, dec_len and n_spans are host arrays.  The source rows are not changed."""
        rule = self._infill_rule(p, mean_span, max_span, lengths, seed, whole_word, dec_len, row_base, ignore_index)
        R, L = self._device_rows("infill_rows_to_device", input_ids)
        args, base = self._infill_call(rule, R, L)
        W = args[7]
        ctx = self._ctx
        out = {"input_ids": self._owned_rows(R, L)}
        out["attention_mask"] = self._owned_rows(R, L)
        out["labels"] = self._owned_rows(R, W)
        out["decoder_input_ids"] = self._owned_rows(R, W)
        counts = np.zeros((3, R), dtype=np.int32)
        d_cnt = ctx.alloc(12 * max(R, 1))
        try:
            ctx.infill_rows_device(input_ids.ptr if R else 0, R, L, base, args, *[out[k].ptr if R else 0 for k in out],
                                   *[d_cnt + 4 * R * k if R else 0 for k in range(3)])
            if R:
                ctx.d2h(counts, d_cnt)
        finally:
            ctx.free(d_cnt)
        out["enc_len"], out["dec_len"], out["n_spans"] = counts[0], counts[1], counts[2]
        return out

    # ---- near-duplicate documents by MinHash signatures --------------------------------------------------------------
    @staticmethod
    def _minhash_rule(num_perm=128, shingle=5, seed=0, bands=16, threshold=0.7, min_agree=None):
        """The arguments of the MinHash calls as integers -- (num_perm, shingle, seed, bands, min_agree) -- or the refusal;
        min_agree defaults to max(1, ceil(threshold * num_perm))."""
        K = _integer("num_perm", num_perm, 1, 257)
        w = _integer("shingle", shingle, 1, 33)
        seed = _integer("seed", seed, 0, 2 ** 64)
        B = _integer("bands", bands, 1, 257)
        if K % B:
            raise ValueError("bands must divide num_perm")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
            raise TypeError("threshold must be a number")
        if not 0 < threshold <= 1:                                         # (NaN fails here too)
            raise ValueError("threshold must lie in (0, 1]")
        if min_agree is None:
            m = max(1, int(math.ceil(float(threshold) * K)))
        else:
            m = _integer("min_agree", min_agree, 1, K + 1)
        return K, w, seed, B, m

    def minhash_rows(self, rows, num_perm=128, shingle=5, seed=0, framed=True):
        """MinHash signatures of token rows, on the GPU.  `rows` as `decode_batch` / `window_rows` take them (`framed=True`: each
        row loses its first and last entry first).  A body's shingles are its runs of `shingle` ids (the whole body when it is
        shorter, none when it is empty), each hashed with MurmurHash3 over the ids; slot k of the signature is the minimum over
        the shingles of fmix32(hash ^ c_k), the c_k drawn from `seed`, and 0xFFFFFFFF in every slot without shingles -- the
        share of equal slots of two signatures estimates the Jaccard index of the two shingle sets.  A row's signature depends
        on its own body alone: `minhash_rows(rows[a:b])` is `minhash_rows(rows)[a:b]`, and signatures of shards concatenate.
        Returns numpy arrays: signatures uint32 [N, num_perm], n_shingles int32 [N]."""
        K, w, seed, _, _ = self._minhash_rule(num_perm, shingle, seed, 1)                # (no bands here: one always divides)
        flat, off = self._flat_rows(rows)
        flat = _int32_ids("minhash_rows", flat)
        return self._ctx.minhash_rows(flat, off, K, w, seed, bool(framed))

    def encode_minhash(self, texts: Sequence[str], num_perm=128, shingle=5, seed=0, word_table=True):
        """`minhash_rows` over the whole token sequence of every text: the texts are encoded without a length limit on the
        device, the signatures are made there, and only they come back, uint32 [N, num_perm].  The rule is `minhash_rows`'s,
        over the rows of `encode_batch(texts, max_len=None)` without their frame; `encode_minhash(texts[a:b])` is
        `encode_minhash(texts)[a:b]`, and signatures of shards concatenate.  Single texts only."""
        return self._encode_minhash(texts, num_perm, shingle, seed, word_table).numpy()

    def encode_minhash_to_device(self, texts: Sequence[str], num_perm=128, shingle=5, seed=0):
        """`encode_minhash` whose [N, num_perm] signatures STAY in HBM as a `handoff.DeviceArray` of dtype uint32, ready for
        `minhash_groups`; the same rule, and the same slicing identity: signatures of shards concatenate."""
        return self._encode_minhash(texts, num_perm, shingle, seed, True)

    def _encode_minhash(self, texts, num_perm, shingle, seed, word_table):
        from .handoff import DeviceArray
        K, w, seed, _, _ = self._minhash_rule(num_perm, shingle, seed, 1)                # (no bands here: one always divides)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        self._sync_tables()
        ctx = self._ctx
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            with self._encode_ragged_to_device(texts, word_table) as (d_ids, d_ro, n, dev):
                d_sig = ctx.alloc(4 * max(n * K, 1))
                try:
                    sig = DeviceArray(ctx, d_sig, (n, K), dtype=np.uint32)
                except BaseException:
                    ctx.free(d_sig)
                    raise
                ctx.minhash_rows_device(d_ids, d_ro, n, 1, 1, w, K, seed, d_sig, 0)
                ctx.sync()                                             # (what the encode call deferred is reported here)
                return sig

    def minhash_groups(self, signatures, bands=16, threshold=0.7, min_agree=None):
        """Near-duplicate groups from MinHash signatures, on the GPU: `signatures` is a numpy uint32 [N, K] array or a
        `handoff.DeviceArray` of this object (`encode_minhash_to_device`); signatures made in many batches are concatenated and
        grouped once.  The K slots are cut into `bands` bands; in every band a row is compared with the SMALLEST row that has the
        same band (and with no other: two rows that share a band only with a smaller third that resembles neither are not joined
        through it), and the two are joined when they agree in at least `min_agree` slots, default max(1, ceil(threshold * K)).
        A row whose slots are all 0xFFFFFFFF (an empty document) stays alone.  Returns group int32 [N] (the smallest row of the
        row's group), keep bool [N] (group == arange(N): the rows to keep) and n_groups."""
        from .handoff import DeviceArray
        on_device = isinstance(signatures, DeviceArray)
        sig = signatures if on_device else np.asarray(signatures)
        if sig.dtype != np.uint32:
            raise TypeError("minhash_groups() expects uint32 signatures")
        if len(sig.shape) != 2 or not 1 <= sig.shape[1] <= 256:
            raise ValueError("minhash_groups() expects signatures [N, K] with 1 <= K <= 256")
        N, K = sig.shape
        if N >= 2 ** 31 - 4096:
            raise ValueError("minhash_groups() takes fewer than 2**31 - 4096 rows")
        _, _, _, B, m = self._minhash_rule(K, 5, 0, bands, threshold, min_agree)
        if on_device and sig._ctx is not self._ctx:
            raise ValueError("the signatures belong to another Tokenize object's device context")
        ctx = self._ctx
        if not on_device:
            group, total = ctx.minhash_groups(sig, B, m)
        else:
            group = np.zeros(N, dtype=np.int32)
            d_group = ctx.alloc(4 * max(N, 1))
            try:
                total = ctx.minhash_groups_device(sig.ptr if N else 0, N, K, B, m, d_group if N else 0)
                if N:
                    ctx.d2h(group, d_group)
            finally:
                ctx.free(d_group)
        return dict(group=group, keep=group == np.arange(N, dtype=np.int32), n_groups=int(total))

    def near_duplicates(self, texts: Sequence[str], num_perm=128, shingle=5, seed=0, bands=16, threshold=0.7, min_agree=None,
                        word_table=True):
        """`encode_minhash_to_device` and `minhash_groups` together: the signatures never leave HBM.  Returns the dict of
        `minhash_groups`; `texts[i]` for the i with keep[i] is the corpus without its near-duplicates."""
        self._minhash_rule(num_perm, shingle, seed, bands, threshold, min_agree)
        sig = self._encode_minhash(texts, num_perm, shingle, seed, word_table)
        return self.minhash_groups(sig, bands, threshold, min_agree)

    # ---- exact token n-gram overlap against a held-out set ("decontamination") ---------------------------------------------
    @staticmethod
    def _ngram_rule(n=13):
        """The width of the n-gram calls as an integer, or the refusal."""
        return _integer("n", n, 1, 33)

    @staticmethod
    def _ngram_rows(name, rows):
        """`rows` as (flat int32, int64 offsets), or the refusal: ids that are not integers (a float is not cut to one here), or
        that do not fit int32"""
        if not (isinstance(rows, np.ndarray) and rows.ndim == 2):
            rows = [np.asarray(r) for r in rows]
            for r in rows:
                if r.size and r.dtype.kind not in "iu":
                    raise TypeError("%s() expects integer ids" % name)
        flat, off = Tokenize._flat_rows(rows)
        return _int32_ids(name, flat), off

    def _ngram_index_of(self, index):
        """The live handle of `index`, or the refusal: not an NgramIndex, closed, or of another Tokenize object."""
        if not isinstance(index, NgramIndex):
            raise TypeError("index must be an NgramIndex (Tokenize.ngram_index, Tokenize.encode_ngram_index)")
        if index.closed:
            raise ValueError("the NgramIndex is closed")
        if index._ctx is not self._ctx:
            raise ValueError("the NgramIndex belongs to another Tokenize object's device context")
        return index._handle

    def ngram_index(self, rows, n=13, framed=True):
        """An `NgramIndex` of the token n-grams of held-out `rows` (benchmark questions, test splits, canaries), built on the GPU and
        resident in HBM.  `rows` as `decode_batch` / `window_rows` take them (`framed=True`: each row loses its first and last
        entry first).  The n-grams of a body are its runs of `n` ids, 1 <= n <= 32; a body shorter than `n` has none.  The index
        owns a copy of the ids.  To find out which benchmark items leaked rather than which documents, swap the roles: index a
        corpus shard and query the benchmark."""
        n = self._ngram_rule(n)
        flat, off = self._ngram_rows("ngram_index", rows)
        return NgramIndex(self._ctx, self._ctx.ngram_index_build(flat, off, n, bool(framed)))

    def encode_ngram_index(self, texts: Sequence[str], n=13, word_table=True):
        """`ngram_index` over the whole token sequence of every text: the texts are encoded without a length limit on the device
        and the index is built there, over the rows of `encode_batch(texts, max_len=None)` without their frame.  Single texts
        only.  Swap the roles -- index a corpus shard, query the benchmark -- to learn which benchmark items leaked."""
        n = self._ngram_rule(n)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        self._sync_tables()
        ctx = self._ctx
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            with self._encode_ragged_to_device(texts, word_table) as (d_ids, d_ro, R, dev):
                handle = ctx.ngram_index_build_device(d_ids, d_ro, R, 1, 1, n)
                ctx.sync()                                             # (what the encode call deferred is reported here)
        return NgramIndex(ctx, handle)

    def ngram_overlap_rows(self, rows, index, framed=True, return_covered=False):
        """Exact n-gram overlap of token `rows` with the held-out set of `index`, on the GPU.  Per row, with body q of m ids and
        n = index.n: n_grams = max(0, m - n + 1); n_hits = the positions i whose n-gram q[i:i+n] is in the index; n_covered = the
        body tokens that lie inside some such n-gram; first_hit = the smallest such i (-1: none); first_ref = the smallest
        reference row that holds that n-gram (-1: none); body_len = m.  Everything is exact -- a hash decides where to look, never
        whether two n-grams are equal.  A row's outputs depend on its own body and the index alone:
        `ngram_overlap_rows(rows[a:b])` is `ngram_overlap_rows(rows)[a:b]`, and results of shards concatenate.
        Returns a dict of numpy int32 [N] arrays; with `return_covered` also `covered`, uint8 over the rows back to back (1 on
        covered body tokens, 0 elsewhere, the frame cells included) and `row_off` int64 [N+1]."""
        handle = self._ngram_index_of(index)
        flat, off = self._ngram_rows("ngram_overlap_rows", rows)
        out = self._ctx.ngram_overlap(handle, flat, off, bool(framed), bool(return_covered))
        skip = 2 if framed else 0
        out["body_len"] = np.maximum(np.diff(off) - skip, 0).astype(np.int32)
        if return_covered:
            out["row_off"] = off
        return out

    def encode_ngram_overlap(self, texts: Sequence[str], index, word_table=True):
        """`ngram_overlap_rows` over the whole token sequence of every text: the texts are encoded without a length limit on the
        device, queried there, and only the per-document arrays come back -- n_grams, n_hits, n_covered, first_hit, first_ref
        and body_len, int32 [N].  The rule is `ngram_overlap_rows`'s over the rows of `encode_batch(texts, max_len=None)`
        without their frame; `encode_ngram_overlap(texts[a:b])` is `encode_ngram_overlap(texts)[a:b]`, and results of
        shards concatenate.  Single texts only."""
        handle = self._ngram_index_of(index)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        self._sync_tables()
        ctx = self._ctx
        names = _native.Context.NGRAM_OUT
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            with self._encode_ragged_to_device(texts, word_table) as (d_ids, d_ro, N, dev):
                d_out = dev(4 * len(names) * max(N, 1))
                ctx.ngram_overlap_device(handle, d_ids, d_ro, N, 1, 1, *[d_out + 4 * N * k if N else 0 for k in range(len(names))], 0)
                ctx.sync()                                             # (what the encode call deferred is reported here)
                host = np.empty((len(names), N), dtype=np.int32)
                row_off = np.zeros(N + 1, dtype=np.int64)
                if N:
                    ctx.d2h(host, d_out)
                ctx.d2h(row_off, d_ro)
        out = {k: host[i] for i, k in enumerate(names)}
        out["body_len"] = np.maximum(np.diff(row_off) - 2, 0).astype(np.int32)
        return out

    def decontaminate(self, texts: Sequence[str], index, max_fraction=0.0):
        """`encode_ngram_overlap` plus the decision every recipe takes from it: fraction = n_covered / max(body_len, 1) (float64,
        the share of a document's tokens inside n-grams of the held-out set) and keep = n_covered <= max_fraction * body_len
        (bool [N]); `max_fraction` is a number in [0, 1], and 0 keeps exactly the documents without a hit.  `texts[i]` for the i
        with keep[i] is the corpus without its contaminated documents.  To learn which benchmark items leaked, swap the roles:
        index a corpus shard and query the benchmark."""
        f = _share("max_fraction", max_fraction)
        out = self.encode_ngram_overlap(texts, index)
        covered, body = out["n_covered"].astype(np.float64), out["body_len"].astype(np.float64)
        out["fraction"] = covered / np.maximum(body, 1.0)
        out["keep"] = covered <= f * body
        return out

    # ---- n-gram repetition inside a document ("quality filtering") -----------------------------------------------------------
    REPEAT_WIDTHS = (2, 3, 4, 5, 6, 7, 8, 9, 10)
    REPEAT_TOP_MAX = {2: 0.20, 3: 0.18, 4: 0.16}
    REPEAT_DUP_MAX = {5: 0.15, 6: 0.14, 7: 0.13, 8: 0.12, 9: 0.11, 10: 0.10}

    @staticmethod
    def _repeat_rule(widths=REPEAT_WIDTHS):
        """The widths of the repetition calls as a tuple of ints, or the refusal: 1..16 distinct integers, each in 1..32."""
        if isinstance(widths, (str, bytes)) or not hasattr(widths, "__iter__"):
            raise TypeError("widths must be a sequence of ints")
        w = tuple(_integer("a width", v, 1, 33) for v in widths)
        if not 1 <= len(w) <= 16:
            raise ValueError("widths must hold 1 to 16 entries")
        if len(set(w)) != len(w):
            raise ValueError("widths must be distinct")
        return w

    @staticmethod
    def _repeat_bounds(name, bounds):
        """{width: largest share kept} of `repetition_filter` as {int: float}, or the refusal"""
        if not isinstance(bounds, dict):
            raise TypeError("%s must be a dict {n: share}" % name)
        return {_integer("a width of %s" % name, n, 1, 33): _share("a share of %s" % name, v) for n, v in bounds.items()}

    @staticmethod
    def _repeat_decide(out, top_max, dup_max):
        """The shares and the decision of `repetition_filter` from the counts of `encode_repetition`, added to `out`."""
        at = {n: k for k, n in enumerate(out["widths"])}
        body = np.maximum(out["body_len"].astype(np.float64), 1.0)
        out["top_fraction"] = {n: n * out["top_count"][at[n]].astype(np.float64) / body for n in top_max}
        out["dup_fraction"] = {n: out["n_covered"][at[n]].astype(np.float64) / body for n in dup_max}
        keep = np.ones(len(body), dtype=bool)
        for n, bound in top_max.items():
            keep &= out["top_fraction"][n] <= bound
        for n, bound in dup_max.items():
            keep &= out["dup_fraction"][n] <= bound
        out["keep"] = keep
        return out

    def repetition_rows(self, rows, widths=REPEAT_WIDTHS, framed=True, return_covered=False):
        """How much token `rows` repeat THEMSELVES, on the GPU: the counts behind the repetition rule of Gopher (Rae et al., 2021,
        table A1).  `rows` as `ngram_overlap_rows` takes them (`framed=True`: each row loses its first and last entry first);
        `widths`: 1..16 distinct ints in 1..32, in any order.  Per row with body q of m ids and per width n = widths[k], with c(g)
        the number of positions whose n-gram is g (occurrences may overlap) and first(g) the smallest of them:
        n_grams = G = max(0, m - n + 1); n_distinct = the different n-grams (G - n_distinct: the later occurrences);
        n_repeated = the positions i with c(q[i:i+n]) >= 2, the first occurrence too; n_covered = the body tokens inside some
        repeated n-gram, each once; top_count = max c(g) (0: no n-gram); top_pos = first(g) of the most frequent n-gram, among
        equal counts the smallest (-1: no n-gram).  Everything is exact -- a hash decides where to look, never whether two
        n-grams are equal, nor whether they stand in the same row.  A row's outputs depend on its own body and the widths alone,
        never on another row: `repetition_rows(rows[a:b])` is `repetition_rows(rows)[:, a:b]`, and results of shards concatenate.
        Rows of any integer ids are legal: the word-id sequences of `BM25(..., positions=True).term_sequences()` give Gopher's
        word n-grams.
        Returns a dict of numpy int32 [K, N] arrays plus body_len int32 [N] and `widths` (the tuple); with `return_covered` also
        `covered`, uint16 over the rows back to back (bit k: the token is covered at widths[k]; 0 on the frame cells) and
        `row_off` int64 [N+1]."""
        w = self._repeat_rule(widths)
        flat, off = self._ngram_rows("repetition_rows", rows)
        out = self._ctx.ngram_repeats(flat, off, w, bool(framed), bool(return_covered))
        skip = 2 if framed else 0
        out["body_len"] = np.maximum(np.diff(off) - skip, 0).astype(np.int32)
        out["widths"] = w
        if return_covered:
            out["row_off"] = off
        return out

    def encode_repetition(self, texts: Sequence[str], widths=REPEAT_WIDTHS, word_table=True):
        """`repetition_rows` over the whole token sequence of every text: the texts are encoded without a length limit on the
        device, counted there, and only the per-document arrays come back -- n_grams, n_distinct, n_repeated, n_covered,
        top_count and top_pos, int32 [K, N], body_len int32 [N] and `widths`.  The rule is `repetition_rows`'s over the rows of
        `encode_batch(texts, max_len=None)` without their frame; `encode_repetition(texts[a:b])` is
        `encode_repetition(texts)[:, a:b]`, and results of shards concatenate.  Single texts only."""
        w = self._repeat_rule(widths)
        texts = list(texts)
        for t in texts:
            _require_str(t)
        self._sync_tables()
        ctx = self._ctx
        names = _native.Context.REPEAT_OUT
        K = len(w)
        with self._batch_lock:                                         # (the pinned text arena is one buffer per object: see pack_pinned)
            with self._encode_ragged_to_device(texts, word_table) as (d_ids, d_ro, N, dev):
                d_out = dev(4 * len(names) * K * max(N, 1))
                ctx.ngram_repeats_device(d_ids, d_ro, N, 1, 1, w, *[d_out + 4 * K * N * i if N else 0 for i in range(len(names))], 0)
                ctx.sync()                                             # (what the encode call deferred is reported here)
                host = np.empty((len(names), K, N), dtype=np.int32)
                row_off = np.zeros(N + 1, dtype=np.int64)
                if N:
                    ctx.d2h(host, d_out)
                ctx.d2h(row_off, d_ro)
        out = {k: host[i] for i, k in enumerate(names)}
        out["body_len"] = np.maximum(np.diff(row_off) - 2, 0).astype(np.int32)
        out["widths"] = w
        return out

    def repetition_filter(self, texts: Sequence[str], top_max=None, dup_max=None):
        """`encode_repetition` plus the decision of the Gopher repetition rule.  `top_max` {n: share} bounds the share of a
        document inside its most frequent n-gram, top_fraction[n] = n * top_count / max(body_len, 1); `dup_max` {n: share} bounds
        the share inside n-grams that occur more than once, dup_fraction[n] = n_covered / max(body_len, 1); both float64 [N] in
        dicts keyed by n.  keep (bool [N]): every fraction is at or under its bound; `texts[i]` for the i with keep[i] is the
        corpus without its repetitive documents.  The defaults, top_max = {2: 0.20, 3: 0.18, 4: 0.16} and dup_max = {5: 0.15,
        6: 0.14, 7: 0.13, 8: 0.12, 9: 0.11, 10: 0.10}, are Gopher's thresholds: they were stated for CHARACTER shares of WORD
        n-grams and are applied here to TOKEN shares of token n-grams, so a caller tunes them (a document of fewer than n / bound
        tokens passes a top bound only without an n-gram: filter very short documents by length).  The call runs
        `encode_repetition` over the union of the widths; an empty dict for either is legal, both empty is refused."""
        top = self._repeat_bounds("top_max", self.REPEAT_TOP_MAX if top_max is None else top_max)
        dup = self._repeat_bounds("dup_max", self.REPEAT_DUP_MAX if dup_max is None else dup_max)
        if not top and not dup:
            raise ValueError("repetition_filter() needs a bound in top_max or dup_max")
        out = self.encode_repetition(texts, self._repeat_rule(sorted(set(top) | set(dup))))
        return self._repeat_decide(out, top, dup)

    @staticmethod
    def _shape(r, n):
        if r["dense"]:
            L = r["max_len"]
            for k in ("input_ids", "attention_mask", "token_type_ids", "sequence_id"):
                if k in r:
                    r[k] = r[k].reshape(n, L)
        return r

    @classmethod
    def fromFile(cls, vocab_file, bpe_file):
        """tokenize.py:261-267.  (The reference loads the bundled tables first and then re-runs __init__;
        here the paths are set before the only load.)"""
        tok = cls.__new__(cls)
        tok.vocab_file = vocab_file
        tok.bpe_file = bpe_file
        tok.__init__()
        return tok


def get_pairs(word):
    """tokenize.py:270-278: the set of adjacent symbol pairs of a word (a tuple of symbols, or a str).  An empty word
    raises IndexError as the reference's `word[0]` does (:272)."""
    word[0]
    return {(a, b) for a, b in zip(word, word[1:])}
