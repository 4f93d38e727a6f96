"""ctypes binding of include/genz_tokenize.h (libgenz_tokenize_hip.so).

Thin by design: argument marshalling only.  There is no CPU fallback -- if the
shared library is missing or no gfx950 device is usable, constructing a context
raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (GZ_LIBRARY: another build of the same library -- the diagnostic build of `make diag` in the tests)
LIB_PATH = os.environ.get("GZ_LIBRARY") or os.path.join(_HERE, "libgenz_tokenize_hip.so")

GZ_OK, GZ_E_INVALID, GZ_E_UTF8, GZ_E_HIP, GZ_E_NOTABLES = 0, -1, -2, -3, -4
GZ_E_CAPACITY, GZ_E_LIMIT, GZ_E_NOMEM, GZ_E_RCCL, GZ_E_NODEVICE = -5, -6, -7, -8, -9
GZ_BM25_POSITIONS, GZ_BM25_PHRASE_MAX = 1, 64
GZ_BM25_NEAR_MAX = 64
GZ_BM25_EDIT_MAX = 64
GZ_BM25_GROUP_MAX = 64
GZ_PADDING, GZ_TRUNCATION, GZ_MAX_LEN_NONE, GZ_TIMING, GZ_NO_WORD_TABLE, GZ_KEEP_WORDS = 0x1, 0x2, 0x4, 0x100, 0x200, 0x400
GZ_NONE = -1
GZ_PP_HTML, GZ_PP_UNICODE, GZ_PP_PUNCT, GZ_PP_EMOJI, GZ_PP_URL = 1, 2, 3, 4, 5

# every symbol include/genz_tokenize.h declares (tests/test_abi.py checks the export list against the header)
SYMBOLS = [
    "gz_version", "gz_create", "gz_destroy", "gz_last_error", "gz_load_tables", "gz_table_info", "gz_table_cache_status", "gz_table_digest",
    "gz_vocab_entry", "gz_merge_entry", "gz_encode_batch", "gz_encode_batch_csr", "gz_host_alloc", "gz_host_free", "gz_encode_batch_device", "gz_encode_batch_device_h", "gz_sync",
    "gz_word_token_counts", "gz_bpe_word", "gz_symbol_utf8", "gz_device_alloc", "gz_device_free", "gz_memcpy_h2d", "gz_memcpy_d2h",
    "gz_timing", "gz_timing_history", "gz_decoder_snapshot", "gz_decode_batch", "gz_decode_batch_device", "gz_preprocess_batch",
    "gz_preprocess_batch_device", "gz_block_create", "gz_block_release", "gz_block_dlpack", "gz_dlpack_capsule_destructor", "gz_exchange_select", "gz_encode_emit_block", "gz_block_total", "gz_comm_unique_id", "gz_comm_init", "gz_gather_rows", "gz_exchange_timing_history", "gz_compact_rows", "gz_expand_rows", "gz_compact_rows16", "gz_expand_rows16", "gz_compact_block", "gz_expand_block",
    "gz_host_tables_create", "gz_host_tables_destroy", "gz_host_tables_array", "gz_host_tables_vocab_entry",
    "gz_host_tables_merge_entry", "gz_host_tables_symbol", "gz_limit", "gz_debug_set",
    "gz_bm25_build", "gz_bm25_build_device", "gz_bm25_info", "gz_bm25_field_lengths", "gz_bm25_lookup", "gz_bm25_score",
    "gz_bm25_score_device", "gz_bm25_destroy", "gz_bm25_topk", "gz_bm25_topk_device",
    "gz_bm25_append", "gz_bm25_append_device", "gz_bm25_remove", "gz_bm25_remove_device",
    "gz_bm25_compact", "gz_bm25_terms", "gz_bm25_footprint",
    "gz_bm25_search", "gz_bm25_search_device", "gz_bm25_match_count",
    "gz_bm25_search_bool", "gz_bm25_search_bool_device", "gz_bm25_match_count_bool",
    "gz_bm25_build_ex", "gz_bm25_build_device_ex", "gz_bm25_flags", "gz_bm25_sequence",
    "gz_bm25_search_phrase", "gz_bm25_search_phrase_device", "gz_bm25_match_count_phrase",
    "gz_bm25_snippets", "gz_bm25_snippets_device", "gz_bm25_occurrences",
    "gz_bm25_search_near", "gz_bm25_search_near_device", "gz_bm25_match_count_near", "gz_bm25_cover", "gz_bm25_cover_device",
    "gz_bm25_similar", "gz_bm25_prefix", "gz_bm25_term_bytes",
    "gz_bm25_search_groups", "gz_bm25_search_groups_device", "gz_bm25_match_count_groups",
    "gz_window_rows", "gz_window_rows_device",
    "gz_pack_rows", "gz_pack_rows_device",
    "gz_mask_rows", "gz_mask_rows_device",
    "gz_infill_rows", "gz_infill_rows_device",
    "gz_minhash_rows", "gz_minhash_rows_device", "gz_minhash_groups", "gz_minhash_groups_device",
    "gz_wordset_build", "gz_wordset_build_device", "gz_wordset_from_counts", "gz_wordset_info", "gz_wordset_words", "gz_wordset_destroy",
    "gz_bpe_learn", "gz_bpe_learn_result",
    "gz_encode_dropout", "gz_encode_dropout_device", "gz_bpe_word_dropout",
    "gz_ngram_index_build", "gz_ngram_index_build_device", "gz_ngram_index_info", "gz_ngram_index_destroy", "gz_ngram_overlap",
    "gz_ngram_overlap_device",
    "gz_word_spans", "gz_word_spans_device", "gz_align_rows", "gz_align_rows_device", "gz_span_labels", "gz_span_labels_device",
    "gz_ngram_repeats", "gz_ngram_repeats_device",
    "gz_pair_window_rows", "gz_pair_window_rows_device", "gz_span_tokens", "gz_span_tokens_device",
    "gz_pack_rows_fit", "gz_pack_rows_fit_device", "gz_pack_rows_fit_info",
]

_lib = None


class GzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("genz_tokenize (HIP): error %d: %s" % (code, msg))
        self.code = code


def load_library():
    """dlopen the C-ABI library and declare its prototypes.  Raises RuntimeError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "genz_tokenize: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C genz-tokenize_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_size_t
    P = C.POINTER
    L.gz_version.restype = C.c_int
    L.gz_create.argtypes = [C.c_int, P(vp)]
    L.gz_destroy.argtypes = [vp]; L.gz_destroy.restype = None
    L.gz_last_error.argtypes = [vp]; L.gz_last_error.restype = C.c_char_p
    L.gz_load_tables.argtypes = [vp, vp, sz, vp, sz, P(C.c_char_p)]
    L.gz_table_info.argtypes = [vp, P(i32), P(i32), P(i32), P(i32)]
    L.gz_table_cache_status.argtypes = [vp]
    L.gz_table_digest.argtypes = [vp, vp]
    L.gz_vocab_entry.argtypes = [vp, i64, P(vp), P(i32), P(i32)]
    L.gz_merge_entry.argtypes = [vp, i64, P(vp), P(i32), P(i32), P(i32)]
    enc = [vp, vp, vp, vp, vp, i64, i32, u32, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gz_encode_batch.argtypes = enc
    L.gz_encode_batch_device.argtypes = enc
    L.gz_encode_batch_device_h.argtypes = enc + [vp, vp]
    L.gz_encode_batch_csr.argtypes = [vp, vp, vp, i64, i32, u32, vp, i64, i32, vp, P(i64)]
    L.gz_host_alloc.argtypes = [vp, sz, P(vp)]
    L.gz_host_free.argtypes = [vp, vp]
    L.gz_sync.argtypes = [vp]
    L.gz_word_token_counts.argtypes = [vp, C.c_int, vp, i64, vp, P(i64)]
    L.gz_bpe_word.argtypes = [vp, vp, i64, vp, i64]; L.gz_bpe_word.restype = i64
    L.gz_symbol_utf8.argtypes = [vp, i32, P(vp), P(i32)]
    L.gz_device_alloc.argtypes = [vp, sz, P(vp)]
    L.gz_device_free.argtypes = [vp, vp]
    L.gz_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.gz_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.gz_timing.argtypes = [vp, P(C.c_double)]
    L.gz_timing_history.argtypes = [vp, P(C.c_double), i32, P(i32)]
    L.gz_decoder_snapshot.argtypes = [vp]
    L.gz_decode_batch.argtypes = [vp, vp, vp, i64, vp, i32, vp, i64, vp]
    L.gz_decode_batch_device.argtypes = [vp, vp, vp, i64, vp, i32, vp, i64, vp, P(i64)]
    win = [vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, P(i64)]
    L.gz_window_rows.argtypes = win
    L.gz_window_rows_device.argtypes = win
    pk = [vp, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, P(i64)]
    L.gz_pack_rows.argtypes = pk
    L.gz_pack_rows_device.argtypes = pk
    if hasattr(L, "gz_pack_rows_fit"):
        pf = pk[:14] + [vp] + pk[14:]                                  # ... plus row_docs in front of pack_off
        L.gz_pack_rows_fit.argtypes = pf
        L.gz_pack_rows_fit_device.argtypes = pf
        L.gz_pack_rows_fit_info.argtypes = [vp, P(C.c_double), P(i64), P(i64)]
    if hasattr(L, "gz_mask_rows"):
        u64 = C.c_uint64
        mk = [vp, vp, i64, i32, i64, u64, u64, u64, u64, i32, i32, i32, i32, i32, vp, vp, vp]
        L.gz_mask_rows.argtypes = mk
        L.gz_mask_rows_device.argtypes = mk
    if hasattr(L, "gz_infill_rows"):
        u64 = C.c_uint64
        fi = [vp, vp, i64, i32, i64, u64, u64, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.gz_infill_rows.argtypes = fi
        L.gz_infill_rows_device.argtypes = fi
    if hasattr(L, "gz_minhash_rows"):
        u64 = C.c_uint64
        mh = [vp, vp, vp, i64, i32, i32, i32, i32, u64, vp, vp]
        L.gz_minhash_rows.argtypes = mh
        L.gz_minhash_rows_device.argtypes = mh
        mg = [vp, vp, i64, i32, i32, i32, vp, P(i64)]
        L.gz_minhash_groups.argtypes = mg
        L.gz_minhash_groups_device.argtypes = mg
    if hasattr(L, "gz_wordset_build"):
        L.gz_wordset_build.argtypes = [vp, vp, vp, i64, P(vp)]
        L.gz_wordset_build_device.argtypes = [vp, vp, vp, i64, i64, P(vp)]
        L.gz_wordset_from_counts.argtypes = [vp, vp, vp, vp, i64, P(vp)]
        L.gz_wordset_info.argtypes = [vp, P(i64), P(i64), P(i64)]
        L.gz_wordset_words.argtypes = [vp, vp, vp, vp, i64]
        L.gz_wordset_destroy.argtypes = [vp]; L.gz_wordset_destroy.restype = None
        L.gz_bpe_learn.argtypes = [vp, i64, i64, vp]
        L.gz_bpe_learn_result.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64]
    L.gz_preprocess_batch.argtypes = [vp, vp, i32, vp, vp, i64, vp, i64, vp]
    L.gz_preprocess_batch_device.argtypes = [vp, vp, i32, vp, vp, i64, i64, vp, i64, vp, P(i64)]
    L.gz_block_create.argtypes = [vp, vp, P(vp)]
    L.gz_block_release.argtypes = [vp]; L.gz_block_release.restype = None
    L.gz_block_dlpack.argtypes = [vp, i32, vp, i32, i32]; L.gz_block_dlpack.restype = vp
    L.gz_dlpack_capsule_destructor.argtypes = [vp]; L.gz_dlpack_capsule_destructor.restype = None
    L.gz_exchange_select.argtypes = [vp, C.c_int]
    L.gz_encode_emit_block.argtypes = [vp, vp, i32]
    L.gz_block_total.argtypes = [vp, i32, P(i64)]
    L.gz_comm_unique_id.argtypes = [vp]
    L.gz_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    L.gz_gather_rows.argtypes = [vp, vp, i64, i32, vp, vp, C.c_int]
    if hasattr(L, "gz_exchange_timing_history"):
        L.gz_exchange_timing_history.argtypes = [vp, P(C.c_double), i32, P(i32)]
    L.gz_compact_rows.argtypes = [vp, vp, vp, i64, i32, vp, P(i64)]
    L.gz_expand_rows.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.gz_compact_rows16.argtypes = [vp, vp, vp, i64, i32, vp, P(i64)]
    L.gz_expand_rows16.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.gz_compact_block.argtypes = [vp, vp, vp, i64, i32, i32, vp, P(i64)]
    L.gz_expand_block.argtypes = [vp, vp, i32, i64, i32, i64, vp, vp]
    L.gz_host_tables_create.argtypes = [vp, sz, vp, sz, P(C.c_char_p), P(vp)]
    L.gz_host_tables_destroy.argtypes = [vp]; L.gz_host_tables_destroy.restype = None
    L.gz_host_tables_array.argtypes = [vp, C.c_int, P(vp), P(i64)]
    L.gz_host_tables_vocab_entry.argtypes = [vp, i64, P(vp), P(i32), P(i32)]
    L.gz_host_tables_merge_entry.argtypes = [vp, i64, P(vp), P(i32), P(i32), P(i32)]
    L.gz_host_tables_symbol.argtypes = [vp, i32, P(vp), P(i32)]
    if hasattr(L, "gz_bm25_build"):
        L.gz_bm25_build.argtypes = [vp, vp, vp, i64, P(vp)]
        L.gz_bm25_build_device.argtypes = [vp, vp, vp, i64, i64, P(vp)]
        L.gz_bm25_info.argtypes = [vp, P(i64), P(i64), P(i64)]
        L.gz_bm25_field_lengths.argtypes = [vp, vp]
        L.gz_bm25_lookup.argtypes = [vp, vp, vp, i64, vp, vp]
        L.gz_bm25_score.argtypes = [vp, vp, vp, vp, i64, vp, i32, vp]
        L.gz_bm25_score_device.argtypes = [vp, vp, vp, vp, i64, vp, i32, vp]
        L.gz_bm25_destroy.argtypes = [vp]; L.gz_bm25_destroy.restype = None
    if hasattr(L, "gz_bm25_topk"):
        L.gz_bm25_topk.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, vp, vp]
        L.gz_bm25_topk_device.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, vp, vp]
    if hasattr(L, "gz_bm25_append"):
        L.gz_bm25_append.argtypes = [vp, vp, vp, i64]
        L.gz_bm25_append_device.argtypes = [vp, vp, vp, i64, i64]
    if hasattr(L, "gz_bm25_remove"):
        L.gz_bm25_remove.argtypes = [vp, vp, i64]
        L.gz_bm25_remove_device.argtypes = [vp, vp, i64]
    if hasattr(L, "gz_bm25_compact"):
        L.gz_bm25_compact.argtypes = [vp]
        L.gz_bm25_terms.argtypes = [vp, vp, vp, vp, i64]
        L.gz_bm25_footprint.argtypes = [vp, vp]
    if hasattr(L, "gz_bm25_search"):
        L.gz_bm25_search.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, vp, vp, vp]
        L.gz_bm25_search_device.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, vp, vp, vp]
        L.gz_bm25_match_count.argtypes = [vp, vp, vp, i64, vp]
    if hasattr(L, "gz_bm25_search_bool"):
        L.gz_bm25_search_bool.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp]
        L.gz_bm25_search_bool_device.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp]
        L.gz_bm25_match_count_bool.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp]
    if hasattr(L, "gz_bm25_search_phrase"):
        L.gz_bm25_build_ex.argtypes = [vp, vp, vp, i64, i32, P(vp)]
        L.gz_bm25_build_device_ex.argtypes = [vp, vp, vp, i64, i64, i32, P(vp)]
        L.gz_bm25_flags.argtypes = [vp, P(i32)]
        L.gz_bm25_sequence.argtypes = [vp, vp, vp]
        L.gz_bm25_search_phrase.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp]
        L.gz_bm25_search_phrase_device.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp]
        L.gz_bm25_match_count_phrase.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp]
    if hasattr(L, "gz_bm25_snippets"):
        L.gz_bm25_snippets.argtypes = [vp, vp, vp, i64, vp, i64, i64, vp, vp]
        L.gz_bm25_snippets_device.argtypes = [vp, vp, vp, i64, vp, i64, i64, vp, vp]
        L.gz_bm25_occurrences.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, i64]
    if hasattr(L, "gz_bm25_search_near"):
        L.gz_bm25_search_near.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.gz_bm25_search_near_device.argtypes = [vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.gz_bm25_match_count_near.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.gz_bm25_cover.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp]
        L.gz_bm25_cover_device.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp]
    if hasattr(L, "gz_bm25_similar"):
        L.gz_bm25_similar.argtypes = [vp, vp, vp, i64, i32, i64, vp, vp, vp, vp]
        L.gz_bm25_prefix.argtypes = [vp, vp, vp, i64, i64, vp, vp, vp]
        L.gz_bm25_term_bytes.argtypes = [vp, vp, i64, vp, vp, i64]
    if hasattr(L, "gz_bm25_search_groups"):
        L.gz_bm25_search_groups.argtypes = [vp, vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp]
        L.gz_bm25_search_groups_device.argtypes = [vp, vp, vp, vp, vp, i64, vp, i32, i64, i32, vp, vp, vp, vp, vp]
        L.gz_bm25_match_count_groups.argtypes = [vp, vp, vp, vp, i64, i32, vp, vp, vp]
    if hasattr(L, "gz_encode_dropout"):
        u64 = C.c_uint64
        dr = [vp, vp, vp, i64, i32, u32, i64, u64, u64, i64, vp, vp, vp, vp]
        L.gz_encode_dropout.argtypes = dr
        L.gz_encode_dropout_device.argtypes = dr
        L.gz_bpe_word_dropout.argtypes = [vp, vp, i64, u64, u64, i64, i64, vp, i64]; L.gz_bpe_word_dropout.restype = i64
    if hasattr(L, "gz_ngram_index_build"):
        nb = [vp, vp, vp, i64, i32, i32, i32, P(vp)]
        L.gz_ngram_index_build.argtypes = nb
        L.gz_ngram_index_build_device.argtypes = nb
        L.gz_ngram_index_info.argtypes = [vp, vp]
        L.gz_ngram_index_destroy.argtypes = [vp]; L.gz_ngram_index_destroy.restype = None
        no = [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp]
        L.gz_ngram_overlap.argtypes = no
        L.gz_ngram_overlap_device.argtypes = no
    if hasattr(L, "gz_word_spans"):
        L.gz_word_spans.argtypes = [vp, vp, vp, i64, i32, vp, vp, i64, P(i64)]
        L.gz_word_spans_device.argtypes = [vp, vp, vp, i64, i64, i32, vp, vp, i64, P(i64)]
        L.gz_align_rows.argtypes = [vp, vp, vp, i64, vp, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp, vp]
        L.gz_align_rows_device.argtypes = [vp, vp, vp, i64, i64, vp, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp, vp]
        L.gz_span_labels.argtypes = [vp, vp, vp, i64, vp, vp, i32, i32, vp, vp]
        L.gz_span_labels_device.argtypes = [vp, vp, vp, i64, i64, vp, vp, i64, i32, i32, vp, vp]
    if hasattr(L, "gz_ngram_repeats"):
        nr = [vp, vp, vp, i64, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.gz_ngram_repeats.argtypes = nr
        L.gz_ngram_repeats_device.argtypes = nr
    if hasattr(L, "gz_pair_window_rows"):
        pw = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, P(i64)]
        L.gz_pair_window_rows.argtypes = pw
        L.gz_pair_window_rows_device.argtypes = pw
        L.gz_span_tokens.argtypes = [vp, vp, vp, i64, vp, vp, vp]
        L.gz_span_tokens_device.argtypes = [vp, vp, vp, i64, i64, vp, vp, i64, vp]
    for name in SYMBOLS:
        if os.environ.get("GZ_LIBRARY") and not hasattr(L, name):
            continue                                     # (an older build loaded for an A/B run: entry points it lacks stay unbound)
        fn = getattr(L, name)
        if name not in ("gz_destroy", "gz_last_error", "gz_bpe_word", "gz_bpe_word_dropout", "gz_host_tables_destroy", "gz_block_release", "gz_block_dlpack",
                        "gz_dlpack_capsule_destructor", "gz_limit", "gz_bm25_destroy", "gz_wordset_destroy", "gz_ngram_index_destroy"):
            fn.restype = C.c_int
    if hasattr(L, "gz_limit"):
        L.gz_limit.argtypes = [C.c_int]
        L.gz_limit.restype = i64
    if hasattr(L, "gz_debug_set"):
        L.gz_debug_set.argtypes = [vp, C.c_char_p, i64]
    _lib = L
    return L


def debug_set(key: str, value: int, ctx: "Context | None" = None):
    """gz_debug_set: a test / experiment switch of the library -- of one context, or (ctx None) the process-wide defaults that
    contexts created afterwards copy and the table builder reads.  Raises ValueError for an unknown key or a bad value."""
    lib = load_library()
    rc = lib.gz_debug_set(ctx.handle if ctx is not None else None, key.encode("ascii"), int(value))
    if rc != GZ_OK:
        raise ValueError("gz_debug_set(%r, %r): unknown key or value out of range" % (key, value))


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _dptrs(*ds):
    """optional device addresses (0 or None: NULL), as one call passes them on: f(..., *_dptrs(d_a, d_b), ...)"""
    return [C.c_void_p(d) if d else None for d in ds]


def default_device() -> int:
    for k in ("GENZ_TOKENIZE_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(k)
        if v is not None and v.strip() != "":
            return int(v)
    return 0


class Context:
    """One gz_ctx: one GPU, one set of tables."""

    def __init__(self, device: int | None = None):
        self.lib = load_library()
        self.handle = C.c_void_p()
        self.device = default_device() if device is None else int(device)
        rc = self.lib.gz_create(self.device, C.byref(self.handle))
        if rc != GZ_OK:
            msg = self.lib.gz_last_error(None).decode("utf-8", "replace")
            self.handle = C.c_void_p()
            raise RuntimeError("genz_tokenize: cannot create a HIP context on device %d (%d: %s). "
                               "This build has no CPU fallback." % (self.device, rc, msg))

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.gz_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _check(self, rc):
        if rc < 0:
            raise GzError(rc, self.lib.gz_last_error(self.handle).decode("utf-8", "replace"))
        return rc

    def _call_total(self, fn, *args) -> int:
        """fn(*args, &total) -> total; a GzError of the call carries `.total` (GZ_E_CAPACITY: what the batch needs)."""
        total = C.c_int64()
        rc = fn(*args, C.byref(total))
        if rc:
            e = GzError(rc, self.lib.gz_last_error(self.handle).decode("utf-8", "replace"))
            e.total = total.value
            raise e
        return total.value

    # ---- tables ------------------------------------------------------------------------------------------
    def load_tables(self, vocab: bytes, bpe: bytes, specials):
        arr = (C.c_char_p * 5)(*[s.encode("utf-8", "surrogatepass") for s in specials])
        vb = C.create_string_buffer(vocab, len(vocab)) if vocab else None
        bb = C.create_string_buffer(bpe, len(bpe)) if bpe else None
        self._check(self.lib.gz_load_tables(self.handle, C.cast(vb, C.c_void_p) if vb else None, len(vocab),
                                            C.cast(bb, C.c_void_p) if bb else None, len(bpe), arr))

    def table_cache_status(self) -> int:
        """What the last load_tables did with the table cache: 0 no cache, 1 hit, 2 miss (written), 3 a file was refused."""
        return int(self.lib.gz_table_cache_status(self.handle))

    def table_digest(self) -> bytes:
        """SHA-256 over the device-resident table images and the dictionaries (gz_table_digest)."""
        out = (C.c_uint8 * 32)()
        self._check(self.lib.gz_table_digest(self.handle, out))
        return bytes(out)

    def table_info(self):
        vs, nr, ns = C.c_int32(), C.c_int32(), C.c_int32()
        sp = (C.c_int32 * 5)()
        self._check(self.lib.gz_table_info(self.handle, C.byref(vs), sp, C.byref(nr), C.byref(ns)))
        return vs.value, list(sp), nr.value, ns.value

    def vocab_items(self):
        n = self.table_info()[0]
        p, ln, idv = C.c_void_p(), C.c_int32(), C.c_int32()
        out = []
        for i in range(n):
            self._check(self.lib.gz_vocab_entry(self.handle, i, C.byref(p), C.byref(ln), C.byref(idv)))
            out.append((C.string_at(p, ln.value).decode("utf-8"), idv.value))
        return out

    def merge_items(self):
        n = self.table_info()[2]
        p, ln, nf, rk = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        out = []
        for i in range(n):
            self._check(self.lib.gz_merge_entry(self.handle, i, C.byref(p), C.byref(ln), C.byref(nf), C.byref(rk)))
            s = C.string_at(p, ln.value).decode("utf-8")
            out.append((tuple(s.split("\n")) if nf.value else (), rk.value))
        return out

    def symbol(self, sym: int) -> str:
        p, ln = C.c_void_p(), C.c_int32()
        self._check(self.lib.gz_symbol_utf8(self.handle, sym, C.byref(p), C.byref(ln)))
        return C.string_at(p, ln.value).decode("utf-8")

    # ---- encode, host buffers ------------------------------------------------------------------------------
    def encode(self, text: np.ndarray, text_off: np.ndarray, pair, pair_off, max_len, padding, truncation,
               extra_flags: int = 0):
        """Returns dict(input_ids, attention_mask, [token_type_ids, sequence_id, pair_len, status], row_off,
        n_real, dense).  Flat int32 arrays + int64 row offsets."""
        n = len(text_off) - 1
        flags = (GZ_PADDING if padding else 0) | (GZ_TRUNCATION if truncation else 0) | extra_flags
        ml = 0
        if max_len is None:
            flags |= GZ_MAX_LEN_NONE
        else:
            ml = int(max_len)
            if not -2**31 <= ml < 2**31:
                raise OverflowError("max_len does not fit in int32")
        is_pair = pair_off is not None
        dense = bool(max_len is not None and padding and truncation and ml >= 1)
        tb = int(text_off[-1] - text_off[0]) if n else 0
        pb = int(pair_off[-1] - pair_off[0]) if (is_pair and n) else 0
        if dense:
            cap = n * ml
        else:
            cap = tb + pb + (4 if is_pair else 2) * n
            if max_len is not None and padding and ml > 0:
                cap += n * ml
        ids = np.empty(max(cap, 1), dtype=np.int32)
        mask = np.empty(max(cap, 1), dtype=np.int32)
        tt = np.empty(max(cap, 1), dtype=np.int32) if is_pair else None
        seq = np.empty(max(cap, 1), dtype=np.int32) if is_pair else None
        row_off = np.zeros(n + 1, dtype=np.int64)
        pair_len = np.zeros(2 * max(n, 1), dtype=np.int32) if is_pair else None
        n_real = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        if is_pair:
            pair = np.ascontiguousarray(pair, dtype=np.uint8)
            pair_off = np.ascontiguousarray(pair_off, dtype=np.int64)
        self._check(self.lib.gz_encode_batch(
            self.handle, _ptr(text), _ptr(text_off), _ptr(pair) if is_pair else None,
            _ptr(pair_off) if is_pair else None, n, ml, flags, cap, _ptr(ids), _ptr(mask), _ptr(tt), _ptr(seq),
            _ptr(row_off), _ptr(pair_len), _ptr(n_real), _ptr(status)))
        total = int(row_off[-1]) if n else 0
        out = dict(input_ids=ids[:total], attention_mask=mask[:total], row_off=row_off, n_real=n_real[:n],
                   status=status[:n], dense=dense, max_len=ml)
        if is_pair:
            out.update(token_type_ids=tt[:total], sequence_id=seq[:total], pair_len=pair_len[:2 * n].reshape(n, 2))
        return out

    # ---- host buffers in, CSR out, copies overlapped with the kernels ---------------------------------------------------
    def pinned_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        """A numpy array in page-locked host memory (gz_host_alloc): H2D / D2H copies of it are real DMA.  The memory is
        returned when the array (and every view of it) is gone."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64))
        p = C.c_void_p()
        self._check(self.lib.gz_host_alloc(self.handle, max(n * dtype.itemsize, 1), C.byref(p)))
        buf = (C.c_char * max(n * dtype.itemsize, 1)).from_address(p.value)
        lib, addr = self.lib, p.value
        import weakref
        arr = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)
        # (gz_host_free does not look at the context: the array may well outlive it -- close(), interpreter exit)
        weakref.finalize(buf, lambda: lib.gz_host_free(None, C.c_void_p(addr)))
        return arr

    def encode_csr(self, text: np.ndarray, text_off: np.ndarray, max_len: int, bits: int = 16, extra_flags: int = 0,
                   tokens: np.ndarray | None = None, n_real: np.ndarray | None = None):
        """gz_encode_batch_csr: (tokens[total] uint16|int32, n_real[N] int32).  `tokens` / `n_real` may be supplied
        (e.g. pinned); tokens must hold min(N * max_len, bytes + 2 N) entries to be safe."""
        n = len(text_off) - 1
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        tb = int(text_off[-1] - text_off[0]) if n else 0
        cap = min(n * int(max_len), tb + 2 * n)
        dt = np.uint16 if bits == 16 else np.int32
        if tokens is None:
            tokens = np.empty(max(cap, 1), dtype=dt)
        if n_real is None:
            n_real = np.empty(max(n, 1), dtype=np.int32)
        assert tokens.dtype == dt and n_real.dtype == np.int32 and tokens.flags["C_CONTIGUOUS"] and n_real.flags["C_CONTIGUOUS"]
        total = C.c_int64()
        self._check(self.lib.gz_encode_batch_csr(self.handle, _ptr(text), _ptr(text_off), n, int(max_len),
                                                 GZ_PADDING | GZ_TRUNCATION | extra_flags, _ptr(tokens), tokens.size, bits,
                                                 _ptr(n_real), C.byref(total)))
        return tokens[:total.value], n_real[:n]

    def word_token_counts(self, which_text: int, n_docs: int, capacity: int):
        """(counts[int32, words], doc_first[int64, n_docs+1]) of the last encode call."""
        counts = np.empty(max(capacity, 1), dtype=np.int32)
        first = np.zeros(n_docs + 1, dtype=np.int64)
        nw = C.c_int64()
        rc = self.lib.gz_word_token_counts(self.handle, which_text, _ptr(counts), capacity, _ptr(first), C.byref(nw))
        if rc == GZ_E_CAPACITY and nw.value > capacity:         # the call says how many words there are: once more, exactly
            capacity = int(nw.value)
            counts = np.empty(capacity, dtype=np.int32)
            rc = self.lib.gz_word_token_counts(self.handle, which_text, _ptr(counts), capacity, _ptr(first), C.byref(nw))
        self._check(rc)
        return counts[:nw.value], first

    def bpe_word(self, word: bytes):
        cap = len(word) + 1
        out = np.empty(cap, dtype=np.int32)
        buf = np.frombuffer(word, dtype=np.uint8)
        n = self.lib.gz_bpe_word(self.handle, _ptr(buf), len(word), _ptr(out), cap)
        self._check(n)
        return out[:n]

    # ---- BPE-dropout ---------------------------------------------------------------------------------------------
    def encode_dropout(self, text: np.ndarray, text_off: np.ndarray, max_len, padding, truncation, thr: int, seed: int, doc_base: int):
        """gz_encode_dropout: the dict `encode` returns for single texts; thr = drop threshold (0 .. 2^32)."""
        n = len(text_off) - 1
        flags = (GZ_PADDING if padding else 0) | (GZ_TRUNCATION if truncation else 0)
        ml = 0
        if max_len is None:
            flags |= GZ_MAX_LEN_NONE
        else:
            ml = int(max_len)
            if not -2**31 <= ml < 2**31:
                raise OverflowError("max_len does not fit in int32")
        dense = bool(max_len is not None and padding and truncation and ml >= 1)
        tb = int(text_off[-1] - text_off[0]) if n else 0
        if dense:
            cap = n * ml
        else:
            cap = tb + 2 * n
            if max_len is not None and padding and ml > 0:
                cap += n * ml
        ids = np.empty(max(cap, 1), dtype=np.int32)
        mask = np.empty(max(cap, 1), dtype=np.int32)
        row_off = np.zeros(n + 1, dtype=np.int64)
        n_real = np.zeros(max(n, 1), dtype=np.int32)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        self._check(self.lib.gz_encode_dropout(self.handle, _ptr(text), _ptr(text_off), n, ml, flags, cap, thr, seed, doc_base,
                                               _ptr(ids), _ptr(mask), _ptr(row_off), _ptr(n_real)))
        total = int(row_off[-1]) if n else 0
        return dict(input_ids=ids[:total], attention_mask=mask[:total], row_off=row_off, n_real=n_real[:n],
                    status=np.zeros(n, dtype=np.int32), dense=dense, max_len=ml)

    def encode_dropout_device(self, d_text, d_text_off, n_docs, max_len, flags, capacity, thr, seed, doc_base, d_ids, d_mask,
                              d_row_off=None, d_n_real=None):
        """gz_encode_dropout_device: every pointer a device address (0 / None: NULL)."""
        vp = C.c_void_p
        self._check(self.lib.gz_encode_dropout_device(self.handle, vp(d_text), vp(d_text_off), n_docs, max_len, flags, capacity, thr, seed, doc_base,
                                                      vp(d_ids), vp(d_mask), *_dptrs(d_row_off, d_n_real)))

    def bpe_word_dropout(self, word: bytes, thr: int, seed: int, doc: int, word_index: int):
        cap = len(word) + 1
        out = np.empty(cap, dtype=np.int32)
        buf = np.frombuffer(word, dtype=np.uint8)
        n = self.lib.gz_bpe_word_dropout(self.handle, _ptr(buf), len(word), thr, seed, doc, word_index, _ptr(out), cap)
        self._check(n)
        return out[:n]

    # ---- device-resident path (bench, multi-GPU) ---------------------------------------------------------------
    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self.lib.gz_device_alloc(self.handle, nbytes, C.byref(p)))
        return p.value

    def free(self, dptr: int):
        self._check(self.lib.gz_device_free(self.handle, C.c_void_p(dptr)))

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._check(self.lib.gz_memcpy_h2d(self.handle, C.c_void_p(dptr), _ptr(arr), arr.nbytes))

    def d2h(self, arr: np.ndarray, dptr: int):
        assert arr.flags["C_CONTIGUOUS"]
        self._check(self.lib.gz_memcpy_d2h(self.handle, _ptr(arr), C.c_void_p(dptr), arr.nbytes))

    def encode_device(self, d_text, d_text_off, d_pair, d_pair_off, n_docs, max_len, flags, capacity,
                      d_ids, d_mask, d_tt=None, d_seq=None, d_row_off=None, d_pair_len=None, d_n_real=None,
                      d_status=None, h_text_off=None, h_pair_off=None):
        """Enqueue one call on device-resident buffers.  h_text_off / h_pair_off: optional host copies (int64 numpy) of
        the offsets; with them the library does not read the batch's byte sizes back from the device first."""
        vp = C.c_void_p
        args = [self.handle, vp(d_text), vp(d_text_off), *_dptrs(d_pair, d_pair_off), n_docs, max_len, flags, capacity, vp(d_ids), vp(d_mask),
                *_dptrs(d_tt, d_seq, d_row_off, d_pair_len, d_n_real, d_status)]
        if h_text_off is not None:
            self._check(self.lib.gz_encode_batch_device_h(*args, _ptr(h_text_off), _ptr(h_pair_off)))
        else:
            self._check(self.lib.gz_encode_batch_device(*args))

    def sync(self):
        self._check(self.lib.gz_sync(self.handle))

    def timing_history(self, max_calls: int = 64):
        """Synchronise; whole-pipeline kernel time (ms) of the last timed calls, oldest first."""
        buf = (C.c_double * max_calls)()
        n = C.c_int32()
        self._check(self.lib.gz_timing_history(self.handle, buf, max_calls, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    def exchange_timing_history(self, max_calls: int = 64):
        """Synchronise the exchange stream; start-possible -> done time (ms) of the last gz_gather_rows calls, oldest first."""
        buf = (C.c_double * max_calls)()
        n = C.c_int32()
        self._check(self.lib.gz_exchange_timing_history(self.handle, buf, max_calls, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    def timing(self):
        t = (C.c_double * 4)()
        self._check(self.lib.gz_timing(self.handle, t))
        return list(t)

    # ---- RCCL ---------------------------------------------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._check(self.lib.gz_comm_unique_id(C.cast(buf, C.c_void_p)))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int):
        buf = C.create_string_buffer(uid, 128)
        self._check(self.lib.gz_comm_init(self.handle, C.cast(buf, C.c_void_p), rank, world))

    # ---- batch decode -----------------------------------------------------------------------------------
    def decoder_snapshot(self):
        self._check(self.lib.gz_decoder_snapshot(self.handle))

    def decode(self, ids: np.ndarray, row_off: np.ndarray, unk: bytes):
        """ids int32 (packed rows), row_off int64 [n+1]  ->  (bytes of all rows, out_off int64 [n+1])."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        n = len(row_off) - 1
        out_off = np.zeros(n + 1, dtype=np.int64)
        ub = C.create_string_buffer(unk, len(unk))
        cap = max(64, 6 * len(ids))
        for _ in range(2):
            out = np.empty(cap, dtype=np.uint8)
            rc = self.lib.gz_decode_batch(self.handle, _ptr(ids) if len(ids) else None, _ptr(row_off), n,
                                          C.cast(ub, C.c_void_p), len(unk), _ptr(out), cap, _ptr(out_off))
            if rc != GZ_E_CAPACITY:
                break
            cap = int(out_off[n])
        self._check(rc)
        return out[:int(out_off[n])], out_off

    def decode_device(self, d_ids, d_row_off, n_rows, unk: bytes, d_out, capacity, d_out_off) -> int:
        total = C.c_int64()
        ub = C.create_string_buffer(unk, len(unk))
        self._check(self.lib.gz_decode_batch_device(self.handle, C.c_void_p(d_ids), C.c_void_p(d_row_off), n_rows,
                                                    C.cast(ub, C.c_void_p), len(unk), *_dptrs(d_out),
                                                    capacity, C.c_void_p(d_out_off), C.byref(total)))
        return total.value

    # ---- overlapping max_len windows -----------------------------------------------------------------------
    def window_rows(self, ids: np.ndarray, row_off: np.ndarray, max_len: int, stride: int, framed: bool):
        """ids int32 (packed rows), row_off int64 [n+1] -> dict(input_ids [W, L], attention_mask [W, L], doc [W], start [W],
        n_real [W], win_off int64 [n+1]) (gz_window_rows: a sizing call, then the windows)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        n, L, skip = len(row_off) - 1, int(max_len), 1 if framed else 0
        win_off = np.zeros(n + 1, dtype=np.int64)
        total = C.c_int64()
        head = (self.handle, _ptr(ids) if len(ids) else None, _ptr(row_off), n, L, int(stride), skip, skip)
        self._check(self.lib.gz_window_rows(*head, None, None, None, None, None, _ptr(win_off), 0, C.byref(total)))
        W = total.value
        out = dict(input_ids=np.empty((W, L), dtype=np.int32), attention_mask=np.empty((W, L), dtype=np.int32),
                   doc=np.empty(W, dtype=np.int32), start=np.empty(W, dtype=np.int32), n_real=np.empty(W, dtype=np.int32), win_off=win_off)
        if W:
            self._check(self.lib.gz_window_rows(*head, _ptr(out["input_ids"]), _ptr(out["attention_mask"]), _ptr(out["doc"]),
                                                _ptr(out["start"]), _ptr(out["n_real"]), _ptr(win_off), W, C.byref(total)))
        return out

    def window_rows_device(self, d_ids, d_row_off, n_rows, max_len, stride, skip_front, skip_back, d_input_ids, d_mask, d_doc, d_start,
                           d_n_real, d_win_off, capacity) -> int:
        """gz_window_rows_device: returns W.  d_input_ids == 0 sizes only; on GZ_E_CAPACITY the GzError carries `.total` = W."""
        return self._call_total(self.lib.gz_window_rows_device, self.handle, *_dptrs(d_ids), C.c_void_p(d_row_off), n_rows, max_len, stride,
                                skip_front, skip_back, *_dptrs(d_input_ids, d_mask, d_doc, d_start, d_n_real),
                                C.c_void_p(d_win_off), capacity)

    # ---- question-context windows with answer positions -----------------------------------------------------
    PAIRWIN_CELLS = ("input_ids", "attention_mask", "token_type_ids")
    PAIRWIN_META = ("pair", "start", "n_real", "q_len")
    PAIRWIN_ANSWER = ("start_positions", "end_positions", "has_answer")

    def pair_window_rows(self, q_ids, q_off, ids, row_off, max_len: int, stride: int, max_query_len: int, q_row, answers, framed: bool):
        """question rows and context rows (packed int32 + int64 offsets), q_row int32 [n] or None, answers int32 [n, 2] or None ->
        dict(input_ids, attention_mask, token_type_ids [W, L], pair, start, n_real, q_len [W], win_off int64 [n+1] and, with answers,
        start_positions, end_positions, has_answer [W]) (gz_pair_window_rows: a sizing call, then the windows)."""
        q_ids = np.ascontiguousarray(q_ids, dtype=np.int32)
        q_off = np.ascontiguousarray(q_off, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        q_row = None if q_row is None else np.ascontiguousarray(q_row, dtype=np.int32)
        answers = None if answers is None else np.ascontiguousarray(answers, dtype=np.int32)
        n, L, skip = len(row_off) - 1, int(max_len), 1 if framed else 0
        win_off = np.zeros(n + 1, dtype=np.int64)
        total = C.c_int64()
        head = (self.handle, _ptr(q_ids) if len(q_ids) else None, _ptr(q_off), len(q_off) - 1, _ptr(ids) if len(ids) else None, _ptr(row_off), n,
                _ptr(q_row), _ptr(answers), L, int(stride), int(max_query_len), skip, skip)
        self._check(self.lib.gz_pair_window_rows(*head, *([None] * 10), _ptr(win_off), 0, C.byref(total)))
        W = total.value
        out = {k: np.empty((W, L), dtype=np.int32) for k in self.PAIRWIN_CELLS}
        out.update({k: np.empty(W, dtype=np.int32) for k in self.PAIRWIN_META + (self.PAIRWIN_ANSWER if answers is not None else ())})
        out["win_off"] = win_off
        if W:
            self._check(self.lib.gz_pair_window_rows(*head, *[_ptr(out.get(k)) for k in self.PAIRWIN_CELLS + self.PAIRWIN_META + self.PAIRWIN_ANSWER],
                                                     _ptr(win_off), W, C.byref(total)))
        return out

    def pair_window_rows_device(self, d_q_ids, d_q_off, n_questions, d_ids, d_row_off, n_rows, d_q_row, d_answers, max_len, stride, max_query_len,
                                skip_front, skip_back, d_input_ids, d_mask, d_type, d_pair, d_start, d_n_real, d_q_len, d_start_pos, d_end_pos,
                                d_has_answer, d_win_off, capacity) -> int:
        """gz_pair_window_rows_device: returns W.  d_input_ids == 0 sizes only; on GZ_E_CAPACITY the GzError carries `.total` = W."""
        return self._call_total(self.lib.gz_pair_window_rows_device, self.handle, *_dptrs(d_q_ids, d_q_off), n_questions, *_dptrs(d_ids),
                                C.c_void_p(d_row_off), n_rows, *_dptrs(d_q_row, d_answers), max_len, stride, max_query_len, skip_front, skip_back,
                                *_dptrs(d_input_ids, d_mask, d_type, d_pair, d_start, d_n_real, d_q_len, d_start_pos, d_end_pos, d_has_answer),
                                C.c_void_p(d_win_off), capacity)

    def span_tokens(self, counts, word_off, mark_words, mark_off):
        """counts int32 [W], word_off int64 [n+1], mark_words int32 [S, 2], mark_off int64 [n+1] -> span_tokens int32 [S, 2] (gz_span_tokens)."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        mark_words = np.ascontiguousarray(mark_words, dtype=np.int32)
        mark_off = np.ascontiguousarray(mark_off, dtype=np.int64)
        out = np.empty((len(mark_words), 2), dtype=np.int32)
        self._check(self.lib.gz_span_tokens(self.handle, _ptr(counts) if len(counts) else None, _ptr(word_off), len(word_off) - 1,
                                            _ptr(mark_words) if len(mark_words) else None, _ptr(mark_off), _ptr(out) if len(out) else None))
        return out

    def span_tokens_device(self, d_counts, d_word_off, n_docs, n_words, d_mark_words, d_mark_off, n_marks, d_span_tokens):
        """gz_span_tokens_device: every pointer a device address (0: NULL)."""
        self._check(self.lib.gz_span_tokens_device(self.handle, *_dptrs(d_counts), C.c_void_p(d_word_off), n_docs, n_words, *_dptrs(d_mark_words),
                                                   C.c_void_p(d_mark_off), n_marks, *_dptrs(d_span_tokens)))

    # ---- short documents packed into rows of max_len ------------------------------------------------------
    def pack_rows(self, ids: np.ndarray, row_off: np.ndarray, max_len: int, framed: bool):
        """ids int32 (packed rows), row_off int64 [n+1] -> dict(input_ids, attention_mask, segment_ids, position_ids [R, L],
        doc_row, doc_col, doc_len [n], row_off int64 [R+1], seg_off int64 [n+1]) (gz_pack_rows: a sizing call, then the rows)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        n, L, skip = len(row_off) - 1, int(max_len), 1 if framed else 0
        maps = dict(doc_row=np.empty(n, dtype=np.int32), doc_col=np.empty(n, dtype=np.int32), doc_len=np.empty(n, dtype=np.int32),
                    row_off=np.zeros(n + 1, dtype=np.int64), seg_off=np.zeros(n + 1, dtype=np.int64))
        total = C.c_int64()
        head = (self.handle, _ptr(ids) if len(ids) else None, _ptr(row_off), n, L, skip, skip)
        tail = tuple(_ptr(maps[k]) for k in ("doc_row", "doc_col", "doc_len", "row_off", "seg_off"))
        self._check(self.lib.gz_pack_rows(*head, None, None, None, None, *tail, 0, C.byref(total)))
        R = total.value
        out = {k: np.empty((R, L), dtype=np.int32) for k in ("input_ids", "attention_mask", "segment_ids", "position_ids")}
        if R:
            self._check(self.lib.gz_pack_rows(*head, *[_ptr(v) for v in out.values()], *tail, R, C.byref(total)))
        out.update(maps)
        out["row_off"] = maps["row_off"][:R + 1].copy()
        return out

    def pack_rows_device(self, d_ids, d_row_off, n_rows, max_len, skip_front, skip_back, d_input_ids, d_mask, d_seg, d_pos, d_doc_row,
                         d_doc_col, d_doc_len, d_pack_off, d_seg_off, capacity) -> int:
        """gz_pack_rows_device: returns R.  d_input_ids == 0 sizes only; on GZ_E_CAPACITY the GzError carries `.total` = R."""
        opt = _dptrs(d_input_ids, d_mask, d_seg, d_pos, d_doc_row, d_doc_col, d_doc_len)
        return self._call_total(self.lib.gz_pack_rows_device, self.handle, *_dptrs(d_ids), C.c_void_p(d_row_off), n_rows, max_len, skip_front,
                                skip_back, *opt, C.c_void_p(d_pack_off), *_dptrs(d_seg_off), capacity)

    # ---- best-fit packing -----------------------------------------------------------------------------------
    def pack_rows_fit(self, ids: np.ndarray, row_off: np.ndarray, max_len: int, framed: bool):
        """`pack_rows` in best-fit order (gz_pack_rows_fit): the same dict plus row_docs int32 [n], the documents in packed order;
        row_off int64 [R+1] indexes row_docs, seg_off int64 [n+1] is the scan of doc_len[row_docs]."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        n, L, skip = len(row_off) - 1, int(max_len), 1 if framed else 0
        maps = dict(doc_row=np.empty(n, dtype=np.int32), doc_col=np.empty(n, dtype=np.int32), doc_len=np.empty(n, dtype=np.int32),
                    row_docs=np.empty(n, dtype=np.int32), row_off=np.zeros(n + 1, dtype=np.int64), seg_off=np.zeros(n + 1, dtype=np.int64))
        total = C.c_int64()
        head = (self.handle, _ptr(ids) if len(ids) else None, _ptr(row_off), n, L, skip, skip)
        tail = tuple(_ptr(maps[k]) for k in ("doc_row", "doc_col", "doc_len", "row_docs", "row_off", "seg_off"))
        self._check(self.lib.gz_pack_rows_fit(*head, None, None, None, None, *tail, 0, C.byref(total)))
        R = total.value
        out = {k: np.empty((R, L), dtype=np.int32) for k in ("input_ids", "attention_mask", "segment_ids", "position_ids")}
        if R:
            self._check(self.lib.gz_pack_rows_fit(*head, *[_ptr(v) for v in out.values()], *tail, R, C.byref(total)))
        out.update(maps)
        out["row_off"] = maps["row_off"][:R + 1].copy()
        return out

    def pack_rows_fit_device(self, d_ids, d_row_off, n_rows, max_len, skip_front, skip_back, d_input_ids, d_mask, d_seg, d_pos, d_doc_row,
                             d_doc_col, d_doc_len, d_row_docs, d_pack_off, d_seg_off, capacity) -> int:
        """gz_pack_rows_fit_device: returns R.  d_input_ids == 0 sizes only; on GZ_E_CAPACITY the GzError carries `.total` = R."""
        opt = _dptrs(d_input_ids, d_mask, d_seg, d_pos, d_doc_row, d_doc_col, d_doc_len, d_row_docs)
        return self._call_total(self.lib.gz_pack_rows_fit_device, self.handle, *_dptrs(d_ids), C.c_void_p(d_row_off), n_rows, max_len, skip_front,
                                skip_back, *opt, C.c_void_p(d_pack_off), *_dptrs(d_seg_off), capacity)

    # ---- masked-LM inputs and labels ------------------------------------------------------------------------
    def mask_rows(self, ids: np.ndarray, rule, row_base: int = 0):
        """ids int32 [R, L]; rule = (seed, t_sel, t1, t2, rand_lo, rand_hi, mask_id, whole_word, ignore_index) as gz_mask_rows takes
        them -> dict(input_ids [R, L], labels [R, L], n_chosen [R])."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        R, L = ids.shape
        out = dict(input_ids=np.empty((R, L), dtype=np.int32), labels=np.empty((R, L), dtype=np.int32), n_chosen=np.empty(R, dtype=np.int32))
        self._check(self.lib.gz_mask_rows(self.handle, _ptr(ids) if R else None, R, L, int(row_base), *rule,
                                          *[_ptr(out[k]) if R else None for k in ("input_ids", "labels", "n_chosen")]))
        return out

    def mask_rows_device(self, d_ids, n_rows, row_len, row_base, rule, d_input_ids, d_labels, d_n_chosen):
        """gz_mask_rows_device: every pointer a device address (0: NULL); `rule` as in mask_rows."""
        self._check(self.lib.gz_mask_rows_device(self.handle, *_dptrs(d_ids), n_rows, row_len, row_base, *rule,
                                                 *_dptrs(d_input_ids, d_labels, d_n_chosen)))

    # ---- span-corruption inputs and targets ------------------------------------------------------------------
    @staticmethod
    def _infill_args(rule):
        """rule = (seed, t_start, len_t (n_len - 1 integers), n_len, mask_id, whole_word, ignore_index, dec_width) -> the eight
        arguments of gz_infill_rows behind row_base, and the array that keeps len_t alive during the call"""
        seed, t_start, len_t, n_len, mask_id, whole_word, ignore_index, dec_width = rule
        arr = np.ascontiguousarray(list(len_t) + [0], dtype=np.uint64)          # (never empty: n_len == 1 reads none of it)
        return (seed, t_start, _ptr(arr), n_len, mask_id, whole_word, ignore_index, dec_width), arr

    def infill_rows(self, ids: np.ndarray, rule, row_base: int = 0):
        """ids int32 [R, L]; rule as in _infill_args -> dict(input_ids [R, L], attention_mask [R, L], labels [R, W],
        decoder_input_ids [R, W], enc_len [R], dec_len [R], n_spans [R])."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        R, L = ids.shape
        W = rule[7]
        out = dict(input_ids=np.empty((R, L), dtype=np.int32), attention_mask=np.empty((R, L), dtype=np.int32),
                   labels=np.empty((R, W), dtype=np.int32), decoder_input_ids=np.empty((R, W), dtype=np.int32),
                   enc_len=np.empty(R, dtype=np.int32), dec_len=np.empty(R, dtype=np.int32), n_spans=np.empty(R, dtype=np.int32))
        args, keep = self._infill_args(rule)
        self._check(self.lib.gz_infill_rows(self.handle, _ptr(ids) if R else None, R, L, int(row_base), *args,
                                            *[_ptr(v) if R else None for v in out.values()]))
        del keep
        return out

    def infill_rows_device(self, d_ids, n_rows, row_len, row_base, rule, d_input_ids, d_attention_mask, d_labels, d_decoder_input_ids,
                           d_enc_len, d_dec_len, d_n_spans):
        """gz_infill_rows_device: every pointer a device address (0: NULL); `rule` as in infill_rows (len_t stays on the host)."""
        args, keep = self._infill_args(rule)
        self._check(self.lib.gz_infill_rows_device(self.handle, *_dptrs(d_ids), n_rows, row_len, row_base, *args,
                                                   *_dptrs(d_input_ids, d_attention_mask, d_labels, d_decoder_input_ids, d_enc_len, d_dec_len,
                                                            d_n_spans)))
        del keep

    # ---- MinHash signatures and near-duplicate groups -------------------------------------------------------
    def minhash_rows(self, ids: np.ndarray, row_off: np.ndarray, num_perm: int, shingle: int, seed: int, framed: bool):
        """ids int32 (packed rows), row_off int64 [n+1] -> dict(signatures uint32 [n, K], n_shingles int32 [n]) (gz_minhash_rows)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        n, K, skip = len(row_off) - 1, int(num_perm), 1 if framed else 0
        out = dict(signatures=np.empty((n, K), dtype=np.uint32), n_shingles=np.empty(n, dtype=np.int32))
        self._check(self.lib.gz_minhash_rows(self.handle, _ptr(ids) if len(ids) else None, _ptr(row_off), n, skip, skip, int(shingle), K,
                                             int(seed), *[_ptr(v) if n else None for v in out.values()]))
        return out

    def minhash_rows_device(self, d_ids, d_row_off, n_rows, skip_front, skip_back, shingle, num_perm, seed, d_signatures, d_n_shingles):
        """gz_minhash_rows_device: every pointer a device address (0: NULL)."""
        self._check(self.lib.gz_minhash_rows_device(self.handle, *_dptrs(d_ids, d_row_off), n_rows, skip_front, skip_back, shingle, num_perm,
                                                    seed, *_dptrs(d_signatures, d_n_shingles)))

    def minhash_groups(self, signatures: np.ndarray, bands: int, min_agree: int):
        """signatures uint32 [n, K] -> (group int32 [n], n_groups) (gz_minhash_groups)."""
        sig = np.ascontiguousarray(signatures, dtype=np.uint32)
        n, K = sig.shape
        group = np.empty(n, dtype=np.int32)
        total = self._call_total(self.lib.gz_minhash_groups, self.handle, _ptr(sig) if n else None, n, K, int(bands), int(min_agree),
                                 _ptr(group) if n else None)
        return group, total

    def minhash_groups_device(self, d_signatures, n_rows, num_perm, bands, min_agree, d_group) -> int:
        """gz_minhash_groups_device: signatures and group device addresses (0: NULL); returns n_groups."""
        return self._call_total(self.lib.gz_minhash_groups_device, self.handle, *_dptrs(d_signatures), n_rows, num_perm, bands, min_agree,
                                *_dptrs(d_group))

    # ---- exact token n-gram overlap against a held-out set -------------------------------------------------------
    NGRAM_OUT = ("n_grams", "n_hits", "n_covered", "first_hit", "first_ref")

    def ngram_index_build(self, ids: np.ndarray, row_off: np.ndarray, n: int, framed: bool) -> int:
        """ids int32 (packed reference rows), row_off int64 [R+1] -> handle of an n-gram index (gz_ngram_index_build)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        R, skip = len(row_off) - 1, 1 if framed else 0
        h = C.c_void_p()
        self._check(self.lib.gz_ngram_index_build(self.handle, _ptr(ids) if len(ids) else None, _ptr(row_off), R, skip, skip, int(n), C.byref(h)))
        return h.value

    def ngram_index_build_device(self, d_ids, d_row_off, n_rows, skip_front, skip_back, n) -> int:
        """gz_ngram_index_build_device: ids and offsets device addresses (0: NULL) -> handle."""
        h = C.c_void_p()
        self._check(self.lib.gz_ngram_index_build_device(self.handle, *_dptrs(d_ids, d_row_off), n_rows, skip_front, skip_back, n, C.byref(h)))
        return h.value

    def ngram_index_info(self, index: int):
        """dict(n, n_rows, n_ids, n_grams, n_distinct, slots, device_bytes, context_bytes) (gz_ngram_index_info)"""
        info = np.zeros(8, dtype=np.int64)
        self._check(self.lib.gz_ngram_index_info(C.c_void_p(index), _ptr(info)))
        return dict(zip(("n", "n_rows", "n_ids", "n_grams", "n_distinct", "slots", "device_bytes", "context_bytes"), (int(v) for v in info)))

    def ngram_index_destroy(self, index: int):
        if index and getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.gz_ngram_index_destroy(C.c_void_p(index))

    def ngram_overlap(self, index: int, ids: np.ndarray, row_off: np.ndarray, framed: bool, with_covered: bool):
        """ids int32 (packed rows), row_off int64 [n+1] -> dict of the five int32 [n] arrays, and `covered` uint8 when asked for
        (gz_ngram_overlap)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        n, skip = len(row_off) - 1, 1 if framed else 0
        out = {k: np.empty(n, dtype=np.int32) for k in self.NGRAM_OUT}
        covered = np.zeros(len(ids), dtype=np.uint8) if with_covered else None
        self._check(self.lib.gz_ngram_overlap(self.handle, C.c_void_p(index), _ptr(ids) if len(ids) else None, _ptr(row_off), n, skip, skip,
                                              *[_ptr(v) if n else None for v in out.values()], _ptr(covered) if with_covered and len(ids) else None))
        if with_covered:
            out["covered"] = covered
        return out

    def ngram_overlap_device(self, index: int, d_ids, d_row_off, n_rows, skip_front, skip_back, d_n_grams, d_n_hits, d_n_covered, d_first_hit,
                             d_first_ref, d_covered):
        """gz_ngram_overlap_device: every pointer a device address (0: NULL)."""
        self._check(self.lib.gz_ngram_overlap_device(self.handle, C.c_void_p(index), *_dptrs(d_ids, d_row_off), n_rows, skip_front, skip_back,
                                                     *_dptrs(d_n_grams, d_n_hits, d_n_covered, d_first_hit, d_first_ref, d_covered)))

    # ---- n-gram repetition inside a document -----------------------------------------------------------------------
    REPEAT_OUT = ("n_grams", "n_distinct", "n_repeated", "n_covered", "top_count", "top_pos")

    def ngram_repeats(self, ids: np.ndarray, row_off: np.ndarray, widths, framed: bool, with_covered: bool):
        """ids int32 (packed rows), row_off int64 [n+1], widths a sequence of ints -> dict of the six int32 [K, n] arrays, and
        `covered` uint16 when asked for (gz_ngram_repeats)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        w = np.ascontiguousarray(widths, dtype=np.int32)
        n, skip = len(row_off) - 1, 1 if framed else 0
        out = {k: np.empty((len(w), n), dtype=np.int32) for k in self.REPEAT_OUT}
        covered = np.zeros(len(ids), dtype=np.uint16) if with_covered else None
        self._check(self.lib.gz_ngram_repeats(self.handle, _ptr(ids) if len(ids) else None, _ptr(row_off), n, skip, skip, _ptr(w), len(w),
                                              *[_ptr(v) if n else None for v in out.values()], _ptr(covered) if with_covered and len(ids) else None))
        if with_covered:
            out["covered"] = covered
        return out

    def ngram_repeats_device(self, d_ids, d_row_off, n_rows, skip_front, skip_back, widths, d_n_grams, d_n_distinct, d_n_repeated, d_n_covered,
                             d_top_count, d_top_pos, d_covered):
        """gz_ngram_repeats_device: ids, offsets and outputs device addresses (0: NULL); widths a sequence of ints on the host."""
        w = np.ascontiguousarray(widths, dtype=np.int32)
        self._check(self.lib.gz_ngram_repeats_device(self.handle, *_dptrs(d_ids, d_row_off), n_rows, skip_front, skip_back, _ptr(w), len(w),
                                                     *_dptrs(d_n_grams, d_n_distinct, d_n_repeated, d_n_covered, d_top_count, d_top_pos, d_covered)))

    # ---- word spans, word ids and aligned labels ----------------------------------------------------------------
    def word_spans(self, text: np.ndarray, text_off: np.ndarray, unit: int):
        """packed UTF-8, int64 offsets [n+1] -> (span int32 [W, 2], word_off int64 [n+1]) (gz_word_spans: a sizing call, then the spans)."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        n = len(text_off) - 1
        word_off = np.zeros(n + 1, dtype=np.int64)
        total = C.c_int64()
        head = (self.handle, _ptr(text) if len(text) else None, _ptr(text_off), n, int(unit))
        self._check(self.lib.gz_word_spans(*head, None, _ptr(word_off), 0, C.byref(total)))
        W = total.value
        span = np.empty((W, 2), dtype=np.int32)
        if W:
            self._check(self.lib.gz_word_spans(*head, _ptr(span), _ptr(word_off), W, C.byref(total)))
        return span, word_off

    def word_spans_device(self, d_text, d_text_off, n_docs, text_bytes, unit, d_span, d_word_off, capacity) -> int:
        """gz_word_spans_device: returns W.  d_span == 0 sizes only; on GZ_E_CAPACITY the GzError carries `.total` = W."""
        return self._call_total(self.lib.gz_word_spans_device, self.handle, *_dptrs(d_text), C.c_void_p(d_text_off), n_docs, text_bytes, unit,
                                *_dptrs(d_span), C.c_void_p(d_word_off), capacity)

    def align_rows(self, counts, word_off, max_len, word_labels, row_doc, row_start, continuation, cont_map, ignore_index, want=(True, True, True)):
        """counts int32 [W], word_off int64 [n+1] (+ optional int32 arrays) -> dict(word_ids [R, L], labels [R, L] when word_labels is given,
        n_real [R]) (gz_align_rows).  want: which of (word_ids, labels, n_real) to take."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        n, L = len(word_off) - 1, int(max_len)
        R = n if row_doc is None else len(row_doc)
        out = {}
        if want[0]:
            out["word_ids"] = np.empty((R, L), dtype=np.int32)
        if want[1] and word_labels is not None:
            out["labels"] = np.empty((R, L), dtype=np.int32)
        if want[2]:
            out["n_real"] = np.empty(R, dtype=np.int32)
        self._check(self.lib.gz_align_rows(self.handle, _ptr(counts) if len(counts) else None, _ptr(word_off), n, _ptr(row_doc), _ptr(row_start), R, L,
                                           _ptr(word_labels), int(continuation), _ptr(cont_map), 0 if cont_map is None else len(cont_map),
                                           int(ignore_index), _ptr(out.get("word_ids")), _ptr(out.get("labels")), _ptr(out.get("n_real"))))
        return out

    def align_rows_device(self, d_counts, d_word_off, n_docs, n_words, d_row_doc, d_row_start, n_rows, max_len, d_word_labels, continuation, d_cont_map,
                          n_map, ignore_index, d_word_ids, d_labels, d_n_real):
        """gz_align_rows_device: every pointer a device address (0: NULL)."""
        self._check(self.lib.gz_align_rows_device(self.handle, *_dptrs(d_counts), C.c_void_p(d_word_off), n_docs, n_words, *_dptrs(d_row_doc, d_row_start),
                                                  n_rows, max_len, *_dptrs(d_word_labels), continuation, *_dptrs(d_cont_map), n_map, ignore_index,
                                                  *_dptrs(d_word_ids, d_labels, d_n_real)))

    def span_labels(self, span, word_off, marks, mark_off, scheme: int, outside: int):
        """span int32 [W, 2], word_off int64 [n+1], marks int32 [S, 3], mark_off int64 [n+1] -> (word_labels int32 [W], mark_words int32 [S, 2])
        (gz_span_labels)."""
        span = np.ascontiguousarray(span, dtype=np.int32)
        word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        marks = np.ascontiguousarray(marks, dtype=np.int32)
        mark_off = np.ascontiguousarray(mark_off, dtype=np.int64)
        n = len(word_off) - 1
        word_labels = np.empty(len(span), dtype=np.int32)
        mark_words = np.empty((len(marks), 2), dtype=np.int32)
        self._check(self.lib.gz_span_labels(self.handle, _ptr(span) if len(span) else None, _ptr(word_off), n, _ptr(marks) if len(marks) else None,
                                            _ptr(mark_off), int(scheme), int(outside), _ptr(word_labels) if len(span) else None,
                                            _ptr(mark_words) if len(marks) else None))
        return word_labels, mark_words

    def span_labels_device(self, d_span, d_word_off, n_docs, n_words, d_marks, d_mark_off, n_marks, scheme, outside, d_word_labels, d_mark_words):
        """gz_span_labels_device: every pointer a device address (0: NULL)."""
        self._check(self.lib.gz_span_labels_device(self.handle, *_dptrs(d_span), C.c_void_p(d_word_off), n_docs, n_words, *_dptrs(d_marks),
                                                   C.c_void_p(d_mark_off), n_marks, scheme, outside, *_dptrs(d_word_labels, d_mark_words)))

    # ---- text pre-pass ----------------------------------------------------------------------------------
    def preprocess(self, ops, text: np.ndarray, text_off: np.ndarray):
        """packed UTF-8 + int64 offsets -> (packed UTF-8, int64 offsets) after applying the GZ_PP_* filters in order."""
        ops = np.ascontiguousarray(ops, dtype=np.int32)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        n = len(text_off) - 1
        cap = int(text_off[n] - text_off[0])
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.int64)
        self._check(self.lib.gz_preprocess_batch(self.handle, _ptr(ops), len(ops), _ptr(text) if len(text) else None,
                                                 _ptr(text_off), n, _ptr(out), cap, _ptr(out_off)))
        return out[:int(out_off[n])], out_off

    def preprocess_device(self, ops, d_text, d_off, n_docs, text_bytes, d_out, capacity, d_out_off) -> int:
        ops = np.ascontiguousarray(ops, dtype=np.int32)
        total = C.c_int64()
        self._check(self.lib.gz_preprocess_batch_device(self.handle, _ptr(ops), len(ops), C.c_void_p(d_text), C.c_void_p(d_off),
                                                        n_docs, text_bytes, *_dptrs(d_out), capacity,
                                                        C.c_void_p(d_out_off), C.byref(total)))
        return total.value

    # ---- BM25 index (ranking.py) ----------------------------------------------------------------------------
    # ---- learn: word sets and the BPE learner ---------------------------------------------------------------------------------
    def wordset_build(self, text: np.ndarray, text_off: np.ndarray) -> int:
        """gz_wordset_build: the distinct words of packed documents (uint8 text, int64 offsets [n + 1]) -> handle"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        h = C.c_void_p()
        self._check(self.lib.gz_wordset_build(self.handle, _ptr(text), _ptr(text_off), len(text_off) - 1, C.byref(h)))
        return h.value

    def wordset_build_device(self, d_text, d_off, n_docs: int, text_bytes: int) -> int:
        h = C.c_void_p()
        self._check(self.lib.gz_wordset_build_device(self.handle, *_dptrs(d_text, d_off), int(n_docs), int(text_bytes), C.byref(h)))
        return h.value

    def wordset_from_counts(self, words: np.ndarray, word_off: np.ndarray, counts: np.ndarray) -> int:
        words = np.ascontiguousarray(words, dtype=np.uint8)
        word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        h = C.c_void_p()
        self._check(self.lib.gz_wordset_from_counts(self.handle, _ptr(words), _ptr(word_off), _ptr(counts), len(counts), C.byref(h)))
        return h.value

    def wordset_destroy(self, ws: int):
        if ws and getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.gz_wordset_destroy(C.c_void_p(ws))

    def wordset_info(self, ws: int):
        """(distinct words, their bytes, the sum of the counts)"""
        n, b, t = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.gz_wordset_info(C.c_void_p(ws), C.byref(n), C.byref(b), C.byref(t)))
        return n.value, b.value, t.value

    def wordset_words(self, ws: int):
        """(bytes uint8, offsets int64 [n + 1], counts int64 [n]) of the distinct words, first-occurrence order"""
        n, nb, _ = self.wordset_info(ws)
        off = np.zeros(n + 1, dtype=np.int64)
        cnt = np.zeros(n, dtype=np.int64)
        data = np.zeros(nb, dtype=np.uint8)
        self._check(self.lib.gz_wordset_words(C.c_void_p(ws), _ptr(off), _ptr(cnt), _ptr(data), nb))
        return data, off, cnt

    def bpe_learn(self, ws: int, n_merges: int, min_frequency: int):
        """gz_bpe_learn + gz_bpe_learn_result -> (info [8], merge bytes, merge offsets, piece bytes, piece offsets, piece counts)"""
        info = np.zeros(8, dtype=np.int64)
        self._check(self.lib.gz_bpe_learn(C.c_void_p(ws), int(n_merges), int(min_frequency), _ptr(info)))
        m, mb, p, pb = int(info[0]), int(info[2]), int(info[3]), int(info[4])
        moff = np.zeros(2 * m + 1, dtype=np.int64)
        mbytes = np.zeros(mb, dtype=np.uint8)
        poff = np.zeros(p + 1, dtype=np.int64)
        pcnt = np.zeros(p, dtype=np.int64)
        pbytes = np.zeros(pb, dtype=np.uint8)
        self._check(self.lib.gz_bpe_learn_result(C.c_void_p(ws), _ptr(moff), _ptr(mbytes), mb, _ptr(poff), _ptr(pcnt), _ptr(pbytes), pb))
        return info, mbytes, moff, pbytes, poff, pcnt

    def bm25_build(self, text: np.ndarray, text_off: np.ndarray, positions: bool = False) -> int:
        """packed UTF-8 + int64 offsets -> a gz_bm25 handle (int), owned by this context.  positions: a positional index
        (gz_bm25_build_ex with GZ_BM25_POSITIONS), which keeps every word's term id for phrase searches; else gz_bm25_build."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        h = C.c_void_p()
        args = [self.handle, _ptr(text) if len(text) else None, _ptr(text_off), len(text_off) - 1]
        if positions:
            self._check(self.lib.gz_bm25_build_ex(*args, GZ_BM25_POSITIONS, C.byref(h)))
        else:
            self._check(self.lib.gz_bm25_build(*args, C.byref(h)))
        return h.value

    def bm25_build_device(self, d_text, d_off, n_docs: int, text_bytes: int, positions: bool = False) -> int:
        h = C.c_void_p()
        args = [self.handle, *_dptrs(d_text), C.c_void_p(d_off), n_docs, text_bytes]
        if positions:
            self._check(self.lib.gz_bm25_build_device_ex(*args, GZ_BM25_POSITIONS, C.byref(h)))
        else:
            self._check(self.lib.gz_bm25_build_device(*args, C.byref(h)))
        return h.value

    def bm25_flags(self, index: int) -> int:
        """the flags the index was built with (GZ_BM25_POSITIONS or 0)"""
        f = C.c_int32()
        self._check(self.lib.gz_bm25_flags(C.c_void_p(index), C.byref(f)))
        return f.value

    def bm25_sequence(self, index: int):
        """(terms int32 [n_words], offsets int64 [documents + 1]) of a positional index: the term id of every word, documents in id
        order, words in str.split() order; document d = terms[offsets[d]:offsets[d + 1]].  GzError (GZ_E_INVALID) without positions."""
        n, _, w = self.bm25_info(index)
        terms = np.empty(max(w, 1), dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.int64)
        self._check(self.lib.gz_bm25_sequence(C.c_void_p(index), _ptr(terms), _ptr(off)))
        return terms[:w], off

    def bm25_append(self, index: int, text: np.ndarray, text_off: np.ndarray) -> None:
        """packed UTF-8 + int64 offsets of more documents behind the index's own: afterwards it answers as one built over all of
        them.  On GzError the index is as it was."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        text_off = np.ascontiguousarray(text_off, dtype=np.int64)
        self._check(self.lib.gz_bm25_append(C.c_void_p(index), _ptr(text) if len(text) else None, _ptr(text_off), len(text_off) - 1))

    def bm25_append_device(self, index: int, d_text, d_off, n_docs: int, text_bytes: int) -> None:
        self._check(self.lib.gz_bm25_append_device(C.c_void_p(index), *_dptrs(d_text, d_off), n_docs, text_bytes))

    def bm25_remove(self, index: int, ids: np.ndarray) -> None:
        """document ids (int64; any order, duplicates allowed) leave the index: afterwards it answers as one built over the
        remaining documents, renumbered in their old order.  On GzError the index is as it was."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        self._check(self.lib.gz_bm25_remove(C.c_void_p(index), _ptr(ids) if len(ids) else None, len(ids)))

    def bm25_remove_device(self, index: int, d_ids, n_ids: int) -> None:
        self._check(self.lib.gz_bm25_remove_device(C.c_void_p(index), *_dptrs(d_ids), n_ids))

    def bm25_compact(self, index: int) -> None:
        """the index becomes the one a fresh build of its current documents gives, term ids and buffer sizes included.  On
        GzError the index is as it was."""
        self._check(self.lib.gz_bm25_compact(C.c_void_p(index)))

    def bm25_terms(self, index: int):
        """(term_off int64 [T + 1], bytes uint8 [term_off[T]], df int32 [T]): the live terms in the order of their first
        occurrence in the current documents.  The index is not modified."""
        t = self.bm25_info(index)[1]
        off = np.zeros(t + 1, dtype=np.int64)
        df = np.empty(max(t, 1), dtype=np.int32)
        self._check(self.lib.gz_bm25_terms(C.c_void_p(index), _ptr(off), _ptr(df), None, 0))       # sizes first
        data = np.empty(max(int(off[t]), 1), dtype=np.uint8)
        if off[t]:
            self._check(self.lib.gz_bm25_terms(C.c_void_p(index), None, None, _ptr(data), int(off[t])))
        return off, data[:int(off[t])], df[:t]

    def bm25_similar(self, index: int, words: np.ndarray, word_off: np.ndarray, max_edits: int, k: int):
        """packed words -> (ids int64 [W, k'], dist int32 [W, k'], df int32 [W, k'], counts int64 [W]) with k' = min(k, live terms):
        the terms within max_edits of every word in ascending (distance, -df, id), ids as bm25_terms numbers them; -1 / -1 / 0 behind
        a row's count.  The index is not modified."""
        words = np.ascontiguousarray(words, dtype=np.uint8)
        word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        n = len(word_off) - 1
        kk = max(0, min(int(k), self.bm25_info(index)[1]))
        ids = np.empty((n, kk), dtype=np.int64)
        dist = np.empty((n, kk), dtype=np.int32)
        df = np.empty((n, kk), dtype=np.int32)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self.lib.gz_bm25_similar(C.c_void_p(index), _ptr(words) if len(words) else None, _ptr(word_off), n, int(max_edits), int(k),
                                             _ptr(ids) if ids.size else None, _ptr(dist) if dist.size else None,
                                             _ptr(df) if df.size else None, _ptr(counts)))
        return ids, dist, df, counts[:n]

    def bm25_prefix(self, index: int, words: np.ndarray, word_off: np.ndarray, k: int):
        """packed words -> (ids int64 [W, k'], df int32 [W, k'], counts int64 [W]): the terms that start with every word in ascending
        (-df, id); shapes, ids and padding as bm25_similar."""
        words = np.ascontiguousarray(words, dtype=np.uint8)
        word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        n = len(word_off) - 1
        kk = max(0, min(int(k), self.bm25_info(index)[1]))
        ids = np.empty((n, kk), dtype=np.int64)
        df = np.empty((n, kk), dtype=np.int32)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self.lib.gz_bm25_prefix(C.c_void_p(index), _ptr(words) if len(words) else None, _ptr(word_off), n, int(k),
                                            _ptr(ids) if ids.size else None, _ptr(df) if df.size else None, _ptr(counts)))
        return ids, df, counts[:n]

    def bm25_term_bytes(self, index: int, ids: np.ndarray):
        """(off int64 [n + 1], bytes uint8 [off[n]]) of the listed terms (ids as bm25_terms numbers them; -1: no term, no bytes):
        only these terms' bytes are gathered and copied."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
        n = len(ids)
        off = np.zeros(n + 1, dtype=np.int64)
        self._check(self.lib.gz_bm25_term_bytes(C.c_void_p(index), _ptr(ids) if n else None, n, _ptr(off), None, 0))     # sizes first
        data = np.empty(max(int(off[n]), 1), dtype=np.uint8)
        if off[n]:
            self._check(self.lib.gz_bm25_term_bytes(C.c_void_p(index), _ptr(ids), n, None, _ptr(data), int(off[n])))
        return off, data[:int(off[n])]

    def bm25_footprint(self, index: int):
        """(text bytes in use, terms held in the term table -- dead ones included, device bytes allocated to the index)"""
        out = (C.c_int64 * 3)()
        self._check(self.lib.gz_bm25_footprint(C.c_void_p(index), out))
        return out[0], out[1], out[2]

    def bm25_destroy(self, index: int):
        if index and self.handle.value:                  # (a closed context has freed its indexes already)
            self.lib.gz_bm25_destroy(C.c_void_p(index))

    def bm25_info(self, index: int):
        """(documents, distinct terms, words)"""
        n, t, w = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.gz_bm25_info(C.c_void_p(index), C.byref(n), C.byref(t), C.byref(w)))
        return n.value, t.value, w.value

    def bm25_field_lengths(self, index: int) -> np.ndarray:
        n = self.bm25_info(index)[0]
        out = np.empty(max(n, 1), dtype=np.int32)
        self._check(self.lib.gz_bm25_field_lengths(C.c_void_p(index), _ptr(out)))
        return out[:n]

    def bm25_lookup(self, index: int, words: np.ndarray, word_off: np.ndarray):
        """packed query words -> (term ids int32, -1 when absent; df int32)"""
        words = np.ascontiguousarray(words, dtype=np.uint8)
        word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        n = len(word_off) - 1
        term = np.empty(max(n, 1), dtype=np.int32)
        df = np.empty(max(n, 1), dtype=np.int32)
        self._check(self.lib.gz_bm25_lookup(C.c_void_p(index), _ptr(words) if len(words) else None, _ptr(word_off), n, _ptr(term), _ptr(df)))
        return term[:n], df[:n]

    def bm25_score(self, index: int, terms: np.ndarray, idf: np.ndarray, query_off: np.ndarray, params, plus: bool,
                   d_out: int | None = None):
        """scores [Q, N] float64 (host), or enqueued into d_out (device pointer; sync() waits) when it is given."""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        idf = np.ascontiguousarray(idf, dtype=np.float64)
        query_off = np.ascontiguousarray(query_off, dtype=np.int64)
        P = np.ascontiguousarray(params, dtype=np.float64)
        assert P.shape == (6,)
        nq = len(query_off) - 1
        args = [C.c_void_p(index), _ptr(terms) if len(terms) else None, _ptr(idf) if len(idf) else None, _ptr(query_off), nq, _ptr(P),
                1 if plus else 0]
        if d_out is not None:
            self._check(self.lib.gz_bm25_score_device(*args, C.c_void_p(d_out)))
            return None
        n = self.bm25_info(index)[0]
        out = np.empty((nq, n), dtype=np.float64)
        self._check(self.lib.gz_bm25_score(*args, _ptr(out) if out.size else None))
        return out

    def bm25_topk(self, index: int, terms: np.ndarray, idf: np.ndarray, query_off: np.ndarray, params, plus: bool, k: int,
                  d_ids: int | None = None, d_scores: int | None = None):
        """(ids int64 [Q, k'], scores float64 [Q, k']) with k' = min(k, documents): the best documents of every query (host), or
        enqueued into d_ids / d_scores (device pointers; sync() waits) when they are given."""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        idf = np.ascontiguousarray(idf, dtype=np.float64)
        query_off = np.ascontiguousarray(query_off, dtype=np.int64)
        P = np.ascontiguousarray(params, dtype=np.float64)
        assert P.shape == (6,)
        nq = len(query_off) - 1
        args = [C.c_void_p(index), _ptr(terms) if len(terms) else None, _ptr(idf) if len(idf) else None, _ptr(query_off), nq, _ptr(P),
                1 if plus else 0, int(k)]
        if d_ids is not None or d_scores is not None:
            self._check(self.lib.gz_bm25_topk_device(*args, C.c_void_p(d_ids), C.c_void_p(d_scores)))
            return None
        kk = max(0, min(int(k), self.bm25_info(index)[0]))
        ids = np.empty((nq, kk), dtype=np.int64)
        scores = np.empty((nq, kk), dtype=np.float64)
        self._check(self.lib.gz_bm25_topk(*args, _ptr(ids) if ids.size else None, _ptr(scores) if scores.size else None))
        return ids, scores

    def bm25_search(self, index: int, terms: np.ndarray, idf: np.ndarray, query_off: np.ndarray, params, plus: bool, k: int,
                    d_ids: int | None = None, d_scores: int | None = None, d_counts: int | None = None,
                    mode: int = 0, ex_terms=None, ex_off=None, ph_terms=None, ph_off=None, nr_terms=None, nr_off=None, nr_window=None):
        """(ids int64 [Q, k'], scores float64 [Q, k'], counts int64 [Q]) with k' = min(k, documents): the best MATCHING documents of
        every query and how many match; positions behind a row's count hold -1 / NaN.  A document matches when it holds at least
        one of the query's words (mode 0) or every one of them (mode 1), and none of the terms ex_terms[ex_off[q]:ex_off[q + 1]]
        (ex_off None: no exclusions).  With mode 0 and ex_off None the call is gz_bm25_search[_device], else gz_bm25_search_bool[_device].
        ph_off (None: no phrases) / ph_terms: the terms ph_terms[ph_off[q]:ph_off[q + 1]] must stand next to each other in this order
        in the document (a positional index only): the call is gz_bm25_search_phrase[_device].
        nr_off (None: no near sets) / nr_terms / nr_window (int64 [Q]): every term of nr_terms[nr_off[q]:nr_off[q + 1]] must stand
        inside some nr_window[q] consecutive words of the document, in any order: the call is gz_bm25_search_near[_device].
        With d_ids / d_scores / d_counts (device pointers, all three): enqueued into them, sync() waits."""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        idf = np.ascontiguousarray(idf, dtype=np.float64)
        query_off = np.ascontiguousarray(query_off, dtype=np.int64)
        P = np.ascontiguousarray(params, dtype=np.float64)
        assert P.shape == (6,)
        nq = len(query_off) - 1
        width, lists, _keep = self._bm25_lists(nq, mode, ex_terms, ex_off, ph_terms, ph_off, nr_terms, nr_off, nr_window)
        args = [C.c_void_p(index), _ptr(terms) if len(terms) else None, _ptr(idf) if len(idf) else None, _ptr(query_off), nq, _ptr(P),
                1 if plus else 0, int(k)] + lists
        if d_ids is not None or d_scores is not None or d_counts is not None:
            self._check(getattr(self.lib, "gz_bm25_search%s_device" % width)(*args, C.c_void_p(d_ids), C.c_void_p(d_scores), C.c_void_p(d_counts)))
            return None
        kk = max(0, min(int(k), self.bm25_info(index)[0]))
        ids = np.empty((nq, kk), dtype=np.int64)
        scores = np.empty((nq, kk), dtype=np.float64)
        counts = np.zeros(max(nq, 1), dtype=np.int64)
        self._check(getattr(self.lib, "gz_bm25_search" + width)(*args, _ptr(ids) if ids.size else None, _ptr(scores) if scores.size else None,
                                                                 _ptr(counts)))
        return ids, scores, counts[:nq]

    # the search entry points by the widest list a call gives: every width takes the lists of the narrower ones before its own
    _BM25_WIDTHS = ("", "_bool", "_phrase", "_near")

    @classmethod
    def _bm25_lists(cls, nq: int, mode, ex_terms, ex_off, ph_terms, ph_off, nr_terms, nr_off, nr_window):
        """(suffix of the entry point, the C arguments between k and the outputs, the arrays behind them -- kept alive by the caller):
        near terms make it _near, else phrase terms _phrase, else a mode other than 0 or exclusions _bool, else the plain call"""
        n = 3 if nr_off is not None else 2 if ph_off is not None else 1 if mode != 0 or ex_off is not None else 0
        ex_terms, ex_off, ex = cls._bm25_exclusions(nq, ex_terms, ex_off)
        ph_terms, ph_off, ph = cls._bm25_exclusions(nq, ph_terms, ph_off)
        nr_terms, nr_off, nr_window, nr = cls._bm25_near(nq, nr_terms, nr_off, nr_window) if n == 3 else (None, None, None, [])
        args = [a for part in ([int(mode)] + ex, ph, nr)[:n] for a in part]
        return cls._BM25_WIDTHS[n], args, (ex_terms, ex_off, ph_terms, ph_off, nr_terms, nr_off, nr_window)

    @staticmethod
    def _bm25_exclusions(nq: int, ex_terms, ex_off):
        """the excluded terms of a boolean search as contiguous arrays (kept alive by the caller) and their two C arguments"""
        if ex_off is None:
            return None, None, [None, None]
        ex_off = np.ascontiguousarray(ex_off, dtype=np.int64)
        assert ex_off.shape == (nq + 1,)
        ex_terms = np.ascontiguousarray(ex_terms if ex_terms is not None else [], dtype=np.int32)
        return ex_terms, ex_off, [_ptr(ex_terms) if len(ex_terms) else None, _ptr(ex_off)]

    @staticmethod
    def _bm25_near(nq: int, nr_terms, nr_off, nr_window):
        """the near terms and windows of a near search as contiguous arrays (kept alive by the caller) and their three C arguments"""
        nr_terms, nr_off, nr = Context._bm25_exclusions(nq, nr_terms, nr_off)
        nr_window = np.ascontiguousarray(nr_window if nr_window is not None else [], dtype=np.int64)
        return nr_terms, nr_off, nr_window, nr + [_ptr(nr_window) if len(nr_window) else None]

    def bm25_match_count(self, index: int, terms: np.ndarray, query_off: np.ndarray, mode: int = 0, ex_terms=None,
                         ex_off=None, ph_terms=None, ph_off=None, nr_terms=None, nr_off=None, nr_window=None) -> np.ndarray:
        """int64 [Q]: the documents that match each query -- counts of bm25_search alone (mode, ex_terms, ex_off, ph_terms, ph_off as
        there; with mode 0 and ex_off None the call is gz_bm25_match_count, else gz_bm25_match_count_bool; with ph_off
        gz_bm25_match_count_phrase; with nr_off gz_bm25_match_count_near)."""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        query_off = np.ascontiguousarray(query_off, dtype=np.int64)
        nq = len(query_off) - 1
        counts = np.zeros(max(nq, 1), dtype=np.int64)
        width, lists, _keep = self._bm25_lists(nq, mode, ex_terms, ex_off, ph_terms, ph_off, nr_terms, nr_off, nr_window)
        self._check(getattr(self.lib, "gz_bm25_match_count" + width)(C.c_void_p(index), _ptr(terms) if len(terms) else None, _ptr(query_off), nq,
                                                                      *lists, _ptr(counts)))
        return counts[:nq]

    @staticmethod
    def _bm25_groups(alt_terms, alt_off, group_off):
        """the groups of a grouped search as contiguous arrays (kept alive by the caller): alternatives, their offsets per group,
        the groups' offsets per query"""
        alt_terms = np.ascontiguousarray(alt_terms, dtype=np.int32)
        alt_off = np.ascontiguousarray(alt_off, dtype=np.int64)
        group_off = np.ascontiguousarray(group_off, dtype=np.int64)
        assert alt_off.ndim == 1 and group_off.ndim == 1 and len(alt_off) >= 1 and len(group_off) >= 1
        return alt_terms, alt_off, group_off

    def bm25_search_groups(self, index: int, alt_terms: np.ndarray, alt_off: np.ndarray, group_idf: np.ndarray, group_off: np.ndarray,
                           params, plus: bool, k: int, mode: int = 0, ex_terms=None, ex_off=None, d_ids: int | None = None,
                           d_scores: int | None = None, d_counts: int | None = None):
        """bm25_search over word groups (gz_bm25_search_groups[_device]): query q = the groups group_off[q]:group_off[q + 1], group g =
        the alternatives alt_terms[alt_off[g]:alt_off[g + 1]] (-1 and repeats are ignored; at most 64 distinct) with idf group_idf[g].
        A group counts as one query word: matched by any alternative, f = the sum of their counts.  mode / ex_terms / ex_off and the
        outputs (or d_ids / d_scores / d_counts) as bm25_search."""
        alt_terms, alt_off, group_off = self._bm25_groups(alt_terms, alt_off, group_off)
        group_idf = np.ascontiguousarray(group_idf, dtype=np.float64)
        P = np.ascontiguousarray(params, dtype=np.float64)
        assert P.shape == (6,)
        nq = len(group_off) - 1
        ex_terms, ex_off, ex = self._bm25_exclusions(nq, ex_terms, ex_off)
        args = [C.c_void_p(index), _ptr(alt_terms) if len(alt_terms) else None, _ptr(alt_off), _ptr(group_idf) if len(group_idf) else None,
                _ptr(group_off), nq, _ptr(P), 1 if plus else 0, int(k), int(mode)] + ex
        if d_ids is not None or d_scores is not None or d_counts is not None:
            self._check(self.lib.gz_bm25_search_groups_device(*args, C.c_void_p(d_ids), C.c_void_p(d_scores), C.c_void_p(d_counts)))
            return None
        kk = max(0, min(int(k), self.bm25_info(index)[0]))
        ids = np.empty((nq, kk), dtype=np.int64)
        scores = np.empty((nq, kk), dtype=np.float64)
        counts = np.zeros(max(nq, 1), dtype=np.int64)
        self._check(self.lib.gz_bm25_search_groups(*args, _ptr(ids) if ids.size else None, _ptr(scores) if scores.size else None, _ptr(counts)))
        return ids, scores, counts[:nq]

    def bm25_match_count_groups(self, index: int, alt_terms: np.ndarray, alt_off: np.ndarray, group_off: np.ndarray, mode: int = 0,
                                ex_terms=None, ex_off=None) -> np.ndarray:
        """int64 [Q]: counts of bm25_search_groups alone (gz_bm25_match_count_groups)"""
        alt_terms, alt_off, group_off = self._bm25_groups(alt_terms, alt_off, group_off)
        nq = len(group_off) - 1
        counts = np.zeros(max(nq, 1), dtype=np.int64)
        ex_terms, ex_off, ex = self._bm25_exclusions(nq, ex_terms, ex_off)
        self._check(self.lib.gz_bm25_match_count_groups(C.c_void_p(index), _ptr(alt_terms) if len(alt_terms) else None, _ptr(alt_off),
                                                        _ptr(group_off), nq, int(mode), *ex, _ptr(counts)))
        return counts[:nq]

    @staticmethod
    def _bm25_pairs(terms, query_off, ids):
        """the packed query terms and the [Q, k] ids of a snippet call as contiguous arrays, and their leading C arguments"""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        query_off = np.ascontiguousarray(query_off, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        nq = len(query_off) - 1
        assert ids.ndim == 2 and ids.shape[0] == nq
        return terms, query_off, ids, nq, [_ptr(terms) if len(terms) else None, _ptr(query_off), nq, _ptr(ids) if ids.size else None, ids.shape[1]]

    def bm25_snippets(self, index: int, terms: np.ndarray, query_off: np.ndarray, ids: np.ndarray, width: int):
        """(starts int32 [Q, k], hits int32 [Q, k]) of a positional index: for every pair (query q, document ids[q, j]) the window
        of `width` words with the most query words in it -- the smallest start among the best, and the count; -1 / 0 for id -1
        (gz_bm25_snippets)."""
        terms, query_off, ids, nq, args = self._bm25_pairs(terms, query_off, ids)
        starts = np.empty(ids.shape, dtype=np.int32)
        hits = np.empty(ids.shape, dtype=np.int32)
        self._check(self.lib.gz_bm25_snippets(C.c_void_p(index), *args, int(width), _ptr(starts) if starts.size else None,
                                              _ptr(hits) if hits.size else None))
        return starts, hits

    def bm25_snippets_device(self, index: int, terms: np.ndarray, query_off: np.ndarray, d_ids: int, k: int, width: int, d_starts: int,
                             d_hits: int) -> None:
        """bm25_snippets with the ids (int64 [Q, k]) and both outputs (int32 [Q, k]) in device memory: what bm25_search wrote into
        d_ids goes straight in.  An id outside [-1, documents) counts as -1 (gz_bm25_snippets_device)."""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        query_off = np.ascontiguousarray(query_off, dtype=np.int64)
        self._check(self.lib.gz_bm25_snippets_device(C.c_void_p(index), _ptr(terms) if len(terms) else None, _ptr(query_off), len(query_off) - 1,
                                                     C.c_void_p(d_ids), int(k), int(width), C.c_void_p(d_starts), C.c_void_p(d_hits)))

    def bm25_occurrences(self, index: int, terms: np.ndarray, query_off: np.ndarray, ids: np.ndarray):
        """(positions int32 [T], words int32 [T], offsets int64 [Q * k + 1]) of a positional index: pair r = q * k + j owns
        [offsets[r], offsets[r + 1]) -- the positions in document ids[q, j] of the words of query q, ascending, and for each the
        first place of that term in the query (gz_bm25_occurrences: sizes first, then the fill)."""
        terms, query_off, ids, nq, args = self._bm25_pairs(terms, query_off, ids)
        off = np.zeros(ids.size + 1, dtype=np.int64)
        self._check(self.lib.gz_bm25_occurrences(C.c_void_p(index), *args, _ptr(off), None, None, 0))       # sizes first
        t = int(off[-1])
        pos = np.empty(max(t, 1), dtype=np.int32)
        word = np.empty(max(t, 1), dtype=np.int32)
        if t:
            self._check(self.lib.gz_bm25_occurrences(C.c_void_p(index), *args, _ptr(off), _ptr(pos), _ptr(word), t))
        return pos[:t], word[:t], off

    def bm25_cover(self, index: int, terms: np.ndarray, query_off: np.ndarray, ids: np.ndarray):
        """(starts, lengths, words), each int32 [Q, k], of a positional index: for every pair (query q, document ids[q, j]) the
        shortest window of the document that holds every term of the query which the document holds at all -- ties to the smallest
        start -- and how many distinct terms that is; (0, 0, 0) for a document with none, (-1, 0, 0) for id -1 (gz_bm25_cover)."""
        terms, query_off, ids, nq, args = self._bm25_pairs(terms, query_off, ids)
        out = [np.empty(ids.shape, dtype=np.int32) for _ in range(3)]
        self._check(self.lib.gz_bm25_cover(C.c_void_p(index), *args, *[_ptr(o) if o.size else None for o in out]))
        return tuple(out)

    def bm25_cover_device(self, index: int, terms: np.ndarray, query_off: np.ndarray, d_ids: int, k: int, d_starts: int, d_lengths: int,
                          d_words: int) -> None:
        """bm25_cover with the ids (int64 [Q, k]) and the three outputs (int32 [Q, k]) in device memory: what bm25_search wrote into
        d_ids goes straight in.  An id outside [-1, documents) counts as -1 (gz_bm25_cover_device)."""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        query_off = np.ascontiguousarray(query_off, dtype=np.int64)
        self._check(self.lib.gz_bm25_cover_device(C.c_void_p(index), _ptr(terms) if len(terms) else None, _ptr(query_off), len(query_off) - 1,
                                                  C.c_void_p(d_ids), int(k), C.c_void_p(d_starts), C.c_void_p(d_lengths), C.c_void_p(d_words)))

    def exchange_select(self, back: int):
        """Exchange operations issued from now on belong to the encode call `back` calls before the latest one."""
        self._check(self.lib.gz_exchange_select(self.handle, back))

    def compact_rows(self, d_rows, d_n_real, n_rows, row_len, d_out, bits: int = 32) -> int:
        """Rows without their padding, back to back, as int32 (bits=32) or uint16 (bits=16) entries; returns the count."""
        total = C.c_int64()
        fn = self.lib.gz_compact_rows16 if bits == 16 else self.lib.gz_compact_rows
        self._check(fn(self.handle, C.c_void_p(d_rows), C.c_void_p(d_n_real), n_rows, row_len, C.c_void_p(d_out), C.byref(total)))
        return total.value

    def expand_rows(self, d_compact, d_n_real, n_rows, row_len, d_ids, d_mask, bits: int = 32):
        fn = self.lib.gz_expand_rows16 if bits == 16 else self.lib.gz_expand_rows
        self._check(fn(self.handle, C.c_void_p(d_compact), C.c_void_p(d_n_real), n_rows, row_len, C.c_void_p(d_ids), C.c_void_p(d_mask)))

    def encode_emit_block(self, d_block, bits: int = 16):
        """Arms the next (dense) encode call to leave its exchange block in d_block as part of the call (0: disarm)."""
        self._check(self.lib.gz_encode_emit_block(self.handle, *_dptrs(d_block), bits))

    def block_total(self, back: int = 0) -> int:
        """Waits for the encode call `back` calls ago; the number of entries of the block it emitted."""
        total = C.c_int64()
        self._check(self.lib.gz_block_total(self.handle, back, C.byref(total)))
        return total.value

    def compact_block(self, d_rows, d_n_real, n_rows, row_len, d_block, bits: int = 16) -> int:
        """One rank's message of the exchange step: [int32 n_real[n_rows] | uint32 first[n_rows] | the rows' real entries, `bits`
        bits each] into d_block; returns the number of entries."""
        total = C.c_int64()
        self._check(self.lib.gz_compact_block(self.handle, C.c_void_p(d_rows), C.c_void_p(d_n_real), n_rows, row_len, bits,
                                              C.c_void_p(d_block), C.byref(total)))
        return total.value

    def expand_block(self, d_block, n_rows, row_len, d_ids, d_mask, bits: int = 16, total: int = 0xFFFFFFFF):
        """`total`: the entry count the block was announced with (block_total / compact_block on the sending side)."""
        self._check(self.lib.gz_expand_block(self.handle, C.c_void_p(d_block), bits, n_rows, row_len, int(total), C.c_void_p(d_ids), C.c_void_p(d_mask)))

    def gather_rows(self, d_send, n_rows_local, row_len, d_recv, rows_per_rank, root=0):
        rpr = np.ascontiguousarray(rows_per_rank, dtype=np.int64)
        self._check(self.lib.gz_gather_rows(self.handle, C.c_void_p(d_send), n_rows_local, row_len,
                                            *_dptrs(d_recv), _ptr(rpr), root))


class HostTables:
    """gz_host_tables: the loader + table builder run on the host only (no GPU).  Used by the CPU test-suite to
    check the integer tables the kernels consume, and by tools that want to inspect them."""

    _DT = {0: (np.uint32, 4), 1: (np.uint32, 4), 2: (np.int32, 2), 3: (np.uint32, 2), 4: (np.uint32, 4), 5: (np.int32, 1),
           6: (np.uint32, 2), 7: (np.uint16, 1), 8: (np.uint32, 1), 9: (np.uint32, 2)}

    def __init__(self, vocab: bytes, bpe: bytes, specials=("<pad>", "<s>", "</s>", "<mask>", "<unk>")):
        self.lib = load_library()
        self.handle = C.c_void_p()
        arr = (C.c_char_p * 5)(*[s.encode("utf-8", "surrogatepass") for s in specials])
        vb = C.create_string_buffer(vocab, len(vocab)) if vocab else None
        bb = C.create_string_buffer(bpe, len(bpe)) if bpe else None
        rc = self.lib.gz_host_tables_create(C.cast(vb, C.c_void_p) if vb else None, len(vocab),
                                            C.cast(bb, C.c_void_p) if bb else None, len(bpe), arr, C.byref(self.handle))
        if rc != GZ_OK:
            raise GzError(rc, self.lib.gz_last_error(None).decode("utf-8", "replace"))

    def array(self, which: int) -> np.ndarray:
        p, n = C.c_void_p(), C.c_int64()
        rc = self.lib.gz_host_tables_array(self.handle, which, C.byref(p), C.byref(n))
        if rc != GZ_OK:
            raise GzError(rc, "gz_host_tables_array")
        dt, w = self._DT[which]
        if n.value == 0:
            return np.zeros((0, w) if w > 1 else 0, dtype=dt)
        buf = (C.c_char * (n.value * w * np.dtype(dt).itemsize)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dt).copy()
        return a.reshape(n.value, w) if w > 1 else a

    def vocab_items(self):
        out, i = [], 0
        p, ln, idv = C.c_void_p(), C.c_int32(), C.c_int32()
        while self.lib.gz_host_tables_vocab_entry(self.handle, i, C.byref(p), C.byref(ln), C.byref(idv)) == GZ_OK:
            out.append((C.string_at(p, ln.value).decode("utf-8"), idv.value)); i += 1
        return out

    def merge_items(self):
        out, i = [], 0
        p, ln, nf, rk = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        while self.lib.gz_host_tables_merge_entry(self.handle, i, C.byref(p), C.byref(ln), C.byref(nf), C.byref(rk)) == GZ_OK:
            s = C.string_at(p, ln.value).decode("utf-8")
            out.append((tuple(s.split("\n")) if nf.value else (), rk.value)); i += 1
        return out

    def symbols(self):
        out, i = [], 0
        p, ln = C.c_void_p(), C.c_int32()
        while self.lib.gz_host_tables_symbol(self.handle, i, C.byref(p), C.byref(ln)) == GZ_OK:
            out.append(C.string_at(p, ln.value).decode("utf-8")); i += 1
        return out

    def close(self):
        if self.handle.value:
            self.lib.gz_host_tables_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
