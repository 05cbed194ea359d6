"""Loader for libatropos_hip.so (the C ABI in include/atropos_hip.h) and the
backend object the Python layer talks to.

There is exactly one product backend: the HIP library running on an MI355X.  If the
shared library has not been built, or no GPU is visible, every entry point raises --
there is no CPU fallback.  (The CPU test-suite injects a lock-step emulation of the
kernel built from the same per-lane source via ``set_backend``; that object lives
under tests/ and is never imported from here.)
"""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ATROPOS_HIP_LIB") or os.path.join(_HERE, "libatropos_hip.so")   # (override: kernel experiments)

ATR_OK = 0
ERRORS = {-1: "invalid argument", -2: "unsupported by the device kernels", -3: "HIP runtime error",
          -4: "out of memory", -5: "no HIP device"}
TABLE_DNA15, TABLE_ACGT, TABLE_IUPAC, TABLE_CUSTOM = 0, 1, 2, 3
MAX_REF_LEN = 128
MAX_READ_LEN = 736
MAX_LONG_READ_LEN = 32736                # Aligner.locate / locate_batch: reads up to here (the full sweep with a rolling origin base)
PLANES_MIN_READS = 65536                 # Aligner.pack: batches from here on are packed as bit planes when the two-pass
                                         # pre-pass takes the aligner (atr_locate_planes_batch)
WAVE_MAX_READS = 32768                   # atr_locate_batch: short batches take the wavefront-per-read kernel
LOCATE_PATHS = {"auto": 0, "full": 1, "filtered": 2, "wave": 3}   # ATR_LOCATE_* of include/atropos_hip.h
PAIRS_PATHS = {"auto": 0, "full": 1, "fast": 2, "wave": 3}        # ATR_PAIRS_*
PAIRS_MAX_LEN = 320
INSERT_MAX_ADAPTER = 128
INSERT_MAX_READ = 320


class InsertConfig(C.Structure):
    """atr_insert_config (include/atropos_hip.h)."""
    _fields_ = [
        ("adapter1", C.c_char_p), ("alen1", C.c_int),
        ("adapter2", C.c_char_p), ("alen2", C.c_int),
        ("insert_max_rmp", C.c_double), ("adapter_max_rmp", C.c_double),
        ("min_insert_overlap", C.c_int), ("max_insert_mismatch_frac", C.c_double),
        ("min_adapter_overlap", C.c_int), ("max_adapter_mismatch_frac", C.c_double),
        ("adapter_check_cutoff", C.c_int),
        ("adapter_wildcards", C.c_int), ("read_wildcards", C.c_int),
        ("rmp_insert", C.c_void_p), ("rmp_adapter", C.c_void_p), ("rmp_ld", C.c_int),
        ("max_mismatch_by_alen", C.c_void_p), ("n_mismatch", C.c_int),
    ]

class LinkedAdapterSpec(C.Structure):
    """atr_linked_adapter (include/atropos_hip.h)."""
    _fields_ = [
        ("front", C.c_void_p), ("back", C.c_void_p),
        ("front_exact_shortcut", C.c_int), ("back_exact_shortcut", C.c_int),
        ("d_front_rmp", C.c_void_p), ("d_back_rmp", C.c_void_p), ("front_rmp_ld", C.c_int), ("back_rmp_ld", C.c_int),
        ("front_max_rmp", C.c_double), ("back_max_rmp", C.c_double),
    ]


LINKED_MAX_ADAPTERS = 4


class STREAM(C.c_void_p):
    """The ``void *stream`` argument of an entry point: a hipStream_t as an integer (0: the null stream).  Where a
    prototype names it, ``_call`` supplies the current stream; the callers never pass one."""


# prototypes of every symbol include/atropos_hip.h declares
PROTOTYPES = {
    "atr_version": (C.c_int, []),
    "atr_device_count": (C.c_int, []),
    "atr_last_error": (C.c_char_p, []),
    "atr_translate_table": (C.c_int, [C.c_int, C.c_char_p]),
    "atr_packed_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "atr_pack_reads": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_char_p,
                                 C.c_void_p, C.c_void_p, STREAM]),
    "atr_planes_count_uncoded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, STREAM]),
    "atr_pack_planes": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_char_p,
                                  C.c_void_p, C.c_void_p, STREAM]),
    "atr_multi_locate_work_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "atr_multi_locate_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, STREAM]),
    "atr_compare_batch": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p, STREAM]),
    "atr_locate_debug_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "atr_locate_debug": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, STREAM]),
    "atr_compare_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, STREAM]),
    "atr_adapter_postfilter": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int,
                                         C.c_double, C.c_int, STREAM]),
    "atr_correct_errors_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_insert_correct_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                           C.c_void_p, C.c_void_p, STREAM]),
    "atr_insert_match_correct_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                                 C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_insert_aligner_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "atr_insert_aligner_destroy": (None, [C.c_void_p]),
    "atr_insert_match_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int, C.c_void_p, STREAM]),
    "atr_insert_match_batch_coded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_int, C.c_int, C.c_void_p, STREAM]),
    "atr_case_sensitive_table": (C.c_int, [C.c_char_p]),
    "atr_aligner_create": (C.c_int, [C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.POINTER(C.c_void_p)]),
    "atr_aligner_destroy": (None, [C.c_void_p]),
    "atr_aligner_set_min_overlap": (C.c_int, [C.c_void_p, C.c_int]),
    "atr_aligner_set_indel_cost": (C.c_int, [C.c_void_p, C.c_int]),
    "atr_aligner_query_table": (C.c_int, [C.c_void_p, C.c_char_p]),
    "atr_locate_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_locate_work_unresolved": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, STREAM, C.POINTER(C.c_int64)]),
    "atr_locate_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                   C.c_void_p, STREAM]),
    "atr_locate_ascii_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, STREAM]),
    "atr_locate_one": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, STREAM]),
    "atr_insert_match_one": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, STREAM]),
    "atr_multi_locate_one": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p, STREAM]),
    "atr_compare_one": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, STREAM]),
    "atr_locate_planes_applies": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "atr_aligner_prepare": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "atr_locate_ascii_planes_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, STREAM]),
    "atr_locate_planes_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, STREAM]),
    "atr_locate_batch_path": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_int, STREAM]),
    "atr_linked_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "atr_linked_destroy": (None, [C.c_void_p]),
    "atr_linked_query_table": (C.c_int, [C.c_void_p]),
    "atr_linked_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "atr_linked_match_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_linked_group_applies": (C.c_int, [C.c_void_p, C.c_int]),
    "atr_linked_group_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "atr_linked_group_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "atr_linked_group_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_char_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int64), C.c_void_p, STREAM]),
    "atr_linked_group_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_locate_pairs_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         STREAM]),
    "atr_locate_pairs_need_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, STREAM]),
    "atr_locate_pairs_path_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_int, C.c_void_p, STREAM]),
    "atr_locate_pairs_long_work_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "atr_locate_pairs_long_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, STREAM]),
    "atr_locate_pair_one": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, STREAM]),
    "atr_locate_pairs_full_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              STREAM]),
    "atr_fastq_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_fastq_count_lines": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, STREAM]),
    "atr_fastq_index": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p, STREAM]),
    "atr_pack_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_char_p,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_pair_filter_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, STREAM]),
    "atr_insert_plan_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_clip_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, STREAM]),
    "atr_quality_trim_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                         C.c_int, C.c_int, STREAM]),
    "atr_nend_trim_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, STREAM]),
    "atr_match_trim_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int64, STREAM]),
    "atr_read_filter_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, STREAM]),
    "atr_merge_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_merge_plan_batch": (C.c_int, [C.c_void_p] * 7 + [C.c_int64] + [C.c_void_p] * 4 + [STREAM]),
    "atr_merge_emit_batch": (C.c_int, [C.c_void_p] * 11 + [C.c_int64, C.c_int, C.c_int, C.c_char_p] + [C.c_void_p] * 4 + [STREAM]),
    "atr_fastq_emit_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_fastq_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_fasta_work_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "atr_fasta_scan": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, STREAM]),
    "atr_fasta_index": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                  C.c_void_p, C.c_void_p, STREAM]),
    "atr_fasta_emit_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_fasta_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_fastq_emit_pairs_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_fastq_emit_pairs": (C.c_int, [C.c_void_p] * 13 + [C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 3 + [STREAM]),
    "atr_overwrite_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_overwrite_plan_batch": (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
                                 + [STREAM]),
    "atr_overwrite_apply_batch": (C.c_int, [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_char_p,
                                                                                            C.c_void_p, STREAM]),
    "atr_fastq_emit_grouped_work_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "atr_fastq_emit_grouped": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 4 + [STREAM]),
    "atr_demux_groups": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int64, C.c_void_p, STREAM]),
    "atr_read_stats_bytes": (C.c_int64, [C.c_int]),
    "atr_read_stats_clear": (C.c_int, [C.c_void_p, C.c_int, STREAM]),
    "atr_read_stats_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
                             + [C.c_int, C.c_int64, C.c_int64, STREAM]),
    "atr_read_stats_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, STREAM]),
    "atr_detect_create": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.POINTER(C.c_void_p)]),
    "atr_detect_destroy": (None, [C.c_void_p]),
    "atr_detect_counter_bytes": (C.c_int64, [C.c_void_p]),
    "atr_detect_clear": (C.c_int, [C.c_void_p, C.c_void_p, STREAM]),
    "atr_detect_filter_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, STREAM]),
    "atr_detect_mark_batch": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p, STREAM]),
    "atr_detect_batch": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, STREAM]),
    "atr_detect_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_detect_kmer_slots": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 3 + [STREAM]),
    "atr_detect_kmer_pair_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_int, C.c_void_p, STREAM]),
    "atr_detect_kmer_rank_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_detect_kmer_rank": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 6 + [C.c_size_t, STREAM]),
    "atr_detect_kmer_level": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 7 + [C.c_int, C.c_int64, C.c_void_p,
                                                                                     C.c_void_p, C.c_int64, C.c_void_p, STREAM]),
    "atr_detect_kmer_next": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [STREAM]),
    "atr_detect_kmer_gather": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, STREAM]),
    "atr_detect_kmer_support": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, STREAM]),
    "atr_report_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "atr_report_destroy": (None, [C.c_void_p]),
    "atr_report_counters": (C.c_int64, [C.c_void_p]),
    "atr_report_intervals": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, STREAM]),
    "atr_report_adapters": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, STREAM]),
    "atr_report_outputs": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, STREAM]),
    "atr_report_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, STREAM]),
    "atr_gzip_bound": (C.c_int64, [C.c_int64]),
    "atr_gzip_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_gzip_eof": (C.c_int, [C.c_void_p]),
    "atr_gzip_blocks": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [STREAM]),
    "atr_bgzf_scan": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "atr_gunzip_members": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 2 + [STREAM]),
    "atr_gunzip_stream_workspace": (C.c_int64, [C.c_int64] * 3),
    "atr_gunzip_stream": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.c_void_p, C.c_int64, C.c_void_p, STREAM]),
    "atr_bam_header": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "atr_bam_walk_workspace": (C.c_int64, [C.c_int64] * 2),
    "atr_bam_walk": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_void_p, C.c_int64, STREAM]),
    "atr_bam_to_fastq_work_bytes": (C.c_size_t, [C.c_int64]),
    "atr_bam_to_fastq": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 4 + [STREAM]),
}
# atr_gunzip_stream: the words of d_result, the two statuses that ask for a larger slab / more room (the others: INF_E_*)
GUNZIP_STREAM_WORDS = ("status", "end_bit", "text_len", "final_seen", "crc_out", "chunks", "confirmed", "redecoded")
GUNZIP_NEED_INPUT, GUNZIP_NEED_ROOM = 101, 102
GUNZIP_STREAM_MAX = (1 << 28) - 1        # bytes of one slab
GZIP_BLOCK = 65280                       # atr_gzip_blocks: bytes of text per BGZF member
GUNZIP_MAX_MEMBERS = 1 << 22             # atr_gunzip_members: members of one call (ATR_GUNZIP_MAX_MEMBERS)
GZIP_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # atr_gzip_eof
DETECT_MAX_READ = 320                    # atr_detect_*: reads up to here (the complexity table is (len + 1)^2 doubles)
DETECT_HDR = 8                           # detect_core.hpp: kept, distinct, invalid, overlong, then 4 x nseq counters
# atr_detect_kmer_* (detect_kmer_core.hpp): the envelope, the words of a candidate row and of the state block
KMER_MIN_K, KMER_MAX_K, KMER_MAX_SLOTS, KMER_MAX_CANDIDATES, KMER_MAX_PATTERNS = 4, 32, (1 << 31) - 1, 1 << 20, 64
KMER_C_LEVEL, KMER_C_COUNT, KMER_C_REP, KMER_C_OFFSET, KMER_C_QUIRK, KMER_C_WORDS = 0, 1, 2, 3, 4, 5
KMER_S_CANDIDATES, KMER_S_SURVIVORS, KMER_S_OVER, KMER_S_WORDS = 0, 1, 8, 330
KMER_NO_KEY = (1 << 63) - 1

# atr_report_*: the words of the counter block (report_core.hpp), the counting modes of a trimmer stage, the variants
REPORT_IN_RECORDS, REPORT_IN_BASES, REPORT_WITH_ADAPTERS, REPORT_OVERFLOW = 0, 1, 2, 3
REPORT_DEST, REPORT_DEST_BP, REPORT_TRIM, REPORT_HDR, REPORT_ADJ = 8, 16, 24, 32, 8
REPORT_SUBSEQ, REPORT_CLIP, REPORT_MINCUT, REPORT_NEND = 0, 1, 2, 3
REPORT_MAX_WORDS = 1 << 22                # report_core.hpp: the bound of a counter block (32 MiB)
REPORT_VARIANTS = {"auto": 0, "lds": 1, "global": 2}

FASTQ_ERR_AT, FASTQ_ERR_PLUS, FASTQ_ERR_NAME2, FASTQ_ERR_LENGTH = 1, 2, 3, 4
FASTA_ERR_HEADER = 1
# atr_bam_*: the result words of the walk and of the decode, their error kinds, the statuses, the product's sizes
BAM_WALK_WORDS = ("count", "consumed", "error", "repaired")
BAM_DECODE_WORDS = ("text_bytes", "error", "records")
BAM_NEED_MORE = 1
BAM_ERR_SMALL, BAM_ERR_BIG, BAM_ERR_LSEQ, BAM_ERR_TRUNCATED = 1, 2, 3, 4
BAM_REC_LSEQ0, BAM_REC_QUAL, BAM_REC_NAME, BAM_REC_PAIR_NAME, BAM_REC_PAIR_FLAGS = 1, 2, 3, 4, 5
BAM_TILE = 8192                          # atr_bam_walk: bytes per speculative tile (some 30 records of 150 bases)
BAM_MAX_BLOCK = 64 << 20                 # the largest block_size: a record must fit a reader's carry (ChunkedFastqReader.RESERVE)
DEST_KEEP, DEST_TOO_SHORT, DEST_TOO_LONG, DEST_TOO_MANY_N, DEST_TRIMMED, DEST_UNTRIMMED = range(6)
INT64_MAX = (1 << 63) - 1
EMIT_MAX_GROUPS = 1024                   # atr_fastq_emit_grouped: outputs per call


class AtroposHipError(RuntimeError):
    pass


class AtroposUnsupported(AtroposHipError):
    """ATR_ERR_UNSUPPORTED: the request is outside the device kernels' envelope."""


def attach_prototypes(lib, prefix="atr_", only=None):
    """Give the symbols of ``lib`` the restype / argtypes of PROTOTYPES; ``{atr_ name: (function, stream position or
    None)}``.  The CPU test-suite attaches the same prototypes to the kernels' CPU twins, which export ``emu_x`` with
    ``atr_x``'s signature (``prefix``, ``only``: the names one twin library stands in for)."""
    fns = {}
    for name in PROTOTYPES if only is None else only:
        res, args = PROTOTYPES[name]
        fn = getattr(lib, prefix + name[4:])   # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
        fns[name] = (fn, args.index(STREAM) if STREAM in args else None)
    return fns


def load_library(path=LIB_PATH):
    """dlopen the C-ABI library and attach prototypes.  Raises if it is missing."""
    if not os.path.exists(path):
        raise AtroposHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C atropos_amd/csrc`). There is no CPU fallback." % path)
    lib = C.CDLL(path)
    attach_prototypes(lib)
    return lib


def _check(lib, rc, what):
    if rc is None or rc >= 0:              # (None: a void function)
        return rc
    if rc == -1:
        raise ValueError("%s: invalid argument" % what)
    if rc == -4:
        raise MemoryError(what)
    detail = ERRORS.get(rc, "error %d" % rc)
    if rc == -2:
        raise AtroposUnsupported("%s: %s" % (what, detail))
    if rc == -3 and lib is not None:
        detail += ": " + (lib.atr_last_error() or b"").decode("ascii", "replace")
    raise AtroposHipError("%s: %s" % (what, detail))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bgzf_scan(fn, buf, lo, hi, max_members):
    # (the arguments are checked here, so that the function's ATR_ERR_INVALID can only mean "not a BGZF header")
    lo, hi, max_members = int(lo), int(hi), int(max_members)
    if (not isinstance(buf, torch.Tensor) or buf.device.type != "cpu" or buf.dtype != torch.uint8 or not buf.is_contiguous()
            or not 0 <= lo <= hi <= buf.numel() or max_members < 0):
        raise ValueError("bgzf_scan: a contiguous uint8 host tensor, 0 <= lo <= hi <= its size and max_members >= 0 are needed")
    member_at = torch.zeros((int(max_members) + 1,), dtype=torch.int64)
    text_at = torch.zeros((int(max_members) + 1,), dtype=torch.int64)
    k, covered = C.c_int64(0), C.c_int64(0)
    rc = fn(C.c_void_p(buf.data_ptr() + int(lo)), C.c_int64(int(hi) - int(lo)), C.c_int64(int(max_members)), _ptr(member_at),
            _ptr(text_at), C.byref(k), C.byref(covered))
    if rc not in (0, -1):
        raise AtroposHipError("atr_bgzf_scan: error %d" % rc)
    return member_at, text_at, int(k.value), int(covered.value), rc == 0


class _PinnedUpload(object):
    """What HipBackend.stage_host_bytes hands to ReadBatch.from_ascii: `.to(device)` starts the DMA from the page-locked
    buffer and records the event the next staging waits for."""

    def __init__(self, host, backend):
        self.host, self.backend = host, backend
        self.dtype, self.shape = host.dtype, host.shape

    def dim(self):
        return self.host.dim()

    def to(self, device):
        dev = self.host.to(device, non_blocking=True)
        self.backend._pinned_event.record(torch.cuda.current_stream(self.backend.device))
        return dev


class LinkedGroups(object):
    """What atr_linked_group_pack leaves on the device for one batch: the per-adapter plane64 sub-batches of
    read[front.rstop:] (``grouped``, ``glens``), the permutation (``perm`` slot -> read, ``slot_of`` read -> slot), the 5'
    results (``which``, ``front``), the host ``info`` block (reads and first tile of every group) and the workspace."""
    __slots__ = ("nreads", "max_len", "grouped", "glens", "perm", "slot_of", "which", "front", "info", "work")

    def group_reads(self):
        return [int(self.info[g]) for g in range(LINKED_MAX_ADAPTERS)]


class AbiCalls(object):
    """The wrappers of the C ABI that every backend serves: ``HipBackend`` below and the CPU test-suite's stand-in, whose
    library exports the kernels' CPU twins under the same signatures.  A subclass supplies

      ``device``            where the tensors of a call live,
      ``empty(shape, dtype)``  an output buffer there,
      ``_call(name, *args)``   calls entry point ``name`` (its ``atr_`` name) on the current device and stream -- the
                            stream argument is the subclass's to add, where PROTOTYPES names one -- and raises on an
                            error code; returns the code otherwise,
      ``_host(name, *args)``   the same for the entry points that touch no device,
      ``_symbol(name)``        the bare ctypes function,
      ``_workspace(need, first=0)``  the kernels' scratch of at least ``need`` bytes, kept between calls (``first``: the
                            size of a new one when none is kept yet)."""

    def translate_table(self, kind):
        buf = C.create_string_buffer(256)
        self._host("atr_translate_table", kind, buf)
        return buf.raw

    def packed_bytes(self, nreads, max_len):
        return self._host("atr_packed_bytes", nreads, max_len)

    def pack_reads(self, ascii_2d, lens, max_len, table, count_invalid=False, starts=None, planes=False):
        """ascii_2d: uint8 [nreads, >=max_len] on self.device (row stride arbitrary);
        lens: int32 [nreads] or None; starts: int32 [nreads] or None (pack read[start:]);
        table: 256 bytes; planes: plane64 layout (the insert aligner's) instead of tile64.
        Returns the packed uint8 tensor (and, with count_invalid, the number of reads
        holding a byte the table maps to 0)."""
        nreads = ascii_2d.shape[0]
        packed = self.empty((max(self.packed_bytes(nreads, max_len), 16),), torch.uint8)
        invalid = torch.zeros((1,), dtype=torch.int32, device=self.device) if count_invalid else None
        if nreads and max_len:
            self._call("atr_pack_planes" if planes else "atr_pack_reads", _ptr(ascii_2d), ascii_2d.stride(0), _ptr(lens),
                       _ptr(starts), nreads, max_len, table, _ptr(packed), _ptr(invalid))
        return (packed, int(invalid.item())) if count_invalid else packed

    def planes_count_uncoded(self, planes, lens, other_lens, nreads, max_len):
        """Number of reads of a plane64 buffer with an uncoded base among their first
        min(lens, other_lens) bases (atr_planes_count_uncoded); either lens may be None (max_len)."""
        count = torch.zeros((1,), dtype=torch.int32, device=self.device)
        if nreads and max_len:
            self._call("atr_planes_count_uncoded", _ptr(planes), _ptr(lens), _ptr(other_lens), nreads, max_len, _ptr(count))
        return int(count.item())

    def multi_locate_batch(self, refs, ref_lens, queries, query_lens, e, flags, min_overlap, max_matches,
                           max_ref_len, out_stride):
        """refs/queries: uint8 [npairs, width] raw ASCII on the device; returns
        (records int16 [npairs, out_stride, 8], counts int32 [npairs])."""
        npairs = refs.shape[0]
        out = self.empty((npairs, out_stride, 8), torch.int16)
        counts = self.empty((npairs,), torch.int32)
        work = self.empty((max(self._host("atr_multi_locate_work_bytes", npairs, max_ref_len), 4),), torch.uint8)
        if npairs:
            self._call("atr_multi_locate_batch", _ptr(refs), refs.stride(0), _ptr(ref_lens), _ptr(queries), queries.stride(0),
                       _ptr(query_lens), npairs, e, flags, min_overlap, max_matches, max_ref_len, _ptr(work), _ptr(out),
                       _ptr(counts), out_stride)
        return out, counts

    def compare_batch(self, ref, queries, lens, max_len, wildcard_ref, wildcard_query, suffix):
        """ref: bytes; queries: uint8 [n, width] raw ASCII on the device."""
        n = queries.shape[0]
        out = self.empty((n, 8), torch.int16)
        if n:
            self._call("atr_compare_batch", ref, len(ref), _ptr(queries), queries.stride(0), _ptr(lens), n, max_len,
                       int(wildcard_ref), int(wildcard_query), int(suffix), _ptr(out))
        return out

    def adapter_postfilter(self, records, m, min_overlap, max_error_rate, rmp, max_rmp, accept_full):
        """In-place acceptance test of Adapter.match_to on int16 [n, 8] records; rmp: float64
        [ld, ld] device tensor or None."""
        if records.shape[0]:
            self._call("atr_adapter_postfilter", _ptr(records), records.shape[0], m, min_overlap, max_error_rate, _ptr(rmp),
                       0 if rmp is None else rmp.shape[1], 0.0 if max_rmp is None else max_rmp, int(accept_full))
        return records

    def correct_errors_batch(self, seq1, qual1, lens1, seq2, qual2, lens2, insert, mask, action, min_qual_diff,
                             truncate, comp):
        """In-place error correction of the overlaps (uint8 [n, width] ASCII tensors on
        the device, same row stride); returns (changed int32 [n, 2], newlen int32 [n, 2])."""
        n = seq1.shape[0]
        changed = self.empty((n, 2), torch.int32)
        newlen = self.empty((n, 2), torch.int32)
        if n:
            if seq1.stride(0) != seq2.stride(0):
                raise ValueError("both reads need the same row stride")
            self._call("atr_correct_errors_batch", _ptr(seq1), _ptr(qual1), _ptr(lens1), _ptr(seq2), _ptr(qual2), _ptr(lens2),
                       seq1.stride(0), _ptr(insert), _ptr(mask), n, seq1.shape[1], action, min_qual_diff, int(truncate), comp,
                       _ptr(changed), _ptr(newlen))
        return changed, newlen

    def insert_correct_batch(self, records, seq1, qual1, lens1, seq2, qual2, lens2, action, min_qual_diff, comp,
                             changed=None, newlen=None, planes1=None, planes2=None):
        """Error correction of the pairs whose insert match (records of insert_match_batch) has
        errors, in place on uint8 [n, width] ASCII tensors; returns (changed, newlen) int32 [n, 2].
        planes1 / planes2: the plane64 ReadBatches the records were computed from (optional; the
        kernel then only visits the positions where the reads disagree)."""
        n = seq1.shape[0]
        changed = self.empty((n, 2), torch.int32) if changed is None else changed
        newlen = self.empty((n, 2), torch.int32) if newlen is None else newlen
        if n:
            if seq1.stride(0) != seq2.stride(0):
                raise ValueError("both reads need the same row stride")
            self._call("atr_insert_correct_batch", _ptr(records), None if planes1 is None else _ptr(planes1.packed),
                       None if planes2 is None else _ptr(planes2.packed), 0 if planes1 is None else planes1.max_len,
                       _ptr(seq1), _ptr(qual1), _ptr(lens1), _ptr(seq2), _ptr(qual2), _ptr(lens2), seq1.stride(0), n,
                       seq1.shape[1], action, min_qual_diff, comp, _ptr(changed), _ptr(newlen))
        return changed, newlen

    def insert_aligner_create(self, cfg):
        h = C.c_void_p()
        self._call("atr_insert_aligner_create", C.addressof(cfg), C.byref(h))
        return h

    def insert_aligner_destroy(self, h):
        self._host("atr_insert_aligner_destroy", h)

    def insert_match_batch(self, h, packed1, lens1, packed2, lens2, npairs, max_len, cased=False):
        """cased: both reads are packed with ``case_sensitive_table()`` (soft-masked reads)."""
        out = self.empty((npairs, 3, 8), torch.int16)
        if npairs:
            self._call("atr_insert_match_batch_coded", h, _ptr(packed1), _ptr(lens1), _ptr(packed2), _ptr(lens2), npairs, max_len,
                       1 if cased else 0, _ptr(out))
        return out

    def case_sensitive_table(self):
        buf = C.create_string_buffer(256)
        self._host("atr_case_sensitive_table", buf)
        return buf.raw

    def aligner_create(self, ref, e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost):
        h = C.c_void_p()
        self._host("atr_aligner_create", ref, len(ref), e, flags, int(wildcard_ref), int(wildcard_query), min_overlap,
                   indel_cost, C.byref(h))
        return h

    def aligner_destroy(self, h):
        self._host("atr_aligner_destroy", h)

    def aligner_set_min_overlap(self, h, v):
        self._host("atr_aligner_set_min_overlap", h, v)

    def aligner_set_indel_cost(self, h, v):
        self._host("atr_aligner_set_indel_cost", h, v)

    def aligner_query_table(self, h):
        buf = C.create_string_buffer(256)
        kind = self._host("atr_aligner_query_table", h, buf)
        return kind, buf.raw

    def locate_batch(self, h, packed, lens, nreads, max_len, filtered=True, path=None):
        """path: one of LOCATE_PATHS ("auto": the fastest applicable kernels -- a wavefront per read for short
        batches, the filtered pipeline (bit-parallel pre-pass + windowed DP) for long ones; "full", "filtered",
        "wave": that kernel family); the records are identical on every path.  ``filtered=False`` is "full"."""
        if path is None:
            path = "auto" if filtered else "full"
        code = LOCATE_PATHS[path]
        out = self.empty((nreads, 8), torch.int16)
        if nreads:
            work = None
            if code in (0, 2) and (code == 2 or nreads > WAVE_MAX_READS):
                work = self._workspace(self._host("atr_locate_work_bytes", nreads))
            elif code == 0:
                # short batches that do not take the wave kernel: references of more than 64 bases never use the
                # scratch, anchored prefixes only need it to be there
                work = self._workspace(0, first=self._host("atr_locate_work_bytes", WAVE_MAX_READS))
            self._call("atr_locate_batch_path", h, _ptr(packed), _ptr(lens), nreads, max_len, _ptr(out), _ptr(work), code)
        return out

    def locate_planes_applies(self, h, max_len, ragged=False):
        """Is this aligner on reads of max_len bases (ragged: of at most max_len) inside the envelope of the
        two-pass pre-pass (plane64 reads, atr_locate_planes_batch)?"""
        return bool(self._host("atr_locate_planes_applies", h, int(max_len), int(bool(ragged))))

    def locate_planes_batch(self, h, planes, lens, nreads, max_len):
        """Batched locate on a plane64 batch (atr_locate_planes_batch); lens None: equal-length reads."""
        out = self.empty((nreads, 8), torch.int16)
        if nreads:
            work = self._workspace(self._host("atr_locate_work_bytes", nreads))
            self._call("atr_locate_planes_batch", h, _ptr(planes), _ptr(lens), nreads, max_len, _ptr(out), _ptr(work))
        return out

    # -- linked adapters (one fused pipeline for the whole set) ---------------------
    def linked_create(self, specs):
        """specs: list of LinkedAdapterSpec.  Returns the set handle; AtroposHipError
        ("unsupported") when the set is outside the fused kernels' envelope."""
        arr = (LinkedAdapterSpec * len(specs))(*specs)
        h = C.c_void_p()
        self._call("atr_linked_create", C.addressof(arr), len(specs), C.byref(h))
        return h

    def linked_destroy(self, h):
        self._host("atr_linked_destroy", h)

    def linked_match_batch(self, h, packed, lens, nreads, max_len):
        """(which int8 [n, 2] = (first matching adapter | -1, number of matching 5' parts),
        front int16 [n, 8], back int16 [n, 8]) -- include/atropos_hip.h, atr_linked_match_batch."""
        which = self.empty((nreads, 2), torch.int8)
        front = self.empty((nreads, 8), torch.int16)
        back = self.empty((nreads, 8), torch.int16)
        if nreads:
            work = self._workspace(self._host("atr_linked_work_bytes", h, nreads))
            self._call("atr_linked_match_batch", h, _ptr(packed), _ptr(lens), nreads, max_len, _ptr(which), _ptr(front),
                       _ptr(back), _ptr(work))
        return which, front, back

    def locate_debug(self, h, packed, m, n):
        """atr_locate_debug: (cost matrix int32 [m + 1, n + 1] on the host, INT32_MIN = not computed; the record)."""
        work = self.empty((max(self._host("atr_locate_debug_bytes", h, n), 16),), torch.uint8)
        out = self.empty((1, 8), torch.int16)
        self._call("atr_locate_debug", h, _ptr(packed), n, _ptr(work), _ptr(out))
        cells = (m + 1) * (n + 1)
        return work[:4 * cells].view(torch.int32).reshape(m + 1, n + 1).cpu(), out.cpu()

    def compare_packed(self, h, packed, lens, nreads, max_len, suffix):
        """atr_compare_packed: compare_prefixes / compare_suffixes of aligner ``h``'s reference against
        reads packed for it.  int16 [nreads, 8]."""
        out = self.empty((nreads, 8), torch.int16)
        if nreads:
            self._call("atr_compare_packed", h, _ptr(packed), _ptr(lens), nreads, max_len, int(suffix), _ptr(out))
        return out

    def locate_pairs_batch(self, ref_packed, ref_lens, ref_max_len, revcomp_ref, query_packed, query_lens,
                           query_max_len, npairs, e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost,
                           need=None, path="auto"):
        """Aligner.locate with a per-pair reference; both sides tile64-packed.  int16 [npairs, 8].
        need: int32 [npairs] or None -- alignments with fewer matches may come back as None
        (atr_locate_pairs_need_batch).  path: PAIRS_PATHS ("auto": a wavefront per pair for short batches, the
        cost / threat / band pipeline or the full sweep for long ones; "full", "fast", "wave": that family)."""
        out = self.empty((npairs, 8), torch.int16)
        self._call("atr_locate_pairs_path_batch", _ptr(ref_packed), _ptr(ref_lens), ref_max_len, int(revcomp_ref),
                   _ptr(query_packed), _ptr(query_lens), query_max_len, npairs, e, flags, int(wildcard_ref),
                   int(wildcard_query), min_overlap, indel_cost, _ptr(need), PAIRS_PATHS[path], _ptr(out))
        return out

    def locate_pairs_long_batch(self, ref_packed, ref_lens, ref_max_len, revcomp_ref, query_packed, query_lens,
                                query_max_len, npairs, e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost):
        """Pairs with a side beyond PAIRS_MAX_LEN (atr_locate_pairs_long_batch: 64-bit cells, the DP column in a
        workspace allocated here).  The caller keeps npairs * ref_max_len small (PairAligner chunks)."""
        out = self.empty((npairs, 8), torch.int16)
        if npairs:
            work = self.empty((max(self._host("atr_locate_pairs_long_work_bytes", npairs, ref_max_len), 16),), torch.uint8)
            self._call("atr_locate_pairs_long_batch", _ptr(ref_packed), _ptr(ref_lens), ref_max_len, int(revcomp_ref),
                       _ptr(query_packed), _ptr(query_lens), query_max_len, npairs, e, flags, int(wildcard_ref),
                       int(wildcard_query), min_overlap, indel_cost, _ptr(out), _ptr(work))
        return out

    def locate_pairs_full_batch(self, ref_packed, ref_lens, ref_max_len, revcomp_ref, query_packed, query_lens,
                                query_max_len, npairs, e, flags, min_overlap, indel_cost):
        """The same records by the full-matrix sweep alone (atr_locate_pairs_full_batch)."""
        out = self.empty((npairs, 8), torch.int16)
        self._call("atr_locate_pairs_full_batch", _ptr(ref_packed), _ptr(ref_lens), ref_max_len, int(revcomp_ref),
                   _ptr(query_packed), _ptr(query_lens), query_max_len, npairs, e, flags, 0, 0, min_overlap, indel_cost,
                   _ptr(out))
        return out

    # -- device-resident FASTQ batch --------------------------------------------
    def fastq_index(self, data, nbytes):
        """data: uint8 device tensor holding nbytes of FASTQ text (16-byte aligned, readable up
        to the next multiple of 16).  Returns (records uint32 [nrec, 8], nlines, error word)."""
        work = self.empty((max(self._host("atr_fastq_work_bytes", nbytes), 16),), torch.uint8)
        info = self.empty((2,), torch.int64)
        self._call("atr_fastq_count_lines", _ptr(data), nbytes, _ptr(work), _ptr(info))
        nlines = int(info[0].item())
        line_ends = self.empty((max(nlines, 1),), torch.int32)
        records = self.empty((nlines // 4, 8), torch.int32)
        self._call("atr_fastq_index", _ptr(data), nbytes, _ptr(work), _ptr(line_ends), nlines, _ptr(records),
                   C.c_void_p(info.data_ptr() + 8))
        return records, line_ends, nlines, int(info[1].item())

    def pack_records(self, data, records, begin, end, max_len, table, count_invalid=False, planes=False):
        n = records.shape[0]
        packed = self.empty((max(self.packed_bytes(n, max_len), 16),), torch.uint8)
        lens = self.empty((n,), torch.int32)
        invalid = torch.zeros((1,), dtype=torch.int32, device=self.device) if count_invalid else None
        if n:
            self._call("atr_pack_records", _ptr(data), _ptr(records), _ptr(begin), _ptr(end), n, max_len, table, int(planes),
                       _ptr(packed), _ptr(lens), _ptr(invalid))
        return (packed, lens, int(invalid.item())) if count_invalid else (packed, lens)

    def clip_batch(self, records, begin, end, front, back):
        self._call("atr_clip_batch", _ptr(records), _ptr(begin), _ptr(end), begin.shape[0], front, back)

    def quality_trim_batch(self, data, records, begin, end, cutoff_front, cutoff_back, base, nextseq):
        self._call("atr_quality_trim_batch", _ptr(data), _ptr(records), _ptr(begin), _ptr(end), begin.shape[0], cutoff_front,
                   cutoff_back, base, int(nextseq))

    def nend_trim_batch(self, data, records, begin, end, ubegin=None, uend=None):
        self._call("atr_nend_trim_batch", _ptr(data), _ptr(records), _ptr(begin), _ptr(end), _ptr(ubegin), _ptr(uend),
                   begin.shape[0])

    def match_trim_batch(self, matches, front, default_front, begin, end, active, matched):
        self._call("atr_match_trim_batch", _ptr(matches), _ptr(front), default_front, _ptr(begin), _ptr(end), _ptr(active),
                   _ptr(matched), begin.shape[0])

    def read_filter_batch(self, data, records, begin, end, ubegin, uend, matched, min_len, max_len, max_n,
                          discard_trimmed, discard_untrimmed, masks=False):
        """The destination byte per read, or (masks=True) the bit mask of the filters that fire."""
        out = self.empty((begin.shape[0],), torch.uint8)
        self._call("atr_read_filter_batch", _ptr(data), _ptr(records), _ptr(begin), _ptr(end), _ptr(ubegin), _ptr(uend),
                   _ptr(matched), begin.shape[0], min_len, max_len, max_n, int(discard_trimmed), int(discard_untrimmed),
                   None if masks else _ptr(out), _ptr(out) if masks else None)
        return out

    def pair_filter_batch(self, mask1, mask2, min_affected):
        dest = self.empty((mask1.shape[0],), torch.uint8)
        self._call("atr_pair_filter_batch", _ptr(mask1), _ptr(mask2), mask1.shape[0], min_affected, _ptr(dest))
        return dest

    def insert_plan_batch(self, insert, fb1, fb2, batch1, batch2, begin1, end1, begin2, end2, uend1, uend2,
                          min_insert_len, symmetric, trim_action, correct_action=-1, min_qual_difference=1, comp=None):
        """InsertAdapterCutter's decision logic (+ optional in-place error correction of the two
        FASTQ chunks).  Returns (matched1, matched2, corrected int32 [n, 2], error word)."""
        n = begin1.shape[0]
        m1, m2 = self.empty((n,), torch.uint8), self.empty((n,), torch.uint8)
        corrected = self.empty((n, 2), torch.int32)
        err = self.empty((1,), torch.int64)
        self._call("atr_insert_plan_batch", _ptr(insert), _ptr(fb1), _ptr(fb2), _ptr(batch1.data), _ptr(batch1.records),
                   _ptr(batch2.data), _ptr(batch2.records), _ptr(begin1), _ptr(end1), _ptr(begin2), _ptr(end2), _ptr(uend1),
                   _ptr(uend2), n, min_insert_len, int(symmetric), trim_action, correct_action, min_qual_difference, comp,
                   _ptr(m1), _ptr(m2), _ptr(corrected), _ptr(err))
        return m1, m2, corrected, int(err.item())

    def merge_batch(self, align, need, insert_matched, batch1, batch2, begin1, end1, begin2, end2, correct_action=-1,
                    min_qual_difference=1, comp=None):
        """MergeOverlapping after the alignments (atr_merge_plan_batch + atr_merge_emit_batch): returns
        (kind uint8 [n] -- 0: the pair stays a pair --, the FASTQ text of the merged reads in input order,
        corrected int32 [n, 2], error word).  With a mismatch action the two chunks are corrected in place."""
        n = begin1.shape[0]
        kind = self.empty((n,), torch.uint8)
        offsets = self.empty((n + 1,), torch.int64)
        corrected = self.empty((n, 2), torch.int32)
        corrected.zero_()
        err = self.empty((1,), torch.int64)
        work = self.empty((max(self._host("atr_merge_work_bytes", n), 16),), torch.uint8)
        self._call("atr_merge_plan_batch", _ptr(align), _ptr(need), _ptr(batch1.records), _ptr(begin1), _ptr(end1),
                   _ptr(begin2), _ptr(end2), n, _ptr(kind), _ptr(offsets), _ptr(work), _ptr(err))
        total = int(offsets[n].item())
        out = self.empty((max(total, 1),), torch.uint8)
        if total and int(err.item()) == INT64_MAX:
            self._call("atr_merge_emit_batch", _ptr(align), _ptr(kind), _ptr(insert_matched), _ptr(batch1.data),
                       _ptr(batch1.records), _ptr(batch2.data), _ptr(batch2.records), _ptr(begin1), _ptr(end1), _ptr(begin2),
                       _ptr(end2), n, correct_action, min_qual_difference, comp, _ptr(offsets), _ptr(corrected), _ptr(err),
                       _ptr(out))
        return kind, out[:total], corrected, int(err.item())

    def fastq_emit(self, data, records, begin, end, ubegin, uend, dest, which):
        """Formatted FASTQ text (uint8 device tensor) of the records with dest == which."""
        n = records.shape[0]
        offsets = self.empty((n + 1,), torch.int64)
        work = self.empty((max(self._host("atr_fastq_emit_work_bytes", n), 16),), torch.uint8)
        hint = int(data.numel() // max(n, 1))
        args = (_ptr(data), _ptr(records), _ptr(begin), _ptr(end), _ptr(ubegin), _ptr(uend), _ptr(dest), which, n, hint,
                _ptr(offsets), _ptr(work))
        self._call("atr_fastq_emit", *args, None)
        total = int(offsets[n].item())
        out = self.empty((max(total, 1),), torch.uint8)
        if total:
            self._call("atr_fastq_emit", *args, _ptr(out))
        return out[:total]

    def fastq_emit_grouped(self, data, records, begin, end, ubegin, uend, group, n_groups):
        """atr_fastq_emit for ``n_groups`` outputs in one pass: (text, bounds) -- the formatted records with
        ``group[r]`` (int32) == 0 first, then those of group 1 ..., input order inside a group, as one uint8 device
        tensor, and the ``n_groups + 1`` segment boundaries as a list of ints.  Records with any other code are not
        written."""
        n = records.shape[0]
        n_groups = int(n_groups)
        if n_groups > EMIT_MAX_GROUPS:
            raise AtroposUnsupported("atr_fastq_emit_grouped: %d outputs (at most %d)" % (n_groups, EMIT_MAX_GROUPS))
        offsets = self.empty((max(n, 1),), torch.int64)
        bounds = self.empty((max(n_groups, 0) + 1,), torch.int64)
        work = self.empty((max(self._host("atr_fastq_emit_grouped_work_bytes", n, n_groups), 16),), torch.uint8)
        hint = int(data.numel() // max(n, 1))
        args = (_ptr(data), _ptr(records), _ptr(begin), _ptr(end), _ptr(ubegin), _ptr(uend), _ptr(group), n_groups, n, hint,
                _ptr(offsets), _ptr(bounds), _ptr(work))
        self._call("atr_fastq_emit_grouped", *args, None)
        edges = bounds.cpu().tolist()
        out = self.empty((max(edges[-1], 1),), torch.uint8)
        if edges[-1]:
            self._call("atr_fastq_emit_grouped", *args, _ptr(out))
        return out[:edges[-1]], edges

    def demux_groups(self, dest, matched, last_which, adapter_group, n_adapters, untrimmed_group):
        """The output code of every read of a demultiplexed run (atr_demux_groups): int32 device tensor."""
        n = dest.shape[0]
        group = self.empty((n,), torch.int32)
        self._call("atr_demux_groups", _ptr(dest), _ptr(matched), _ptr(last_which), _ptr(adapter_group), int(n_adapters),
                   int(untrimmed_group), n, _ptr(group))
        return group

    # -- .gz output on the device (atr_gzip_*) ------------------------------------------------------------------
    def gzip_bound(self, nbytes):
        return self._host("atr_gzip_bound", int(nbytes))

    def gzip_blocks(self, text, offsets=False):
        """``text`` (uint8 device tensor) as a stream of BGZF members, one per ``GZIP_BLOCK`` bytes: (stream, total) --
        a uint8 device tensor whose first ``total`` bytes are the members in input order -- and with ``offsets`` also
        the int64 device tensor of the member starts followed by the total.  Reading ``total`` waits for the kernels."""
        n = int(text.numel())
        if not text.is_contiguous():
            text = text.contiguous()
        cap = self.gzip_bound(n)
        out = self.empty((max(cap, 1),), torch.uint8)
        total = self.empty((1,), torch.int64)
        starts = self.empty(((n + GZIP_BLOCK - 1) // GZIP_BLOCK + 1,), torch.int64) if offsets else None
        work = self.empty((max(self._host("atr_gzip_work_bytes", n), 16),), torch.uint8)
        self._call("atr_gzip_blocks", _ptr(text), n, _ptr(out), cap, _ptr(total), _ptr(starts), _ptr(work))
        size = int(total.item())
        return (out, size, starts) if offsets else (out, size)

    # -- BGZF .gz input on the device (atr_bgzf_scan, atr_gunzip_members) ------------------------------------------
    def bgzf_scan(self, buf, lo, hi, max_members):
        """The whole BGZF members at the front of ``buf[lo:hi]`` (a uint8 HOST tensor), at most ``max_members``:
        (member_at, text_at, k, covered, ok) -- int64 host tensors whose entries 0 .. k are the members' offsets from
        ``lo`` and the running sum of their text sizes; ``covered`` = member_at[k]; ``ok`` is False when the walk
        stopped at a header that is no BGZF member (at ``lo + covered``)."""
        return _bgzf_scan(self._symbol("atr_bgzf_scan"), buf, lo, hi, max_members)

    def gunzip_members(self, stream, n_stream, member_at, text_at, n_members, text, capacity):
        """Inflate ``n_members`` BGZF members of ``stream`` (uint8 device tensor, readable to the next multiple of 16
        beyond ``n_stream``) into ``text[text_at[m]:text_at[m + 1]]``; ``member_at`` / ``text_at``: int64 device
        tensors.  Returns (status int32 [n_members], bad int32 [1]) on the device: nothing here waits for the kernel."""
        status = self.empty((max(int(n_members), 1),), torch.int32)
        bad = self.empty((1,), torch.int32)
        self._call("atr_gunzip_members", _ptr(stream), int(n_stream), _ptr(member_at), _ptr(text_at), int(n_members),
                   _ptr(text), int(capacity), _ptr(status), _ptr(bad))
        return status, bad

    # -- known-contaminant detection (atr_detect_*) ---------------------------------------------------------------
    def detect_create(self, seqs, kmer_size, past_end_bases, thresholds, complexity, max_len):
        """seqs: list of bytes; thresholds: list of int (-1 = never); complexity: float64 ndarray
        [max_len + 1, max_len + 1].  Returns the handle."""
        lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
        thr = np.asarray(thresholds, dtype=np.int32)
        cx = np.ascontiguousarray(complexity, dtype=np.float64)
        h = C.c_void_p()
        self._call("atr_detect_create", b"".join(seqs), lens.ctypes.data, len(seqs), int(kmer_size), bytes(past_end_bases),
                   len(past_end_bases), thr.ctypes.data, cx.ctypes.data, int(max_len), C.byref(h))
        return h

    def detect_destroy(self, h):
        self._host("atr_detect_destroy", h)

    def detect_counters(self, h):
        """A zeroed counter block (int64 tensor; the words are uint64 counters)."""
        block = self.empty((self._host("atr_detect_counter_bytes", h) // 8,), torch.int64)
        self._call("atr_detect_clear", h, _ptr(block))
        return block

    def detect_filter(self, h, data, records, longest, counters):
        """(kept int32 [n], hashes int64 [n]) of the records."""
        n = records.shape[0]
        kept = self.empty((n,), torch.int32)
        hashes = self.empty((n,), torch.int64)
        self._call("atr_detect_filter_batch", h, _ptr(data), _ptr(records), n, int(longest), _ptr(kept), _ptr(hashes),
                   _ptr(counters))
        return kept, hashes

    def detect_mark(self, h, data, records, kept, order, head, counters):
        """rep uint8 [m]: 1 for one read of every distinct kept sequence (order / head: int64 [m])."""
        m = order.shape[0]
        rep = self.empty((m,), torch.uint8)
        self._call("atr_detect_mark_batch", h, _ptr(data), _ptr(records), _ptr(kept), _ptr(order), _ptr(head), m, _ptr(rep),
                   _ptr(counters))
        return rep

    def detect_match(self, h, data, records, kept, order, rep, counters):
        self._call("atr_detect_batch", h, _ptr(data), _ptr(records), _ptr(kept), _ptr(order), _ptr(rep), order.shape[0],
                   _ptr(counters))

    def detect_read(self, h, counters):
        """The counter block as a host int64 ndarray."""
        out = np.zeros((counters.shape[0],), dtype=np.int64)
        self._call("atr_detect_read", h, _ptr(counters), out.ctypes.data)
        return out

    # -- the trim report (atr_report_*) ---------------------------------------------------------------------------
    def report_create(self, n_adapters, max_read_len, max_errors):
        h = C.c_void_p()
        self._host("atr_report_create", int(n_adapters), int(max_read_len), int(max_errors), C.byref(h))
        return h

    def report_destroy(self, h):
        self._host("atr_report_destroy", h)

    def report_counters(self, h):
        """A zeroed counter block (int64 tensor) for the handle's layout."""
        return torch.zeros((self._host("atr_report_counters", h),), dtype=torch.int64, device=self.device)

    def report_intervals(self, h, records, begin0, end0, begin1, end1, mode, front, back, slot, counters):
        self._call("atr_report_intervals", h, _ptr(records), _ptr(begin0), _ptr(end0), _ptr(begin1), _ptr(end1),
                   begin0.shape[0], int(mode), int(front), int(back), int(slot), _ptr(counters))

    def report_adapters(self, h, data, records, took, best, which, front, default_front, begin, end, longest, weight,
                        variant, counters):
        self._call("atr_report_adapters", h, _ptr(data), _ptr(records), _ptr(took), _ptr(best), _ptr(which), _ptr(front),
                   int(default_front), _ptr(begin), _ptr(end), begin.shape[0], int(longest), int(weight), int(variant),
                   _ptr(counters))

    def report_outputs(self, h, records, begin, end, matched, dest, counters):
        self._call("atr_report_outputs", h, _ptr(records), _ptr(begin), _ptr(end), _ptr(matched), _ptr(dest), begin.shape[0],
                   _ptr(counters))

    def report_read(self, h, counters):
        """The counter block as a host int64 ndarray (the one device -> host copy of a report)."""
        out = np.zeros((counters.shape[0],), dtype=np.int64)
        self._call("atr_report_read", h, _ptr(counters), out.ctypes.data)
        return out


class StatsCalls(object):
    """The wrappers of the read-statistics entry points (atr_read_stats_*), written against ``_call`` / ``_host`` like
    ``AbiCalls``' methods.  A mixin of its own: the CPU test-suite serves these entry points from a twin library of
    their own (tests/emu/emu_stats.cpp)."""

    def read_stats_words(self, max_len):
        """uint64 words of a statistics block for reads of up to ``max_len`` bases."""
        return self._host("atr_read_stats_bytes", int(max_len)) // 8

    def read_stats_clear(self, block, max_len):
        self._call("atr_read_stats_clear", _ptr(block), int(max_len))

    def read_stats_batch(self, block, max_len, longest, quality_base, data, records, begin=None, end=None, ubegin=None,
                         uend=None, dest=None, which=0, index_base=0):
        """Adds the records (their kept intervals, masks and destination filter as atr_fastq_emit) into ``block``;
        record r is read ``index_base + r`` of the stream."""
        self._call("atr_read_stats_batch", _ptr(block), int(max_len), int(longest), int(quality_base), _ptr(data),
                   _ptr(records), _ptr(begin), _ptr(end), _ptr(ubegin), _ptr(uend), _ptr(dest), int(which), records.shape[0],
                   int(index_base))

    def read_stats_merge(self, dst, dst_max_len, src, src_max_len, index_offset=0):
        self._call("atr_read_stats_merge", _ptr(dst), int(dst_max_len), _ptr(src), int(src_max_len), int(index_offset))


class PairTextCalls(object):
    """The wrappers of the paired-text entry points (interleaved output), written against ``_call`` / ``_host`` /
    ``empty`` like ``AbiCalls``' methods.  A mixin of its own: the CPU test-suite serves these entry points from a
    twin library of their own (tests/emu/emu_pairtext.cpp)."""

    def fastq_emit_pairs(self, batch1, begin1, end1, ubegin1, uend1, batch2, begin2, end2, ubegin2, uend2, dest, which):
        """Formatted FASTQ text (uint8 device tensor) of the pairs with dest == which (dest None: all of them): read
        1's record, then read 2's, pair after pair (atr_fastq_emit_pairs).  ``batch1`` / ``batch2``: anything with
        ``data`` and ``records`` (a FastqBatch); the two may share one ``data`` tensor (interleaved input)."""
        n = batch1.records.shape[0]
        if batch2.records.shape[0] != n:
            raise ValueError("fastq_emit_pairs: the two record arrays hold different numbers of records")
        offsets = self.empty((n + 1,), torch.int64)
        work = self.empty((max(self._host("atr_fastq_emit_pairs_work_bytes", n), 16),), torch.uint8)
        nbytes = batch1.data.numel()
        if batch2.data.data_ptr() != batch1.data.data_ptr():
            nbytes += batch2.data.numel()
        hint = int(nbytes // max(n, 1))
        args = (_ptr(batch1.data), _ptr(batch1.records), _ptr(begin1), _ptr(end1), _ptr(ubegin1), _ptr(uend1),
                _ptr(batch2.data), _ptr(batch2.records), _ptr(begin2), _ptr(end2), _ptr(ubegin2), _ptr(uend2),
                _ptr(dest), which, n, hint, _ptr(offsets), _ptr(work))
        self._call("atr_fastq_emit_pairs", *args, None)
        total = int(offsets[n].item())
        out = self.empty((max(total, 1),), torch.uint8)
        if total:
            self._call("atr_fastq_emit_pairs", *args, _ptr(out))
        return out[:total]


    def overwrite_plan(self, batch1, begin1, end1, batch2, begin2, end2, lowq, highq, window, quality_base):
        """OverwriteRead's decisions over the kept intervals (atr_overwrite_plan_batch): (which uint8 [n] -- 0 none, 1
        read 1 overwritten, 2 read 2 --, grow1, grow2 int64 [n + 1]: where every clone goes in the tail of the chunk of
        read 1 / read 2, [n] the bytes that tail needs)."""
        n = batch1.records.shape[0]
        which = self.empty((n,), torch.uint8)
        grow1, grow2 = self.empty((n + 1,), torch.int64), self.empty((n + 1,), torch.int64)
        work = self.empty((max(self._host("atr_overwrite_work_bytes", n), 16),), torch.uint8)
        self._call("atr_overwrite_plan_batch", _ptr(batch1.data), _ptr(batch1.records), _ptr(begin1), _ptr(end1),
                   _ptr(batch2.data), _ptr(batch2.records), _ptr(begin2), _ptr(end2), n, int(lowq), int(highq), int(window),
                   int(quality_base), _ptr(which), _ptr(grow1), _ptr(grow2), _ptr(work))
        return which, grow1, grow2

    def overwrite_apply(self, data1, records1, begin1, end1, data2, records2, begin2, end2, which, grow1, grow2, tail1, tail2,
                        comp):
        """Writes the clones into the grown chunks and re-points ``records`` / ``begin`` / ``end`` of the overwritten
        reads IN PLACE (atr_overwrite_apply_batch); returns the error word."""
        n = records1.shape[0]
        err = self.empty((1,), torch.int64)
        self._call("atr_overwrite_apply_batch", _ptr(data1), _ptr(records1), _ptr(begin1), _ptr(end1), _ptr(data2),
                   _ptr(records2), _ptr(begin2), _ptr(end2), n, _ptr(which), _ptr(grow1), _ptr(grow2), int(tail1), int(tail2),
                   comp, _ptr(err))
        return int(err.item())


class FastaCalls(object):
    """The wrappers of the FASTA entry points (index and formatter), written against ``_call`` / ``_host`` / ``empty``
    like ``AbiCalls``' methods.  A mixin of its own: the CPU test-suite serves these entry points from a twin library
    of their own (tests/emu/emu_fasta.cpp)."""

    def fasta_index(self, data, nbytes):
        """data: uint8 device tensor holding nbytes of FASTA text (16-byte aligned, zero-padded to the next multiple of
        16 and 16 bytes more).  Returns (data, records int32 [nrec, 8], record_ends int32 [nrec], tail_end, nlines,
        error word): ``data`` is the tensor given, or -- when records are wrapped -- a longer one whose tail
        [padded text, tail_end) holds their sequences in one piece; the records point into it."""
        info = self.empty((4,), torch.int64)
        work = self.empty((max(self._host("atr_fastq_work_bytes", nbytes), 16),), torch.uint8)
        self._call("atr_fastq_count_lines", _ptr(data), nbytes, _ptr(work), _ptr(info))     # (the same lines as FASTQ's)
        nlines = int(info[0].item())
        line_ends = self.empty((max(nlines, 1),), torch.int32)
        work = self.empty((max(self._host("atr_fasta_work_bytes", nbytes, nlines), 16),), torch.uint8)
        self._call("atr_fasta_scan", _ptr(data), nbytes, _ptr(line_ends), nlines, _ptr(work), C.c_void_p(info.data_ptr() + 8))
        _, nrec, gather, err = (int(v) for v in info.cpu().tolist())
        tail_off = (nbytes + 15) // 16 * 16 + 16
        if gather:
            if tail_off + gather >= (1 << 32) - 32:
                raise ValueError("a FASTA chunk and its unwrapped sequences must stay below 4 GiB; read the file in smaller chunks")
            grown = self.empty((tail_off + (gather + 15) // 16 * 16 + 16,), torch.uint8)
            have = min(tail_off, data.numel())
            grown[:have].copy_(data[:have])
            grown[have:tail_off].zero_()
            grown[tail_off + gather:].zero_()
            data = grown
        records = self.empty((nrec, 8), torch.int32)
        record_ends = self.empty((nrec,), torch.int32)
        self._call("atr_fasta_index", _ptr(data), nbytes, _ptr(line_ends), nlines, _ptr(work), nrec, tail_off, gather,
                   _ptr(records), _ptr(record_ends))
        return data, records, record_ends, (tail_off + gather if gather else nbytes), nlines, err

    def fasta_emit(self, data, records, begin, end, ubegin, uend, dest, which):
        """Formatted FASTA text (uint8 device tensor) of the records with dest == which (FASTA or FASTQ records)."""
        n = records.shape[0]
        offsets = self.empty((n + 1,), torch.int64)
        work = self.empty((max(self._host("atr_fasta_emit_work_bytes", n), 16),), torch.uint8)
        hint = int(data.numel() // max(n, 1))
        args = (_ptr(data), _ptr(records), _ptr(begin), _ptr(end), _ptr(ubegin), _ptr(uend), _ptr(dest), which, n, hint,
                _ptr(offsets), _ptr(work))
        self._call("atr_fasta_emit", *args, None)
        total = int(offsets[n].item())
        out = self.empty((max(total, 1),), torch.uint8)
        if total:
            self._call("atr_fasta_emit", *args, _ptr(out))
        return out[:total]


class GunzipStreamCalls(object):
    """The wrappers of the stream gunzip entry points (an ordinary .gz member inflated on the device), written against
    ``_call`` / ``_host`` / ``empty`` like ``AbiCalls``' methods.  A mixin of its own: the CPU test-suite serves these
    entry points from a twin library of their own (tests/emu/emu_gunzip_stream.cpp)."""

    def gunzip_stream_workspace(self, n_stream, chunk_bytes, capacity):
        return self._host("atr_gunzip_stream_workspace", int(n_stream), int(chunk_bytes), int(capacity))

    def gunzip_stream(self, stream, n_stream, start_bit, window, window_len, crc_in, text, capacity, chunk_bytes, work=None):
        """Inflate the blocks of ONE deflate stream that begin at bit ``start_bit`` of ``stream[:n_stream]`` (uint8 device
        tensor) into ``text[:capacity]``; ``window[:window_len]``: the text before them, ``crc_in`` its CRC-32 so far;
        ``chunk_bytes``: the spacing of the speculative starts.  Returns the 8 int64 result words on the device
        (``GUNZIP_STREAM_WORDS``): nothing here waits for the kernels.  ``work``: a uint8 device tensor of at least
        ``gunzip_stream_workspace`` bytes to use again."""
        need = self.gunzip_stream_workspace(n_stream, chunk_bytes, capacity)
        if work is None or work.numel() < need:
            work = self.empty((need,), torch.uint8)
        result = self.empty((len(GUNZIP_STREAM_WORDS),), torch.int64)
        self._call("atr_gunzip_stream", _ptr(stream), int(n_stream), int(start_bit), _ptr(window), int(window_len),
                   int(crc_in) & 0xffffffff, _ptr(text), int(capacity), int(chunk_bytes), _ptr(work), work.numel(), _ptr(result))
        return result


class BamCalls(object):
    """The wrappers of the unaligned BAM entry points (header, record walk, decode to FASTQ text), written against
    ``_call`` / ``_host`` / ``empty`` like ``AbiCalls``' methods.  A mixin of its own: the CPU test-suite serves these
    entry points from a twin library of their own (tests/emu/emu_bam.cpp)."""

    def bam_header(self, buf):
        """``buf``: bytes from the front of an inflated BAM stream.  (header bytes, n_ref), or None when ``buf`` ends
        inside the header; another magic is a ValueError."""
        raw = bytes(buf)
        length, n_ref = C.c_int64(0), C.c_int32(0)
        rc = self._host("atr_bam_header", C.c_char_p(raw), len(raw), C.byref(length), C.byref(n_ref))
        return None if rc == BAM_NEED_MORE else (int(length.value), int(n_ref.value))

    def bam_walk(self, data, nbytes, entry, n_ref, final, tile_bytes=BAM_TILE, max_block=BAM_MAX_BLOCK, work=None):
        """The record starts of ``data[:nbytes]`` (uint8 device tensor, 16-byte aligned, padded to the next multiple of
        16) from ``entry`` on.  Returns (starts int32 [capacity], the 4 int64 result words on the device:
        ``BAM_WALK_WORDS``): nothing here waits for the kernels."""
        need = self._host("atr_bam_walk_workspace", int(nbytes), int(tile_bytes))
        if work is None or work.numel() < need:
            work = self.empty((max(need, 16),), torch.uint8)
        capacity = (int(nbytes) - int(entry)) // 36 + 1
        starts = self.empty((capacity,), torch.int32)
        result = self.empty((len(BAM_WALK_WORDS),), torch.int64)
        self._call("atr_bam_walk", _ptr(data), int(nbytes), int(entry), int(n_ref), int(bool(final)), int(tile_bytes),
                   int(max_block), _ptr(starts), capacity, _ptr(result), _ptr(work), work.numel())
        return starts, result

    def bam_to_fastq(self, data, nbytes, starts, n, paired=False):
        """FASTQ text (uint8 device tensor, zero-padded to the next multiple of 16 and 16 bytes more) of the records
        ``starts[:n]``; (text, its bytes, records written, error word, offsets int64 [written + 1])."""
        n = int(n)
        offsets = self.empty((n + 1,), torch.int64)
        result = self.empty((len(BAM_DECODE_WORDS),), torch.int64)
        work = self.empty((max(self._host("atr_bam_to_fastq_work_bytes", n), 16),), torch.uint8)
        args = (_ptr(data), int(nbytes), _ptr(starts), n, int(bool(paired)), _ptr(offsets), _ptr(result), _ptr(work))
        self._call("atr_bam_to_fastq", *args, None)
        total, err, used = (int(v) for v in result.cpu().tolist())
        if total >= (1 << 32) - 32:
            raise ValueError("the FASTQ text of a BAM chunk must stay below 4 GiB; read the file in smaller chunks")
        text = self.empty(((total + 15) // 16 * 16 + 16,), torch.uint8)
        text[total:].zero_()
        if used and err == INT64_MAX:
            self._call("atr_bam_to_fastq", *args, _ptr(text))
            err = int(result[1].item())
        return text, total, used, err, offsets[:used + 1]


class KmerCalls(object):
    """The wrappers of the de-novo discovery entry points (atr_detect_kmer_*), written against ``_call`` / ``_host`` /
    ``empty`` like ``AbiCalls``' methods.  A mixin of its own: the CPU test-suite serves these entry points from a twin
    library of their own (tests/emu/emu_kmer.cpp)."""

    def detect_kmer_slots(self, records, kept, reps, start, total, kmer_size):
        """reps / start: int64 [nrep].  (table of representatives int64 [nrep, 3], slot_rep int32 [total], level int32
        [nrep])."""
        nrep = int(reps.shape[0])
        tab = self.empty((max(nrep, 1), 3), torch.int64)
        slot_rep = self.empty((max(int(total), 1),), torch.int32)
        level = self.empty((max(nrep, 1),), torch.int32)
        self._call("atr_detect_kmer_slots", _ptr(records), _ptr(kept), _ptr(reps), _ptr(start), nrep, int(total), int(kmer_size),
                   _ptr(tab), _ptr(slot_rep), _ptr(level))
        return tab, slot_rep[:int(total)], level[:nrep]

    def detect_kmer_pair_keys(self, tab, slot_rep, data, id_a, a, id_b, b):
        """int64 keys [slots] of the (a + b)-mers (``None`` for the classes of 1-mers: the bytes)."""
        total = int(slot_rep.shape[0])
        keys = self.empty((max(total, 1),), torch.int64)
        self._call("atr_detect_kmer_pair_keys", _ptr(tab), _ptr(slot_rep), total, _ptr(data), _ptr(id_a), int(a), _ptr(id_b), int(b),
                   _ptr(keys))
        return keys[:total]

    def detect_kmer_rank(self, keys, idx, slot_list, cls):
        """``keys`` sorted, ``idx`` where each came from, ``slot_list`` (or None) the slot of an entry; writes ``cls``
        at the slots.  (begin, end, head int32 [n], nclasses int64 [1] on the device)."""
        n = int(keys.shape[0])
        begin, end, head = (self.empty((max(n, 1),), torch.int32) for _ in range(3))
        nclasses = self.empty((1,), torch.int64)
        need = self._host("atr_detect_kmer_rank_work_bytes", n)
        work = self.empty((max(need, 16),), torch.uint8)
        self._call("atr_detect_kmer_rank", _ptr(keys), _ptr(idx), _ptr(slot_list), n, _ptr(cls), _ptr(begin), _ptr(end), _ptr(head),
                   _ptr(nclasses), _ptr(work), work.numel())
        return begin, end, head, nclasses

    def detect_kmer_state(self, capacity):
        """(zeroed state block int64 [KMER_S_WORDS], candidate table int32 [capacity, KMER_C_WORDS])."""
        state = self.empty((KMER_S_WORDS,), torch.int64)
        state.zero_()
        return state, self.empty((max(int(capacity), 1), KMER_C_WORDS), torch.int32)

    def detect_kmer_level(self, tab, slot_rep, slot_list, n, cls, cls_prev, classes, cand_of_prev, k, min_count, level, cand,
                          capacity, state):
        """One level; returns cand_of int32 [n] (class -> its row or -1)."""
        begin, end, head = classes
        cand_of = self.empty((max(int(n), 1),), torch.int32)
        self._call("atr_detect_kmer_level", _ptr(tab), _ptr(slot_rep), _ptr(slot_list), int(n), _ptr(cls), _ptr(cls_prev),
                   _ptr(begin), _ptr(end), _ptr(head), _ptr(cand_of), _ptr(cand_of_prev), int(k), int(min_count), _ptr(level),
                   _ptr(cand), int(capacity), _ptr(state))
        return cand_of

    def detect_kmer_next(self, tab, slot_rep, slot_list, n, cls, data, level, k, state):
        """(list_next int32 [n], keys_next int64 [n]); how many are filled is word KMER_S_SURVIVORS of ``state``."""
        list_next = self.empty((max(int(n), 1),), torch.int32)
        keys_next = self.empty((max(int(n), 1),), torch.int64)
        self._call("atr_detect_kmer_next", _ptr(tab), _ptr(slot_rep), _ptr(slot_list), int(n), _ptr(cls), _ptr(data), _ptr(level),
                   int(k), _ptr(list_next), _ptr(keys_next), _ptr(state))
        return list_next, keys_next

    def detect_kmer_gather(self, tab, nrep, data, cand, text_off):
        """The texts of the rows of ``cand`` back to back (uint8); text_off int64 [rows + 1] on the device."""
        ncand = int(text_off.shape[0]) - 1
        out = self.empty((max(int(text_off[-1].item()), 1),), torch.uint8)
        self._call("atr_detect_kmer_gather", _ptr(tab), int(nrep), _ptr(data), _ptr(cand), _ptr(text_off), ncand, _ptr(out))
        return out

    def detect_kmer_support(self, tab, nrep, data, level, patterns):
        """patterns: list of bytes (at most KMER_MAX_PATTERNS, each at most DETECT_MAX_READ).  (abundance int64 [P],
        longest uint64 words as int64 [P]) on the host."""
        npat = len(patterns)
        mat = np.zeros((max(npat, 1), DETECT_MAX_READ), dtype=np.uint8)
        lens = np.zeros((max(npat, 1),), dtype=np.int32)
        for i, p in enumerate(patterns[:KMER_MAX_PATTERNS]):
            if len(p) > DETECT_MAX_READ:
                raise AtroposUnsupported("atr_detect_kmer_support: a pattern of %d bytes (at most %d)" % (len(p), DETECT_MAX_READ))
            mat[i, :len(p)] = np.frombuffer(p, dtype=np.uint8)
            lens[i] = len(p)
        d_mat = torch.from_numpy(mat).to(self.device)
        d_lens = torch.from_numpy(lens).to(self.device)
        abundance = self.empty((max(npat, 1),), torch.int64)
        longest = self.empty((max(npat, 1),), torch.int64)
        self._call("atr_detect_kmer_support", _ptr(tab), int(nrep), _ptr(data), _ptr(level), _ptr(d_mat), _ptr(d_lens), npat,
                   _ptr(abundance), _ptr(longest))
        return abundance[:npat].cpu().numpy(), longest[:npat].cpu().numpy()


class HipBackend(AbiCalls, PairTextCalls, StatsCalls, FastaCalls, GunzipStreamCalls, BamCalls, KmerCalls):
    """Thin object view of the C ABI; all buffers are torch tensors on one GPU.  The calls the CPU test-suite's stand-in
    serves as well are ``AbiCalls``'; here are the plumbing under them and the device-only calls."""

    name = "hip"
    WORKS_KEPT = 4

    def __init__(self, device=None):
        self.lib = load_library()
        self._fns = attach_prototypes(self.lib)
        if not torch.cuda.is_available():
            raise AtroposHipError("no HIP device visible to torch; the alignment kernels need an MI355X")
        if self._host("atr_device_count") < 1:
            raise AtroposHipError("atr_device_count() == 0: no HIP device")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._works = {}                  # the kernels' scratch, one per stream calls are issued on (Aligner.locate_stream)
        self._side = []

    # -- the call path -----------------------------------------------------------
    def _call(self, name, *args):
        """Entry point ``name`` on this backend's device, on the current stream where the prototype has one."""
        fn, at = self._fns[name]
        with torch.cuda.device(self.device):
            if at is None:
                rc = fn(*args)
            else:
                stream = torch.cuda.current_stream(self.device).cuda_stream
                rc = fn(*args, stream) if at == len(args) else fn(*args[:at], stream, *args[at:])
        return rc if rc is None or rc >= 0 else _check(self.lib, rc, name)

    def _host(self, name, *args):
        """An entry point that touches no device: no device guard, no stream."""
        rc = self._fns[name][0](*args)
        return rc if rc is None or rc >= 0 else _check(self.lib, rc, name)

    def _symbol(self, name):
        return self._fns[name][0]

    def _stream(self):
        """The current stream as an argument for a direct call of a library function (tests, tools)."""
        return STREAM(torch.cuda.current_stream(self.device).cuda_stream)

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    @property
    def _work(self):
        return self._works.get(torch.cuda.current_stream(self.device).cuda_stream)

    @_work.setter
    def _work(self, tensor):
        # one scratch per stream that issues calls, most recently used last; at most WORKS_KEPT of them are kept (a
        # 10 M-read workspace is ~1 GB: a backend whose callers come and go on fresh streams -- worker_context() -- would
        # otherwise pin one per stream it ever saw).  Dropping an entry frees nothing a kernel still
        # reads: the tensor's memory goes back to torch's caching allocator, which orders re-use on the stream it
        # was allocated on.
        key = torch.cuda.current_stream(self.device).cuda_stream
        self._works.pop(key, None)
        self._works[key] = tensor
        while len(self._works) > self.WORKS_KEPT:
            self._works.pop(next(iter(self._works)))

    def _workspace(self, need, first=0):
        work = self._work
        if work is None or work.numel() < need:
            work = self._work = self.empty((max(need, first),), torch.uint8)
        return work

    def last_unresolved(self, nreads, n_adapters=1):
        """Reads the pre-pass of the last filtered call on the current stream left to the exact DP kernels
        (atr_locate_work_unresolved); None when no such call used this stream's workspace."""
        work = self._work
        if work is None:
            return None
        out = C.c_int64(0)
        self._call("atr_locate_work_unresolved", _ptr(work), int(nreads), int(n_adapters), C.byref(out))
        return int(out.value)

    def stage_host_bytes(self, mat):
        """A uint8 ndarray [n, w] -> the same bytes in a page-locked host tensor (kept and re-used): the upload that
        follows is one DMA.  The previous upload from the buffer is waited for first."""
        need = int(mat.size)
        buf = getattr(self, "_pinned", None)
        if buf is None or buf.numel() < need:
            buf = self._pinned = torch.empty((max(need, 1 << 20),), dtype=torch.uint8).pin_memory()
            self._pinned_event = None
        if self._pinned_event is not None:
            self._pinned_event.synchronize()
        view = buf[:need].view(mat.shape)
        np.copyto(view.numpy(), mat)
        self._pinned_event = torch.cuda.Event()
        return _PinnedUpload(view, self)

    def side_streams(self, count):
        """``count`` streams of this backend's device, created once (Aligner.locate_stream issues consecutive batches
        on them in turn; every stream gets a workspace of its own)."""
        while len(self._side) < count:
            self._side.append(torch.cuda.Stream(device=self.device))
        return self._side[:count]

    @contextlib.contextmanager
    def worker_context(self):
        """Device + a stream of its own for a host thread that drives this GPU next to other
        threads driving theirs; the stream is synchronised on exit."""
        stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            yield stream
            stream.synchronize()

    # -- device-only calls ---------------------------------------------------------
    def insert_match_correct_batch(self, h, planes1, planes2, seq1, qual1, seq2, qual2, action, min_qual_diff, comp,
                                   changed=None, newlen=None):
        """insert_match_batch + insert_correct_batch as ONE kernel (atr_insert_match_correct_batch): the reads'
        planes are streamed once.  planes1 / planes2: plane64 ReadBatches whose lengths are also the lengths of
        the matrix rows.  Returns (records int16 [n, 3, 8], changed, newlen)."""
        n = planes1.nreads
        if planes1.max_len != planes2.max_len:
            raise ValueError("both read batches must be packed with the same max_len")
        if seq1.stride(0) != seq2.stride(0):
            raise ValueError("both reads need the same row stride")
        out = self.empty((n, 3, 8), torch.int16)
        changed = self.empty((n, 2), torch.int32) if changed is None else changed
        newlen = self.empty((n, 2), torch.int32) if newlen is None else newlen
        if n:
            self._call("atr_insert_match_correct_batch", h, _ptr(planes1.packed), _ptr(planes1.lens), _ptr(planes2.packed),
                       _ptr(planes2.lens), n, planes1.max_len, _ptr(out), _ptr(seq1), _ptr(qual1), _ptr(seq2), _ptr(qual2),
                       seq1.stride(0), action, min_qual_diff, comp, _ptr(changed), _ptr(newlen))
        return out, changed, newlen

    def aligner_prepare(self, h, max_len, ragged=False):
        """atr_aligner_prepare: build / load the pre-pass kernel specialised for this aligner and read length on this
        backend's device.  True: ready; False: there is none (the generic kernel serves the calls)."""
        try:
            self._call("atr_aligner_prepare", h, int(max_len), int(bool(ragged)))
        except AtroposUnsupported:                        # (no specialised kernel, not an error)
            return False
        return True

    def locate_ascii_planes_batch(self, h, ascii_2d, lens, max_len, planes=None):
        """atr_locate_ascii_planes_batch: a long batch of ASCII rows -> (records int16 [n, 8], the packed plane64 buffer the
        call wrote) in one pre-pass launch + the DP kernels."""
        nreads = ascii_2d.shape[0]
        out = self.empty((nreads, 8), torch.int16)
        if planes is None:
            planes = self.empty((max(self.packed_bytes(nreads, max_len), 16),), torch.uint8)
        if nreads:
            work = self._workspace(self._host("atr_locate_work_bytes", nreads))
            self._call("atr_locate_ascii_planes_batch", h, _ptr(ascii_2d), ascii_2d.stride(0), _ptr(lens), nreads, int(max_len),
                       _ptr(planes), _ptr(out), _ptr(work))
        return out, planes

    def locate_ascii_batch(self, h, ascii_2d, lens, max_len):
        """atr_locate_ascii_batch: a short batch of ASCII rows (uint8 [n, width] on the device, row stride a multiple of
        four) through the wavefront-per-read kernel without packing; int16 [n, 8] records."""
        n = ascii_2d.shape[0]
        out = self.empty((n, 8), torch.int16)
        if n:
            self._call("atr_locate_ascii_batch", h, _ptr(ascii_2d), ascii_2d.stride(0), _ptr(lens), n, max_len, _ptr(out))
        return out

    def _tls_buffer(self, name, make, fits=None):
        """The result buffer of a one-object call, one per host thread: ctypes releases the GIL during the call and
        the C side stages per thread, so two threads on one backend must not share the record they read back."""
        tls = self.__dict__.get("_tls")
        if tls is None:
            tls = self.__dict__.setdefault("_tls", threading.local())
        buf = getattr(tls, name, None)
        if buf is None or (fits is not None and not fits(buf)):
            buf = make()
            setattr(tls, name, buf)
        return buf

    def locate_one(self, h, query):
        """``Aligner.locate`` of ONE read (bytes) -- what the module swap of INTEGRATION.md section 1 calls per
        read: atr_locate_one (the kernel reads the read from a page-locked staging buffer and writes the record
        into one; one launch, one synchronisation, no allocation).  Returns the six numbers or None."""
        rec = self._tls_buffer("one_rec", lambda: (C.c_int16 * 8)())
        self._call("atr_locate_one", h, query, len(query), C.addressof(rec))
        return None if rec[1] < 0 else (rec[0], rec[1], rec[2], rec[3], rec[4], rec[5])

    def multi_locate_one(self, ref, query, e, flags, min_overlap, max_matches):
        """``MultiAligner.locate`` of ONE pair of byte strings (atr_multi_locate_one); list of 6-tuples or None."""
        cap = max_matches + len(ref) + 2              # the last-column scan appends past max_matches (_align.pyx:750-763)
        buf = self._tls_buffer("multi_buf", lambda: (C.c_int16 * (cap * 8))(), lambda b: len(b) >= cap * 8)
        cnt = self._tls_buffer("multi_cnt", C.c_int32)
        self._call("atr_multi_locate_one", ref, len(ref), query, len(query), e, flags, min_overlap, max_matches,
                   C.addressof(buf), cap, C.addressof(cnt))
        c = cnt.value
        return None if c == 0 else [tuple(buf[8 * t:8 * t + 6]) for t in range(c)]

    def compare_one(self, ref, query, wildcard_ref, wildcard_query, suffix):
        """compare_prefixes / compare_suffixes of one pair of byte strings (atr_compare_one); the 6-tuple."""
        rec = self._tls_buffer("cmp_rec", lambda: (C.c_int16 * 8)())
        self._call("atr_compare_one", ref, len(ref), query, len(query), int(wildcard_ref), int(wildcard_query), int(suffix),
                   C.addressof(rec))
        return (rec[0], rec[1], rec[2], rec[3], rec[4], rec[5])

    def locate_pair_one(self, ref_codes, revcomp_ref, query_codes, e, flags, wildcard_ref, wildcard_query, min_overlap,
                        indel_cost):
        """``Aligner(ref, ...).locate(query)`` for ONE pair of translated byte strings (atr_locate_pair_one)."""
        rec = self._tls_buffer("pair_rec", lambda: (C.c_int16 * 8)())
        self._call("atr_locate_pair_one", ref_codes, len(ref_codes), int(revcomp_ref), query_codes, len(query_codes), e, flags,
                   int(wildcard_ref), int(wildcard_query), min_overlap, indel_cost, C.addressof(rec))
        return None if rec[1] < 0 else (rec[0], rec[1], rec[2], rec[3], rec[4], rec[5])

    def insert_match_one(self, h, seq1, seq2):
        """``InsertAligner.match_insert`` of ONE pair of byte strings (upper-case IUPAC letters only: the caller checks);
        the three records as a flat list of 24 int16 values (atr_insert_match_one)."""
        rec = self._tls_buffer("ins_rec", lambda: (C.c_int16 * 24)())
        self._call("atr_insert_match_one", h, seq1, len(seq1), seq2, len(seq2), C.addressof(rec))
        return rec

    def linked_group_applies(self, h, max_len):
        return bool(self._host("atr_linked_group_applies", h, int(max_len)))

    def linked_group_pack(self, h, ascii_2d, lens, max_len, table):
        """atr_linked_group_pack: the 5' parts decided from the ASCII rows, read[front.rstop:] packed as bit planes into
        a sub-batch per adapter.  Returns a ``LinkedGroups`` (device buffers + the host info block); waits for the stream."""
        nreads = ascii_2d.shape[0]
        g = LinkedGroups()
        g.nreads, g.max_len = nreads, int(max_len)
        g.grouped = self.empty((max(self._host("atr_linked_group_bytes", nreads, max_len), 16),), torch.uint8)
        g.glens = self.empty((nreads + 64 * LINKED_MAX_ADAPTERS,), torch.int32)
        g.perm = self.empty((nreads + 64 * LINKED_MAX_ADAPTERS,), torch.int32)
        g.slot_of = self.empty((nreads,), torch.int32)
        g.which = self.empty((nreads, 2), torch.int8)
        g.front = self.empty((nreads, 8), torch.int16)
        g.info = (C.c_int64 * 8)()
        g.work = self.empty((max(self._host("atr_linked_group_work_bytes", h, nreads), 16),), torch.uint8)
        if nreads:
            self._call("atr_linked_group_pack", h, _ptr(ascii_2d), ascii_2d.stride(0), _ptr(lens), nreads, int(max_len), table,
                       _ptr(g.grouped), _ptr(g.glens), _ptr(g.perm), _ptr(g.slot_of), _ptr(g.which), _ptr(g.front), g.info,
                       _ptr(g.work))
        return g

    def linked_group_match(self, h, g, ordered=True):
        """atr_linked_group_match on a ``LinkedGroups``: (slab int16 [slots, 8] raw 3' records in slot order, back int16
        [n, 8] in batch order after the acceptance test -- None unless ``ordered``)."""
        slots = g.glens.shape[0]
        slab = self.empty((slots, 8), torch.int16)
        back = self.empty((g.nreads, 8), torch.int16) if ordered else None
        if g.nreads:
            self._call("atr_linked_group_match", h, _ptr(g.grouped), _ptr(g.glens), g.info, g.max_len, _ptr(g.slot_of),
                       _ptr(g.which), g.nreads, _ptr(slab), _ptr(back), _ptr(g.work))
        return slab, back


_backend = None
_thread_local = threading.local()


def get_backend():
    """The backend of the calling thread (``thread_backend``: one per GPU in a multi-device
    process), else the process-wide one, created on first use.  Raises (never falls back)
    when the HIP library or the GPU is missing."""
    global _backend
    mine = getattr(_thread_local, "backend", None)
    if mine is not None:
        return mine
    if _backend is None:
        _backend = HipBackend()
    return _backend


@contextlib.contextmanager
def thread_backend(backend):
    """Make ``backend`` the backend of the calling thread: objects built inside the block
    (aligners, adapters) live on its GPU.  Used by the single-process multi-device drivers
    (atropos_amd.shard), one host thread per device."""
    prev = getattr(_thread_local, "backend", None)
    _thread_local.backend = backend
    try:
        yield backend
    finally:
        _thread_local.backend = prev


def set_backend(backend, _test_double=False):
    """Install the process-wide backend: a ``HipBackend`` (bench.py pins one device per rank with it)
    or None (forget the current one).  Returns the previous one.  Anything else is refused -- the
    product never computes on a stand-in; the CPU test-suite injects its kernel emulation by saying so
    explicitly (``_test_double=True``, tests/ only)."""
    global _backend
    if backend is not None and not isinstance(backend, HipBackend) and not _test_double:
        raise TypeError("set_backend: only a HipBackend can be installed")
    prev, _backend = _backend, backend
    return prev
