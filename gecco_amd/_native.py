"""ctypes binding of the C ABI in ``include/gecco_crf.h`` (``gecco_amd/lib/libgecco_crf.so``).

This is the stub a GECCO maintainer would add on the reference side: it
replaces the per-window python-crfsuite crossing at ``gecco/crf/__init__.py:253`` with one
call per batch of contigs.  There is no CPU fallback: if the library cannot be loaded the
import error propagates, and compute calls on a box without a HIP device raise.
"""
import ctypes
import operator
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgecco_crf.so")

OK, EINVAL, EFORMAT, ENOMEM, EHIP, ENODEV, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -6

_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_f64p = ctypes.POINTER(ctypes.c_double)
_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_c_i8p = ctypes.POINTER(ctypes.c_int8)
_c_u32p = ctypes.POINTER(ctypes.c_uint32)
_vp = ctypes.c_void_p

# name -> (restype, argtypes); every symbol include/gecco_crf.h declares
SIGNATURES = {
    "gecco_crf_last_error": (ctypes.c_char_p, []),
    "gecco_crf_version": (ctypes.c_int, []),
    "gecco_crf_model_load": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "gecco_crf_model_from_tables": (ctypes.c_int, [_c_f64p, _c_f64p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    "gecco_crf_model_free": (None, [_vp]),
    "gecco_crf_model_num_labels": (ctypes.c_int32, [_vp]),
    "gecco_crf_model_num_attrs": (ctypes.c_int32, [_vp]),
    "gecco_crf_model_num_features": (ctypes.c_int32, [_vp]),
    "gecco_crf_model_label_name": (ctypes.c_char_p, [_vp, ctypes.c_int32]),
    "gecco_crf_model_attr_name": (ctypes.c_char_p, [_vp, ctypes.c_int32]),
    "gecco_crf_model_label_id": (ctypes.c_int32, [_vp, ctypes.c_char_p]),
    "gecco_crf_model_attr_id": (ctypes.c_int32, [_vp, ctypes.c_char_p]),
    "gecco_crf_model_map_attrs": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, _c_i32p]),
    "gecco_crf_model_state_weights": (ctypes.c_int, [_vp, _c_f64p, _c_u8p]),
    "gecco_crf_model_trans_weights": (ctypes.c_int, [_vp, _c_f64p, _c_u8p]),
    "gecco_crf_model_slot_table": (ctypes.c_int, [_vp, ctypes.c_int32, _c_f64p, _c_f64p, _c_i32p]),
    "gecco_crf_slot_prod_max_cnt": (ctypes.c_int32, [ctypes.c_double]),
    "gecco_crf_device_count": (ctypes.c_int, [_c_i32p]),
    "gecco_crf_windowed_marginals": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, _c_f64p],
    ),
    "gecco_crf_windowed_marginals_all": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, _c_f64p, _c_f64p],
    ),
    "gecco_crf_marginals_full": (ctypes.c_int, [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_f64p]),
    "gecco_crf_viterbi": (ctypes.c_int, [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_i8p, _c_f64p]),
    "gecco_crf_windowed_marginals_valued": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_int32, _c_f64p],
    ),
    "gecco_crf_windowed_marginals_all_valued": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_int32, _c_f64p, _c_f64p],
    ),
    "gecco_crf_marginals_full_valued": (
        ctypes.c_int, [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_f64p, _c_f64p]),
    "gecco_crf_viterbi_valued": (
        ctypes.c_int, [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_i8p, _c_f64p]),
    "gecco_crf_windowed_marginals_constrained": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_int32, _c_f64p],
    ),
    "gecco_crf_windowed_marginals_all_constrained": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_int32, _c_f64p, _c_f64p],
    ),
    "gecco_crf_marginals_full_constrained": (
        ctypes.c_int, [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_f64p, _c_f64p]),
    "gecco_crf_viterbi_constrained": (
        ctypes.c_int, [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_i8p, _c_f64p]),
    "gecco_crf_span_probabilities": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_i32p, _c_i32p, _c_i32p, _c_u32p,
         ctypes.c_int32, _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_span_conditionals": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_i32p, _c_i32p, _c_i32p, _c_u32p,
         ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), _c_f64p, _c_f64p, _c_f64p,
         _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_run_posteriors": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_i32p, _c_i32p, _c_u32p,
         ctypes.c_int32, ctypes.c_int32, _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_i32p, _c_i32p, _c_i32p, _c_u32p,
         ctypes.c_int32, _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_sample_paths": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_int32, ctypes.c_uint64,
         _c_i32p, _c_i32p, _c_u32p, ctypes.c_int32, _c_i8p, _c_i32p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_viterbi_kbest": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_int32, _c_i8p, _c_f64p,
         _c_i32p, _c_f64p],
    ),
    "gecco_crf_max_marginals": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_u32p, ctypes.c_int32, _c_i32p,
         _c_i32p, _c_i32p, _c_u32p, ctypes.c_int32, _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_viterbi_min_run": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_uint32, ctypes.c_int32, _c_i8p,
         _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_marginals_min_run": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_uint32, ctypes.c_int32, _c_f64p,
         _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_viterbi_run_length": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_uint32, ctypes.c_int32, _c_f64p,
         ctypes.c_double, _c_i8p, _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_marginals_run_length": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_uint32, ctypes.c_int32, _c_f64p,
         ctypes.c_double, _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_ring": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_i8p, _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_run_counts": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, ctypes.c_uint32, ctypes.c_int32, _c_f64p,
         _c_f64p, _c_i8p, _c_f64p],
    ),
    "gecco_crf_edge_posteriors": (
        ctypes.c_int,
        [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_f64p, _c_u32p, _c_u32p, ctypes.c_int32, _c_f64p,
         _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_f64p, _c_f64p],
    ),
    "gecco_crf_segment": (
        ctypes.c_int,
        [ctypes.c_int32, _c_f64p, _c_u8p, _c_i32p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p],
    ),
    "gecco_crf_segment_ex": (
        ctypes.c_int, [ctypes.c_int32, _c_f64p, _c_u8p, _c_i32p, ctypes.c_int32, _vp, _c_i32p, ctypes.c_int32, _c_i32p]
    ),
    "gecco_crf_domain_composition": (
        ctypes.c_int,
        [ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_f64p, ctypes.c_int32, ctypes.c_int32, _c_f64p],
    ),
    "gecco_crf_plan_create": (
        ctypes.c_int, [_vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp)]
    ),
    "gecco_crf_plan_free": (None, [_vp]),
    "gecco_crf_plan_num_genes": (ctypes.c_int32, [_vp]),
    "gecco_crf_plan_num_windows": (ctypes.c_int64, [_vp]),
    "gecco_crf_plan_num_tiles": (ctypes.c_int32, [_vp]),
    "gecco_crf_plan_tile_out": (ctypes.c_int32, [_vp]),
    "gecco_crf_plan_kernel_name": (ctypes.c_char_p, [_vp]),
    "gecco_crf_plan_run_windowed": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int32, _vp, _vp]),
    "gecco_crf_plan_run_windowed_all": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp]),
    "gecco_crf_plan_all_kernel_name": (ctypes.c_char_p, [_vp]),
    "gecco_crf_plan_time_windowed_all": (
        ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)]
    ),
    "gecco_crf_plan_run_decode": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "gecco_crf_plan_run_decode_pipelined": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "gecco_crf_plan_run_marginals_full": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "gecco_crf_plan_run_viterbi": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "gecco_crf_plan_run_segment": (
        ctypes.c_int,
        [_vp, _vp, _vp, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp],
    ),
    "gecco_crf_plan_run_segment_ex": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp]),
    "gecco_crf_host_alloc": (ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "gecco_crf_host_free": (None, [_vp]),
    "gecco_crf_session_create": (ctypes.c_int, [_vp, _c_i32p, ctypes.c_int32, ctypes.POINTER(_vp)]),
    "gecco_crf_session_free": (None, [_vp]),
    "gecco_crf_session_set_chunk_genes": (ctypes.c_int, [_vp, ctypes.c_int32]),
    "gecco_crf_session_set_direct_genes": (ctypes.c_int, [_vp, ctypes.c_int32]),
    "gecco_crf_session_stats": (
        ctypes.c_int,
        [_vp, _c_i32p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), _c_f64p, _c_f64p],
    ),
    "gecco_crf_session_stats_ex": (ctypes.c_int, [_vp, _vp]),
    "gecco_crf_session_set_reference_bits": (ctypes.c_int, [_vp, ctypes.c_int32]),
    "gecco_crf_exp_correctly_rounded": (ctypes.c_int, [_c_f64p, ctypes.c_int64, _c_f64p]),
    "gecco_crf_session_windowed": (
        ctypes.c_int,
        # (array arguments as addresses: `ndarray.ctypes.data_as` costs 2 us per array, a quarter of a warm call on one contig)
        [_vp, _vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp],
    ),
    "gecco_crf_session_windowed_degrees": (
        ctypes.c_int,
        [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp],
    ),
    "gecco_crf_session_decode": (
        ctypes.c_int,
        [_vp, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f64p,
         _c_i8p],
    ),
    "gecco_crf_session_clusters": (
        ctypes.c_int,
        [_vp, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_u8p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f64p, _c_i32p, ctypes.c_int32, _c_i32p, _c_f64p,
         ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
    ),
    "gecco_crf_session_clusters_ex": (
        ctypes.c_int,
        [_vp, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_u8p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         _vp, _c_f64p, _c_i32p, ctypes.c_int32, _c_i32p, _c_f64p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
    ),
    "gecco_crf_session_clusters_degrees": (
        ctypes.c_int,
        [_vp, _c_i32p, ctypes.c_int32, _c_i32p, _c_u8p, _c_i32p, _c_u8p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         _vp, _c_f64p, _c_i32p, ctypes.c_int32, _c_i32p, _c_f64p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)],
    ),
    "gecco_crf_session_decode_wire": (
        ctypes.c_int,
        [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp],
    ),
    "gecco_crf_session_clusters_wire": (
        ctypes.c_int,
        # (array arguments as plain addresses: a typed ctypes pointer costs 3.5 us to make, an address half of that)
        [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, ctypes.c_int64, _vp],
    ),
    "gecco_crf_pack_columns": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp)]),
    "gecco_crf_packed_free": (None, [_vp]),
    "gecco_crf_packed_info": (
        ctypes.c_int,
        [_vp, _c_i32p, _c_i32p, ctypes.POINTER(ctypes.c_int64), _c_i32p, _c_i32p, _c_i32p],
    ),
    "gecco_crf_packed_contig_ptr": (_vp, [_vp]),
    "gecco_crf_packed_gene_ptr": (_vp, [_vp]),
    "gecco_crf_packed_attr_id": (_vp, [_vp]),
    "gecco_crf_packed_annotated": (_vp, [_vp]),
    "gecco_crf_packed_gene_row": (_vp, [_vp]),
    "gecco_crf_packed_row_gene": (_vp, [_vp]),
    "gecco_crf_packed_row_order": (_vp, [_vp]),
    "gecco_crf_packed_row_ptr": (_vp, [_vp]),
    "gecco_crf_packed_marker_ptr": (_vp, [_vp]),
    "gecco_crf_packed_marker_id": (_vp, [_vp]),
    "gecco_crf_cluster_rows_build": (ctypes.c_int, [_vp, _vp, _vp, _vp, _c_i32p, ctypes.c_int32, _c_f64p, _vp, ctypes.POINTER(_vp)]),
    "gecco_crf_cluster_rows_free": (None, [_vp]),
    "gecco_crf_cluster_rows_start": (_vp, [_vp]),
    "gecco_crf_cluster_rows_end": (_vp, [_vp]),
    "gecco_crf_cluster_rows_average_p": (_vp, [_vp]),
    "gecco_crf_cluster_rows_max_p": (_vp, [_vp]),
    "gecco_crf_cluster_rows_strings": (ctypes.c_int, [_vp, ctypes.c_int32, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "gecco_crf_exact_mean": (ctypes.c_double, [_c_f64p, ctypes.c_int64]),
    "gecco_crf_gather_f64": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp]),
    "gecco_crf_packed_order_info": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "gecco_crf_tsv_format": (
        ctypes.c_int,
        [ctypes.c_int64, ctypes.c_int32, _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.c_char_p, ctypes.POINTER(_vp),
         ctypes.POINTER(ctypes.c_int64)],
    ),
    "gecco_crf_buffer_free": (None, [_vp]),
    "gecco_crf_trainer_create": (
        ctypes.c_int, [ctypes.c_int32, _c_i32p, ctypes.c_int32, _c_i32p, _c_i32p, _c_i32p, ctypes.c_int32, ctypes.c_int32,
                       ctypes.c_int32, ctypes.c_int32, _c_i32p, _c_i32p, ctypes.c_int32, ctypes.POINTER(_vp)]
    ),
    # (the three evals take the double arrays as addresses: `_TrainerHandle._eval_problems` has checked them)
    "gecco_crf_trainer_eval": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "gecco_crf_trainer_num_windows": (ctypes.c_int64, [_vp]),
    "gecco_crf_trainer_free": (None, [_vp]),
    "gecco_crf_trainer_batch_create": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp),
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, _c_i32p, ctypes.c_int32, ctypes.c_int32,
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp)]
    ),
    "gecco_crf_trainer_batch_eval": (ctypes.c_int, [_vp, _c_u8p, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp)]),
    "gecco_crf_trainer_batch_num_problems": (ctypes.c_int32, [_vp]),
    "gecco_crf_trainer_batch_num_windows": (ctypes.c_int64, [_vp, ctypes.c_int32]),
    "gecco_crf_trainer_batch_free": (None, [_vp]),
    "gecco_crf_trainer_grid_create": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp),
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, _c_i32p, _c_i32p, _c_i32p,
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, ctypes.c_int32, _c_i32p, ctypes.c_int64,
                       ctypes.POINTER(_vp)]
    ),
    "gecco_crf_trainer_grid_eval": (ctypes.c_int, [_vp, _c_u8p, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp)]),
    "gecco_crf_trainer_grid_num_problems": (ctypes.c_int32, [_vp]),
    "gecco_crf_trainer_grid_num_windows": (ctypes.c_int64, [_vp, ctypes.c_int32]),
    "gecco_crf_trainer_grid_scratch_bytes": (ctypes.c_int64, [_vp, ctypes.c_int32]),
    "gecco_crf_trainer_grid_free": (None, [_vp]),
    "gecco_crf_trainer_general_create": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp),
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, _c_i32p, _c_i32p, _c_i32p,
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp)]
    ),
    "gecco_crf_trainer_general_create_valued": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp),
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, _c_i32p, _c_i32p, _c_i32p,
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp)]
    ),
    "gecco_crf_trainer_general_create_partial": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp),
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, _c_i32p,
                       _c_i32p, _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp)]
    ),
    "gecco_crf_trainer_general_create_weighted": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp),
                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                       ctypes.POINTER(_vp), _c_i32p, _c_i32p, _c_i32p, _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                       _c_i32p, ctypes.POINTER(_vp)]
    ),
    "gecco_crf_trainer_general_eval": (ctypes.c_int, [_vp, _c_u8p, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp)]),
    "gecco_crf_trainer_general_num_problems": (ctypes.c_int32, [_vp]),
    "gecco_crf_trainer_general_num_windows": (ctypes.c_int64, [_vp, ctypes.c_int32]),
    "gecco_crf_trainer_general_scratch_bytes": (ctypes.c_int64, [_vp, ctypes.c_int32]),
    "gecco_crf_trainer_general_free": (None, [_vp]),
    "gecco_crf_trainer_sequences_create": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
         ctypes.POINTER(_vp), _c_i32p, _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp)],
    ),
    "gecco_crf_trainer_sequences_create_valued": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
         ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p,
         ctypes.POINTER(_vp)],
    ),
    "gecco_crf_trainer_sequences_create_partial": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
         ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, _c_i32p, ctypes.POINTER(_vp),
         ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp)],
    ),
    "gecco_crf_trainer_sequences_create_weighted": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
         ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p,
         _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_i32p, ctypes.POINTER(_vp)],
    ),
    "gecco_crf_trainer_sequences_eval": (ctypes.c_int, [_vp, _c_u8p, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp)]),
    "gecco_crf_trainer_sequences_num_problems": (ctypes.c_int32, [_vp]),
    "gecco_crf_trainer_sequences_num_sequences": (ctypes.c_int64, [_vp, ctypes.c_int32]),
    "gecco_crf_trainer_sequences_scratch_bytes": (ctypes.c_int64, [_vp, ctypes.c_int32]),
    "gecco_crf_trainer_sequences_free": (None, [_vp]),
    "gecco_crf_fisher_exact": (ctypes.c_int, [ctypes.c_int32, _vp, ctypes.c_int64, _vp]),
    "gecco_crf_cluster_overlaps": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp,
                       ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    ),
    "gecco_crf_domain_composition_members": (
        ctypes.c_int, [ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp]
    ),
    "gecco_crf_forest_fit": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32, _vp,
                       _vp, ctypes.c_int32, ctypes.POINTER(_vp)]
    ),
    "gecco_crf_forest_info": (ctypes.c_int, [_vp, _c_i32p, _c_i32p, _c_i32p, _vp, _vp]),
    "gecco_crf_forest_export": (ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gecco_crf_forest_predict": (ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp]),
    "gecco_crf_forest_free": (None, [_vp]),
    "gecco_crf_forest_fit_batch": (
        ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp,
                       _vp, _vp, _vp, _vp, _vp, _vp]
    ),
    "gecco_crf_forest_predict_batch": (ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, _vp]),
    "gecco_crf_plan_time_windowed": (
        ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)]
    ),
    "gecco_crf_plan_time_decode_pipelined": (
        ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)]
    ),
    "gecco_crf_plan_viterbi_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]),
}

_lib = None


def _elf_dynamic_strings(path: str, tags=(1, 14)) -> dict:
    """DT_NEEDED (1) / DT_SONAME (14) strings of a 64-bit little-endian ELF shared object, read from the file (nothing is loaded)."""
    import struct

    out = {t: [] for t in tags}
    with open(path, "rb") as fh:
        hdr = fh.read(64)
        if hdr[:4] != b"\x7fELF" or hdr[4] != 2 or hdr[5] != 1:
            return out
        shoff, = struct.unpack_from("<Q", hdr, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", hdr, 0x3A)
        secs = []
        for i in range(shnum):
            fh.seek(shoff + i * shentsize)
            sh = fh.read(shentsize)
            _, typ, _, _, off, size, link = struct.unpack_from("<IIQQQQI", sh, 0)
            secs.append((typ, off, size, link))
        for typ, off, size, link in secs:
            if typ != 6:  # SHT_DYNAMIC
                continue
            _, stroff, strsize, _ = secs[link]
            fh.seek(stroff)
            strtab = fh.read(strsize)
            fh.seek(off)
            dyn = fh.read(size)
            for k in range(0, len(dyn) - 15, 16):
                tag, val = struct.unpack_from("<qQ", dyn, k)
                if tag == 0:
                    break
                if tag in out:
                    out[tag].append(strtab[val:strtab.index(b"\0", val)].decode())
    return out


def _preload_hip_runtime(lib_path: str) -> Optional[str]:
    """A PyTorch wheel carries its own copy of libamdhip64, and whichever copy a process loads first serves everybody: loaded
    second, torch's copy finds no device.  `GECCO_AMD_HIP_RUNTIME` decides what a process that has NOT imported torch yet does:

    * unset / ``auto``: the wheel's copy is loaded ahead of libgecco_crf.so ONLY when its SONAME equals the libamdhip64 SONAME
      libgecco_crf.so was linked against (same ABI major: one runtime in the process, whatever the import order); a different
      SONAME gets a warning and the system's runtime (a later `import torch` in that process will then not see the device);
    * ``system``: never preload;  * ``torch``: preload whatever the wheel carries (the caller vouches for it).

    A process that has imported torch already has made the choice.  Returns the path that was loaded, or None."""
    import sys
    import warnings

    mode = os.environ.get("GECCO_AMD_HIP_RUNTIME", "auto").lower()
    if "torch" in sys.modules or mode == "system":
        return None
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return None
    if mode != "torch":
        try:
            wheel = _elf_dynamic_strings(cand)[14]
            needed = [n for n in _elf_dynamic_strings(lib_path)[1] if n.startswith("libamdhip64")]
        except (OSError, ValueError, IndexError) as err:
            warnings.warn(f"gecco_amd: could not compare the HIP runtime of the installed torch wheel with the one {lib_path} was linked "
                          f"against ({err}); keeping the system's runtime", RuntimeWarning, stacklevel=3)
            return None
        if not wheel or not needed or wheel[0] != needed[0]:
            warnings.warn(f"gecco_amd: the installed torch wheel carries {wheel[0] if wheel else 'an unnamed libamdhip64'}, "
                          f"libgecco_crf.so is linked against {needed[0] if needed else 'no libamdhip64'}: keeping the system's HIP "
                          "runtime (import torch BEFORE gecco_amd if this process needs both, or set GECCO_AMD_HIP_RUNTIME=torch)",
                          RuntimeWarning, stacklevel=3)
            return None
    try:
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except OSError as err:
        warnings.warn(f"gecco_amd: could not load {cand} ({err}); the system's HIP runtime serves", RuntimeWarning, stacklevel=3)
        return None
    return cand


# host-only views of what the library builds for its kernels: no inference or training call goes through them
_INTROSPECTION_ONLY = frozenset({"gecco_crf_model_slot_table", "gecco_crf_slot_prod_max_cnt"})


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen the native library and bind every declared symbol (raises if one is missing, the introspection-only ones excepted)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("GECCO_CRF_LIBRARY") or LIB_PATH  # the variable is for A/B runs of two builds
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: build it with `python -m gecco_amd.build` (hipcc, gfx950). "
            "gecco_amd has no CPU fallback."
        )
    _preload_hip_runtime(p)
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        if name in _INTROSPECTION_ONLY and not hasattr(lib, name):
            continue  # (a library built before these existed still loads for A/B runs; calling them then raises AttributeError)
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


class NativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (gecco_crf status {code})")
        self.code = code


def _check(rc: int) -> None:
    if rc == OK:
        return
    msg = load_library().gecco_crf_last_error().decode("utf-8", "replace")
    if rc == EINVAL:
        raise ValueError(msg)
    if rc == EFORMAT:
        raise ValueError(msg)
    if rc == ENOMEM:
        raise MemoryError(msg)
    raise NativeError(rc, msg)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(t)


def device_count() -> int:
    n = ctypes.c_int32(0)
    _check(load_library().gecco_crf_device_count(ctypes.byref(n)))
    return n.value


class Model:
    """Handle on a parsed CRF model (immutable, thread-safe)."""

    def __init__(self, handle):
        self._h = handle
        self._lib = load_library()

    @classmethod
    def from_lcrf(cls, blob: bytes) -> "Model":
        lib = load_library()
        h = _vp()
        _check(lib.gecco_crf_model_load(blob, len(blob), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_tables(cls, state: np.ndarray, trans: np.ndarray) -> "Model":
        lib = load_library()
        state = np.ascontiguousarray(state, dtype=np.float64)
        trans = np.ascontiguousarray(trans, dtype=np.float64)
        A, L = state.shape
        assert trans.shape == (L, L)
        h = _vp()
        _check(lib.gecco_crf_model_from_tables(_ptr(state, _c_f64p), _ptr(trans, _c_f64p), A, L, ctypes.byref(h)))
        return cls(h)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.gecco_crf_model_free(h)

    @property
    def num_labels(self) -> int:
        return self._lib.gecco_crf_model_num_labels(self._h)

    @property
    def num_attrs(self) -> int:
        return self._lib.gecco_crf_model_num_attrs(self._h)

    @property
    def num_features(self) -> int:
        return self._lib.gecco_crf_model_num_features(self._h)

    def labels(self):
        return [self._lib.gecco_crf_model_label_name(self._h, i).decode() for i in range(self.num_labels)]

    def attrs(self):
        return [self._lib.gecco_crf_model_attr_name(self._h, i).decode() for i in range(self.num_attrs)]

    def label_id(self, name: str) -> int:
        return self._lib.gecco_crf_model_label_id(self._h, name.encode())

    def attr_id(self, name: str) -> int:
        return self._lib.gecco_crf_model_attr_id(self._h, name.encode())

    def map_attrs(self, names: Sequence[str]) -> np.ndarray:
        n = len(names)
        arr = (ctypes.c_char_p * max(n, 1))(*[s.encode() for s in names])
        ids = np.empty(max(n, 1), dtype=np.int32)
        _check(self._lib.gecco_crf_model_map_attrs(self._h, arr, n, _ptr(ids, _c_i32p)))
        return ids[:n]

    def state_weights(self):
        A, L = self.num_attrs, self.num_labels
        w = np.zeros((A, L), dtype=np.float64)
        present = np.zeros((A, L), dtype=np.uint8)
        _check(self._lib.gecco_crf_model_state_weights(self._h, _ptr(w, _c_f64p), _ptr(present, _c_u8p)))
        return w, present.astype(bool)

    def slot_table(self, label: int = 1):
        """Two-label models: the factor table of the window kernels' slot constants, as the devices get it: an (A + 1, 2) array of
        (delta_a, exp(delta_a)) with the neutral pair (0, 1) last, max |delta_a| and the attribute count up to which a slot's
        constant is the running product (`gecco_crf_model_slot_table`)."""
        pairs = np.zeros((self.num_attrs + 1, 2), dtype=np.float64)
        dmax = ctypes.c_double(0.0)
        cnt = ctypes.c_int32(0)
        _check(self._lib.gecco_crf_model_slot_table(self._h, int(label), _ptr(pairs, _c_f64p),
                                                    ctypes.cast(ctypes.byref(dmax), _c_f64p), ctypes.cast(ctypes.byref(cnt), _c_i32p)))
        return pairs, dmax.value, cnt.value

    def trans_weights(self):
        L = self.num_labels
        w = np.zeros((L, L), dtype=np.float64)
        present = np.zeros((L, L), dtype=np.uint8)
        _check(self._lib.gecco_crf_model_trans_weights(self._h, _ptr(w, _c_f64p), _ptr(present, _c_u8p)))
        return w, present.astype(bool)

    # ---- one-shot compute (host buffers) ----
    # ``values=``: one float64 per attribute entry, parallel to ``attr_id`` (CRFsuite's name:value items): the state score of
    # a gene is the sum of value * weight, and the call takes the ``*_valued`` entry (the any-L kernels at every label
    # count).  None: the unvalued entry, as ever.
    # ``allowed=``: one uint32 per gene, bit y set when the gene may take label y (the trainers' masks): the call is the same
    # call on the lattice without the disallowed (gene, label) pairs, and takes the ``*_constrained`` entry, with ``values``
    # or without.  None: today's call, bit for bit.
    def _csr_head(self, contig_ptr, gene_ptr, attr_id, values, allowed, device):
        """A batch's CSR arrays as every one-shot entry takes them: ``(head, values, allowed, n, n0, nc)``.  ``head`` is the
        start of the entry's argument list (handle, device, ``contig_ptr``, the number of contigs ``nc``, ``gene_ptr``,
        ``attr_id``); ``values`` and ``allowed`` are the pointers of the checked arrays, None where the argument is (a pointer
        keeps its array alive).  The batch's genes are ``n0 .. n - 1``."""
        contig_ptr, gene_ptr, attr_id = _i32(contig_ptr), _i32(gene_ptr), _i32(attr_id)
        n, nc = (int(contig_ptr[-1]) if len(contig_ptr) else 0), max(len(contig_ptr) - 1, 0)
        n0 = int(contig_ptr[0]) if len(contig_ptr) else 0
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float64).ravel()
            if values.size != attr_id.size:
                raise ValueError(f"values holds {values.size} entries, attr_id {attr_id.size}")
            values = _ptr(values if values.size else np.zeros(1, dtype=np.float64), _c_f64p)
        if attr_id.size == 0:
            attr_id = np.zeros(1, dtype=np.int32)
        if allowed is not None:
            allowed = np.ascontiguousarray(allowed, dtype=np.uint32).ravel()
            if allowed.size != n:
                raise ValueError(f"allowed holds {allowed.size} masks for {n} genes")
            allowed = _ptr(allowed if allowed.size else np.zeros(1, dtype=np.uint32), _c_u32p)
        head = [self._h, device, _ptr(contig_ptr, _c_i32p), nc, _ptr(gene_ptr, _c_i32p), _ptr(attr_id, _c_i32p)]
        return head, values, allowed, n, n0, nc

    def _oneshot(self, name, contig_ptr, gene_ptr, attr_id, values, device, allowed=None):
        """The CSR arguments of the one-shot entry ``name``, or of ``name + "_valued"`` when ``values`` are given (their
        pointer goes in behind ``attr_id``'s), or of ``name + "_constrained"`` when ``allowed`` is (the values' pointer, or
        NULL, then the masks').  Returns ``(n_genes, n_contigs, run)``; ``run(*tail)`` calls the entry with the arguments
        that follow the CSR arrays."""
        head, values, allowed, n, _, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, device)
        if allowed is not None:
            head += [values, allowed]
            name += "_constrained"
        elif values is not None:
            head.append(values)
            name += "_valued"
        entry = getattr(self._lib, name)
        return n, nc, lambda *tail: _check(entry(*head, *tail))

    def windowed_marginals(self, contig_ptr, gene_ptr, attr_id, window, step=1, label=1, pad=True, device=0, values=None,
                           allowed=None):
        n, _, run = self._oneshot("gecco_crf_windowed_marginals", contig_ptr, gene_ptr, attr_id, values, device, allowed)
        out = np.zeros(max(n, 1), dtype=np.float64)
        run(int(window), int(step), int(label), int(bool(pad)), _ptr(out, _c_f64p))
        return out[:n]

    def windowed_marginals_all(self, contig_ptr, gene_ptr, attr_id, window, step=1, background=None, pad=True, device=0,
                               values=None, allowed=None):
        """Every label's windowed probability in one device pass: ``(p_all [n, L], p_any [n] or None)``; ``p_any`` is the
        windowed probability of any label but ``background`` (a label id)."""
        n, _, run = self._oneshot("gecco_crf_windowed_marginals_all", contig_ptr, gene_ptr, attr_id, values, device, allowed)
        p_all = np.zeros((max(n, 1), self.num_labels), dtype=np.float64)
        p_any = None if background is None else np.zeros(max(n, 1), dtype=np.float64)
        run(int(window), int(step), -1 if background is None else int(background), int(bool(pad)), _ptr(p_all, _c_f64p),
            None if p_any is None else _ptr(p_any, _c_f64p))
        return p_all[:n], (None if p_any is None else p_any[:n])

    def marginals_full(self, contig_ptr, gene_ptr, attr_id, device=0, values=None, allowed=None):
        """``(marginals [n, L], log Z [n_contigs])``; with ``allowed``, the marginals given that the path lies inside the
        sets (a disallowed entry is exactly 0.0) and ``log Z_A``."""
        n, nc, run = self._oneshot("gecco_crf_marginals_full", contig_ptr, gene_ptr, attr_id, values, device, allowed)
        marg = np.zeros((max(n, 1), self.num_labels), dtype=np.float64)
        ln = np.zeros(max(nc, 1), dtype=np.float64)
        run(_ptr(marg, _c_f64p), _ptr(ln, _c_f64p))
        return marg[:n], ln[:nc]

    def viterbi(self, contig_ptr, gene_ptr, attr_id, device=0, want_score=True, values=None, allowed=None):
        """Best label path per contig; with `want_score=False` returns (labels, None) and 2-label
        models take the cheaper score-difference form of the recursion.  With ``allowed``: the best path inside the sets."""
        n, nc, run = self._oneshot("gecco_crf_viterbi", contig_ptr, gene_ptr, attr_id, values, device, allowed)
        y = np.zeros(max(n, 1), dtype=np.int8)
        sc = np.zeros(max(nc, 1), dtype=np.float64) if want_score else None
        run(_ptr(y, _c_i8p), _ptr(sc, _c_f64p) if want_score else None)
        return y[:n], (sc[:nc] if want_score else None)

    def span_log_probabilities(self, contig_ptr, gene_ptr, attr_id, span_contig, span_begin, span_end, span_mask, device=0,
                               values=None, allowed=None, want_marginals=False):
        """Region posteriors: ``logp[q] = log P(y_t in set q for span_begin[q] <= t < span_end[q] | x)`` on the whole-contig
        lattice (``gecco_crf_span_probabilities``), for any number of spans behind one forward-backward pass of the batch.
        ``span_begin`` / ``span_end`` are offsets from the first gene of contig ``span_contig[q]``, the end exclusive;
        ``span_mask[q]`` has bit y set when label y is in the set.  ``values`` and ``allowed`` as in ``marginals_full``: with
        ``allowed`` the lattice is the restricted one.  Returns ``logp`` (float64, <= 0, ``-inf`` for probability zero), or
        with ``want_marginals`` ``(logp, marginals [n, L], log Z [n_contigs])``, the latter two as ``marginals_full`` gives
        them."""
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        sc, sb, se = _i32(span_contig).ravel(), _i32(span_begin).ravel(), _i32(span_end).ravel()
        sm = np.ascontiguousarray(span_mask, dtype=np.uint32).ravel()
        ns = sc.size
        if not (sb.size == ns and se.size == ns and sm.size == ns):
            raise ValueError("span_contig, span_begin, span_end and span_mask differ in length")
        pad_i, pad_u = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
        logp = np.zeros(max(ns, 1), dtype=np.float64)
        marg = np.zeros((max(n - n0, 1), self.num_labels), dtype=np.float64) if want_marginals else None
        ln = np.zeros(max(nc, 1), dtype=np.float64) if want_marginals else None
        _check(self._lib.gecco_crf_span_probabilities(
            *head, values, allowed, _ptr(sc if ns else pad_i, _c_i32p), _ptr(sb if ns else pad_i, _c_i32p),
            _ptr(se if ns else pad_i, _c_i32p), _ptr(sm if ns else pad_u, _c_u32p), ns, _ptr(logp, _c_f64p),
            None if marg is None else _ptr(marg, _c_f64p), None if ln is None else _ptr(ln, _c_f64p)))
        if want_marginals:
            return logp[:ns], marg[:n - n0], ln[:nc]
        return logp[:ns]

    def span_conditionals(self, contig_ptr, gene_ptr, attr_id, span_contig, span_begin, span_end, span_mask, reach=0, device=0,
                          values=None, allowed=None, want_contributions=True, want_marginals=False, row_ptr=None, occ_ptr=None):
        """Marginals given a region, and exact knock-out attributions (``gecco_crf_span_conditionals``): for every span of
        ``span_log_probabilities`` and the event E "every gene of the span carries a label of its set", the rows of the genes
        ``max(begin - reach, 0) .. min(end + reach, T)`` of its contig.  Returns a dict: ``logp [n_spans]``
        (``span_log_probabilities``' bytes), ``first [n_spans]`` (the offset of a query's first row inside its contig),
        ``row_ptr [n_spans + 1]`` (a query's rows are ``row_ptr[q] .. row_ptr[q + 1]``), ``cond [n_rows, L]`` = P(y_t = l | E, x),
        and with ``want_contributions`` ``occ_ptr [n_rows + 1]``, ``item [n_rows]`` and ``attr [n_occ]``: log P(E | x) minus
        log P(E | x without the row's gene's scores / without one attribute occurrence of it), the occurrences of row r at
        ``occ_ptr[r] .. occ_ptr[r + 1]`` in CSR order.  With ``want_marginals`` also ``marginals`` and ``lognorm`` as
        ``marginals_full`` gives them.  Where ``logp[q]`` is ``-inf`` the query's rows and contributions are 0.0.
        ``row_ptr`` / ``occ_ptr``: the tables are computed here and checked by the library; given, they are passed on as they
        are (tests of that check)."""
        reach = operator.index(reach)
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        cptr, gptr = _i32(contig_ptr).astype(np.int64), _i32(gene_ptr).astype(np.int64)
        sc, sb, se = _i32(span_contig).ravel(), _i32(span_begin).ravel(), _i32(span_end).ravel()
        sm = np.ascontiguousarray(span_mask, dtype=np.uint32).ravel()
        ns = sc.size
        if not (sb.size == ns and se.size == ns and sm.size == ns):
            raise ValueError("span_contig, span_begin, span_end and span_mask differ in length")
        # the rows of every query (the library refuses a bad span or reach before it looks at the tables: they only need a size)
        c64, b64, e64 = sc.astype(np.int64), sb.astype(np.int64), se.astype(np.int64)
        known = (c64 >= 0) & (c64 < nc)
        length = np.where(known, cptr[np.where(known, c64 + 1, 0)] - cptr[np.where(known, c64, 0)], 0) if nc else np.zeros(ns, np.int64)
        good = bool(reach >= 0 and np.all(known & (b64 >= 0) & (b64 < e64) & (e64 <= length)))
        first = np.maximum(b64 - reach, 0) if good else np.zeros(ns, dtype=np.int64)
        count = np.minimum(e64 + reach, length) - first if good else np.zeros(ns, dtype=np.int64)
        rows = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        n_rows = int(rows[-1])
        occ = None
        if want_contributions:
            gene = np.repeat(cptr[c64] + first - rows[:-1], count) + np.arange(n_rows) if n_rows else np.zeros(0, dtype=np.int64)
            occ = np.concatenate([[0], np.cumsum(gptr[gene + 1] - gptr[gene])]).astype(np.int64)
        if row_ptr is not None:
            rows = np.ascontiguousarray(row_ptr, dtype=np.int64).ravel()
        if occ_ptr is not None:
            occ = np.ascontiguousarray(occ_ptr, dtype=np.int64).ravel()
        n_occ = int(occ[-1]) if occ is not None and occ.size else 0
        L = self.num_labels
        pad_i, pad_u = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
        logp = np.zeros(max(ns, 1), dtype=np.float64)
        cond = np.zeros((max(n_rows, 1), L), dtype=np.float64)
        item = np.zeros(max(n_rows, 1), dtype=np.float64) if want_contributions else None
        attr = np.zeros(max(n_occ, 1), dtype=np.float64) if want_contributions else None
        marg = np.zeros((max(n - n0, 1), L), dtype=np.float64) if want_marginals else None
        ln = np.zeros(max(nc, 1), dtype=np.float64) if want_marginals else None
        p = lambda x: None if x is None else _ptr(x, _c_f64p)
        i64 = lambda x: None if x is None else _ptr(x, ctypes.POINTER(ctypes.c_int64))
        _check(self._lib.gecco_crf_span_conditionals(
            *head, values, allowed, _ptr(sc if ns else pad_i, _c_i32p), _ptr(sb if ns else pad_i, _c_i32p),
            _ptr(se if ns else pad_i, _c_i32p), _ptr(sm if ns else pad_u, _c_u32p), ns, reach, i64(rows), i64(occ), p(logp), p(cond),
            p(item), p(attr), p(marg), p(ln)))
        out = dict(logp=logp[:ns], first=first.astype(np.int64), row_ptr=rows, cond=cond[:n_rows])
        if want_contributions:
            out.update(occ_ptr=occ, item=item[:n_rows], attr=attr[:n_occ])
        if want_marginals:
            out.update(marginals=marg[:n - n0], lognorm=ln[:nc])
        return out

    def run_posteriors(self, contig_ptr, gene_ptr, attr_id, anchors=None, reach=64, runs=None, device=0, values=None, allowed=None,
                       want_marginals=False):
        """Run posteriors on the whole-contig lattice (``gecco_crf_run_posteriors``), any number of queries behind one
        forward-backward pass of the batch.  ``anchors=(contig, item, mask)``, three arrays of one length: for the run through
        gene ``item[q]`` of contig ``contig[q]`` -- the maximal stretch of genes around it whose labels all lie in ``mask[q]`` --
        ``log_anchor [n]`` (log P(the gene's label is in the set)), ``log_start [n, reach + 1]`` (entry r: log P(the run starts
        at ``item - r``)), ``log_start_beyond [n]`` (the run starts before the reach), and ``log_end`` / ``log_end_beyond``
        likewise towards the contig's end (entry r: the run's last gene is ``item + r``).  ``runs=(contig, begin, end, mask)``,
        four arrays of one length: ``log_run [n]``, log P(a run is exactly ``[begin, end)``).  Natural logs, ``<= 0``, ``-inf``
        for probability zero.  ``values`` and ``allowed`` as in ``marginals_full``.  Returns a dict with the keys named above
        (those of a list that was not given are left out), and with ``want_marginals`` also ``marginals`` and ``lognorm`` as
        ``marginals_full`` gives them.  A model whose largest |transition weight| (among those whose exp is not 0) exceeds 150 is
        refused with ``ValueError``: subtract a constant from every transition weight."""
        reach = operator.index(reach)
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        na = nr = 0
        if anchors is not None:
            ac, ai = _i32(anchors[0]).ravel(), _i32(anchors[1]).ravel()
            am = np.ascontiguousarray(anchors[2], dtype=np.uint32).ravel()
            na = ac.size
            if not (ai.size == na and am.size == na):
                raise ValueError("the anchors' contig, item and mask differ in length")
        if runs is not None:
            rc, rb, re_ = _i32(runs[0]).ravel(), _i32(runs[1]).ravel(), _i32(runs[2]).ravel()
            rm = np.ascontiguousarray(runs[3], dtype=np.uint32).ravel()
            nr = rc.size
            if not (rb.size == nr and re_.size == nr and rm.size == nr):
                raise ValueError("the runs' contig, begin, end and mask differ in length")
        # (the library refuses any other reach, or more than 2^31 - 1 entries: the buffers only need a size)
        row = reach + 1 if 0 <= reach <= 65536 and na * (reach + 1) < 1 << 31 else 1
        small = [np.zeros(max(na, 1), dtype=np.float64) for _ in range(3)]
        wide = [np.zeros((max(na, 1), row), dtype=np.float64) for _ in range(2)]
        log_run = np.zeros(max(nr, 1), dtype=np.float64)
        marg = np.zeros((max(n - n0, 1), self.num_labels), dtype=np.float64) if want_marginals else None
        ln = np.zeros(max(nc, 1), dtype=np.float64) if want_marginals else None
        p = lambda x: _ptr(x, _c_f64p)
        _check(self._lib.gecco_crf_run_posteriors(
            *head, values, allowed,
            _ptr(ac, _c_i32p) if na else None, _ptr(ai, _c_i32p) if na else None, _ptr(am, _c_u32p) if na else None, na, reach,
            p(small[0]), p(wide[0]), p(small[1]), p(wide[1]), p(small[2]),
            _ptr(rc, _c_i32p) if nr else None, _ptr(rb, _c_i32p) if nr else None, _ptr(re_, _c_i32p) if nr else None,
            _ptr(rm, _c_u32p) if nr else None, nr, p(log_run),
            None if marg is None else p(marg), None if ln is None else p(ln)))
        out = {}
        if anchors is not None:
            out.update(log_anchor=small[0][:na], log_start=wide[0][:na], log_start_beyond=small[1][:na], log_end=wide[1][:na],
                       log_end_beyond=small[2][:na])
        if runs is not None:
            out["log_run"] = log_run[:nr]
        if want_marginals:
            out.update(marginals=marg[:n - n0], lognorm=ln[:nc])
        return out

    def sample_paths(self, contig_ptr, gene_ptr, attr_id, n_samples, seed=0, device=0, values=None, allowed=None, runs=None,
                     want_marginals=False, want_paths=True):
        """Label paths drawn from ``p(y | x)`` on the whole-contig lattice (``gecco_crf_sample_paths``): ``y`` as int8
        ``[n, n_samples]``, ``y[g, s]`` the label of gene g in sample s, every sample of a contig one draw by forward filtering
        and backward sampling behind ONE forward-backward pass of the batch.  The uniforms are Philox4x32-10 under ``seed``
        (0 .. 2**64 - 1) with counters (gene offset, sample, contig): equal arguments give equal bytes, and sample s does not
        depend on ``n_samples`` (1 .. 2**20).  ``values`` and ``allowed`` as in ``marginals_full``: with ``allowed`` no sample
        carries a disallowed label.  ``runs=(contig, anchor, mask)``, three arrays of one length: also returns int32
        ``[n_runs, n_samples, 2]``, per query and sample the maximal run ``(first, last + 1)`` of genes around the anchor (offsets
        inside contig ``contig[q]``) whose labels all lie in ``mask[q]``, or ``(-1, -1)`` where the anchor's label does not.
        With ``want_marginals`` also ``marginals [n, L], log Z [n_contigs]`` as ``marginals_full`` gives them.  Returns ``y``,
        or a tuple ``(y[, runs][, marginals, log Z])``.  ``want_paths=False`` passes ``y = NULL``: the paths stay in device
        workspace, serve the runs, and ``y`` is left out of what is returned (None when nothing else was asked for)."""
        n_samples, seed = operator.index(n_samples), operator.index(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed {seed} is outside 0 .. 2**64 - 1")
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        nr = 0
        if runs is not None:
            rc, ra = _i32(runs[0]).ravel(), _i32(runs[1]).ravel()
            rm = np.ascontiguousarray(runs[2], dtype=np.uint32).ravel()
            nr = rc.size
            if not (ra.size == nr and rm.size == nr):
                raise ValueError("the runs' contig, anchor and mask differ in length")
        ns = n_samples if 1 <= n_samples <= 1 << 20 else 1  # (the library refuses any other n_samples: the buffers only need a size)
        y = np.zeros((max(n - n0, 1), ns), dtype=np.int8) if want_paths else None
        out_runs = np.zeros((max(nr, 1), ns, 2), dtype=np.int32)
        marg = np.zeros((max(n - n0, 1), self.num_labels), dtype=np.float64) if want_marginals else None
        ln = np.zeros(max(nc, 1), dtype=np.float64) if want_marginals else None
        _check(self._lib.gecco_crf_sample_paths(
            *head, values, allowed, n_samples, seed,
            _ptr(rc, _c_i32p) if nr else None, _ptr(ra, _c_i32p) if nr else None, _ptr(rm, _c_u32p) if nr else None, nr,
            None if y is None else _ptr(y, _c_i8p), _ptr(out_runs, _c_i32p) if nr else None,
            None if marg is None else _ptr(marg, _c_f64p), None if ln is None else _ptr(ln, _c_f64p)))
        out = [y[:n - n0]] if want_paths else []
        if runs is not None:
            out.append(out_runs[:nr])
        if want_marginals:
            out += [marg[:n - n0], ln[:nc]]
        return None if not out else out[0] if len(out) == 1 else tuple(out)

    def viterbi_kbest(self, contig_ptr, gene_ptr, attr_id, k, device=0, values=None, allowed=None):
        """The ``k`` best label paths of every contig on the whole-contig lattice (``gecco_crf_viterbi_kbest``), 1 <= k <= 32.
        Returns ``(y, score, n_paths, lognorm)``: ``y`` int8 ``[n, k]``, ``y[g, r]`` the label of gene g on its contig's rank-r
        path (-1 where no path fills the rank); ``score`` float64 ``[n_contigs, k]``, non-increasing along a row, the path's
        left-to-right score (``-inf`` at an empty rank); ``n_paths`` int32 ``[n_contigs]``; ``lognorm`` ``[n_contigs]`` as
        ``marginals_full`` gives it, so that ``exp(score - lognorm[:, None])`` are the paths' exact probabilities.  Equal
        scores are ordered by the reversed path (last gene's label first); rank r does not depend on ``k``; rank 0 is
        ``viterbi``'s path.  ``values`` and ``allowed`` as in ``marginals_full``: with ``allowed`` no path carries a disallowed
        label.  A contig without genes has ``n_paths`` 0, scores ``-inf`` and ``lognorm`` 0."""
        k = operator.index(k)
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        kk = k if 1 <= k <= 32 else 1  # (the library refuses any other k: the buffers only need a size)
        y = np.zeros((max(n - n0, 1), kk), dtype=np.int8)
        score = np.zeros((max(nc, 1), kk), dtype=np.float64)
        n_paths = np.zeros(max(nc, 1), dtype=np.int32)
        ln = np.zeros(max(nc, 1), dtype=np.float64)
        _check(self._lib.gecco_crf_viterbi_kbest(
            *head, values, allowed, k, _ptr(y, _c_i8p), _ptr(score, _c_f64p), _ptr(n_paths, _c_i32p), _ptr(ln, _c_f64p)))
        return y[:n - n0], score[:nc], n_paths[:nc], ln[:nc]

    def max_marginals(self, contig_ptr, gene_ptr, attr_id, sets=None, spans=None, device=0, values=None, allowed=None,
                      want_through=True, want_inside=True, want_outside=True, want_span_best=True, want_span_broken=True,
                      want_lognorm=False):
        """Max-marginals of the whole-contig lattice (``gecco_crf_max_marginals``): scores of best paths under a restriction,
        from one max-plus forward and one backward walk of the batch.  Returns a dict that holds only what was asked for:
        ``"best"`` float64 ``[n_contigs]``, the score of the contig's best path (``viterbi_kbest``'s rank-0 bits; 0 for a
        contig without genes);
        ``"through"`` (``want_through``) ``[n, L]``: the score of the best path of the gene's contig that gives the gene that
        label -- ``-inf`` where no such path exists, never NaN, and not clamped to ``best``;
        ``"inside"``, ``"outside"`` (``sets``: 1 to 32 uint32 masks, bit y set when label y is in the set) ``[n, n_sets]``:
        the maximum of ``through`` over the labels in / not in the set (``-inf`` for an empty or wholly disallowed side);
        ``"span_best"``, ``"span_broken"`` (``spans``: ``(contig, begin, end, mask)`` arrays as ``span_log_probabilities``
        takes them) ``[n_spans]``: the score of the best path whose labels on the span all lie in the set, and of the best
        path with a label outside it somewhere on the span;
        ``"lognorm"`` (``want_lognorm``) ``[n_contigs]`` as ``marginals_full`` gives it -- the only output that runs the
        sum-product pass.
        The numbers are path scores: a difference of two is the log of the ratio of two single paths' probabilities, not a
        posterior.  ``values`` and ``allowed`` as in ``marginals_full``: with ``allowed`` the lattice is the restricted one."""
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        L = self.num_labels
        ns = nq = 0
        sm = None
        if sets is not None:
            sm = np.ascontiguousarray(sets, dtype=np.uint32).ravel()
            ns = sm.size
        if spans is not None:
            sc, sb, se = (_i32(x).ravel() for x in spans[:3])
            sq = np.ascontiguousarray(spans[3], dtype=np.uint32).ravel()
            nq = sc.size
            if not (sb.size == nq and se.size == nq and sq.size == nq):
                raise ValueError("max_marginals: the span arrays differ in length")
        rows = max(n - n0, 1)
        width = ns if 1 <= ns <= 32 else 1  # (the library refuses any other number of sets: the buffers only need a size)
        out = {"best": np.zeros(max(nc, 1), dtype=np.float64)}
        if want_through:
            out["through"] = np.zeros((rows, L), dtype=np.float64)
        if sets is not None and want_inside:
            out["inside"] = np.zeros((rows, width), dtype=np.float64)
        if sets is not None and want_outside:
            out["outside"] = np.zeros((rows, width), dtype=np.float64)
        if spans is not None and want_span_best:
            out["span_best"] = np.zeros(max(nq, 1), dtype=np.float64)
        if spans is not None and want_span_broken:
            out["span_broken"] = np.zeros(max(nq, 1), dtype=np.float64)
        if want_lognorm:
            out["lognorm"] = np.zeros(max(nc, 1), dtype=np.float64)
        ptr = {k: _ptr(v, _c_f64p) for k, v in out.items()}
        pad_i, pad_u = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
        span_args = [None, None, None, None] if spans is None else [
            _ptr(sc if nq else pad_i, _c_i32p), _ptr(sb if nq else pad_i, _c_i32p), _ptr(se if nq else pad_i, _c_i32p),
            _ptr(sq if nq else pad_u, _c_u32p)]
        _check(self._lib.gecco_crf_max_marginals(
            *head, values, allowed, None if sm is None else _ptr(sm if ns else pad_u, _c_u32p), ns, *span_args, nq,
            ptr.get("through"), ptr.get("inside"), ptr.get("outside"), ptr.get("span_best"), ptr.get("span_broken"), ptr["best"],
            ptr.get("lognorm")))
        size = {"through": n - n0, "inside": n - n0, "outside": n - n0, "span_best": nq, "span_broken": nq, "best": nc, "lognorm": nc}
        return {k: v[:size[k]] for k, v in out.items()}

    def viterbi_min_run(self, contig_ptr, gene_ptr, attr_id, set_mask, min_run, device=0, values=None, allowed=None,
                        want_lognorm=True):
        """The best label path of every contig among those whose every maximal run of labels of a set has at least ``min_run``
        genes (``gecco_crf_viterbi_min_run``), 1 <= min_run <= 32; ``set_mask`` has bit y set when label y is in the set.
        Returns ``(y, score, lognorm_min_run, lognorm)``: ``y`` int8 ``[n]`` (-1 at every gene of a contig without a feasible
        path); ``score`` float64 ``[n_contigs]``, the path's left-to-right score (``-inf`` likewise); ``lognorm_min_run``
        ``[n_contigs]``, the log-mass of all feasible paths (``-inf`` where there is none); ``lognorm`` ``[n_contigs]`` as
        ``marginals_full`` gives it -- so ``exp(lognorm_min_run - lognorm)`` is the probability that no run is shorter than
        ``min_run`` and ``exp(score - lognorm)`` the path's.  With ``want_lognorm=False`` the last two are None and the
        sum-semiring launch does not run; ``y`` and ``score`` are the same bytes either way.  Ties go by the kernel's scan
        order over expanded states (include/gecco_crf.h), which at ``min_run = 1`` is ``viterbi``'s rule.  ``values`` and
        ``allowed`` as in ``marginals_full``.  A contig without genes has score 0 and 0 for both log Z."""
        min_run, set_mask = operator.index(min_run), operator.index(set_mask)
        if not 0 <= set_mask < 1 << 32:
            raise ValueError(f"viterbi_min_run: set_mask {set_mask} is outside 0 .. 2**32 - 1")
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        y = np.zeros(max(n - n0, 1), dtype=np.int8)
        score = np.zeros(max(nc, 1), dtype=np.float64)
        ln_c = np.zeros(max(nc, 1), dtype=np.float64) if want_lognorm else None
        ln = np.zeros(max(nc, 1), dtype=np.float64) if want_lognorm else None
        _check(self._lib.gecco_crf_viterbi_min_run(
            *head, values, allowed, set_mask, min_run, _ptr(y, _c_i8p), _ptr(score, _c_f64p),
            None if ln_c is None else _ptr(ln_c, _c_f64p), None if ln is None else _ptr(ln, _c_f64p)))
        return y[:n - n0], score[:nc], (None if ln_c is None else ln_c[:nc]), (None if ln is None else ln[:nc])

    def marginals_min_run(self, contig_ptr, gene_ptr, attr_id, set_mask, min_run, device=0, values=None, allowed=None,
                          want_marginals=True, want_inside=True):
        """The marginals of every gene among the paths ``viterbi_min_run`` decodes over: those whose every maximal run of labels
        of a set has at least ``min_run`` genes (``gecco_crf_marginals_min_run``), 1 <= min_run <= 32; ``set_mask`` has bit y
        set when label y is in the set.  Returns ``(marg, inside, lognorm_min_run, lognorm)``: ``marg`` float64 ``[n, L]``,
        P(gene has label | x, the constraint), or None with ``want_marginals=False``; ``inside`` ``[n]``, the sum of ``marg``
        over the labels of the set, or None with ``want_inside=False`` (the same bytes whether ``marg`` is asked for or not;
        without it 8 bytes per gene come back); ``lognorm_min_run`` ``[n_contigs]``, ``viterbi_min_run``'s bits; ``lognorm``
        ``[n_contigs]`` as ``marginals_full`` gives it.  A disallowed (gene, label) pair has exactly 0.0; a contig without a
        feasible path has 0.0 at every gene and ``lognorm_min_run`` ``-inf``; a contig without genes has 0 for both log Z.
        ``values`` and ``allowed`` as in ``marginals_full``."""
        min_run, set_mask = operator.index(min_run), operator.index(set_mask)
        if not 0 <= set_mask < 1 << 32:
            raise ValueError(f"marginals_min_run: set_mask {set_mask} is outside 0 .. 2**32 - 1")
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        marg = np.zeros((max(n - n0, 1), self.num_labels), dtype=np.float64) if want_marginals else None
        inside = np.zeros(max(n - n0, 1), dtype=np.float64) if want_inside else None
        ln_c = np.zeros(max(nc, 1), dtype=np.float64)
        ln = np.zeros(max(nc, 1), dtype=np.float64)
        _check(self._lib.gecco_crf_marginals_min_run(
            *head, values, allowed, set_mask, min_run, None if marg is None else _ptr(marg, _c_f64p),
            None if inside is None else _ptr(inside, _c_f64p), _ptr(ln_c, _c_f64p), _ptr(ln, _c_f64p)))
        return (None if marg is None else marg[:n - n0]), (None if inside is None else inside[:n - n0]), ln_c[:nc], ln[:nc]

    def ring(self, contig_ptr, gene_ptr, attr_id, device=0, values=None, allowed=None, want_path=True, want_marginals=True):
        """Every contig of the batch as a RING, whose last gene has a transition into its first (``gecco_crf_ring``).  Returns a
        dict that holds only what was asked for: ``"lognorm"`` float64 ``[n_contigs]``, log Z of the ring (always);
        ``"labels"`` int8 ``[n]`` and ``"score"`` float64 ``[n_contigs]`` (``want_path``), the ring's best path and its score,
        closing edge included -- -1 at every gene and ``-inf`` for a ring without a feasible path; ``"marginals"`` float64
        ``[n, L]`` (``want_marginals``), P(gene has label | x) on the ring, exactly 0.0 at a disallowed pair.  What is not asked
        for is neither computed nor stored on the device, and changes no byte of the rest.  Ties: the smaller start label, then
        ``viterbi``'s rule.  ``values`` and ``allowed`` as in ``marginals_full``.  A ring without genes has log Z 0 and score
        0."""
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        out = {"lognorm": np.zeros(max(nc, 1), dtype=np.float64)}
        y = score = marg = None
        if want_path:
            y = out["labels"] = np.zeros(max(n - n0, 1), dtype=np.int8)
            score = out["score"] = np.zeros(max(nc, 1), dtype=np.float64)
        if want_marginals:
            marg = out["marginals"] = np.zeros((max(n - n0, 1), self.num_labels), dtype=np.float64)
        _check(self._lib.gecco_crf_ring(
            *head, values, allowed, None if y is None else _ptr(y, _c_i8p), None if score is None else _ptr(score, _c_f64p),
            None if marg is None else _ptr(marg, _c_f64p), _ptr(out["lognorm"], _c_f64p)))
        size = {"lognorm": nc, "labels": n - n0, "score": nc, "marginals": n - n0}
        return {k: v[:size[k]] for k, v in out.items()}

    @staticmethod
    def _length_model(who, set_mask, length_scores, tail):
        """(set_mask, M, the table as a contiguous float64 array, tail): the shapes only -- the library checks the values."""
        set_mask = operator.index(set_mask)
        if not 0 <= set_mask < 1 << 32:
            raise ValueError(f"{who}: set_mask {set_mask} is outside 0 .. 2**32 - 1")
        g = np.ascontiguousarray(length_scores, dtype=np.float64)
        if g.ndim != 1:
            raise ValueError(f"{who}: length_scores is a one-dimensional table, got shape {g.shape}")
        M = int(g.size)
        if M == 0:  # (the library names the range; the pointer only has to be valid)
            g = np.zeros(1, dtype=np.float64)
        return set_mask, M, g, float(tail)

    def viterbi_run_length(self, contig_ptr, gene_ptr, attr_id, set_mask, length_scores, tail=0.0, device=0, values=None,
                           allowed=None, want_lognorm=True):
        """The best label path of every contig under run-length potentials (``gecco_crf_viterbi_run_length``): every maximal
        run of n genes with labels of the set (``set_mask`` has bit y set when label y is in it) adds ``length_scores[min(n, M)
        - 1] + tail * max(n - M, 0)`` to the path's score, M = ``len(length_scores)``, 1 <= M <= 32; an entry is finite or
        ``-inf``, and ``-inf`` forbids what it scores.  Returns ``(y, score, lognorm_run_length, lognorm)``: ``y`` int8 ``[n]``
        (-1 at every gene of a contig without a feasible path); ``score`` float64 ``[n_contigs]``, the path's score with its
        length terms (``-inf`` likewise); ``lognorm_run_length`` ``[n_contigs]``, the log-mass of all paths under that score;
        ``lognorm`` as ``marginals_full`` gives it.  With ``want_lognorm=False`` the last two are None and the sum-semiring
        launch does not run; ``y`` and ``score`` are the same bytes either way.  Zeros decode the plain lattice; ``(-inf, ...,
        -inf, 0)`` is ``viterbi_min_run``; ``tail=-inf`` is a maximum run length.  Ties go by the kernel's scan order over
        expanded states (include/gecco_crf.h).  ``values`` and ``allowed`` as in ``marginals_full``."""
        set_mask, M, g, tail = self._length_model("viterbi_run_length", set_mask, length_scores, tail)
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        y = np.zeros(max(n - n0, 1), dtype=np.int8)
        score = np.zeros(max(nc, 1), dtype=np.float64)
        ln_g = np.zeros(max(nc, 1), dtype=np.float64) if want_lognorm else None
        ln = np.zeros(max(nc, 1), dtype=np.float64) if want_lognorm else None
        _check(self._lib.gecco_crf_viterbi_run_length(
            *head, values, allowed, set_mask, M, _ptr(g, _c_f64p), tail, _ptr(y, _c_i8p), _ptr(score, _c_f64p),
            None if ln_g is None else _ptr(ln_g, _c_f64p), None if ln is None else _ptr(ln, _c_f64p)))
        return y[:n - n0], score[:nc], (None if ln_g is None else ln_g[:nc]), (None if ln is None else ln[:nc])

    def marginals_run_length(self, contig_ptr, gene_ptr, attr_id, set_mask, length_scores, tail=0.0, device=0, values=None,
                             allowed=None, want_marginals=True, want_inside=True, want_counts=True):
        """The marginals and the expected run-length counts under the length model of ``viterbi_run_length``
        (``gecco_crf_marginals_run_length``; the same model arguments).  Returns ``(marg, inside, counts, lognorm_run_length,
        lognorm)``: ``marg`` float64 ``[n, L]``; ``inside`` ``[n]``, its sum over the labels of the set; ``counts``
        ``[n_contigs, M + 1]``, column d - 1 the expected number of runs with min(length, M) = d and column M the expected
        number of genes beyond the M-th of their runs -- the derivatives of ``lognorm_run_length`` by the table and the tail;
        each is None when not asked for, and asking for one changes no byte of another.  ``lognorm_run_length``
        ``[n_contigs]`` has ``viterbi_run_length``'s bits.  A contig without a feasible path has 0.0 everywhere and ``-inf``;
        a contig without genes 0 for both log Z and zeros in ``counts``."""
        set_mask, M, g, tail = self._length_model("marginals_run_length", set_mask, length_scores, tail)
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        marg = np.zeros((max(n - n0, 1), self.num_labels), dtype=np.float64) if want_marginals else None
        inside = np.zeros(max(n - n0, 1), dtype=np.float64) if want_inside else None
        counts = np.zeros((max(nc, 1), M + 1), dtype=np.float64) if want_counts else None
        ln_g = np.zeros(max(nc, 1), dtype=np.float64)
        ln = np.zeros(max(nc, 1), dtype=np.float64)
        opt = lambda a: None if a is None else _ptr(a, _c_f64p)  # noqa: E731
        _check(self._lib.gecco_crf_marginals_run_length(
            *head, values, allowed, set_mask, M, _ptr(g, _c_f64p), tail, opt(marg), opt(inside), opt(counts), _ptr(ln_g, _c_f64p),
            _ptr(ln, _c_f64p)))
        return (None if marg is None else marg[:n - n0]), (None if inside is None else inside[:n - n0]), \
            (None if counts is None else counts[:nc]), ln_g[:nc], ln[:nc]

    def run_counts(self, contig_ptr, gene_ptr, attr_id, set_mask, max_runs, device=0, values=None, allowed=None,
                   want_log_mass=True, want_paths=True, want_lognorm=True):
        """How many maximal runs of labels of a set every contig holds, and the best path of every count
        (``gecco_crf_run_counts``), 1 <= max_runs <= 32 = K; ``set_mask`` has bit y set when label y is in the set.  Returns
        ``(log_mass, score, y, lognorm)``: ``log_mass`` float64 ``[n_contigs, K + 1]``, column k the log-mass of the paths with
        exactly k runs and the last column that of the paths with at least K (None with ``want_log_mass=False``: the
        sum-semiring launch does not run); ``score`` ``[n_contigs, K + 1]``, the left-to-right score of the best path of every
        column, and ``y`` int8 ``[K + 1, n]``, its labels (both None with ``want_paths=False``: the max-semiring launch and the
        backtrack do not run); ``lognorm`` ``[n_contigs]`` as ``marginals_full`` gives it (None with ``want_lognorm=False``).
        A count that no path has gives ``-inf`` twice and -1 at every gene of its plane.  ``log_mass - logsumexp(log_mass,
        axis=1)`` is log P(count | x); ``score - lognorm[:, None]`` a path's log-probability.  Either output has the same bytes
        whether the other is asked for or not.  ``values`` and ``allowed`` as in ``marginals_full``.  A contig without genes
        has 0 in column 0 of ``log_mass`` and ``score``, ``-inf`` in the others, and ``lognorm`` 0."""
        max_runs, set_mask = operator.index(max_runs), operator.index(set_mask)
        if not 0 <= set_mask < 1 << 32:
            raise ValueError(f"run_counts: set_mask {set_mask} is outside 0 .. 2**32 - 1")
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        k1 = (max_runs if 1 <= max_runs <= 32 else 1) + 1  # (the library refuses any other max_runs: the buffers only need a size)
        mass = np.zeros((max(nc, 1), k1), dtype=np.float64) if want_log_mass else None
        score = np.zeros((max(nc, 1), k1), dtype=np.float64) if want_paths else None
        y = np.zeros((k1, n - n0), dtype=np.int8) if want_paths else None
        ln = np.zeros(max(nc, 1), dtype=np.float64) if want_lognorm else None
        _check(self._lib.gecco_crf_run_counts(
            *head, values, allowed, set_mask, max_runs, None if mass is None else _ptr(mass, _c_f64p),
            None if score is None else _ptr(score, _c_f64p), None if y is None or y.size == 0 else _ptr(y, _c_i8p),
            None if ln is None else _ptr(ln, _c_f64p)))
        return (None if mass is None else mass[:nc]), (None if score is None else score[:nc]), y, (None if ln is None else ln[:nc])

    def edge_posteriors(self, contig_ptr, gene_ptr, attr_id, sets=None, want_pair=False, want_transitions=True, want_entropy=True,
                        want_marginals=False, device=0, values=None, allowed=None):
        """Edge posteriors of the whole-contig lattice (``gecco_crf_edge_posteriors``), behind ONE forward-backward pass of the
        batch.  Returns a dict that holds only what was asked for -- nothing else is allocated, computed or copied:
        ``"pair"`` (``want_pair``) float64 ``[n, L, L]``, ``pair[g, i, j] = P(y_{g-1} = i, y_g = j | x)``, zeros at a contig's
        first gene -- 8 L^2 bytes per gene, 8 KB at 32 labels;
        ``"enter"``, ``"leave"`` (``sets``: 1 to 32 uint32 masks, bit y set when label y is in the set) float64
        ``[n, n_sets]``: the probability that a run of labels of the set starts / ends at the gene;
        ``"transitions"`` (``want_transitions``) ``[n_contigs, L, L]``: the expected number of (i, j) transitions of a contig;
        ``"entropy"`` (``want_entropy``) ``[n_contigs]``: the entropy of the contig's path distribution in nats;
        ``"marginals"`` ``[n, L]`` and ``"lognorm"`` ``[n_contigs]`` (``want_marginals``) as ``marginals_full`` gives them.
        ``values`` and ``allowed`` as in ``marginals_full``: with ``allowed`` the lattice is the restricted one."""
        head, values, allowed, n, n0, nc = self._csr_head(contig_ptr, gene_ptr, attr_id, values, allowed, int(device))
        L = self.num_labels
        ns = 0
        if sets is not None:
            sm = np.ascontiguousarray(sets, dtype=np.uint32).ravel()
            ns = sm.size
        rows = max(n - n0, 1)
        width = ns if 1 <= ns <= 32 else 1  # (the library refuses any other number of sets: the buffers only need a size)
        out = {}
        if want_pair:
            out["pair"] = np.zeros((rows, L, L), dtype=np.float64)
        if sets is not None:
            out["enter"] = np.zeros((rows, width), dtype=np.float64)
            out["leave"] = np.zeros((rows, width), dtype=np.float64)
        if want_transitions:
            out["transitions"] = np.zeros((max(nc, 1), L, L), dtype=np.float64)
        if want_entropy:
            out["entropy"] = np.zeros(max(nc, 1), dtype=np.float64)
        if want_marginals:
            out["marginals"] = np.zeros((rows, L), dtype=np.float64)
            out["lognorm"] = np.zeros(max(nc, 1), dtype=np.float64)
        ptr = {k: _ptr(v, _c_f64p) for k, v in out.items()}
        _check(self._lib.gecco_crf_edge_posteriors(
            *head, values, allowed, _ptr(sm if ns else np.zeros(1, dtype=np.uint32), _c_u32p) if sets is not None else None, ns,
            ptr.get("pair"), ptr.get("enter"), ptr.get("leave"), ptr.get("transitions"), ptr.get("entropy"), ptr.get("marginals"),
            ptr.get("lognorm")))
        per_gene = ("pair", "enter", "leave", "marginals")
        return {k: v[:n - n0] if k in per_gene else v[:nc] for k, v in out.items()}


def domain_composition(seg, dom_ptr, dom_col, dom_weight, n_cols, normalize=True, device=0) -> np.ndarray:
    """Dense (n_seg, n_cols) weighted domain compositions of the clusters in `seg` (gecco_crf_domain_composition)."""
    lib = load_library()
    seg = np.ascontiguousarray(seg, dtype=np.int32).reshape(-1, 4)
    dom_ptr, dom_col = _i32(dom_ptr), _i32(dom_col)
    dom_weight = np.ascontiguousarray(dom_weight, dtype=np.float64)
    if dom_col.size == 0:
        dom_col, dom_weight = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float64)
    out = np.zeros((len(seg), int(n_cols)), dtype=np.float64)
    seg_buf = seg if len(seg) else np.zeros((1, 4), dtype=np.int32)
    out_buf = out if out.size else np.zeros(1, dtype=np.float64)
    _check(lib.gecco_crf_domain_composition(
        device, _ptr(seg_buf, _c_i32p), len(seg), _ptr(dom_ptr, _c_i32p), len(dom_ptr) - 1, _ptr(dom_col, _c_i32p),
        _ptr(dom_weight, _c_f64p), int(n_cols), int(bool(normalize)), _ptr(out_buf, _c_f64p)))
    return out


def _addr(a: np.ndarray):
    return a.ctypes.data if a.size else None


def cluster_overlaps(gene_seq, gene_start, gene_end, cluster_ptr, cluster_start, cluster_end, device=0):
    """The interval join of genes and clusters (gecco_crf_cluster_overlaps): ``(labels, member_ptr, member_gene)``.

    Genes are grouped by sequence code (codes ``0 <= c < len(cluster_ptr) - 1``, non-decreasing) and sorted by start inside
    a sequence; the clusters of sequence s are rows ``cluster_ptr[s]:cluster_ptr[s + 1]`` of ``cluster_start`` /
    ``cluster_end``, sorted by start.  ``labels[g]`` (uint8) is 1 where gene g overlaps any cluster of its sequence, bounds
    inclusive; ``member_gene[member_ptr[k]:member_ptr[k + 1]]`` are the genes of cluster k in gene order."""
    lib = load_library()
    seq = np.ascontiguousarray(gene_seq, dtype=np.int32)
    start = np.ascontiguousarray(gene_start, dtype=np.int64)
    end = np.ascontiguousarray(gene_end, dtype=np.int64)
    cptr = np.ascontiguousarray(cluster_ptr, dtype=np.int32)
    cs = np.ascontiguousarray(cluster_start, dtype=np.int64)
    ce = np.ascontiguousarray(cluster_end, dtype=np.int64)
    n, n_seqs = len(seq), len(cptr) - 1
    if len(start) != n or len(end) != n:
        raise ValueError("cluster_overlaps: gene_seq, gene_start and gene_end differ in length")
    if n_seqs < 0 or int(cptr[-1]) != len(cs) or len(ce) != len(cs):
        raise ValueError("cluster_overlaps: cluster_ptr[-1] must be the number of clusters")
    m = len(cs)
    labels = np.zeros(n, dtype=np.uint8)
    member_ptr = np.zeros(m + 1, dtype=np.int32)
    members = np.zeros(n + 64, dtype=np.int32)  # (a gene is usually in one cluster at most: one retry otherwise)
    count = ctypes.c_int64(0)
    for _ in range(2):
        rc = lib.gecco_crf_cluster_overlaps(int(device), n, _addr(seq), _addr(start), _addr(end), n_seqs, cptr.ctypes.data,
                                            _addr(cs), _addr(ce), _addr(labels), member_ptr.ctypes.data, members.ctypes.data,
                                            len(members), ctypes.byref(count))
        if rc == EINVAL and count.value > len(members):
            members = np.zeros(count.value, dtype=np.int32)
            continue
        _check(rc)
        break
    return labels, member_ptr, members[:count.value].copy()


def domain_composition_members(member_ptr, member_gene, dom_ptr, dom_col, dom_weight, n_cols, normalize=True,
                               device=0) -> np.ndarray:
    """Dense (n_clusters, n_cols) weighted domain compositions of clusters given as member lists
    (gecco_crf_domain_composition_members): cluster k is the genes ``member_gene[member_ptr[k]:member_ptr[k + 1]]`` in
    that order, gene g the domain rows ``dom_ptr[g]:dom_ptr[g + 1]``; the bits of ``domain_composition`` on the
    concatenated rows."""
    lib = load_library()
    mptr, mgene, dptr, dcol = _i32(member_ptr), _i32(member_gene), _i32(dom_ptr), _i32(dom_col)
    dw = np.ascontiguousarray(dom_weight, dtype=np.float64)
    if len(dcol) != int(dptr[-1]) or len(dw) != len(dcol):
        raise ValueError("domain_composition_members: dom_ptr[-1] must be the number of domain rows")
    k = len(mptr) - 1
    out = np.zeros((k, int(n_cols)), dtype=np.float64)
    _check(lib.gecco_crf_domain_composition_members(int(device), mptr.ctypes.data, k, _addr(mgene), dptr.ctypes.data,
                                                    len(dptr) - 1, _addr(dcol), _addr(dw), int(n_cols), int(bool(normalize)),
                                                    _addr(out)))
    return out


class RefineParams(ctypes.Structure):
    """``gecco_crf_refine_params``: ClusterRefiner's parameters (gecco/refine.py:75-116)."""
    _fields_ = [("threshold", ctypes.c_double), ("average_threshold", ctypes.c_double), ("criterion", ctypes.c_int32),
                ("n_cds", ctypes.c_int32), ("n_biopfams", ctypes.c_int32), ("edge_distance", ctypes.c_int32),
                ("trim", ctypes.c_int32), ("carry_state", ctypes.c_int32), ("marker_ptr", _vp), ("marker_id", _vp)]


CRITERIA = {"gecco": 0, "antismash": 1}


def refine_params(criterion="gecco", threshold=0.8, n_cds=5, n_biopfams=5, average_threshold=0.6, edge_distance=0, trim=True,
                  carry_state=False, marker_ptr=None, marker_id=None, keep=None) -> RefineParams:
    """The C struct; `marker_ptr` / `marker_id` are host int32 arrays (parked in `keep`) or integer device addresses."""
    if criterion not in CRITERIA:
        raise ValueError(f"Unknown cluster filtering criterion: {criterion}")  # refine.py:165
    q = RefineParams(float(threshold), float(average_threshold), CRITERIA[criterion], int(n_cds), int(n_biopfams),
                     int(edge_distance), int(bool(trim)), int(bool(carry_state)), None, None)
    for name, arr in (("marker_ptr", marker_ptr), ("marker_id", marker_id)):
        if arr is None:
            continue
        if isinstance(arr, int):
            setattr(q, name, arr or None)
            continue
        a = _i32(arr)
        if a.size == 0:
            a = np.zeros(1, dtype=np.int32)
        if keep is not None:
            keep.append(a)
        setattr(q, name, a.ctypes.data)
    return q


def segment(p, annotated, contig_ptr, threshold=0.8, n_cds=3, edge_distance=0, trim=True, device=0,
            carry_state=False, criterion="gecco", n_biopfams=5, average_threshold=0.6, marker_ptr=None,
            marker_id=None) -> np.ndarray:
    """Cluster rows (contig, number, first gene, last gene + 1) of per-gene probabilities.  `carry_state`:
    False = one grouper per contig (the CLI's ``iter_clusters`` call per contig), True = one grouper
    over all contigs (a single ``iter_clusters`` call).  `criterion="antismash"` needs the genes' marker domains
    (`marker_ptr[n_genes+1]`, `marker_id`: indices into the caller's marker list, refine.py:157-163)."""
    lib = load_library()
    p = np.ascontiguousarray(p, dtype=np.float64)
    annotated = np.ascontiguousarray(annotated, dtype=np.uint8)
    contig_ptr = _i32(contig_ptr)
    cap = max(1, len(p))
    seg = np.zeros((cap, 4), dtype=np.int32)
    n_seg = ctypes.c_int32(0)
    keep = []
    q = refine_params(criterion, threshold, n_cds, n_biopfams, average_threshold, edge_distance, trim, carry_state, marker_ptr,
                      marker_id, keep)
    _check(lib.gecco_crf_segment_ex(device, _ptr(p, _c_f64p), _ptr(annotated, _c_u8p), _ptr(contig_ptr, _c_i32p),
                                    len(contig_ptr) - 1, ctypes.byref(q), _ptr(seg, _c_i32p), cap, ctypes.byref(n_seg)))
    return seg[: n_seg.value].copy()


# ---- columnar host side (gecco_crf_pack_columns / gecco_crf_cluster_rows_build) ----------------------
class _Strings(ctypes.Structure):
    _fields_ = [("data", _vp), ("offsets", _vp)]


class _TableColumns(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("sequence_id", _Strings), ("protein_id", _Strings), ("domain", _Strings),
                ("start", _vp), ("domain_start", _vp), ("n_genes", ctypes.c_int64), ("gene_sequence_id", _Strings),
                ("gene_protein_id", _Strings), ("gene_start", _vp), ("n_markers", ctypes.c_int64), ("markers", _Strings)]


def _view(ptr, n, dtype, owner):
    """numpy view over `n` items of library-owned memory; `owner` (the handle wrapper) is kept alive by it."""
    n = int(n)
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    buf._owner = owner
    return np.frombuffer(buf, dtype=dtype, count=n)


def _strings_arg(col, keep):
    """(data uint8, offsets int64) of a string column -> the C struct; arrays are parked in `keep`."""
    data = np.ascontiguousarray(col.data, dtype=np.uint8)
    off = np.ascontiguousarray(col.offsets, dtype=np.int64)
    if data.size == 0:
        data = np.zeros(1, dtype=np.uint8)
    keep.extend((data, off))
    return _Strings(data.ctypes.data, off.ctypes.data)


def _i64_arg(a, keep):
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a.size == 0:
        a = np.zeros(1, dtype=np.int64)
    keep.append(a)
    return a.ctypes.data


class PackedTables:
    """CSR batch + row bookkeeping of a feature table (and gene table), built by `gecco_crf_pack_columns`.
    The arrays are views of library-owned memory (pinned when a device is present)."""

    def __init__(self, model: "Model", f_sequence_id, f_protein_id, f_start, f_domain, f_domain_start,
                 g_sequence_id=None, g_protein_id=None, g_start=None, markers=None):
        self._lib = load_library()
        keep = []
        t = _TableColumns()
        t.n_rows = len(f_protein_id)
        t.sequence_id = _strings_arg(f_sequence_id, keep)
        t.protein_id = _strings_arg(f_protein_id, keep)
        t.domain = _strings_arg(f_domain, keep)
        t.start = _i64_arg(f_start, keep)
        t.domain_start = _i64_arg(f_domain_start, keep)
        t.n_genes = 0 if g_protein_id is None else len(g_protein_id)
        if g_protein_id is not None:
            t.gene_sequence_id = _strings_arg(g_sequence_id, keep)
            t.gene_protein_id = _strings_arg(g_protein_id, keep)
            t.gene_start = _i64_arg(g_start, keep)
        t.n_markers = 0 if markers is None else len(markers)
        if t.n_markers:
            t.markers = _strings_arg(markers, keep)
        self._cols, self._keep = t, keep  # the cluster-row builder reads the same columns again
        h = _vp()
        _check(self._lib.gecco_crf_pack_columns(model._h, ctypes.byref(t), ctypes.byref(h)))
        self._h = h
        ng, nc, dup, unl, pin = (ctypes.c_int32(0) for _ in range(5))
        nnz = ctypes.c_int64(0)
        _check(self._lib.gecco_crf_packed_info(h, ctypes.byref(ng), ctypes.byref(nc), ctypes.byref(nnz), ctypes.byref(dup),
                                               ctypes.byref(unl), ctypes.byref(pin)))
        self.n_genes, self.n_contigs, self.nnz = ng.value, nc.value, nnz.value
        self.n_rows = int(t.n_rows)
        self.n_duplicate_gene_ids, self.n_unlisted_proteins, self.pinned = dup.value, unl.value, bool(pin.value)
        L = self._lib
        self.contig_ptr = _view(L.gecco_crf_packed_contig_ptr(h), self.n_contigs + 1, np.int32, self)
        self.gene_ptr = _view(L.gecco_crf_packed_gene_ptr(h), self.n_genes + 1, np.int32, self)
        self.attr_id = _view(L.gecco_crf_packed_attr_id(h), self.nnz, np.int32, self)
        self.annotated = _view(L.gecco_crf_packed_annotated(h), self.n_genes, np.uint8, self)
        self.gene_row = _view(L.gecco_crf_packed_gene_row(h), self.n_genes, np.int64, self)
        self.row_gene = _view(L.gecco_crf_packed_row_gene(h), self.n_rows, np.int32, self)
        self.row_order = _view(L.gecco_crf_packed_row_order(h), self.n_rows, np.int64, self)
        self.row_ptr = _view(L.gecco_crf_packed_row_ptr(h), self.n_genes + 1, np.int64, self)
        self.marker_ptr = self.marker_id = None  # per gene its marker domains (antismash criterion), when asked for
        if t.n_markers:
            self.marker_ptr = _view(L.gecco_crf_packed_marker_ptr(h), self.n_genes + 1, np.int32, self)
            if self.n_genes == 0:
                self.marker_ptr = np.zeros(1, dtype=np.int32)
            self.marker_id = _view(L.gecco_crf_packed_marker_id(h), int(self.marker_ptr[-1]), np.int32, self)
        if self.n_contigs == 0:
            self.contig_ptr = np.zeros(1, dtype=np.int32)
        if self.n_genes == 0:
            self.gene_ptr = np.zeros(1, dtype=np.int32)
            self.row_ptr = np.zeros(1, dtype=np.int64)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.gecco_crf_packed_free(h)

    def order_info(self, gene_start: np.ndarray, gene_end: np.ndarray):
        """(rows_in_order, refiner_order_differs) from the gene table's `start` / `end` columns (`gecco_crf_packed_order_info`):
        whether the genes in scoring order are the gene table's rows 0 .. n - 1, and whether the refiner's (start, end) order
        differs from the scoring order somewhere (equal starts with decreasing ends)."""
        gs = np.ascontiguousarray(gene_start, dtype=np.int64)
        ge = np.ascontiguousarray(gene_end, dtype=np.int64)
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        _check(self._lib.gecco_crf_packed_order_info(self._h, gs.ctypes.data, ge.ctypes.data, min(gs.size, ge.size), ctypes.byref(a),
                                                     ctypes.byref(b)))
        return bool(a.value), bool(b.value)

    def cluster_rows(self, seg, seg_p, seg_off, gene_end, feature_end) -> dict:
        """Columns of clusters.tsv for `seg` rows: dict of numpy arrays and (data, offsets) string columns."""
        seg = np.ascontiguousarray(seg, dtype=np.int32).reshape(-1, 4)
        seg_p = np.ascontiguousarray(seg_p, dtype=np.float64)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        keep = []
        h = _vp()
        k = len(seg)
        segb = seg if k else np.zeros((1, 4), dtype=np.int32)
        spb = seg_p if seg_p.size else np.zeros(1, dtype=np.float64)
        _check(self._lib.gecco_crf_cluster_rows_build(
            self._h, ctypes.byref(self._cols), _i64_arg(gene_end if gene_end is not None else [], keep),
            _i64_arg(feature_end if feature_end is not None else [], keep), _ptr(segb, _c_i32p), k, _ptr(spb, _c_f64p),
            seg_off.ctypes.data, ctypes.byref(h)))
        try:
            L = self._lib
            out = {
                "start": _view(L.gecco_crf_cluster_rows_start(h), k, np.int64, None).copy(),
                "end": _view(L.gecco_crf_cluster_rows_end(h), k, np.int64, None).copy(),
                "average_p": _view(L.gecco_crf_cluster_rows_average_p(h), k, np.float64, None).copy(),
                "max_p": _view(L.gecco_crf_cluster_rows_max_p(h), k, np.float64, None).copy(),
            }
            for which, name in enumerate(("sequence_id", "cluster_id", "proteins", "domains")):
                d, o = _vp(), _vp()
                _check(L.gecco_crf_cluster_rows_strings(h, which, ctypes.byref(d), ctypes.byref(o)))
                off = _view(o.value, k + 1, np.int64, None).copy()
                out[name] = (_view(d.value, int(off[-1]) if k else 0, np.uint8, None).copy(), off)
        finally:
            self._lib.gecco_crf_cluster_rows_free(h)
        return out


def tsv_format(header: str, columns) -> bytes:
    """TSV text of `columns` (each a (data uint8, offsets int64) string column, an int64 array or a float64 array)
    below `header`: floats as Python's repr() writes them, NaN as an empty field (`gecco_crf_tsv_format`)."""
    lib = load_library()
    keep, kinds, data, offs = [], [], [], []
    n_rows = None
    for col in columns:
        if isinstance(col, tuple):
            d = np.ascontiguousarray(col[0], dtype=np.uint8)
            o = np.ascontiguousarray(col[1], dtype=np.int64)
            if d.size == 0:
                d = np.zeros(1, dtype=np.uint8)
            keep.extend((d, o))
            kinds.append(0)
            data.append(d.ctypes.data)
            offs.append(o.ctypes.data)
            n = len(o) - 1
        else:
            a = np.asarray(col)
            a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype.kind == "f" else np.int64)
            if a.size == 0:
                a = np.zeros(1, dtype=a.dtype)
            keep.append(a)
            kinds.append(2 if a.dtype.kind == "f" else 1)
            data.append(a.ctypes.data)
            offs.append(None)
            n = len(np.asarray(col))
        if n_rows is None:
            n_rows = n
        elif n != n_rows:
            raise ValueError("columns of different lengths")
    nc = len(kinds)
    k = np.array(kinds or [0], dtype=np.int32)
    dp = (_vp * max(nc, 1))(*data)
    op = (_vp * max(nc, 1))(*offs)
    out, out_len = _vp(), ctypes.c_int64(0)
    _check(lib.gecco_crf_tsv_format(n_rows or 0, nc, _ptr(k, _c_i32p), dp, op, header.encode("utf-8"), ctypes.byref(out),
                                    ctypes.byref(out_len)))
    try:
        return ctypes.string_at(out.value, out_len.value)
    finally:
        lib.gecco_crf_buffer_free(out)


def gather_f64(src: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """src[idx] on several host threads (`gecco_crf_gather_f64`; idx int32, src float64)."""
    src = np.ascontiguousarray(src, dtype=np.float64)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    out = np.empty(idx.size, dtype=np.float64)
    if idx.size:
        _check(load_library().gecco_crf_gather_f64(src.ctypes.data, src.size, idx.ctypes.data, idx.size, out.ctypes.data))
    return out


def exact_mean(values) -> float:
    """``statistics.mean`` of the non-NaN values (exact sum, one rounding), natively."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.size == 0:
        return float("nan")
    return float(load_library().gecco_crf_exact_mean(_ptr(v, _c_f64p), v.size))


def exp_correctly_rounded(x) -> np.ndarray:
    """The double nearest to exp(x), elementwise (`gecco_crf_exp_correctly_rounded`: what reference-bits mode puts in libm's place)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    if x.size:
        _check(load_library().gecco_crf_exp_correctly_rounded(_ptr(x.reshape(-1), _c_f64p), x.size, _ptr(out.reshape(-1), _c_f64p)))
    return out


class _PinnedBlock:
    """Owner of one gecco_crf_host_alloc block (freed when the last array over it dies)."""

    def __init__(self, nbytes: int):
        self._lib = load_library()
        ptr = _vp()
        _check(self._lib.gecco_crf_host_alloc(max(int(nbytes), 1), ctypes.byref(ptr)))
        self.ptr = ptr.value
        self.nbytes = max(int(nbytes), 1)

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr:
            self._lib.gecco_crf_host_free(ptr)


def pinned_empty(shape, dtype) -> np.ndarray:
    """numpy array over pinned (page-locked, device-visible) host memory: the batch driver copies to
    and from such arrays asynchronously, so uploads, kernels and downloads of a batch overlap."""
    dtype = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    block = _PinnedBlock(n * dtype.itemsize)
    buf = (ctypes.c_char * block.nbytes).from_address(block.ptr)
    buf._pinned_block = block  # numpy keeps `buf` (the buffer exporter) alive, `buf` keeps the block
    return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)


def pinned_copy(a, dtype=None) -> np.ndarray:
    a = np.asarray(a, dtype=dtype)
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


class DecodeStream:
    """The pipelined decode (`gecco_crf_plan_run_decode_pipelined`) over a sequence of resident batches on one HIP stream:
    `submit` enqueues the window marginals of a batch and the Viterbi labels of the batch submitted before it (one launch
    when both qualify), `flush` the labels of the last one.  Two of these on two streams, batches alternating between
    them, keep two launches in flight (bench.py's schedule).  The caller keeps a batch's device arrays alive until the
    next `submit` / `flush` has been enqueued."""

    def __init__(self, stream: int = 0):
        self.stream = stream
        self._prev = None  # (plan, address of its label buffer)

    def submit(self, plan: "Plan", d_gene_ptr: int, d_attr_id: int, d_p_out: int, d_y_out: int, label: int = 1) -> None:
        prev_plan, prev_y = self._prev if self._prev is not None else (None, 0)
        plan.run_decode_pipelined(d_gene_ptr, d_attr_id, d_p_out, prev_plan, prev_y, label, self.stream)
        self._prev = (plan, d_y_out)

    def flush(self) -> None:
        if self._prev is not None:
            self._prev[0].flush_decode_pipelined(self._prev[1], self.stream)
            self._prev = None


def degree_bytes(gene_ptr) -> np.ndarray:
    """The wire format of `Session.windowed_marginals(degree=...)`: domain counts of the genes as bytes."""
    d = np.diff(np.asarray(gene_ptr, dtype=np.int64))
    if d.size and (d.min() < 0 or d.max() > 255):
        raise ValueError("degree bytes need 0 <= domains per gene <= 255")
    return np.ascontiguousarray(d, dtype=np.uint8) if d.size else np.zeros(1, dtype=np.uint8)


class SessionStatsStruct(ctypes.Structure):
    """``gecco_crf_session_stats_t``"""
    _fields_ = [("n_chunks", ctypes.c_int32), ("n_devices", ctypes.c_int32), ("direct", ctypes.c_int32), ("host_threads", ctypes.c_int32),
                ("h2d_bytes", ctypes.c_int64), ("d2h_bytes", ctypes.c_int64), ("host_plan_seconds", ctypes.c_double),
                ("host_issue_seconds", ctypes.c_double), ("wall_seconds", ctypes.c_double)]


class Session:
    """Batch driver over one or several devices (include/gecco_crf.h, `gecco_crf_session_*`): host
    arrays in, host arrays out; contig chunks are dealt to the devices longest-first and pipelined
    (upload / compute / download) on each of them."""

    def __init__(self, model: "Model", devices: Sequence[int] = (0,)):
        self._lib = load_library()
        self.model = model  # the session must not outlive its model
        devs = _i32(list(devices))
        h = _vp()
        _check(self._lib.gecco_crf_session_create(model._h, _ptr(devs, _c_i32p), len(devs), ctypes.byref(h)))
        self._h = h
        self.devices = [int(d) for d in devs]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.gecco_crf_session_free(h)

    def set_chunk_genes(self, genes: int) -> None:
        _check(self._lib.gecco_crf_session_set_chunk_genes(self._h, int(genes)))

    def set_reference_bits(self, on: bool = True) -> None:
        """Windowed marginals in CRFsuite's own operation order with a correctly rounded exp: the reference's output files bit
        for bit, at about six times the fast kernels' time (`gecco_crf_session_set_reference_bits`)."""
        _check(self._lib.gecco_crf_session_set_reference_bits(self._h, int(bool(on))))

    def set_direct_genes(self, genes: int) -> None:
        """Largest batch (genes) that takes the direct path -- one chunk, kernels on pinned host memory, no copy commands
        (`gecco_crf_session_set_direct_genes`; 0: never; -1: the defaults -- every one-chunk batch on a one-device session,
        131 072 genes on a session over several devices, 65 536 for cluster calls)."""
        _check(self._lib.gecco_crf_session_set_direct_genes(self._h, int(genes)))

    def stats(self) -> dict:
        """Figures of the last batch (`gecco_crf_session_stats_ex`)."""
        st = SessionStatsStruct()
        _check(self._lib.gecco_crf_session_stats_ex(self._h, ctypes.addressof(st)))
        return {name: getattr(st, name) for name, _ in SessionStatsStruct._fields_}

    @staticmethod
    def _csr(contig_ptr, gene_ptr, attr_id):
        contig_ptr, gene_ptr, attr_id = _i32(contig_ptr), _i32(gene_ptr), _i32(attr_id)
        if attr_id.size == 0:
            attr_id = np.zeros(1, dtype=np.int32)
        n = int(contig_ptr[-1]) if len(contig_ptr) else 0
        return contig_ptr, gene_ptr, attr_id, n, max(len(contig_ptr) - 1, 0)

    def windowed_marginals(self, contig_ptr, gene_ptr, attr_id, window, step=1, label=1, pad=True, out=None, degree=None):
        """`degree`: the genes' domain counts as uint8 (== numpy.diff(gene_ptr)): they cross PCIe instead of the row pointers
        (gecco_crf_session_windowed_degrees); `degree_bytes(gene_ptr)` makes them."""
        contig_ptr, gene_ptr, attr_id, n, nc = self._csr(contig_ptr, gene_ptr, attr_id)
        if out is None:
            out = np.empty(max(n, 1), dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.size >= n
        if degree is not None:
            assert degree.dtype == np.uint8 and degree.flags.c_contiguous and degree.size >= n
            _check(self._lib.gecco_crf_session_windowed_degrees(self._h, contig_ptr.ctypes.data, nc, gene_ptr.ctypes.data,
                                                                degree.ctypes.data if degree.size else None, attr_id.ctypes.data,
                                                                int(window), int(step), int(label), int(bool(pad)), out.ctypes.data))
            return out[:n]
        _check(self._lib.gecco_crf_session_windowed(self._h, contig_ptr.ctypes.data, nc, gene_ptr.ctypes.data, attr_id.ctypes.data,
                                                    int(window), int(step), int(label), int(bool(pad)), out.ctypes.data))
        return out[:n]

    def decode(self, contig_ptr, gene_ptr, attr_id, window, step=1, label=1, pad=True, out_p=None, out_y=None, degree=None,
               labels=True):
        """Windowed marginals + whole-contig Viterbi labels of a batch in host memory; `out_p` / `out_y`: caller buffers
        (pinned ones make the downloads asynchronous).  The compact wire format (gecco_crf_session_decode_wire): `degree`
        = the genes' domain counts as uint8 (`degree_bytes(gene_ptr)`), sent instead of the row pointers; `attr_id` as a
        uint16 array (a model with at most 65536 attributes) crosses PCIe as it is.  `labels=False`: marginals only
        (returns (p, None))."""
        attr16 = None
        if isinstance(attr_id, np.ndarray) and attr_id.dtype == np.uint16:
            attr16 = np.ascontiguousarray(attr_id) if attr_id.size else np.zeros(1, dtype=np.uint16)
            attr_id = np.zeros(1, dtype=np.int32)
        contig_ptr, gene_ptr, attr_id, n, nc = self._csr(contig_ptr, gene_ptr, attr_id)
        p = np.empty(max(n, 1), dtype=np.float64) if out_p is None else out_p
        y = (np.empty(max(n, 1), dtype=np.int8) if out_y is None else out_y) if labels else None
        assert p.dtype == np.float64 and p.flags.c_contiguous and p.size >= n
        assert y is None or (y.dtype == np.int8 and y.flags.c_contiguous and y.size >= n)
        if degree is not None:
            assert degree.dtype == np.uint8 and degree.flags.c_contiguous and degree.size >= n
        adr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
        _check(self._lib.gecco_crf_session_decode_wire(
            self._h, adr(contig_ptr), nc, adr(gene_ptr), adr(degree), adr(attr_id) if attr16 is None else None, adr(attr16),
            int(window), int(step), int(label), int(bool(pad)), p.ctypes.data, None if y is None else y.ctypes.data))
        return p[:n], (None if y is None else y[:n])

    def clusters(self, contig_ptr, gene_ptr, attr_id, annotated, window, step=1, label=1, pad=True, threshold=0.8, n_cds=3,
                 edge_distance=0, trim=True, want_p=False, want_seg_p=True, p_out=None, criterion="gecco", n_biopfams=5,
                 average_threshold=0.6, marker_ptr=None, marker_id=None, degree=None, seg_p_out=None):
        """Windowed marginals + cluster calls in one pass; the probabilities stay on the device unless
        `want_p` / `p_out`.  Returns (seg rows (k, 4), seg_p, seg_off, p or None): `seg_p[seg_off[i]:seg_off[i+1]]`
        are the probabilities of the genes of row i.  `degree` (uint8, = diff(gene_ptr)): the degree-byte wire format.
        `seg_p_out`: a caller buffer of n doubles for the rows' probabilities (a pinned one is filled by the copy engine at
        full rate; a fresh pageable array costs a page fault per 4 KB); the returned seg_p is then a view of it.
        `attr_id` may be a uint16 array (a model with at most 65536 attributes): it then crosses PCIe as it is."""
        attr16 = None
        if isinstance(attr_id, np.ndarray) and attr_id.dtype == np.uint16:
            attr16 = np.ascontiguousarray(attr_id) if attr_id.size else np.zeros(1, dtype=np.uint16)
            attr_id = np.zeros(1, dtype=np.int32)
        contig_ptr, gene_ptr, attr_id, n, nc = self._csr(contig_ptr, gene_ptr, attr_id)
        if annotated is None:  # (with `degree`: annotated iff the gene has a domain the model knows)
            if degree is None:
                raise ValueError("clusters: `annotated` may only be left out together with `degree`")
        else:
            annotated = np.ascontiguousarray(annotated, dtype=np.uint8)
            if annotated.size == 0:
                annotated = np.zeros(1, dtype=np.uint8)
        if p_out is None and want_p:
            p_out = np.empty(max(n, 1), dtype=np.float64)
        cap = min(n, n // 2 + nc) + 1
        # the row buffers are kept between calls (no 24 MB of fresh pages per batch); a second thread inside this method on the
        # same session takes fresh ones
        held = self.__dict__.pop("_row_buffers", None)
        if held is None or held[0].shape[0] < cap:
            held = (np.empty((cap, 4), dtype=np.int32), np.zeros(cap + 1, dtype=np.int64))
        seg, seg_off = held[0][:cap], held[1][: cap + 1]
        if p_out is not None:
            assert p_out.dtype == np.float64 and p_out.flags.c_contiguous and p_out.size >= n
        if seg_p_out is not None:
            assert seg_p_out.dtype == np.float64 and seg_p_out.flags.c_contiguous and seg_p_out.size >= n
            want_seg_p = True
        seg_p = (seg_p_out if seg_p_out is not None else np.empty(max(n, 1), dtype=np.float64)) if want_seg_p else None
        n_seg = ctypes.c_int32(0)
        keep = []
        q = refine_params(criterion, threshold, n_cds, n_biopfams, average_threshold, edge_distance, trim, False, marker_ptr,
                          marker_id, keep)
        if degree is not None:
            assert degree.dtype == np.uint8 and degree.flags.c_contiguous and degree.size >= n
        adr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        _check(self._lib.gecco_crf_session_clusters_wire(
            self._h, adr(contig_ptr), nc, adr(gene_ptr), adr(degree), adr(attr_id) if attr16 is None else None, adr(attr16),
            adr(annotated), int(window), int(step), int(label), int(bool(pad)), ctypes.addressof(q), adr(p_out), adr(seg), cap,
            ctypes.addressof(n_seg), adr(seg_p) if want_seg_p else None, max(n, 1), adr(seg_off)))
        k = n_seg.value
        # (without seg_p the C side writes no offsets: the reused buffer would show those of an earlier call)
        res = (seg[:k].copy(), ((seg_p[: seg_off[k]] if seg_p_out is not None else seg_p[: seg_off[k]].copy()) if want_seg_p else None),
               (seg_off[: k + 1].copy() if want_seg_p else None),
               (p_out[:n] if p_out is not None else None))
        self._row_buffers = held  # (handed back only now: nobody else wrote into them meanwhile)
        return res


class Plan:
    """Resident batch: contig layout + model tables on one device; bulk arrays stay in
    caller-owned device memory (e.g. torch tensors) and launches go to the caller's stream."""

    def __init__(self, model: Model, contig_ptr, window, step=1, pad=True, device=0):
        self._lib = load_library()
        self.model = model
        contig_ptr = _i32(contig_ptr)
        h = _vp()
        _check(
            self._lib.gecco_crf_plan_create(
                model._h, int(device), _ptr(contig_ptr, _c_i32p), max(len(contig_ptr) - 1, 0), int(window), int(step),
                int(bool(pad)), ctypes.byref(h),
            )
        )
        self._h = h
        self.device = device

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.gecco_crf_plan_free(h)

    @property
    def num_genes(self) -> int:
        return self._lib.gecco_crf_plan_num_genes(self._h)

    @property
    def num_windows(self) -> int:
        return self._lib.gecco_crf_plan_num_windows(self._h)

    @property
    def num_tiles(self) -> int:
        return self._lib.gecco_crf_plan_num_tiles(self._h)

    @property
    def tile_out(self) -> int:
        return self._lib.gecco_crf_plan_tile_out(self._h)

    @property
    def kernel_name(self) -> str:
        return self._lib.gecco_crf_plan_kernel_name(self._h).decode()

    def run_windowed(self, d_gene_ptr: int, d_attr_id: int, d_p_out: int, label=1, stream: int = 0):
        _check(self._lib.gecco_crf_plan_run_windowed(self._h, d_gene_ptr, d_attr_id, int(label), d_p_out, stream or None))

    @property
    def all_kernel_name(self) -> str:
        """The kernel `run_windowed_all` dispatches to."""
        return self._lib.gecco_crf_plan_all_kernel_name(self._h).decode()

    def run_windowed_all(self, d_gene_ptr: int, d_attr_id: int, d_p_all: int, d_p_any: int = 0, background=None, stream: int = 0):
        """Every label's windowed probability into ``d_p_all [n, L]``; with ``background`` also ``d_p_any [n]``."""
        _check(self._lib.gecco_crf_plan_run_windowed_all(self._h, d_gene_ptr, d_attr_id, -1 if background is None else int(background),
                                                         d_p_all, d_p_any or None, stream or None))

    def time_windowed_all(self, d_gene_ptr: int, d_attr_id: int, d_p_all: int, d_p_any: int = 0, background=None, stream: int = 0,
                          warmup=2, iters=10) -> float:
        ms = ctypes.c_float(0)
        _check(self._lib.gecco_crf_plan_time_windowed_all(self._h, d_gene_ptr, d_attr_id, -1 if background is None else int(background),
                                                          d_p_all, d_p_any or None, stream or None, int(warmup), int(iters),
                                                          ctypes.byref(ms)))
        return ms.value

    def run_decode(self, d_gene_ptr: int, d_attr_id: int, d_p_out: int, d_y: int, label: int = 1, d_score: int = 0, stream: int = 0):
        """Windowed marginals + Viterbi labels in one pass over the CSR (shared state scores)."""
        _check(self._lib.gecco_crf_plan_run_decode(self._h, d_gene_ptr, d_attr_id or None, int(label), d_p_out, d_y,
                                                   d_score or None, stream or None))

    def run_decode_pipelined(self, d_gene_ptr: int, d_attr_id: int, d_p_out: int, prev: "Plan" = None, d_prev_y: int = 0, label: int = 1,
                             stream: int = 0):
        """Marginals of this plan's batch + Viterbi labels of the batch the previous call scored on `prev` (one launch
        when both qualify); `Plan.flush_decode_pipelined` delivers the labels of the last batch."""
        _check(self._lib.gecco_crf_plan_run_decode_pipelined(self._h, d_gene_ptr, d_attr_id or None, int(label), d_p_out,
                                                             prev._h if prev is not None else None, d_prev_y or None, stream or None))

    def bind_decode_pipelined(self, d_gene_ptr: int, d_attr_id: int, d_p_out: int, prev: "Plan" = None, d_prev_y: int = 0, label: int = 1,
                              stream: int = 0):
        """The same call with its arguments converted ONCE: returns a zero-argument callable for loops that repeat it on resident
        buffers (a launch-bound step is bound by what the host spends per call; the conversions of eight Python values are
        ~0.7 us of it)."""
        fn = self._lib.gecco_crf_plan_run_decode_pipelined
        args = (self._h, _vp(d_gene_ptr), _vp(d_attr_id or None), ctypes.c_int32(int(label)), _vp(d_p_out),
                prev._h if prev is not None else None, _vp(d_prev_y or None), _vp(stream or None))

        def call():
            rc = fn(*args)
            if rc:
                _check(rc)

        return call

    def flush_decode_pipelined(self, d_y: int, stream: int = 0):
        """Labels of the batch the last `run_decode_pipelined` call on this plan scored."""
        _check(self._lib.gecco_crf_plan_run_decode_pipelined(None, None, None, 1, None, self._h, d_y, stream or None))

    def run_marginals_full(self, d_gene_ptr: int, d_attr_id: int, d_marg: int, d_lognorm: int = 0, stream: int = 0):
        _check(self._lib.gecco_crf_plan_run_marginals_full(self._h, d_gene_ptr, d_attr_id, d_marg, d_lognorm or None, stream or None))

    def run_viterbi(self, d_gene_ptr: int, d_attr_id: int, d_y: int, d_score: int = 0, stream: int = 0):
        _check(self._lib.gecco_crf_plan_run_viterbi(self._h, d_gene_ptr, d_attr_id, d_y, d_score or None, stream or None))

    def run_segment(self, d_p: int, d_annotated: int, d_seg: int, max_seg: int, d_n_seg: int, threshold=0.8, n_cds=3,
                    edge_distance=0, trim=True, carry_state=False, stream: int = 0, criterion="gecco", n_biopfams=5,
                    average_threshold=0.6, d_marker_ptr: int = 0, d_marker_id: int = 0):
        """Cluster rows of device-resident probabilities, on the same stream as the marginals (no copies);
        `d_marker_ptr` / `d_marker_id`: device addresses of the genes' marker domains (antismash criterion)."""
        q = refine_params(criterion, threshold, n_cds, n_biopfams, average_threshold, edge_distance, trim, carry_state,
                          int(d_marker_ptr), int(d_marker_id))
        _check(self._lib.gecco_crf_plan_run_segment_ex(self._h, d_p, d_annotated, ctypes.byref(q), d_seg, int(max_seg), d_n_seg,
                                                       stream or None))

    def time_decode_pipelined(self, d_gene_ptr: int, d_attr_id: int, d_p_out: int, d_y: int, label=1, stream: int = 0, warmup=2,
                              iters=10) -> float:
        """ms per pipelined decode launch (this plan following itself), HIP events on `stream`."""
        ms = ctypes.c_float(0)
        _check(self._lib.gecco_crf_plan_time_decode_pipelined(self._h, d_gene_ptr, d_attr_id, int(label), d_p_out, d_y, stream or None,
                                                              int(warmup), int(iters), ctypes.byref(ms)))
        return ms.value

    def viterbi_stats(self, reset=True) -> dict:
        """What the 2-label Viterbi decoder met since the last reset: decisions inside the coarse margin (`candidates`),
        inside the margin where the difference form is not provably CRFsuite's (`inside_margin`), and the contigs / genes
        decoded again with CRFsuite's own recursion because of them.  Waits for the device."""
        out = (ctypes.c_int64 * 4)()
        _check(self._lib.gecco_crf_plan_viterbi_stats(self._h, out, int(bool(reset))))
        return {"candidates": int(out[0]), "inside_margin": int(out[1]), "contigs_redecoded": int(out[2]), "genes_redecoded": int(out[3])}

    def time_windowed(self, d_gene_ptr: int, d_attr_id: int, d_p_out: int, label=1, stream: int = 0, warmup=2, iters=10) -> float:
        ms = ctypes.c_float(0)
        _check(
            self._lib.gecco_crf_plan_time_windowed(
                self._h, d_gene_ptr, d_attr_id, int(label), d_p_out, stream or None, int(warmup), int(iters), ctypes.byref(ms)
            )
        )
        return ms.value


def _trainer_sets(sets):
    """The C arguments of training sets ``(seq_ptr, item_ptr, attr_id, labels, num_attrs, state_fid, trans_fid,
    num_features[, window, step])``: per array name the int32 arrays of every set (an empty one replaced by one zero, so
    that its pointer is valid), and per count name (``n_seqs``, ``num_attrs``, ``num_labels``, ``num_features``,
    ``window``, ``step``) the list of every set's value."""
    arrays = {name: [] for name in ("seq_ptr", "item_ptr", "attr_id", "labels", "state_fid", "trans_fid")}
    counts = {name: [] for name in ("n_seqs", "num_attrs", "num_labels", "num_features", "window", "step")}
    for seq_ptr, item_ptr, attr_id, labels, A, state_fid, trans_fid, K, *window_step in sets:
        state_fid, trans_fid = _i32(state_fid).ravel(), _i32(trans_fid).ravel()
        if int(A) < 1 or state_fid.size % int(A) != 0:
            raise ValueError("state_fid must have num_attrs * L entries")
        L = state_fid.size // int(A)  # (the library says which label counts a family trains)
        if trans_fid.size != L * L:
            raise ValueError(f"trans_fid must have L * L = {L * L} entries, got {trans_fid.size}")
        seq_ptr = _i32(seq_ptr)
        for name, a in zip(arrays, (seq_ptr, _i32(item_ptr), _i32(attr_id), _i32(labels), state_fid, trans_fid)):
            arrays[name].append(a if a.size else np.zeros(1, dtype=np.int32))
        for name, v in zip(counts, (len(seq_ptr) - 1, A, L, K, *window_step)):
            counts[name].append(int(v))
    return arrays, counts


def _ptr_table(arrays):
    return (_vp * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def _i32_vector(values):
    return _ptr(np.ascontiguousarray(values if len(values) else [0], dtype=np.int32), _c_i32p)  # (keeps its array alive)


def _out_address(a: np.ndarray) -> int:
    """Address of a non-empty float64 array the library writes to (a read-only one is a ``TypeError``).  This and the
    plain ctypes mask keep the marshalling of a one-problem ``eval`` at a few microseconds: ``data_as`` costs 2 µs each."""
    return ctypes.addressof(ctypes.c_double.from_buffer(a))


class _TrainerHandle:
    """What the three trainer families share: the handle, and the evaluation of a list of problems.  A subclass names its
    C family (``_family``) and marshals that family's ``create`` and ``eval`` arguments."""

    _family = ""

    def _c(self, name):
        return getattr(self._lib, f"{self._family}_{name}")

    def _create(self, *args, entry: str = "create"):
        self._lib = load_library()
        self._h = None
        h = _vp()
        _check(self._c(entry)(*args, ctypes.byref(h)))
        self._h = h

    @staticmethod
    def _value_table(values, attr_sizes):
        """``values=`` of the general and whole-sequence families: None, or per problem None (a problem without values)
        or one float64 per attribute entry.  Returns None when no problem has values (the unvalued ``create`` is called),
        else the table of pointers (NULL for a problem without) and the arrays it points to."""
        if values is None or all(v is None for v in values):
            return None, None
        if len(values) != len(attr_sizes):
            raise ValueError(f"values holds {len(values)} entries for {len(attr_sizes)} problems")
        keep = []
        for v, attr in zip(values, attr_sizes):
            if v is None:
                keep.append(None)
                continue
            v = np.ascontiguousarray(v, dtype=np.float64).ravel()
            if v.size != attr:
                raise ValueError(f"values of a problem hold {v.size} entries, its attr_id {attr}")
            keep.append(v if v.size else np.zeros(1, dtype=np.float64))
        return (_vp * len(keep))(*[None if v is None else v.ctypes.data for v in keep]), keep

    @staticmethod
    def _allowed_table(allowed, item_counts):
        """``allowed=`` of the general and whole-sequence families: None, or per problem None (a labelled problem) or one
        uint32 mask per item, bit y set when label y is allowed.  Returns None when no problem has masks (the labelled
        creates are called), else the table of pointers (NULL for a labelled problem) and the arrays it points to."""
        if allowed is None or all(a is None for a in allowed):
            return None, None
        if len(allowed) != len(item_counts):
            raise ValueError(f"allowed holds {len(allowed)} entries for {len(item_counts)} problems")
        keep = []
        for a, n in zip(allowed, item_counts):
            if a is None:
                keep.append(None)
                continue
            a = np.asarray(a)
            if a.dtype.kind not in "ui" or (a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF)):
                raise ValueError("allowed masks are unsigned 32-bit integers")
            a = np.ascontiguousarray(a, dtype=np.uint32).ravel()
            if a.size != n:
                raise ValueError(f"allowed masks of a problem hold {a.size} entries, the problem {n} items")
            keep.append(a if a.size else np.zeros(1, dtype=np.uint32))
        return (_vp * len(keep))(*[None if a is None else a.ctypes.data for a in keep]), keep

    @staticmethod
    def _double_table(name, arrays, sizes):
        """``weights=`` / ``costs=`` of the general and whole-sequence families: None, or per problem None or a float64
        array of the size given (one weight per sequence; the cost matrix [L, L], row = gold).  Returns None when no
        problem has any, else the table of pointers (NULL for a problem without) and the arrays it points to.  The
        values themselves are checked by the library, which names the problem and the index."""
        if arrays is None or all(a is None for a in arrays):
            return None, None
        if len(arrays) != len(sizes):
            raise ValueError(f"{name} holds {len(arrays)} entries for {len(sizes)} problems")
        keep = []
        for a, n in zip(arrays, sizes):
            if a is None:
                keep.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float64).ravel()
            if a.size != n:
                raise ValueError(f"{name} of a problem hold {a.size} entries, the problem needs {n}")
            keep.append(a if a.size else np.zeros(1, dtype=np.float64))
        return (_vp * len(keep))(*[None if a is None else a.ctypes.data for a in keep]), keep

    def _create_general(self, problems, device, values, whole: bool, allowed=None, weights=None, costs=None):
        """The constructor of the general (``whole=False``: every problem with a window and a step) and the whole-sequence
        family, on ``create`` or, when a problem has values, on ``create_valued``, or, when a problem has allowed-label
        masks, on ``create_partial`` (a problem with masks may give None as its labels), or, when a problem has sequence
        weights or label costs, on ``create_weighted``."""
        wt, _keep_weights = self._double_table("weights", weights, [int(np.asarray(p[0]).size) - 1 for p in problems])
        ct, _keep_costs = self._double_table("costs", costs, [int(np.asarray(p[6]).size) for p in problems])  # (trans_fid's L * L)
        at, _keep_allowed = self._allowed_table(allowed, [int(np.asarray(p[0])[-1]) for p in problems])
        if at is not None:  # (the labels of a problem with masks are not read: any array of the right kind will do)
            problems = [p if a is None or p[3] is not None else (*p[:3], np.zeros(1, dtype=np.int32), *p[4:])
                        for p, a in zip(problems, allowed)]
        if whole and any(len(p) != 8 for p in problems):
            raise ValueError("a whole-sequence problem has 8 entries: no window and no step")
        arrays, counts = _trainer_sets(problems)
        if not whole and any(len(v) != len(problems) for v in counts.values()):
            raise ValueError("every problem needs a window and a step")
        t = {name: _ptr_table(arrs) for name, arrs in arrays.items()}
        c = {name: _i32_vector(v) for name, v in counts.items()}
        vt, _keep = self._value_table(values, [int(np.asarray(p[2]).size) for p in problems])
        value_table = () if vt is None else (vt,)
        entry = "create" if vt is None else "create_valued"
        allowed_table = ()
        if at is not None:  # (the partial create takes the values' table always: NULL when no problem has values)
            value_table, allowed_table, entry = (vt,), (at,), "create_partial"
        if wt is not None or ct is not None:  # (the weighted create takes every table: NULL where no problem has one)
            value_table, allowed_table, entry = (vt,), (at, wt, ct), "create_weighted"
        window_step = () if whole else (c["window"], c["step"])
        self._create(int(device), len(problems), t["seq_ptr"], c["n_seqs"], t["item_ptr"], t["attr_id"], *value_table,
                     t["labels"], *allowed_table, c["num_attrs"], c["num_labels"], *window_step, t["state_fid"],
                     t["trans_fid"], c["num_features"], entry=entry)
        self.num_features = self._features = counts["num_features"]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._c("free")(h)

    def __len__(self) -> int:
        return int(self._c("num_problems")(self._h))

    def num_windows(self, k: int) -> int:
        return int(self._c("num_windows")(self._h, int(k)))

    def _eval_problems(self, ws, active=None, f=None, g=None):
        """f and g of every active problem (all of them when ``active`` is None) under the weights ``ws[k]`` (None for
        an inactive problem).  Returns ``(f, g)``: an ``(n,)`` float64 array and a list of gradient arrays.  Given ``f``
        and ``g`` are written in place, and the entries of inactive problems are left as they were."""
        features = self._features  # (of every problem)
        n = len(features)
        active = [True] * n if active is None else [bool(a) for a in active]
        if len(active) != n:
            raise ValueError(f"expected an active mask of {n} entries, got {len(active)}")
        if f is None:
            f = np.full(n, np.nan)
        if g is None:
            g = [np.empty(K) for K in features]
        if not (isinstance(f, np.ndarray) and f.dtype == np.float64 and f.shape == (n,) and f.flags.c_contiguous):
            raise ValueError("f must be a contiguous float64 array of one entry per problem")
        keep = []
        w_ptr, g_ptr = (_vp * n)(), (_vp * n)()
        for k in range(n):
            if not active[k]:
                continue
            K = features[k]
            w = np.ascontiguousarray(ws[k], dtype=np.float64)
            if w.shape != (K,):
                raise ValueError(f"problem {k}: expected {K} weights, got shape {w.shape}")
            gg = g[k]
            if not (isinstance(gg, np.ndarray) and gg.dtype == np.float64 and gg.shape == (K,) and gg.flags.c_contiguous):
                raise ValueError(f"problem {k}: the gradient must be a contiguous float64 array of {K} entries")
            w = w if w.size else np.zeros(1)
            gb = gg if gg.size else np.zeros(1)
            keep += [w, gb]
            w_ptr[k], g_ptr[k] = w.ctypes.data, _out_address(gb)
        _check(self._eval_native((ctypes.c_uint8 * n)(*active), w_ptr, _out_address(f), g_ptr))
        return f, g

    def _eval_native(self, act, w_ptr, f, g_ptr):
        return self._c("eval")(self._h, act, w_ptr, f, g_ptr)


class Trainer(_TrainerHandle):
    """Training set of a 2-label CRF resident on one device (``gecco_crf_trainer_*``): ``eval(w)`` returns the summed
    negative log-likelihood of every training window and its gradient over the ``num_features`` generated features."""

    _family = "gecco_crf_trainer"

    def __init__(self, seq_ptr, item_ptr, attr_id, labels, num_attrs: int, window: int, step: int, state_fid, trans_fid,
                 num_features: int, device: int = 0):
        arrays, counts = _trainer_sets([(seq_ptr, item_ptr, attr_id, labels, num_attrs, state_fid, trans_fid, num_features)])
        a = {name: _ptr(arrs[0], _c_i32p) for name, arrs in arrays.items()}
        self._create(int(device), a["seq_ptr"], counts["n_seqs"][0], a["item_ptr"], a["attr_id"], a["labels"],
                     counts["num_attrs"][0], counts["num_labels"][0], int(window), int(step), a["state_fid"], a["trans_fid"],
                     counts["num_features"][0])
        self._features = counts["num_features"]
        self.num_features = self._features[0]

    def __len__(self) -> int:  # (the lone family has no num_problems)
        return 1

    @property
    def num_windows(self) -> int:
        return int(self._c("num_windows")(self._h))

    def eval(self, w):
        f, g = self._eval_problems([w])
        return float(f[0]), g[0]

    def _eval_native(self, act, w_ptr, f, g_ptr):
        return self._c("eval")(self._h, w_ptr[0], f, g_ptr[0])


class TrainerBatch(_TrainerHandle):
    """Several training sets of 2-label CRFs resident on one device at once (``gecco_crf_trainer_batch_*``).

    ``problems`` holds one tuple ``(seq_ptr, item_ptr, attr_id, labels, num_attrs, state_fid, trans_fid, num_features)``
    per problem, as ``Trainer`` takes them; ``window`` and ``step`` are shared.  ``eval(ws, active)`` evaluates the active
    problems in one batched pass; problem k's f and g are bitwise what a lone ``Trainer`` of it returns for ``ws[k]``."""

    _family = "gecco_crf_trainer_batch"
    eval = _TrainerHandle._eval_problems

    def __init__(self, problems, window: int, step: int, device: int = 0):
        arrays, counts = _trainer_sets(problems)
        t = {name: _ptr_table(arrs) for name, arrs in arrays.items()}
        c = {name: _i32_vector(v) for name, v in counts.items()}
        self._create(int(device), len(problems), t["seq_ptr"], c["n_seqs"], t["item_ptr"], t["attr_id"], t["labels"],
                     c["num_attrs"], c["num_labels"], int(window), int(step), t["state_fid"], t["trans_fid"],
                     c["num_features"])
        self.num_features = self._features = counts["num_features"]


class TrainerGrid(TrainerBatch):
    """A grid of problems over shared training sets on one device (``gecco_crf_trainer_grid_*``).

    ``sets`` holds one tuple ``(seq_ptr, item_ptr, attr_id, labels, num_attrs, state_fid, trans_fid, num_features,
    window, step)`` per training set, each uploaded once; problem k is set ``problem_set[k]`` with weights of its own.
    ``scratch_budget_bytes`` caps the work space of one group of problems (0: no cap).  ``eval`` is ``TrainerBatch``'s;
    problem k's f and g are bitwise what a lone ``Trainer`` of its set returns for ``ws[k]``."""

    _family = "gecco_crf_trainer_grid"

    def __init__(self, sets, problem_set, scratch_budget_bytes: int = 0, device: int = 0):
        arrays, counts = _trainer_sets(sets)
        t = {name: _ptr_table(arrs) for name, arrs in arrays.items()}
        c = {name: _i32_vector(v) for name, v in counts.items()}
        pset = _i32(problem_set).ravel()
        self._create(int(device), len(sets), t["seq_ptr"], c["n_seqs"], t["item_ptr"], t["attr_id"], t["labels"],
                     c["num_attrs"], c["num_labels"], c["window"], c["step"], t["state_fid"], t["trans_fid"],
                     c["num_features"], int(pset.size), _i32_vector(pset), int(scratch_budget_bytes))
        self.num_features = self._features = [counts["num_features"][s] for s in pset.tolist()]

    def scratch_bytes(self, k: int = -1) -> int:
        """Scratch bytes of problem k; for k = -1 the work space allocated (the most one group of problems uses)."""
        return int(self._c("scratch_bytes")(self._h, int(k)))


class TrainerGeneral(_TrainerHandle):
    """Training sets of CRFs with 2 to 32 labels resident on one device (``gecco_crf_trainer_general_*``).

    ``problems`` holds one tuple ``(seq_ptr, item_ptr, attr_id, labels, num_attrs, state_fid, trans_fid, num_features,
    window, step)`` per problem, as ``TrainerGrid`` takes its sets; the label count of a problem is that of its
    ``state_fid`` [A, L].  ``eval(ws, active)`` evaluates the active problems; problem k's f and g are bitwise what a
    ``TrainerGeneral`` of problem k alone returns for ``ws[k]``.  ``values=``: per problem None or one float64 per
    attribute entry, parallel to its ``attr_id`` (``gecco_crf_trainer_general_create_valued``).  ``allowed=``: per problem
    None (a labelled problem) or one uint32 mask per item, bit y set when label y is allowed: the problem then minimises
    log Z - log Z_A (``gecco_crf_trainer_general_create_partial``), and its ``labels`` entry is not read and may be None.
    ``weights=``: per problem None or one float64 >= 0 per sequence, the weight of every window cut from it; ``costs=``:
    per problem None or the label-cost matrix [L, L], row = gold, >= 0 with a zero diagonal
    (``gecco_crf_trainer_general_create_weighted``): the problem then minimises the weighted cost-augmented objective.  A
    problem with neither is the problem the other creates build, with their kernels and their bits."""

    _family = "gecco_crf_trainer_general"
    eval = _TrainerHandle._eval_problems

    def __init__(self, problems, device: int = 0, values=None, allowed=None, weights=None, costs=None):
        self._create_general(problems, device, values, whole=False, allowed=allowed, weights=weights, costs=costs)

    def scratch_bytes(self, k: int = -1) -> int:
        """Scratch bytes of problem k; for k = -1 the sum over the problems, which is what is allocated."""
        return int(self._c("scratch_bytes")(self._h, int(k)))


class TrainerSequences(_TrainerHandle):
    """Training sets of CRFs with 2 to 32 labels whose instances are the whole sequences, of any length from one item up
    (``gecco_crf_trainer_sequences_*``): CRFsuite's own training mode.

    ``problems`` holds one tuple ``(seq_ptr, item_ptr, attr_id, labels, num_attrs, state_fid, trans_fid, num_features)``
    per problem; the label count of a problem is that of its ``state_fid`` [A, L].  ``eval(ws, active)`` evaluates the
    active problems; problem k's f and g are bitwise what a ``TrainerSequences`` of problem k alone returns for
    ``ws[k]``.  ``values=``: as ``TrainerGeneral``'s (``gecco_crf_trainer_sequences_create_valued``); ``allowed=``: as
    ``TrainerGeneral``'s (``gecco_crf_trainer_sequences_create_partial``); ``weights=`` and ``costs=``: as
    ``TrainerGeneral``'s (``gecco_crf_trainer_sequences_create_weighted``)."""

    _family = "gecco_crf_trainer_sequences"
    eval = _TrainerHandle._eval_problems

    def __init__(self, problems, device: int = 0, values=None, allowed=None, weights=None, costs=None):
        self._create_general(problems, device, values, whole=True, allowed=allowed, weights=weights, costs=costs)

    def num_sequences(self, k: int) -> int:
        return int(self._c("num_sequences")(self._h, int(k)))

    num_windows = num_sequences  # (the instances of problem k)

    def scratch_bytes(self, k: int = -1) -> int:
        """Scratch bytes of problem k; for k = -1 the sum over the problems, which is what is allocated."""
        return int(self._c("scratch_bytes")(self._h, int(k)))


def fisher_exact(tables, device: int = 0) -> np.ndarray:
    """Two-sided Fisher exact p-values of the 2x2 tables ``tables[i] = [[a, b], [c, d]]`` (any shape that reshapes to
    ``(n, 4)``), computed on ``device`` (``gecco_crf_fisher_exact``): scipy's semantics, in fp64."""
    lib = load_library()
    t = np.ascontiguousarray(np.asarray(tables, dtype=np.int64).reshape(-1, 4))
    out = np.empty(len(t), dtype=np.float64)
    _check(lib.gecco_crf_fisher_exact(int(device), t.ctypes.data if len(t) else None, len(t),
                                      out.ctypes.data if len(t) else None))
    return out


class Forest:
    """A random forest fitted on the device (``gecco_crf_forest_*``): sklearn 1.7's RandomForestClassifier for the
    configuration GECCO's TypeClassifier uses, tree for tree.  The host draws the random streams (see ``gecco_amd.types``).
    Near-equal feature values follow the sklearn 1.7.2 build, not its source: a split position is valid when
    ``Xf[p] > Xf[p - 1]`` on the float32 values (no 1e-7 margin), so values one ulp apart can be split."""

    @staticmethod
    def _arrays(col_ptr, row_idx, values, n_samples, y, n_classes, sample_counts, rand_state):
        cp = np.ascontiguousarray(col_ptr, dtype=np.int32)
        ri = np.ascontiguousarray(row_idx, dtype=np.int32)
        va = np.ascontiguousarray(values, dtype=np.float32)
        yy = np.ascontiguousarray(y, dtype=np.uint8)
        nc = np.ascontiguousarray(n_classes, dtype=np.uint8)
        sc = np.ascontiguousarray(sample_counts, dtype=np.int32)
        rs = np.ascontiguousarray(rand_state, dtype=np.uint32)
        if yy.shape != (int(n_samples), len(nc)) or sc.shape != (len(rs), int(n_samples)):
            raise ValueError("forest fit: y must be (n_samples, n_outputs) and sample_counts (n_trees, n_samples)")
        return cp, ri, va, yy, nc, sc, rs

    def __init__(self, col_ptr, row_idx, values, n_samples: int, y, n_classes, sample_counts, rand_state, max_features: int,
                 device: int = 0):
        lib = self._lib = load_library()
        cp, ri, va, yy, nc, sc, rs = self._arrays(col_ptr, row_idx, values, n_samples, y, n_classes, sample_counts, rand_state)
        h = _vp()
        self._h = None
        _check(lib.gecco_crf_forest_fit(int(device), int(n_samples), len(cp) - 1, _addr(cp), _addr(ri), _addr(va), len(nc),
                                        _addr(nc), _addr(yy), len(rs), _addr(sc), _addr(rs), int(max_features), ctypes.byref(h)))
        self._adopt(h, len(cp) - 1)

    def _adopt(self, h, n_features: int) -> None:
        """Take over the fitted handle `h` and read its sizes."""
        lib = self._lib
        self._h = h
        n_trees, n_out, mc = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(lib.gecco_crf_forest_info(h, ctypes.byref(n_trees), ctypes.byref(n_out), ctypes.byref(mc), None, None))
        nodes = np.zeros(n_trees.value, dtype=np.int32)
        depth = np.zeros(n_trees.value, dtype=np.int32)
        _check(lib.gecco_crf_forest_info(h, None, None, None, nodes.ctypes.data, depth.ctypes.data))
        self.n_trees, self.n_outputs, self.max_n_classes = n_trees.value, n_out.value, mc.value
        self.n_features = n_features
        self.node_count, self.max_depth = nodes, depth

    def export(self, tree: int) -> dict:
        """Tree `tree` as sklearn's ``Tree`` arrays (intp arrays as int64, ``value`` as (nodes, n_outputs, max_n_classes))."""
        n = int(self.node_count[tree])
        i32 = {k: np.zeros(n, dtype=np.int32) for k in ("children_left", "children_right", "feature", "n_node_samples")}
        f64 = {k: np.zeros(n, dtype=np.float64) for k in ("threshold", "impurity", "weighted_n_node_samples")}
        value = np.zeros((n, self.n_outputs, self.max_n_classes), dtype=np.float64)
        _check(self._lib.gecco_crf_forest_export(
            self._h, int(tree), i32["children_left"].ctypes.data, i32["children_right"].ctypes.data, i32["feature"].ctypes.data,
            f64["threshold"].ctypes.data, f64["impurity"].ctypes.data, i32["n_node_samples"].ctypes.data,
            f64["weighted_n_node_samples"].ctypes.data, value.ctypes.data))
        out = {k: v.astype(np.int64) for k, v in i32.items()}
        out.update(f64)
        out["value"] = value
        return out

    def predict(self, x) -> np.ndarray:
        """``posit[r, k] = 1 - predict_proba(x)[k][r, 0]`` of the dense rows ``x`` (n_rows, n_features)."""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        if xx.ndim != 2 or xx.shape[1] != self.n_features:
            raise ValueError(f"forest predict: expected rows of {self.n_features} features, got shape {xx.shape}")
        out = np.zeros((xx.shape[0], self.n_outputs), dtype=np.float64)
        if len(xx):
            _check(self._lib.gecco_crf_forest_predict(self._h, len(xx), xx.ctypes.data, out.ctypes.data))
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.gecco_crf_forest_free(h)
            self._h = None


def fit_forests(problems: Sequence[dict], max_features: int, device: int = 0) -> list:
    """Fit one forest per problem in one launch (``gecco_crf_forest_fit_batch``): each problem is a dict of `Forest`'s
    per-problem arguments (``col_ptr, row_idx, values, n_samples, y, n_classes, sample_counts, rand_state``); the number of
    features, outputs and trees is shared.  Every returned `Forest` is bit for bit the one its problem gives alone."""
    lib = load_library()
    keys = ("col_ptr", "row_idx", "values", "n_samples", "y", "n_classes", "sample_counts", "rand_state")
    arrs = [Forest._arrays(*(p[k] for k in keys)) for p in problems]
    K = len(arrs)
    if K == 0:
        return []
    shared = {(len(a[0]) - 1, len(a[4]), len(a[6])) for a in arrs}
    if len(shared) != 1:
        raise ValueError(f"forest fit: the problems of a batch share n_features, n_outputs and n_trees, got {sorted(shared)}")
    n_features, n_outputs, n_trees = shared.pop()
    n_samples = np.array([int(p["n_samples"]) for p in problems], dtype=np.int32)
    ptrs = [(_vp * K)(*(_addr(a[i]) for a in arrs)) for i in range(7)]  # col_ptr, row_idx, values, y, n_classes, counts, states
    out = (_vp * K)()
    _check(lib.gecco_crf_forest_fit_batch(int(device), K, n_features, n_outputs, n_trees, int(max_features), _addr(n_samples),
                                          ptrs[0], ptrs[1], ptrs[2], ptrs[4], ptrs[3], ptrs[5], ptrs[6], out))
    forests = []
    for k in range(K):  # (every handle has its owner before anything else can fail)
        f = Forest.__new__(Forest)
        f._lib, f._h = lib, _vp(out[k])
        forests.append(f)
    for f in forests:
        f._adopt(f._h, n_features)
    return forests


def predict_forests(forests: Sequence[Forest], xs: Sequence) -> list:
    """``forests[k].predict(xs[k])`` for every k with one launch and one download
    (``gecco_crf_forest_predict_batch``); blocks without rows are allowed."""
    if len(forests) != len(xs):
        raise ValueError(f"forest predict: {len(forests)} forests but {len(xs)} blocks of rows")
    K = len(forests)
    if K == 0:
        return []
    xx = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    for f, x in zip(forests, xx):
        if x.ndim != 2 or x.shape[1] != f.n_features:
            raise ValueError(f"forest predict: expected rows of {f.n_features} features, got shape {x.shape}")
    outs = [np.zeros((len(x), f.n_outputs), dtype=np.float64) for f, x in zip(forests, xx)]
    n_rows = np.array([len(x) for x in xx], dtype=np.int32)
    hs = (_vp * K)(*(f._h for f in forests))
    xp = (_vp * K)(*(x.ctypes.data for x in xx))
    op = (_vp * K)(*(o.ctypes.data for o in outs))
    _check(load_library().gecco_crf_forest_predict_batch(hs, K, _addr(n_rows), xp, op))
    return outs
