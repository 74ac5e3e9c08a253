"""ctypes binding of libmm2chain_hip.so (include/mm2chain.h).  No fallback: a missing library raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MM2C_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "libmm2chain_hip.so")   # MM2C_LIB_PATH: an experimental build (tools/probe_prices.sh)

MM2C_F_IGNORE_SEG = 0x1
MM2C_F_FORCE_GENERAL = 0x2


class Params(C.Structure):
    """mm2c_params_t"""
    _fields_ = [("max_dist_x", C.c_int32), ("max_dist_y", C.c_int32), ("bw", C.c_int32),
                ("max_skip", C.c_int32), ("max_iter", C.c_int32), ("gap_scale", C.c_float),
                ("is_cdna", C.c_int32), ("n_segs", C.c_int32), ("q_span_override", C.c_int32),
                ("flags", C.c_int32)]


class Stream(C.Structure):
    """mm2c_stream_t"""
    _fields_ = [("par", Params), ("min_cnt", C.c_int32), ("min_sc", C.c_int32), ("n_tasks", C.c_int64), ("total", C.c_int64),
                ("offsets", C.POINTER(C.c_int64)), ("anchors", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("tasks", C.c_uint64), ("anchors", C.c_uint64), ("launches", C.c_uint64), ("segments", C.c_uint64), ("host_call_ns", C.c_uint64), ("passes", C.c_uint64)]


class SlotStats(C.Structure):
    """mm2c_slot_stats_t"""
    _fields_ = [("device", C.c_int32), ("reserved", C.c_int32), ("passes", C.c_uint64), ("calls", C.c_uint64), ("anchors", C.c_uint64), ("declined", C.c_uint64)]


class StageStats(C.Structure):
    """mm2c_stage_stats_t"""
    _fields_ = [(k, C.c_uint64) for k in ("calls", "chunks", "total_ns", "alloc_ns", "n_alloc", "free_ns", "n_free", "setup_ns", "h2d_ns", "seed_ns", "dp_ns",
                                          "epi_ns", "d2h_ns", "wait_ns")]


# every symbol include/mm2chain.h declares with C linkage: name -> (restype, argtypes)
class ReadResult(C.Structure):
    """mm2c_read_result_t (library-owned arrays)"""
    _fields_ = [("n_reads", C.c_int64),
                ("n_sketch", C.c_int64), ("sketch_off", C.c_void_p), ("sketch", C.c_void_p),
                ("n_matches", C.c_int64), ("match_off", C.c_void_p), ("matches", C.c_void_p),
                ("n_anchors", C.c_int64), ("anchor_off", C.c_void_p), ("rep_len", C.c_void_p),
                ("n_mini_pos", C.c_int64), ("mini_off", C.c_void_p), ("mini_pos", C.c_void_p),
                ("n_u", C.c_int64), ("n_b", C.c_int64), ("u_off", C.c_void_p), ("u", C.c_void_p), ("b_off", C.c_void_p), ("b", C.c_void_p),
                ("priv", C.c_void_p), ("n_rechained", C.c_int64), ("rechained", C.c_void_p)]


class SketchStats(C.Structure):
    """mm2c_sketch_stats_t"""
    _fields_ = [(k, C.c_uint64) for k in ("calls", "chunks", "bases", "minimizers", "matches", "h2d_ns", "sketch_ns", "lookup_ns")]


class FragGaps(C.Structure):
    """mm2c_frag_gaps_t: the four scalars the per-fragment chaining distances are made from (map.c:305-314)"""
    _fields_ = [(k, C.c_int32) for k in ("is_sr", "max_gap", "max_gap_ref", "max_frag_len")]


class FragStats(C.Structure):
    """mm2c_frag_stats_t"""
    _fields_ = [(k, C.c_uint64) for k in ("calls", "fragments", "rechained", "rechain_ns")]


class IndexStats(C.Structure):
    """mm2c_index_stats_t"""
    _fields_ = [(k, C.c_uint64) for k in ("calls", "chunks", "bases", "minimizers", "keys", "h2d_ns", "sketch_ns", "sort_ns", "group_ns", "occ_ns", "replicate_ns")]


class Reg(C.Structure):
    """mm2c_reg_t = mm_reg1_t (minimap.h:85-100), 80 bytes; flags: mapq bits 0-7, split bits 8-9, rev bit 10"""
    _fields_ = [(k, C.c_int32) for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as_", "mlen", "blen", "n_sub", "score0")] + \
               [("flags", C.c_uint32), ("hash", C.c_uint32), ("div", C.c_float), ("p", C.c_uint64)]


class HitOpt(C.Structure):
    """mm2c_hit_opt_t: mm_set_parent's mask_level, mask_len, MM_F_HARD_MLEVEL and mm_select_sub's pri_ratio, min_diff (2k), best_n"""
    _fields_ = [("mask_level", C.c_float), ("mask_len", C.c_int32), ("hard_mask_level", C.c_int32), ("pri_ratio", C.c_float), ("min_diff", C.c_int32),
                ("best_n", C.c_int32)]


class HitMultiOpt(C.Structure):
    """mm2c_hit_multi_opt_t: what mm_select_sub_multi takes beyond mm2c_hit_opt_t (pe.c:6; map.c:254 passes 0.2f, 0.7f)"""
    _fields_ = [("pri1", C.c_float), ("pri2", C.c_float), ("n_segs", C.c_int32), ("max_gap_ref", C.c_int32)]


class MapqOpt(C.Structure):
    """mm2c_mapq_opt_t: mm_join_long's switch and thresholds (options.c:38-41), mm_filter_regs' min_cnt, mm_set_mapq's min_chain_sc"""
    _fields_ = [("do_join", C.c_int32), ("max_join_long", C.c_int32), ("max_join_short", C.c_int32), ("min_join_flank_sc", C.c_int32),
                ("min_join_flank_ratio", C.c_float), ("min_cnt", C.c_int32), ("min_chain_score", C.c_int32)]


class FinOpt(C.Structure):
    """mm2c_fin_opt_t: mm_filter_regs' min_cnt, min_chain_score, min_dp_max, max_clip_ratio; mm_set_parent's mask_level, mask_len, MM_F_HARD_MLEVEL, sub_diff (a * 2 + b);
    mm_select_sub's pri_ratio, min_diff (2k), best_n; mm_set_mapq's match_sc (opt->a) and is_sr; MM_F_ALL_CHAINS"""
    _fields_ = [("min_cnt", C.c_int32), ("min_chain_score", C.c_int32), ("min_dp_max", C.c_int32), ("max_clip_ratio", C.c_float), ("mask_level", C.c_float),
                ("mask_len", C.c_int32), ("hard_mask_level", C.c_int32), ("sub_diff", C.c_int32), ("pri_ratio", C.c_float), ("min_diff", C.c_int32), ("best_n", C.c_int32),
                ("match_sc", C.c_int32), ("is_sr", C.c_int32), ("all_chains", C.c_int32)]


class PairOpt(C.Structure):
    """mm2c_pair_opt_t: mm_pair's max_gap_ref (one scalar, for a run without per-fragment values), pe_bonus, sub_diff (a * 2 + b), match_sc (a); opt->pe_ori and
    whether the flip of map.c:455-466 runs"""
    _fields_ = [(k, C.c_int32) for k in ("max_gap_ref", "pe_bonus", "sub_diff", "match_sc", "pe_ori", "flip")]


class Err(C.Structure):
    """mm2c_err_t: the counts of mm_est_err per final region (esterr.c:53-61); n_match 0: div = -1, n_match -1: the read has no mini_pos"""
    _fields_ = [("n_match", C.c_int32), ("n_tot", C.c_int32)]


MM2C_REG_SAM_PRI_BIT = 12
MM2C_REG_PROPER_FRAG_BIT = 13
MM2C_REG_PE_THRU_BIT = 14
MM2C_PAIR_LDS_REGIONS = 128
MM2C_HIT_LDS_REGIONS = 128
MM2C_MAPQ_MAX_LOG_ARG = (1 << 24) - 1
MM2C_MAX_SEG = 255
MM2C_REG_SEG_SPLIT_BIT = 15
MM2C_REG_SEG_ID_SHIFT = 16
MM2C_SEED_LONG_JOIN_BIT = 40
MM2C_FIN_LDS_REGIONS = 128

C_SYMBOLS = {
    "mm2c_init": (C.c_int, [C.c_int]),
    "mm2c_init_devices": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "mm2c_init_async": (C.c_int, [C.c_int]),
    "mm2c_init_wait": (C.c_int, []),
    "mm2c_warm_up": (C.c_int, []),
    "mm2c_device_count": (C.c_int, []),
    "mm2c_numa_cpulist": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "mm2c_slot_worker_node": (C.c_int, [C.c_int]),
    "mm2c_split_tasks": (C.c_int, [C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "mm2c_shutdown": (None, []),
    "mm2c_last_error": (C.c_char_p, []),
    "mm2c_device_info": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "mm2c_device_identity": (C.c_int, [C.POINTER(C.c_int), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "mm2c_tune": (C.c_int, [C.c_char_p, C.c_int]),
    "mm2c_tune_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_tune_key": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
    "mm2c_split_model": (C.c_int, [C.c_char_p] + [C.POINTER(C.c_float)] * 5),
    "mm2c_params_map_ont": (None, [C.POINTER(Params)]),
    "mm2c_params_fpga_v2": (None, [C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mm2c_plan_create": (C.c_void_p, [C.POINTER(Params), C.c_int64, C.c_void_p]),
    "mm2c_plan_destroy": (None, [C.c_void_p]),
    "mm2c_plan_total_anchors": (C.c_int64, [C.c_void_p]),
    "mm2c_plan_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_plan_set_device_offsets": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mm2c_plan_set_task_dists": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mm2c_plan_run_device_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "mm2c_plan_predict_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_plan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_plan_last_variant": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "mm2c_plan_last_classes": (C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte), C.c_int64]),
    "mm2c_plan_last_route": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_route_pieces": (C.c_int, [C.c_int64, C.c_int64, C.c_int64]),
    "mm2c_last_host_variant": (C.c_int, [C.c_char_p, C.c_size_t]),
    "mm2c_debug_label_hits": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "mm2c_plan_last_prepass_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_chain_batch_host": (C.c_int, [C.POINTER(Params), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_pinned_alloc": (C.c_void_p, [C.c_size_t]),
    "mm2c_pinned_free": (None, [C.c_void_p]),
    "mm2c_chain_task_host": (C.c_int, [C.POINTER(Params), C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int]),
    "mm2c_chain_task_host_pred": (C.c_int, [C.POINTER(Params), C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "mm2c_get_slot_stats": (C.c_int, [C.c_int, C.POINTER(SlotStats)]),
    "mm2c_route_slot": (C.c_int, [C.c_int, C.c_void_p, C.c_int]),
    "mm_chain_dp": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                 C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p, C.c_int]),
    "mm2c_plan_chains_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_plan_chains_device_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                            C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "mm2c_plan_last_epilogue_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_chain_epilogue_host": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_mm_chain_dp_batch_host": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_regplan_create": (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64]),
    "mm2c_regplan_destroy": (None, [C.c_void_p]),
    "mm2c_regplan_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_regplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mm2c_regplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_regplan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mm2c_gen_regs_batch_host": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_read_hash": (C.c_uint32, [C.c_char_p, C.c_int32, C.c_int32]),
    "mm2c_hitplan_create": (C.c_void_p, [C.c_int64, C.c_int64]),
    "mm2c_hitplan_destroy": (None, [C.c_void_p]),
    "mm2c_hitplan_run_device": (C.c_int, [C.c_void_p, C.POINTER(HitOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_hitplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mm2c_hitplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_select_hits_batch_host": (C.c_int, [C.c_int64, C.POINTER(HitOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_hitplan_run_device_multi": (C.c_int, [C.c_void_p, C.POINTER(HitOpt), C.POINTER(HitMultiOpt)] + [C.c_void_p] * 7),
    "mm2c_select_hits_multi_batch_host": (C.c_int, [C.c_int64, C.POINTER(HitOpt), C.POINTER(HitMultiOpt)] + [C.c_void_p] * 6),
    "mm2c_segplan_create": (C.c_void_p, [C.c_int64, C.c_int32, C.c_int64, C.c_int64]),
    "mm2c_segplan_destroy": (None, [C.c_void_p]),
    "mm2c_segplan_seg_chain_cap": (C.c_int64, [C.c_void_p]),
    "mm2c_segplan_run_device": (C.c_int, [C.c_void_p] * 17),
    "mm2c_segplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_segplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_segplan_last_kernel_ms": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_float)] * 5),
    "mm2c_seg_gen_batch_host": (C.c_int, [C.c_int64, C.c_int32] + [C.c_void_p] * 15),
    "mm2c_kswplan_create": (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mm2c_kswplan_create_slots": (C.c_void_p, [C.c_int64] * 5),
    "mm2c_kswplan_destroy": (None, [C.c_void_p]),
    "mm2c_kswplan_slot_bytes": (C.c_int64, [C.c_void_p]),
    "mm2c_kswplan_n_slots": (C.c_int64, [C.c_void_p]),
    "mm2c_ksw_task_scratch": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mm2c_kswplan_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6),
    "mm2c_kswplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_kswplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_kswplan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_ksw_extd2_batch_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]),
    "mm2c_extraplan_create": (C.c_void_p, [C.c_int64] * 6),
    "mm2c_extraplan_destroy": (None, [C.c_void_p]),
    "mm2c_extraplan_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 8),
    "mm2c_extraplan_zdrop_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 7),
    "mm2c_extraplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_extraplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_extraplan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mm2c_update_extra_batch_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
    "mm2c_test_zdrop_batch_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "mm2c_refseq_create": (C.c_void_p, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "mm2c_refseq_destroy": (None, [C.c_void_p]),
    "mm2c_alnplan_create": (C.c_void_p, [C.c_int64] * 6 + [C.c_int32, C.c_int64, C.c_int64]),
    "mm2c_alnplan_destroy": (None, [C.c_void_p]),
    "mm2c_alnplan_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 13),
    "mm2c_alnplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_alnplan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_cigplan_create": (C.c_void_p, [C.c_int64] * 10),
    "mm2c_cigplan_destroy": (None, [C.c_void_p]),
    "mm2c_cigplan_second_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 9),
    "mm2c_cigplan_second_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_cigplan_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 22),
    "mm2c_cigplan_check": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int64)] * 4),
    "mm2c_cigplan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_second_pass_batch_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_assemble_regions_batch_host": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 4 +
                                                   [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
    "mm2c_align_tasks_batch_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mm2c_mapqplan_create": (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    "mm2c_mapqplan_destroy": (None, [C.c_void_p]),
    "mm2c_mapqplan_run_device": (C.c_int, [C.c_void_p, C.POINTER(MapqOpt)] + [C.c_void_p] * 12),
    "mm2c_mapqplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_mapqplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_mapqplan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mm2c_join_mapq_batch_host": (C.c_int, [C.c_int64, C.POINTER(MapqOpt), C.c_int32] + [C.c_void_p] * 11),
    "mm2c_finplan_create": (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "mm2c_finplan_destroy": (None, [C.c_void_p]),
    "mm2c_finplan_apply_run_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6 +
                                      [C.c_int64] + [C.c_void_p] * 4),
    "mm2c_finplan_apply_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_finplan_run_device": (C.c_int, [C.c_void_p, C.POINTER(FinOpt)] + [C.c_void_p] * 9),
    "mm2c_finplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_finplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mm2c_apply_regions_batch_host": (C.c_int, [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 3),
    "mm2c_finish_regions_batch_host": (C.c_int, [C.c_int64, C.POINTER(FinOpt), C.c_int32] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 5),
    "mm2c_pairplan_create": (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    "mm2c_pairplan_destroy": (None, [C.c_void_p]),
    "mm2c_pairplan_run_device": (C.c_int, [C.c_void_p, C.POINTER(PairOpt)] + [C.c_void_p] * 8),
    "mm2c_pairplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mm2c_pairplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_pair_ends_batch_host": (C.c_int, [C.c_int64, C.POINTER(PairOpt), C.c_int32] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4),
    "mm2c_errplan_create": (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mm2c_errplan_destroy": (None, [C.c_void_p]),
    "mm2c_errplan_run_device": (C.c_int, [C.c_void_p] * 9 + [C.c_int32] + [C.c_void_p] * 4),
    "mm2c_errplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mm2c_errplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_errplan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mm2c_est_err_div": (C.c_float, [C.c_int32, C.c_int32, C.c_float]),
    "mm2c_est_err_apply_host": (C.c_int, [C.c_int64] + [C.c_void_p] * 5),
    "mm2c_est_err_batch_host": (C.c_int, [C.c_int64] + [C.c_void_p] * 8 + [C.c_int32] + [C.c_void_p] * 3),
    "mm2c_seedplan_create": (C.c_void_p, [C.c_int64, C.c_void_p, C.c_void_p]),
    "mm2c_seedplan_destroy": (None, [C.c_void_p]),
    "mm2c_seedplan_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_seedplan_run_device_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                             C.c_void_p]),
    "mm2c_seedplan_run_device_skip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.c_int64, C.c_void_p, C.c_void_p]),
    "mm2c_seedplan_set_heap_sort": (C.c_int, [C.c_void_p, C.c_int]),
    "mm2c_seedplan_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mm2c_seedplan_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mm2c_seedplan_last_expand_mw": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mm2c_seed_hits_batch_host": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_seed_chain_batch_host": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_seed_chain_batch_pool": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_seed_hits_batch_host_skip": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_seed_chain_batch_host_skip": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_seed_chain_batch_pool_skip": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_hitpool_create": (C.c_void_p, [C.c_void_p, C.c_int64]),
    "mm2c_hitpool_size": (C.c_int64, [C.c_void_p]),
    "mm2c_hitpool_destroy": (None, [C.c_void_p]),
    "mm2c_minidx_create": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_minidx_destroy": (None, [C.c_void_p]),
    "mm2c_minidx_lookup": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_minidx_build": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_int)]),
    "mm2c_minidx_n_keys": (C.c_int64, [C.c_void_p]),
    "mm2c_minidx_n_hits": (C.c_int64, [C.c_void_p]),
    "mm2c_minidx_pool": (C.c_void_p, [C.c_void_p]),
    "mm2c_minidx_cal_max_occ": (C.c_int, [C.c_void_p, C.c_float]),
    "mm2c_minidx_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm2c_get_index_stats": (None, [C.POINTER(IndexStats)]),
    "mm2c_reset_index_stats": (None, []),
    "mm2c_read_result_create": (C.POINTER(ReadResult), []),
    "mm2c_read_result_free": (None, [C.POINTER(ReadResult)]),
    "mm2c_sketch_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(ReadResult)]),
    "mm2c_sketch_match_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(ReadResult)]),
    "mm2c_read_chain_batch": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(ReadResult)]),
    "mm2c_sketch_frag_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(ReadResult)]),
    "mm2c_sketch_match_frag_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(ReadResult)]),
    "mm2c_frag_chain_batch": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(ReadResult)]),
    "mm2c_frag_chain_batch_gaps": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(FragGaps), C.c_int64, C.c_void_p, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReadResult)]),
    "mm2c_read_result_task_dists": (C.c_int, [C.POINTER(ReadResult), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "mm2c_get_frag_stats": (None, [C.POINTER(FragStats)]),
    "mm2c_reset_frag_stats": (None, []),
    "mm2c_get_sketch_stats": (None, [C.POINTER(SketchStats)]),
    "mm2c_reset_sketch_stats": (None, []),
    "mm2c_get_stats": (None, [C.POINTER(Stats)]),
    "mm2c_get_stage_stats": (None, [C.POINTER(StageStats)]),
    "mm2c_reset_stage_stats": (None, []),
    "mm2c_stream_write": (C.c_int, [C.c_char_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "mm2c_stream_read": (C.c_int, [C.c_char_p, C.POINTER(Stream)]),
    "mm2c_stream_from_seed_dump": (C.c_int, [C.c_char_p, C.POINTER(Params), C.c_int, C.c_int, C.POINTER(Stream)]),
    "mm2c_stream_free": (None, [C.POINTER(Stream)]),
}
# C++-linkage drop-in symbols the reference objects import (chain_hardware.h:68-71)
CXX_SYMBOLS = {
    "_Z18run_chaining_on_hwliiiifP7mm128_tPiS1_Phliff": (C.c_int, [C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long,
                                                                   C.c_int, C.c_float, C.c_float]),
    "_Z13hardware_initlPc": (C.c_bool, [C.c_long, C.c_char_p]),
    "_Z7cleanupv": (None, []),
    "_Z10checkErroriNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEE": (None, [C.c_int, C.c_void_p]),   # chain_hardware.h:72 (a std::string by value: not callable from ctypes, only checked for presence)
}

_lib = None


def load():
    """dlopen the in-tree library and type every entry point; raises if it is absent (no CPU path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `make -C minimap2-fpga_amd` (or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in {**C_SYMBOLS, **CXX_SYMBOLS}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class SeedSkip(C.Structure):
    """mm2c_seed_skip_t"""
    _fields_ = [("flag", C.c_int32), ("d_ref_rank", C.c_void_p), ("d_ref_len", C.c_void_p), ("d_q_lo", C.c_void_p), ("d_q_eq", C.c_void_p)]


class SeedSkipHost(C.Structure):
    """mm2c_seed_skip_host_t"""
    _fields_ = [("flag", C.c_int32), ("n_ref", C.c_int32), ("ref_rank", C.c_void_p), ("ref_len", C.c_void_p), ("q_lo", C.c_void_p), ("q_eq", C.c_void_p)]


class Mm2cError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        msg = load().mm2c_last_error()
        raise Mm2cError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
