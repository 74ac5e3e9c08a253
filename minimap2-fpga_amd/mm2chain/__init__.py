"""mm2chain: MI355X-native chaining DP (mm_chain_dp hot path of kisarur/minimap2-fpga) behind the reference's
dispatch surface.  The compute lives in libmm2chain_hip.so (HIP, gfx950); this package is the host-side mirror."""
from ._native import Params, Mm2cError, LIB_PATH, MM2C_F_IGNORE_SEG, MM2C_F_FORCE_GENERAL, load
from . import params, synth, sharding, stream
from .batch import (device_identity, last_host_variant, init, split_model, init_devices, device_count, split_tasks, shutdown, device_info, tune, tune_get, tune_keys, tuned, ChainPlan, chain_batch_host, chain_batch_host_into, PinnedArray, chain_task, hardware_init, cleanup,
                    run_chaining_on_hw, mm_chain_dp, mm_chain_dp_batch, chain_epilogue_host, SeedPlan, seed_hits_batch, seed_chain_batch, MATCH_DTYPE,
                    HitPool, seed_chain_batch_pool, stage_stats, slot_stats, chain_task_pred, SeedSkip, seed_hits_batch_skip, seed_chain_batch_skip,
                    seed_chain_batch_pool_skip, MinimizerIndex, sketch_batch, sketch_match_batch, read_chain_batch, sketch_stats, index_stats,
                    sketch_frag_batch, sketch_match_frag_batch, frag_chain_batch, frag_stats, frag_chain_batch_gaps, frag_gaps,
                    RegPlan, REG_DTYPE, gen_regs_batch, read_hash, HitPlan, select_hits_batch, MapqPlan, join_mapq_batch,
                    EstErrPlan, est_err_batch, est_err_div, est_err_apply, ERR_DTYPE, select_hits_multi_batch, SegPlan, seg_gen_batch,
                    KswPlan, ksw_extd2_batch, ksw_task_scratch, KSW_TASK_DTYPE, KSW_RES_DTYPE, KSW_REFUSED, KSW_TOO_BIG, KSW_CIGAR_CUT,
                    ExtraPlan, update_extra_batch, test_zdrop_batch, EXTRA_TASK_DTYPE, EXTRA_RES_DTYPE, ZDROP_OPT_DTYPE, ZDROP_RES_DTYPE, EXTRA_REFUSED, EXTRA_TOO_BIG,
                    EXTRA_CIGAR_CUT, EXTRA_LDS_WORDS,
                    RefSeq, AlnPlan, align_tasks_batch, ALN_OPT_DTYPE, ALN_REG_DTYPE, ALN_ITEM_DTYPE, ALN_REFUSED, ALN_TOO_BIG, ALN_OVER_CAP, ALN_LDS_GAPS,
                    CigPlan, second_pass_batch, assemble_regions_batch, CIG_OPT_DTYPE, CIG_REG_DTYPE, CIG_REFUSED, CIG_INCOMPLETE, CIG_OVER_CAP, CIG_PIECE, CIG_NO_ROOM, CIG_LOST,
                    FinPlan, apply_regions_batch, finish_regions_batch, interleave_rounds, PEXT_DTYPE, FIN_REFUSED, FIN_INCOMPLETE, FIN_OVER_CAP, PairPlan, pair_ends_batch)

__all__ = ["Params", "Mm2cError", "LIB_PATH", "MM2C_F_IGNORE_SEG", "MM2C_F_FORCE_GENERAL", "load", "params", "synth",
           "sharding", "stream", "device_identity", "last_host_variant", "init", "split_model", "init_devices", "device_count", "split_tasks", "shutdown", "device_info", "tune", "tune_get", "tune_keys", "tuned", "ChainPlan", "chain_batch_host", "chain_batch_host_into", "PinnedArray", "chain_task", "hardware_init",
           "cleanup", "run_chaining_on_hw", "mm_chain_dp", "mm_chain_dp_batch", "chain_epilogue_host", "SeedPlan", "seed_hits_batch", "seed_chain_batch", "MATCH_DTYPE",
           "HitPool", "seed_chain_batch_pool", "stage_stats", "slot_stats", "chain_task_pred", "SeedSkip", "seed_hits_batch_skip", "seed_chain_batch_skip",
           "seed_chain_batch_pool_skip", "MinimizerIndex", "sketch_batch", "sketch_match_batch", "read_chain_batch", "sketch_stats", "index_stats",
           "sketch_frag_batch", "sketch_match_frag_batch", "frag_chain_batch", "frag_stats", "frag_chain_batch_gaps", "frag_gaps",
           "RegPlan", "REG_DTYPE", "gen_regs_batch", "read_hash", "HitPlan", "select_hits_batch", "MapqPlan", "join_mapq_batch",
           "EstErrPlan", "est_err_batch", "est_err_div", "est_err_apply", "ERR_DTYPE",
           "select_hits_multi_batch", "SegPlan", "seg_gen_batch",
           "KswPlan", "ksw_extd2_batch", "ksw_task_scratch", "KSW_TASK_DTYPE", "KSW_RES_DTYPE", "KSW_REFUSED", "KSW_TOO_BIG", "KSW_CIGAR_CUT",
           "ExtraPlan", "update_extra_batch", "test_zdrop_batch", "EXTRA_TASK_DTYPE", "EXTRA_RES_DTYPE", "ZDROP_OPT_DTYPE", "ZDROP_RES_DTYPE", "EXTRA_REFUSED", "EXTRA_TOO_BIG",
           "EXTRA_CIGAR_CUT", "EXTRA_LDS_WORDS",
           "RefSeq", "AlnPlan", "align_tasks_batch", "ALN_OPT_DTYPE", "ALN_REG_DTYPE", "ALN_ITEM_DTYPE", "ALN_REFUSED", "ALN_TOO_BIG", "ALN_OVER_CAP", "ALN_LDS_GAPS",
           "CigPlan", "second_pass_batch", "assemble_regions_batch", "CIG_OPT_DTYPE", "CIG_REG_DTYPE", "CIG_REFUSED", "CIG_INCOMPLETE", "CIG_OVER_CAP", "CIG_PIECE", "CIG_NO_ROOM", "CIG_LOST",
           "FinPlan", "apply_regions_batch", "finish_regions_batch", "interleave_rounds", "PEXT_DTYPE", "FIN_REFUSED", "FIN_INCOMPLETE", "FIN_OVER_CAP", "PairPlan", "pair_ends_batch"]
