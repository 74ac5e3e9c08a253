"""CPU test of the alignment-task section of include/mm2chain.h: the three structs' sizes and offsets, the section compiles as C99 and C++11 with the signatures the
interface gives, the NumPy record types and the ctypes mirror agree with them, the symbols are exported, params.aln_opts makes the reference's presets (options.c),
and the host entry and the plan make their argument refusals before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
typedef char opt_is_80[sizeof(mm2c_aln_opt_t) == 80 && offsetof(mm2c_aln_opt_t, e2) == 16 && offsetof(mm2c_aln_opt_t, bw_ext) == 24 && offsetof(mm2c_aln_opt_t, min_chain_score) == 28 &&
                       offsetof(mm2c_aln_opt_t, zdrop_inv) == 52 && offsetof(mm2c_aln_opt_t, max_sw_mat) == 56 && offsetof(mm2c_aln_opt_t, flag) == 64 && offsetof(mm2c_aln_opt_t, k) == 72 ? 1 : -1];
typedef char reg_is_104[sizeof(mm2c_aln_reg_t) == 104 && offsetof(mm2c_aln_reg_t, rs0) == 24 && offsetof(mm2c_aln_reg_t, n_items) == 40 && offsetof(mm2c_aln_reg_t, status) == 48 &&
                        offsetof(mm2c_aln_reg_t, rev) == 52 && offsetof(mm2c_aln_reg_t, item0) == 56 && offsetof(mm2c_aln_reg_t, q_off) == 80 && offsetof(mm2c_aln_reg_t, left_off) == 96 ? 1 : -1];
typedef char item_is_40[sizeof(mm2c_aln_item_t) == 40 && offsetof(mm2c_aln_item_t, kind) == 4 && offsetof(mm2c_aln_item_t, anchor) == 8 && offsetof(mm2c_aln_item_t, task) == 28 &&
                        offsetof(mm2c_aln_item_t, score) == 32 ? 1 : -1];
typedef char consts[MM2C_ALN_LDS_GAPS == 2048 && MM2C_ALN_MAX_SLOTS == 4096 && MM2C_ALN_REFUSED == 1 && MM2C_ALN_TOO_BIG == 2 && MM2C_ALN_OVER_CAP == 3 && MM2C_ALN_F_SR == 1 &&
                    MM2C_ALN_F_NO_END_FLT == 2 && MM2C_ALN_F_SPLICE == 4 && MM2C_ALN_I_HPC == 1 && MM2C_ALN_LEFT == 0 && MM2C_ALN_GAP == 1 && MM2C_ALN_RIGHT == 2 && MM2C_ALN_UNGAPPED == 3 &&
                    MM2C_ALN_OVER == 16 && MM2C_REG_SPLIT_INV_BIT == 24 ? 1 : -1];
mm2c_refseq_t *(*f1)(int64_t, const uint64_t *, const uint32_t *, const uint32_t *, int64_t) = mm2c_refseq_create;
void (*f2)(mm2c_refseq_t *) = mm2c_refseq_destroy;
mm2c_alnplan_t *(*f3)(int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int32_t, int64_t, int64_t) = mm2c_alnplan_create;
void (*f4)(mm2c_alnplan_t *) = mm2c_alnplan_destroy;
int (*f5)(mm2c_alnplan_t *, const mm2c_aln_opt_t *, const mm2c_refseq_t *, int64_t, int64_t, const int64_t *, const mm2c_reg_t *, const int64_t *, const int64_t *, void *, const int64_t *,
          const uint8_t *, mm2c_aln_reg_t *, mm2c_aln_item_t *, mm2c_ksw_task_t *, int64_t *, uint8_t *, void *) = mm2c_alnplan_run_device;
int (*f6)(mm2c_alnplan_t *, int64_t *, int64_t *, int64_t *) = mm2c_alnplan_check;
int (*f7)(mm2c_alnplan_t *, float *) = mm2c_alnplan_last_kernel_ms;
int (*f8)(const mm2c_aln_opt_t *, int64_t, const uint64_t *, const uint32_t *, const uint32_t *, int64_t, int64_t, const int64_t *, const mm2c_reg_t *, const int64_t *, mm2c_anchor_t *,
          const int64_t *, const uint8_t *, int32_t, mm2c_aln_reg_t *, int64_t, mm2c_aln_item_t *, int64_t, mm2c_ksw_task_t *, int64_t *, int64_t, uint8_t *, int64_t *) = mm2c_align_tasks_batch_host;
int main(void) { mm2c_aln_item_t t; t.kind = 0; return t.kind; }
'''


def test_aln_section_compiles(tmp_path):
    src = tmp_path / "m.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_mirror_symbols_and_params():
    import mm2chain
    from mm2chain import _native as N, params
    import aln_data
    import aln_model
    offs = lambda dt: [(n, dt.fields[n][1]) for n in dt.names]
    assert mm2chain.ALN_OPT_DTYPE.itemsize == 80 and dict(offs(mm2chain.ALN_OPT_DTYPE))["max_sw_mat"] == 56 and dict(offs(mm2chain.ALN_OPT_DTYPE))["k"] == 72
    assert mm2chain.ALN_REG_DTYPE.itemsize == 104 and offs(mm2chain.ALN_REG_DTYPE) == offs(aln_model.ALN_REG_DTYPE) and dict(offs(mm2chain.ALN_REG_DTYPE))["left_off"] == 96
    assert mm2chain.ALN_ITEM_DTYPE.itemsize == 40 and offs(mm2chain.ALN_ITEM_DTYPE) == offs(aln_model.ALN_ITEM_DTYPE)
    assert offs(mm2chain.KSW_TASK_DTYPE) == offs(aln_model.KSW_TASK_DTYPE) and offs(mm2chain.REG_DTYPE) == offs(aln_model.REG_DTYPE) == offs(aln_data.REG_DTYPE)
    assert (mm2chain.ALN_REFUSED, mm2chain.ALN_TOO_BIG, mm2chain.ALN_OVER_CAP, mm2chain.ALN_LDS_GAPS) == (1, 2, 3, 2048)
    lib = N.load()
    for name in ("mm2c_refseq_create", "mm2c_refseq_destroy", "mm2c_alnplan_create", "mm2c_alnplan_destroy", "mm2c_alnplan_run_device", "mm2c_alnplan_check", "mm2c_alnplan_last_kernel_ms",
                 "mm2c_align_tasks_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    for name in ("RefSeq", "AlnPlan", "align_tasks_batch", "ALN_OPT_DTYPE", "ALN_REG_DTYPE", "ALN_ITEM_DTYPE"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__
    # the reference's presets (options.c:24-27, 45-50 and :91-135); bw_ext is :580
    ont = params.aln_opts()
    assert ont == dict(a=2, b=4, q=4, e=2, e2=1, bw=500, bw_ext=751, min_chain_score=40, max_gap=5000, min_cnt=3, min_ksw_len=200, end_bonus=-1, zdrop=400, zdrop_inv=200, max_sw_mat=0,
                       flag=0, idx_flag=0, k=15, reserved=0)
    assert params.aln_opts("map-pb") == dict(ont, idx_flag=1, k=19)
    assert params.aln_opts("asm20") == dict(ont, a=1, b=4, q=6, e=2, zdrop=200, zdrop_inv=200, k=19)
    assert params.aln_opts("sr") == dict(ont, b=8, q=12, bw=100, bw_ext=151, min_chain_score=25, max_gap=100, min_cnt=2, end_bonus=10, zdrop=100, zdrop_inv=100, flag=1, k=21)
    assert params.aln_opts(bw=2000)["bw_ext"] == 3001 and params.aln_opts(flag=2)["flag"] == 2
    # the fixture's option sets are these presets
    for name, preset in (("ont", "map-ont"), ("asm20", "asm20")):
        o = aln_data.OPTS[name]
        assert all(o[k] == v for k, v in params.aln_opts(preset).items() if k in o)
    rec = mm2chain.batch._aln_opt_bytes(params.aln_opts("sr", max_sw_mat=1 << 40))
    assert rec.tobytes()[56:64] == (1 << 40).to_bytes(8, "little") and int(rec["k"][0]) == 21


def test_host_entry_and_plan_refuse_before_any_device_work():
    """NULL options, e <= 0, k out of range, a contig that leaves S, negative counts, offsets that do not start at 0 or run backwards, missing arrays, a base code above 4
    in the reads or in a contig: MM2C_E_ARG, with or without a device"""
    import mm2chain
    from mm2chain import _native as N, params
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    opt = mm2chain.batch._aln_opt_bytes(params.aln_opts())
    off, ln, S = np.array([0, 20], np.uint64), np.array([20, 12], np.uint32), np.zeros(4, np.uint32)
    regs = np.zeros(1, mm2chain.REG_DTYPE); regs["cnt"] = 1
    b = np.array([[10, (15 << 32) | 20]], np.uint64)
    reads = np.zeros(40, np.uint8)
    ar, it, tk, co, pool, tot = np.zeros(1, mm2chain.ALN_REG_DTYPE), np.zeros(4, mm2chain.ALN_ITEM_DTYPE), np.zeros(4, mm2chain.KSW_TASK_DTYPE), np.zeros(5, np.int64), np.zeros(256, np.uint8), (C.c_int64 * 4)()

    def go(o=opt, n_seq=2, off_=off, ln_=ln, S_=S, n_words=4, n_reads=1, uo=(0, 1), rg=regs, bo=(0, 1), b_=b, ro=(0, 40), rd=reads, shift=0, ar_=ar, ni=4, it_=it, nt=4, tk_=tk, co_=co,
           pc=256, pool_=pool):
        return lib.mm2c_align_tasks_batch_host(ptr(o), n_seq, ptr(off_), ptr(ln_), ptr(S_), n_words, n_reads, ptr(np.asarray(uo, np.int64)), ptr(rg), ptr(np.asarray(bo, np.int64)), ptr(b_),
                                               ptr(np.asarray(ro, np.int64)), ptr(rd), shift, ptr(ar_), ni, ptr(it_), nt, ptr(tk_), ptr(co_), pc, ptr(pool_), tot)
    assert go(o=None) == -2 and b"options are NULL" in lib.mm2c_last_error()
    bad = opt.copy(); bad["e"] = 0
    assert go(o=bad) == -2 and b"e must be > 0" in lib.mm2c_last_error()
    bad = opt.copy(); bad["k"] = 0
    assert go(o=bad) == -2 and b"k outside" in lib.mm2c_last_error()
    assert go(ln_=np.array([20, 13], np.uint32)) == -2 and b"contig 1 leaves the 4 words" in lib.mm2c_last_error()
    assert go(ln_=np.array([20, 1 << 31], np.uint32)) == -2 and go(n_seq=-1) == -2 and go(n_words=-1) == -2 and go(S_=None) == -2 and go(off_=None) == -2
    assert go(n_reads=-1) == -2 and go(n_reads=0) == 0 and go(ni=-1) == -2 and go(nt=-1) == -2 and go(pc=-1) == -2 and go(shift=-1) == -2 and go(shift=31) == -2
    assert go(uo=(1, 1)) == -2 and b"must be 0" in lib.mm2c_last_error()
    assert go(uo=(0, -1)) == -2 and b"not monotone at read 0" in lib.mm2c_last_error()
    assert go(bo=(0, -1)) == -2 and go(ro=(0, -1)) == -2
    for k in ("rg", "b_", "rd", "ar_", "it_", "tk_", "pool_"):
        assert go(**{k: None}) == -2 and b"NULL" in lib.mm2c_last_error(), k
    r5 = reads.copy(); r5[7] = 5
    assert go(rd=r5) == -2 and b"base code 5 at 7 of the reads" in lib.mm2c_last_error()
    S5 = S.copy(); S5[3] = 6 << 4                          # base 25 of S = base 5 of contig 1
    assert go(S_=S5) == -2 and b"at 5 of contig 1" in lib.mm2c_last_error()
    S6 = S.copy(); S6[0] = 7                                # outside no contig? base 0 belongs to contig 0
    assert go(S_=S6) == -2
    # the plan's own refusals need no plan
    assert lib.mm2c_alnplan_run_device(None, ptr(opt), None, 0, 0, *([None] * 13)) == -2 and lib.mm2c_alnplan_check(None, None, None, None) == -2
    ms = (C.c_float * 3)()
    assert lib.mm2c_alnplan_last_kernel_ms(None, ms) == -2
    lib.mm2c_alnplan_destroy(None); lib.mm2c_refseq_destroy(None)
