"""CPU test of the fragment side of include/mm2chain.h behind mm_gen_regs: mm2c_hit_multi_opt_t's size and offsets, the two sections compile as C99 and C++11 with
the signatures the interface gives, the ctypes mirror agrees, the symbols are exported, and the host-buffer entries and the plans make their refusals before any
device work."""
import ctypes as C
import os
import subprocess

import numpy as np

from regs_model import REG as N_REG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
typedef char pri1_at_0[offsetof(mm2c_hit_multi_opt_t, pri1) == 0 ? 1 : -1];
typedef char pri2_at_4[offsetof(mm2c_hit_multi_opt_t, pri2) == 4 ? 1 : -1];
typedef char n_segs_at_8[offsetof(mm2c_hit_multi_opt_t, n_segs) == 8 ? 1 : -1];
typedef char gap_at_12[offsetof(mm2c_hit_multi_opt_t, max_gap_ref) == 12 ? 1 : -1];
typedef char size_is_16[sizeof(mm2c_hit_multi_opt_t) == 16 ? 1 : -1];
typedef char flags_at_60[offsetof(mm2c_reg_t, flags) == 60 ? 1 : -1];
typedef char consts[MM2C_MAX_SEG == 255 && MM2C_REG_SEG_SPLIT_BIT == 15 && MM2C_REG_SEG_ID_SHIFT == 16 ? 1 : -1];
int (*f1)(mm2c_hitplan_t *, const mm2c_hit_opt_t *, const mm2c_hit_multi_opt_t *, const int64_t *, const int32_t *, const int32_t *, const mm2c_reg_t *, mm2c_reg_t *,
          int32_t *, void *) = mm2c_hitplan_run_device_multi;
int (*f2)(int64_t, const mm2c_hit_opt_t *, const mm2c_hit_multi_opt_t *, const int64_t *, const int32_t *, const int32_t *, const mm2c_reg_t *, mm2c_reg_t *,
          int32_t *) = mm2c_select_hits_multi_batch_host;
mm2c_segplan_t *(*f3)(int64_t, int32_t, int64_t, int64_t) = mm2c_segplan_create;
void (*f4)(mm2c_segplan_t *) = mm2c_segplan_destroy;
int64_t (*f5)(const mm2c_segplan_t *) = mm2c_segplan_seg_chain_cap;
int (*f6)(mm2c_segplan_t *, const int64_t *, const mm2c_reg_t *, const int32_t *, const int64_t *, const void *, const int32_t *, const uint32_t *, const int32_t *,
          int64_t *, uint64_t *, int64_t *, void *, mm2c_reg_t *, uint32_t *, int32_t *, void *) = mm2c_segplan_run_device;
int (*f7)(mm2c_segplan_t *, int64_t *, int64_t *, int64_t *) = mm2c_segplan_check;
int (*f8)(mm2c_segplan_t *, float *) = mm2c_segplan_last_ms;
int (*f9)(mm2c_segplan_t *, float *, float *, float *, float *, float *) = mm2c_segplan_last_kernel_ms;
int (*f10)(int64_t, int32_t, const int64_t *, const mm2c_reg_t *, const int32_t *, const int64_t *, const mm2c_anchor_t *, const int32_t *, const uint32_t *,
           const int32_t *, int64_t *, uint64_t *, int64_t *, mm2c_anchor_t *, mm2c_reg_t *, uint32_t *, int32_t *) = mm2c_seg_gen_batch_host;
int main(void) { mm2c_hit_multi_opt_t m; m.n_segs = 2; return m.n_segs - 2; }
'''


def test_fragment_sections_compile(tmp_path):
    src = tmp_path / "m.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_ctypes_mirror_and_symbols():
    import mm2chain
    from mm2chain import _native as N, params
    assert C.sizeof(N.HitMultiOpt) == 16 and [(f, getattr(N.HitMultiOpt, f).offset) for f, _ in N.HitMultiOpt._fields_] == [("pri1", 0), ("pri2", 4), ("n_segs", 8), ("max_gap_ref", 12)]
    assert (N.MM2C_MAX_SEG, N.MM2C_REG_SEG_SPLIT_BIT, N.MM2C_REG_SEG_ID_SHIFT) == (255, 15, 16)
    m = params.hit_multi_opts()
    assert (m.n_segs, m.max_gap_ref) == (2, 500) and np.float32(m.pri1) == np.float32(0.2) and np.float32(m.pri2) == np.float32(0.7)
    assert params.hit_multi_opts(3, 100, 0.25, 0.5).n_segs == 3
    assert N.C_SYMBOLS["mm2c_hitplan_run_device_multi"] == (C.c_int, [C.c_void_p, C.POINTER(N.HitOpt), C.POINTER(N.HitMultiOpt)] + [C.c_void_p] * 7)
    assert N.C_SYMBOLS["mm2c_segplan_create"] == (C.c_void_p, [C.c_int64, C.c_int32, C.c_int64, C.c_int64])
    assert N.C_SYMBOLS["mm2c_segplan_run_device"] == (C.c_int, [C.c_void_p] * 17)
    assert N.C_SYMBOLS["mm2c_seg_gen_batch_host"] == (C.c_int, [C.c_int64, C.c_int32] + [C.c_void_p] * 15)
    lib = N.load()
    for name in ("mm2c_hitplan_run_device_multi", "mm2c_select_hits_multi_batch_host", "mm2c_segplan_create", "mm2c_segplan_destroy", "mm2c_segplan_seg_chain_cap",
                 "mm2c_segplan_run_device", "mm2c_segplan_check", "mm2c_segplan_last_ms", "mm2c_segplan_last_kernel_ms", "mm2c_seg_gen_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    for name in ("select_hits_multi_batch", "SegPlan", "seg_gen_batch"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__
    assert hasattr(mm2chain.HitPlan, "run_multi")


def test_host_entries_and_plans_refuse_before_any_device_work():
    """bad n_segs, offsets that are not monotone, n_in beyond its room, missing arrays, a region beyond the fragment's anchors, an anchor of a segment >= n_segs:
    MM2C_E_ARG, with or without a device"""
    from mm2chain import _native as N, params
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    opt = params.hit_opts()
    regs = np.zeros(8, N_REG)
    out, n_out, sl = np.zeros(8, N_REG), np.zeros(4, np.int32), np.full(8, 150, np.int32)

    def sel(u_off, n_segs=2, seg_len=sl, r=regs, mopt=True):
        m = params.hit_multi_opts(n_segs)
        return lib.mm2c_select_hits_multi_batch_host(len(u_off) - 1, C.byref(opt), C.byref(m) if mopt else None, ptr(np.asarray(u_off, np.int64)), ptr(seg_len), None, ptr(r),
                                                     ptr(out), ptr(n_out))
    assert sel([0, 5, 3]) == -2 and b"region offsets not monotone at read 1" in lib.mm2c_last_error()
    assert sel([0, 3], n_segs=0) == -2 and b"n_segs 0" in lib.mm2c_last_error()
    assert sel([0, 3], n_segs=256) == -2 and sel([0, 3], seg_len=None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert sel([0, 3], r=None) == -2 and sel([0, 3], mopt=False) == -2
    assert lib.mm2c_hitplan_run_device_multi(None, C.byref(opt), C.byref(params.hit_multi_opts()), *([None] * 7)) == -2
    assert lib.mm2c_hitplan_run_device_multi(None, C.byref(opt), None, *([None] * 7)) == -2

    b = np.zeros((16, 2), np.uint64)
    h, rl = np.zeros(4, np.uint32), np.zeros(4, np.int32)
    su_off, sb_off, su, sb, sr, sh = np.zeros(9, np.int64), np.zeros(9, np.int64), np.zeros(16, np.uint64), np.zeros((16, 2), np.uint64), np.zeros(16, N_REG), np.zeros(8, np.uint32)

    def seg(u_off, n_in, b_off, n_segs=2, r=regs, bb=b, seg_len=sl, hash_=h):
        return lib.mm2c_seg_gen_batch_host(len(u_off) - 1, n_segs, ptr(np.asarray(u_off, np.int64)), ptr(r), ptr(np.asarray(n_in, np.int32)), ptr(np.asarray(b_off, np.int64)),
                                           ptr(bb), ptr(seg_len), ptr(hash_), None, ptr(su_off), ptr(su), ptr(sb_off), ptr(sb), ptr(sr), ptr(sh), None)
    assert seg([0, 5, 3], [1, 1], [0, 4, 8]) == -2 and b"region offsets not monotone at fragment 1" in lib.mm2c_last_error()
    assert seg([0, 3, 5], [1, 1], [0, 9, 8]) == -2 and b"anchor offsets not monotone at fragment 1" in lib.mm2c_last_error()
    assert seg([0, 3, 5], [1, 3], [0, 4, 8]) == -2 and b"fragment 1: 3 regions in room for 2" in lib.mm2c_last_error()
    assert seg([0, 3, 5], [-1, 1], [0, 4, 8]) == -2 and b"fragment 0" in lib.mm2c_last_error()
    assert seg([0, 3], [1], [0, 4], n_segs=0) == -2 and seg([0, 3], [1], [0, 4], n_segs=256) == -2
    assert seg([0, 3], [1], [0, 4], r=None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert seg([0, 3], [1], [0, 4], seg_len=None) == -2 and seg([0, 3], [1], [0, 4], hash_=None) == -2
    r2 = regs.copy(); r2["cnt"][0], r2["as"][0] = 3, 2                           # [2, 5) of 4 anchors
    assert seg([0, 3], [1], [0, 4], r=r2) == -2 and b"region 0 leaves the fragment's anchors" in lib.mm2c_last_error()
    r2["as"][0] = -1
    assert seg([0, 3], [1], [0, 4], r=r2) == -2 and b"leaves the fragment's anchors" in lib.mm2c_last_error()
    r2["as"][0], r2["cnt"][1], r2["as"][1] = 0, 3, 1                             # two hits of three anchors among four
    assert seg([0, 3], [2], [0, 4], r=r2) == -2 and b"region 1 leaves the fragment's anchors" in lib.mm2c_last_error()
    b2 = b.copy(); b2[2, 1] = np.uint64(2) << np.uint64(48)
    assert seg([0, 3], [1], [0, 4], r=r2, bb=b2) == -2 and b"an anchor of segment 2 with n_segs 2" in lib.mm2c_last_error()
    assert lib.mm2c_seg_gen_batch_host(-1, 2, *([None] * 15)) == -2 and lib.mm2c_seg_gen_batch_host(0, 2, *([None] * 15)) == 0
    # the plan's own refusals need no plan
    assert lib.mm2c_segplan_run_device(None, *([None] * 16)) == -2 and lib.mm2c_segplan_check(None, None, None, None) == -2
    ms = C.c_float(0)
    assert lib.mm2c_segplan_last_ms(None, C.byref(ms)) == -2 and lib.mm2c_segplan_last_kernel_ms(None, *([C.byref(ms)] * 5)) == -2
    assert lib.mm2c_segplan_seg_chain_cap(None) == 0
    lib.mm2c_segplan_destroy(None)
