"""CPU test of the regions-to-hits side of include/mm2chain.h: mm2c_hit_opt_t's size and offsets, the sam_pri bit (minimap.h:96) and the LDS class as constants, the
section compiles as C99 and C++11 with the signatures the issue gives, the ctypes mirror agrees, the symbols are exported, params.hit_opts carries the numbers of
options.c:33-36, and the host-buffer entry makes its refusals before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
#define AT(f, o) typedef char f##_at_##o[offsetof(mm2c_hit_opt_t, f) == o ? 1 : -1]
AT(mask_level, 0); AT(mask_len, 4); AT(hard_mask_level, 8); AT(pri_ratio, 12); AT(min_diff, 16); AT(best_n, 20);
typedef char size_is_24[sizeof(mm2c_hit_opt_t) == 24 ? 1 : -1];
typedef char sam_pri_is_bit_12[MM2C_REG_SAM_PRI_BIT == 12 ? 1 : -1];
typedef char lds_class_is_128[MM2C_HIT_LDS_REGIONS == 128 ? 1 : -1];
mm2c_hitplan_t *(*f1)(int64_t, int64_t) = mm2c_hitplan_create;
void (*f2)(mm2c_hitplan_t *) = mm2c_hitplan_destroy;
int (*f3)(mm2c_hitplan_t *, const mm2c_hit_opt_t *, const int64_t *, const mm2c_reg_t *, mm2c_reg_t *, int32_t *, void *) = mm2c_hitplan_run_device;
int (*f4)(mm2c_hitplan_t *, int64_t *) = mm2c_hitplan_check;
int (*f5)(mm2c_hitplan_t *, float *) = mm2c_hitplan_last_ms;
int (*f6)(int64_t, const mm2c_hit_opt_t *, const int64_t *, const mm2c_reg_t *, mm2c_reg_t *, int32_t *) = mm2c_select_hits_batch_host;
int main(void) { mm2c_reg_t r; r.flags = 1u << MM2C_REG_SAM_PRI_BIT; return (int)(r.flags >> 12) - 1; }
'''


def test_hit_section_compiles(tmp_path):
    src = tmp_path / "h.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_ctypes_mirror_and_constants():
    from mm2chain import _native as N
    import hits_data
    import hits_model
    assert C.sizeof(N.HitOpt) == 24
    assert [(f, getattr(N.HitOpt, f).offset) for f, _ in N.HitOpt._fields_] == [("mask_level", 0), ("mask_len", 4), ("hard_mask_level", 8), ("pri_ratio", 12),
                                                                                 ("min_diff", 16), ("best_n", 20)]
    assert N.MM2C_REG_SAM_PRI_BIT == 12 == hits_model.SAM_PRI_BIT and N.MM2C_HIT_LDS_REGIONS == 128 == hits_data.LDS_CLASS
    assert int(np.load(os.path.join(GOLDEN, "ref_hits.npz"))["reg_size"]) == 80
    assert N.C_SYMBOLS["mm2c_hitplan_create"] == (C.c_void_p, [C.c_int64, C.c_int64])
    assert N.C_SYMBOLS["mm2c_hitplan_run_device"] == (C.c_int, [C.c_void_p, C.POINTER(N.HitOpt)] + [C.c_void_p] * 5)
    assert N.C_SYMBOLS["mm2c_hitplan_check"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)])
    assert N.C_SYMBOLS["mm2c_hitplan_last_ms"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float)])
    assert N.C_SYMBOLS["mm2c_select_hits_batch_host"] == (C.c_int, [C.c_int64, C.POINTER(N.HitOpt)] + [C.c_void_p] * 4)


def test_symbols_are_exported():
    import mm2chain
    from mm2chain import _native as N
    lib = N.load()
    for name in ("mm2c_hitplan_create", "mm2c_hitplan_destroy", "mm2c_hitplan_run_device", "mm2c_hitplan_check", "mm2c_hitplan_last_ms", "mm2c_select_hits_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    assert mm2chain.HitPlan is not None and mm2chain.select_hits_batch is not None and "HitPlan" in mm2chain.__all__ and "select_hits_batch" in mm2chain.__all__


def test_hit_opts_defaults_are_those_of_options_c():
    """options.c:33-36: mask_level 0.5f, mask_len INT_MAX, pri_ratio 0.8f, best_n 5; min_diff = 2k (map.c:253)"""
    from mm2chain import params
    o = params.hit_opts()
    assert (o.mask_level, o.mask_len, o.hard_mask_level, o.min_diff, o.best_n) == (0.5, 2**31 - 1, 0, 30, 5)
    assert np.float32(o.pri_ratio) == np.float32(0.8) and o.pri_ratio == float(np.float32(0.8))
    assert params.hit_opts(19).min_diff == 38 and params.hit_opts(k=21, pri_ratio=0.5, best_n=20).best_n == 20
    a = params.hit_opts(15, pri_ratio=0.0, hard_mask_level=True, mask_len=100, mask_level=0.3)
    assert (a.pri_ratio, a.hard_mask_level, a.mask_len) == (0.0, 1, 100) and np.float32(a.mask_level) == np.float32(0.3)
    with pytest.raises(TypeError):
        params.hit_opts(bestn=3)
    for word in ("ava-ont", "asm", "sr", "best_n 50", "pri_ratio 0"):
        assert word in params.hit_opts.__doc__


def test_host_entry_refuses_before_any_device_work():
    """non-monotone offsets and missing arrays: MM2C_E_ARG, with or without a device"""
    from mm2chain import _native as N, params
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    regs, out, n_out = np.zeros(8 * 80, np.uint8), np.zeros(8 * 80, np.uint8), np.zeros(4, np.int32)
    o = params.hit_opts()
    call = lambda off, r=regs: lib.mm2c_select_hits_batch_host(len(off) - 1, C.byref(o), ptr(np.asarray(off, np.int64)), ptr(r) if r is not None else None, ptr(out), ptr(n_out))
    assert call([0, 5, 3]) == -2 and b"region offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([4, 2]) == -2 and b"read 0" in lib.mm2c_last_error()
    assert call([0, 3], None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert lib.mm2c_select_hits_batch_host(-1, C.byref(o), None, None, None, None) == -2
    assert lib.mm2c_select_hits_batch_host(2, None, ptr(np.zeros(3, np.int64)), ptr(regs), ptr(out), ptr(n_out)) == -2
    assert lib.mm2c_select_hits_batch_host(0, C.byref(o), None, None, None, None) == 0
