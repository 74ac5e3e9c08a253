"""CPU test of the hits-to-mapping-quality side of include/mm2chain.h: mm2c_mapq_opt_t's size and offsets, the constants, the section compiles as C99 and C++11
with the signatures the interface gives, the ctypes mirror agrees, the symbols are exported, params.mapq_opts carries the numbers of options.c, and the
host-buffer entry and the plan make their refusals before any device work."""
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
#define AT(f, o) typedef char f##_at_##o[offsetof(mm2c_mapq_opt_t, f) == o ? 1 : -1]
AT(do_join, 0); AT(max_join_long, 4); AT(max_join_short, 8); AT(min_join_flank_sc, 12); AT(min_join_flank_ratio, 16); AT(min_cnt, 20); AT(min_chain_score, 24);
typedef char size_is_28[sizeof(mm2c_mapq_opt_t) == 28 ? 1 : -1];
typedef char table_cap[MM2C_MAPQ_MAX_LOG_ARG == (1 << 24) - 1 ? 1 : -1];
typedef char join_bit[MM2C_SEED_LONG_JOIN_BIT == 40 ? 1 : -1];
mm2c_mapqplan_t *(*f1)(int64_t, int64_t, int64_t, int32_t) = mm2c_mapqplan_create;
void (*f2)(mm2c_mapqplan_t *) = mm2c_mapqplan_destroy;
int (*f3)(mm2c_mapqplan_t *, const mm2c_mapq_opt_t *, const int64_t *, const mm2c_reg_t *, const int32_t *, const int64_t *, const void *, const int32_t *,
          const int32_t *, mm2c_reg_t *, int32_t *, void *, int64_t *, void *) = mm2c_mapqplan_run_device;
int (*f4)(mm2c_mapqplan_t *, int64_t *, int64_t *) = mm2c_mapqplan_check;
int (*f5)(mm2c_mapqplan_t *, float *) = mm2c_mapqplan_last_ms;
int (*f6)(mm2c_mapqplan_t *, float *, float *) = mm2c_mapqplan_last_kernel_ms;
int (*f7)(int64_t, const mm2c_mapq_opt_t *, int32_t, const int64_t *, const mm2c_reg_t *, const int32_t *, const int64_t *, const mm2c_anchor_t *, const int32_t *,
          const int32_t *, mm2c_reg_t *, int32_t *, mm2c_anchor_t *, int64_t *) = mm2c_join_mapq_batch_host;
int main(void) { mm2c_mapq_opt_t o; o.min_cnt = 3; return o.min_cnt - 3; }
'''


def test_mapq_section_compiles(tmp_path):
    src = tmp_path / "m.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_ctypes_mirror_and_constants():
    from mm2chain import _native as N
    import mapq_data
    import mapq_model
    assert C.sizeof(N.MapqOpt) == 28
    assert [(f, getattr(N.MapqOpt, f).offset) for f, _ in N.MapqOpt._fields_] == [("do_join", 0), ("max_join_long", 4), ("max_join_short", 8), ("min_join_flank_sc", 12),
                                                                                   ("min_join_flank_ratio", 16), ("min_cnt", 20), ("min_chain_score", 24)]
    assert N.MM2C_MAPQ_MAX_LOG_ARG == 2**24 - 1 and 1 << N.MM2C_SEED_LONG_JOIN_BIT == mapq_model.MM_SEED_LONG_JOIN and N.MM2C_HIT_LDS_REGIONS == mapq_data.LDS_CLASS
    assert float(np.float32(N.MM2C_MAPQ_MAX_LOG_ARG)) == N.MM2C_MAPQ_MAX_LOG_ARG and float(np.float32(N.MM2C_MAPQ_MAX_LOG_ARG + 2)) != N.MM2C_MAPQ_MAX_LOG_ARG + 2
    assert int(np.load(os.path.join(GOLDEN, "ref_mapq.npz"))["reg_size"]) == 80
    assert N.C_SYMBOLS["mm2c_mapqplan_create"] == (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int32])
    assert N.C_SYMBOLS["mm2c_mapqplan_run_device"] == (C.c_int, [C.c_void_p, C.POINTER(N.MapqOpt)] + [C.c_void_p] * 12)
    assert N.C_SYMBOLS["mm2c_mapqplan_check"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    assert N.C_SYMBOLS["mm2c_mapqplan_last_ms"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float)])
    assert N.C_SYMBOLS["mm2c_mapqplan_last_kernel_ms"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)])
    assert N.C_SYMBOLS["mm2c_join_mapq_batch_host"] == (C.c_int, [C.c_int64, C.POINTER(N.MapqOpt), C.c_int32] + [C.c_void_p] * 11)


def test_symbols_are_exported():
    import mm2chain
    from mm2chain import _native as N
    lib = N.load()
    for name in ("mm2c_mapqplan_create", "mm2c_mapqplan_destroy", "mm2c_mapqplan_run_device", "mm2c_mapqplan_check", "mm2c_mapqplan_last_ms",
                 "mm2c_mapqplan_last_kernel_ms", "mm2c_join_mapq_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    assert mm2chain.MapqPlan is not None and mm2chain.join_mapq_batch is not None and "MapqPlan" in mm2chain.__all__ and "join_mapq_batch" in mm2chain.__all__


def test_mapq_opts_defaults_are_those_of_options_c():
    """options.c:24-25, 38-41: min_cnt 3, min_chain_score 40, max_join_long 20000, max_join_short 2000, min_join_flank_sc 1000, min_join_flank_ratio 0.5f"""
    from mm2chain import params
    import mapq_data
    o = params.mapq_opts()
    assert {k: getattr(o, k) for k, _ in o._fields_} == mapq_data.MAPQ_DEFAULT
    a = params.mapq_opts(do_join=False, min_cnt=2, min_chain_score=25, min_join_flank_ratio=0.01)
    assert (a.do_join, a.min_cnt, a.min_chain_score, a.max_join_long) == (0, 2, 25, 20000) and np.float32(a.min_join_flank_ratio) == np.float32(0.01)
    with pytest.raises(TypeError):
        params.mapq_opts(min_count=3)
    for word in ("MM_F_NO_LJOIN", "sr", "splice", "ava-ont"):
        assert word in params.mapq_opts.__doc__


def test_host_entry_refuses_before_any_device_work():
    """offsets that are not monotone, n_in beyond its room, missing arrays, a table beyond 2^24 - 1: MM2C_E_ARG, with or without a device"""
    from mm2chain import _native as N, params
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    regs, out, b = np.zeros(8 * 80, np.uint8), np.zeros(8 * 80, np.uint8), np.zeros((16, 2), np.uint64)
    n_out, q, rep = np.zeros(4, np.int32), np.full(4, 1000, np.int32), np.zeros(4, np.int32)
    o = params.mapq_opts()

    def call(u_off, n_in, b_off, r=regs, table=4096, b_out=None, n_b_out=None, opt=o):
        return lib.mm2c_join_mapq_batch_host(len(u_off) - 1, C.byref(opt) if opt is not None else None, table, ptr(np.asarray(u_off, np.int64)), ptr(r),
                                             ptr(np.asarray(n_in, np.int32)), ptr(np.asarray(b_off, np.int64)), ptr(b), ptr(q), ptr(rep), ptr(out), ptr(n_out),
                                             ptr(b_out), ptr(n_b_out))
    assert call([0, 5, 3], [1, 1], [0, 4, 8]) == -2 and b"region offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([0, 3, 5], [1, 1], [0, 9, 8]) == -2 and b"anchor offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([0, 3, 5], [1, 3], [0, 4, 8]) == -2 and b"read 1: 3 hits in room for 2" in lib.mm2c_last_error()
    assert call([0, 3, 5], [-1, 1], [0, 4, 8]) == -2 and b"read 0" in lib.mm2c_last_error()
    assert call([0, 3], [1], [0, 4], r=None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert call([0, 3], [1], [0, 4], b_out=b) == -2 and b"together" in lib.mm2c_last_error()
    assert call([0, 3], [1], [0, 4], table=1 << 24) == -2 and call([0, 3], [1], [0, 4], table=-1) == -2 and call([0, 3], [1], [0, 4], opt=None) == -2
    assert lib.mm2c_join_mapq_batch_host(-1, C.byref(o), 4096, *([None] * 11)) == -2
    assert lib.mm2c_join_mapq_batch_host(0, C.byref(o), 4096, *([None] * 11)) == 0
    # the plan's own refusals need no plan
    assert lib.mm2c_mapqplan_run_device(None, C.byref(o), *([None] * 12)) == -2 and lib.mm2c_mapqplan_check(None, None, None) == -2
    ms = C.c_float(0)
    assert lib.mm2c_mapqplan_last_ms(None, C.byref(ms)) == -2 and lib.mm2c_mapqplan_last_kernel_ms(None, C.byref(ms), C.byref(ms)) == -2
    lib.mm2c_mapqplan_destroy(None)
