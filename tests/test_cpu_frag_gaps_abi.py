"""CPU test of the per-fragment-distances side of include/mm2chain.h: mm2c_plan_set_task_dists, mm2c_frag_gaps_t, mm2c_frag_chain_batch_gaps and
mm2c_read_result_task_dists compile as C99 and C++11, mm2c_read_result_t keeps its 176 bytes (the pairs live behind priv), the ctypes mirrors agree, and the
refusals that need no device are made before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
typedef char size_is_176[sizeof(mm2c_read_result_t) == 176 ? 1 : -1];
typedef char gaps_is_16[sizeof(mm2c_frag_gaps_t) == 16 ? 1 : -1];
typedef char gap_at_4[offsetof(mm2c_frag_gaps_t, max_gap) == 4 && offsetof(mm2c_frag_gaps_t, max_gap_ref) == 8 && offsetof(mm2c_frag_gaps_t, max_frag_len) == 12 ? 1 : -1];
int (*f1)(mm2c_plan_t *, const int32_t *) = mm2c_plan_set_task_dists;
int (*f2)(const mm2c_params_t *, int, int, const mm2c_minidx_t *, int, int, const mm2c_frag_gaps_t *, int64_t, const int64_t *, int64_t, const int64_t *,
          const uint8_t *, const mm2c_seed_skip_host_t *, mm2c_read_result_t *) = mm2c_frag_chain_batch_gaps;
int (*f3)(const mm2c_read_result_t *, const int32_t **, int64_t *) = mm2c_read_result_task_dists;
int main(void) { mm2c_frag_gaps_t g; g.is_sr = 1; g.max_gap = 100; g.max_gap_ref = -1; g.max_frag_len = 800; return (int)(g.is_sr + g.max_gap + g.max_gap_ref + g.max_frag_len); }
'''


def test_entries_compile(tmp_path):
    src = tmp_path / "h.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_ctypes_mirrors():
    import mm2chain
    from mm2chain import _native as N
    assert C.sizeof(N.ReadResult) == 176
    assert [f[0] for f in N.FragGaps._fields_] == ["is_sr", "max_gap", "max_gap_ref", "max_frag_len"] and C.sizeof(N.FragGaps) == 16
    lib = N.load()
    for name in ("mm2c_plan_set_task_dists", "mm2c_frag_chain_batch_gaps", "mm2c_read_result_task_dists"):
        assert getattr(lib, name).argtypes is not None, name
    g = mm2chain.frag_gaps()
    assert (g.is_sr, g.max_gap, g.max_gap_ref, g.max_frag_len) == (1, 100, -1, 800)
    assert hasattr(mm2chain.ChainPlan, "set_task_dists") and callable(mm2chain.frag_chain_batch_gaps)


def test_refusals_come_before_any_device_work():
    """NULL gaps and max_gap < 0 are MM2C_E_ARG, and so is what mm2c_frag_chain_batch refuses (a malformed frag_off, a NULL index) -- with or without a device"""
    import mm2chain
    from mm2chain import _native as N, params
    lib = N.load()
    res = lib.mm2c_read_result_create()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    P = params.make_params(max_dist_x=500, max_dist_y=300, bw=100, n_segs=2)
    fo, so, seq = np.array([0, 2], np.int64), np.array([0, 50, 100], np.int64), np.zeros(100, np.uint8)
    fake_idx = C.c_void_p(8)                                                  # never dereferenced: the refusals below come first

    def call(gaps, idx=fake_idx, frag_off=fo):
        return lib.mm2c_frag_chain_batch_gaps(C.byref(P), 2, 25, idx, 8, 40, C.byref(gaps) if gaps is not None else None, frag_off.size - 1, ptr(frag_off),
                                              so.size - 1, ptr(so), ptr(seq), None, res)
    assert call(None) == -2 and b"gaps is NULL" in lib.mm2c_last_error()
    assert call(mm2chain.frag_gaps(max_gap=-1)) == -2 and b"max_gap" in lib.mm2c_last_error()
    assert call(mm2chain.frag_gaps(), idx=None) == -2 and b"index is NULL" in lib.mm2c_last_error()
    assert call(mm2chain.frag_gaps(), frag_off=np.array([0, 1], np.int64)) == -2          # does not end at n_reads
    assert call(mm2chain.frag_gaps(), frag_off=np.array([0, 1, 2], np.int64)) == -2 and b"n_segs" in lib.mm2c_last_error()
    d, n = C.c_void_p(1), C.c_int64(-1)
    assert lib.mm2c_read_result_task_dists(res, C.byref(d), C.byref(n)) == 0 and n.value == 0 and not d.value
    assert lib.mm2c_read_result_task_dists(None, C.byref(d), C.byref(n)) == -2
    assert lib.mm2c_plan_set_task_dists(None, None) == -2
    lib.mm2c_read_result_free(res)
