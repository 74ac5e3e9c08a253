"""CPU test of the extra-plan section of include/mm2chain.h: the four structs' sizes and offsets, the section compiles as C99 and C++11 with the signatures the
interface gives, the NumPy record types and the ctypes mirror agree with them, the symbols are exported, the params helper makes the z-drop options of the presets,
and the host entries and the plan make their refusals before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
typedef char task_is_32[sizeof(mm2c_extra_task_t) == 32 && offsetof(mm2c_extra_task_t, t_off) == 8 && offsetof(mm2c_extra_task_t, qlen) == 16 && offsetof(mm2c_extra_task_t, tlen) == 20 &&
                        offsetof(mm2c_extra_task_t, n_cigar) == 24 && offsetof(mm2c_extra_task_t, rev) == 28 ? 1 : -1];
typedef char res_is_32[sizeof(mm2c_extra_res_t) == 32 && offsetof(mm2c_extra_res_t, qshift) == 4 && offsetof(mm2c_extra_res_t, tshift) == 8 && offsetof(mm2c_extra_res_t, blen) == 12 &&
                       offsetof(mm2c_extra_res_t, mlen) == 16 && offsetof(mm2c_extra_res_t, n_ambi) == 20 && offsetof(mm2c_extra_res_t, dp_max) == 24 && offsetof(mm2c_extra_res_t, status) == 28 ? 1 : -1];
typedef char opt_is_16[sizeof(mm2c_zdrop_opt_t) == 16 && offsetof(mm2c_zdrop_opt_t, zdrop_inv) == 4 && offsetof(mm2c_zdrop_opt_t, max_gap) == 8 && offsetof(mm2c_zdrop_opt_t, no_inv) == 12 ? 1 : -1];
typedef char zres_is_32[sizeof(mm2c_zdrop_res_t) == 32 && offsetof(mm2c_zdrop_res_t, t0) == 4 && offsetof(mm2c_zdrop_res_t, t1) == 8 && offsetof(mm2c_zdrop_res_t, q0) == 12 &&
                        offsetof(mm2c_zdrop_res_t, q1) == 16 && offsetof(mm2c_zdrop_res_t, code) == 20 && offsetof(mm2c_zdrop_res_t, inv_cand) == 24 && offsetof(mm2c_zdrop_res_t, status) == 28 ? 1 : -1];
typedef char consts[MM2C_EXTRA_LDS_WORDS == 2048 && MM2C_EXTRA_RUN_LANE == 16 && MM2C_EXTRA_MAX_SLOTS == 4096 && MM2C_EXTRA_REFUSED == 1 && MM2C_EXTRA_TOO_BIG == 2 && MM2C_EXTRA_CIGAR_CUT == 3 ? 1 : -1];
mm2c_extraplan_t *(*f1)(int64_t, int64_t, int64_t, int64_t, int64_t, int64_t) = mm2c_extraplan_create;
void (*f2)(mm2c_extraplan_t *) = mm2c_extraplan_destroy;
int (*f3)(mm2c_extraplan_t *, const mm2c_ksw_score_t *, int, int64_t, const mm2c_extra_task_t *, const uint8_t *, const int64_t *, const uint32_t *, const int64_t *, mm2c_extra_res_t *, uint32_t *,
          void *) = mm2c_extraplan_run_device;
int (*f4)(mm2c_extraplan_t *, const mm2c_ksw_score_t *, const mm2c_zdrop_opt_t *, int64_t, const mm2c_ksw_task_t *, const uint8_t *, const int64_t *, const mm2c_ksw_res_t *, const uint32_t *,
          mm2c_zdrop_res_t *, void *) = mm2c_extraplan_zdrop_run_device;
int (*f5)(mm2c_extraplan_t *, int64_t *, int64_t *) = mm2c_extraplan_check;
int (*f6)(mm2c_extraplan_t *, float *) = mm2c_extraplan_last_ms;
int (*f7)(mm2c_extraplan_t *, float *, float *) = mm2c_extraplan_last_kernel_ms;
int (*f8)(const mm2c_ksw_score_t *, int, int64_t, const mm2c_extra_task_t *, int64_t, const uint8_t *, const int64_t *, int64_t, const uint32_t *, const int64_t *, mm2c_extra_res_t *,
          uint32_t *) = mm2c_update_extra_batch_host;
int (*f9)(const mm2c_ksw_score_t *, const mm2c_zdrop_opt_t *, int64_t, const mm2c_ksw_task_t *, int64_t, const uint8_t *, const int64_t *, const mm2c_ksw_res_t *, const uint32_t *,
          mm2c_zdrop_res_t *) = mm2c_test_zdrop_batch_host;
int main(void) { mm2c_extra_task_t t; t.rev = 0; return t.rev; }
'''


def test_extra_section_compiles(tmp_path):
    src = tmp_path / "m.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_mirror_symbols_and_params():
    import mm2chain
    from mm2chain import _native as N, params
    offs = lambda dt: [(n, dt.fields[n][1]) for n in dt.names]
    assert mm2chain.EXTRA_TASK_DTYPE.itemsize == 32 and offs(mm2chain.EXTRA_TASK_DTYPE) == [("q_off", 0), ("t_off", 8), ("qlen", 16), ("tlen", 20), ("n_cigar", 24), ("rev", 28)]
    assert mm2chain.EXTRA_RES_DTYPE.itemsize == 32 and offs(mm2chain.EXTRA_RES_DTYPE) == [("n_cigar", 0), ("qshift", 4), ("tshift", 8), ("blen", 12), ("mlen", 16), ("n_ambi", 20), ("dp_max", 24),
                                                                                        ("status", 28)]
    assert mm2chain.ZDROP_OPT_DTYPE.itemsize == 16 and offs(mm2chain.ZDROP_OPT_DTYPE) == [("zdrop", 0), ("zdrop_inv", 4), ("max_gap", 8), ("no_inv", 12)]
    assert mm2chain.ZDROP_RES_DTYPE.itemsize == 32 and offs(mm2chain.ZDROP_RES_DTYPE) == [("max_zdrop", 0), ("t0", 4), ("t1", 8), ("q0", 12), ("q1", 16), ("code", 20), ("inv_cand", 24), ("status", 28)]
    assert (mm2chain.EXTRA_REFUSED, mm2chain.EXTRA_TOO_BIG, mm2chain.EXTRA_CIGAR_CUT, mm2chain.EXTRA_LDS_WORDS) == (1, 2, 3, 2048)
    lib = N.load()
    names = ("mm2c_extraplan_create", "mm2c_extraplan_destroy", "mm2c_extraplan_run_device", "mm2c_extraplan_zdrop_run_device", "mm2c_extraplan_check", "mm2c_extraplan_last_ms",
             "mm2c_extraplan_last_kernel_ms", "mm2c_update_extra_batch_host", "mm2c_test_zdrop_batch_host")
    for name in names:
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    assert N.C_SYMBOLS["mm2c_extraplan_run_device"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 8)
    assert N.C_SYMBOLS["mm2c_extraplan_zdrop_run_device"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 7)
    assert N.C_SYMBOLS["mm2c_update_extra_batch_host"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4)
    for name in ("ExtraPlan", "update_extra_batch", "test_zdrop_batch", "EXTRA_TASK_DTYPE", "EXTRA_RES_DTYPE", "ZDROP_OPT_DTYPE", "ZDROP_RES_DTYPE"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__
    assert params.zdrop_opts() == dict(zdrop=400, zdrop_inv=200, max_gap=5000, no_inv=0)
    assert params.zdrop_opts("sr") == dict(zdrop=100, zdrop_inv=100, max_gap=100, no_inv=1) and params.zdrop_opts("asm5", no_inv=True)["no_inv"] == 1
    assert list(mm2chain.batch._zdrop_opt_bytes(params.zdrop_opts("asm20"))) == [200, 200, 5000, 0]
    import extra_data
    assert extra_data.LDS_WORDS == mm2chain.EXTRA_LDS_WORDS and list(extra_data.score_set("ont")[0]) == params.ksw_scores()["mat"]


def test_host_entries_and_plan_refuse_before_any_device_work():
    """a NULL score set or options, a negative gap cost, negative counts, missing arrays, output offsets that do not start at 0 or run backwards, a CIGAR that leaves the
    input words, input and output words that overlap, a base code above 4: MM2C_E_ARG, with or without a device"""
    import mm2chain
    from mm2chain import _native as N, params
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    sc = mm2chain.batch._ksw_score_bytes(params.ksw_scores())
    zo = mm2chain.batch._zdrop_opt_bytes(params.zdrop_opts())
    seq = np.zeros(64, np.uint8)
    cig = np.array([10 << 4, 10 << 4], np.uint32)
    res, out = np.zeros(2, mm2chain.EXTRA_RES_DTYPE), np.zeros(8, np.uint32)
    ok = [(0, 10, 10, 10, 1, 0), (20, 30, 10, 10, 1, 1)]

    def upd(tasks=ok, io=(0, 1), oo=(0, 4, 8), score=sc, s=seq, ci=cig, r=res, o=out, n=None, n_ci=None):
        tk = np.array(tasks, mm2chain.EXTRA_TASK_DTYPE)
        return lib.mm2c_update_extra_batch_host(ptr(score), 0, len(tk) if n is None else n, ptr(tk), s.size if s is not None else 8, ptr(s), ptr(np.asarray(io, np.int64)),
                                                (ci.size if ci is not None else 2) if n_ci is None else n_ci, ptr(ci), ptr(np.asarray(oo, np.int64)), ptr(r), ptr(o))
    assert upd(score=None) == -2 and b"score set is NULL" in lib.mm2c_last_error()
    for at in (25, 26):
        bad = sc.copy(); bad[at] = -1
        assert upd(score=bad) == -2 and b">= 0" in lib.mm2c_last_error()
    assert upd(n=-1) == -2 and upd(n=0) == 0 and upd(n_ci=-1) == -2
    assert upd(s=None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert upd(r=None) == -2 and upd(o=None) == -2 and upd(ci=None) == -2
    assert upd(oo=(1, 4, 8)) == -2 and b"out_off[0]" in lib.mm2c_last_error()
    assert upd(oo=(0, 4, 2)) == -2 and b"not monotone at region 1" in lib.mm2c_last_error()
    assert upd(io=(0, 2)) == -2 and b"region 1: its CIGAR leaves the input words" in lib.mm2c_last_error()
    assert upd(io=(-1, 1)) == -2 and upd(tasks=[ok[0], (20, 30, 10, 10, -1, 0)]) == -2
    both = np.zeros(16, np.uint32)
    assert upd(ci=both[:2], o=both[1:9]) == -2 and b"overlap" in lib.mm2c_last_error()
    s5 = seq.copy(); s5[33] = 5
    assert upd(s=s5) == -2 and b"base code 5 at 33" in lib.mm2c_last_error()
    # the z-drop host entry
    ktasks = np.array([(0, 10, 10, 10, 5, 100, -1, 0), (20, 30, 10, 10, 5, 100, -1, 0)], mm2chain.KSW_TASK_DTYPE)
    kres = np.zeros(2, mm2chain.KSW_RES_DTYPE); kres["n_cigar"] = 1
    zres = np.zeros(2, mm2chain.ZDROP_RES_DTYPE)

    def zd(score=sc, opt=zo, co=(0, 1, 2), s=seq, kr=kres, cg=cig, z=zres, n=2):
        return lib.mm2c_test_zdrop_batch_host(ptr(score), ptr(opt), n, ptr(ktasks), s.size if s is not None else 8, ptr(s), ptr(np.asarray(co, np.int64)), ptr(kr), ptr(cg), ptr(z))
    assert zd(score=None) == -2 and zd(opt=None) == -2 and b"options are NULL" in lib.mm2c_last_error()
    bad = sc.copy(); bad[26] = -2
    assert zd(score=bad) == -2
    assert zd(n=-1) == -2 and zd(n=0) == 0 and zd(s=None) == -2 and zd(kr=None) == -2 and zd(z=None) == -2 and zd(cg=None) == -2
    assert zd(co=(1, 1, 2)) == -2 and b"cig_off[0]" in lib.mm2c_last_error()
    assert zd(co=(0, 2, 1)) == -2 and b"not monotone at task 1" in lib.mm2c_last_error()
    assert zd(s=s5) == -2 and b"base code 5" in lib.mm2c_last_error()
    # the plan's own refusals need no plan
    assert lib.mm2c_extraplan_run_device(None, ptr(sc), 0, 0, *([None] * 8)) == -2 and lib.mm2c_extraplan_zdrop_run_device(None, ptr(sc), ptr(zo), 0, *([None] * 7)) == -2
    assert lib.mm2c_extraplan_check(None, None, None) == -2
    ms = C.c_float(0)
    assert lib.mm2c_extraplan_last_ms(None, C.byref(ms)) == -2 and lib.mm2c_extraplan_last_kernel_ms(None, C.byref(ms), C.byref(ms)) == -2
    lib.mm2c_extraplan_destroy(None)
