"""CPU test of the CIGAR-join section of include/mm2chain.h: the two structs' sizes and offsets, the section compiles as C99 and C++11 with the signatures the
interface gives, the NumPy record types and the ctypes mirror agree with them, the symbols are exported, and the host entries and the plan make their argument
refusals before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
typedef char opt_is_24[sizeof(mm2c_cig_opt_t) == 24 && offsetof(mm2c_cig_opt_t, zdrop_inv) == 4 && offsetof(mm2c_cig_opt_t, bw_ext) == 8 && offsetof(mm2c_cig_opt_t, min_cnt) == 12 &&
                       offsetof(mm2c_cig_opt_t, flag) == 16 && offsetof(mm2c_cig_opt_t, cig_shift) == 20 ? 1 : -1];
typedef char reg_is_72[sizeof(mm2c_cig_reg_t) == 72 && offsetof(mm2c_cig_reg_t, n_used) == 4 && offsetof(mm2c_cig_reg_t, drop_item) == 12 && offsetof(mm2c_cig_reg_t, split_n) == 20 &&
                       offsetof(mm2c_cig_reg_t, has_p) == 28 && offsetof(mm2c_cig_reg_t, n_cigar) == 32 && offsetof(mm2c_cig_reg_t, dp_score) == 36 && offsetof(mm2c_cig_reg_t, rs1) == 40 &&
                       offsetof(mm2c_cig_reg_t, r_qs) == 56 && offsetof(mm2c_cig_reg_t, cig0) == 64 ? 1 : -1];
typedef char consts[MM2C_CIG_REFUSED == 1 && MM2C_CIG_INCOMPLETE == 2 && MM2C_CIG_OVER_CAP == 3 && MM2C_CIG_PIECE == 256 && MM2C_CIG_NO_ROOM == -2 && MM2C_CIG_LOST == -3 ? 1 : -1];
mm2c_cigplan_t *(*f1)(int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t) = mm2c_cigplan_create;
void (*f2)(mm2c_cigplan_t *) = mm2c_cigplan_destroy;
int (*f3)(mm2c_cigplan_t *, const mm2c_cig_opt_t *, const mm2c_ksw_score_t *, int64_t, const mm2c_aln_reg_t *, const mm2c_aln_item_t *, const mm2c_ksw_task_t *, const mm2c_zdrop_res_t *,
          const uint8_t *, mm2c_ksw_task_t *, int64_t *, int32_t *, void *) = mm2c_cigplan_second_run_device;
int (*f4)(mm2c_cigplan_t *, int64_t *, int64_t *, int64_t *) = mm2c_cigplan_second_check;
int (*f5)(mm2c_cigplan_t *, const mm2c_cig_opt_t *, int64_t, int64_t, const int64_t *, const mm2c_reg_t *, const int64_t *, const int64_t *, const void *, const int64_t *,
          const mm2c_aln_reg_t *, const mm2c_aln_item_t *, const int64_t *, const mm2c_ksw_res_t *, const uint32_t *, const mm2c_zdrop_res_t *, const int32_t *, const int64_t *,
          const mm2c_ksw_res_t *, const uint32_t *, mm2c_cig_reg_t *, uint32_t *, int64_t *, mm2c_extra_task_t *, int32_t *, void *) = mm2c_cigplan_run_device;
int (*f6)(mm2c_cigplan_t *, int64_t *, int64_t *, int64_t *, int64_t *) = mm2c_cigplan_check;
int (*f7)(mm2c_cigplan_t *, float *) = mm2c_cigplan_last_kernel_ms;
int (*f8)(const mm2c_cig_opt_t *, const mm2c_ksw_score_t *, int64_t, const mm2c_aln_reg_t *, int64_t, const mm2c_aln_item_t *, int64_t, const mm2c_ksw_task_t *, const mm2c_zdrop_res_t *,
          int64_t, const uint8_t *, int64_t, mm2c_ksw_task_t *, int64_t *, int32_t *, int64_t *) = mm2c_second_pass_batch_host;
int (*f9)(const mm2c_cig_opt_t *, int64_t, const int64_t *, const mm2c_reg_t *, const int64_t *, const mm2c_anchor_t *, const int64_t *, const mm2c_aln_reg_t *, int64_t,
          const mm2c_aln_item_t *, int64_t, const int64_t *, const mm2c_ksw_res_t *, const uint32_t *, const mm2c_zdrop_res_t *, const int32_t *, int64_t, const int64_t *,
          const mm2c_ksw_res_t *, const uint32_t *, mm2c_cig_reg_t *, int64_t, uint32_t *, int64_t, int64_t *, mm2c_extra_task_t *, int32_t *, int64_t *) = mm2c_assemble_regions_batch_host;
int main(void) { mm2c_cig_reg_t t; t.status = 0; return t.status; }
'''


def test_cig_section_compiles(tmp_path):
    src = tmp_path / "m.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_mirror_and_symbols():
    import mm2chain
    from mm2chain import _native as N
    import cig_model
    offs = lambda dt: [(n, dt.fields[n][1]) for n in dt.names]
    assert mm2chain.CIG_OPT_DTYPE.itemsize == 24 and offs(mm2chain.CIG_OPT_DTYPE) == offs(cig_model.CIG_OPT_DTYPE) and dict(offs(mm2chain.CIG_OPT_DTYPE))["cig_shift"] == 20
    assert mm2chain.CIG_REG_DTYPE.itemsize == 72 and offs(mm2chain.CIG_REG_DTYPE) == offs(cig_model.CIG_REG_DTYPE) and dict(offs(mm2chain.CIG_REG_DTYPE))["cig0"] == 64
    assert offs(mm2chain.KSW_RES_DTYPE) == offs(cig_model.KSW_RES_DTYPE) and offs(mm2chain.ZDROP_RES_DTYPE) == offs(cig_model.ZDROP_RES_DTYPE)
    assert offs(mm2chain.EXTRA_TASK_DTYPE) == offs(cig_model.EXTRA_TASK_DTYPE)
    assert (mm2chain.CIG_REFUSED, mm2chain.CIG_INCOMPLETE, mm2chain.CIG_OVER_CAP, mm2chain.CIG_PIECE, mm2chain.CIG_NO_ROOM, mm2chain.CIG_LOST) == (1, 2, 3, 256, -2, -3)
    assert (cig_model.REFUSED, cig_model.INCOMPLETE, cig_model.OVER_CAP, cig_model.NO_ROOM, cig_model.LOST) == (1, 2, 3, -2, -3)
    lib = N.load()
    for name in ("mm2c_cigplan_create", "mm2c_cigplan_destroy", "mm2c_cigplan_second_run_device", "mm2c_cigplan_second_check", "mm2c_cigplan_run_device", "mm2c_cigplan_check",
                 "mm2c_cigplan_last_kernel_ms", "mm2c_second_pass_batch_host", "mm2c_assemble_regions_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    for name in ("CigPlan", "second_pass_batch", "assemble_regions_batch", "CIG_OPT_DTYPE", "CIG_REG_DTYPE", "CIG_REFUSED", "CIG_INCOMPLETE", "CIG_OVER_CAP", "CIG_PIECE", "CIG_NO_ROOM"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__
    rec = mm2chain.batch._cig_opt_bytes(dict(zdrop=400, zdrop_inv=200, bw_ext=751, min_cnt=3, flag=1, cig_shift=2, a=2))
    assert rec.tobytes() == np.array([400, 200, 751, 3, 1, 2], np.int32).tobytes()


def test_host_entries_and_plan_refuse_before_any_device_work():
    """NULL options, a shift or counts out of range, splice, a NULL score set, offsets that do not start at 0 or run backwards, missing arrays, a base code above 4 under
    sr: MM2C_E_ARG, with or without a device"""
    import mm2chain
    from mm2chain import _native as N
    import cig_data as D
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    B = D.build([D.planted()["code1"]])
    opt = mm2chain.batch._cig_opt_bytes(B["opt"])
    sc = mm2chain.batch._ksw_score_bytes((B["mat"], 4, 2, 24, 1))
    tot = (C.c_int64 * 2)()
    n2 = len(B["tasks2"])
    t2, co2, so = np.zeros(max(n2, 1), mm2chain.KSW_TASK_DTYPE), np.zeros(n2 + 1, np.int64), np.zeros(len(B["items"]), np.int32)
    pool = np.zeros(64, np.uint8)

    def second(o=opt, s=sc, nr=1, ar=B["aregs"], ni=len(B["items"]), it=B["items"], nt=len(B["tasks"]), tk=B["tasks"], z=B["zres"], pl=64, p=pool, cap=n2, t2_=t2, co=co2, so_=so):
        return lib.mm2c_second_pass_batch_host(ptr(o), ptr(s), nr, ptr(ar), ni, ptr(it), nt, ptr(tk), ptr(z), pl, ptr(p), cap, ptr(t2_), ptr(co), ptr(so_), tot)
    assert second(o=None) == -2 and b"options are NULL" in lib.mm2c_last_error()
    for k, v in (("cig_shift", 31), ("cig_shift", -1), ("bw_ext", -1), ("min_cnt", -1)):
        bad = opt.copy(); bad[k] = v
        assert second(o=bad) == -2 and b"out of range" in lib.mm2c_last_error(), k
    bad = opt.copy(); bad["flag"] = 4
    assert second(o=bad) == -2 and b"splice" in lib.mm2c_last_error()
    assert second(s=None) == -2 and b"score set is NULL" in lib.mm2c_last_error()
    assert second(nr=-1) == -2 and second(ni=-1) == -2 and second(nt=-1) == -2 and second(pl=-1) == -2 and second(cap=-1) == -2 and second(co=None) == -2
    for k in ("ar", "it", "tk", "z", "t2_", "so_", "p"):
        assert second(**{k: None}) == -2 and b"NULL" in lib.mm2c_last_error(), k
    srf = opt.copy(); srf["flag"] = 1
    p5 = pool.copy(); p5[9] = 5
    assert second(o=srf, p=p5) == -2 and b"base code 5 at 9" in lib.mm2c_last_error()
    co2[0] = 77
    assert second(nr=0) == 0 and co2[0] == 0

    m = D.model(B)
    wc, xc = m["totals"][0], m["totals"][1]
    cr, og, io = np.zeros(1, mm2chain.CIG_REG_DTYPE), np.zeros(max(wc, 1), np.uint32), np.zeros(xc + 1, np.int64)
    xt, xr = np.zeros(max(xc, 1), mm2chain.EXTRA_TASK_DTYPE), np.zeros(max(xc, 1), np.int32)

    def join(o=opt, n_reads=1, uo=B["u_off"], rg=B["regs"], bo=B["b_off"], b=B["b"], ro=B["read_off"], ar=B["aregs"], ni=len(B["items"]), it=B["items"], nt=len(B["tasks"]),
             co=B["cig_off"], rs=B["res"], cg=B["cigar"], z=B["zres"], so_=B["second_of"], nt2=n2, c2=B["cig_off2"], r2=B["res2"], g2=B["cigar2"], cr_=cr, wc_=wc, og_=og, xc_=xc,
             io_=io, xt_=xt, xr_=xr):
        i64 = lambda v: None if v is None else np.ascontiguousarray(v, np.int64)
        keep = [i64(uo), i64(bo), i64(ro), i64(co), i64(c2)]
        return lib.mm2c_assemble_regions_batch_host(ptr(o), n_reads, ptr(keep[0]), ptr(rg), ptr(keep[1]), ptr(b), ptr(keep[2]), ptr(ar), ni, ptr(it), nt, ptr(keep[3]), ptr(rs), ptr(cg), ptr(z),
                                                    ptr(so_), nt2, ptr(keep[4]), ptr(r2), ptr(g2), ptr(cr_), wc_, ptr(og_), xc_, ptr(io_), ptr(xt_), ptr(xr_), tot)
    assert join(o=None) == -2 and b"options are NULL" in lib.mm2c_last_error()
    assert join(n_reads=-1) == -2 and join(ni=-1) == -2 and join(nt=-1) == -2 and join(nt2=-1) == -2 and join(wc_=-1) == -2 and join(xc_=-1) == -2 and join(io_=None) == -2
    assert join(uo=(1, 1)) == -2 and b"must be 0" in lib.mm2c_last_error()
    assert join(uo=(0, -1)) == -2 and b"not monotone at read 0" in lib.mm2c_last_error()
    assert join(bo=(0, -1)) == -2 and join(ro=(0, -1)) == -2
    c_bad = B["cig_off"].copy(); c_bad[1] = -1
    assert join(co=c_bad) == -2 and b"not monotone at task 0" in lib.mm2c_last_error()
    c_bad = B["cig_off"].copy(); c_bad[0] = 1
    assert join(co=c_bad) == -2 and b"cig_off[0] must be 0" in lib.mm2c_last_error()
    c_bad = B["cig_off2"].copy(); c_bad[0] = 1
    assert join(c2=c_bad) == -2 and b"cig_off2[0] must be 0" in lib.mm2c_last_error()
    for k in ("rg", "b", "ar", "it", "co", "rs", "cg", "z", "so_", "c2", "r2", "g2", "cr_", "og_", "xt_", "xr_"):
        assert join(**{k: None}) == -2 and b"NULL" in lib.mm2c_last_error(), k
    io[0] = 77
    assert join(n_reads=0) == 0 and io[0] == 0
    # the plan's own refusals need no plan
    assert lib.mm2c_cigplan_second_run_device(None, ptr(opt), ptr(sc), 0, *([None] * 9)) == -2 and lib.mm2c_cigplan_run_device(None, ptr(opt), 0, 0, *([None] * 22)) == -2
    assert lib.mm2c_cigplan_check(None, None, None, None, None) == -2 and lib.mm2c_cigplan_second_check(None, None, None, None) == -2
    ms = (C.c_float * 5)()
    assert lib.mm2c_cigplan_last_kernel_ms(None, ms) == -2
    lib.mm2c_cigplan_destroy(None)
