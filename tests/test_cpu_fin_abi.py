"""CPU tests of the finish plan's ABI (include/mm2chain.h, mm2chain/_native.py, mm2chain/batch.py): record sizes and offsets against the dtypes, the binding table,
every argument refusal that needs no device -- before any device work, so it answers without a GPU -- and params.fin_opts against options.c."""
import ctypes as C

import numpy as np
import pytest

import mm2chain
from mm2chain import _native as N
from mm2chain import params, PEXT_DTYPE, REG_DTYPE

import fin_data as D
import fin_model as M


def test_records_and_dtypes():
    assert PEXT_DTYPE.itemsize == 32 == M.PEXT.itemsize and PEXT_DTYPE == M.PEXT
    assert [PEXT_DTYPE.fields[k][1] for k in ("dp_score", "dp_max", "dp_max2", "ambi_strand", "n_cigar", "reserved", "cig0")] == [0, 4, 8, 12, 16, 20, 24]
    assert C.sizeof(N.FinOpt) == 56 and [f[0] for f in N.FinOpt._fields_] == list(M.OPT_FIELDS)
    assert [getattr(N.FinOpt, k).offset for k in M.OPT_FIELDS] == list(range(0, 56, 4))
    assert REG_DTYPE.fields["p"][1] == 72 and M.CIG_REG == mm2chain.CIG_REG_DTYPE and M.EXTRA_RES == mm2chain.EXTRA_RES_DTYPE
    assert N.MM2C_FIN_LDS_REGIONS == D.LDS_CLASS == 128 and (mm2chain.FIN_REFUSED, mm2chain.FIN_INCOMPLETE, mm2chain.FIN_OVER_CAP) == (M.REFUSED, M.INCOMPLETE, M.OVER_CAP)


def test_binding_table():
    lib = N.load()
    for name in ("mm2c_finplan_create", "mm2c_finplan_destroy", "mm2c_finplan_apply_run_device", "mm2c_finplan_apply_check", "mm2c_finplan_run_device", "mm2c_finplan_check",
                 "mm2c_finplan_last_ms", "mm2c_apply_regions_batch_host", "mm2c_finish_regions_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    assert N.C_SYMBOLS["mm2c_finplan_create"] == (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32])
    assert N.C_SYMBOLS["mm2c_finplan_run_device"] == (C.c_int, [C.c_void_p, C.POINTER(N.FinOpt)] + [C.c_void_p] * 9)
    assert len(N.C_SYMBOLS["mm2c_finplan_apply_run_device"][1]) == 22 and len(N.C_SYMBOLS["mm2c_apply_regions_batch_host"][1]) == 18
    assert len(N.C_SYMBOLS["mm2c_finish_regions_batch_host"][1]) == 12
    for name in ("FinPlan", "apply_regions_batch", "finish_regions_batch", "PEXT_DTYPE"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__


def _finish(opt, f_off, n_in, regs=None, pext=None, max_log_arg=64, n_reads=None):
    lib = N.load()
    fo = np.asarray(f_off, np.int64); ni = np.asarray(n_in, np.int32)
    n = fo.size - 1 if n_reads is None else n_reads
    rg = np.zeros(max(int(fo.max()), 1), REG_DTYPE) if regs is None else regs
    px = np.zeros(1, PEXT_DTYPE) if pext is None else pext
    q = np.full(max(n, 1), 1000, np.int32); out = np.zeros_like(rg); no = np.zeros(max(n, 1), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return lib.mm2c_finish_regions_batch_host(n, C.byref(opt) if opt is not None else None, max_log_arg, p(fo), p(rg), p(ni), px.size, p(px), p(q), p(q), p(out), p(no))


def test_refusals_before_any_device_work():
    """none of these needs mm2c_init: the argument checks come first (code -2); a sound call without a device then answers -1"""
    lib = N.load()
    ok = params.fin_opts()
    for bad in (dict(min_dp_max=0), dict(match_sc=0), dict(match_sc=-1)):
        assert _finish(params.fin_opts(**bad), [0, 1], [1]) == -2
    assert _finish(None, [0, 1], [1]) == -2
    assert _finish(ok, [0, 2, 1], [1, 0]) == -2 and b"monotone" in lib.mm2c_last_error()
    assert _finish(ok, [0, 1], [2]) == -2 and b"in room for" in lib.mm2c_last_error()
    assert _finish(ok, [0, 1], [-1]) == -2
    assert _finish(ok, [0, 1], [1], max_log_arg=-1) == -2 and _finish(ok, [0, 1], [1], max_log_arg=1 << 24) == -2
    assert _finish(ok, [0, 1], [1], n_reads=-1) == -2
    for args in ((-1, 0, 0, 16, 2), (1, -1, 0, 16, 2), (1, 1, -1, 16, 2), (1, 1, 1, -1, 2), (1, 1, 1, 1 << 24, 2), (1, 1, 1, 16, 0), (1 << 31, 1, 1, 16, 2)):
        assert not lib.mm2c_finplan_create(*args) and b"bad argument" in lib.mm2c_last_error()
    assert lib.mm2c_finplan_run_device(None, C.byref(ok), None, None, None, None, None, None, None, None, None) == -2
    assert lib.mm2c_finplan_check(None, None, None, None) == -2 and lib.mm2c_finplan_apply_check(None, None, None, None) == -2
    ms = C.c_float(0)
    assert lib.mm2c_finplan_last_ms(None, C.byref(ms), C.byref(ms)) == -2
    # the apply entry: offsets that do not start at 0 or run backwards, an extra list that does not ascend
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    z = np.zeros(4, np.int64); regs = np.zeros(2, REG_DTYPE); cr = np.zeros(2, M.CIG_REG); px = np.zeros(2, PEXT_DTYPE); st = np.zeros(2, np.int32); nc = np.zeros(1, np.int64)
    xr = np.array([1, 0], np.int32); xe = np.zeros(2, M.EXTRA_RES)

    def apply(u_off, b_off=(0, 0), n_extra=0):
        uo, bo = np.asarray(u_off, np.int64), np.asarray(b_off, np.int64)
        return lib.mm2c_apply_regions_batch_host(uo.size - 1, p(uo), p(regs), p(bo), None, p(z), p(cr), n_extra, p(xr), p(xe), p(z), p(regs.copy()), p(px), p(st), 0, None, None, p(nc))
    assert apply([1, 2]) == -2 and b"start at 0" in lib.mm2c_last_error()
    assert apply([0, 2, 1], (0, 0, 0)) == -2 and apply([0, 2], (0, -1)) == -2
    assert apply([0, 2], n_extra=2) == -2 and b"ascend" in lib.mm2c_last_error()
    assert apply([0, 1], n_extra=2) == -2
    assert lib.mm2c_apply_regions_batch_host(1, p(z), p(regs), p(z), None, p(z), p(cr), 0, None, None, None, p(regs), p(px), p(st), 0, None, None, None) == -2


def test_fin_opts_against_options_c():
    d = lambda o: {k: getattr(o, k) for k in M.OPT_FIELDS}
    o = d(params.fin_opts())
    assert o == dict(min_cnt=3, min_chain_score=40, min_dp_max=80, max_clip_ratio=1.0, mask_level=0.5, mask_len=2 ** 31 - 1, hard_mask_level=0, sub_diff=8, pri_ratio=pytest.approx(0.8),
                     min_diff=30, best_n=5, match_sc=2, is_sr=0, all_chains=0)
    assert {k: v for k, v in o.items() if k != "pri_ratio"} == {k: v for k, v in D.DEFAULT.items() if k != "pri_ratio"}
    a = d(params.fin_opts("asm20"))
    assert (a["min_dp_max"], a["best_n"], a["sub_diff"], a["min_diff"], a["match_sc"]) == (200, 50, 6, 38, 1)
    assert d(params.fin_opts("asm5"))["sub_diff"] == 21 and d(params.fin_opts("asm10"))["sub_diff"] == 11
    s = d(params.fin_opts("sr"))
    assert (s["min_cnt"], s["min_chain_score"], s["min_dp_max"], s["best_n"], s["sub_diff"], s["min_diff"], s["is_sr"]) == (2, 25, 40, 20, 12, 42, 1) and s["pri_ratio"] == 0.5
    v = d(params.fin_opts("ava-ont"))
    assert v["all_chains"] == 1 and v["pri_ratio"] == 0.0 and v["min_chain_score"] == 100
    assert d(params.fin_opts("map-pb"))["min_diff"] == 38
    assert d(params.fin_opts(min_dp_max=7, hard_mask_level=5))["min_dp_max"] == 7 and d(params.fin_opts(hard_mask_level=5))["hard_mask_level"] == 1
    with pytest.raises(TypeError):
        params.fin_opts(alt_drop=0.15)
