"""CPU test of the chain-anchor divergence side of include/mm2chain.h: mm2c_err_t's size and offsets, the section compiles as C99 and C++11 with the signatures the
interface gives, the ctypes mirror agrees, the symbols are exported, mm2c_est_err_div equals the model (the host's pow) over the fixture's triples and at its
edges, mm2c_est_err_apply_host writes div and leaves a read without mini_pos alone, and the host-buffer entry and the plan make their refusals before any device
work."""
import ctypes as C
import os
import subprocess

import numpy as np

import esterr_data as D
import esterr_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
typedef char n_match_at_0[offsetof(mm2c_err_t, n_match) == 0 ? 1 : -1];
typedef char n_tot_at_4[offsetof(mm2c_err_t, n_tot) == 4 ? 1 : -1];
typedef char size_is_8[sizeof(mm2c_err_t) == 8 ? 1 : -1];
typedef char div_at_68[offsetof(mm2c_reg_t, div) == 68 ? 1 : -1];
mm2c_errplan_t *(*f1)(int64_t, int64_t, int64_t, int64_t) = mm2c_errplan_create;
void (*f2)(mm2c_errplan_t *) = mm2c_errplan_destroy;
int (*f3)(mm2c_errplan_t *, const int64_t *, const mm2c_reg_t *, const int32_t *, const int64_t *, const void *, const int64_t *, const uint64_t *, const int32_t *,
          int32_t, const uint32_t *, mm2c_err_t *, float *, void *) = mm2c_errplan_run_device;
int (*f4)(mm2c_errplan_t *, int64_t *) = mm2c_errplan_check;
int (*f5)(mm2c_errplan_t *, float *) = mm2c_errplan_last_ms;
int (*f6)(mm2c_errplan_t *, float *, float *, float *) = mm2c_errplan_last_kernel_ms;
float (*f7)(int32_t, int32_t, float) = mm2c_est_err_div;
int (*f8)(int64_t, const int64_t *, const int32_t *, const mm2c_err_t *, const float *, mm2c_reg_t *) = mm2c_est_err_apply_host;
int (*f9)(int64_t, const int64_t *, mm2c_reg_t *, const int32_t *, const int64_t *, const mm2c_anchor_t *, const int64_t *, const uint64_t *, const int32_t *, int32_t,
          const uint32_t *, mm2c_err_t *, float *) = mm2c_est_err_batch_host;
int main(void) { mm2c_err_t e; e.n_match = 3; return e.n_match - 3; }
'''


def test_esterr_section_compiles(tmp_path):
    src = tmp_path / "m.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_ctypes_mirror():
    import mm2chain
    from mm2chain import _native as N
    assert C.sizeof(N.Err) == 8 and [(f, getattr(N.Err, f).offset) for f, _ in N.Err._fields_] == [("n_match", 0), ("n_tot", 4)]
    assert mm2chain.ERR_DTYPE.itemsize == 8 and mm2chain.ERR_DTYPE.fields["n_tot"][1] == 4 and mm2chain.REG_DTYPE.fields["div"][1] == 68
    assert N.C_SYMBOLS["mm2c_errplan_create"] == (C.c_void_p, [C.c_int64] * 4)
    assert N.C_SYMBOLS["mm2c_errplan_run_device"] == (C.c_int, [C.c_void_p] * 9 + [C.c_int32] + [C.c_void_p] * 4)
    assert N.C_SYMBOLS["mm2c_errplan_check"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)])
    assert N.C_SYMBOLS["mm2c_errplan_last_kernel_ms"] == (C.c_int, [C.c_void_p] + [C.POINTER(C.c_float)] * 3)
    assert N.C_SYMBOLS["mm2c_est_err_div"] == (C.c_float, [C.c_int32, C.c_int32, C.c_float])
    assert N.C_SYMBOLS["mm2c_est_err_batch_host"] == (C.c_int, [C.c_int64] + [C.c_void_p] * 8 + [C.c_int32] + [C.c_void_p] * 3)


def test_symbols_are_exported():
    import mm2chain
    from mm2chain import _native as N
    lib = N.load()
    for name in ("mm2c_errplan_create", "mm2c_errplan_destroy", "mm2c_errplan_run_device", "mm2c_errplan_check", "mm2c_errplan_last_ms", "mm2c_errplan_last_kernel_ms",
                 "mm2c_est_err_div", "mm2c_est_err_apply_host", "mm2c_est_err_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    for name in ("EstErrPlan", "est_err_batch", "est_err_div", "est_err_apply"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__


def test_div_equals_the_model_over_the_fixtures_triples_and_at_its_edges():
    import mm2chain
    seen = set()
    for R in D.reference():
        c = R["case"]
        cnts, avg_k = M.counts(R["in"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"])
        for (nm, nt), want in zip(cnts.tolist(), R["out"]["div"]):
            if nm == -1:
                continue
            got = mm2chain.est_err_div(nm, nt, avg_k)
            assert got.tobytes() == M.div(nm, nt, avg_k).tobytes(), (R["name"], nm, nt, avg_k)
            libm = " (a libm-sensitive case: this machine's libm may not be the fixture's, " + R["libm"] + ")" if R["name"].startswith(("libm_", "avgk_frac_")) else ""
            assert got.tobytes() == np.float32(want).tobytes(), f"{R['name']}: div({nm}, {nt}, {avg_k}) = {got}, the reference {want}" + libm
            seen.add((nm, nt, float(avg_k)))
    assert len(seen) > 40
    f = mm2chain.est_err_div
    assert f(0, 0, 15.0) == -1.0 and f(0, 7, 15.0) == -1.0 and f(5, 5, 15.0) == 0.0 and f(6, 5, 15.0) == 0.0 and f(1, 1, 15.5) == 0.0
    assert 0.0 < f(4999, 5000, 15.0) < 2e-5 and f(1, 2, 15.0).tobytes() == M.div(1, 2, np.float32(15)).tobytes()
    rng = np.random.default_rng(5)
    for _ in range(2000):                                                       # n_tot large, few mismatches: where the result is most sensitive
        nt = int(rng.integers(2, 200000)); nm = nt - int(rng.integers(1, 4)); k = np.float32(rng.integers(10, 29)) + np.float32(rng.integers(0, 64)) / np.float32(64)
        if nm >= 1:
            assert f(nm, nt, k).tobytes() == M.div(nm, nt, k).tobytes(), (nm, nt, k)


def test_apply_host_writes_div_and_leaves_a_read_without_mini_pos_alone():
    import mm2chain
    rs = [R for R in D.reference() if R["name"] in ("both_strands", "no_mini", "first_absent", "two_rids", "no_regions", "all_matched_no_flanks")]
    room = [R["in"].size + 1 for R in rs]                                       # one row of filler behind every read
    u_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    regs = np.full((int(u_off[-1]), 80), 0xee, np.uint8)
    err = np.full((int(u_off[-1]), 2), 77, np.int32)
    avg = np.zeros(len(rs), np.float32)
    for k, R in enumerate(rs):
        c = R["case"]
        regs[u_off[k]:u_off[k] + R["in"].size] = R["in"].view(np.uint8).reshape(-1, 80)
        err[u_off[k]:u_off[k] + R["in"].size], avg[k] = M.counts(R["in"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"])
    sentinel = np.float32(0.125)
    no_mini = [k for k, R in enumerate(rs) if R["name"] == "no_mini"][0]
    regs[u_off[no_mini]:u_off[no_mini] + 1].reshape(-1).view(M.REG)["div"] = sentinel
    before = regs.copy()
    mm2chain.est_err_apply(u_off[:-1], [R["in"].size for R in rs], err, avg, regs)
    for k, R in enumerate(rs):
        g = regs[u_off[k]:u_off[k] + R["in"].size].reshape(-1).view(M.REG)
        if k == no_mini:
            assert g["div"][0] == sentinel and g.tobytes() == before[u_off[k]:u_off[k] + 1].tobytes()
        else:
            assert g.tobytes() == R["out"].tobytes(), R["name"]
        assert (regs[u_off[k] + R["in"].size] == 0xee).all(), "a row behind n_in was written"
    from mm2chain import _native as N
    lib = N.load()
    assert lib.mm2c_est_err_apply_host(-1, None, None, None, None, None) == -2 and lib.mm2c_est_err_apply_host(0, None, None, None, None, None) == 0
    assert lib.mm2c_est_err_apply_host(1, None, None, None, None, None) == -2 and b"NULL" in lib.mm2c_last_error()


def test_host_entry_and_plan_refuse_before_any_device_work():
    """offsets that are not monotone, n_in beyond its room, missing arrays, a negative n_ref: MM2C_E_ARG, with or without a device"""
    from mm2chain import _native as N
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    regs, b, mp = np.zeros(8 * 80, np.uint8), np.zeros((16, 2), np.uint64), np.zeros(16, np.uint64)
    q, rl = np.full(4, 1000, np.int32), np.full(2, 5000, np.uint32)

    def call(u_off, n_in, b_off, m_off, r=regs, n_ref=2, ref=rl):
        return lib.mm2c_est_err_batch_host(len(u_off) - 1, ptr(np.asarray(u_off, np.int64)), ptr(r), ptr(np.asarray(n_in, np.int32)), ptr(np.asarray(b_off, np.int64)), ptr(b),
                                           ptr(np.asarray(m_off, np.int64)), ptr(mp), ptr(q), n_ref, ptr(ref), None, None)
    assert call([0, 5, 3], [1, 1], [0, 4, 8], [0, 4, 8]) == -2 and b"region offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([0, 3, 5], [1, 1], [0, 9, 8], [0, 4, 8]) == -2 and b"anchor offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([0, 3, 5], [1, 1], [0, 4, 8], [0, 9, 8]) == -2 and b"mini_pos offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([0, 3, 5], [1, 3], [0, 4, 8], [0, 4, 8]) == -2 and b"read 1: 3 regions in room for 2" in lib.mm2c_last_error()
    assert call([0, 3, 5], [-1, 1], [0, 4, 8], [0, 4, 8]) == -2 and b"read 0" in lib.mm2c_last_error()
    assert call([0, 3], [1], [0, 4], [0, 4], r=None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert call([0, 3], [1], [0, 4], [0, 4], ref=None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert call([0, 3], [1], [0, 4], [0, 4], n_ref=-1) == -2
    assert lib.mm2c_est_err_batch_host(-1, *([None] * 8), 0, None, None, None) == -2
    assert lib.mm2c_est_err_batch_host(0, *([None] * 8), 0, None, None, None) == 0
    # the plan's own refusals need no plan
    assert lib.mm2c_errplan_run_device(None, *([None] * 8), 0, *([None] * 4)) == -2 and lib.mm2c_errplan_check(None, None) == -2
    ms = C.c_float(0)
    assert lib.mm2c_errplan_last_ms(None, C.byref(ms)) == -2 and lib.mm2c_errplan_last_kernel_ms(None, C.byref(ms), C.byref(ms), C.byref(ms)) == -2
    lib.mm2c_errplan_destroy(None)
