"""CPU test of the base-alignment section of include/mm2chain.h: the three structs' sizes and offsets, the section compiles as C99 and C++11 with the signatures
the interface gives, the ctypes mirror and the NumPy record types agree, the symbols are exported, the params helper makes mat as ksw_gen_simple_mat and the
presets' scalars, and the host entry and the plan make their refusals before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
typedef char score_is_29[sizeof(mm2c_ksw_score_t) == 29 && offsetof(mm2c_ksw_score_t, q) == 25 && offsetof(mm2c_ksw_score_t, e2) == 28 ? 1 : -1];
typedef char task_is_40[sizeof(mm2c_ksw_task_t) == 40 && offsetof(mm2c_ksw_task_t, t_off) == 8 && offsetof(mm2c_ksw_task_t, qlen) == 16 && offsetof(mm2c_ksw_task_t, flag) == 36 ? 1 : -1];
typedef char res_is_48[sizeof(mm2c_ksw_res_t) == 48 && offsetof(mm2c_ksw_res_t, zdropped) == 4 && offsetof(mm2c_ksw_res_t, n_cigar) == 36 && offsetof(mm2c_ksw_res_t, status) == 44 ? 1 : -1];
typedef char consts[MM2C_KSW_FLAGS == (0x01 | 0x02 | 0x08 | 0x10 | 0x40 | 0x80) && MM2C_KSW_MAX_LEN == 1048576 && MM2C_KSW_LDS_LEN == 2304 && MM2C_KSW_REFUSED == 1 &&
                    MM2C_KSW_TOO_BIG == 2 && MM2C_KSW_CIGAR_CUT == 3 && MM2C_KSW_MAX_SLOTS == 2048 && MM2C_KSW_SLOT_BYTES == 4194304 ? 1 : -1];
mm2c_kswplan_t *(*f1)(int64_t, int64_t, int64_t, int64_t) = mm2c_kswplan_create;
mm2c_kswplan_t *(*f1b)(int64_t, int64_t, int64_t, int64_t, int64_t) = mm2c_kswplan_create_slots;
void (*f2)(mm2c_kswplan_t *) = mm2c_kswplan_destroy;
int (*f3)(mm2c_kswplan_t *, const mm2c_ksw_score_t *, int64_t, const mm2c_ksw_task_t *, const uint8_t *, const int64_t *, mm2c_ksw_res_t *, uint32_t *, void *) = mm2c_kswplan_run_device;
int (*f4)(mm2c_kswplan_t *, int64_t *, int64_t *) = mm2c_kswplan_check;
int (*f5)(mm2c_kswplan_t *, float *) = mm2c_kswplan_last_ms;
int (*f6)(mm2c_kswplan_t *, float *) = mm2c_kswplan_last_kernel_ms;
int (*f7)(const mm2c_ksw_score_t *, int64_t, const mm2c_ksw_task_t *, int64_t, const uint8_t *, const int64_t *, mm2c_ksw_res_t *, uint32_t *, int64_t) = mm2c_ksw_extd2_batch_host;
int64_t (*f8)(const mm2c_kswplan_t *) = mm2c_kswplan_slot_bytes;
int64_t (*f9)(const mm2c_kswplan_t *) = mm2c_kswplan_n_slots;
int64_t (*f10)(int32_t, int32_t, int32_t, int32_t) = mm2c_ksw_task_scratch;
int main(void) { mm2c_ksw_task_t t; t.flag = 0; return t.flag; }
'''


def test_ksw_section_compiles(tmp_path):
    src = tmp_path / "m.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_mirror_symbols_and_params():
    import mm2chain
    from mm2chain import _native as N, params
    assert mm2chain.KSW_TASK_DTYPE.itemsize == 40 and mm2chain.KSW_TASK_DTYPE.fields["flag"][1] == 36 and mm2chain.KSW_TASK_DTYPE.fields["qlen"][1] == 16
    assert mm2chain.KSW_RES_DTYPE.itemsize == 48 and mm2chain.KSW_RES_DTYPE.fields["status"][1] == 44 and mm2chain.KSW_RES_DTYPE.fields["n_cigar"][1] == 36
    assert (mm2chain.KSW_REFUSED, mm2chain.KSW_TOO_BIG, mm2chain.KSW_CIGAR_CUT) == (1, 2, 3)
    lib = N.load()
    for name in ("mm2c_kswplan_create", "mm2c_kswplan_create_slots", "mm2c_kswplan_destroy", "mm2c_kswplan_slot_bytes", "mm2c_kswplan_n_slots", "mm2c_ksw_task_scratch", "mm2c_kswplan_run_device",
                 "mm2c_kswplan_check", "mm2c_kswplan_last_ms", "mm2c_kswplan_last_kernel_ms", "mm2c_ksw_extd2_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    assert N.C_SYMBOLS["mm2c_kswplan_run_device"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6)
    for name in ("KswPlan", "ksw_extd2_batch", "ksw_task_scratch", "KSW_TASK_DTYPE", "KSW_RES_DTYPE"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__
    # ksw_gen_simple_mat (align.c:9-22) and the scalars of options.c
    s = params.ksw_scores()
    assert s["mat"] == [2, -4, -4, -4, -1, -4, 2, -4, -4, -1, -4, -4, 2, -4, -1, -4, -4, -4, 2, -1, -1, -1, -1, -1, -1]
    assert (s["q"], s["e"], s["q2"], s["e2"], s["zdrop"], s["zdrop_inv"], s["end_bonus"], s["bw"]) == (4, 2, 24, 1, 400, 200, -1, 500)
    a5 = params.ksw_scores("asm5")
    assert (a5["mat"][0], a5["mat"][1], a5["q"], a5["e"], a5["q2"], a5["e2"], a5["zdrop"]) == (1, -19, 39, 3, 81, 1, 200)
    assert params.ksw_scores("sr")["end_bonus"] == 10 and params.ksw_scores("asm20", sc_ambi=0)["mat"][24] == 0 and params.ksw_scores(b=-6)["mat"][1] == -6
    import ksw_data
    for name, v in (("map-ont", "ont"), ("asm5", "asm5"), ("asm10", "asm10"), ("asm20", "asm20"), ("sr", "sr")):
        assert params.ksw_scores(name)["mat"] == list(ksw_data.score_set(v)[0])
    # what a task takes of a slot: p at the pitch of :94 plus off / off_end, the walk's CIGAR, and the image beyond the LDS classes
    assert lib.mm2c_ksw_task_scratch(0, 5, 10, 0) == 0 and lib.mm2c_ksw_task_scratch(100, 100, 10, 1) == 0
    rows, pitch = 199, ((11 + 15) // 16 + 1) * 16
    assert lib.mm2c_ksw_task_scratch(100, 100, 10, 0) == (rows * pitch + rows * 8 + (rows + 4) * 4 + 15) // 16 * 16
    assert lib.mm2c_ksw_task_scratch(100, 2305, 10, 1) == 12 * 2320 + 32 + 128 and lib.mm2c_ksw_task_scratch(100, 2304, 10, 1) == 0
    assert lib.mm2c_ksw_task_scratch(2305, 100, 10, 1) == 12 * 112 + 32 + 2336 and lib.mm2c_ksw_task_scratch(2304, 100, 10, 1) == 0


def test_host_entry_and_plan_refuse_before_any_device_work():
    """a NULL or impossible score set, negative counts, missing arrays, CIGAR offsets that do not start at 0 or run backwards, a flag outside MM2C_KSW_FLAGS, a length
    above MM2C_KSW_MAX_LEN, a task that leaves the sequences, a base code above 4: MM2C_E_ARG, with or without a device"""
    import mm2chain
    from mm2chain import _native as N, params
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    sc = mm2chain.batch._ksw_score_bytes(params.ksw_scores())
    seq = np.zeros(64, np.uint8)
    res, cig = np.zeros(2, mm2chain.KSW_RES_DTYPE), np.zeros(32, np.uint32)

    def run(tasks, co=(0, 16, 32), score=sc, s=seq, r=res, c=cig, n=None):
        tk = np.array(tasks, mm2chain.KSW_TASK_DTYPE)
        return lib.mm2c_ksw_extd2_batch_host(ptr(score), len(tk) if n is None else n, ptr(tk), s.size if s is not None else 8, ptr(s), ptr(np.asarray(co, np.int64)), ptr(r), ptr(c), 0)
    ok = [(0, 10, 10, 10, 5, 100, -1, 0), (20, 30, 10, 10, 5, 100, -1, 0x40)]
    assert run(ok, score=None) == -2 and b"score set is NULL" in lib.mm2c_last_error()
    bad_sc = sc.copy(); bad_sc[25] = 101
    assert run(ok, score=bad_sc) == -2 and b"127" in lib.mm2c_last_error()
    bad_sc = sc.copy(); bad_sc[26] = -1
    assert run(ok, score=bad_sc) == -2
    assert run(ok, n=-1) == -2 and run(ok, n=0) == 0
    assert run(ok, s=None) == -2 and b"NULL" in lib.mm2c_last_error()
    assert run(ok, r=None) == -2 and run(ok, c=None) == -2
    assert run(ok, co=(1, 16, 32)) == -2 and b"cig_off[0]" in lib.mm2c_last_error()
    assert run(ok, co=(0, 16, 8)) == -2 and b"not monotone at task 1" in lib.mm2c_last_error()
    for f in (0x04, 0x20, 0x100, 0x200, 0x400):
        assert run([ok[0], (20, 30, 10, 10, 5, 100, -1, f)]) == -2 and b"task 1: flag" in lib.mm2c_last_error()
    assert run([ok[0], (20, 30, (1 << 20) + 1, 10, 5, 100, -1, 0)]) == -2 and b"MM2C_KSW_MAX_LEN" in lib.mm2c_last_error()
    for t in ((-1, 30, 10, 10, 5, 100, -1, 0), (60, 30, 10, 10, 5, 100, -1, 0), (0, 55, 10, 10, 5, 100, -1, 0), (0, 1 << 40, 10, 10, 5, 100, -1, 0)):
        assert run([t, ok[1]]) == -2 and b"task 0 leaves the sequences" in lib.mm2c_last_error()
    s5 = seq.copy(); s5[33] = 5
    assert run(ok, s=s5) == -2 and b"task 1: target code 5 at 3" in lib.mm2c_last_error()
    s5 = seq.copy(); s5[9] = 200
    assert run(ok, s=s5) == -2 and b"task 0: query code 200 at 9" in lib.mm2c_last_error()
    # the plan's own refusals need no plan
    assert lib.mm2c_kswplan_run_device(None, ptr(sc), 0, *([None] * 6)) == -2 and lib.mm2c_kswplan_check(None, None, None) == -2
    ms = C.c_float(0)
    assert lib.mm2c_kswplan_last_ms(None, C.byref(ms)) == -2 and lib.mm2c_kswplan_last_kernel_ms(None, C.byref(ms)) == -2
    assert lib.mm2c_kswplan_slot_bytes(None) == 0 and lib.mm2c_kswplan_n_slots(None) == 0
    lib.mm2c_kswplan_destroy(None)
