"""CPU test of the chains-to-regions side of include/mm2chain.h: mm2c_reg_t has the size and the field offsets of mm_reg1_t (minimap.h:85-100; written out as constants,
the reference header is not everywhere this runs), the section compiles as C99 and C++11, the ctypes mirror and the NumPy dtype agree with it, the symbols are exported,
mm2c_read_hash equals the reference's values without any device, and the host-buffer entry makes its refusals before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# offsetof(mm_reg1_t, .) of the reference, and sizeof(mm_reg1_t): the fixture records the latter (reg_size) from the reference's own build
OFFSETS = {"id": 0, "cnt": 4, "rid": 8, "score": 12, "qs": 16, "qe": 20, "rs": 24, "re": 28, "parent": 32, "subsc": 36, "as": 40, "mlen": 44, "blen": 48, "n_sub": 52,
           "score0": 56, "flags": 60, "hash": 64, "div": 68, "p": 72}
SIZE = 80

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
#define AT(f, o) typedef char f##_at_##o[offsetof(mm2c_reg_t, f) == o ? 1 : -1]
AT(id, 0); AT(cnt, 4); AT(rid, 8); AT(score, 12); AT(qs, 16); AT(qe, 20); AT(rs, 24); AT(re, 28); AT(parent, 32); AT(subsc, 36); AT(as, 40); AT(mlen, 44); AT(blen, 48);
AT(n_sub, 52); AT(score0, 56); AT(flags, 60); AT(hash, 64); AT(div, 68); AT(p, 72);
typedef char size_is_80[sizeof(mm2c_reg_t) == 80 ? 1 : -1];
typedef char rev_is_bit_10[MM2C_REG_REV_BIT == 10 ? 1 : -1];
mm2c_regplan_t *(*f1)(int64_t, int64_t, int64_t) = mm2c_regplan_create;
void (*f2)(mm2c_regplan_t *) = mm2c_regplan_destroy;
int (*f3)(mm2c_regplan_t *, const int64_t *, const uint64_t *, const int64_t *, const void *, const int32_t *, const uint32_t *, mm2c_reg_t *, void *) = mm2c_regplan_run_device;
int (*f4)(mm2c_regplan_t *, int64_t *) = mm2c_regplan_check;
int (*f5)(mm2c_regplan_t *, float *) = mm2c_regplan_last_ms;
int (*f6)(int64_t, const int64_t *, const uint64_t *, const int64_t *, const mm2c_anchor_t *, const int32_t *, const uint32_t *, mm2c_reg_t *) = mm2c_gen_regs_batch_host;
uint32_t (*f7)(const char *, int32_t, int32_t) = mm2c_read_hash;
int (*f8)(mm2c_regplan_t *, float *, float *) = mm2c_regplan_last_kernel_ms;
int main(void) { mm2c_reg_t r; r.flags = 1u << MM2C_REG_REV_BIT; r.p = 0; return (int)(r.flags >> 10) - 1 + (int)r.p; }
'''


def test_reg_layout_and_entries_compile(tmp_path):
    src = tmp_path / "h.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_the_reference_records_the_same_size():
    assert int(np.load(os.path.join(GOLDEN, "ref_regs.npz"))["reg_size"]) == SIZE


def test_ctypes_mirror_and_dtype_agree():
    import mm2chain
    from mm2chain import _native as N
    import regs_model
    assert C.sizeof(N.Reg) == SIZE and mm2chain.REG_DTYPE.itemsize == SIZE
    for name, off in OFFSETS.items():
        assert getattr(N.Reg, "as_" if name == "as" else name).offset == off, name
        assert mm2chain.REG_DTYPE.fields[name][1] == off, name
    assert [f[0].rstrip("_") for f in N.Reg._fields_] == list(OFFSETS) == list(mm2chain.REG_DTYPE.names)
    assert mm2chain.REG_DTYPE == regs_model.REG


def test_symbols_are_exported():
    from mm2chain import _native as N
    lib = N.load()
    for name in ("mm2c_regplan_create", "mm2c_regplan_destroy", "mm2c_regplan_run_device", "mm2c_regplan_check", "mm2c_regplan_last_ms", "mm2c_regplan_last_kernel_ms",
                 "mm2c_gen_regs_batch_host", "mm2c_read_hash"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None


def test_read_hash_equals_the_reference_without_a_device():
    import mm2chain
    import regs_data
    want = np.load(os.path.join(GOLDEN, "ref_regs.npz"))["hashes"]
    got = [mm2chain.read_hash(name, qlen_sum, seed) for name, qlen_sum, seed in regs_data.HASH_CASES]
    assert got == [int(h) for h in want]
    assert mm2chain.read_hash("read1", 1000) == mm2chain.read_hash(b"read1", 1000, 11) and mm2chain.read_hash(None, 250) == int(want[-1])


def test_host_entry_refuses_before_any_device_work():
    """non-monotone offsets, cnt <= 0, a count sum that differs from the extent of b: MM2C_E_ARG, with or without a device"""
    from mm2chain import _native as N
    lib = N.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    b = np.zeros((16, 2), np.uint64)
    qlen, hash_, regs = np.full(2, 1000, np.int32), np.zeros(2, np.uint32), np.zeros(8 * 80, np.uint8)

    def call(u_off, u, b_off):
        uo, bo, uu = np.asarray(u_off, np.int64), np.asarray(b_off, np.int64), np.asarray(u, np.uint64)
        return lib.mm2c_gen_regs_batch_host(uo.size - 1, ptr(uo), ptr(uu), ptr(bo), ptr(b), ptr(qlen), ptr(hash_), ptr(regs))
    sc = 50 << 32
    assert call([0, 2, 1], [sc | 3, sc | 4], [0, 7, 7]) == -2 and b"chain offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([0, 1, 2], [sc | 3, sc | 4], [0, 7, 3]) == -2 and b"anchor offsets not monotone at read 1" in lib.mm2c_last_error()
    assert call([0, 1, 2], [sc | 3, sc | 0], [0, 3, 3]) == -2 and b"cnt 0" in lib.mm2c_last_error()
    assert call([0, 1, 2], [sc | 3, sc | 0xffffffff], [0, 3, 3]) == -2 and b"cnt -1" in lib.mm2c_last_error()
    assert call([0, 1, 2], [sc | 3, sc | 4], [0, 3, 8]) == -2 and b"count 4 anchors" in lib.mm2c_last_error()
    assert call([0, 1, 2], [sc | 3, sc | 4], [0, 4, 8]) == -2 and b"read 0" in lib.mm2c_last_error()
    assert call([0, 0, 0], [], [0, 0, 2]) == -2                                # anchors without a chain
    assert lib.mm2c_gen_regs_batch_host(-1, None, None, None, None, None, None, None) == -2
