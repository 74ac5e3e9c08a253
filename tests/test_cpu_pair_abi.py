"""CPU tests of the pair plan's ABI (include/mm2chain.h, mm2chain/_native.py, mm2chain/batch.py): mm2c_pair_opt_t field by field through the built library, the two
new bit positions against the fixture's mm_reg1_t, the binding table, every argument refusal that needs no device -- before any device work, so it answers without
a GPU -- and params.pair_opts against options.c."""
import ctypes as C
import os

import numpy as np
import pytest

import mm2chain
from mm2chain import _native as N
from mm2chain import params, PEXT_DTYPE, REG_DTYPE

import pair_data as D
import pair_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
p = lambda a: a.ctypes.data_as(C.c_void_p)


def _pair(opt, f_off, n, regs=None, pext=None, max_log_arg=64, n_frags=None, gap=None):
    lib = N.load()
    fo = np.asarray(f_off, np.int64); nn = np.asarray(n, np.int32)
    nf = (fo.size - 1) // 2 if n_frags is None else n_frags
    rg = np.zeros(max(int(fo.max()), 1), REG_DTYPE) if regs is None else regs
    px = np.zeros(1, PEXT_DTYPE) if pext is None else pext
    q = np.full(max(2 * nf, 2), 150, np.int32); st = np.zeros(max(nf, 1), np.int32)
    return lib.mm2c_pair_ends_batch_host(nf, C.byref(opt) if opt is not None else None, max_log_arg, p(fo), p(rg), p(nn), px.size, p(px), p(q), None if gap is None else p(gap), p(st))


def test_opt_struct_through_the_library():
    """size and order by ctypes; the offsets of the three checked fields by what the library says it read there"""
    assert C.sizeof(N.PairOpt) == 24 and [f[0] for f in N.PairOpt._fields_] == list(M.OPT_FIELDS)
    assert [getattr(N.PairOpt, k).offset for k in M.OPT_FIELDS] == list(range(0, 24, 4))
    lib = N.load()
    for field, value, says in (("sub_diff", -5, b"sub_diff -5 < 0"), ("match_sc", -7, b"match_sc -7 < 1"), ("pe_ori", 9, b"pe_ori 9 outside 0..3")):
        o = N.PairOpt(101, 102, 103, 104, 1, 1)
        setattr(o, field, value)
        assert _pair(o, [0, 1, 2], [1, 1]) == -2 and says in lib.mm2c_last_error()
    assert N.MM2C_PAIR_LDS_REGIONS == D.LDS_CLASS == 128


def test_bits_against_the_fixture():
    """proper_frag and pe_thru where GCC puts them in the reference's mm_reg1_t: the fixture's regions are its own bytes"""
    assert (N.MM2C_REG_PROPER_FRAG_BIT, N.MM2C_REG_PE_THRU_BIT) == (13, 14) == (M.PROPER_FRAG_BIT, M.PE_THRU_BIT)
    Z = np.load(os.path.join(HERE, "golden", "ref_pair.npz"))
    assert int(Z["reg_size"]) == 80 == REG_DTYPE.itemsize
    names = list(Z["names"])
    cs = {c["name"]: c for c in D.cases()}

    def out(name):
        k = names.index(name)
        o = Z["out_off"]
        return [Z["regs_out"][o[2 * k + s]:o[2 * k + s + 1]].copy().view(REG_DTYPE).reshape(-1) for s in range(2)]
    # only pe_thru is set: one bit differs, on both regions
    for s, r in enumerate(out("no_pair_pe_thru")):
        assert int(r["flags"][0]) ^ int(cs["no_pair_pe_thru"]["regs"][s]["flags"][0]) == 1 << N.MM2C_REG_PE_THRU_BIT
    # a single candidate of two mapq-0 primaries: proper_frag and the floor 2, nothing else
    for s, r in enumerate(out("single_floor2")):
        assert int(r["flags"][0]) ^ int(cs["single_floor2"]["regs"][s]["flags"][0]) == (1 << N.MM2C_REG_PROPER_FRAG_BIT | 2)


def test_binding_table():
    lib = N.load()
    for name in ("mm2c_pairplan_create", "mm2c_pairplan_destroy", "mm2c_pairplan_run_device", "mm2c_pairplan_check", "mm2c_pairplan_last_ms", "mm2c_pair_ends_batch_host"):
        assert name in N.C_SYMBOLS and getattr(lib, name) is not None
    assert N.C_SYMBOLS["mm2c_pairplan_create"] == (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int32])
    assert N.C_SYMBOLS["mm2c_pairplan_run_device"] == (C.c_int, [C.c_void_p, C.POINTER(N.PairOpt)] + [C.c_void_p] * 8)
    assert len(N.C_SYMBOLS["mm2c_pair_ends_batch_host"][1]) == 11
    for name in ("PairPlan", "pair_ends_batch"):
        assert getattr(mm2chain, name) is not None and name in mm2chain.__all__


def test_refusals_before_any_device_work():
    """none of these needs mm2c_init: the argument checks come first (code -2)"""
    lib = N.load()
    ok = params.pair_opts()
    for bad in (dict(sub_diff=-1), dict(match_sc=0), dict(match_sc=-1), dict(pe_ori=-1), dict(pe_ori=4)):
        assert _pair(params.pair_opts(**bad), [0, 1, 2], [1, 1]) == -2
    assert _pair(None, [0, 1, 2], [1, 1]) == -2
    assert _pair(ok, [0, 2, 1], [1, 0]) == -2 and b"monotone" in lib.mm2c_last_error()
    assert _pair(ok, [0, 1, 2], [2, 1]) == -2 and b"in room for" in lib.mm2c_last_error()
    assert _pair(ok, [0, 1, 2], [1, -1]) == -2
    assert _pair(ok, [0, 1, 2], [1, 1], max_log_arg=-1) == -2 and _pair(ok, [0, 1, 2], [1, 1], max_log_arg=1 << 24) == -2
    assert _pair(ok, [0, 1, 2], [1, 1], n_frags=-1) == -2
    z = np.zeros(4, np.int64)
    assert lib.mm2c_pair_ends_batch_host(1, C.byref(ok), 16, None, None, None, 0, None, None, None, None) == -2
    assert lib.mm2c_pair_ends_batch_host(1, C.byref(ok), 16, p(np.array([0, 1, 2], np.int64)), None, p(np.ones(2, np.int32)), 0, None, p(z), None, p(z)) == -2   # regions NULL
    for args in ((-1, 0, 0, 16), (1, -1, 0, 16), (1, 1, -1, 16), (1, 1, 1, -1), (1, 1, 1, 1 << 24), (1 << 31, 1, 1, 16)):
        assert not lib.mm2c_pairplan_create(*args) and b"bad argument" in lib.mm2c_last_error()
    assert lib.mm2c_pairplan_run_device(None, C.byref(ok), None, None, None, None, None, None, None, None) == -2
    assert lib.mm2c_pairplan_check(None, None, None, None) == -2
    ms = C.c_float(0)
    assert lib.mm2c_pairplan_last_ms(None, C.byref(ms)) == -2
    with pytest.raises(ValueError):
        mm2chain.pair_ends_batch(ok, [0, 1], np.zeros(1, REG_DTYPE), [1], np.zeros(1, PEXT_DTYPE), [150])   # an even number of offsets
    with pytest.raises(ValueError):
        mm2chain.pair_ends_batch(ok, [0, 1, 2], np.zeros(1, REG_DTYPE), [1, 1], np.zeros(1, PEXT_DTYPE), [150, 150])   # offsets beyond the array


def test_pair_opts_against_options_c():
    d = lambda o: {k: getattr(o, k) for k in M.OPT_FIELDS}
    assert d(params.pair_opts()) == dict(max_gap_ref=500, pe_bonus=33, sub_diff=12, match_sc=2, pe_ori=1, flip=1)       # -x sr: a = 2, b = 8, FR
    assert {k: v for k, v in d(params.pair_opts()).items() if k != "flip"} == {k: v for k, v in D.DEFAULT.items() if k != "flip"}
    o = d(params.pair_opts("map-ont"))
    assert (o["sub_diff"], o["match_sc"], o["pe_ori"], o["pe_bonus"], o["max_gap_ref"]) == (8, 2, 0, 33, 500)
    assert d(params.pair_opts("asm20"))["sub_diff"] == 6 and d(params.pair_opts("asm20"))["match_sc"] == 1
    assert d(params.pair_opts(flip=0, pe_ori=3, max_gap_ref=77)) == dict(max_gap_ref=77, pe_bonus=33, sub_diff=12, match_sc=2, pe_ori=3, flip=0)
    with pytest.raises(TypeError):
        params.pair_opts(pe_thru=1)
