"""CPU tests of the skip_seed host entries' Python side (mm2chain.SeedSkip, seed_hits_batch_skip, seed_chain_batch_skip, seed_chain_batch_pool_skip): the argument checks
that run before the library is called, and the library's exports of the new C entries."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_read():
    import mm2chain
    m = np.zeros(2, mm2chain.MATCH_DTYPE)
    m["n"] = [2, 1]; m["cr_off"] = [0, 2]; m["q_pos"] = [40, 81]; m["q_span"] = 15
    hits = np.array([(1 << 32) | 20, 100, (2 << 32) | 41], np.uint64)
    return np.array([0, 2], np.int64), m, hits, np.array([1000], np.int32)


def test_seed_skip_refuses_inconsistent_descriptions():
    import mm2chain
    S = mm2chain.SeedSkip
    assert (S.NO_DIAG, S.NO_DUAL, S.FOR_ONLY, S.REV_ONLY) == (0x001, 0x002, 0x100000, 0x200000)
    S(S.NO_DIAG | S.NO_DUAL, [0, 1, 2], [10, 10, 10], [1], [1])
    S(S.FOR_ONLY)
    S(S.NO_DIAG | S.NO_DUAL)                                                   # no names: qname == NULL (map.c:125)
    S(S.REV_ONLY, [0, 1], [5, 5])                                              # ranks without the per-read arrays: no flag compares names
    with pytest.raises(ValueError, match="bits"):
        S(0x4)
    with pytest.raises(ValueError, match="ref_len"):
        S(S.NO_DUAL, [0, 1, 2], [10, 10], [1], [1])
    with pytest.raises(ValueError, match="ref_len without"):
        S(S.NO_DUAL, None, [10, 10])
    with pytest.raises(ValueError, match="q_lo and q_eq"):
        S(S.NO_DUAL, [0, 1], [10, 10], [1], None)
    with pytest.raises(ValueError, match="q_lo and q_eq"):
        S(S.NO_DUAL, [0, 1], [10, 10], [1, 2], [1])
    with pytest.raises(ValueError, match="need ref_len, q_lo and q_eq"):
        S(S.NO_DUAL, [0, 1], [10, 10])
    with pytest.raises(ValueError, match="need ref_len, q_lo and q_eq"):
        S(S.NO_DIAG, [0, 1], None, [0], [0])


def test_batch_wrappers_check_lengths_before_calling_the_library():
    import mm2chain
    from mm2chain import params
    mo, m, h, ql = _one_read()
    two_reads = mm2chain.SeedSkip(3, [0, 1, 2], [10, 10, 10], [1, 0], [1, 0])   # per-read arrays of another batch
    P = params.map_ont()
    with pytest.raises(ValueError, match="2 entries for 1 reads"):
        mm2chain.seed_hits_batch_skip(mo, m, h, ql, two_reads)
    with pytest.raises(ValueError, match="2 entries for 1 reads"):
        mm2chain.seed_chain_batch_skip(P, 3, 40, mo, m, h, ql, two_reads)
    with pytest.raises(ValueError, match="2 entries for 1 reads"):
        mm2chain.seed_chain_batch_pool_skip(P, 3, 40, mo, m, None, ql, two_reads)
    ok = mm2chain.SeedSkip(3, [0, 1, 2], [10, 10, 10], [1], [1])
    with pytest.raises(ValueError, match="offsets do not fit"):
        mm2chain.seed_hits_batch_skip(mo, m, h, np.array([1000, 1000], np.int32), ok)
    with pytest.raises(ValueError, match="offsets do not fit"):
        mm2chain.seed_chain_batch_skip(P, 3, 40, np.array([0, 5], np.int64), m, h, ql, ok)


def test_library_exports_the_skip_entries():
    from mm2chain import _native as N
    N.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    for name in ("mm2c_seed_hits_batch_host_skip", "mm2c_seed_chain_batch_host_skip", "mm2c_seed_chain_batch_pool_skip", "mm2c_seedplan_last_expand_mw"):
        assert name in N.C_SYMBOLS
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported"
    hdr = open(os.path.join(ROOT, "include", "mm2chain.h")).read()
    assert "mm2c_seed_skip_host_t" in hdr
    import ctypes as C
    assert C.sizeof(N.SeedSkipHost) == 40                                       # int32 flag, int32 n_ref, four pointers
