"""CPU test of the fragment entries' side of include/mm2chain.h: the three entries, the statistics getter and the two result fields compile as C99 and C++11, the
result's earlier fields keep their offsets, the ctypes mirror agrees, and the refusals that need no device are made before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include "mm2chain.h"
#define AT(f, o) typedef char f##_at_##o[offsetof(mm2c_read_result_t, f) == o ? 1 : -1]
AT(n_reads, 0); AT(n_sketch, 8); AT(sketch_off, 16); AT(sketch, 24); AT(n_matches, 32); AT(match_off, 40); AT(matches, 48); AT(n_anchors, 56);
AT(anchor_off, 64); AT(rep_len, 72); AT(n_mini_pos, 80); AT(mini_off, 88); AT(mini_pos, 96); AT(n_u, 104); AT(n_b, 112); AT(u_off, 120); AT(u, 128);
AT(b_off, 136); AT(b, 144); AT(priv, 152); AT(n_rechained, 160); AT(rechained, 168);
typedef char size_is_176[sizeof(mm2c_read_result_t) == 176 ? 1 : -1];
int (*f1)(int, int, int, int64_t, const int64_t *, int64_t, const int64_t *, const uint8_t *, mm2c_read_result_t *) = mm2c_sketch_frag_batch;
int (*f2)(const mm2c_minidx_t *, int, int64_t, const int64_t *, int64_t, const int64_t *, const uint8_t *, mm2c_read_result_t *) = mm2c_sketch_match_frag_batch;
int (*f3)(const mm2c_params_t *, int, int, const mm2c_minidx_t *, int, int, int64_t, const int64_t *, int64_t, const int64_t *, const uint8_t *,
          const mm2c_seed_skip_host_t *, mm2c_read_result_t *) = mm2c_frag_chain_batch;
void (*f4)(mm2c_frag_stats_t *) = mm2c_get_frag_stats;
int main(void) { mm2c_read_result_t r; mm2c_frag_stats_t s; r.n_rechained = 0; r.rechained = (uint8_t *)0; s.rechain_ns = 0; return (int)(r.n_rechained + (int64_t)s.rechain_ns); }
'''


def test_fragment_entries_and_result_fields_compile(tmp_path):
    src = tmp_path / "h.c"
    src.write_text(SRC)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])


def test_ctypes_mirror_has_the_fields_behind_priv():
    from mm2chain import _native as N
    names = [f[0] for f in N.ReadResult._fields_]
    assert names[-3:] == ["priv", "n_rechained", "rechained"]
    assert N.ReadResult.priv.offset == 152 and N.ReadResult.n_rechained.offset == 160 and N.ReadResult.rechained.offset == 168 and C.sizeof(N.ReadResult) == 176
    assert [f[0] for f in N.FragStats._fields_] == ["calls", "fragments", "rechained", "rechain_ns"]


def test_fragment_refusals_come_before_any_device_work():
    """a malformed frag_off, an empty fragment, more than 255 segments: MM2C_E_ARG; a total length beyond 31 bits: MM2C_E_TOOBIG -- with or without a device"""
    from mm2chain import _native as N
    lib = N.load()
    res = lib.mm2c_read_result_create()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(frag_off, seq_off, seq=None):
        fo, so = np.asarray(frag_off, np.int64), np.asarray(seq_off, np.int64)
        s = np.zeros(max(int(so[-1]), 1), np.uint8) if seq is None else seq
        return lib.mm2c_sketch_frag_batch(15, 10, 0, fo.size - 1, ptr(fo), so.size - 1, ptr(so), ptr(s), res)
    assert call([0, 1, 1, 2], [0, 5, 9]) == -2 and b"no segment" in lib.mm2c_last_error()          # an empty fragment
    assert call([0, 1], [0, 5, 9]) == -2                                                             # does not end at n_reads
    assert call([1, 2], [0, 5, 9]) == -2                                                             # does not begin at 0
    assert call([0, 2, 1, 2], [0, 5, 9]) == -2                                                       # not monotone
    assert call([0, 256], np.arange(257)) == -2 and b"MM_MAX_SEG" in lib.mm2c_last_error()          # 256 segments
    big = np.array([0, 2**30 + 5, 2**31 + 10], np.int64)                                             # two legal segments, 2^31 + 10 bases together
    assert call([0, 2], big, seq=np.zeros(1, np.uint8)) == -3
    late = np.array([0, 2**30, 2**30 + 5], np.int64)                                                 # fits 31 bits, but `sum << 1` overflows the reference's int
    assert call([0, 2], late, seq=np.zeros(1, np.uint8)) == -3 and b"2^30" in lib.mm2c_last_error()
    lib.mm2c_read_result_free(res)


def _entries_with_seq_off_not_monotone():
    """every reads-in entry handed seq_off = [0, 5, 3]: (name, code, message) per entry.  The index is never read before the offsets are refused; a zeroed
    block stands in for it"""
    from mm2chain import _native as N
    from mm2chain import params
    lib = N.load()
    res = lib.mm2c_read_result_create()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    so, fo, seq = np.array([0, 5, 3], np.int64), np.array([0, 1, 2], np.int64), np.zeros(8, np.uint8)
    par, idx = params.map_ont(), C.cast(C.create_string_buffer(256), C.c_void_p)
    gaps = N.FragGaps(1, 100, -1, 800)
    calls = {
        "mm2c_sketch_batch": lambda: lib.mm2c_sketch_batch(15, 10, 0, 2, ptr(so), ptr(seq), res),
        "mm2c_sketch_match_batch": lambda: lib.mm2c_sketch_match_batch(idx, 50, 2, ptr(so), ptr(seq), res),
        "mm2c_read_chain_batch": lambda: lib.mm2c_read_chain_batch(C.byref(par), 3, 40, idx, 50, 2, ptr(so), ptr(seq), None, res),
        "mm2c_sketch_frag_batch": lambda: lib.mm2c_sketch_frag_batch(15, 10, 0, 2, ptr(fo), 2, ptr(so), ptr(seq), res),
        "mm2c_sketch_match_frag_batch": lambda: lib.mm2c_sketch_match_frag_batch(idx, 50, 2, ptr(fo), 2, ptr(so), ptr(seq), res),
        "mm2c_frag_chain_batch": lambda: lib.mm2c_frag_chain_batch(C.byref(par), 3, 40, idx, 50, 50, 2, ptr(fo), 2, ptr(so), ptr(seq), None, res),
        "mm2c_frag_chain_batch_gaps": lambda: lib.mm2c_frag_chain_batch_gaps(C.byref(par), 3, 40, idx, 50, 50, C.byref(gaps), 2, ptr(fo), 2, ptr(so), ptr(seq), None, res),
    }
    out = [(name, f(), lib.mm2c_last_error() or b"") for name, f in calls.items()]
    lib.mm2c_read_result_free(res)
    return out


def test_fragment_entries_refuse_malformed_seq_off_before_asking_for_a_device():
    """the fragment entries check every argument first: MM2C_E_ARG for seq_off that is not monotone, with or without a device"""
    for name, code, msg in _entries_with_seq_off_not_monotone():
        if "frag" in name:
            assert code == -2 and b"not monotone at read 1" in msg, (name, code, msg)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the order of refusals where the library cannot be initialised")
def test_read_entries_answer_not_initialised_before_any_argument_check():
    """the three read entries share the fragment entries' code path but keep their own order of refusals: without mm2c_init they answer MM2C_E_NODEVICE,
    malformed seq_off or not"""
    for name, code, msg in _entries_with_seq_off_not_monotone():
        if "frag" not in name:
            assert code == -1 and b"not monotone" not in msg, (name, code, msg)
