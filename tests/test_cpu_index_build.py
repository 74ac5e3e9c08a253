"""mm2c_minidx_build without a GPU: every argument error the header lists is refused with its code before any device work (the message of a NULL-returning
entry starts with the code's name), and a valid call without a device fails loudly -- there is no CPU path behind it."""
import ctypes as C

import numpy as np
import pytest
import torch


def _build(k, w, off, seq=b"ACGT", n_seqs=None, hpc=0):
    """the C entry itself: (handle, message)"""
    from mm2chain import _native as N
    lib = N.load()
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    buf = None if seq is None else np.frombuffer(seq, np.uint8)
    occ = C.c_int(-7)
    h = lib.mm2c_minidx_build(k, w, hpc, (off.size - 1) if n_seqs is None else n_seqs, None if off is None else off.ctypes.data_as(C.c_void_p),
                              None if buf is None else buf.ctypes.data_as(C.c_void_p), 2e-4, C.byref(occ))
    msg = (lib.mm2c_last_error() or b"").decode()
    if h:
        lib.mm2c_minidx_destroy(h)
    assert occ.value == -7 or h, "mid_occ is only written on success"
    return h, msg


@pytest.mark.parametrize("k,w", [(0, 10), (29, 10), (-1, 10), (15, 0), (15, 256), (15, -3)])
def test_k_and_w_limits_are_argument_errors(k, w):
    h, msg = _build(k, w, [0, 4])
    assert not h and msg.startswith("MM2C_E_ARG:"), msg


@pytest.mark.parametrize("off,what", [([1, 4], "seq_off[0]"), ([0, 4, 2], "monotone"), ([0, 2, 1, 4], "monotone"), ([0, -1], "monotone")])
def test_bad_offsets_are_argument_errors(off, what):
    h, msg = _build(15, 10, off)
    assert not h and msg.startswith("MM2C_E_ARG:") and what in msg, msg


def test_null_pointers_and_negative_counts_are_argument_errors():
    for kw in (dict(off=None, n_seqs=1), dict(off=[0, 4], seq=None), dict(off=[0, 4], n_seqs=-1)):
        h, msg = _build(15, 10, **kw)
        assert not h and msg.startswith("MM2C_E_ARG:"), (kw, msg)


def test_a_sequence_of_2_to_the_31_bases_is_too_big():
    """pos << 1 must fit 32 bits; only the offsets are read before the refusal"""
    for off in ([0, 1 << 31], [0, 5, 5 + (1 << 31), 6 + (1 << 31)], [0, 1 << 40]):
        h, msg = _build(15, 10, off)
        assert not h and msg.startswith("MM2C_E_TOOBIG:") and "2^31" in msg, msg
    h, msg = _build(15, 10, [0, (1 << 31) - 1])                              # the longest legal sequence passes the checks (and then finds no device here)
    assert not msg.startswith("MM2C_E_TOOBIG") and not msg.startswith("MM2C_E_ARG"), msg


def test_more_than_2_to_the_31_minus_1_sequences_is_too_big():
    """refused on the count alone, before the offsets are read"""
    h, msg = _build(15, 10, [0, 4], n_seqs=1 << 31)
    assert not h and msg.startswith("MM2C_E_TOOBIG:") and "sequences" in msg, msg


def test_python_build_raises_with_the_code():
    import mm2chain
    with pytest.raises(mm2chain.Mm2cError, match=r"code -2\).*MM2C_E_ARG"):
        mm2chain.MinimizerIndex.build([b"ACGT"], 29, 10)
    with pytest.raises(mm2chain.Mm2cError, match=r"code -2\).*MM2C_E_ARG"):
        mm2chain.MinimizerIndex.build([b"ACGT"], 15, 256)


def test_index_chunk_bases_is_a_tune_knob():
    import mm2chain
    mm2chain.tune("index_chunk_bases", 1 << 27)
    with pytest.raises(mm2chain.Mm2cError):
        mm2chain.tune("index_chunk_bases", 0)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_gpu_means_loud_failure_not_cpu_fallback():
    import mm2chain
    h, msg = _build(15, 10, [0, 4])
    assert not h and msg.startswith("MM2C_E_NODEVICE:"), msg
    with pytest.raises(mm2chain.Mm2cError, match=r"code -1\)"):
        mm2chain.MinimizerIndex.build([b"ACGTACGTACGTACGTACGTACGT"], 15, 10)
    with pytest.raises(mm2chain.Mm2cError, match=r"code -1\)"):
        mm2chain.MinimizerIndex.build([], 15, 10)                         # an empty list is legal, and needs the device all the same
