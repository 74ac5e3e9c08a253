"""GPU tests of reads in, chains out (mm2c_read_chain_batch): sketch, lookups, seed hits, DP and epilogue on the device give, read for read, what the
matches-in path (mm2c_seed_chain_batch_pool[_skip]) gives on the same reads' matches -- checked against the reference's (tests/golden/ref_sketch.npz)
-- and what the CPU oracle's
collect_seed_hits + mm_chain_dp give -- with and without skip_seed, with the heap order, over several chunks and with two device slots."""
import os

import numpy as np
import pytest
import torch

import oracle_binding as ob
import sketch_model as sm
from helpers import knobs  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sketch.npz")
MIN_CNT, MIN_SC = 3, 40


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


@pytest.fixture(autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def _setup(fx, name):
    import mm2chain
    k, w, hpc = (int(v) for v in fx[name + "_kwh"])
    pool = mm2chain.HitPool(fx[name + "_pool"])
    idx = mm2chain.MinimizerIndex(k, w, hpc, fx[name + "_keys"], fx[name + "_cr_off"], fx[name + "_n"], pool=pool)
    return pool, idx, int(fx[name + "_mid_occ"][0])


def _skip(fx, name, rng):
    """FOR_ONLY-free all-vs-all flags with made-up name ranks: both paths and the oracle see the same ones"""
    import mm2chain
    n_ref = int((fx[name + "_pool"] >> np.uint64(32)).max()) + 1
    n_reads = fx["seq_off"].size - 1
    rank = rng.permutation(n_ref).astype(np.int32)
    ref_len = rng.integers(1000, 20000, n_ref).astype(np.int32)
    q_lo = rng.integers(0, n_ref + 1, n_reads).astype(np.int32)
    q_eq = (rng.random(n_reads) < 0.5).astype(np.int32)
    return mm2chain.SeedSkip(ob.F_NO_DIAG | ob.F_NO_DUAL, rank, ref_len, q_lo, q_eq), (rank, ref_len, q_lo, q_eq)


def _compare(fx, name, P, skip=None, skip_arrays=None, heap=False, check_oracle=True):
    import mm2chain
    pool, idx, mid_occ = _setup(fx, name)
    off = fx["seq_off"]
    got = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, (off, fx["seq"]), idx, mid_occ, skip=skip)
    sm_ = mm2chain.sketch_match_batch((off, fx["seq"]), idx, mid_occ)        # the matches-in path's input: the reference's matches
    mo, m = sm_["match_off"], sm_["matches"]
    assert np.array_equal(mo, fx[name + "_match_off"])
    assert all(np.array_equal(sm.sha(m[mo[q]:mo[q + 1]]), fx[name + "_match_sha"][q]) for q in range(mo.size - 1))
    qlen = np.diff(off).astype(np.int32)
    if skip is None:
        ref_chains = mm2chain.seed_chain_batch_pool(P, MIN_CNT, MIN_SC, mo, m, pool, qlen)
        ref_ao = None
    else:
        ref_ao, ref_chains = mm2chain.seed_chain_batch_pool_skip(P, MIN_CNT, MIN_SC, mo, m, pool, qlen, skip)
        assert np.array_equal(got["anchor_off"], ref_ao)
    assert np.array_equal(got["rep_len"], fx[name + "_rep_len"])
    assert np.array_equal(got["mini_off"], mo)
    assert all(np.array_equal(sm.sha(got["mini_pos"][mo[q]:mo[q + 1]]), fx[name + "_mini_pos_sha"][q]) for q in range(mo.size - 1))
    hits = fx[name + "_pool"]
    n_chains = 0
    for r in range(off.size - 1):
        u, b = got["chains"][r]
        assert np.array_equal(u, ref_chains[r][0]) and np.array_equal(b, ref_chains[r][1]), f"read {r}: chains differ from the matches-in path"
        n_chains += u.size
        if check_oracle:
            kw = {}
            if skip_arrays is not None:
                rank, ref_len, q_lo, q_eq = skip_arrays
                kw = dict(flag=skip.flag, ref_rank=rank, ref_len=ref_len, q_lo=int(q_lo[r]), q_eq=int(q_eq[r]))
            a = ob.collect_seed_hits(m[mo[r]:mo[r + 1]], hits, int(qlen[r]), heap=heap, **kw)
            if skip is None:
                assert a.shape[0] == got["anchor_off"][r + 1] - got["anchor_off"][r]
            u_ref, b_ref = ob.mm_chain_dp(P, MIN_CNT, MIN_SC, a)
            assert np.array_equal(u, u_ref) and np.array_equal(b, b_ref), f"read {r}: chains differ from the oracle's mm_chain_dp"
    assert n_chains > 0
    idx.close(); pool.close()


def test_read_chain_map_ont(fx):
    from mm2chain import params
    _compare(fx, "map_ont", params.map_ont())


def test_read_chain_ava_ont_skip(fx):
    from mm2chain import params
    skip, arrays = _skip(fx, "ava_ont", np.random.default_rng(9))
    _compare(fx, "ava_ont", params.ava_ont(), skip=skip, skip_arrays=arrays)


def test_read_chain_heap_sort(fx, knobs):
    import mm2chain
    from mm2chain import params
    knobs("heap_sort", 1)
    _compare(fx, "map_ont", params.map_ont(), heap=True)
    skip, arrays = _skip(fx, "ava_ont", np.random.default_rng(10))
    _compare(fx, "ava_ont", params.ava_ont(), skip=skip, skip_arrays=arrays, heap=True)


def test_read_chain_several_chunks(fx, knobs):
    import mm2chain
    from mm2chain import params
    before = mm2chain.sketch_stats()
    knobs("read_chunk_bases", 20000)
    _compare(fx, "map_ont", params.map_ont(), check_oracle=False)
    skip, arrays = _skip(fx, "ava_ont", np.random.default_rng(11))
    _compare(fx, "ava_ont", params.ava_ont(), skip=skip, skip_arrays=arrays, check_oracle=False)
    after = mm2chain.sketch_stats()
    assert after["chunks"] - before["chunks"] >= 8
    assert after["sketch_ns"] > before["sketch_ns"] and after["lookup_ns"] > before["lookup_ns"]


def test_read_chain_two_device_slots(fx):
    import mm2chain
    from mm2chain import params
    mm2chain.shutdown()
    mm2chain.init_devices([0, 0])
    assert mm2chain.device_count() == 2
    _compare(fx, "map_ont", params.map_ont(), check_oracle=False)
