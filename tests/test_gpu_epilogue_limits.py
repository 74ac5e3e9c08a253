"""The device epilogue (csrc/chain_epilogue.hip) at the limits of its keys, sorts and LDS classes: the forests of tests/epilogue_limit_data.py
(tests/test_cpu_epilogue_limit_data.py asserts that each reaches its limit) through ChainPlan.chains in both forms of the epilogue and through the library's host
epilogue, u[] and b[] element for element against the oracle's backtrack; and three tasks whose score crosses 2^19 in the real DP through mm_chain_dp_batch."""
import numpy as np
import pytest
import torch

import epilogue_limit_data as ed
import oracle_binding as ob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(params=[1, 0], ids=["epi-lds", "epi-hbm"])
def epi_path(request):
    """the two forms of the device epilogue: tasks that fit the LDS in the fused kernel (default), or kernels A / B / C for every task"""
    import mm2chain
    with mm2chain.tuned(epi_fused=request.param):
        yield request.param


def _compare(cases, task, got, min_cnt, min_sc, what):
    """got[k] = (u, b) of task k; every case against the oracle under the given thresholds, every empty task empty"""
    used = set(task)
    for k, (u, b) in enumerate(got):
        if k not in used:
            assert u.size == 0 and b.shape[0] == 0, f"{what}: the empty task {k} has {u.size} chains"
    for c, k in zip(cases, task):
        u, b = got[k]
        u_ref, b_ref = ed.reference(c, min_cnt, min_sc)
        where = f"{what}, min_cnt={min_cnt} min_sc={min_sc}: {c['name']} (task {k}, n={c['facts']['n']})"
        assert u.size == u_ref.size, f"{where}: {u.size} chains, expected {u_ref.size}"
        bad = np.nonzero(u != u_ref)[0]
        assert bad.size == 0, f"{where}: {bad.size} of {u_ref.size} chains differ, first at {int(bad[0])}: {int(u[bad[0]]):#x} instead of {int(u_ref[bad[0]]):#x}"
        assert b.shape == b_ref.shape, f"{where}: {b.shape[0]} anchors in b, expected {b_ref.shape[0]}"
        bad = np.nonzero((b != b_ref).any(axis=1))[0]
        assert bad.size == 0, f"{where}: {bad.size} of {b_ref.shape[0]} anchors of b differ, first at {int(bad[0])}"


def _device(cases, empty_at, what):
    """one plan over the batch, ChainPlan.chains once per (min_cnt, min_sc) group of the cases: every case is compared under every group"""
    import mm2chain
    from mm2chain import params
    off, a, f, p, task = ed.batch(cases, empty_at)
    plan = mm2chain.ChainPlan(params.map_ont(), off)
    try:
        d_a = torch.from_numpy(a.view(np.int64)).cuda(); d_f = torch.from_numpy(f).cuda(); d_p = torch.from_numpy(p).cuda()
        for min_cnt, min_sc in ed.groups(cases):
            u_off, u, b_off, b = plan.chains(d_a, d_f, d_p, min_cnt, min_sc)
            torch.cuda.synchronize()
            u_off, b_off = u_off.cpu().numpy(), b_off.cpu().numpy()
            u, b = u.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64)
            got = [(u[u_off[k]:u_off[k + 1]], b[b_off[k]:b_off[k + 1]]) for k in range(off.size - 1)]
            _compare(cases, task, got, min_cnt, min_sc, what)
    finally:
        plan.close()


def test_all_limit_forests_in_one_batch(epi_path):
    """46 tasks (three of them empty), not in order of size: a scratch overrun of one task into its neighbour shows in the neighbour"""
    _device(ed.forest_cases(), ed.EMPTY_AT, "whole batch, " + ("fused" if epi_path else "kernels A / B / C"))


def test_all_limit_forests_through_the_host_epilogue():
    import mm2chain
    cases = ed.forest_cases()
    off, a, f, p, task = ed.batch(cases, ed.EMPTY_AT)
    for min_cnt, min_sc in ed.groups(cases):
        got = mm2chain.chain_epilogue_host(min_cnt, min_sc, off, a, f, p, n_threads=4)
        _compare(cases, task, got, min_cnt, min_sc, "host epilogue")


@pytest.mark.parametrize("pair", sorted(ed.PAIRS))
def test_boundary_pair_alone(pair, epi_path):
    """the cases on either side of one switch in a plan of their own: the plan's longest task decides which size classes are launched at all"""
    cases = [ed.by_name(n) for n in ed.PAIRS[pair]]
    _device(cases[::-1], (1,), f"{pair} alone, " + ("fused" if epi_path else "kernels A / B / C"))


@pytest.mark.parametrize("epilogue_threads", [0, 2])
def test_dp_scores_that_cross_2_to_the_19(epilogue_threads):
    """colinear chains of span 255 and 2 056 / 2 057 / 2 058 anchors: the DP itself hands the epilogue a peak score below, then above 2^19"""
    import mm2chain
    P, tasks = ed.dp_score_19()
    off = np.concatenate([[0], np.cumsum([t.shape[0] for t in tasks])]).astype(np.int64)
    res = mm2chain.mm_chain_dp_batch(P, 3, 40, off, np.concatenate(tasks), epilogue_threads=epilogue_threads)
    for k, t in enumerate(tasks):
        u_ref, b_ref = ob.mm_chain_dp(P, 3, 40, t)
        assert u_ref.size >= 1
        assert np.array_equal(res[k][0], u_ref), f"epilogue_threads={epilogue_threads}: task {k} ({t.shape[0]} anchors): u differs ({res[k][0].size} vs {u_ref.size} chains)"
        assert np.array_equal(res[k][1], b_ref), f"epilogue_threads={epilogue_threads}: task {k} ({t.shape[0]} anchors): b differs"
