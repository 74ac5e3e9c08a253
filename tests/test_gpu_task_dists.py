"""Plans with per-task chaining distances (mm2c_plan_set_task_dists): every task chains with its own (max_dist_x, max_dist_y) in the window-start prepass, in the
device-side cut and in the filters of the DP.  All expected f / p come from the CPU oracle run task by task with that task's scalars; compared element for element,
for single-segment tasks and for tasks of two segments."""
import numpy as np
import pytest
import torch

import oracle_binding as ob
from helpers import assert_same, fold_driver_tasks
from reuse_data import batch

pytestmark = pytest.mark.gpu
INT32_MAX = 2**31 - 1
BW = 100


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def _params(n_segs, x=500, y=300, **kw):
    from mm2chain import params
    return params.make_params(max_dist_x=int(x), max_dist_y=int(y), bw=kw.pop("bw", BW), n_segs=n_segs, **kw)


def _with(P, x, y):
    from mm2chain import params
    return params.make_params(max_dist_x=int(x), max_dist_y=int(y), bw=P.bw, max_skip=P.max_skip, max_iter=P.max_iter, gap_scale=P.gap_scale, is_cdna=P.is_cdna,
                              n_segs=P.n_segs)


def _task(rng, n, step_hi, n_segs, jump=0.1):
    """n anchors on one reference: x steps of 0 .. step_hi, q following x with jumps; with n_segs = 2 every anchor is given a segment at random (the second
    segment's q shifted, as collect_minimizers does)"""
    step = rng.integers(0, step_hi + 1, n)
    pos = 1000 + np.cumsum(step)
    q = 50 + np.cumsum(np.where(rng.random(n) < jump, rng.integers(-60, 200, n), np.minimum(step, 400)))
    seg = rng.integers(0, n_segs, n)
    q = np.maximum(q, 1) + seg * 20000
    span = np.where(rng.random(n) < 0.7, 15, rng.integers(8, 40, n))
    x = (np.uint64(1) << np.uint64(32)) | pos.astype(np.uint64)
    y = (seg.astype(np.uint64) << np.uint64(48)) | (span.astype(np.uint64) << np.uint64(32)) | q.astype(np.uint64)
    o = np.argsort(x, kind="stable")
    return np.stack((x[o], y[o]), 1)


def _oracle(P, tasks, dists):
    f, p = [], []
    for t, (x, y) in zip(tasks, dists):
        ft, pt, _ = ob.chain_fpv(_with(P, x, y), t)
        f.append(ft); p.append(pt)
    return np.concatenate(f), np.concatenate(p)


def _run(plan, d_a, total):
    d_f = torch.full((total,), -77, dtype=torch.int32, device="cuda")
    d_p = torch.full((total,), -77, dtype=torch.int32, device="cuda")
    plan.run(d_a, d_f, d_p)
    torch.cuda.synchronize()
    return d_f.cpu().numpy(), d_p.cpu().numpy()


def _gpu(P, tasks, dists):
    """f, p, variant, route of a plan over `tasks` with the per-task distances `dists` (None: the plan's own scalars)"""
    import mm2chain
    a, off = batch(tasks)
    d_a = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 2)).cuda()
    plan = mm2chain.ChainPlan(P, off)
    if dists is not None:
        plan.set_task_dists(torch.from_numpy(np.ascontiguousarray(dists, dtype=np.int32)).cuda())
    f, p = _run(plan, d_a, a.shape[0])
    v, route = plan.last_variant(), plan.last_route()
    plan.close()
    return f, p, v, route, off


@pytest.mark.parametrize("n_segs", [1, 2])
def test_random_pairs_and_edge_values(n_segs):
    rng = np.random.default_rng(11 + n_segs)
    edge = [0, 1, BW, 65535, 65536, INT32_MAX]
    tasks, dists = [], []
    for k in range(200):
        n = int(rng.integers(1, 601)) if k % 10 else (1, 2, 63, 64, 65, 600)[k // 10 % 6]
        x = edge[int(rng.integers(0, 6))] if rng.random() < 0.3 else int(rng.integers(2, 3000))
        y = edge[int(rng.integers(0, 6))] if rng.random() < 0.3 else int(rng.integers(2, 3000))
        tasks.append(_task(rng, n, int(rng.choice([3, 30, 300, 1500])), n_segs))
        dists.append((x, y))
    for e in edge:                                                          # every edge value on either side, with the other one below and above it
        for other in (7, 70000):
            for pair in ((e, other), (other, e)):
                tasks.append(_task(rng, 300, 40, n_segs)); dists.append(pair)
    d = np.array(dists)
    assert (d[:, 0] < d[:, 1]).sum() > 40 and (d[:, 0] > d[:, 1]).sum() > 40
    P = _params(n_segs)
    f, p, v, _, off = _gpu(P, tasks, d)
    f_ref, p_ref = _oracle(P, tasks, d)
    assert_same(f, p, f_ref, p_ref, off, f"per-task distances, n_segs {n_segs}: {v}")
    assert v.startswith("chain_dp_wave<R=256,SKIP=1,GEN=1"), v
    # the distances matter: the same tasks with one pair for all come out differently
    f1, p1, _ = ob.chain_batch(P, off, batch(tasks)[0], 2)
    assert not (np.array_equal(f1, f_ref) and np.array_equal(p1, p_ref))


@pytest.mark.parametrize("n_segs", [1, 2])
def test_two_copies_of_a_long_task_are_cut_in_different_places(n_segs):
    """20 000 anchors, x gaps of 400 and of 2 000 among steps of a few bases, as two tasks with max_dist_x 300 and 500: the device-side cut (tasks of 8 192 anchors
    or more) cuts the first copy at both kinds of gap and the second at the wide ones only, and a chain of the second copy runs across the gaps of 400"""
    rng = np.random.default_rng(5)
    n = 20000
    step = rng.integers(1, 8, n)
    step[rng.choice(np.arange(300, n, 300), 30, replace=False)] = 400
    step[[5000, 11000, 17000]] = 2000
    pos = 1000 + np.cumsum(step)
    seg = rng.integers(0, n_segs, n)
    q = 50 + np.cumsum(np.minimum(step, 20)) + seg * 200000
    x = (np.uint64(1) << np.uint64(32)) | pos.astype(np.uint64)
    y = (seg.astype(np.uint64) << np.uint64(48)) | (np.uint64(15) << np.uint64(32)) | q.astype(np.uint64)
    t = np.stack((x, y), 1)
    tasks, dists = [t, t.copy(), _task(rng, 100, 30, n_segs)], np.array([(300, 900), (500, 900), (40, 40)])
    P = _params(n_segs, bw=500)
    f, p, v, route, off = _gpu(P, tasks, dists)
    f_ref, p_ref = _oracle(P, tasks, dists)
    assert_same(f, p, f_ref, p_ref, off, f"two copies, n_segs {n_segs}: {v}")
    assert "cut=1" in v and v.startswith("chain_dp_wave<R=256"), v
    assert route[0] > 3 + 6, route                                           # more pieces than the wide gaps alone make
    assert not np.array_equal(f[:n], f[n:2 * n]) and not np.array_equal(p[:n], p[n:2 * n])


@pytest.mark.parametrize("max_skip", [25, 5000])
@pytest.mark.parametrize("n_segs", [1, 2])
def test_look_back_beyond_the_lds_ring(n_segs, max_skip):
    """about 3 000 dense anchors with max_iter 5000: windows of well over the 256 anchors of the LDS ring and the three tiles kept in registers, as wide as the
    task's own max_dist_x makes them"""
    rng = np.random.default_rng(3)
    base = fold_driver_tasks(rng, shapes=((3000, 4, 0.05, 0.15),))[0]
    if n_segs == 2:
        base = base.copy()
        base[:, 1] |= rng.integers(0, 2, base.shape[0]).astype(np.uint64) << np.uint64(48)
    tasks, dists = [base, base.copy(), base[:700].copy()], np.array([(5000, 5000), (1500, 2000), (300, 100)])
    P = _params(n_segs, bw=500, max_skip=max_skip, max_iter=5000)
    f, p, v, _, off = _gpu(P, tasks, dists)
    f_ref, p_ref = _oracle(P, tasks, dists)
    assert_same(f, p, f_ref, p_ref, off, f"far look-back, n_segs {n_segs}, max_skip {max_skip}: {v}")
    assert "FAR=1" in v and f"SKIP={int(max_skip < 5000)}" in v, v
    assert not np.array_equal(f[:3000], f[3000:6000])


@pytest.mark.parametrize("n_segs", [1, 2])
def test_pairs_equal_to_the_plans_own_and_back_to_them(n_segs):
    """all pairs equal to par's: the results of the same plan without distances; set_task_dists(None) afterwards restores the call-scalar run and its variant"""
    import mm2chain
    rng = np.random.default_rng(21)
    tasks = [_task(rng, int(rng.integers(1, 601)), 30, n_segs) for _ in range(64)]
    P = _params(n_segs, 700, 400)
    f0, p0, v0, _, off = _gpu(P, tasks, None)
    f_ref, p_ref, _ = ob.chain_batch(P, off, batch(tasks)[0], 2)
    assert_same(f0, p0, f_ref, p_ref, off, f"no distances: {v0}")
    a = batch(tasks)[0]
    d_a = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 2)).cuda()
    plan = mm2chain.ChainPlan(P, off)
    plan.set_task_dists(torch.tensor([[700, 400]] * len(tasks), dtype=torch.int32, device="cuda"))
    f1, p1 = _run(plan, d_a, a.shape[0])
    v1 = plan.last_variant()
    assert np.array_equal(f1, f0) and np.array_equal(p1, p0), v1
    assert v1.startswith("chain_dp_wave<R=256,SKIP=1,GEN=1"), v1
    plan.set_task_dists(None)
    f2, p2 = _run(plan, d_a, a.shape[0])
    assert np.array_equal(f2, f0) and np.array_equal(p2, p0) and plan.last_variant() == v0, (plan.last_variant(), v0)
    plan.close()
    if n_segs == 1:
        assert v0.startswith("chain_dp_tile<") or v0.startswith("chain_dp_coop<"), v0


def test_a_plan_never_given_distances_runs_what_it_ran():
    """the simple route, one wave per piece: the hand-written loop with the compact x / q ring and the packed f / p word (what tests/test_gpu_packed_fp.py expects of it)"""
    import mm2chain
    from mm2chain import params, synth
    P = params.map_ont()
    off, a = synth.make_stream("mixed", 64, 2000, seed=1, device="cuda")
    f = torch.empty(a.shape[0], dtype=torch.int32, device="cuda"); p = torch.empty_like(f)
    with mm2chain.tuned(coop_plans=0):
        plan = mm2chain.ChainPlan(P, off.numpy())
        plan.run(a, f, p)
        torch.cuda.synchronize()
        v = plan.last_variant()
        plan.close()
    assert v.startswith("chain_dp_tile<") and "GEN=0" in v and "loop=asm" in v and "compact=1" in v and "packed_fp=1" in v, v
    f_ref, p_ref, _ = ob.chain_batch(P, off.numpy(), a.cpu().numpy().view(np.uint64), 2)
    assert np.array_equal(f.cpu().numpy(), f_ref) and np.array_equal(p.cpu().numpy(), p_ref)
