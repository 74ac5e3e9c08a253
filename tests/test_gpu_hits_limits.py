"""Regions to hits on the device at the limits of the kernel's own implementation (csrc/chain_hits.hip): the cases of tests/hits_limit_data.py -- the gap measure with
the region's start in a round of its own, equal ends in one round and across rounds, the passing primary in the last lane of a ballot and the first of the next, the
covered length out of the third round, the record move with 1 and 129 of 130 kept -- byte for byte against what the reference's hit.o made of them
(tests/golden/ref_hits_limits.npz): as batches grouped by equal options, one read per call through one reused plan, and through select_hits_batch."""
import os

import numpy as np
import pytest
import torch

import hits_limit_data as L
import hits_model as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def ref():
    Z = np.load(os.path.join(GOLDEN, "ref_hits_limits.npz"))
    assert int(Z["reg_size"]) == M.REG.itemsize and [str(s) for s in Z["names"]] == [c["name"] for c in L.cases()]
    return [Z["hits"][Z["hit_off"][k]:Z["hit_off"][k + 1]].reshape(-1).view(M.REG) for k in range(Z["n_out"].size)]


def _opt(o):
    from mm2chain import params
    return params.hit_opts(**o)


def _run_plan(plan, o, cs):
    """the cases as one batch through plan.run on device tensors -> [REG array of n_out[r] hits per case]"""
    u_off, regs = L.batch(cs)
    assert regs.size <= plan.n_u_cap and len(cs) == plan.n_reads
    buf = np.zeros((max(plan.n_u_cap, 1), 80), np.uint8)
    buf[:regs.size] = regs.view(np.uint8).reshape(-1, 80)
    out, n_out = plan.run(_opt(o), torch.from_numpy(u_off).cuda(), torch.from_numpy(buf).cuda())
    total = plan.check()
    out, n_out = out.cpu().numpy(), n_out.cpu().numpy()
    assert total == int(n_out.sum())
    return [out[u_off[r]:u_off[r] + n_out[r]].reshape(-1).view(M.REG) for r in range(len(cs))]


def _assert_equal(got, want, cs, what):
    bad = []
    for g, w, c in zip(got, want, cs):
        if g.size != w.size:
            bad.append(f"{c['name']}: n_out = {g.size}, the reference {w.size}")
            continue
        d = [i for i in range(g.size) if g[i].tobytes() != w[i].tobytes()]
        if d:
            bad.append(f"{c['name']}: {len(d)} of {g.size} hits differ, first at {d[0]}:\n got {g[d[0]]}\nwant {w[d[0]]}")
    assert not bad, f"{what}: {len(bad)} case(s) differ from the reference:\n" + "\n".join(bad)


def test_every_case_in_batches_equals_the_reference(ref):
    import mm2chain
    cs = L.cases()
    seen = 0
    for o, idx in L.groups():
        sub = [cs[k] for k in idx]
        plan = mm2chain.HitPlan(len(sub), sum(c["regs"].size for c in sub))
        try:
            _assert_equal(_run_plan(plan, o, sub), [ref[k] for k in idx], sub, "HitPlan.run, one batch")
        finally:
            plan.close()
        seen += len(idx)
    assert seen == len(cs)


def test_one_read_per_call_through_one_plan(ref):
    """the plan's scratch is reused with other data and other options every time: the reads beyond the LDS class leave their tables behind for the next"""
    import mm2chain
    cs = L.cases()
    plan = mm2chain.HitPlan(1, max(c["regs"].size for c in cs))
    try:
        got = [_run_plan(plan, c["opt"], [c])[0] for c in cs]
    finally:
        plan.close()
    _assert_equal(got, ref, cs, "HitPlan.run, one read per call")


def test_every_case_through_the_host_entry(ref):
    import mm2chain
    cs = L.cases()
    for o, idx in L.groups():
        sub = [cs[k] for k in idx]
        u_off, regs = L.batch(sub)
        out, n_out = mm2chain.select_hits_batch(_opt(o), u_off, regs)
        assert out.dtype == mm2chain.REG_DTYPE and n_out.dtype == np.int32
        _assert_equal([out[u_off[r]:u_off[r] + n_out[r]] for r in range(len(sub))], [ref[k] for k in idx], sub, "select_hits_batch")
