"""Regions to hits on the device (csrc/chain_hits.hip: mm_set_parent hit.c:125-186, mm_select_sub hit.c:255-272): every case of tests/hits_data.py through HitPlan.run
and select_hits_batch, byte for byte against what the reference's own hit.o made of it (tests/golden/ref_hits.npz) over the first n_out regions of every read; the
cases as batches (grouped by equal options) and one read per call through one reused plan; DP -> epilogue -> RegPlan -> HitPlan on one stream without a host
synchronisation, against tests/hits_model.py on tests/regs_model.py on the oracle's chains; offsets beyond the capacities reported by check()."""
import os

import numpy as np
import pytest
import torch

import hits_data as D
import hits_model as M
import oracle_binding as ob
import regs_model

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
    Z = np.load(os.path.join(GOLDEN, "ref_hits.npz"))
    assert int(Z["reg_size"]) == M.REG.itemsize
    return [Z["hits"][Z["hit_off"][k]:Z["hit_off"][k + 1]].reshape(-1).view(M.REG) for k in range(Z["n_out"].size)]


def _opt(o):
    from mm2chain import params
    return params.hit_opts(**o)


def _run_plan(plan, o, cs):
    """the cases as one batch through plan.run on device tensors -> [REG array of n_out[r] hits per case]"""
    u_off, regs = D.batch(cs)
    assert regs.size <= plan.n_u_cap and len(cs) == plan.n_reads
    buf = np.zeros((max(plan.n_u_cap, 1), 80), np.uint8)
    buf[:regs.size] = regs.view(np.uint8).reshape(-1, 80)
    out, n_out = plan.run(_opt(o), torch.from_numpy(u_off).cuda(), torch.from_numpy(buf).cuda())
    total = plan.check()
    out, n_out = out.cpu().numpy(), n_out.cpu().numpy()
    assert total == int(n_out.sum())
    return [out[u_off[r]:u_off[r] + n_out[r]].reshape(-1).view(M.REG) for r in range(len(cs))]


def _assert_equal(got, want, cs, what):
    for g, w, c in zip(got, want, cs):
        assert g.size == w.size, f"{what}: {c['name']}: n_out = {g.size}, the reference {w.size}"
        bad = [i for i in range(g.size) if g[i].tobytes() != w[i].tobytes()]
        assert not bad, f"{what}: {c['name']}: {len(bad)} of {g.size} hits differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {w[bad[0]]}"


def test_every_case_in_batches_equals_the_reference(ref):
    import mm2chain
    cs = D.cases()
    seen = 0
    for o, idx in D.groups():
        sub = [cs[k] for k in idx]
        plan = mm2chain.HitPlan(len(sub), sum(c["regs"].size for c in sub))
        try:
            _assert_equal(_run_plan(plan, o, sub), [ref[k] for k in idx], sub, "HitPlan.run, one batch")
            assert plan.last_ms() > 0
        finally:
            plan.close()
        u_off, regs = D.batch(sub)
        out, n_out = mm2chain.select_hits_batch(_opt(o), u_off, regs)
        assert out.dtype == mm2chain.REG_DTYPE and n_out.dtype == np.int32
        _assert_equal([out[u_off[r]:u_off[r] + n_out[r]] for r in range(len(sub))], [ref[k] for k in idx], sub, "select_hits_batch")
        seen += len(idx)
    assert seen == len(cs)


def test_one_read_per_call_through_one_plan(ref):
    """reads do not leak into each other, and the plan's scratch is reused with other data and other options every time"""
    import mm2chain
    cs = D.cases()
    plan = mm2chain.HitPlan(1, max(c["regs"].size for c in cs))
    try:
        for k, c in enumerate(cs):
            _assert_equal(_run_plan(plan, c["opt"], [c]), [ref[k]], [c], "HitPlan.run, one read per call")
    finally:
        plan.close()
    u_off, regs = D.batch(cs)                                                  # ... and through the host entry, with offsets that do not start at 0
    for k in (1, len(cs) // 2, len(cs) - 1):
        out, n_out = mm2chain.select_hits_batch(_opt(cs[k]["opt"]), u_off[k:k + 2], regs)
        _assert_equal([out[:n_out[0]]], [ref[k]], [cs[k]], "select_hits_batch, one read")


def test_dp_epilogue_regions_hits_on_one_stream_without_a_host_sync():
    import mm2chain
    from mm2chain import synth, params
    P = params.map_ont()
    off, a = synth.make_stream("mixed", 64, 2000, seed=1, device="cuda")
    n_reads, total = off.numel() - 1, a.shape[0]
    f = torch.empty(total, dtype=torch.int32, device="cuda"); p = torch.empty_like(f)
    qlen = np.arange(n_reads, dtype=np.int32) * 37 + 20000
    hash_ = np.array([regs_model.read_hash(b"read%d" % r, int(qlen[r])) for r in range(n_reads)], np.uint32)
    d_q, d_h = torch.from_numpy(qlen).cuda(), torch.from_numpy(hash_.view(np.int32)).cuda()
    plan = mm2chain.ChainPlan(P, off.numpy())
    rp = mm2chain.RegPlan(n_reads, total, total)
    hp = mm2chain.HitPlan(n_reads, total)
    o = dict(D.DEFAULT)
    try:
        plan.run(a, f, p)
        u_off, u, b_off, b = plan.chains(a, f, p, 3, 40)
        regs = rp.run(u_off, u, b_off, b, d_q, d_h)
        hits, n_out = hp.run(_opt(o), u_off, regs)                            # nothing has come back to the host yet
        rp.check()
        n_total = hp.check()
        uo, got, no = u_off.cpu().numpy(), hits.cpu().numpy(), n_out.cpu().numpy()
        a_h, o_h = a.cpu().numpy().view(np.uint64), off.numpy()
        assert uo[-1] > n_reads and n_total == int(no.sum()) and 0 < n_total < uo[-1]
        for r in range(n_reads):
            u_ref, b_ref = ob.mm_chain_dp(P, 3, 40, a_h[o_h[r]:o_h[r + 1]])
            want = M.select_hits(regs_model.gen_regs(int(hash_[r]), int(qlen[r]), u_ref, b_ref), o)
            g = got[uo[r]:uo[r] + no[r]].reshape(-1).view(M.REG)
            assert no[r] == want.size and g.tobytes() == want.tobytes(), f"read {r}: the hits differ from the model on the oracle's chains"
    finally:
        hp.close(); rp.close(); plan.close()


def test_offsets_beyond_the_capacities_are_reported_and_a_second_run_is_clean(ref):
    """a read whose offsets leave the capacities touches nothing and makes check() an argument error; the reads beside it are right all the same, and the same plan
    then runs other data to that data's result"""
    import mm2chain
    cs = [c for c in D.cases() if c["opt"] == D.DEFAULT and c["name"] in ("n_sub_subsc", "random70", "first_not_best", "child_of_65th")]
    idx = {c["name"]: k for k, c in enumerate(D.cases())}
    assert len(cs) == 4
    u_off, regs = D.batch(cs)
    cap = regs.size
    plan = mm2chain.HitPlan(4, cap)
    buf = torch.from_numpy(regs.view(np.uint8).reshape(-1, 80).copy()).cuda()
    try:
        for broken in (np.array([u_off[0], u_off[1], cap + 5, cap + 5, cap + 9]), np.array([u_off[0], u_off[1], u_off[3], u_off[2], u_off[4]]),
                       np.array([u_off[0], u_off[1], -4, u_off[3], u_off[4]])):
            out = torch.full((cap, 80), 0xee, dtype=torch.uint8, device="cuda")
            n_out = torch.full((4,), -9, dtype=torch.int32, device="cuda")
            plan.run(_opt(D.DEFAULT), torch.from_numpy(broken.astype(np.int64)).cuda(), buf, regs_out=out, n_out=n_out)
            with pytest.raises(mm2chain.Mm2cError, match="code -2"):
                plan.check()
            got, no = out.cpu().numpy(), n_out.cpu().numpy()
            w = ref[idx[cs[0]["name"]]]
            assert no[0] == w.size and got[:w.size].reshape(-1).view(M.REG).tobytes() == w.tobytes(), "the read beside the broken ones"
            bad = [r for r in range(1, 4) if not (0 <= broken[r] <= broken[r + 1] <= cap)]
            assert bad and all(no[r] == -9 for r in bad), "a read with bad offsets wrote its n_out"
            if broken[2] >= cap:
                assert (got[u_off[1]:] == 0xee).all(), "reads with bad offsets touched the output"
        _assert_equal(_run_plan(plan, D.DEFAULT, cs[::-1]), [ref[idx[c["name"]]] for c in cs[::-1]], cs[::-1], "second run of the plan")
    finally:
        plan.close()
