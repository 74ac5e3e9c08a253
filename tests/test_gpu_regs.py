"""Chains to regions on the device (csrc/chain_regs.hip, mm_gen_regs hit.c:52-88): every case of tests/regs_data.py through RegPlan.run and gen_regs_batch, byte for
byte against what the reference's own hit.o made of it (tests/golden/ref_regs.npz); the cases as one batch and one read per call; DP -> epilogue -> regions on one
stream without a host synchronisation in between, against tests/regs_model.py on the oracle's mm_chain_dp; the check accessor; a plan run again on other data."""
import os

import numpy as np
import pytest
import torch

import oracle_binding as ob
import regs_data
import regs_model as M

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
    Z = np.load(os.path.join(GOLDEN, "ref_regs.npz"))
    assert int(Z["reg_size"]) == M.REG.itemsize
    return {"regs": Z["regs"], "off": Z["reg_off"], "n_tie_reads": int(Z["n_tie_reads"])}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view({8: np.int64, 4: np.int32}[x.dtype.itemsize])).cuda()


def _run_plan(plan, cs):
    """the cases as one batch through plan.run on device tensors -> (uint8 [n_u, 80] on the host, reads with ties)"""
    u_off, u, b_off, b, qlen, hash_ = regs_data.batch(cs)
    assert u.size <= plan.n_u_cap and b.shape[0] <= plan.n_b_cap
    pad = lambda x, n: np.concatenate([x, np.zeros((n - x.shape[0],) + x.shape[1:], x.dtype)])
    regs = plan.run(_dev(u_off), _dev(pad(u, max(plan.n_u_cap, 1))), _dev(b_off), _dev(pad(b, max(plan.n_b_cap, 1))), _dev(qlen), _dev(hash_))
    ties = plan.check()
    return regs.cpu().numpy()[:u.size], ties


def _assert_equal(got, want, cs, what):
    """got / want: uint8 [n, 80] of the cases one after another"""
    assert got.shape == want.shape, f"{what}: {got.shape[0]} regions, expected {want.shape[0]}"
    at = 0
    for c in cs:
        n = c["u"].size
        g, w = got[at:at + n].reshape(-1).view(M.REG), want[at:at + n].reshape(-1).view(M.REG)
        bad = [i for i in range(n) if g[i].tobytes() != w[i].tobytes()]
        assert not bad, f"{what}: {c['name']}: {len(bad)} of {n} regions differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {w[bad[0]]}"
        at += n


def test_every_case_as_one_batch_equals_the_reference(ref):
    import mm2chain
    cs = regs_data.cases()
    n_u, n_b = sum(c["u"].size for c in cs), sum(c["a"].shape[0] for c in cs)
    plan = mm2chain.RegPlan(len(cs), n_u, n_b)
    try:
        got, ties = _run_plan(plan, cs)
        _assert_equal(got, ref["regs"], cs, "RegPlan.run, one batch")
        assert ties == ref["n_tie_reads"], f"check() counts {ties} reads with equal keys, the fixture {ref['n_tie_reads']}"
        assert plan.last_ms() > 0 and min(plan.last_kernel_ms()) > 0
    finally:
        plan.close()
    u_off, u, b_off, b, qlen, hash_ = regs_data.batch(cs)
    host = mm2chain.gen_regs_batch(u_off, u, b_off, b, qlen, hash_)
    assert host.dtype == mm2chain.REG_DTYPE and host.dtype.itemsize == 80
    _assert_equal(host.view(np.uint8).reshape(-1, 80), ref["regs"], cs, "gen_regs_batch, one batch")


def test_one_read_per_call_equals_the_batch(ref):
    """reads do not leak into each other: every case alone (its chain anchors then start at 0 of b, so the slices of the fill pass fall elsewhere) gives the rows it has
    in the batch; the plan is the same for all of them, so its scratch is reused with other data every time"""
    import mm2chain
    cs = regs_data.cases()
    plan = mm2chain.RegPlan(1, max(c["u"].size for c in cs), max(c["a"].shape[0] for c in cs))
    try:
        for k, c in enumerate(cs):
            got, _ = _run_plan(plan, [c])
            _assert_equal(got, ref["regs"][ref["off"][k]:ref["off"][k + 1]], [c], "RegPlan.run, one read per call")
    finally:
        plan.close()
    for k in (0, len(cs) // 2, len(cs) - 1):                                 # ... and through the host entry, with offsets that do not start at 0
        u_off, u, b_off, b, qlen, hash_ = regs_data.batch(cs)
        host = mm2chain.gen_regs_batch(u_off[k:k + 2], u, b_off[k:k + 2], b, qlen[k:k + 1], hash_[k:k + 1])
        _assert_equal(host.view(np.uint8).reshape(-1, 80), ref["regs"][ref["off"][k]:ref["off"][k + 1]], [cs[k]], "gen_regs_batch, one read")


def test_dp_epilogue_regions_on_one_stream_without_a_host_sync():
    import mm2chain
    from mm2chain import synth, params
    P = params.map_ont()
    off, a = synth.make_stream("mixed", 64, 2000, seed=1, device="cuda")
    n_reads, total = off.numel() - 1, a.shape[0]
    f = torch.empty(total, dtype=torch.int32, device="cuda"); p = torch.empty_like(f)
    qlen = np.arange(n_reads, dtype=np.int32) * 37 + 20000
    hash_ = np.array([M.read_hash(b"read%d" % r, int(qlen[r])) for r in range(n_reads)], np.uint32)
    d_q, d_h = _dev(qlen), _dev(hash_)
    plan = mm2chain.ChainPlan(P, off.numpy())
    rp = mm2chain.RegPlan(n_reads, total, total)
    try:
        plan.run(a, f, p)
        u_off, u, b_off, b = plan.chains(a, f, p, 3, 40)
        regs = rp.run(u_off, u, b_off, b, d_q, d_h)                          # nothing has come back to the host yet
        rp.check()
        uo = u_off.cpu().numpy()
        got = regs.cpu().numpy()
        a_h, o_h = a.cpu().numpy().view(np.uint64), off.numpy()
        assert uo[-1] > n_reads
        for r in range(n_reads):
            u_ref, b_ref = ob.mm_chain_dp(P, 3, 40, a_h[o_h[r]:o_h[r + 1]])
            want = M.gen_regs(int(hash_[r]), int(qlen[r]), u_ref, b_ref)
            g = got[uo[r]:uo[r + 1]].reshape(-1).view(M.REG)
            assert g.size == want.size and g.tobytes() == want.tobytes(), f"read {r}: the regions differ from the model on the oracle's chains"
    finally:
        rp.close(); plan.close()


def test_inconsistent_counts_are_reported_and_a_second_run_is_clean(ref):
    """a count sum that differs from the extent of b is an argument error reported by check() (the kernels clamp what they read); the regions of the reads beside it
    are right all the same, and the same plan then runs other data to that data's result"""
    import mm2chain
    cs = [c for c in regs_data.cases() if c["name"] in ("cnt1_among", "rows", "one_chain", "sort65")]
    bad = dict(cs[1]); bad["u"] = bad["u"].copy(); bad["u"][2] += np.uint64(5)         # five anchors more than the read has
    short = dict(cs[2]); short["u"] = short["u"].copy(); short["u"][0] -= np.uint64(3)   # three fewer
    hollow = dict(cs[2]); hollow["u"] = np.full(1100, 50 << 32, np.uint64)              # 1 100 chains without anchors: more chains than a slice of the fill pass has anchors
    want = {c["name"]: M.gen_regs(c["hash"], c["qlen"], c["u"], c["a"]).view(np.uint8).reshape(-1, 80) for c in cs}
    plan = mm2chain.RegPlan(4, 1400, 2000)
    try:
        for broken in ([cs[0], bad, cs[2], cs[3]], [cs[0], cs[1], short, cs[3]], [cs[0], cs[1], hollow, cs[3]]):
            u_off, u, b_off, b, qlen, hash_ = regs_data.batch(broken)          # (batch() goes by the sizes of the arrays, not by the counts in u)
            pad = lambda x, n: np.concatenate([x, np.zeros((n - x.shape[0],) + x.shape[1:], x.dtype)])
            regs = plan.run(_dev(u_off), _dev(pad(u, 1400)), _dev(b_off), _dev(pad(b, 2000)), _dev(qlen), _dev(hash_))
            with pytest.raises(mm2chain.Mm2cError, match="code -2"):
                plan.check()
            got = regs.cpu().numpy()
            for k in (0, 3):
                assert np.array_equal(got[u_off[k]:u_off[k + 1]], want[cs[k]["name"]]), f"read {k} beside the inconsistent one"
        got, _ = _run_plan(plan, cs[::-1])
        _assert_equal(got, np.concatenate([want[c["name"]] for c in cs[::-1]]), cs[::-1], "second run of the plan")
    finally:
        plan.close()
