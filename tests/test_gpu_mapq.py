"""Hits to mapping quality on the device (csrc/chain_mapq.hip: mm_join_long hit.c:295-371, mm_set_mapq hit.c:463-508): every case of tests/mapq_data.py through
MapqPlan.run and join_mapq_batch, byte for byte against what the reference's own hit.o made of it (tests/golden/ref_mapq.npz) -- the first n_out regions of every
read and, with anchors, the first n_b_out anchors; in batches through one plan that is reused, one read per call through another, with d_b_out and with NULL;
DP -> epilogue -> RegPlan -> HitPlan -> MapqPlan on one stream against the models on the oracle's chains; bad offsets, guard rows, the table's range, and a plan
run again on other data in another order."""
import os

import numpy as np
import pytest
import torch

import hits_model
import mapq_data as D
import mapq_model as M
import oracle_binding as ob
import regs_model

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL = 0xee


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def ref():
    Z = np.load(os.path.join(GOLDEN, "ref_mapq.npz"))
    cs = D.cases()
    assert int(Z["reg_size"]) == M.REG.itemsize and [str(v) for v in Z["names"]] == [c["name"] for c in cs]
    cut = lambda key, off, k: Z[key][Z[off][k]:Z[off][k + 1]]
    return [{"in": cut("hits_in", "in_off", k).reshape(-1).view(M.REG), "out": cut("hits_out", "out_off", k).reshape(-1).view(M.REG), "a": cut("a_out", "a_off", k),
             "case": c, "name": c["name"]} for k, c in enumerate(cs)]


def _opt(o):
    from mm2chain import params
    return params.mapq_opts(**o)


def _batch(rs, n_reads=None):
    """the reads one after another, each with room for as many regions as it has chains (the hits lie in front, the rest is filler); padded with empty reads"""
    n_reads = len(rs) if n_reads is None else n_reads
    room = [R["case"]["u"].size for R in rs] + [0] * (n_reads - len(rs))
    nb = [R["case"]["a"].shape[0] for R in rs] + [0] * (n_reads - len(rs))
    u_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64); b_off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    regs = np.full((max(int(u_off[-1]), 1), 80), FILL, np.uint8)
    for k, R in enumerate(rs):
        regs[u_off[k]:u_off[k] + R["in"].size] = R["in"].view(np.uint8).reshape(-1, 80)
    b = np.concatenate([R["case"]["a"] for R in rs] + [np.zeros((0, 2), np.uint64)])
    pad = lambda v, fill: np.array(v + [fill] * (n_reads - len(rs)), np.int32)
    return {"u_off": u_off, "b_off": b_off, "regs": regs, "b": b, "n_in": pad([R["in"].size for R in rs], 0), "qlen": pad([R["case"]["qlen"] for R in rs], 1000),
            "rep_len": pad([R["case"]["rep_len"] for R in rs], 0)}


def _run(plan, o, B, anchors, guard=0):
    """-> (regs_out [rows, 80] uint8, n_out, b_out or None, n_b_out or None) on the host; guard: rows and anchors behind the capacities, filled and looked at"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    regs = np.full((max(plan.n_u_cap, 1), 80), FILL, np.uint8); regs[:B["regs"].shape[0]] = B["regs"]
    b = np.zeros((max(plan.n_b_cap, 1), 2), np.int64); b[:B["b"].shape[0]] = B["b"].view(np.int64)
    out = torch.full((max(plan.n_u_cap, 1) + guard, 80), FILL, dtype=torch.uint8, device="cuda")
    n_out = torch.full((plan.n_reads + guard,), -9, dtype=torch.int32, device="cuda")
    b_out = torch.full((max(plan.n_b_cap, 1) + guard, 2), -3, dtype=torch.int64, device="cuda") if anchors else None
    n_b_out = torch.full((plan.n_reads + guard,), -9, dtype=torch.int64, device="cuda") if anchors else None
    d_b = t(b)
    plan.run(_opt(o), t(B["u_off"]), t(regs), t(B["n_in"]), t(B["b_off"]), d_b, t(B["qlen"]), t(B["rep_len"]), regs_out=out, n_out=n_out, b_out=b_out, n_b_out=n_b_out)
    torch.cuda.synchronize()
    assert np.array_equal(d_b.cpu().numpy(), b), "d_b was written"
    return out.cpu().numpy(), n_out.cpu().numpy(), (b_out.cpu().numpy().view(np.uint64) if anchors else None), (n_b_out.cpu().numpy() if anchors else None)


def _assert_read(got, B, k, R, what, anchors=True, want=None, tail=-3):
    """tail: what _run filled b_out with -- a squeezed read's anchors from n_b_out on still hold it; None for the host entry, whose b_out is its own"""
    out, n_out, b_out, n_b_out = got
    w = R["out"] if want is None else want
    assert n_out[k] == w.size, f"{what}: {R['name']}: n_out = {n_out[k]}, the reference {w.size}"
    g = out[B["u_off"][k]:B["u_off"][k] + w.size].reshape(-1).view(M.REG)
    bad = [i for i in range(w.size) if g[i].tobytes() != w[i].tobytes()]
    assert not bad, f"{what}: {R['name']}: {len(bad)} of {w.size} regions differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {w[bad[0]]}"
    if anchors and b_out is not None:
        assert n_b_out[k] == R["a"].shape[0], f"{what}: {R['name']}: n_b_out = {n_b_out[k]}, the reference {R['a'].shape[0]}"
        ga = b_out[B["b_off"][k]:B["b_off"][k] + R["a"].shape[0]]
        assert ga.tobytes() == R["a"].tobytes(), f"{what}: {R['name']}: a[] differs at {np.nonzero((ga != R['a']).any(axis=1))[0][:5]}"
        if tail is not None:
            gt = b_out[B["b_off"][k] + R["a"].shape[0]:B["b_off"][k + 1]]
            assert (gt.view(np.int64) == tail).all(), f"{what}: {R['name']}: {int((gt.view(np.int64) != tail).any(axis=1).sum())} anchors behind n_b_out were written"


def test_every_case_in_batches_through_one_plan_and_the_host_entry(ref):
    import mm2chain
    groups = D.groups()
    n_reads = max(len(idx) for _, idx in groups)
    plan = mm2chain.MapqPlan(n_reads, max(sum(ref[k]["case"]["u"].size for k in idx) for _, idx in groups), max(sum(ref[k]["case"]["a"].shape[0] for k in idx) for _, idx in groups))
    seen = n_joined = 0
    try:
        for o, idx in groups:
            rs = [ref[k] for k in idx]
            B = _batch(rs, n_reads)
            for anchors in (True, False):
                got = _run(plan, o, B, anchors)
                n_joined = plan.check()
                for k, R in enumerate(rs):
                    _assert_read(got, B, k, R, f"MapqPlan.run, one batch, anchors={anchors}")
                assert (got[1][len(rs):n_reads] == 0).all()
            assert plan.last_ms() > 0 and plan.last_kernel_ms()[0] > 0
            want_joined = sum(M.join_mapq(R["in"], R["case"]["a"], R["case"]["qlen"], o, R["case"]["rep_len"])[2] for R in rs)
            assert n_joined == want_joined
            Bh = _batch(rs)
            for anchors in (True, False):
                h = mm2chain.join_mapq_batch(_opt(o), Bh["u_off"], Bh["regs"], Bh["n_in"], Bh["b_off"], Bh["b"], Bh["qlen"], Bh["rep_len"], anchors=anchors)
                assert h[0].dtype == mm2chain.REG_DTYPE and h[1].dtype == np.int32 and (h[2] is None) == (not anchors)
                for k, R in enumerate(rs):
                    _assert_read((h[0].view(np.uint8).reshape(-1, 80), h[1], h[2], h[3]), Bh, k, R, f"join_mapq_batch, anchors={anchors}", tail=None)
            seen += len(idx)
    finally:
        plan.close()
    assert seen == len(ref)


def test_one_read_per_call_through_one_plan(ref):
    """reads do not leak into each other, and the plan's scratch is reused with other data and other options every time"""
    import mm2chain
    plan = mm2chain.MapqPlan(1, max(R["case"]["u"].size for R in ref), max(R["case"]["a"].shape[0] for R in ref))
    try:
        for j, R in enumerate(ref):
            B = _batch([R])
            _assert_read(_run(plan, R["case"]["mapq"], B, j % 2 == 0), B, 0, R, "MapqPlan.run, one read per call")
            plan.check()
    finally:
        plan.close()
    cs = [R for R in ref if R["case"]["mapq"] == D.MAPQ_DEFAULT]                # ... and through the host entry, with offsets that do not start at 0
    B = _batch(cs)
    for k in (1, len(cs) // 2, len(cs) - 1):
        h = mm2chain.join_mapq_batch(_opt(D.MAPQ_DEFAULT), B["u_off"][k:k + 2], B["regs"], B["n_in"][k:k + 1], B["b_off"][k:k + 2], B["b"], B["qlen"][k:k + 1], B["rep_len"][k:k + 1])
        one = {"u_off": np.array([0]), "b_off": np.array([0])}
        _assert_read((h[0].view(np.uint8).reshape(-1, 80), h[1], h[2], h[3]), one, 0, cs[k], "join_mapq_batch, one read", tail=None)


def test_dp_epilogue_regions_hits_mapq_on_one_stream_without_a_host_sync():
    import mm2chain
    from mm2chain import synth, params
    P = params.map_ont()
    off, a = synth.make_stream("mixed", 64, 2000, seed=1, device="cuda")
    n_reads, total = off.numel() - 1, a.shape[0]
    f = torch.empty(total, dtype=torch.int32, device="cuda"); p = torch.empty_like(f)
    qlen = np.arange(n_reads, dtype=np.int32) * 37 + 20000
    rep_len = (np.arange(n_reads, dtype=np.int32) * 131) % 900
    hash_ = np.array([regs_model.read_hash(b"read%d" % r, int(qlen[r])) for r in range(n_reads)], np.uint32)
    d_q, d_h, d_rep = torch.from_numpy(qlen).cuda(), torch.from_numpy(hash_.view(np.int32)).cuda(), torch.from_numpy(rep_len).cuda()
    plan = mm2chain.ChainPlan(P, off.numpy())
    rp = mm2chain.RegPlan(n_reads, total, total)
    hp = mm2chain.HitPlan(n_reads, total)
    mp = mm2chain.MapqPlan(n_reads, total, total)
    ho, mo = dict(D.HIT_DEFAULT), dict(D.MAPQ_DEFAULT)
    try:
        plan.run(a, f, p)
        u_off, u, b_off, b = plan.chains(a, f, p, 3, 40)
        regs = rp.run(u_off, u, b_off, b, d_q, d_h)
        hits, n_hits = hp.run(params.hit_opts(**ho), u_off, regs)
        fin, n_out, b_out, n_b_out = mp.run(_opt(mo), u_off, hits, n_hits, b_off, b, d_q, d_rep, anchors=True)   # nothing has come back to the host yet
        rp.check(); hp.check()
        n_joined = mp.check()
        uo, bo, got, no = u_off.cpu().numpy(), b_off.cpu().numpy(), fin.cpu().numpy(), n_out.cpu().numpy()
        ga, nb = b_out.cpu().numpy().view(np.uint64), n_b_out.cpu().numpy()
        a_h, o_h = a.cpu().numpy().view(np.uint64), off.numpy()
        want_joined = 0
        for r in range(n_reads):
            u_ref, b_ref = ob.mm_chain_dp(P, 3, 40, a_h[o_h[r]:o_h[r + 1]])
            h = hits_model.select_hits(regs_model.gen_regs(int(hash_[r]), int(qlen[r]), u_ref, b_ref), ho)
            want, wa, nj = M.join_mapq(h, b_ref, int(qlen[r]), mo, int(rep_len[r]))
            want_joined += nj
            g = got[uo[r]:uo[r] + no[r]].reshape(-1).view(M.REG)
            assert no[r] == want.size and g.tobytes() == want.tobytes(), f"read {r}: the final regions differ from the models on the oracle's chains"
            assert nb[r] == wa.shape[0] and ga[bo[r]:bo[r] + nb[r]].tobytes() == wa.tobytes(), f"read {r}: a[] differs from the model"
        assert n_joined == want_joined
        print(f"{n_reads} reads, {int(no.sum())} final regions, {n_joined} joins")
    finally:
        mp.close(); hp.close(); rp.close(); plan.close()


def test_bad_offsets_are_reported_and_the_neighbours_stay_exact(ref):
    """a read whose u_off / b_off / n_in leave the capacities or each other, or a hit of which leaves the read's anchors, touches nothing and makes check() an
    argument error; the reads beside it are exact, regions and anchors (the gather then goes read by read); guard rows behind the capacities stay untouched"""
    import mm2chain
    names = ("adjacent_by_drop", "grown_r1", "hier_third_outranks_fourth", "mapq_several_primaries")
    rs = [next(R for R in ref if R["name"] == n) for n in names]
    B0 = _batch(rs)
    cap_u, cap_b = int(B0["u_off"][-1]), int(B0["b_off"][-1])
    plan = mm2chain.MapqPlan(4, cap_u, cap_b)

    def broken(**kw):
        B = {k: v.copy() for k, v in B0.items()}
        for key, (at, val) in kw.items():
            B[key][at] = val
        return B
    hit_beyond = broken()
    h = hit_beyond["regs"][B0["u_off"][1]:B0["u_off"][1] + 1].reshape(-1).view(M.REG)
    h["as"] = 1000                                                              # read 1: a hit that leaves the read's anchors
    pats = {"u_off beyond the capacity": (broken(u_off=(slice(2, 4), cap_u + 5)), [1, 2, 3]), "u_off descending": (broken(u_off=(2, B0["u_off"][3] + 1)), [2]),
            "u_off negative": (broken(u_off=(2, -4)), [1, 2]), "b_off beyond the capacity": (broken(b_off=(slice(2, 4), cap_b + 9)), [1, 2, 3]),
            "b_off descending": (broken(b_off=(2, B0["b_off"][1] - 1)), [1]), "n_in beyond its room": (broken(n_in=(1, rs[1]["case"]["u"].size + 1)), [1]),
            "n_in negative": (broken(n_in=(2, -1)), [2]), "a hit beyond the read's anchors": (hit_beyond, [1])}
    try:
        for what, (B, bad) in pats.items():
            for anchors in (True, False):
                got = _run(plan, D.MAPQ_DEFAULT, B, anchors, guard=3)
                rc, _, _ = plan.counts()
                assert rc == -2, f"{what}: check() = {rc}"
                out, n_out, b_out, n_b_out = got
                for k in range(4):
                    if k in bad:
                        assert n_out[k] == -9 and (not anchors or n_b_out[k] == -9), f"{what}: the refused read {k} wrote its counts"
                    elif not (what.startswith("b_off descending") and k == 2):   # (its own offsets are sound, but its segment then overlaps read 1's)
                        # (read 2's segment then begins on the last anchor of read 0's tail: no tail check in that pattern)
                        _assert_read(got, B, k, rs[k], what, anchors, tail=None if what.startswith("b_off descending") else -3)
                assert (out[cap_u:] == FILL).all() and (n_out[4:] == -9).all(), f"{what}: guard rows were written"
                if anchors:
                    assert (b_out[cap_b:].view(np.int64) == -3).all() and (n_b_out[4:] == -9).all(), f"{what}: guard anchors were written"
                if "beyond the capacity" in what:
                    lo = B0["u_off"][1] if what.startswith("u_off") else None
                    assert lo is None or (out[lo:cap_u] == FILL).all(), f"{what}: refused reads touched the output"
        got = _run(plan, D.MAPQ_DEFAULT, B0, True, guard=3)                      # the same plan on sound data afterwards
        plan.check()
        for k in range(4):
            _assert_read(got, B0, k, rs[k], "sound data behind the broken ones")
        assert (got[0][cap_u:] == FILL).all() and (got[2][cap_b:].view(np.int64) == -3).all()
    finally:
        plan.close()


def test_beyond_the_table_is_reported_and_nothing_else_changes(ref):
    import mm2chain
    names = (f"table_score{D.SMALL_TABLE}", f"table_score{D.SMALL_TABLE + 1}", "n2_join", "n1")
    rs = [next(R for R in ref if R["name"] == n) for n in names]
    B = _batch(rs)
    plan = mm2chain.MapqPlan(4, int(B["u_off"][-1]), int(B["b_off"][-1]), max_log_arg=D.SMALL_TABLE)
    try:
        got = _run(plan, D.MAPQ_DEFAULT, B, True)
        rc, n_joined, n_beyond = plan.counts()
        assert (rc, n_joined, n_beyond) == (-3, 1, 2), "score 4097 and the joined 5900 lie beyond a table of 4096"
        with pytest.raises(mm2chain.Mm2cError, match="code -3"):
            plan.check()
        for k in (0, 3):
            _assert_read(got, B, k, rs[k], "beside a primary beyond the table")
        for k in (1, 2):
            c = rs[k]["case"]
            want = M.join_mapq(rs[k]["in"], c["a"], c["qlen"], c["mapq"], c["rep_len"], beyond=D.SMALL_TABLE)[0]
            assert want.tobytes() != rs[k]["out"].tobytes()
            _assert_read(got, B, k, rs[k], "a primary beyond the table: mapq 0, the rest as the reference", want=want)
        got = _run(plan, D.MAPQ_DEFAULT, _batch([rs[0], rs[3]], 4), True)        # the count is per run
        assert plan.counts() == (0, 0, 0)
    finally:
        plan.close()


def test_a_plan_run_again_on_other_data_in_another_order(ref):
    import mm2chain
    rs = [R for R in ref if R["case"]["mapq"] == D.MAPQ_DEFAULT]
    first, second = rs[:len(rs) // 2], rs[len(rs) // 2:][::-1]
    n_reads = max(len(first), len(second))
    plan = mm2chain.MapqPlan(n_reads, max(sum(R["case"]["u"].size for R in g) for g in (first, second)), max(sum(R["case"]["a"].shape[0] for R in g) for g in (first, second)))
    try:
        for g, anchors in ((first, True), (second, False), (first[::-1], False), (second[::2], True)):
            B = _batch(g, n_reads)
            got = _run(plan, D.MAPQ_DEFAULT, B, anchors)
            plan.check()
            for k, R in enumerate(g):
                _assert_read(got, B, k, R, "a plan run again")
    finally:
        plan.close()
