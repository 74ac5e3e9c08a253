"""Chain-anchor divergence on the device (csrc/chain_esterr.hip: mm_est_err map.c:357, esterr.c): every case of tests/esterr_data.py through EstErrPlan.run and
est_err_batch -- (n_match, n_tot) per region and avg_k per read equal the model's exactly, and after mm2c_est_err_apply_host the regions are, byte for byte, what
the reference's own hit.o and esterr.o made of the case (tests/golden/ref_esterr.npz); in one batch through a plan that is reused, one read per call through
another; reads in -> chains -> RegPlan -> HitPlan -> MapqPlan (anchors out) -> EstErrPlan on one stream against the models on the oracle's chains; every kind of refusal with guard rows;
and a plan run again on other data, in another order and of another size.  The model's counts are made once per module.

Reads of a batch share one ref_len array: every read's reference lengths are appended to it and the rid of its regions is moved accordingly in the plan's input."""
import numpy as np
import pytest
import torch

import esterr_data as D
import esterr_model as M
import hits_model
import index_model as im
import mapq_data
import mapq_model
import oracle_binding as ob
import regs_model
import sketch_model as sm

pytestmark = pytest.mark.gpu
ERR_FILL, AVG_FILL = -7, -5.0


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def ref():
    rs = D.reference()
    for R in rs:
        c = R["case"]
        R["cnts"], R["avg_k"] = M.counts(R["in"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"])
    return rs


def _batch(rs, n_reads=None, room=1):
    """the reads one after another, each with `room` filler rows behind its regions; padded with empty reads"""
    n_reads = len(rs) if n_reads is None else n_reads
    pad = n_reads - len(rs)
    off = lambda v: np.concatenate([[0], np.cumsum(v + [0] * pad)]).astype(np.int64)
    u_off, b_off = off([R["in"].size + room for R in rs]), off([R["a"].shape[0] for R in rs])
    m_off, r_off = off([R["case"]["mini_pos"].size for R in rs]), off([R["case"]["ref_len"].size for R in rs])
    regs = np.full((max(int(u_off[-1]), 1), 80), 0xee, np.uint8)
    for k, R in enumerate(rs):
        g = R["in"].copy()
        g["rid"] += int(r_off[k])
        regs[u_off[k]:u_off[k] + g.size] = g.view(np.uint8).reshape(-1, 80)
    cat = lambda parts, empty: np.concatenate(list(parts) + [empty])
    return {"u_off": u_off, "b_off": b_off, "mini_off": m_off, "regs": regs, "b": cat((R["a"] for R in rs), np.zeros((0, 2), np.uint64)),
            "mini_pos": cat((R["case"]["mini_pos"] for R in rs), np.zeros(0, np.uint64)), "ref_len": cat((R["case"]["ref_len"] for R in rs), np.zeros(0, np.uint32)),
            "n_in": np.array([R["in"].size for R in rs] + [0] * pad, np.int32), "qlen": np.array([R["case"]["qlen"] for R in rs] + [1000] * pad, np.int32)}


def _run(plan, B, guard=0):
    """-> (err [rows, 2] int32, avg_k float32) on the host; guard: rows in front of the outputs and behind the capacities, filled and looked at: those in front here, those behind
    by the caller.  The inputs must come back unwritten."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    regs = np.full((max(plan.n_u_cap, 1), 80), 0xee, np.uint8); regs[:B["regs"].shape[0]] = B["regs"]
    b = np.zeros((max(plan.n_b_cap, 1), 2), np.int64); b[:B["b"].shape[0]] = B["b"].view(np.int64)
    mp = np.zeros(max(plan.n_mini_cap, 1), np.int64); mp[:B["mini_pos"].size] = B["mini_pos"].view(np.int64)
    rl = np.zeros(max(B["ref_len"].size, 1), np.int32); rl[:B["ref_len"].size] = B["ref_len"].view(np.int32)
    err = torch.full((guard + max(plan.n_u_cap, 1) + guard, 2), ERR_FILL, dtype=torch.int32, device="cuda")    # guard rows in front of the outputs and behind them
    avg = torch.full((guard + plan.n_reads + guard,), AVG_FILL, dtype=torch.float32, device="cuda")
    d_regs, d_b, d_mp = t(regs), t(b), t(mp)
    plan.run(t(B["u_off"]), d_regs, t(B["n_in"]), t(B["b_off"]), d_b, t(B["mini_off"]), d_mp, t(B["qlen"]), t(rl)[:B["ref_len"].size], err=err[guard:], avg_k=avg[guard:])
    torch.cuda.synchronize()
    assert np.array_equal(d_regs.cpu().numpy(), regs) and np.array_equal(d_b.cpu().numpy(), b) and np.array_equal(d_mp.cpu().numpy(), mp), "an input was written"
    err, avg = err.cpu().numpy(), avg.cpu().numpy()
    assert (err[:guard] == ERR_FILL).all() and (avg[:guard] == AVG_FILL).all(), "guard rows in front of the outputs were written"
    return err[guard:], avg[guard:]


def _assert_read(got, B, k, R, what):
    """counts and avg_k equal the model's; applied to the host's regions they give the reference's bytes"""
    import mm2chain
    err, avg = got
    n, lo = R["in"].size, int(B["u_off"][k])
    g = err[lo:lo + n]
    assert np.array_equal(g, R["cnts"]), f"{what}: {R['name']}: counts differ at regions {np.nonzero((g != R['cnts']).any(axis=1))[0][:5]}:\n got {g[:6].tolist()}\nwant {R['cnts'][:6].tolist()}"
    assert np.float32(avg[k]).tobytes() == np.float32(R["avg_k"]).tobytes(), f"{what}: {R['name']}: avg_k = {avg[k]!r}, the model {R['avg_k']!r}"
    regs = R["in"].copy()
    mm2chain.est_err_apply([0], [n], g.copy(), avg[k:k + 1], regs)
    if regs.tobytes() != R["out"].tobytes():
        model = M.apply(R["in"], R["cnts"], R["avg_k"])
        assert regs.tobytes() == model.tobytes(), f"{what}: {R['name']}: div differs from the model's: {regs['div'][:4]} / {model['div'][:4]}"
        assert False, f"{what}: {R['name']}: div {regs['div'][:4]} equals the model's but not the fixture's {R['out']['div'][:4]}: this machine's libm is not the fixture's ({R['libm']})"


def _caps(groups):
    s = lambda g, f: sum(f(R) for R in g)
    return (max(s(g, lambda R: R["in"].size + 1) for g in groups), max(s(g, lambda R: R["a"].shape[0]) for g in groups),
            max(s(g, lambda R: R["case"]["mini_pos"].size) for g in groups))


def test_every_case_in_one_batch_through_one_plan_and_the_host_entry(ref):
    import mm2chain
    n_reads = len(ref) + 3
    plan = mm2chain.EstErrPlan(n_reads, *_caps([ref]))
    try:
        for order in (ref, ref[::-1]):                                          # (the slice cases then lie at other positions of the b index space)
            B = _batch(order, n_reads)
            got = _run(plan, B)
            plan.check()
            for k, R in enumerate(order):
                _assert_read(got, B, k, R, "EstErrPlan.run, one batch")
            assert plan.last_ms() > 0 and all(v > 0 for v in plan.last_kernel_ms())
    finally:
        plan.close()
    B = _batch(ref, room=0)
    regs, err, avg = mm2chain.est_err_batch(B["u_off"], B["regs"], B["n_in"], B["b_off"], B["b"], B["mini_off"], B["mini_pos"], B["qlen"], B["ref_len"])
    assert regs.dtype == mm2chain.REG_DTYPE and err.dtype == mm2chain.ERR_DTYPE and avg.dtype == np.float32
    r_off = np.concatenate([[0], np.cumsum([R["case"]["ref_len"].size for R in ref])])
    for k, R in enumerate(ref):
        lo = int(B["u_off"][k])
        g = regs[lo:lo + R["in"].size].copy()
        g["rid"] -= int(r_off[k])
        assert np.array_equal(err[lo:lo + R["in"].size].view(np.int32).reshape(-1, 2), R["cnts"]) and avg[k].tobytes() == np.float32(R["avg_k"]).tobytes(), R["name"]
        libm = f" (a libm-sensitive case: this machine's libm may not be the fixture's, {R['libm']})" if R["name"].startswith(("libm_", "avgk_frac_")) else ""
        assert g.tobytes() == R["out"].tobytes(), f"est_err_batch: {R['name']}: regions differ from the reference's" + libm


def test_one_read_per_call_through_one_plan(ref):
    """reads do not leak into each other, the plan's scratch is reused with other data every time, and every read starts at position 0 of the b index space: the
    slice cases then have their boundary at a[] position 4096 exactly"""
    import mm2chain
    plan = mm2chain.EstErrPlan(1, *_caps([[R] for R in ref]))
    try:
        for R in ref:
            B = _batch([R])
            _assert_read(_run(plan, B), B, 0, R, "EstErrPlan.run, one read per call")
            plan.check()
    finally:
        plan.close()
    some = [R for R in ref if R["name"] in ("both_strands", "joined", "unsqueezed_as_nonzero", "two_rids", "no_mini", "cnt65")]
    B = _batch(some, room=0)                                                    # ... and through the host entry, with offsets that do not start at 0
    for k in (1, 2, len(some) - 1):
        regs, err, avg = mm2chain.est_err_batch(B["u_off"][k:k + 2], B["regs"], B["n_in"][k:k + 1], B["b_off"][k:k + 2], B["b"], B["mini_off"][k:k + 2], B["mini_pos"],
                                                B["qlen"][k:k + 1], B["ref_len"])
        _assert_read((err.view(np.int32).reshape(-1, 2), avg), {"u_off": [0]}, 0, some[k], "est_err_batch, one read")


def _genome_and_reads():
    rng = np.random.default_rng(20261022)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    refs = [acgt[rng.integers(0, 4, n)] for n in (90000, 60000)]
    comp = np.zeros(256, np.uint8); comp[acgt] = acgt[::-1]
    reads = []
    for k in range(36):
        g = refs[k % 2]
        n = int(rng.integers(2000, 5001))
        at = int(rng.integers(0, g.size - n))
        s = g[at:at + n].copy()
        hit = rng.random(n) < 0.04                                              # substitutions: minimizers that match nothing, chains with gaps
        s[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        if k % 9 == 4:                                                          # a read of two pieces: more than one region
            n2 = int(rng.integers(1500, 2500)); at2 = int(rng.integers(0, g.size - n2))
            s = np.concatenate([s, g[at2:at2 + n2]])
        reads.append((comp[s[::-1]] if k % 2 else s).tobytes())
    return [g.tobytes() for g in refs], reads


def test_reads_in_to_div_on_one_stream_without_a_host_sync():
    """reads in, chains out (read_chain_batch: sketch, lookups, seed hits, DP, epilogue on the device, with the real mini_pos), then RegPlan -> HitPlan -> MapqPlan
    with anchors out -> EstErrPlan on one stream, nothing coming back in between; against the models of all four steps on the ORACLE's chains and the CPU
    pipeline's mini_pos (the model index and sketch, collect_matches, collect_seed_hits and mm_chain_dp of the oracle, as tests/test_gpu_read_chain_e2e.py)"""
    import mm2chain
    from mm2chain import params
    refs, reads = _genome_and_reads()
    P = params.map_ont()
    keys, cr_off, n_occ, pool_h = im.build_index(refs, 15, 10, 0)
    mid_occ = im.cal_max_occ(n_occ)
    lookup = sm.table_lookup(keys, cr_off, n_occ)
    cpu = []                                                                    # per read: (u, b, rep_len, mini_pos) of the CPU pipeline
    for s in reads:
        matches, rep_len, mini_pos = sm.collect_matches(sm.sketch_array(s, 10, 15, 0), lookup, mid_occ)
        ur, br = ob.mm_chain_dp(P, 3, 40, ob.collect_seed_hits(sm.match_array(matches), pool_h, len(s)))
        cpu.append((ur, br, int(rep_len), np.array(mini_pos, np.uint64)))
    pool = mm2chain.HitPool(pool_h)
    idx = mm2chain.MinimizerIndex(15, 10, 0, keys, cr_off, n_occ, pool=pool)
    rc = mm2chain.read_chain_batch(P, 3, 40, reads, idx, mid_occ)
    idx.close(); pool.close()
    n_reads = len(reads)
    n_u, n_b, n_m = int(rc["u_off"][-1]), int(rc["b_off"][-1]), int(rc["mini_off"][-1])
    assert n_u >= n_reads and n_m > 100 * n_reads
    qlen = np.array([len(s) for s in reads], np.int32)
    hash_ = np.array([regs_model.read_hash(b"read%d" % r, int(qlen[r])) for r in range(n_reads)], np.uint32)
    ref_len = np.array([len(g) for g in refs], np.uint32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u_off, u, b_off, b = t(rc["u_off"]), t(rc["u"].view(np.int64)), t(rc["b_off"]), t(rc["b"].view(np.int64))
    d_q, d_h, d_rep = t(qlen), t(hash_.view(np.int32)), t(rc["rep_len"])
    d_mo, d_mp, d_rl = t(rc["mini_off"]), t(rc["mini_pos"].view(np.int64)), t(ref_len.view(np.int32))
    ho, mo = dict(mapq_data.HIT_DEFAULT), dict(mapq_data.MAPQ_DEFAULT)
    rp, hp = mm2chain.RegPlan(n_reads, n_u, n_b), mm2chain.HitPlan(n_reads, n_u)
    mp, ep = mm2chain.MapqPlan(n_reads, n_u, n_b), mm2chain.EstErrPlan(n_reads, n_u, n_b, n_m)
    try:
        regs = rp.run(u_off, u, b_off, b, d_q, d_h)
        hits, n_hits = hp.run(params.hit_opts(**ho), u_off, regs)
        fin, n_out, b_out, n_b_out = mp.run(params.mapq_opts(**mo), u_off, hits, n_hits, b_off, b, d_q, d_rep, anchors=True)
        err, avg = ep.run(u_off, fin, n_out, b_off, b_out, d_mo, d_mp, d_q, d_rl)      # nothing has come back to the host yet
        rp.check(); hp.check(); mp.check(); ep.check()
        uo, got, no = rc["u_off"], fin.cpu().numpy(), n_out.cpu().numpy()
        ge, ga = err.cpu().numpy(), avg.cpu().numpy()
        n_regions = n_rev = n_unmatched = 0
        for r in range(n_reads):
            ur, br, rep_len, mini = cpu[r]
            h = hits_model.select_hits(regs_model.gen_regs(int(hash_[r]), int(qlen[r]), ur, br), ho)
            want, wa, _ = mapq_model.join_mapq(h, br, int(qlen[r]), mo, rep_len)
            cn, ak = M.counts(want, wa, mini, int(qlen[r]), ref_len)
            assert no[r] == want.size and np.array_equal(ge[uo[r]:uo[r] + no[r]], cn), f"read {r}: counts {ge[uo[r]:uo[r] + no[r]].tolist()}, the model {cn.tolist()}"
            assert ga[r].tobytes() == np.float32(ak).tobytes(), f"read {r}: avg_k {ga[r]!r}, the model {ak!r}"
            g = got[uo[r]:uo[r] + no[r]].reshape(-1).view(M.REG).copy()
            mm2chain.est_err_apply([0], [g.size], ge[uo[r]:uo[r] + no[r]].copy(), ga[r:r + 1], g)
            assert g.tobytes() == M.est_err(want, wa, mini, int(qlen[r]), ref_len).tobytes(), f"read {r}: the final regions differ from the models on the oracle's chains"
            # a chain anchor of a real read is one of its minimizers and the positions of a chain increase: every walk runs to its end, and what div measures is
            # the minimizers of the read between the anchors that matched nothing (the substitutions)
            assert (cn[:, 0] == want["cnt"]).all(), f"read {r}: a walk of a real read stopped early: {cn.tolist()} of {want['cnt'].tolist()}"
            n_regions += want.size
            n_unmatched += int((cn[:, 1] - cn[:, 0] > 2).sum())
            n_rev += int(((want["flags"] >> 10) & 1).sum())
        assert n_regions > n_reads and 0 < n_rev < n_regions, "more than one region in some read, both strands"
        # 4 % substitutions over 2 000 bases and more destroy dozens of a read's minimizers, which then lie unmatched between the anchors of its region; the second
        # piece of a two-piece read is an exact copy of the reference and has none
        assert n_unmatched >= n_reads, "the region of every substituted piece has unmatched minimizers between its anchors: n_tot - n_match beyond the two flanks"
        print(f"{n_reads} reads, {n_regions} final regions ({n_rev} reverse), {n_m} minimizers")
    finally:
        ep.close(); mp.close(); hp.close(); rp.close()


def test_refusals_are_reported_and_the_neighbours_stay_exact(ref):
    """a read whose u_off / b_off / mini_off / n_in leave the capacities or each other, whose mini_pos does not increase strictly, or with a region that leaves the
    read's anchors or the reference sequences touches nothing and makes check() an argument error with the count; the reads beside it are exact (err_walk then goes
    read by read); guard rows in front of the outputs and behind the capacities stay untouched"""
    import mm2chain
    names = ("both_strands", "middle_absent_extras", "joined", "two_rids")
    rs = [next(R for R in ref if R["name"] == n) for n in names]
    B0 = _batch(rs)
    cap_u, cap_b, cap_m, n_ref = int(B0["u_off"][-1]), int(B0["b_off"][-1]), int(B0["mini_off"][-1]), B0["ref_len"].size
    plan = mm2chain.EstErrPlan(4, cap_u, cap_b, cap_m)

    def broken(**kw):
        B = {k: v.copy() for k, v in B0.items()}
        for key, (at, val) in kw.items():
            B[key][at] = val
        return B

    def region(k, **fields):
        B = broken()
        g = B["regs"][B0["u_off"][k]:B0["u_off"][k] + 1].reshape(-1).view(M.REG)
        for f, v in fields.items():
            g[f] = v
        return B
    m1 = int(B0["mini_off"][1])
    pats = {"u_off beyond the capacity": (broken(u_off=(slice(2, 5), cap_u + 5)), [1, 2, 3]), "u_off descending": (broken(u_off=(4, B0["u_off"][3] - 1)), [3]),
            "u_off negative": (broken(u_off=(0, -4)), [0]), "b_off negative": (broken(b_off=(0, -2)), [0]), "mini_off negative": (broken(mini_off=(0, -1)), [0]),
            "b_off beyond the capacity": (broken(b_off=(slice(2, 5), cap_b + 9)), [1, 2, 3]),
            "b_off descending": (broken(b_off=(4, B0["b_off"][3] - 1)), [3]), "mini_off beyond the capacity": (broken(mini_off=(slice(3, 5), cap_m + 1)), [2, 3]),
            "mini_off descending": (broken(mini_off=(4, B0["mini_off"][3] - 1)), [3]), "n_in beyond its room": (broken(n_in=(1, rs[1]["in"].size + 2)), [1]),
            "n_in negative": (broken(n_in=(2, -1)), [2]),
            "mini_pos with a repeated position": (broken(mini_pos=(m1 + 3, B0["mini_pos"][m1 + 2])), [1]),
            "mini_pos decreasing": (broken(mini_pos=(m1 + 3, B0["mini_pos"][m1 + 1])), [1]),
            "mini_pos decreasing at its end": (broken(mini_pos=(int(B0["mini_off"][3]) - 1, 3)), [2]),
            "a region beyond the read's anchors": (region(1, cnt=rs[1]["a"].shape[0] + 1), [1]), "a region with a negative as": (region(0, **{"as": -1}), [0]),
            "a region with a negative cnt": (region(2, cnt=-3), [2]), "rid at n_ref": (region(3, rid=n_ref), [3]), "rid negative": (region(1, rid=-1), [1])}
    try:
        for what, (B, bad) in pats.items():
            err, avg = got = _run(plan, B, guard=3)
            rc, n_refused = plan.refused()
            assert (rc, n_refused) == (-2, len(bad)), f"{what}: check() = {rc}, {n_refused} refused"
            with pytest.raises(mm2chain.Mm2cError, match="code -2"):
                plan.check()
            for k in range(4):
                if k in bad:
                    lo, hi = (int(B0["u_off"][k]), int(B0["u_off"][k + 1]))
                    assert (err[lo:hi] == ERR_FILL).all() and avg[k] == AVG_FILL, f"{what}: the refused read {k} wrote"
                else:
                    _assert_read(got, B, k, rs[k], what)
            assert (err[cap_u:] == ERR_FILL).all() and (avg[4:] == AVG_FILL).all(), f"{what}: guard rows were written"
        got = _run(plan, B0, guard=3)                                            # the same plan on sound data afterwards
        assert plan.refused() == (0, 0)
        for k in range(4):
            _assert_read(got, B0, k, rs[k], "sound data behind the broken ones")
        assert (got[0][cap_u:] == ERR_FILL).all() and (got[1][4:] == AVG_FILL).all()
        for k in range(4):                                                      # rows behind n_in but inside the read's room are not written either
            assert (got[0][int(B0["u_off"][k]) + rs[k]["in"].size:int(B0["u_off"][k + 1])] == ERR_FILL).all()
    finally:
        plan.close()


def test_a_plan_run_again_on_other_data_in_another_order_and_of_another_size(ref):
    import mm2chain
    small = [R for R in ref if R["a"].shape[0] < 1000]
    first, second = small[:len(small) // 2], small[len(small) // 2:][::-1]
    big = [R for R in ref if R["name"] in ("slice_missing_at4096", "regions129", "libm_3001")]
    groups = (first, second, first[::-1], big, second[::3], big[::-1] + first[:5])
    n_reads = max(len(g) for g in groups)
    plan = mm2chain.EstErrPlan(n_reads, *_caps(groups))
    try:
        for g in groups:
            B = _batch(g, n_reads)
            got = _run(plan, B)
            plan.check()
            for k, R in enumerate(g):
                _assert_read(got, B, k, R, "a plan run again")
    finally:
        plan.close()
