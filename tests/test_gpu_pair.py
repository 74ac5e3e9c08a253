"""The two ends of a fragment paired on the device (csrc/pair_ends.hip).  Every case of tests/pair_data.py and every simulated pair of
tests/golden/ref_pair.npz through one PairPlan three ways -- one batch per option set, one fragment per call, and pair_ends_batch -- byte for byte against what the
reference's own pe.o made of it, with and without the flip of map.c:455-466 (the flip turned by hand on the reference's bytes); refusals beside exact neighbours,
the table's end, the 128 / 129 boundary, a plan run again on other data, and the chain FinPlan.run -> PairPlan.run in device memory on the simulated pairs."""
import numpy as np
import pytest
import torch

import fin_model as FM
import pair_data as D
import pair_model as M

pytestmark = pytest.mark.gpu
FILL = 0xee
ROOM = 1                                                                       # rows a segment read's room holds beyond its regions
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def fx():
    """(cases: name -> (case, what the plan must give without the flip: [mate 0, mate 1], or None for a refused fragment), simulated pairs as cases likewise)"""
    planted, real, _ = D.fixture()
    W = {}
    for c in D.cases():
        if c["refuse"]:
            W[c["name"]] = (c, None)
        elif "max_log_arg" in c:                                               # the table's end: the model, which is the reference but for the winners' mapq (CPU tests)
            W[c["name"]] = (c, list(M.pair_case(c)[:2]))
        else:
            W[c["name"]] = (c, planted[c["name"]]["out"])
    R = []
    for d in real:
        c = D.real_case(d)
        out1 = d["out"][1][0].copy()
        out1["p"] = c["regs"][1]["p"]
        R.append((c, [d["out"][0][0], out1]))
    return W, R, real


def _opt(o, **over):
    from mm2chain import params
    return params.pair_opts(**dict(o, **over))


def flipped(want, qlens, pe_ori):
    """map.c:455-466 by hand on the expected regions"""
    out = []
    for j, r in enumerate(want):
        r = r.copy()
        if (j == 0 and pe_ori >> 1 & 1) or (j == 1 and pe_ori & 1):
            qs, qe = r["qs"].copy(), r["qe"].copy()
            r["qs"], r["qe"] = qlens[j] - qe, qlens[j] - qs
            r["flags"] ^= np.uint32(1 << 10)
        out.append(r)
    return out


def groups(cs):
    G = {}
    for c in cs:
        G.setdefault(tuple(c["opt"][k] for k in M.OPT_FIELDS) + (c.get("max_log_arg"),), []).append(c)
    return [(g[0]["opt"], g) for g in G.values()]


def _batch(cs, n_frags):
    """the fragments one after another, every segment read in room for ROOM rows more than it has regions; p shifted to the batch's records"""
    rooms = [r.size + ROOM for c in cs for r in c["regs"]] + [0, 0] * (n_frags - len(cs))
    f_off = np.concatenate([[0], np.cumsum(rooms)]).astype(np.int64)
    regs = np.full(max(int(f_off[-1]), 1) * 80, FILL, np.uint8).view(M.REG)
    pext, p_off = [], []
    for k, c in enumerate(cs):
        p_off.append(sum(x.size for x in pext))
        for s in range(2):
            r = c["regs"][s].copy()
            r["p"][r["p"] != 0] += np.uint64(p_off[-1])
            regs[f_off[2 * k + s]:f_off[2 * k + s] + r.size] = r
        pext.append(c["pext"])
    pad = lambda v, fill, m: np.array(v + [fill] * (m * (n_frags - len(cs))), np.int32)
    return dict(f_off=f_off, regs=regs, pext=np.concatenate(pext + [np.zeros(0, M.PEXT)]), p_off=p_off, n=pad([r.size for c in cs for r in c["regs"]], 0, 2),
                seg_len=pad([q for c in cs for q in c["qlens"]], 150, 2), gap=pad([c["opt"]["max_gap_ref"] if c["gap"] is None else c["gap"] for c in cs], 500, 1))


def _run(plan, opt, B, guard=3, gap=True):
    regs = np.full((max(plan.n_u_cap, 1) + guard) * 80, FILL, np.uint8)
    nb = min(plan.n_u_cap * 80, B["regs"].size * 80)
    regs[:nb] = B["regs"].view(np.uint8)[:nb]
    px = np.zeros(max(plan.n_pext_cap, 1), M.PEXT); px[:B["pext"].size] = B["pext"]
    d_regs, d_px = t(regs.reshape(-1, 80)), t(px.view(np.uint8))
    status = torch.full((plan.n_frags + guard,), -9, dtype=torch.int32, device="cuda")
    plan.run(opt, t(B["f_off"]), d_regs, t(B["n"]), d_px, t(B["seg_len"]), gap_ref=t(B["gap"]) if gap else None, status=status)
    torch.cuda.synchronize()
    assert d_px.cpu().numpy().tobytes() == px.tobytes(), "the p records were written"
    r_h, s_h = d_regs.cpu().numpy(), status.cpu().numpy()
    assert (r_h[max(plan.n_u_cap, 1):] == FILL).all() and (s_h[plan.n_frags:] == -9).all(), "rows behind the capacities were written"
    return r_h.reshape(-1).view(M.REG), s_h


def _assert_frag(got, B, k, c, w, what, untouched=-9):
    regs, status = got
    for s in range(2):
        room = regs[B["f_off"][2 * k + s]:B["f_off"][2 * k + s + 1]]
        n = c["regs"][s].size
        assert (room[n:].view(np.uint8) == FILL).all(), f"{what}: {c['name']}: rows behind mate {s}'s regions were written"
        g = room[:n].copy()
        g["p"][g["p"] != 0] -= np.uint64(B["p_off"][k])
        want = c["regs"][s] if w is None else w[s]                             # refused: nothing of the fragment is written
        bad = [i for i in range(n) if g[i].tobytes() != want[i].tobytes()]
        assert not bad, f"{what}: {c['name']}: mate {s}: {len(bad)} of {n} regions differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {want[bad[0]]}"
    assert status[k] == (1 if w is None else 0), f"{what}: {c['name']}: status {status[k]}"


def _caps(G):
    return (max(len(cs) for _, cs in G), max(sum(r.size + ROOM for c in cs for r in c["regs"]) for _, cs in G), max(sum(c["pext"].size for c in cs) for _, cs in G))


def _proper(w):
    return int(w is not None and bool((w[0]["flags"] >> 13 & 1).any()))


def test_every_case_three_ways_through_one_plan(fx):
    import mm2chain
    W, R, _ = fx
    cs_all = [c for c, _ in W.values() if "max_log_arg" not in c] + [c for c, _ in R]
    want = {id(c): w for c, w in list(W.values()) + R}
    G = groups(cs_all)
    n_frags, n_u, n_p = _caps(G)
    plan = mm2chain.PairPlan(n_frags, n_u, n_p, max_log_arg=D.MAX_LOG_ARG)
    try:
        for o, cs in G:
            B = _batch(cs, n_frags)
            for over in (dict(flip=0), dict(flip=1, pe_ori=3), dict(flip=1, pe_ori=1)):
                exp = lambda c: None if want[id(c)] is None else want[id(c)] if not over["flip"] else flipped(want[id(c)], c["qlens"], over["pe_ori"])
                got = _run(plan, _opt(o, **over), B)
                rc, refused, beyond, proper = plan.counts()
                for k, c in enumerate(cs):
                    _assert_frag(got, B, k, c, exp(c), f"one batch {over}")
                assert (got[1][len(cs):n_frags] == 0).all()
                n_ref = sum(want[id(c)] is None for c in cs)
                assert (refused, beyond, proper) == (n_ref, 0, sum(_proper(want[id(c)]) for c in cs)), (o, plan.counts())
                assert rc == (-2 if n_ref else 0)
            for c in [c for c in cs if c["name"] != "real"] + [c for c in cs if c["name"] == "real"][::9]:   # one fragment per call (of the simulated pairs every ninth)
                B1 = _batch([c], n_frags)
                _assert_frag(_run(plan, _opt(o), B1), B1, 0, c, want[id(c)], "one fragment per call")
            m = len(cs)
            H = mm2chain.pair_ends_batch(_opt(o), B["f_off"][:2 * m + 1], B["regs"], B["n"][:2 * m], B["pext"], B["seg_len"][:2 * m], gap_ref=B["gap"][:m],
                                         max_log_arg=D.MAX_LOG_ARG, fill=FILL)
            assert H["rc"] == (-2 if any(want[id(c)] is None for c in cs) else 0)
            for k, c in enumerate(cs):
                _assert_frag((H["regs"], H["status"]), B, k, c, want[id(c)], "pair_ends_batch")
        assert plan.last_ms() > 0
    finally:
        plan.close()


def test_scalar_gap_when_no_array_is_given(fx):
    import mm2chain
    W, _, _ = fx
    cs = [W[n][0] for n in ("gap_eq", "gap_plus1", "single_floor2")]
    plan = mm2chain.PairPlan(3, 16, 16, max_log_arg=64)
    try:
        B = _batch(cs, 3)
        got = _run(plan, _opt(cs[0]["opt"]), B, gap=False)
        for k, c in enumerate(cs):
            _assert_frag(got, B, k, c, W[c["name"]][1], "scalar gap")
        got = _run(plan, _opt(cs[0]["opt"], max_gap_ref=501), B, gap=False)      # one more: gap_plus1 pairs as gap_per_fragment does
        assert (got[0][B["f_off"][2]]["flags"] >> 13 & 1) == 1 and plan.check() == 3
    finally:
        plan.close()


def test_beyond_the_table(fx):
    """n_sub = 10 with a table that ends at 8: both winners' mapq as they came in, the rest of the fragment done, counted, MM2C_E_TOOBIG; its neighbours exact"""
    import mm2chain
    W, _, _ = fx
    c, w = W["n_sub_beyond_table"]
    nb = [W["single_floor2"][0], c, W["alt_lowers"][0]]
    plan = mm2chain.PairPlan(3, 32, 32, max_log_arg=c["max_log_arg"])
    try:
        for o, cs in groups(nb):
            B = _batch(cs, 3)
            got = _run(plan, _opt(o), B)
            for k, x in enumerate(cs):
                _assert_frag(got, B, k, x, W[x["name"]][1], "beyond the table")
            rc, refused, beyond, proper = plan.counts()
            assert (rc, refused, beyond, proper) == ((-3, 0, 1, 1) if any(x is c for x in cs) else (0, 0, 0, len(cs)))
        with pytest.raises(mm2chain.Mm2cError):
            B = _batch([c], 3)
            _run(plan, _opt(c["opt"]), B)
            plan.check()
        H = mm2chain.pair_ends_batch(_opt(c["opt"]), B["f_off"][:3], B["regs"], B["n"][:2], B["pext"], B["seg_len"][:2], max_log_arg=c["max_log_arg"])
        assert H["rc"] == -3
        _assert_frag((H["regs"], H["status"]), B, 0, c, w, "pair_ends_batch beyond the table")
    finally:
        plan.close()


def test_refused_offsets_and_counts_leave_neighbours_exact(fx):
    """every per-region refusal is a case of pair_data (test_every_case...); here: offsets or counts that leave the capacities or each other"""
    import mm2chain
    W, _, _ = fx
    cs = [W[n][0] for n in ("lift_mate0", "blend_raises", "alt_lowers")]
    o = cs[0]["opt"]
    B0 = _batch(cs, 3)
    n_u = int(B0["f_off"][-1])

    def run(edit, cap=n_u, bad=(1,)):
        B = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in B0.items()}
        edit(B)
        plan = mm2chain.PairPlan(3, cap, 16, max_log_arg=64)
        try:
            outs = {}
            for k, c in enumerate(cs):
                outs[k] = W[c["name"]][1] if c["opt"] == o else list(M.pair(c["regs"][0], c["regs"][1], c["pext"], c["qlens"], o)[:2])
            regs, status = _run(plan, _opt(o), B)
            rc, refused, _, _ = plan.counts()
            assert rc == -2 and refused == len(bad)
            for k, c in enumerate(cs):
                if k in bad:
                    assert status[k] == 1
                    lo, hi = int(B0["f_off"][2 * k]), int(B0["f_off"][2 * k + 2])
                    assert regs[lo:min(hi, cap)].tobytes() == B0["regs"][lo:min(hi, cap)].tobytes(), "a refused fragment was written"
                else:
                    _assert_frag((regs, status), B0, k, c, outs[k], "beside a refused fragment")
        finally:
            plan.close()

    def count_over_room(B): B["n"][3] = B0["f_off"][4] - B0["f_off"][3] + 1
    def count_negative(B): B["n"][2] = -1
    def middle_backwards(B): B["f_off"][3] = B0["f_off"][2] - 1
    for edit in (count_over_room, count_negative, middle_backwards):
        run(edit)
    run(lambda B: None, cap=n_u - 1, bad=(2,))                                 # the last fragment's room leaves the capacity by one row

    def first_negative(B): B["f_off"][0] = -1
    run(first_negative, bad=(0,))


def test_lds_and_scratch_give_the_same_answer(fx):
    """128 regions in all stay in LDS, 129 go through the plan's scratch: mixed_64_64 as it is, and with one more region of mate 1 on a reference of its own, which
    pairs with nothing; alternate_128 / alternate_129 (the replayed sort on either side) are cases of the first test"""
    import mm2chain
    W, _, _ = fx
    c, w = W["mixed_64_64"]
    extra = np.zeros(1, M.REG)
    extra[0] = c["regs"][1][0]
    extra["id"], extra["parent"], extra["rid"], extra["flags"] = 64, 0, 9, 1 << 16
    c2 = dict(c, name="mixed_64_65", regs=[c["regs"][0], np.concatenate([c["regs"][1], extra])])
    m = M.pair_case(c2)[:2]
    assert m[0].tobytes() == w[0].tobytes() and m[1][:64].tobytes() == w[1].tobytes()      # (the added region is a child of region 0 and follows its lift)
    plan = mm2chain.PairPlan(2, 300, 300, max_log_arg=D.MAX_LOG_ARG)
    try:
        B = _batch([c, c2], 2)
        got = _run(plan, _opt(c["opt"]), B)
        _assert_frag(got, B, 0, c, w, "128 in LDS")
        _assert_frag(got, B, 1, c2, list(m), "129 in scratch")
    finally:
        plan.close()


def test_plan_runs_again_on_other_data(fx):
    import mm2chain
    W, R, _ = fx
    a = [W[n][0] for n in ("alternate_132", "lift_both", "mixed_60_69")]
    a = [c for c in a if c["opt"] == a[0]["opt"]] + [R[0][0]]
    b = [c for c, _ in R[5:40]]
    want = {id(c): w for c, w in list(W.values()) + R}
    plan = mm2chain.PairPlan(40, 600, 600, max_log_arg=D.MAX_LOG_ARG)
    try:
        for cs in (a, b, a):
            for o, g in groups(cs):
                B = _batch(g, 40)
                got = _run(plan, _opt(o), B)
                for k, c in enumerate(g):
                    _assert_frag(got, B, k, c, want[id(c)], "run again")
    finally:
        plan.close()


def test_chain_finplan_then_pairplan_in_device_memory(fx):
    """the recorded lists of mm_align_skeleton in front of mm_filter_regs, both mates as segment reads 2f and 2f + 1, through FinPlan.run; PairPlan.run on its
    outputs as they lie in device memory; the end is the reference's lists behind mm_pair, and behind the flip turned by hand"""
    import mm2chain
    from mm2chain import params
    _, _, real = fx
    F = len(real)
    sizes = [d["pre"][s][0].size for d in real for s in range(2)]
    f_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    regs = np.zeros(max(int(f_off[-1]), 1), M.REG)
    pext, p_base = [], []
    for f, d in enumerate(real):
        for s in range(2):
            r, px = d["pre"][s]
            r = r.copy()
            p_base.append(sum(x.size for x in pext))
            r["p"][r["p"] != 0] += np.uint64(p_base[-1])
            regs[f_off[2 * f + s]:f_off[2 * f + s + 1]] = r
            pext.append(px)
    pext = np.concatenate(pext)
    qlen = np.array([q for d in real for q in d["qlens"]], np.int32)
    rep = np.array([d["rep_len"] for d in real for _ in range(2)], np.int32)
    gap = np.array([d["gap"] for d in real], np.int32)
    fin = mm2chain.FinPlan(2 * F, int(f_off[-1]), pext.size, max_log_arg=1 << 16, match_sc=2)
    pair = mm2chain.PairPlan(F, int(f_off[-1]), pext.size, max_log_arg=D.MAX_LOG_ARG)
    try:
        d_off, d_px, d_q = t(f_off), t(pext.view(np.uint8).reshape(-1, 32)), t(qlen)
        for over in (dict(flip=0), dict(flip=1)):
            d_px = t(pext.view(np.uint8).reshape(-1, 32))
            out, n_out = fin.run(params.fin_opts("sr"), d_off, t(regs.view(np.uint8).reshape(-1, 80)), t(np.array(sizes, np.int32)), d_px, d_q, t(rep))
            status = pair.run(params.pair_opts("sr", **over), d_off, out, n_out, d_px, d_q, gap_ref=t(gap))
            torch.cuda.synchronize()
            assert fin.check() >= 0 and pair.check() == sum(bool(k & {"real_one_candidate", "real_several_candidates"}) for k in (d["kinds"] for d in real))
            assert not status.cpu().numpy().any()
            o_h, n_h, px_h = out.cpu().numpy().reshape(-1).view(M.REG), n_out.cpu().numpy(), d_px.cpu().numpy().reshape(-1).view(FM.PEXT)
            for f, d in enumerate(real):
                want = [d["out"][0][0], d["out"][1][0]]
                if over["flip"]:
                    want = flipped(want, d["qlens"], 1)
                for s in range(2):
                    w, wpx = want[s].copy(), d["out"][s][1]
                    assert n_h[2 * f + s] == w.size, f"pair {f} mate {s}: {n_h[2 * f + s]} regions, want {w.size}"
                    g = o_h[f_off[2 * f + s]:f_off[2 * f + s] + w.size].copy()
                    if w.size:
                        assert px_h[g["p"].astype(np.int64) - 1].tobytes() == wpx[w["p"].astype(np.int64) - 1].tobytes(), f"pair {f} mate {s}: the p records differ"
                    g["p"] = w["p"] = 0
                    assert g.tobytes() == w.tobytes(), f"pair {f} mate {s} differs"
    finally:
        fin.close(); pair.close()
