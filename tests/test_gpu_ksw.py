"""Base alignment on the device (csrc/ksw_extd2.hip: ksw_extd2_sse, ksw2_extd2_sse.c): every case of tests/ksw_data.py through KswPlan.run and ksw_extd2_batch, equal
in every field and CIGAR word to what the reference's own ksw2_extd2_sse.o made of it (tests/golden/ref_ksw.npz) -- in one batch per score set, in reverse order
through the same plan, one task per call, and through the host entry; guard rows around the results and the CIGAR words, and fill behind every CIGAR; each kind of
refusal and both kinds of too-big with exact neighbours; a plan run again on other data of another size; a run on the caller's stream behind another plan's kernel.
The size classes of the kernel (ksw_data.limits): the array image in LDS up to 2 304 padded target and 2 304 query bases and in scratch beyond, padded rows of 64 / 80 /
144 cells (one chunk of 64 lanes and the first widths beyond one and two), and the 2 000 x 2 100 task at w = 500."""
import os

import numpy as np
import pytest
import torch

import ksw_data as D

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL, GUARD, SLACK = 0x5e5e5e5e, 3, 2
EZ = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "n_cigar", "reach_end")
SCRATCH = 256 << 22                                                              # 256 slots of 4 MiB


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def ref():
    path = os.path.join(GOLDEN, "ref_ksw.npz")
    assert os.path.exists(path), "tests/golden/ref_ksw.npz is absent"
    fx = np.load(path)
    cs = D.cases()
    assert [c["name"] for c in cs] == list(fx["names"])
    ez, off, cig = fx["ez"], fx["cig_off"], fx["cigar"]
    out = []
    for k, c in enumerate(cs):
        out.append(dict(case=c, ez=ez[k], cigar=cig[off[k]:off[k + 1]]))
    return out


def need_of(rs):
    """the scratch slot the largest of the tasks takes"""
    from mm2chain import ksw_task_scratch
    return max(ksw_task_scratch(r["case"]["q"].size, r["case"]["t"].size, r["case"]["w"], r["case"]["flag"]) for r in rs)


def by_score(rs):
    g = {}
    for r in rs:
        g.setdefault(r["case"]["sc"], []).append(r)
    return g


def pack(rs, slack=SLACK, room=None):
    """-> (tasks, seq, cig_off): the sequences one after another in one pool, a CIGAR slot of the expected length plus `slack` words (or room[k])"""
    from mm2chain import KSW_TASK_DTYPE
    tk = np.zeros(len(rs), KSW_TASK_DTYPE)
    seqs, at, co = [], 0, [0]
    for k, r in enumerate(rs):
        c = r["case"]
        tk[k] = (at, at + c["q"].size, c["q"].size, c["t"].size, c["w"], c["zdrop"], c["end_bonus"], c["flag"])
        seqs += [c["q"], c["t"]]; at += c["q"].size + c["t"].size
        co.append(co[-1] + (r["cigar"].size + slack if room is None else room[k]))
    return tk, np.concatenate(seqs).astype(np.uint8), np.array(co, np.int64)


def t(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    return torch.from_numpy(a).cuda()


def guarded(n, width, dtype, fill):
    shape = (n + 2 * GUARD, width) if width else (n + 2 * GUARD,)
    whole = torch.full(shape, fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def check_out(rs, res, cigar, co, skip=()):
    """every field and CIGAR word of the tasks not in `skip`, status 0, and the fill behind each CIGAR"""
    from mm2chain import KSW_RES_DTYPE
    res = res.view(KSW_RES_DTYPE).reshape(-1)
    fill = np.uint32(FILL)
    for k, r in enumerate(rs):
        if k in skip:
            continue
        got = np.array([int(res[f][k]) for f in EZ], np.int64)
        assert np.array_equal(got, r["ez"].astype(np.int64)) and res["status"][k] == 0, (r["case"]["name"], got, r["ez"], res["status"][k])
        n = r["cigar"].size
        assert np.array_equal(cigar[co[k]:co[k] + n], r["cigar"]), (r["case"]["name"], cigar[co[k]:co[k] + n], r["cigar"])
        assert (cigar[co[k] + n:co[k + 1]] == fill).all(), r["case"]["name"]


def run_plan(plan, sc, rs, tk, seq, co, stream=None):
    """-> (res, cigar) on the host, guard rows checked"""
    from mm2chain import KSW_RES_DTYPE
    n = len(rs)
    rw, rv = guarded(n, KSW_RES_DTYPE.itemsize, torch.uint8, 0xee)
    cw, cv = guarded(plan.cigar_cap, 0, torch.int32, FILL)
    plan.run(D.score_set(sc), n, t(tk), _pad(t(seq), plan.seq_cap), t(co), rv, cv, stream=stream)
    return plan, rw, rv, cw, cv


def _pad(x, n):
    if x.numel() >= n:
        return x
    return torch.cat([x, torch.zeros(n - x.numel(), dtype=x.dtype, device=x.device)])


def guards_ok(rw, cw):
    r, c = rw.cpu().numpy(), cw.cpu().numpy().view(np.uint32)
    return (r[:GUARD] == 0xee).all() and (r[-GUARD:] == 0xee).all() and (c[:GUARD] == FILL).all() and (c[-GUARD:] == FILL).all()


def test_every_case_in_batches_both_orders(ref):
    from mm2chain import KswPlan
    for sc, rs in by_score(ref).items():
        plan = None
        for order in (rs, rs[::-1]):
            tk, seq, co = pack(order)
            if plan is None:
                plan = KswPlan(len(order), seq.size, int(co[-1]), n_slots=256, slot_bytes=need_of(order))
            _, rw, rv, cw, cv = run_plan(plan, sc, order, tk, seq, co)
            plan.check()
            check_out(order, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), co)
            assert guards_ok(rw, cw)
        assert plan.last_ms() > 0 and plan.last_kernel_ms()[0] > 0
        plan.close()


def test_one_task_per_call(ref):
    from mm2chain import KswPlan, KSW_RES_DTYPE, KSW_TASK_DTYPE
    for sc, rs in by_score(ref).items():
        tk, seq, co = pack(rs)
        plan = KswPlan(1, seq.size, int(co[-1]), n_slots=2, slot_bytes=need_of(rs))
        assert plan.n_slots == 2
        d_tk, d_seq, d_co = t(tk).reshape(-1, KSW_TASK_DTYPE.itemsize), t(seq), t(co)
        rw, rv = guarded(len(rs), KSW_RES_DTYPE.itemsize, torch.uint8, 0xee)
        cw, cv = guarded(plan.cigar_cap, 0, torch.int32, FILL)
        score = D.score_set(sc)
        for k in range(len(rs)):
            plan.run(score, 1, d_tk[k:], d_seq, d_co[k:], rv[k:], cv)
        plan.check()
        check_out(rs, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), co)
        assert guards_ok(rw, cw)
        plan.close()


def test_host_entry(ref):
    from mm2chain import ksw_extd2_batch, KSW_RES_DTYPE
    for sc, rs in by_score(ref).items():
        tk, seq, co = pack(rs)
        res = np.zeros(len(rs), KSW_RES_DTYPE); cigar = np.full(int(co[-1]), FILL, np.uint32)
        ksw_extd2_batch(D.score_set(sc), tk, seq, co, res=res, cigar=cigar)
        check_out(rs, res, cigar, co)


def _some(ref, n=40, sc="ont"):
    rs = [r for r in ref if r["case"]["sc"] == sc and r["case"]["name"].startswith(("ins60/", "zdrop_20_off/", "w_3/", "extz_clip_eb10/"))]
    return rs[::max(1, len(rs) // n)][:n]


def test_refusals_leave_neighbours_exact(ref):
    """a flag outside MM2C_KSW_FLAGS (GENERIC_SC, a splice bit), offsets in front of and behind the pool, a length that leaves it, a length above MM2C_KSW_MAX_LEN,
    a CIGAR slot that runs backwards and one behind cigar_cap: status 1 and nothing else of theirs written, counted, MM2C_E_ARG, the tasks beside them exact;
    lengths <= 0 leave the reset ez"""
    from mm2chain import KswPlan, KSW_RES_DTYPE, KSW_REFUSED, Mm2cError
    rs = _some(ref)
    tk, seq, co = pack(rs)
    co = co.copy()
    bad = {1: ("flag", 0x04), 3: ("flag", 0x100), 5: ("q_off", -1), 7: ("t_off", seq.size), 9: ("qlen", seq.size + 1), 11: ("tlen", (1 << 20) + 1), 13: ("q_off", 1 << 40)}
    for k, (f, v) in bad.items():
        tk[f][k] = v
    empty = {15: ("qlen", 0), 17: ("tlen", -3)}
    for k, (f, v) in empty.items():
        tk[f][k] = v
    plan = KswPlan(len(rs), seq.size, int(co[-1]), SCRATCH)
    _, rw, rv, cw, cv = run_plan(plan, "ont", rs, tk, seq, co)
    rc, n_ref, n_big = plan.counts()
    refused = set(bad)
    assert rc == -2 and n_ref == len(refused) and n_big == 0
    with pytest.raises(Mm2cError):
        plan.check()
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    r = res.view(KSW_RES_DTYPE).reshape(-1)
    for k in refused:
        assert r["status"][k] == KSW_REFUSED and (res[k, :44] == 0xee).all()
        assert (cig[co[k]:co[k + 1]] == np.uint32(FILL)).all()
    for k in empty:
        assert [int(r[f][k]) for f in EZ] == [0, 0, -1, -1, -0x40000000, -1, -0x40000000, -1, -0x40000000, 0, 0] and r["status"][k] == 0
        assert (cig[co[k]:co[k + 1]] == np.uint32(FILL)).all()
    check_out(rs, res, cig, co, skip=refused | set(empty))
    assert guards_ok(rw, cw)
    # a slot behind cigar_cap
    plan2 = KswPlan(len(rs), seq.size, int(co[-2]), SCRATCH)
    _, rw, rv, cw, cv = run_plan(plan2, "ont", rs, pack(rs)[0], seq, co)
    rc, n_ref, n_big = plan2.counts()
    assert rc == -2 and n_ref == 1
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    assert res.view(KSW_RES_DTYPE).reshape(-1)["status"][-1] == KSW_REFUSED
    check_out(rs[:-1], res, cig, co[:-1])
    assert guards_ok(rw, cw)
    # a slot that runs backwards: [0, 40) for task 0, (40, 20) for task 1, [20, 60) for task 2
    three = [r for r in rs if r["cigar"].size <= 20][:3]
    tk3, seq3, _ = pack(three)
    co3 = np.array([0, 40, 20, 60], np.int64)
    plan3 = KswPlan(3, seq3.size, 60, SCRATCH)
    _, rw, rv, cw, cv = run_plan(plan3, "ont", three, tk3, seq3, co3)
    rc, n_ref, n_big = plan3.counts()
    assert rc == -2 and n_ref == 1 and n_big == 0
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    assert res.view(KSW_RES_DTYPE).reshape(-1)["status"][1] == KSW_REFUSED and (res[1, :44] == 0xee).all()
    n0, n2 = three[0]["cigar"].size, three[2]["cigar"].size
    assert np.array_equal(cig[:n0], three[0]["cigar"]) and (cig[n0:20] == np.uint32(FILL)).all() and np.array_equal(cig[20:20 + n2], three[2]["cigar"])
    assert (cig[20 + n2:60] == np.uint32(FILL)).all() and guards_ok(rw, cw)
    plan.close(); plan2.close(); plan3.close()


def test_too_big_for_the_scratch_and_cigar_cut(ref):
    """a task whose p does not fit its scratch slot is not run (status 2); a CIGAR longer than its slot is cut (status 3): the words that fit, every scalar exact,
    nothing behind the slot; MM2C_E_TOOBIG; the tasks beside them exact"""
    from mm2chain import KswPlan, KSW_RES_DTYPE, KSW_TOO_BIG, KSW_CIGAR_CUT, ksw_task_scratch
    rs = _some(ref)
    big = next(r for r in ref if r["case"]["name"] == "len_257/f00")
    rs = rs[:6] + [big] + rs[6:]
    room = [r["cigar"].size + SLACK for r in rs]
    cut = [k for k, r in enumerate(rs) if r["cigar"].size >= 3 and k != 6][:2]
    room[cut[0]] = rs[cut[0]]["cigar"].size - 1
    room[cut[1]] = 0
    tk, seq, co = pack(rs, room=room)
    need = [ksw_task_scratch(r["case"]["q"].size, r["case"]["t"].size, r["case"]["w"], r["case"]["flag"]) for r in rs]
    slot = max(n for k, n in enumerate(need) if k != 6) + 256
    assert need[6] > slot
    plan = KswPlan(len(rs), seq.size, int(co[-1]), slot)
    assert plan.n_slots == 1 and plan.slot_bytes < need[6] and plan.slot_bytes >= max(n for k, n in enumerate(need) if k != 6)
    _, rw, rv, cw, cv = run_plan(plan, "ont", rs, tk, seq, co)
    rc, n_ref, n_big = plan.counts()
    assert rc == -3 and n_ref == 0 and n_big == 3
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    r = res.view(KSW_RES_DTYPE).reshape(-1)
    assert r["status"][6] == KSW_TOO_BIG and (res[6, :44] == 0xee).all() and (cig[co[6]:co[7]] == np.uint32(FILL)).all()
    for k in cut:
        assert r["status"][k] == KSW_CIGAR_CUT and np.array_equal(np.array([int(r[f][k]) for f in EZ]), rs[k]["ez"].astype(np.int64))
        assert np.array_equal(cig[co[k]:co[k + 1]], rs[k]["cigar"][:room[k]])
    check_out(rs, res, cig, co, skip={6, *cut})
    assert guards_ok(rw, cw)
    plan.close()


def test_plan_runs_again_on_other_data_and_behind_another_plan_on_the_callers_stream(ref):
    from mm2chain import KswPlan
    a = [r for r in ref if r["case"]["sc"] == "asm20"][:300]
    b = [r for r in ref if r["case"]["sc"] == "ont" and r["case"]["name"].startswith(("len_", "big_", "lds_", "scratch_", "row_"))]
    c = [r for r in ref if r["case"]["sc"] == "swap"][:77]
    packs = [pack(x) for x in (a, b, c)]
    plan = KswPlan(max(len(a), len(b), len(c)), max(p[1].size for p in packs), max(int(p[2][-1]) for p in packs), SCRATCH)
    other = KswPlan(len(a), packs[0][1].size, int(packs[0][2][-1]), 64 << 20)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        outs = []
        for sc, rs, (tk, seq, co) in (("asm20", a, packs[0]), ("ont", b, packs[1]), ("swap", c, packs[2]), ("asm20", a[::-1], pack(a[::-1]))):
            o = run_plan(other, "asm20", a, *packs[0], stream=st.cuda_stream)        # another plan's kernel in front, no wait in between
            outs.append((rs, co, run_plan(plan, sc, rs, tk, seq, co, stream=st.cuda_stream), o))
            st.synchronize()                                                     # the plan's scratch and counters belong to one run at a time
            plan.check(); other.check()
    for rs, co, (_, rw, rv, cw, cv), (_, orw, orv, ocw, ocv) in outs:
        check_out(rs, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), co)
        check_out(a, orv.cpu().numpy(), ocv.cpu().numpy().view(np.uint32), packs[0][2])
        assert guards_ok(rw, cw) and guards_ok(orw, ocw)
    plan.close(); other.close()


def test_tasks_beyond_the_default_slots_run_in_slots_of_their_size(ref):
    """three tasks whose p takes 4.56 MB each (1 500 x 1 500 at w = 2 000, the band of -x ava-*) among small ones: not run in a plan with the default cut into 4 MiB
    slots (status 2, MM2C_E_TOOBIG, neighbours exact); exact in a plan whose two slots have their size, so a slot is used again; exact through the host entry with
    its own sizing (the slots follow the largest task, whatever the number of tasks) and with a scratch for two such slots; too big again with a scratch below one"""
    from mm2chain import KswPlan, ksw_extd2_batch, KSW_RES_DTYPE, KSW_TOO_BIG, Mm2cError
    big = [r for r in ref if r["case"]["name"].startswith("p_over_4mib_")]
    small = _some(ref, 9)
    rs = small[:2] + [big[0]] + small[2:5] + big[1:] + small[5:]
    where = {k for k, r in enumerate(rs) if r["case"]["name"].startswith("p_over_4mib_")}
    need = need_of(rs)
    assert len(big) == 3 and len(where) == 3 and all(need_of([b]) > (4 << 20) for b in big) and need_of(small) < (1 << 20)
    tk, seq, co = pack(rs)
    plan = KswPlan(len(rs), seq.size, int(co[-1]), 64 << 20)                      # the default cut
    assert plan.n_slots == 16 and plan.slot_bytes == 4 << 20
    _, rw, rv, cw, cv = run_plan(plan, "ont", rs, tk, seq, co)
    rc, n_ref, n_big = plan.counts()
    assert rc == -3 and n_ref == 0 and n_big == 3
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    for k in where:
        assert res.view(KSW_RES_DTYPE).reshape(-1)["status"][k] == KSW_TOO_BIG and (res[k, :44] == 0xee).all() and (cig[co[k]:co[k + 1]] == np.uint32(FILL)).all()
    check_out(rs, res, cig, co, skip=where)
    assert guards_ok(rw, cw)
    plan.close()
    plan = KswPlan(len(rs), seq.size, int(co[-1]), n_slots=2, slot_bytes=need)    # the caller's cut
    assert plan.n_slots == 2 and need <= plan.slot_bytes < need + 256
    _, rw, rv, cw, cv = run_plan(plan, "ont", rs, tk, seq, co)
    assert plan.counts() == (0, 0, 0)
    check_out(rs, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), co)
    assert guards_ok(rw, cw)
    plan.close()
    for scratch in (0, 2 * need + need // 2):
        res = np.zeros(len(rs), KSW_RES_DTYPE); cigar = np.full(int(co[-1]), FILL, np.uint32)
        ksw_extd2_batch(D.score_set("ont"), tk, seq, co, scratch_bytes=scratch, res=res, cigar=cigar)
        check_out(rs, res, cigar, co)
    res = np.zeros(len(rs), KSW_RES_DTYPE); cigar = np.full(int(co[-1]), FILL, np.uint32)
    with pytest.raises(Mm2cError, match="code -3"):
        ksw_extd2_batch(D.score_set("ont"), tk, seq, co, scratch_bytes=min(need_of([b]) for b in big) - 4096, res=res, cigar=cigar)
    assert {k for k in range(len(rs)) if res["status"][k] == KSW_TOO_BIG} == where
    check_out(rs, res, cigar, co, skip=where)
