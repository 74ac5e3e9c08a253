"""The extra plan on the device (csrc/align_extra.hip: mm_update_extra and mm_test_zdrop, align.c): every case of tests/extra_data.py through ExtraPlan and the host
entries, equal in every field and CIGAR word to what the reference's own functions made of it (tests/golden/ref_extra.npz) -- one batch per score set and is_eqx, the
same in reverse order through the same plan, the planted cases one region per call, guard rows around the results and the CIGAR words and fill behind every CIGAR,
each kind of refusal with exact neighbours, an EQX result cut to its slot and then exact in a slot of its size, and the z-drop entry straight on a KswPlan's device
outputs.  Size classes (extra_data.LDS_WORDS): CIGARs of 2 048 words in LDS and of 2 049 in a scratch slot; match runs of 15 .. 300 bases around the 16 a lane
walks alone and the 64 the wave takes per step.  Everything is integer and compared with ==."""
import os

import numpy as np
import pytest
import torch

import extra_data as D
import extra_model as M
import ksw_data

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL, GUARD, SLACK = 0x5e5e5e5e, 3, 2
UF = ("n_cigar", "qshift", "tshift", "blen", "mlen", "n_ambi", "dp_max")
SLOT_WORDS = 25000


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def fx():
    f = np.load(os.path.join(GOLDEN, "ref_extra.npz"))
    us, zs = D.update_cases(), D.zdrop_cases()
    assert [c["name"] for c in us] == list(f["u_names"]) and [c["name"] for c in zs] == list(f["z_names"])
    off, cig = f["u_cig_off"], f["u_cigar"]
    u = [dict(case=c, res=f["u_res"][k], cigar=(cig[off[2 * k]:off[2 * k + 1]], cig[off[2 * k + 1]:off[2 * k + 2]])) for k, c in enumerate(us)]
    z = [dict(case=c, res=f["z_res"][k]) for k, c in enumerate(zs)]
    return u, z


def t(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def guarded(n, width, dtype, fill):
    shape = (n + 2 * GUARD, width) if width else (n + 2 * GUARD,)
    whole = torch.full(shape, fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_ok(rw, cw):
    r, c = rw.cpu().numpy(), cw.cpu().numpy().view(np.uint32)
    return (r[:GUARD] == 0xee).all() and (r[-GUARD:] == 0xee).all() and (c[:GUARD] == FILL).all() and (c[-GUARD:] == FILL).all()


def pack(rs, x, room=None):
    """-> (tasks, seq, in_off, cig_in, out_off): sequences and input CIGARs one after another; an output slot of the expected length plus SLACK words (or room[k])"""
    from mm2chain import EXTRA_TASK_DTYPE
    tk = np.zeros(len(rs), EXTRA_TASK_DTYPE)
    seqs, cigs, at, ci, io, oo = [np.zeros(0, np.uint8)], [np.zeros(0, np.uint32)], 0, 0, [], [0]
    for k, r in enumerate(rs):
        c = r["case"]
        tk[k] = (at, at + c["q"].size, c["q"].size, c["t"].size, c["cigar"].size, c["rev"])
        seqs += [c["q"], c["t"]]; at += c["q"].size + c["t"].size
        io.append(ci); cigs.append(c["cigar"]); ci += c["cigar"].size
        oo.append(oo[-1] + (r["cigar"][x].size + SLACK if room is None else room[k]))
    return tk, np.concatenate(seqs).astype(np.uint8), np.array(io, np.int64), np.concatenate(cigs).astype(np.uint32), np.array(oo, np.int64)


def check_out(rs, x, res, cig, oo, skip=()):
    from mm2chain import EXTRA_RES_DTYPE
    res = res.view(EXTRA_RES_DTYPE).reshape(-1)
    for k, r in enumerate(rs):
        if k in skip:
            continue
        got = [int(res[f][k]) for f in UF]
        assert got == [int(v) for v in r["res"][x, :7]] and res["status"][k] == 0, (r["case"]["name"], x, got, r["res"][x], res["status"][k])
        n = r["cigar"][x].size
        assert np.array_equal(cig[oo[k]:oo[k] + n], r["cigar"][x]), (r["case"]["name"], x, D.text(cig[oo[k]:oo[k] + n]), D.text(r["cigar"][x]))
        assert (cig[oo[k] + n:oo[k + 1]] == np.uint32(FILL)).all(), r["case"]["name"]


def run_update(plan, sc, x, rs, packed, stream=None):
    from mm2chain import EXTRA_RES_DTYPE
    tk, seq, io, ci, oo = packed
    rw, rv = guarded(len(rs), EXTRA_RES_DTYPE.itemsize, torch.uint8, 0xee)
    cw, cv = guarded(plan.cig_out_cap, 0, torch.int32, FILL)
    pad = lambda v, n: v if v.numel() >= n else torch.cat([v, torch.zeros(n - v.numel(), dtype=v.dtype, device=v.device)])
    plan.update(D.score_set(sc), x, len(rs), t(tk), pad(t(seq), plan.seq_cap), t(io), pad(t(ci), plan.cig_in_cap), t(oo), rv, cv, stream=stream)
    return rw, rv, cw, cv


def by_score(rs):
    g = {}
    for r in rs:
        g.setdefault(r["case"]["sc"], []).append(r)
    return g


def test_every_update_case_in_batches_both_orders(fx):
    from mm2chain import ExtraPlan
    for sc, rs in by_score(fx[0]).items():
        for x in (0, 1):
            plan = None
            for order in (rs, rs[::-1]):
                p = pack(order, x)
                if plan is None:
                    plan = ExtraPlan(len(order), p[1].size, p[3].size, int(p[4][-1]), n_slots=64, slot_words=SLOT_WORDS)
                rw, rv, cw, cv = run_update(plan, sc, x, order, p)
                plan.check()
                check_out(order, x, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), p[4])
                assert guards_ok(rw, cw)
            assert plan.last_ms() > 0 and plan.last_kernel_ms()[0] > 0
            plan.close()


def test_planted_cases_one_region_per_call_and_host_entry(fx):
    from mm2chain import ExtraPlan, EXTRA_RES_DTYPE, EXTRA_TASK_DTYPE, update_extra_batch
    rs = [r for r in fx[0] if r["case"]["sc"] == "ont" and not r["case"]["name"].startswith(("rnd", "ksw/", "big_"))]
    for x in (0, 1):
        tk, seq, io, ci, oo = pack(rs, x)
        plan = ExtraPlan(1, seq.size, ci.size, int(oo[-1]), n_slots=2, slot_words=SLOT_WORDS)
        d_tk, d_seq, d_io, d_ci, d_oo = t(tk).reshape(-1, EXTRA_TASK_DTYPE.itemsize), t(seq), t(io), t(ci), t(oo)
        rw, rv = guarded(len(rs), EXTRA_RES_DTYPE.itemsize, torch.uint8, 0xee)
        cw, cv = guarded(plan.cig_out_cap, 0, torch.int32, FILL)
        for k in range(len(rs)):
            plan.update(D.score_set("ont"), x, 1, d_tk[k:], d_seq, d_io[k:], d_ci, d_oo[k:], rv[k:], cv)
        plan.check()
        check_out(rs, x, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), oo)
        assert guards_ok(rw, cw)
        plan.close()
        res = np.zeros(len(rs), EXTRA_RES_DTYPE); out = np.full(int(oo[-1]), FILL, np.uint32)
        update_extra_batch(D.score_set("ont"), x, tk, seq, io, ci, oo, res=res, cig_out=out)
        check_out(rs, x, res, out, oo)


def test_refusals_and_cut_leave_neighbours_exact(fx):
    """an op above 3, an empty N, only empty words, lengths that do not add up, offsets that leave the pools, a slot that runs backwards, a length above the limit:
    status 1 and nothing else, counted, MM2C_E_ARG; an EQX result longer than its slot: cut, scalars exact, MM2C_E_TOOBIG, then exact in a slot of its size"""
    from mm2chain import ExtraPlan, EXTRA_RES_DTYPE, EXTRA_REFUSED, EXTRA_CIGAR_CUT
    rs = [r for r in fx[0] if r["case"]["name"].startswith("rnd") and r["case"]["sc"] == "ont" and r["case"]["cigar"].size >= 3][:40]
    tk, seq, io, ci, oo = pack(rs, 1)
    ci = ci.copy()
    ci[io[1]] = (ci[io[1]] & ~np.uint32(0xf)) | 4                                  # op 4
    ci[io[3] + 1] = 3                                                             # 0N
    ci[io[5]:io[5] + tk["n_cigar"][5]] &= np.uint32(0xf)                          # only empty words
    ci[io[7]] += 16                                                               # one base too many
    bad = {1, 3, 5, 7, 9, 11, 13, 15}
    tk["q_off"][9] = -1; tk["t_off"][11] = seq.size; tk["qlen"][13] = (1 << 20) + 1; tk["n_cigar"][15] = ci.size + 1
    plan = ExtraPlan(len(rs), seq.size, ci.size, int(oo[-1]))
    rw, rv, cw, cv = run_update(plan, "ont", 1, rs, (tk, seq, io, ci, oo))
    rc, n_ref, n_big = plan.counts()
    assert rc == -2 and n_ref == len(bad) and n_big == 0
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    r = res.view(EXTRA_RES_DTYPE).reshape(-1)
    for k in bad:
        assert r["status"][k] == EXTRA_REFUSED and (res[k, :28] == 0xee).all() and (cig[oo[k]:oo[k + 1]] == np.uint32(FILL)).all()
    check_out(rs, 1, res, cig, oo, skip=bad)
    assert guards_ok(rw, cw)
    # cut
    grow = [k for k, q in enumerate(rs) if q["cigar"][1].size > q["case"]["cigar"].size][:2]
    room = [q["cigar"][1].size + SLACK for q in rs]
    room[grow[0]] = rs[grow[0]]["case"]["cigar"].size; room[grow[1]] = 0
    p = pack(rs, 1, room=room)
    rw, rv, cw, cv = run_update(plan, "ont", 1, rs, p)
    rc, n_ref, n_big = plan.counts()
    assert rc == -3 and n_ref == 0 and n_big == 2
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    r = res.view(EXTRA_RES_DTYPE).reshape(-1)
    for k in grow:
        assert r["status"][k] == EXTRA_CIGAR_CUT and [int(r[f][k]) for f in UF] == [int(v) for v in rs[k]["res"][1, :7]]
        assert np.array_equal(cig[p[4][k]:p[4][k + 1]], rs[k]["cigar"][1][:room[k]])
    check_out(rs, 1, res, cig, p[4], skip=set(grow))
    assert guards_ok(rw, cw)
    exact = pack(rs, 1, room=[int(v) for v in r["n_cigar"]])
    rw, rv, cw, cv = run_update(plan, "ont", 1, rs, exact)
    assert plan.counts() == (0, 0, 0)
    check_out(rs, 1, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), exact[4])
    # a CIGAR beyond LDS in a plan without slots is too big; overlapping buffers are refused at the entry
    big = [q for q in fx[0] if q["case"]["name"].startswith("words_%d" % (D.LDS_WORDS + 1))] + rs[:2]
    p = pack(big, 0)
    small = ExtraPlan(len(big), p[1].size, p[3].size, int(p[4][-1]))
    rw, rv, cw, cv = run_update(small, "ont", 0, big, p)
    assert small.counts() == (-3, 0, 1) and rv.cpu().numpy().view(EXTRA_RES_DTYPE).reshape(-1)["status"][0] == 2
    check_out(big, 0, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), p[4], skip={0})
    from mm2chain import Mm2cError
    both = t(np.zeros(max(small.cig_in_cap, small.cig_out_cap) + 8, np.uint32))
    with pytest.raises(Mm2cError):
        small.update(D.score_set("ont"), 0, len(big), t(p[0]), t(p[1]), t(p[2]), both, t(p[4]), None, both)
    plan.close(); small.close()


def z_expect(r, s):
    """the model's result for threshold set s, after it is checked against what the fixture recorded of the reference"""
    c = r["case"]
    mat, q, e = D.score_set(c["sc"])[:3]
    thr = D.ZD_THR[s]
    g = M.test_zdrop(c["q"], c["t"], c["cigar"], mat, q, e, thr[0], thr[1], thr[2], thr[3] != 0)
    ref = r["res"]
    assert (g["max_zdrop"], g["t0"], g["t1"] - g["t0"], g["q1"] - g["q0"]) == tuple(int(v) for v in ref[:4]) and (g["code"], g["inv_cand"]) == (int(ref[5 + 2 * s]), int(ref[6 + 2 * s]))
    return [g[f] for f in ("max_zdrop", "t0", "t1", "q0", "q1", "code", "inv_cand")]


def test_zdrop_on_a_ksw_plans_device_outputs_and_planted_cases(fx):
    """ksw_extd2 and mm_test_zdrop back to back on one stream, nothing downloaded in between; among the tasks a refused one (a flag outside MM2C_KSW_FLAGS) and one
    too big for its scratch slot: both get status 1 from the z-drop entry.  Then the planted CIGARs, uploaded as a ksw plan would have left them, in both orders
    through one plan, and through the host entry."""
    from mm2chain import ExtraPlan, KswPlan, KSW_TASK_DTYPE, KSW_RES_DTYPE, ZDROP_RES_DTYPE, test_zdrop_batch, ksw_task_scratch
    zs = [r for r in fx[1] if "ksw" in r["case"] and r["case"]["sc"] == "ont" and r["case"]["name"].startswith(("ksw/zdrop_", "ksw/ins60/", "ksw/w_3/", "ksw/len_6", "ksw/homo"))]
    kc = ksw_data.cases()
    tk = np.zeros(len(zs), KSW_TASK_DTYPE)
    seqs, at, co = [], 0, [0]
    for k, r in enumerate(zs):
        c = kc[r["case"]["ksw"]]
        tk[k] = (at, at + c["q"].size, c["q"].size, c["t"].size, c["w"], c["zdrop"], c["end_bonus"], c["flag"])
        seqs += [c["q"], c["t"]]; at += c["q"].size + c["t"].size
        co.append(co[-1] + r["case"]["cigar"].size + SLACK)
    need = [ksw_task_scratch(int(x["qlen"]), int(x["tlen"]), int(x["w"]), int(x["flag"])) for x in tk]
    big = int(np.argmax(need))
    slot = sorted(need)[-2] + 256 if sorted(need)[-2] < need[big] else need[big]
    tk["flag"][2] = 0x04
    skip = {2} | ({big} if slot < need[big] else set())
    seq, co = np.concatenate(seqs).astype(np.uint8), np.array(co, np.int64)
    kp = KswPlan(len(zs), seq.size, int(co[-1]), n_slots=64, slot_bytes=slot)
    xp = ExtraPlan(len(zs), seq.size, int(co[-1]))
    d_tk, d_seq, d_co = t(tk), t(seq), t(co)
    zw, zv = guarded(len(zs), ZDROP_RES_DTYPE.itemsize, torch.uint8, 0xee)
    kres, kcig = kp.run(D.score_set("ont"), len(zs), d_tk, d_seq, d_co)
    xp.zdrop(D.score_set("ont"), D.ZD_THR[1], len(zs), d_tk, d_seq, d_co, kres, kcig, zv)
    rc, n_ref, n_big = xp.counts()
    assert rc == -2 and n_ref == len(skip) and n_big == 0
    z = zv.cpu().numpy()
    zz = z.view(ZDROP_RES_DTYPE).reshape(-1)
    for k, r in enumerate(zs):
        if k in skip:
            assert zz["status"][k] == 1 and (z[k, :28] == 0xee).all()
        else:
            assert [int(v) for v in list(zz[k])[:7]] == z_expect(r, 1) and zz["status"][k] == 0, r["case"]["name"]
    assert (zw.cpu().numpy()[:GUARD] == 0xee).all() and (zw.cpu().numpy()[-GUARD:] == 0xee).all() and xp.last_kernel_ms()[1] > 0
    kp.close(); xp.close()
    # planted CIGARs
    ps = [r for r in fx[1] if "ksw" not in r["case"]]
    plan = None
    for order in (ps, ps[::-1]):
        tk = np.zeros(len(order), KSW_TASK_DTYPE); kr = np.zeros(len(order), KSW_RES_DTYPE)
        seqs, cigs, at, co = [], [np.zeros(0, np.uint32)], 0, [0]
        for k, r in enumerate(order):
            c = r["case"]
            tk[k] = (at, at + c["q"].size, c["q"].size, c["t"].size, 50, 400, -1, 0)
            kr["n_cigar"][k] = c["cigar"].size
            seqs += [c["q"], c["t"]]; at += c["q"].size + c["t"].size
            cigs.append(c["cigar"]); co.append(co[-1] + c["cigar"].size)
        seq, co, cg = np.concatenate(seqs).astype(np.uint8), np.array(co, np.int64), np.concatenate(cigs).astype(np.uint32)
        if plan is None:
            plan = ExtraPlan(len(order), seq.size, cg.size, 0, n_slots=8, slot_words=SLOT_WORDS)
        for s in (0, 1):
            sets = by_score(order)
            for sc in sets:
                zw, zv = guarded(len(order), ZDROP_RES_DTYPE.itemsize, torch.uint8, 0xee)
                plan.zdrop(D.score_set(sc), D.ZD_THR[s], len(order), t(tk), t(seq), t(co), t(kr), t(cg), zv)
                plan.check()
                zz = zv.cpu().numpy().view(ZDROP_RES_DTYPE).reshape(-1)
                for k, r in enumerate(order):
                    if r["case"]["sc"] == sc:
                        assert [int(v) for v in list(zz[k])[:7]] == z_expect(r, s) and zz["status"][k] == 0, (r["case"]["name"], s)
                assert (zw.cpu().numpy()[:GUARD] == 0xee).all() and (zw.cpu().numpy()[-GUARD:] == 0xee).all()
        ont = [k for k, r in enumerate(order) if r["case"]["sc"] == "ont"]
        zh = test_zdrop_batch(D.score_set("ont"), D.ZD_THR[1], tk, seq, co, kr, cg)
        for k in ont:
            assert [int(v) for v in list(zh[k])[:7]] == z_expect(order[k], 1)
    plan.close()


def test_backward_slot_and_zdrop_refusals_leave_neighbours_exact(fx):
    """an output slot that runs backwards ([0, 40) for region 0, (40, 20) for region 1, [20, 60) for region 2); z-drop tasks whose n_cigar is longer than their slot,
    whose CIGAR leaves the target or the query, whose slot lies behind the plan's words, whose sequences leave the pool: status 1 and nothing else, counted,
    MM2C_E_ARG, the items beside them exact"""
    from mm2chain import ExtraPlan, EXTRA_RES_DTYPE, EXTRA_REFUSED, KSW_TASK_DTYPE, KSW_RES_DTYPE, ZDROP_RES_DTYPE
    three = [r for r in fx[0] if r["case"]["name"].startswith("rnd") and r["case"]["sc"] == "ont" and 3 <= r["cigar"][0].size <= 20][:3]
    tk, seq, io, ci, _ = pack(three, 0)
    oo = np.array([0, 40, 20, 60], np.int64)
    plan = ExtraPlan(3, seq.size, ci.size, 60)
    rw, rv, cw, cv = run_update(plan, "ont", 0, three, (tk, seq, io, ci, oo))
    assert plan.counts() == (-2, 1, 0)
    res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
    assert res.view(EXTRA_RES_DTYPE).reshape(-1)["status"][1] == EXTRA_REFUSED and (res[1, :28] == 0xee).all()
    n0, n2 = three[0]["cigar"][0].size, three[2]["cigar"][0].size
    assert np.array_equal(cig[:n0], three[0]["cigar"][0]) and (cig[n0:20] == np.uint32(FILL)).all() and np.array_equal(cig[20:20 + n2], three[2]["cigar"][0])
    assert (cig[20 + n2:60] == np.uint32(FILL)).all() and guards_ok(rw, cw)
    plan.close()
    ps = [r for r in fx[1] if "ksw" not in r["case"] and r["case"]["sc"] == "ont" and 2 <= r["case"]["cigar"].size <= 64 and r["case"]["name"] != "partial"][:12]
    tk = np.zeros(len(ps), KSW_TASK_DTYPE); kr = np.zeros(len(ps), KSW_RES_DTYPE)
    seqs, cigs, at, co = [], [], 0, [0]
    for k, r in enumerate(ps):
        c = r["case"]
        tk[k] = (at, at + c["q"].size, c["q"].size, c["t"].size, 50, 400, -1, 0)
        kr["n_cigar"][k] = c["cigar"].size
        seqs += [c["q"], c["t"]]; at += c["q"].size + c["t"].size
        cigs.append(c["cigar"]); co.append(co[-1] + c["cigar"].size)
    seq, co, cg = np.concatenate(seqs).astype(np.uint8), np.array(co, np.int64), np.concatenate(cigs).astype(np.uint32)
    bad = {1, 3, 5, 7, len(ps) - 1}
    kr["n_cigar"][1] += 1                                                        # longer than its slot
    tk["tlen"][3] -= 1; tk["qlen"][5] -= 1                                       # the walk would leave the target, the query
    tk["t_off"][7] = seq.size                                                    # the sequences leave the pool
    plan = ExtraPlan(len(ps), seq.size, int(co[-1]) - 1)                         # the last task's slot lies behind the plan's words
    zw, zv = guarded(len(ps), ZDROP_RES_DTYPE.itemsize, torch.uint8, 0xee)
    plan.zdrop(D.score_set("ont"), D.ZD_THR[1], len(ps), t(tk), t(seq), t(co), t(kr), t(cg), zv)
    assert plan.counts() == (-2, len(bad), 0)
    z = zv.cpu().numpy()
    zz = z.view(ZDROP_RES_DTYPE).reshape(-1)
    for k, r in enumerate(ps):
        if k in bad:
            assert zz["status"][k] == EXTRA_REFUSED and (z[k, :28] == 0xee).all()
        else:
            assert [int(v) for v in list(zz[k])[:7]] == z_expect(r, 1) and zz["status"][k] == 0, r["case"]["name"]
    assert (zw.cpu().numpy()[:GUARD] == 0xee).all() and (zw.cpu().numpy()[-GUARD:] == 0xee).all()
    plan.close()


def test_plan_runs_again_on_other_data_behind_another_plans_kernel(fx):
    from mm2chain import ExtraPlan
    a = [r for r in fx[0] if r["case"]["sc"] == "asm20"][:200]
    b = [r for r in fx[0] if r["case"]["sc"] == "ont" and r["case"]["name"].startswith(("words_", "homo_", "ont_"))]
    packs = [pack(a, 1), pack(b, 0), pack(a[::-1], 0)]
    plan = ExtraPlan(max(len(a), len(b)), max(p[1].size for p in packs), max(p[3].size for p in packs), max(int(p[4][-1]) for p in packs), n_slots=16, slot_words=SLOT_WORDS)
    other = ExtraPlan(len(a), packs[0][1].size, packs[0][3].size, int(packs[0][4][-1]))
    st = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(st):
        for sc, x, rs, p in (("asm20", 1, a, packs[0]), ("ont", 0, b, packs[1]), ("asm20", 0, a[::-1], packs[2])):
            o = run_update(other, "asm20", 1, a, packs[0], stream=st.cuda_stream)
            outs.append((rs, x, p, run_update(plan, sc, x, rs, p, stream=st.cuda_stream), o))
            st.synchronize()
            plan.check(); other.check()
    for rs, x, p, (rw, rv, cw, cv), (orw, orv, ocw, ocv) in outs:
        check_out(rs, x, rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32), p[4])
        check_out(a, 1, orv.cpu().numpy(), ocv.cpu().numpy().view(np.uint32), packs[0][4])
        assert guards_ok(rw, cw) and guards_ok(orw, ocw)
    plan.close(); other.close()
