"""Aligned regions to final hits on the device (csrc/align_finish.hip).  fin_select: every case of tests/fin_data.py through one FinPlan three ways --
one batch per option set, one read per call, and finish_regions_batch -- byte for byte against what the reference's own hit.o made of it (tests/golden/ref_fin.npz)
and against the model, dp_max2 in the p records included; refusals beside exact neighbours, capacities exceeded by one, an empty batch, the lifecycle.  fin_apply:
regions, p records and the children of mm_split_reg against the model and the reference's mm_split_reg, through the plan and apply_regions_batch."""
import os

import numpy as np
import pytest
import torch

import fin_data as D
import fin_model as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL = 0xee
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def want():
    """name -> what the plan must give: dict(regs, pext, beyond) or None for a refused read; the fixture's bytes wherever the reference was run, checked against the model"""
    Z = np.load(os.path.join(GOLDEN, "ref_fin.npz"))
    names = [str(s) for s in Z["names"]]
    W = {}
    for c in D.cases():
        if c["refuse"]:
            W[c["name"]] = None
            continue
        m = M.finish(c["regs"], c["pext"], c["qlen"], c["rep_len"], c["opt"], max_log_arg=D.MAX_LOG_ARG)
        k = names.index(c["name"])
        ref = Z["hits_out"][int(Z["out_off"][k]):int(Z["out_off"][k + 1])].reshape(-1).view(M.REG)
        if m["beyond"] == 0:
            assert m["regs"].tobytes() == ref.tobytes(), c["name"]
        W[c["name"]] = m
    return W


def _opt(o):
    from mm2chain import params
    return params.fin_opts(**o)


def groups():
    """[(opt, [cases])]: the cases of one option set make one batch"""
    G = {}
    for c in D.cases():
        G.setdefault(tuple(c["opt"][k] for k in M.OPT_FIELDS), []).append(c)
    return [(cs[0]["opt"], cs) for cs in G.values()]


def _batch(cs, n_reads, room=2):
    """the reads one after another with `room` rows more than they have regions; p shifted to the batch's records"""
    rooms = [c["regs"].size + room for c in cs] + [0] * (n_reads - len(cs))
    f_off = np.concatenate([[0], np.cumsum(rooms)]).astype(np.int64)
    regs = np.full(max(int(f_off[-1]), 1) * 80, FILL, np.uint8).view(M.REG)
    pext, p_off = [], []
    for k, c in enumerate(cs):
        r = c["regs"].copy()
        p_off.append(sum(x.size for x in pext))
        r["p"][r["p"] != 0] += p_off[-1]
        regs[f_off[k]:f_off[k] + r.size] = r
        pext.append(c["pext"])
    pad = lambda v, fill: np.array(v + [fill] * (n_reads - len(cs)), np.int32)
    return dict(f_off=f_off, regs=regs, pext=np.concatenate(pext + [np.zeros(0, M.PEXT)]), p_off=p_off, n_in=pad([c["regs"].size for c in cs], 0),
                qlen=pad([c["qlen"] for c in cs], 1000), rep_len=pad([c["rep_len"] for c in cs], 0))


def _run(plan, o, B, guard=3):
    regs = np.full(max(plan.n_u_cap, 1) * 80, FILL, np.uint8)
    nb = min(regs.size, B["regs"].size * 80)                                   # (a batch may be longer than the plan's capacity: the read that leaves it is refused)
    regs[:nb] = B["regs"].view(np.uint8)[:nb]
    px = np.zeros(max(plan.n_pext_cap, 1) + guard, M.PEXT); px[:B["pext"].size] = B["pext"]; px["reserved"][B["pext"].size:] = -7
    out = torch.full((max(plan.n_u_cap, 1) + guard, 80), FILL, dtype=torch.uint8, device="cuda")
    n_out = torch.full((plan.n_reads + guard,), -9, dtype=torch.int32, device="cuda")
    d_px = t(px.view(np.uint8))
    plan.run(_opt(o), t(B["f_off"]), t(regs.reshape(-1, 80)), t(B["n_in"]), d_px, t(B["qlen"]), t(B["rep_len"]), regs_out=out, n_out=n_out)
    torch.cuda.synchronize()
    got_px = d_px.cpu().numpy().view(M.PEXT)
    assert got_px[B["pext"].size:].tobytes() == px[B["pext"].size:].tobytes(), "records behind the batch's were written"
    o_h, n_h = out.cpu().numpy(), n_out.cpu().numpy()
    assert (o_h[max(plan.n_u_cap, 1):] == FILL).all() and (n_h[plan.n_reads:] == -9).all(), "rows behind the capacities were written"
    return o_h.reshape(-1).view(M.REG), n_h, got_px[:B["pext"].size]


def _assert_read(got, B, k, c, w, what, untouched=-9):
    out, n_out, px = got
    room = out[B["f_off"][k]:B["f_off"][k + 1]]
    if w is None:                                                              # refused: nothing of the read is written
        assert n_out[k] == untouched and (room.view(np.uint8) == FILL).all(), f"{what}: {c['name']}: a refused read was written"
        assert px[B["p_off"][k]:B["p_off"][k] + c["pext"].size].tobytes() == c["pext"].tobytes()
        return
    assert n_out[k] == w["regs"].size, f"{what}: {c['name']}: n_out = {n_out[k]}, want {w['regs'].size}"
    g = room[:w["regs"].size].copy()
    g["p"][g["p"] != 0] -= B["p_off"][k]
    bad = [i for i in range(g.size) if g[i].tobytes() != w["regs"][i].tobytes()]
    assert not bad, f"{what}: {c['name']}: {len(bad)} of {g.size} hits differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {w['regs'][bad[0]]}"
    assert px[B["p_off"][k]:B["p_off"][k] + c["pext"].size].tobytes() == w["pext"].tobytes(), f"{what}: {c['name']}: the p records differ"


def _caps():
    G = groups()
    return max(len(cs) for _, cs in G), max(sum(c["regs"].size + 2 for c in cs) for _, cs in G), max(sum(c["pext"].size for c in cs) for _, cs in G)


def test_every_case_three_ways_through_one_plan(want):
    import mm2chain
    n_reads, n_u, n_p = _caps()
    plan = mm2chain.FinPlan(n_reads, n_u, n_p, max_log_arg=D.MAX_LOG_ARG, match_sc=2)
    try:
        for o, cs in groups():
            B = _batch(cs, n_reads)
            got = _run(plan, o, B)
            rc, refused, beyond, hits = plan.counts()
            for k, c in enumerate(cs):
                _assert_read(got, B, k, c, want[c["name"]], "one batch")
            assert (got[1][len(cs):n_reads] == 0).all()
            n_ref = sum(want[c["name"]] is None for c in cs)
            n_bey = sum(want[c["name"]]["beyond"] for c in cs if want[c["name"]])
            assert (refused, beyond, hits) == (n_ref, n_bey, sum(want[c["name"]]["regs"].size for c in cs if want[c["name"]])), (o, plan.counts())
            assert rc == (-2 if n_ref else -3 if n_bey else 0)
            for c in cs:                                                       # one read per call
                B1 = _batch([c], n_reads)
                _assert_read(_run(plan, o, B1), B1, 0, c, want[c["name"]], "one read per call")
            H = mm2chain.finish_regions_batch(_opt(o), B["f_off"][:len(cs) + 1], B["regs"], B["n_in"][:len(cs)], B["pext"], B["qlen"][:len(cs)], B["rep_len"][:len(cs)],
                                              max_log_arg=D.MAX_LOG_ARG, fill=FILL)
            assert H["rc"] == rc
            for k, c in enumerate(cs):
                _assert_read((H["regs"], H["n_out"], H["pext"]), B, k, c, want[c["name"]], "finish_regions_batch", untouched=np.frombuffer(bytes([FILL] * 4), np.int32)[0])
    finally:
        plan.close()


def _good(want):
    cs = {c["name"]: c for c in D.cases()}
    return [cs[n] for n in ("dp_max2_of_three", "n65_ties", "identical_after_dp")]


def test_refusals_leave_the_neighbours_exact(want):
    """between exact neighbours: offsets that run backwards, n_in beyond the read's room, a read that leaves n_u_cap by one region, a p one past n_pext_cap (and the
    same p with one record more: accepted), inv, is_alt, mixed p"""
    import mm2chain
    by = {c["name"]: c for c in D.cases()}
    g = _good(want)
    o = g[0]["opt"]
    cs = [g[0], by["inv_region"], g[1], by["alt_region"], by["mixed_p"], g[2], by["one"], by["two_reordered"]]
    B = _batch(cs, len(cs))
    n_u, n_p = int(B["f_off"][-1]), B["pext"].size
    W = [want[c["name"]] for c in cs]
    # read 6 ("one"): its p names the record one past the capacity; read 7: n_in beyond its room
    B["regs"]["p"][B["f_off"][6]] = n_p + 1
    B["n_in"][7] = int(B["f_off"][8] - B["f_off"][7]) + 1
    W[6] = W[7] = None
    plan = mm2chain.FinPlan(len(cs), n_u, n_p, max_log_arg=D.MAX_LOG_ARG)
    got = _run(plan, o, B)
    assert plan.counts()[:2] == (-2, 5)
    for k, c in enumerate(cs):
        if k != 6:
            _assert_read(got, B, k, c, W[k], "refusals")
    assert got[1][6] == -9 and got[1][7] == -9 and (got[0][B["f_off"][6]:B["f_off"][7]].view(np.uint8) == FILL).all()
    with pytest.raises(mm2chain.Mm2cError, match=r"code -2\).*5 read\(s\) refused.*1 offsets.*2 with inv or is_alt.*1 with a p that names no record.*1 that mix"):
        plan.check()
    plan.close()
    # offsets that run backwards between two reads, and a last read that leaves n_u_cap by one region
    B = _batch(cs[:1] + [by["one"], g[1], by["two_reordered"]], 4)
    B["f_off"][2] = B["f_off"][1] - 1
    plan = mm2chain.FinPlan(4, int(B["f_off"][-1]) - 1, B["pext"].size, max_log_arg=D.MAX_LOG_ARG)
    got = _run(plan, o, B)
    assert plan.counts()[:2] == (-2, 3)
    _assert_read(got, B, 0, g[0], want[g[0]["name"]], "bad offsets beside")
    assert list(got[1][1:4]) == [-9, -9, -9]
    plan.close()


def test_an_empty_batch_and_the_lifecycle(want):
    import ctypes as C
    import mm2chain
    from mm2chain import _native as N

    def launches():
        st = N.Stats()
        N.load().mm2c_get_stats(C.byref(st))
        return int(st.launches)
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")
    empty = mm2chain.FinPlan(0, 0, 0, max_log_arg=16)
    at = launches()
    out, n_out = empty.run(_opt(D.DEFAULT), z(1, torch.int64), z(80, torch.uint8), z(1, torch.int32), z(32, torch.uint8), z(0, torch.int32), z(0, torch.int32))
    assert launches() == at and empty.counts() == (0, 0, 0, 0) and n_out.numel() == 0
    empty.close(); empty.close()
    assert empty.handle is None
    c = _good(want)[0]
    B = _batch([c], 1)
    plan = mm2chain.FinPlan(1, int(B["f_off"][-1]), B["pext"].size, max_log_arg=D.MAX_LOG_ARG)
    assert plan.counts() == (0, 0, 0, 0) and plan.apply_counts() == (0, 0, 0, 0)
    with pytest.raises(mm2chain.Mm2cError, match=r"code -2\).*has not been run"):
        plan.last_ms()
    with pytest.raises(mm2chain.Mm2cError, match=r"code -2\).*match_sc 1 is not the plan's 2"):
        plan.run(_opt(dict(D.DEFAULT, match_sc=1)), t(B["f_off"]), t(B["regs"].view(np.uint8)), t(B["n_in"]), t(B["pext"].view(np.uint8)), t(B["qlen"]), t(B["rep_len"]))
    at = launches()
    g1 = _run(plan, c["opt"], B)
    assert launches() - at == 1 and plan.check() == want[c["name"]]["regs"].size
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):                                                # a run on a caller's stream (torch's current one)
        g2 = _run(plan, c["opt"], B)
    assert g1[0].tobytes() == g2[0].tobytes() and g1[2].tobytes() == g2[2].tobytes()
    _assert_read(g2, B, 0, c, want[c["name"]], "second run")
    ms = plan.last_ms()
    assert ms[0] == 0 and ms[1] >= 0
    plan.close(); plan.close()


# ---- fin_apply ----
def apply_batch():
    """one read per split case of fin_data, region and anchors as the reference's mm_split_reg got them, and between them regions that are not split: with p on
    either strand, without p, refused in front, incomplete in front"""
    S = D.split_cases()
    regs, cig, anc, qlens, xr, xe = [], [], [], [], [], []

    def add(r, a, qlen, **c):
        C = np.zeros((), M.CIG_REG)
        g = len(regs)
        C["rs1"], C["re1"], C["r_qs"], C["r_qe"], C["qs1"], C["qe1"] = 1000 + g, 2000 + g, 10 + g, 900 + g, 10 + g, 900 + g
        C["dp_score"], C["n_cigar"], C["cig0"] = 500 + g, 7, 100 * g
        ex = c.pop("extra", None)
        for k, v in c.items():
            C[k] = v
        if C["has_p"] and ex != "none":
            E = np.zeros((), M.EXTRA_RES)
            E["n_cigar"], E["qshift"], E["tshift"], E["blen"], E["mlen"], E["n_ambi"], E["dp_max"], E["status"] = 5 + g, 3, 4, 800 + g, 700 + g, g, 450 + g, ex or 0
            xr.append(g); xe.append(E)
        regs.append(r); cig.append(C); anc.append(a); qlens.append(qlen)
    plain = S[0]["reg"].copy(); plain["cnt"] = 4; plain["as"] = 0
    rv = plain.copy(); rv["flags"] |= 1 << 10
    add(plain, D.anchors(4, 0), 700, has_p=1)
    for s in S:
        add(s["reg"], s["a"], s["qlen"], has_p=1, split_n=s["n"], split_inv=s["split_inv"], zdrop_code=2 if s["split_inv"] else 1, dropped=1)
        add(rv, D.anchors(4, 1), 800, has_p=1)
    add(plain, D.anchors(4, 0), 700, has_p=0)
    add(plain, D.anchors(4, 0), 700, has_p=1, status=1)
    add(plain, D.anchors(4, 0), 700, has_p=1, extra=2)
    add(plain, D.anchors(4, 0), 700, has_p=1, extra=1)
    add(S[0]["reg"], S[0]["a"][:5], 700, has_p=1, split_n=S[0]["n"])           # the child's anchors leave the read's
    add(plain, D.anchors(4, 0), 700, has_p=1)
    n = len(regs)
    off = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    out_off = off([int(e["n_cigar"]) + 1 for e in xe])
    return dict(u_off=off([1] * n), regs=np.array(regs, M.REG), b_off=off([len(a) for a in anc]), b=np.concatenate(anc), read_off=off(qlens), cig=np.array(cig, M.CIG_REG),
                xr=np.array(xr, np.int32), xe=np.array(xe, M.EXTRA_RES), out_off=out_off, n_split=len(S))


def _apply_check(G, m, cap, what):
    n = len(m["status"])
    assert np.array_equal(G["status"], m["status"]), (what, G["status"], m["status"])
    for g in range(n):
        if m["status"][g] in (0, M.OVER_CAP):
            assert G["regs"][g].tobytes() == m["regs"][g].tobytes(), f"{what}: region {g}:\n got {G['regs'][g]}\nwant {m['regs'][g]}"
            assert G["pext"][g].tobytes() == m["pext"][g].tobytes(), f"{what}: p record {g}: {G['pext'][g]} {m['pext'][g]}"
        else:
            assert (G["regs"][g:g + 1].view(np.uint8) == FILL).all() and (G["pext"][g:g + 1].view(np.uint8) == FILL).all(), f"{what}: a refused region was written"
    assert G["n_child"] == m["n_child"]
    k = min(cap, m["n_child"])
    assert list(G["child_of"][:k]) == m["child_of"][:k]
    for j in range(k):
        assert G["child"][j].tobytes() == m["child"][j].tobytes(), f"{what}: child {j}:\n got {G['child'][j]}\nwant {m['child'][j]}"
    assert (G["child"][k:].view(np.uint8) == FILL).all() and (G["child_of"][k:].view(np.uint8) == FILL).all(), f"{what}: written behind the children"


@pytest.mark.parametrize("short", [0, 1])
def test_apply_through_the_plan_and_the_host_entry(short):
    """short = 1: n_child_cap is one below the children the batch has"""
    import mm2chain
    A = apply_batch()
    cap = A["n_split"] - 1 if short else A["n_split"] + 2
    m = M.apply(A["u_off"], A["regs"], A["b_off"], A["b"], A["read_off"], A["cig"], A["xr"], A["xe"], A["out_off"], cap)
    assert m["n_child"] == A["n_split"] and m["counts"] == (3, 1, short)
    Z = np.load(os.path.join(GOLDEN, "ref_fin.npz"))
    for j, s in enumerate(D.split_cases()[:min(cap, 4)]):                       # the model's children are the reference's r2, with align.c:759 on top
        w = Z["split_r2"][j].view(M.REG)[0].copy()
        w["flags"] |= s["split_inv"] << M.SPLIT_INV_BIT
        assert m["child"][j].tobytes() == w.tobytes(), s["name"]
    n = len(A["regs"])
    plan = mm2chain.FinPlan(n, n, n, max_log_arg=16)
    filled = lambda rows, width: torch.full((max(rows, 1) + 2, width), FILL, dtype=torch.uint8, device="cuda")
    out, px, ch = filled(n, 80), filled(n, 32), filled(cap, 80)
    st, co = torch.full((n + 2,), -9, dtype=torch.int32, device="cuda"), filled(cap, 4).view(torch.int32).reshape(-1)
    d_b = t(A["b"].view(np.int64))
    r = plan.apply(n, n, t(A["u_off"]), t(A["regs"].view(np.uint8)), t(A["b_off"]), d_b, t(A["read_off"]), t(A["cig"].view(np.uint8)), len(A["xr"]), t(A["xr"]),
                   t(A["xe"].view(np.uint8)), t(A["out_off"]), cap, regs_out=out, pext=px, status=st, child=ch, child_of=co)
    torch.cuda.synchronize()
    h = lambda x, dt: x.cpu().numpy().reshape(-1).view(dt)
    G = dict(regs=h(out, M.REG)[:n], pext=h(px, M.PEXT)[:n], status=h(st, np.int32)[:n], child=h(ch, M.REG)[:cap], child_of=h(co, np.int32)[:cap], n_child=int(r[5].cpu()[0]))
    _apply_check(G, m, cap, "FinPlan.apply")
    assert (h(out, np.uint8)[n * 80:] == FILL).all() and (h(ch, np.uint8)[max(cap, 1) * 80:] == FILL).all() and (h(st, np.int32)[n:] == -9).all()
    assert plan.apply_counts() == (-2,) + m["counts"] and plan.last_ms()[0] >= 0
    plan.close()
    H = mm2chain.apply_regions_batch(A["u_off"], A["regs"], A["b_off"], A["b"], A["read_off"], A["cig"], A["xr"], A["xe"], A["out_off"], cap, fill=FILL)
    assert H["rc"] == -2
    _apply_check(H, m, cap, "apply_regions_batch")


@pytest.mark.parametrize("name", ["ont", "asm20", "sr"])
def test_the_chain_in_device_memory_with_apply_in_the_place_of_the_python_split(name):
    """the rounds of tests/test_gpu_cig.py::test_the_chain_in_device_memory -- AlnPlan -> KswPlan -> ExtraPlan.zdrop -> CigPlan.second -> KswPlan -> CigPlan.join ->
    ExtraPlan.update on the regions of tests/cig_data.ref_batches() -- with FinPlan.apply behind them on the same device arrays: the regions and p records it writes
    hold the reference's r and r->p (tests/golden/ref_cig.npz), and the children it returns are, byte for byte, the regions the reference split off and called
    mm_align1 on next (cig_ref.batch(name, level + 1)); they go into the next round as they lie on the GPU, their per-read offsets being index arithmetic on child_of"""
    import aln_data as AD
    import cig_data as CD
    import cig_ref
    from mm2chain import AlnPlan, KswPlan, ExtraPlan, CigPlan, FinPlan, RefSeq, params, ksw_task_scratch, KSW_RES_DTYPE
    fx = cig_ref.fixture()
    o = CD.cached_ref_batches()[name][0]
    aopt = params.aln_opts(**{k: o[k] for k in o if k not in ("q2", "sc_ambi")})
    score = params.ksw_scores("map-ont", a=o["a"], b=o["b"], q=o["q"], e=o["e"], q2=o["q2"], e2=o["e2"], sc_ambi=o["sc_ambi"])
    ref = RefSeq(*AD.reference())
    fwd = cig_ref.inputs(name, 0)[6]
    d_b = t(cig_ref.inputs(name, 0)[4]).reshape(-1)
    d_regs, u_off, rounds, made = None, None, 0, []
    for level in range(3):
        B, names = cig_ref.batch(name, level)
        b_off, read_off = B["b_off"], B["read_off"]
        n_reads = len(b_off) - 1
        if level == 0:
            u_off, d_regs = B["u_off"], t(cig_ref.inputs(name, 0)[2].view(np.uint8))
        assert np.array_equal(u_off, B["u_off"]), (name, level, "the children's reads are not the recorded ones")
        n_regs = int(u_off[-1])
        if n_regs == 0:
            break
        rounds += 1
        tot = (len(B["items"]), len(B["tasks"]), int(B["cig_off"][-1]), len(B["pool"]))
        n_b = d_b.numel() // 2
        slot = max([ksw_task_scratch(int(T["qlen"]), int(T["tlen"]), int(T["w"]), int(T["flag"]) & ~8) for T in B["tasks"]] + [1 << 20])
        ap = AlnPlan(n_regs, tot[0], tot[1], tot[3], n_b, fwd.size, cig_shift=0, n_slots=64)
        kp = KswPlan(tot[1], tot[3], tot[2], n_slots=32, slot_bytes=slot)
        ep = ExtraPlan(max(tot[1], n_regs), tot[3], tot[2], tot[2], n_slots=32, slot_words=min(max(tot[2], 16), 1 << 18))
        cp = CigPlan(n_regs, tot[0], tot[1], tot[2], tot[1], tot[2], tot[3], n_b, tot[2], n_regs)
        fp = FinPlan(n_reads, n_regs, n_regs, max_log_arg=16)
        d_u, d_bo, d_ro = t(u_off), t(b_off), t(read_off)
        ar, items, tasks, cig_off, pool = ap.run(aopt, ref, n_reads, n_regs, d_u, d_regs, d_bo, d_b, d_ro, t(fwd))
        assert ap.counts()[:3] == (0, 0, 0)
        res, cigar = kp.run(score, tot[1], tasks, pool, cig_off)
        zres = ep.zdrop(score, dict(zdrop=o["zdrop"], zdrop_inv=o["zdrop_inv"], max_gap=o["max_gap"], no_inv=o["flag"] & 1), tot[1], tasks, pool, cig_off, res, cigar)
        two = np.nonzero(B["zres"]["code"] == 2)[0]
        if two.size:                                                               # ksw_ll_i16 is the host's: its verdict comes from the record
            zres.view(torch.int32).reshape(-1, 8)[torch.from_numpy(two).cuda(), 5] = 2
        tasks2, cig_off2, second_of = cp.second(B["opt"], score, n_regs, ar, items, tasks, zres, pool)
        n2, w2 = cp.second_check()
        res2 = torch.zeros((max(tot[1], 1), KSW_RES_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        res2, cigar2 = kp.run(score, n2, tasks2, pool, cig_off2, res=res2)
        cig_regs, cig_out, in_off, xt, xr = cp.join(B["opt"], n_reads, n_regs, d_u, d_regs, d_bo, d_b, d_ro, ar, items, cig_off, res, cigar, zres, second_of, cig_off2, res2, cigar2)
        rc, n_ref, n_inc, n_over, (words, n_extra) = cp.counts()
        assert (n_inc, n_over) == (0, 0)
        xres, xcig = ep.update(score, 0, n_extra, xt, pool, in_off, cig_out, in_off)
        assert ep.counts()[0] == 0
        cap = n_regs
        regs_out, pext, status, child, child_of, n_child = fp.apply(n_reads, n_regs, d_u, d_regs, d_bo, d_b, d_ro, cig_regs, n_extra, xr, xres, in_off, cap)
        rc, a_ref, a_inc, a_bey = fp.apply_counts()
        assert (a_ref, a_inc, a_bey) == (n_ref, 0, 0)
        R, P, S = regs_out.cpu().numpy().reshape(-1).view(M.REG), pext.cpu().numpy().reshape(-1).view(M.PEXT), status.cpu().numpy()
        hd = fx[cig_ref.prefix(name, level) + "hd"]
        io = in_off.cpu().numpy()
        for k, g in enumerate(xr.cpu().numpy()[:n_extra]):                         # r and r->p as mm_align1 returns them
            r, p, w = R[g], P[g], hd[g]
            assert S[g] == 0 and r["p"] == g + 1
            got = tuple(int(v) for v in (r["rs"], r["re"], r["qs"], r["qe"], p["dp_score"], p["dp_max"], r["blen"], r["mlen"], p["ambi_strand"], p["n_cigar"], p["cig0"], p["dp_max2"]))
            assert got == tuple(int(v) for v in (w[1], w[2], w[3], w[4], w[6], w[7], w[8], w[9], w[10], w[11], io[k], 0)), (name, level, names[g], got)
        nxt = cig_ref.batch(name, level + 1)[0] if level < 2 else None
        nc = int(n_child.cpu()[0])
        assert a_ref == 0 and not S.any()
        made.append(dict(u_off=u_off, regs=R.copy(), pext=P.copy(), child_of=child_of.cpu().numpy()[:nc].copy()))
        if nxt is not None:
            assert nc == len(nxt["regs"]), (name, level, nc, len(nxt["regs"]))
            got = child.cpu().numpy().reshape(-1).view(M.REG)[:nc]
            bad = [j for j in range(nc) if got[j].tobytes() != nxt["regs"][j].tobytes()]
            assert not bad, f"{name} level {level}: child {bad[0]}:\n got {got[bad[0]]}\nwant {nxt['regs'][bad[0]]}"
            of = child_of.cpu().numpy()[:nc]
            per = np.bincount(np.searchsorted(u_off, of, side="right") - 1, minlength=n_reads)
            u_off, d_regs = np.concatenate([[0], np.cumsum(per)]).astype(np.int64), child[:max(nc, 1)].contiguous()
        else:
            assert nc == 0
        for p in (fp, cp, ep, kp, ap):
            p.close()
    assert rounds == {"ont": 3, "asm20": 2}.get(name, 1)
    ref.close()
    # ---- the interleave (index arithmetic on child_of, on the host), then fin_select on the lists: the reference's final hits ----
    import mm2chain
    f_off, L, LP = mm2chain.interleave_rounds(made)
    rc = D.real_reads(name)
    n_reads = len(rc)
    assert f_off.size == n_reads + 1 and L.size == sum(m["regs"].size for m in made) == LP.size

    def same(got, gpx, want, wpx, what):
        """regions equal but for p, and the records their p name equal but for cig0 (the device's is its own CIGAR buffer's)"""
        assert got.size == want.size, what
        g, w = got.copy(), want.copy()
        gp, wp = g["p"].astype(np.int64), w["p"].astype(np.int64)
        g["p"] = 0; w["p"] = 0
        bad = [i for i in range(g.size) if g[i].tobytes() != w[i].tobytes()]
        assert not bad, f"{what}: region {bad[0]}:\n got {g[bad[0]]}\nwant {w[bad[0]]}"
        assert np.array_equal(gp != 0, wp != 0), what
        a, b = gpx[gp[gp != 0] - 1].copy(), wpx[wp[wp != 0] - 1].copy()
        a["cig0"] = 0; b["cig0"] = 0
        assert a.tobytes() == b.tobytes(), (what, a, b)
    for rd, c in enumerate(rc):                                                # the lists are the ones rebuilt from the reference's record
        same(L[f_off[rd]:f_off[rd + 1]], LP, c["regs"], c["pext"], f"{c['name']}: the list behind the loop")
    Z = np.load(os.path.join(GOLDEN, "ref_fin.npz"))
    k0 = [str(v) for v in Z["real_names"]].index(rc[0]["name"])
    plan = mm2chain.FinPlan(n_reads, L.size, LP.size, max_log_arg=1 << 16, match_sc=o["a"])
    d_px = t(LP.view(np.uint8))
    qlen = np.array([c["qlen"] for c in rc], np.int32)
    out, n_out = plan.run(_opt(D.REAL_OPT[name]), t(f_off), t(L.view(np.uint8)), t(np.diff(f_off).astype(np.int32)), d_px, t(qlen), t(np.zeros(n_reads, np.int32)))
    rcode, refused, beyond, hits = plan.counts()
    H, NO, PX = out.cpu().numpy().reshape(-1).view(M.REG), n_out.cpu().numpy(), d_px.cpu().numpy().reshape(-1).view(M.PEXT)
    assert (rcode, refused, beyond) == (0, 0, 0)
    total = 0
    for rd, c in enumerate(rc):
        lo, hi = int(Z["real_out_off"][k0 + rd]), int(Z["real_out_off"][k0 + rd + 1])
        want = Z["real_hits_out"][lo:hi].reshape(-1).view(M.REG)
        assert NO[rd] == want.size, (c["name"], NO[rd], want.size)
        wpx = c["pext"].copy()
        for tt, i in enumerate(Z["real_out_idx"][lo:hi]):                      # the reference's dp_max2 of every survivor
            wpx["dp_max2"][int(c["regs"]["p"][i]) - 1] = Z["real_out_dp_max2"][lo + tt]
        same(H[f_off[rd]:f_off[rd] + want.size], PX, want, wpx, f"{c['name']}: the final hits")
        total += want.size
    assert hits == total and total > 0
    plan.close()
