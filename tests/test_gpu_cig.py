"""The CIGAR-join plan on the device (csrc/align_cigar.hip: the rest of mm_align1, align.c:698-705, 736-764, 772-783): the batches of tests/cig_data.py through
CigPlan.second and CigPlan.join and through the two host entries, equal in every byte -- the second list, its map, the region records, the appended CIGARs, in_off,
the extra tasks -- to the model (tests/cig_model.py), with guard rows around every output and fill behind every list.  Size classes: regions of 0, 1, 2, 63, 64,
65 and 129 items; appended CIGARs of 1, 255, 256 and 257 words; merges across lanes 63 / 64, across the gather's piece and longer than a piece; a drop at item 63
and 64; j in the first and the last anchor of 129.  Every refusal with exact neighbours, each capacity exceeded by one, an empty batch, the plan's lifecycle, and the
chain AlnPlan -> KswPlan -> z-drop -> second -> KswPlan -> join -> ExtraPlan.update in device memory.  Everything is integer and compared with ==."""
import numpy as np
import pytest
import torch

import cig_data as D
import cig_model as M

pytestmark = pytest.mark.gpu
GUARD = 3
FILL = 0xee


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def cases():
    """every batch and the model's outputs of it, computed once"""
    out = {"planted": D.planted_batch()[1], "sr": D.sr_batch()}
    out.update(D.limits())
    return {k: (b, D.model(b)) for k, b in out.items()}


def t(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    if a.dtype in (np.uint32, np.uint64):
        a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
    if a.size == 0:
        a = np.zeros(16, a.dtype)
    return torch.from_numpy(a).cuda()


def score_of(B):
    return (B["mat"], 4, 2, 24, 1)


def plan_for(B, n_tasks2_cap=None, words_cap=None, extra_cap=None, cigar2_cap=None):
    from mm2chain import CigPlan
    n2 = len(B["tasks2"]) if n_tasks2_cap is None else n_tasks2_cap
    return CigPlan(len(B["aregs"]), len(B["items"]), len(B["tasks"]), len(B["cigar"]), n2, max(len(B["cigar2"]), 1) if cigar2_cap is None else cigar2_cap, len(B["pool"]), len(B["b"]),
                   int(sum(B["res"]["n_cigar"].clip(0)) + sum(B["res2"]["n_cigar"].clip(0)) + len(B["items"])) if words_cap is None else words_cap,
                   len(B["aregs"]) if extra_cap is None else extra_cap)


def guarded(n, width, dtype=torch.uint8):
    """an output array of n rows between GUARD rows, all filled"""
    if dtype == torch.uint8:
        w = torch.full((n + 2 * GUARD, width), FILL, dtype=dtype, device="cuda")
    else:
        w = torch.full((n + 2 * GUARD, torch.iinfo(dtype).bits // 8), FILL, dtype=torch.uint8, device="cuda").view(dtype).reshape(-1)
    return w, w[GUARD:GUARD + n]


def guards_ok(whole, n):
    a = whole.cpu().numpy().view(np.uint8)
    rows = a.reshape(whole.shape[0], -1)
    return bool((rows[:GUARD] == FILL).all() and (rows[GUARD + n:] == FILL).all())


def run_second(plan, B):
    from mm2chain import KSW_TASK_DTYPE
    n2, ni = plan.n_tasks2_cap, plan.n_items_cap
    t2w, t2 = guarded(max(n2, 1), KSW_TASK_DTYPE.itemsize)
    cow, co = guarded(n2 + 1, 0, torch.int64)
    sow, so = guarded(max(ni, 1), 0, torch.int32)
    plan.second(B["opt"], score_of(B), len(B["aregs"]), t(B["aregs"]), t(B["items"]), t(B["tasks"]), t(B["zres"]), t(B["pool"]) if len(B["pool"]) else None, tasks2=t2, cig_off2=co, second_of=so)
    rc, n_ref, n_over, tot = plan.second_counts()
    assert guards_ok(t2w, max(n2, 1)) and guards_ok(cow, n2 + 1) and guards_ok(sow, max(ni, 1))
    return dict(tasks2=t2.cpu().numpy().reshape(-1).view(KSW_TASK_DTYPE)[:n2], cig_off2=co.cpu().numpy(), second_of=so.cpu().numpy()[:ni], totals=tot, rc=rc, n_refused=n_ref,
                n_over=n_over, dev=(t2, co, so))


def filled(dtype, n):
    return np.full(n * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


def want_second(B, S, n2):
    """the model's second list in the layout of the device's outputs: the fill where nothing is written"""
    tk, co, so = filled(M.KSW_TASK_DTYPE, n2), filled(np.int64, n2 + 1), filled(np.int32, len(B["items"]))
    for i in range(min(n2, len(S["tasks2"]))):
        if S["written"][i]:
            tk[i], co[i] = S["tasks2"][i], S["cig_off2"][i]
    if S["totals"][0] <= n2:
        co[S["totals"][0]] = S["totals"][1]
    for R in B["aregs"]:                                                           # an item no region owns is not written
        if R["status"] == 0:
            i0, n = int(R["item0"]), int(R["n_items"])
            so[i0:i0 + n] = S["second_of"][i0:i0 + n]
    return tk, co, so


def same_second(got, B, S, n2, what=""):
    tk, co, so = want_second(B, S, n2)
    assert got["tasks2"].tobytes() == tk.tobytes(), (what, "tasks2")
    assert got["cig_off2"].tobytes() == co.tobytes(), (what, "cig_off2", got["cig_off2"][:8], co[:8])
    assert got["second_of"].tobytes() == so.tobytes(), (what, "second_of")
    assert tuple(got["totals"]) == tuple(S["totals"]) and got["n_over"] == S["n_over"], (what, got["totals"], S["totals"])


def run_join(plan, B, second=None):
    from mm2chain import CIG_REG_DTYPE, EXTRA_TASK_DTYPE
    n, wc, xc = len(B["aregs"]), plan.words_cap, plan.n_extra_cap
    crw, cr = guarded(max(n, 1), CIG_REG_DTYPE.itemsize)
    ogw, og = guarded(max(wc, 1), 0, torch.int32)
    iow, io = guarded(xc + 1, 0, torch.int64)
    xtw, xt = guarded(max(xc, 1), EXTRA_TASK_DTYPE.itemsize)
    xrw, xr = guarded(max(xc, 1), 0, torch.int32)
    co2, so = (t(B["cig_off2"]), t(B["second_of"])) if second is None else (second[1], second[2])
    pad = lambda v, k: v if v.numel() >= k else torch.cat([v, torch.zeros(k - v.numel(), dtype=v.dtype, device=v.device)])
    plan.join(B["opt"], len(B["u_off"]) - 1, n, t(B["u_off"]), t(B["regs"]), t(B["b_off"]), t(B["b"]).reshape(-1), t(B["read_off"]), t(B["aregs"]), t(B["items"]), t(B["cig_off"]),
              t(B["res"]), t(B["cigar"]), t(B["zres"]), pad(so, plan.n_items_cap), pad(co2, plan.n_tasks2_cap + 1), pad(t(B["res2"]).reshape(-1), plan.n_tasks2_cap * 48),
              pad(t(B["cigar2"]), plan.cigar2_cap), cig_regs=cr, cig_out=og, in_off=io, extra_tasks=xt, extra_reg=xr)
    rc, n_ref, n_inc, n_over, tot = plan.counts()
    assert guards_ok(crw, max(n, 1)) and guards_ok(ogw, max(wc, 1)) and guards_ok(iow, xc + 1) and guards_ok(xtw, max(xc, 1)) and guards_ok(xrw, max(xc, 1))
    return dict(cig_regs=cr.cpu().numpy().reshape(-1).view(CIG_REG_DTYPE)[:n], cig_out=og.cpu().numpy().view(np.uint32)[:wc], in_off=io.cpu().numpy(),
                extra_tasks=xt.cpu().numpy().reshape(-1).view(EXTRA_TASK_DTYPE)[:xc], extra_reg=xr.cpu().numpy()[:xc], totals=tot, rc=rc, counts=(n_ref, n_inc, n_over),
                dev=(cr, og, io, xt, xr))


def want_join(m, n, wc, xc):
    """the model's outputs in the layout of the device's: only the status word of a region that is not run, the fill behind every list"""
    cr, og, io = filled(M.CIG_REG_DTYPE, n), filled(np.uint32, wc), filled(np.int64, xc + 1)
    xt, xr = filled(M.EXTRA_TASK_DTYPE, xc), filled(np.int32, xc)
    for g in range(n):
        if m["cig_regs"][g]["status"] == 0:
            cr[g] = m["cig_regs"][g]
            c0, c = int(cr[g]["cig0"]), m["cigs"][g]
            og[c0:c0 + len(c)] = c
        elif m["cig_regs"][g]["status"] == M.OVER_CAP:
            cr[g] = m["cig_regs"][g]
        else:
            cr[g]["status"] = m["cig_regs"][g]["status"]
    k = len(m["extra_reg"])
    io[:k], xt[:k], xr[:k] = m["in_off"][:k], m["extra_tasks"], m["extra_reg"]
    if m["totals"][1] <= xc:
        io[m["totals"][1]] = m["totals"][0]
    return cr, og, io, xt, xr


def same_join(got, m, what=""):
    n, wc, xc = len(got["cig_regs"]), len(got["cig_out"]), len(got["extra_reg"])
    cr, og, io, xt, xr = want_join(m, n, wc, xc)
    for g in range(n):
        assert got["cig_regs"][g] == cr[g], (what, "region", g, got["cig_regs"][g], cr[g])
    bad = np.nonzero(got["cig_out"] != og)[0]
    assert bad.size == 0, (what, "cig_out", bad[:5], got["cig_out"][bad[:5]], og[bad[:5]])
    assert got["in_off"].tobytes() == io.tobytes() and got["extra_tasks"].tobytes() == xt.tobytes() and got["extra_reg"].tobytes() == xr.tobytes(), (what, "extra tasks")
    assert tuple(got["totals"]) == tuple(m["totals"]) and tuple(got["counts"]) == tuple(m["counts"]), (what, got["totals"], m["totals"], got["counts"], m["counts"])


@pytest.mark.parametrize("name", ["planted", "sr", "items", "words", "merges", "drops"])
def test_both_entries_equal_the_model(cases, name):
    """the second list from the device's own count, scan and emit; the join on the device's second list; twice through one plan"""
    B, m = cases[name]
    plan = plan_for(B)
    try:
        for rnd in range(2):
            S = run_second(plan, B)
            assert S["rc"] == 0 and S["n_refused"] == 0
            same_second(S, B, B["second"], plan.n_tasks2_cap, name)
            J = run_join(plan, B, second=S["dev"])
            assert J["rc"] == 0, (name, J["counts"])
            same_join(J, m, name)
        ms = plan.last_kernel_ms()
        assert len(ms) == 5 and all(x >= 0 for x in ms)
    finally:
        plan.close()


def both(B, m, what):
    plan = plan_for(B)
    try:
        S = run_second(plan, B)
        assert S["n_refused"] == 0
        same_second(S, B, B["second"], plan.n_tasks2_cap, what)
        J = run_join(plan, B, second=S["dev"])
        same_join(J, m, what)
        return J
    finally:
        plan.close()


def test_more_regions_than_one_scan_chunk():
    """the planted regions 43 times over in one call, 1 075 regions: cig_second_scan and cig_scan take them in chunks of 1 024, so the offsets of the second chunk are
    the first chunk's totals plus its own prefix sums"""
    names = D.planted_batch()[0] * 43
    _, B = D.planted_batch(names)
    assert len(B["aregs"]) > 1024 and len(B["aregs"]) % 1024 != 0 and B["second"]["totals"][0] > 0
    assert both(B, D.model(B), "1075 regions")["rc"] == 0


def test_reverse_order_option_sets_and_a_shift_that_cuts():
    """the planted regions in reverse order; under the z-drop, band and min_cnt scalars of every option set of aln_data.OPTS with q != q2 (sr has its own batch); and at
    cig_shift 4, where the slot rule of the second list differs from qlen + tlen and the long CIGARs of the word limits no longer fit their slots: those regions are
    INCOMPLETE, their neighbours exact"""
    import aln_data as AD
    names = D.planted_batch()[0]
    _, R = D.planted_batch(names[::-1])
    J = both(R, D.model(R), "reverse")
    assert J["rc"] == 0
    for name, o in AD.OPTS.items():
        if o["q"] == o["q2"] or o["flag"] & 1:
            continue
        opt = dict(zdrop=o["zdrop"], zdrop_inv=o["zdrop_inv"], bw_ext=int(o["bw"] * 1.5 + 1.), min_cnt=o["min_cnt"], flag=0, cig_shift=0)
        _, B = D.planted_batch(opt=opt)
        assert both(B, D.model(B), name)["rc"] == 0
    opt = dict(D.OPT, cig_shift=4)
    _, B = D.planted_batch(opt=opt)
    assert (np.diff(B["cig_off2"]) < B["tasks2"]["qlen"] + B["tasks2"]["tlen"]).any()                     # the second list's slots are the shifted ones
    assert both(B, D.model(B), "shift 4")["rc"] == 0
    W = D.limits(opt)["words"]
    m = D.model(W)
    assert m["counts"][1] > 0 and (m["cig_regs"]["status"] == 0).any()                                 # CIGARs longer than their slots, beside ones that fit
    assert both(W, m, "shift 4, words")["rc"] == -3


def test_planted_cases_say_what_they_plant(cases):
    B, m = cases["planted"]
    names = D.planted_batch()[0]
    r = {k: m["cig_regs"][i] for i, k in enumerate(names)}
    assert all(x["status"] == 0 for x in r.values())
    assert r["drop_split"]["split_n"] > 0 and r["drop_no_split"]["dropped"] == 1 and r["drop_no_split"]["split_n"] == 0 and r["code2_split_inv"]["split_inv"] == 1
    assert r["run65"]["n_cigar"] == 1 and r["run65"]["n_used"] == 70 and r["merge"]["n_cigar"] == 3 and r["no_merge"]["n_cigar"] == 4 and r["inside_item"]["n_cigar"] == 4
    assert r["bad_behind_cut"]["n_used"] == 2 and r["over_gap"]["dropped"] == 1 and r["rev"]["r_qs"] != r["rev"]["qs1"]


def test_one_region_per_call_and_the_host_entries(cases):
    from mm2chain import second_pass_batch, assemble_regions_batch
    P = D.planted()
    for name in ("both_ext", "merge", "drop_split", "code2_split_inv", "rev_drop", "over_gap", "j_clamp"):
        B = D.build([P[name]])
        plan = plan_for(B)
        J = run_join(plan, B)
        same_join(J, D.model(B), name)
        plan.close()
    for name in ("planted", "sr"):
        B, m = cases[name]
        n2 = len(B["tasks2"])
        S = second_pass_batch(B["opt"], score_of(B), B["aregs"], B["items"], B["tasks"], B["zres"], B["pool"], n2, fill=FILL)
        assert S["rc"] == 0
        same_second(dict(S, n_over=0), B, B["second"], n2, name)
        wc, xc = m["totals"][0] + 5, m["totals"][1] + 2
        J = assemble_regions_batch(B["opt"], B["u_off"], B["regs"], B["b_off"], B["b"], B["read_off"], B["aregs"], B["items"], B["cig_off"], B["res"], B["cigar"], B["zres"], S["second_of"],
                                   S["cig_off2"], B["res2"], B["cigar2"], wc, xc, fill=FILL)
        assert J["rc"] == 0
        same_join(dict(J, counts=(0, 0, 0)), m, name)


def mutate(B, **kw):
    C = dict(B)
    for k in ("aregs", "items", "res", "zres", "second_of", "cigar", "read_off", "res2", "cig_off"):
        C[k] = B[k].copy()
    return C


def test_every_refusal_keeps_its_neighbours_exact(cases):
    """each refusal planted into one region of the planted batch: its status and count are the model's, which implements the same rules, and every other region, every
    word and every extra task stay exact"""
    B0, _ = cases["planted"]
    names = D.planted_batch()[0]
    g_of = lambda n: names.index(n)
    item_of = lambda n, k: int(B0["aregs"][g_of(n)]["item0"]) + k
    task_of = lambda n, k: int(B0["items"][item_of(n, k)]["task"])
    plan = plan_for(B0)
    muts = []

    def m_(what, name, status, f):
        C = mutate(B0)
        f(C)
        muts.append((what, g_of(name), status, C))
    m_("aln status", "merge", M.REFUSED, lambda C: C["aregs"].__setitem__(g_of("merge"), np.array((0,) * 12 + (2, 0) + (0,) * 6, M.ALN_REG_DTYPE)))
    m_("code 3", "both_ext", M.REFUSED, lambda C: C["zres"]["code"].__setitem__(task_of("both_ext", 1), 3))
    m_("zres status", "both_ext", M.REFUSED, lambda C: C["zres"]["status"].__setitem__(task_of("both_ext", 2), 1))
    m_("second where code 0", "no_left", M.REFUSED, lambda C: C["second_of"].__setitem__(item_of("no_left", 0), 0))
    m_("item0 leaves items", "no_right", M.REFUSED, lambda C: C["aregs"]["item0"].__setitem__(g_of("no_right"), len(B0["items"]) - 1))
    m_("task out of range", "no_right", M.REFUSED, lambda C: C["items"]["task"].__setitem__(item_of("no_right", 1), len(B0["tasks"])))
    m_("lengths do not add up", "merge", M.REFUSED, lambda C: C["cigar"].__setitem__(int(B0["cig_off"][task_of("merge", 2)]), (61 << 4)))
    m_("qe1 > qlen", "rev_drop", M.REFUSED, lambda C: C["read_off"].__setitem__(slice(g_of("rev_drop") // 3 + 1, None), C["read_off"][g_of("rev_drop") // 3 + 1:] - 130))
    for st in (1, 2, 3):
        m_(f"ksw status {st}", "drop_split", M.INCOMPLETE, lambda C, st=st: C["res"]["status"].__setitem__(task_of("drop_split", 1), st))
    m_("n_cigar beyond its slot", "no_merge", M.INCOMPLETE, lambda C: C["res"]["n_cigar"].__setitem__(task_of("no_merge", 0), 5000))
    m_("code 1 without a second pass", "code1", M.INCOMPLETE, lambda C: C["second_of"].__setitem__(item_of("code1", 1), -1))
    m_("second pass without room", "code1", M.INCOMPLETE, lambda C: C["second_of"].__setitem__(item_of("code1", 1), M.NO_ROOM))
    m_("second pass beyond the second list", "code1", M.REFUSED, lambda C: C["second_of"].__setitem__(item_of("code1", 1), len(B0["tasks2"])))
    m_("re1 - rs1 > re0 - rs0", "both_ext", M.REFUSED, lambda C: C["aregs"]["re0"].__setitem__(g_of("both_ext"), int(B0["aregs"]["rs0"][g_of("both_ext")]) + 1))
    m_("a CIGAR offset leaves the ksw plan's words", "j_eq", M.REFUSED, lambda C: C["cig_off"].__setitem__(task_of("j_eq", 2) + 1, len(B0["cigar"]) + 5))
    m_("second pass not run", "second_differs", M.INCOMPLETE, lambda C: C["res2"]["status"].__setitem__(int(B0["second_of"][item_of("second_differs", 1)]), 2))
    try:
        for what, g, status, C in muts:
            m = D.model(C)
            assert m["cig_regs"][g]["status"] == status and sum(m["counts"]) >= 1, (what, m["cig_regs"][g], m["counts"])
            J = run_join(plan, C)
            assert J["rc"] == (-2 if status == M.REFUSED else -3), what
            same_join(J, m, what)
        # a bad task behind the cut changes nothing: the same batch with those statuses 0 gives the same bytes
        J = run_join(plan, B0)
        assert J["rc"] == 0 and J["cig_regs"][g_of("bad_behind_cut")]["status"] == 0
        C = mutate(B0)
        bad = [task_of("bad_behind_cut", k) for k in (2, 3, 4)]
        assert sorted(int(C["res"]["status"][i]) + int(C["zres"]["status"][i]) for i in bad) == [1, 1, 2]
        C["res"]["status"][bad] = 0; C["zres"]["status"][bad] = 0
        G = run_join(plan, C)
        for k in ("cig_regs", "cig_out", "in_off", "extra_tasks", "extra_reg"):
            assert G[k].tobytes() == J[k].tobytes(), k
    finally:
        plan.close()


def test_one_anchor_without_sr_and_an_ungapped_item_off_the_pool(cases):
    """cnt1 == 1 without sr: the gap loop never runs, so the right extension starts at the region's re / qe while rs1 / qs1 stay at rs / qs, and the appended CIGAR does
    not add up (:284): REFUSED, its neighbours exact.  An sr ungapped item whose bases leave the pool: the second-pass entry counts it and marks it MM2C_CIG_LOST, and
    the join refuses its region instead of taking it for an item that passed its test"""
    P = D.planted()
    B = D.build([P["both_ext"], D.region([], right=D.ez("7M")), P["merge"]])
    k = int(B["aregs"][1]["item0"])
    assert B["aregs"][1]["cnt1"] == 1 and B["aregs"][1]["n_items"] == 1 and B["items"][k]["kind"] == M.RIGHT
    for f in ("rs", "re", "qs", "qe"):                                             # as mm_align1 has it: re = rs + k, qe = qs + k of the one anchor
        B["items"][k][f] += 15
    B["aregs"][1]["re0"] += 15; B["aregs"][1]["qe0"] += 15
    m = D.model(B)
    assert m["cig_regs"]["status"].tolist() == [0, M.REFUSED, 0]
    plan = plan_for(B)
    J = run_join(plan, B)
    assert J["rc"] == -2
    same_join(J, m, "cnt1 == 1")
    plan.close()
    S0, _ = cases["sr"]
    S = dict(S0, aregs=S0["aregs"].copy())
    S["aregs"]["q_off"][1] = len(S0["pool"]) - 20                                  # region 1's ungapped item now leaves the pool
    ms = M.second_pass(S["opt"], S["aregs"], S["items"], S["tasks"], S["zres"], S["pool"], S["mat"])
    assert ms["n_lost"] == 1 and (ms["second_of"] == M.LOST).sum() == 1
    plan = plan_for(S0)
    G = run_second(plan, S)
    assert G["rc"] == -2 and G["n_refused"] == 1
    same_second(G, S, ms, plan.n_tasks2_cap, "lost")
    S = dict(S, second_of=ms["second_of"])
    mj = D.model(S)
    assert mj["cig_regs"]["status"].tolist() == [0, M.REFUSED, 0, 0]
    same_join(run_join(plan, S, second=G["dev"]), mj, "lost")
    plan.close()


def test_capacities_exceeded_by_one_and_an_empty_batch(cases):
    B, m = cases["planted"]
    tot_w, tot_x = m["totals"]
    for wc, xc in ((tot_w - 1, tot_x), (tot_w, tot_x - 1), (40, tot_x), (tot_w, tot_x)):
        plan = plan_for(B, words_cap=wc, extra_cap=xc)
        J = run_join(plan, B)
        mm = D.model(B, words_cap=wc, extra_cap=xc)
        assert tuple(J["totals"]) == (tot_w, tot_x) and J["rc"] == (0 if mm["counts"][2] == 0 else -3)
        assert (mm["counts"][2] > 0) == ((wc, xc) != (tot_w, tot_x))
        same_join(J, mm, f"caps {wc} {xc}")
        plan.close()
    n2 = len(B["tasks2"])
    for cap in (n2 - 1, 1, 0):
        plan = plan_for(B, n_tasks2_cap=cap)
        S = run_second(plan, B)
        ms = M.second_pass(B["opt"], B["aregs"], B["items"], B["tasks"], B["zres"], B["pool"], B["mat"], n_tasks2_cap=cap)
        assert S["rc"] == -3 and ms["n_over"] > 0 and (ms["second_of"] == M.NO_ROOM).any()
        same_second(S, B, ms, cap, f"second cap {cap}")
        plan.close()
    w2 = int(B["cig_off2"][-1])
    plan = plan_for(B, cigar2_cap=w2 - 1)                                          # the second list's words leave cigar2_cap by one
    S = run_second(plan, B)
    ms = M.second_pass(B["opt"], B["aregs"], B["items"], B["tasks"], B["zres"], B["pool"], B["mat"], cigar2_cap=w2 - 1)
    assert S["rc"] == -3 and ms["n_over"] == 1 and tuple(S["totals"]) == (n2, w2)
    same_second(S, B, ms, n2, "cigar2_cap")
    plan.close()
    # an empty batch: only in_off[0] and cig_off2[0]
    plan = plan_for(B)
    E = dict(B, aregs=B["aregs"][:0], u_off=np.zeros(1, np.int64), b_off=np.zeros(1, np.int64), read_off=np.zeros(1, np.int64), regs=B["regs"][:0])
    S = run_second(plan, E)
    assert S["rc"] == 0 and S["cig_off2"][0] == 0 and (S["cig_off2"][1:].view(np.uint8) == FILL).all() and (S["second_of"].view(np.uint8) == FILL).all()
    J = run_join(plan, E)
    assert J["rc"] == 0 and J["in_off"][0] == 0 and (J["in_off"][1:].view(np.uint8) == FILL).all() and (J["cig_out"].view(np.uint8) == FILL).all() and tuple(J["totals"]) == (0, 0)
    plan.close()


def _launches():
    import ctypes as C
    from mm2chain import _native as N
    st = N.Stats()
    N.load().mm2c_get_stats(C.byref(st))
    return int(st.launches)


def test_lifecycle(cases):
    """zeros and "has not been run" before a run, close twice, two equal runs, and the launches a run adds: cig_second_count, its scan, cig_second_emit; cig_cut, cig_scan,
    cig_gather"""
    import mm2chain
    B, m = cases["planted"]
    plan = plan_for(B)
    assert plan.counts() == (0, 0, 0, 0, (0, 0)) and plan.second_counts() == (0, 0, 0, (0, 0))
    with pytest.raises(mm2chain.Mm2cError, match=r"code -2\).*has not been run"):
        plan.last_kernel_ms()
    idle = plan_for(B)
    idle.close(); idle.close()
    assert idle.handle is None
    del idle
    at = _launches()
    S1 = run_second(plan, B)
    assert _launches() - at == 3
    at = _launches()
    J1 = run_join(plan, B, second=S1["dev"])
    assert _launches() - at == 3
    ms = plan.last_kernel_ms()
    assert all(x >= 0 for x in ms)
    S2 = run_second(plan, B)
    J2 = run_join(plan, B, second=S2["dev"])
    for k in ("tasks2", "cig_off2", "second_of"):
        assert S1[k].tobytes() == S2[k].tobytes()
    for k in ("cig_regs", "cig_out", "in_off", "extra_tasks", "extra_reg"):
        assert J1[k].tobytes() == J2[k].tobytes()
    same_join(J2, m, "second run")
    at = _launches()
    E = dict(B, aregs=B["aregs"][:0], u_off=np.zeros(1, np.int64), b_off=np.zeros(1, np.int64), read_off=np.zeros(1, np.int64), regs=B["regs"][:0])
    run_second(plan, E); run_join(plan, E)
    assert _launches() - at == 0
    plan.close(); plan.close()


@pytest.mark.parametrize("name,level", [("ont", 0), ("ont", 1), ("ont", 2), ("asm20", 0), ("asm20", 1), ("ont_noflt", 0), ("ont_g300", 0), ("ont_sw", 0), ("ont_sw", 1), ("ont_sw", 2),
                                        ("sr", 0), ("hpc", 0)])
def test_both_entries_on_the_reference_record(name, level):
    """the recorded ez and CIGAR words of the reference's own mm_align1 (tests/golden/ref_cig.npz through tests/cig_ref.py) as the join's inputs, for the regions of
    tests/cig_data.ref_batches() and (level 1, 2) for the regions the reference split off them: the second list is the calls the reference made, every output byte
    equals the model's, and the record's CIGAR and dp_score in front of mm_update_extra, has_p, the split, r2 and the final region come out; a task the reference
    never called (behind a drop) carries ksw status 1 and changes nothing"""
    import cig_ref
    B, names = cig_ref.batch(name, level)
    assert len(B["aregs"]) > 0
    m = cig_ref.model_of(name, level)
    J = both(B, m, name)
    assert J["rc"] == (0 if m["counts"][0] == 0 else -2)
    cigs = [J["cig_out"][int(r["cig0"]):int(r["cig0"]) + int(r["n_cigar"])] if r["status"] == 0 else None for r in J["cig_regs"]]
    bad = cig_ref.mismatches(name, B, J["cig_regs"], cigs, level)
    assert not bad, (name, len(bad), [(names[x[0]],) + tuple(x[1:]) for x in bad[:5]])


@pytest.mark.parametrize("name", ["ont", "asm20", "ont_g300", "ont_sw", "sr"])
def test_the_chain_in_device_memory(name):
    """AlnPlan -> KswPlan -> ExtraPlan.zdrop -> CigPlan.second -> KswPlan -> CigPlan.join -> ExtraPlan.update on the regions of tests/cig_data.ref_batches(): every array
    goes from one plan into the next as it lies on the GPU (only the totals of each check come to the host in between, and the codes 2 of the record go up for the
    tasks whose ksw_ll_i16 the host would run: no CIGAR word).  The final regions equal the reference's r and r->p (tests/golden/ref_cig.npz): rs, re, qs, qe,
    dp_score, dp_max, blen, mlen, n_ambi, n_cigar and the words out of ExtraPlan.update, the split and r2 out of the join.  A region the join splits goes through the
    Python mm_split_reg (float32) and a second and a third round over the same anchors, flags in place, equal the records of the regions the reference split off."""
    import aln_data as AD
    import cig_ref
    from mm2chain import (AlnPlan, KswPlan, ExtraPlan, CigPlan, RefSeq, params, ksw_task_scratch, KSW_RES_DTYPE, CIG_REG_DTYPE, EXTRA_RES_DTYPE)
    fx = cig_ref.fixture()
    o = D.cached_ref_batches()[name][0]
    aopt = params.aln_opts(**{k: o[k] for k in o if k not in ("q2", "sc_ambi")})
    score = params.ksw_scores("map-ont", a=o["a"], b=o["b"], q=o["q"], e=o["e"], q2=o["q2"], e2=o["e2"], sc_ambi=o["sc_ambi"])
    ref = RefSeq(*AD.reference())
    h = lambda x, dt, n: x.cpu().numpy().reshape(-1).view(dt)[:n]
    d_b, prev, rounds = None, None, 0
    for level in range(3):
        B, names = cig_ref.batch(name, level)
        u_off, b_off, read_off, fwd = B["u_off"], B["b_off"], B["read_off"], cig_ref.inputs(name, 0)[6]
        n_reads, n_regs = len(u_off) - 1, int(u_off[-1])
        if level == 0:
            regs = cig_ref.inputs(name, 0)[2]
            d_b = t(cig_ref.inputs(name, 0)[4]).reshape(-1)
        else:                                                                      # the split, from what the device's join of the level above said
            pB, pR = prev
            anchors = d_b.cpu().numpy().view(np.uint64).reshape(-1, 2)
            regs = []
            for rd in range(n_reads):
                a = anchors[int(b_off[rd]):int(b_off[rd + 1])]
                for g in range(int(pB["u_off"][rd]), int(pB["u_off"][rd + 1])):
                    if pR[g]["status"] == 0 and pR[g]["split_n"] > 0:
                        regs.append(cig_ref.split_reg(pB["regs"][g], int(pR[g]["split_n"]), int(pR[g]["split_inv"]), int(read_off[rd + 1] - read_off[rd]), a))
            regs = np.array(regs, AD.REG_DTYPE).reshape(-1) if regs else np.zeros(0, AD.REG_DTYPE)
            assert regs.tobytes() == B["regs"].tobytes(), (name, level, "the split regions are not the recorded ones")
        if n_regs == 0:
            break
        rounds += 1
        tot = (len(B["items"]), len(B["tasks"]), int(B["cig_off"][-1]), len(B["pool"]))
        n_b = d_b.numel() // 2
        # slots of the largest task and of the longest CIGAR, so that nothing is too big for the ksw plan or the extra plan
        slot = max([ksw_task_scratch(int(T["qlen"]), int(T["tlen"]), int(T["w"]), int(T["flag"]) & ~8) for T in B["tasks"]] + [1 << 20])
        ap = AlnPlan(n_regs, tot[0], tot[1], tot[3], n_b, fwd.size, cig_shift=0, n_slots=64)
        kp = KswPlan(tot[1], tot[3], tot[2], n_slots=32, slot_bytes=slot)
        ep = ExtraPlan(max(tot[1], n_regs), tot[3], tot[2], tot[2], n_slots=32, slot_words=min(max(tot[2], 16), 1 << 18))
        cp = CigPlan(n_regs, tot[0], tot[1], tot[2], tot[1], tot[2], tot[3], n_b, tot[2], n_regs)
        d_u, d_regs, d_bo, d_ro = t(u_off), t(regs), t(b_off), t(read_off)
        ar, items, tasks, cig_off, pool = ap.run(aopt, ref, n_reads, n_regs, d_u, d_regs, d_bo, d_b, d_ro, t(fwd))
        assert ap.counts()[:3] == (0, 0, 0)
        res, cigar = kp.run(score, tot[1], tasks, pool, cig_off)
        assert kp.counts() == (0, 0, 0)
        zres = ep.zdrop(score, dict(zdrop=o["zdrop"], zdrop_inv=o["zdrop_inv"], max_gap=o["max_gap"], no_inv=o["flag"] & 1), tot[1], tasks, pool, cig_off, res, cigar)
        two = np.nonzero(B["zres"]["code"] == 2)[0]
        if two.size:                                                               # ksw_ll_i16 is the host's: its verdict comes from the record
            zres.view(torch.int32).reshape(-1, 8)[torch.from_numpy(two).cuda(), 5] = 2
        tasks2, cig_off2, second_of = cp.second(B["opt"], score, n_regs, ar, items, tasks, zres, pool)
        n2, w2 = cp.second_check()
        res2 = torch.zeros((max(tot[1], 1), KSW_RES_DTYPE.itemsize), dtype=torch.uint8, device="cuda")  # of the second list's capacity, as the join takes it
        res2, cigar2 = kp.run(score, n2, tasks2, pool, cig_off2, res=res2)
        cig_regs, cig_out, in_off, xt, xr = cp.join(B["opt"], n_reads, n_regs, d_u, d_regs, d_bo, d_b, d_ro, ar, items, cig_off, res, cigar, zres, second_of, cig_off2, res2, cigar2)
        rc, n_ref, n_inc, n_over, (words, n_extra) = cp.counts()
        # the device lists a second pass for every item whose test asks for one, also behind a drop, where the reference makes no call: a superset of the recorded ones
        assert (n_ref, n_inc, n_over) == (int((B["aregs"]["status"] != 0).sum()), 0, 0) and n2 >= len(B["tasks2"])
        xres, xcig = ep.update(score, 0, n_extra, xt, pool, in_off, cig_out, in_off)
        assert ep.counts()[0] == 0
        R, X, xg, io = h(cig_regs, CIG_REG_DTYPE, n_regs), h(xres, EXTRA_RES_DTYPE, n_extra), xr.cpu().numpy()[:n_extra], in_off.cpu().numpy()[:n_extra + 1]
        co, xc = cig_out.cpu().numpy().view(np.uint32), xcig.cpu().numpy().view(np.uint32)
        cigs = [co[int(r["cig0"]):int(r["cig0"]) + int(r["n_cigar"])] if r["status"] == 0 else None for r in R]
        bad = cig_ref.mismatches(name, B, R, cigs, level)
        assert not bad, (name, level, len(bad), [(names[x[0]],) + tuple(x[1:]) for x in bad[:5]])
        pf = cig_ref.prefix(name, level)
        hd, fin, fin_off = fx[pf + "hd"], fx[pf + "fin"], fx[pf + "fin_off"]
        assert n_extra == int(((hd[:, 11] > 0) & (B["aregs"]["status"] == 0)).sum())
        for k, g in enumerate(xg):                                                 # r and r->p as ExtraPlan.update leaves them
            O, x, w = R[g], X[k], hd[g]
            rs, re = int(O["rs1"]) + int(x["tshift"]), int(O["re1"])
            qs, qe = (int(O["r_qs"]), int(O["r_qe"]) - int(x["qshift"])) if B["aregs"][g]["rev"] else (int(O["r_qs"]) + int(x["qshift"]), int(O["r_qe"]))
            got = (rs, re, qs, qe, int(O["dp_score"]), int(x["dp_max"]), int(x["blen"]), int(x["mlen"]), int(x["n_ambi"]), int(x["n_cigar"]), int(x["status"]))
            assert got == tuple(int(v) for v in (w[1], w[2], w[3], w[4], w[6], w[7], w[8], w[9], w[10], w[11], 0)), (name, level, names[g], got)
            assert xc[int(io[k]):int(io[k]) + int(x["n_cigar"])].tolist() == fin[int(fin_off[g]):int(fin_off[g + 1])].tolist(), (name, level, names[g])
        print(f"chain {name} level {level}: {n_regs} regions, {tot[1]} tasks, {n2} second passes, {int(R['dropped'].sum())} dropped, {int((R['split_n'] > 0).sum())} split, {words} words")
        prev = (B, R.copy())
        for p in (cp, ep, kp, ap):
            p.close()
    assert rounds == {"ont": 3, "asm20": 2, "ont_sw": 3}.get(name, 1)
    ref.close()
