"""Fragment hits per segment on the device (csrc/chain_hits.hip: mm_select_sub_multi pe.c:6-43; csrc/chain_segs.hip: mm_seg_gen hit.c:373-427): every case of
tests/seg_data.py through HitPlan.run_multi / select_hits_multi_batch and SegPlan.run / seg_gen_batch, byte for byte against what the reference's own hit.o and pe.o
made of it (tests/golden/ref_seg.npz) -- in batches in two orders through one plan that is reused, one fragment per call, and through the host entries; the five plans
RegPlan -> HitPlan.run_multi -> SegPlan -> HitPlan (pri_ratio 0) -> MapqPlan (do_join 0) on one stream without a host synchronisation between them; pairs of mixed
lengths from reads to final per-segment regions against the models on the reference's chains; every kind of refusal with exact neighbours and guard rows; and a
plan run again on other data of another size and order."""
import os

import numpy as np
import pytest
import torch

import regs_model
import seg_data as D
import seg_model as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REG = regs_model.REG
FILL, GUARD = 0xee, 3


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def ref():
    R = D.reference()
    assert R is not None, "tests/golden/ref_seg.npz is absent"
    for r in R:                                                                 # the hit plan's input: the regions as the region plan writes them (model of mm_gen_regs)
        c = r["case"]
        r["regs0"] = regs_model.gen_regs(c["hash"], int(c["qlens"].sum()), c["u"], c["a"])
    return R


def t(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def guarded(rows, width, dtype, fill):
    """-> (the whole tensor, the view the plan gets): GUARD rows in front and behind"""
    shape = (rows + 2 * GUARD, width) if width else (rows + 2 * GUARD,)
    whole = torch.full(shape, fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + rows]


def guards_untouched(whole, fill):
    h = whole.cpu().numpy()
    return (h[:GUARD] == (fill if h.dtype != np.uint8 else fill & 0xff)).all() and (h[-GUARD:] == (fill if h.dtype != np.uint8 else fill & 0xff)).all()


def _hit_opt(c, **kw):
    from mm2chain import params
    o = dict(c["hit"]); o.update(kw)
    return params.hit_opts(**o)


def _multi_opt(c):
    from mm2chain import params
    return params.hit_multi_opts(c["n_segs"], 12345, c["multi"]["pri1"], c["multi"]["pri2"])      # max_gap_ref: never used, d_gap_ref is given


def _frag_batch(rs, n_frags, regs_key):
    """the fragments one after another, each with room for as many regions as it has chains (the regions lie in front, the rest is filler); padded with empty
    fragments.  regs_key: "regs0" (the hit plan's input) or "sel" (the seg plan's)"""
    n_segs = rs[0]["case"]["n_segs"]
    pad = n_frags - len(rs)
    room = [R["case"]["u"].size for R in rs] + [0] * pad
    nb = [R["case"]["a"].shape[0] for R in rs] + [0] * pad
    u_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64); b_off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    regs = np.full((max(int(u_off[-1]), 1), 80), FILL, np.uint8)
    for k, R in enumerate(rs):
        regs[u_off[k]:u_off[k] + R[regs_key].size] = R[regs_key].view(np.uint8).reshape(-1, 80)
    ints = lambda v, fill: np.array(list(v) + [fill] * pad, np.int32)
    return {"n_segs": n_segs, "u_off": u_off, "b_off": b_off, "regs": regs, "b": np.concatenate([R["case"]["a"] for R in rs] + [np.zeros((0, 2), np.uint64)]),
            "u": np.concatenate([R["case"]["u"] for R in rs] + [np.zeros(0, np.uint64)]),
            "n_in": ints([R[regs_key].size for R in rs], 0), "seg_len": np.concatenate([D.seg_len([R["case"] for R in rs]), np.full(pad * n_segs, 100, np.int32)]),
            "gap_ref": ints([R["case"]["gap_ref"] for R in rs], 500), "hash": np.array([R["case"]["hash"] for R in rs] + [7] * pad, np.uint32),
            "rep_len": ints([R["case"]["rep_len"] for R in rs], 0), "qlen_sum": ints([int(R["case"]["qlens"].sum()) for R in rs], 200)}


def _padded(a, rows, fill=0):
    out = np.full((max(rows, 1),) + a.shape[1:], fill, a.dtype)
    out[:a.shape[0]] = a
    return out


# ---------------------------------------------------------------- mm_select_sub_multi ----------------------------------------------------------------
def _run_sel(plan, rs, B):
    whole_r, out = guarded(max(plan.n_u_cap, 1), 80, torch.uint8, FILL)
    whole_n, n_out = guarded(plan.n_reads, 0, torch.int32, -9)
    c = rs[0]["case"]
    plan.run_multi(_hit_opt(c), _multi_opt(c), t(B["u_off"]), t(B["seg_len"]), t(_padded(B["regs"], plan.n_u_cap, FILL)), t(B["gap_ref"]), regs_out=out, n_out=n_out)
    total = plan.check()
    assert guards_untouched(whole_r, FILL) and guards_untouched(whole_n, -9)
    return out.cpu().numpy(), n_out.cpu().numpy(), total


def _assert_sel(got, B, rs, what):
    out, n_out, total = got
    for k, R in enumerate(rs):
        w = R["sel"]
        assert n_out[k] == w.size, f"{what}: {R['name']}: n_out = {n_out[k]}, the reference {w.size}"
        g = out[B["u_off"][k]:B["u_off"][k] + w.size].reshape(-1).view(REG)
        bad = [i for i in range(w.size) if g[i].tobytes() != w[i].tobytes()]
        assert not bad, f"{what}: {R['name']}: {len(bad)} of {w.size} hits differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {w[bad[0]]}"
    assert (n_out[len(rs):] == 0).all()
    if total is not None:
        assert total == sum(R["sel"].size for R in rs)


def test_select_sub_multi_every_case_in_batches_alone_and_through_the_host_entry(ref):
    import mm2chain
    groups = D.groups()
    n_frags = max(len(g) for g in groups)
    plan = mm2chain.HitPlan(n_frags, max(sum(ref[k]["case"]["u"].size for k in g) for g in groups))
    one = mm2chain.HitPlan(1, max(R["case"]["u"].size for R in ref))
    seen = 0
    try:
        for g in groups:
            for order in (g, g[::-1]):
                rs = [ref[k] for k in order]
                B = _frag_batch(rs, n_frags, "regs0")
                _assert_sel(_run_sel(plan, rs, B), B, rs, "HitPlan.run_multi, one batch")
            assert plan.last_ms() > 0
            rs = [ref[k] for k in g]
            for R in rs:
                B1 = _frag_batch([R], 1, "regs0")
                _assert_sel(_run_sel(one, [R], B1), B1, [R], "HitPlan.run_multi, one fragment per call")
            Bh = _frag_batch(rs, len(rs), "regs0")
            c = rs[0]["case"]
            h = mm2chain.select_hits_multi_batch(_hit_opt(c), _multi_opt(c), Bh["u_off"], Bh["seg_len"], Bh["regs"], Bh["gap_ref"])
            assert h[0].dtype == mm2chain.REG_DTYPE and h[1].dtype == np.int32
            _assert_sel((h[0].view(np.uint8).reshape(-1, 80), h[1], None), Bh, rs, "select_hits_multi_batch")
            seen += len(g)
    finally:
        plan.close(); one.close()
    assert seen == len(ref)
    # two fragments of one batch, one geometry, that differ only in gap_ref decide differently -- and mopt.max_gap_ref serves when d_gap_ref is NULL
    by = {R["name"]: R for R in ref}
    rs = [by["sel_gap_ref_500"], by["sel_gap_ref_499"]]
    assert rs[0]["sel"].size == 2 and rs[1]["sel"].size == 1
    B = _frag_batch(rs, 2, "regs0")
    from mm2chain import params
    for gap, want in ((500, [2, 2]), (499, [1, 1])):
        h = mm2chain.select_hits_multi_batch(_hit_opt(rs[0]["case"]), params.hit_multi_opts(2, gap), B["u_off"], B["seg_len"], B["regs"], None)
        assert h[1].tolist() == want


# ---------------------------------------------------------------- mm_seg_gen ----------------------------------------------------------------
def _seg_out(plan):
    ns = max(plan.n_seg_reads, 1)
    w = {"su_off": guarded(ns + 1, 0, torch.int64, -5), "sb_off": guarded(ns + 1, 0, torch.int64, -5), "su": guarded(max(plan.n_su_cap, 1), 0, torch.int64, -3),
         "sb": guarded(max(plan.n_b_cap, 1), 2, torch.int64, -3), "seg_regs": guarded(max(plan.n_su_cap, 1), 80, torch.uint8, FILL),
         "seg_hash": guarded(ns, 0, torch.int32, -7), "seg_rep_len": guarded(ns, 0, torch.int32, -7)}
    return {k: v[0] for k, v in w.items()}, {k: v[1] for k, v in w.items()}


FILLS = {"su_off": -5, "sb_off": -5, "su": -3, "sb": -3, "seg_regs": FILL, "seg_hash": -7, "seg_rep_len": -7}


def _run_seg(plan, B):
    whole, out = _seg_out(plan)
    d_regs, d_b = t(_padded(B["regs"], plan.n_u_cap, FILL)), t(_padded(B["b"], plan.n_b_cap))
    plan.run(t(B["u_off"]), d_regs, t(B["n_in"]), t(B["b_off"]), d_b, t(B["seg_len"]), t(B["hash"]), t(B["rep_len"]), out=out)
    rc, n_ref, nu, na = plan.counts()
    for k, w in whole.items():
        assert guards_untouched(w, FILLS[k]), f"guard rows of {k} were written"
    assert np.array_equal(d_regs.cpu().numpy(), _padded(B["regs"], plan.n_u_cap, FILL)) and np.array_equal(d_b.cpu().numpy().view(np.uint64), _padded(B["b"], plan.n_b_cap))
    h = {k: v.cpu().numpy() for k, v in out.items()}
    h["su"], h["sb"], h["seg_hash"] = h["su"].view(np.uint64), h["sb"].view(np.uint64), h["seg_hash"].view(np.uint32)
    return h, (rc, n_ref, nu, na)


def _assert_seg(h, rs, n_segs, what, skip=()):
    for f, R in enumerate(rs):
        if f in skip:
            continue
        for s, S in enumerate(R["segs"]):
            k = f * n_segs + s
            u0, u1, b0, b1 = (int(v) for v in (h["su_off"][k], h["su_off"][k + 1], h["sb_off"][k], h["sb_off"][k + 1]))
            assert u1 - u0 == S["u"].size and b1 - b0 == S["a"].shape[0], f"{what}: {R['name']} segment {s}: {u1 - u0} chains, {b1 - b0} anchors; the reference {S['u'].size}, {S['a'].shape[0]}"
            assert np.array_equal(h["su"][u0:u1], S["u"]), f"{what}: {R['name']} segment {s}: u differs"
            assert np.array_equal(h["sb"][b0:b1], S["a"]), f"{what}: {R['name']} segment {s}: a differs at {np.nonzero((h['sb'][b0:b1] != S['a']).any(axis=1))[0][:5]}"
            g = h["seg_regs"][u0:u1].reshape(-1).view(REG) if h["seg_regs"].dtype == np.uint8 else h["seg_regs"][u0:u1]
            bad = [i for i in range(S["regs"].size) if g[i].tobytes() != S["regs"][i].tobytes()]
            assert not bad, f"{what}: {R['name']} segment {s}: {len(bad)} of {S['regs'].size} regions differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {S['regs'][bad[0]]}"
            assert h["seg_hash"][k] == R["case"]["hash"] and (h["seg_rep_len"] is None or h["seg_rep_len"][k] == R["case"]["rep_len"])


def test_seg_gen_every_case_in_batches_alone_and_through_the_host_entry(ref):
    import mm2chain
    seen = 0
    for n_segs in (2, 3):
        idx = [k for k, R in enumerate(ref) if R["case"]["n_segs"] == n_segs]
        n_frags = len(idx) + 2
        plan = mm2chain.SegPlan(n_frags, n_segs, sum(ref[k]["case"]["u"].size for k in idx) + 5, sum(ref[k]["case"]["a"].shape[0] for k in idx) + 9)
        one = mm2chain.SegPlan(1, n_segs, max(ref[k]["case"]["u"].size for k in idx), max(ref[k]["case"]["a"].shape[0] for k in idx))
        try:
            for order in (idx, idx[::-1]):
                rs = [ref[k] for k in order]
                h, (rc, n_refused, nu, na) = _run_seg(plan, _frag_batch(rs, n_frags, "sel"))
                assert (rc, n_refused) == (0, 0)
                _assert_seg(h, rs, n_segs, "SegPlan.run, one batch")
                assert nu == h["su_off"][n_frags * n_segs] == sum(S["u"].size for R in rs for S in R["segs"])
                assert na == h["sb_off"][n_frags * n_segs] == sum(S["a"].shape[0] for R in rs for S in R["segs"])
                assert (np.diff(h["su_off"][len(rs) * n_segs:n_frags * n_segs + 1]) == 0).all()
            assert plan.last_ms() > 0 and len(plan.last_kernel_ms()) == 5 and plan.last_kernel_ms()[0] > 0
            for k in idx:
                h, (rc, n_refused, _, _) = _run_seg(one, _frag_batch([ref[k]], 1, "sel"))
                assert (rc, n_refused) == (0, 0)
                _assert_seg(h, [ref[k]], n_segs, "SegPlan.run, one fragment per call")
            rs = [ref[k] for k in idx]
            B = _frag_batch(rs, len(rs), "sel")
            for with_rep in (True, False):
                h = mm2chain.seg_gen_batch(n_segs, B["u_off"], B["regs"], B["n_in"], B["b_off"], B["b"], B["seg_len"], B["hash"], B["rep_len"] if with_rep else None)
                assert h["seg_regs"].dtype == mm2chain.REG_DTYPE and (h["seg_rep_len"] is None) == (not with_rep)
                _assert_seg(h, rs, n_segs, "seg_gen_batch")
            seen += len(idx)
        finally:
            plan.close(); one.close()
    assert seen == len(ref)


# ---------------------------------------------------------------- the five plans ----------------------------------------------------------------
class Five:
    """RegPlan -> HitPlan.run_multi -> SegPlan -> HitPlan (pri_ratio 0) -> MapqPlan (do_join 0) for batches of up to n_frags fragments of n_segs segments"""

    def __init__(self, n_frags, n_segs, n_u_cap, n_b_cap):
        import mm2chain
        self.n_frags, self.n_segs, self.n_u_cap, self.n_b_cap = n_frags, n_segs, n_u_cap, n_b_cap
        self.reg = mm2chain.RegPlan(n_frags, n_u_cap, n_b_cap)
        self.hit = mm2chain.HitPlan(n_frags, n_u_cap)
        self.seg = mm2chain.SegPlan(n_frags, n_segs, n_u_cap, n_b_cap)
        self.hit2 = mm2chain.HitPlan(n_frags * n_segs, self.seg.n_su_cap)
        self.mapq = mm2chain.MapqPlan(n_frags * n_segs, self.seg.n_su_cap, n_b_cap, max_log_arg=1 << 14)

    def run(self, B, hit_opt, multi_opt, mapq_opt):
        """B: u_off, u, b_off, b, qlen_sum, hash, seg_len, gap_ref, rep_len on the host.  Everything is enqueued on the current stream; the first host
        synchronisation is the download of the results."""
        from mm2chain import params
        d = {k: t(v) for k, v in (("u_off", B["u_off"]), ("u", _padded(B["u"], self.n_u_cap)), ("b_off", B["b_off"]), ("b", _padded(B["b"], self.n_b_cap)),
                                  ("qlen_sum", B["qlen_sum"]), ("hash", B["hash"]), ("seg_len", B["seg_len"]), ("gap_ref", B["gap_ref"]), ("rep_len", B["rep_len"]))}
        regs = self.reg.run(d["u_off"], d["u"], d["b_off"], d["b"], d["qlen_sum"], d["hash"])
        regs1, n1 = self.hit.run_multi(hit_opt, multi_opt, d["u_off"], d["seg_len"], regs, d["gap_ref"])
        out = self.seg.run(d["u_off"], regs1, n1, d["b_off"], d["b"], d["seg_len"], d["hash"], d["rep_len"])
        opt0 = params.hit_opts(mask_level=hit_opt.mask_level, mask_len=hit_opt.mask_len, hard_mask_level=hit_opt.hard_mask_level, pri_ratio=0.0)
        regs2, n2 = self.hit2.run(opt0, out["su_off"], out["seg_regs"])
        regs3, n3, _, _ = self.mapq.run(mapq_opt, out["su_off"], regs2, n2, out["sb_off"], out["sb"], d["seg_len"], out["seg_rep_len"])
        h = {"su_off": out["su_off"].cpu().numpy(), "final": regs3.cpu().numpy(), "n_final": n3.cpu().numpy(), "sel": regs1.cpu().numpy(), "n_sel": n1.cpu().numpy()}
        self.reg.check(); self.hit.check(); self.seg.check(); self.hit2.check(); self.mapq.check()
        return h

    def close(self):
        for p in (self.reg, self.hit, self.seg, self.hit2, self.mapq):
            p.close()


def _assert_final(h, n_segs, names, sels, finals, u_off, what):
    for f, (name, sel, fin) in enumerate(zip(names, sels, finals)):
        assert h["n_sel"][f] == sel.size and h["sel"][u_off[f]:u_off[f] + sel.size].tobytes() == sel.tobytes(), f"{what}: {name}: the fragment's hits differ"
        for s, w in enumerate(fin):
            k = f * n_segs + s
            assert h["n_final"][k] == w.size == h["su_off"][k + 1] - h["su_off"][k], f"{what}: {name} segment {s}: {h['n_final'][k]} final regions, want {w.size}"
            g = h["final"][h["su_off"][k]:h["su_off"][k] + w.size].reshape(-1).view(REG)
            bad = [i for i in range(w.size) if g[i].tobytes() != w[i].tobytes()]
            assert not bad, f"{what}: {name} segment {s}: {len(bad)} of {w.size} final regions differ, first at {bad[0]}:\n got {g[bad[0]]}\nwant {w[bad[0]]}"


def test_five_plans_on_one_stream_equal_the_fixture(ref):
    from mm2chain import params
    groups = D.groups()
    seen = 0
    for n_segs in (2, 3):
        gs = [g for g in groups if ref[g[0]]["case"]["n_segs"] == n_segs]
        n_frags = max(len(g) for g in gs)
        five = Five(n_frags, n_segs, max(sum(ref[k]["case"]["u"].size for k in g) for g in gs), max(sum(ref[k]["case"]["a"].shape[0] for k in g) for g in gs))
        try:
            for g in gs:
                rs = [ref[k] for k in g]
                c = rs[0]["case"]
                B = _frag_batch(rs, n_frags, "regs0")
                h = five.run(B, _hit_opt(c), _multi_opt(c), params.mapq_opts(**c["mapq"]))
                _assert_final(h, n_segs, [R["name"] for R in rs], [R["sel"] for R in rs], [[S["final"] for S in R["segs"]] for R in rs], B["u_off"], "five plans")
                assert (h["n_final"][len(rs) * n_segs:n_frags * n_segs] == 0).all()
                seen += len(g)
        finally:
            five.close()
    assert seen == len(ref)


def test_pairs_of_mixed_lengths_from_reads_to_final_segment_regions():
    """the pairs of tests/golden/ref_frag_gaps.npz (2 x 150 and other lengths over the 150 kb test genome) through mm2c_frag_chain_batch_gaps, then the five plans with
    gap_ref = the first of each pair of task_dists; against the models on the reference's own chains"""
    import mm2chain
    from mm2chain import params
    z = np.load(os.path.join(GOLDEN, "ref_frag_gaps.npz"))
    fx = {k: z[k] for k in z.files}
    ids = np.nonzero(np.diff(fx["frag_off"]) == 2)[0]
    assert ids.size >= 30
    fo, so = fx["frag_off"], fx["seq_off"]
    frags = [[fx["seq"][so[s]:so[s + 1]].tobytes() for s in range(fo[g], fo[g + 1])] for g in ids]
    hp = [int(v) for v in fx["par"][ids[0]]]
    par = params.make_params(max_dist_x=1, max_dist_y=1, bw=hp[2], max_skip=hp[3], max_iter=hp[4], gap_scale=1.0, is_cdna=hp[7], n_segs=hp[8])
    idx = mm2chain.MinimizerIndex(int(fx["k"]), int(fx["w"]), False, fx["keys"], fx["cr_off"], fx["n"], pool=mm2chain.HitPool(fx["pool"]))
    try:
        with mm2chain.tuned(heap_sort=1):
            got = mm2chain.frag_chain_batch_gaps(par, hp[5], hp[6], frags, idx, int(fx["mid_occ"]), int(fx["max_occ"]),
                                                 mm2chain.frag_gaps(*(int(v) for v in fx["gaps"])))
    finally:
        idx.close()
    qlens = np.array([[len(s) for s in f] for f in frags], np.int32)
    gap_ref = got["task_dists"][:, 0].astype(np.int32)
    assert np.array_equal(gap_ref, fx["par"][ids, 0]) and len(set(gap_ref.tolist())) >= 5
    hashes = np.array([regs_model.read_hash(b"pair%d" % g, int(qlens[j].sum())) for j, g in enumerate(ids)], np.uint32)
    hit = dict(D.HIT_SR, min_diff=2 * int(fx["k"]))
    B = {"u_off": got["u_off"], "u": got["u"], "b_off": got["b_off"], "b": got["b"], "qlen_sum": qlens.sum(axis=1).astype(np.int32), "hash": hashes,
         "seg_len": qlens.reshape(-1), "gap_ref": gap_ref, "rep_len": got["rep_len"].astype(np.int32)}
    five = Five(ids.size, 2, int(got["u_off"][-1]), int(got["b_off"][-1]))
    try:
        h = five.run(B, params.hit_opts(**hit), params.hit_multi_opts(2, 777), params.mapq_opts(**D.MAPQ_SR))
    finally:
        five.close()
    sels, finals, n_seg_regs, n_dropped = [], [], 0, 0
    for j, g in enumerate(ids):
        u = fx["heap_u"][fx["heap_u_off"][g]:fx["heap_u_off"][g + 1]]; b = fx["heap_b"][fx["heap_b_off"][g]:fx["heap_b_off"][g + 1]]
        c = {"hash": int(hashes[j]), "n_segs": 2, "qlens": qlens[j], "u": u, "a": b, "hit": hit, "multi": D.MULTI, "gap_ref": int(gap_ref[j]), "mapq": D.MAPQ_SR,
             "rep_len": int(fx["heap_rep_len"][g])}
        sel = M.frag_hits(c)
        fin = [M.seg_final(c, r) for _, _, r in M.seg_gen(c["hash"], 2, qlens[j], sel, b)]
        sels.append(sel); finals.append(fin)
        n_seg_regs += sum(w.size for w in fin); n_dropped += u.size - sel.size
    assert n_seg_regs >= 60, "the pairs give segment regions to compare"
    _assert_final(h, 2, [f"pair {g}" for g in ids], sels, finals, got["u_off"], "reads in, segment regions out")


# ---------------------------------------------------------------- refusals, reuse ----------------------------------------------------------------
def _refusal_batch(ref):
    by = {R["name"]: R for R in ref}
    rs = [by["seg_which_segment"], by["seg_reverse_spans"], by["seg_empty_fragment"], by["seg_dropped_region"]]      # A, the victim, an empty one, B
    return rs, _frag_batch(rs, 4, "sel")


def test_every_kind_of_refusal_leaves_the_neighbours_exact(ref):
    import mm2chain
    rs, B0 = _refusal_batch(ref)
    n_u, n_b = int(B0["u_off"][-1]), int(B0["b_off"][-1])
    plan = mm2chain.SegPlan(4, 2, n_u, n_b)
    V = 1
    v0 = int(B0["u_off"][V])

    def reg_field(B, i, name, val):
        B["regs"][v0 + i:v0 + i + 1].reshape(-1).view(REG)[name] = val

    def sid(B, j, s):
        y = int(B["b"][int(B["b_off"][V]) + j, 1])
        B["b"][int(B["b_off"][V]) + j, 1] = np.uint64((y & ~(0xff << 48)) | (s << 48))

    sel = rs[V]["sel"]
    kinds = {                                                                   # name -> (what breaks, fragments refused, fragments that stay exact)
        "u_off end below start": (lambda B: B["u_off"].__setitem__(2, B["u_off"][1] - 1), 1, (0, 3)),
        "u_off negative": (lambda B: B["u_off"].__setitem__(2, -5), 2, (0, 3)),
        "u_off beyond the capacity": (lambda B: B["u_off"].__setitem__(2, n_u + 1), 2, (0, 3)),
        "n_in negative": (lambda B: B["n_in"].__setitem__(V, -1), 1, (0, 2, 3)),
        "n_in beyond its room": (lambda B: B["n_in"].__setitem__(V, int(B["u_off"][2] - B["u_off"][1]) + 1), 1, (0, 2, 3)),
        "b_off end below start": (lambda B: B["b_off"].__setitem__(2, B["b_off"][1] - 1), 1, (0, 3)),
        "b_off negative": (lambda B: B["b_off"].__setitem__(2, -1), 2, (0, 3)),
        "b_off beyond the capacity": (lambda B: B["b_off"].__setitem__(2, n_b + 1), 2, (0, 3)),
        "as negative": (lambda B: reg_field(B, 1, "as", -1), 1, (0, 2, 3)),
        "as + cnt beyond the anchors": (lambda B: reg_field(B, 0, "as", int(B["b_off"][2] - B["b_off"][1]) - int(sel["cnt"][0]) + 1), 1, (0, 2, 3)),
        "cnt negative": (lambda B: reg_field(B, 2, "cnt", -3), 1, (0, 2, 3)),
        "more anchors than the fragment has": (lambda B: [reg_field(B, i, "as", 0) or reg_field(B, i, "cnt", 9) for i in range(sel.size)], 1, (0, 2, 3)),
        "segment 2 of two": (lambda B: sid(B, int(sel["as"][sel.size - 1]) + 1, 2), 1, (0, 2, 3)),
        "segment 255": (lambda B: sid(B, int(sel["as"][0]), 255), 1, (0, 2, 3)),
    }
    assert sel.size >= 3 and 9 * sel.size > int(B0["b_off"][2] - B0["b_off"][1]) and int(sel["cnt"][sel.size - 1]) >= 2
    try:
        for name, (breaker, n_refused, exact) in kinds.items():
            B = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in B0.items()}
            breaker(B)
            h, (rc, got_refused, _, _) = _run_seg(plan, B)                      # (the guard rows in front of and behind every output are looked at in there)
            assert rc == -2 and got_refused == n_refused, f"{name}: rc {rc}, {got_refused} refused"
            with pytest.raises(mm2chain.Mm2cError):
                plan.check()
            _assert_seg(h, rs, 2, name, skip=[f for f in range(4) if f not in exact])
            for s in range(2):                                                  # the victim's segment reads are empty: the CSR stays sound
                assert h["su_off"][V * 2 + s + 1] == h["su_off"][V * 2 + s] and h["sb_off"][V * 2 + s + 1] == h["sb_off"][V * 2 + s], name
            assert (np.diff(h["su_off"][:9]) >= 0).all() and (np.diff(h["sb_off"][:9]) >= 0).all()
            assert (h["seg_hash"][2:4].view(np.int32) == -7).all() and (h["seg_rep_len"][2:4] == -7).all(), f"{name}: the refused fragment's hash or rep_len was written"
        h, (rc, got_refused, _, _) = _run_seg(plan, B0)                         # the plan is sound afterwards
        assert (rc, got_refused) == (0, 0)
        _assert_seg(h, rs, 2, "after the refusals")
    finally:
        plan.close()
    # the hit plan's second mode refuses as the first does
    hp = mm2chain.HitPlan(2, 8)
    try:
        R = {R["name"]: R for R in ref}["sel_nothing_dropped"]
        B = _frag_batch([R], 2, "regs0")
        B["u_off"][2] = 9
        whole_r, out = guarded(8, 80, torch.uint8, FILL)
        whole_n, n_out = guarded(2, 0, torch.int32, -9)
        hp.run_multi(_hit_opt(R["case"]), _multi_opt(R["case"]), t(B["u_off"]), t(B["seg_len"]), t(_padded(B["regs"], 8, FILL)), t(B["gap_ref"]), regs_out=out, n_out=n_out)
        with pytest.raises(mm2chain.Mm2cError):
            hp.check()
        assert guards_untouched(whole_r, FILL) and n_out.cpu().numpy().tolist() == [R["sel"].size, -9]
        assert out.cpu().numpy()[:R["sel"].size].tobytes() == R["sel"].tobytes()
    finally:
        hp.close()


def test_a_plan_run_again_on_other_data_of_another_size_and_order(ref):
    import mm2chain
    two = [R for R in ref if R["case"]["n_segs"] == 2]
    big = [R for R in two if R["name"].startswith("seg_")]
    small = [R for R in two if R["name"].startswith("sel_both")][::-1]
    n_frags = len(big)
    plan = mm2chain.SegPlan(n_frags, 2, sum(R["case"]["u"].size for R in big), sum(R["case"]["a"].shape[0] for R in big))
    try:
        for rs in (big, small, big[::-1], small[:3], big):
            h, (rc, n_refused, nu, na) = _run_seg(plan, _frag_batch(rs, n_frags, "sel"))
            assert (rc, n_refused) == (0, 0) and nu == sum(S["u"].size for R in rs for S in R["segs"])
            _assert_seg(h, rs, 2, "SegPlan.run again")
    finally:
        plan.close()
    hp = mm2chain.HitPlan(n_frags, sum(R["case"]["u"].size for R in big))
    try:
        default = [R for R in two if R["case"]["hit"] == D.HIT_SR and R["case"]["multi"] == D.MULTI]
        assert len(default) > n_frags
        for rs in (default[:n_frags], default[-5:], default[n_frags - 1::-1]):
            B = _frag_batch(rs, n_frags, "regs0")
            if int(B["u_off"][-1]) <= hp.n_u_cap:
                _assert_sel(_run_sel(hp, rs, B), B, rs, "HitPlan.run_multi again")
    finally:
        hp.close()
