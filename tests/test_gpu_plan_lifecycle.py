"""The lifecycle the eight stand-alone device plans share (RegPlan, HitPlan, MapqPlan, EstErrPlan, SegPlan, KswPlan, ExtraPlan, AlnPlan), on the smallest valid input of
each: the first two or three reads, regions or tasks of the plan's own fixture, packed and judged by the helpers of the plan's own test module.  Per plan: the check
accessors answer zeros before any run; the timing accessors refuse with "has not been run"; a plan that never ran closes, closes again and dies; two runs on one plan
give the same bytes, which are the fixture's; the host entry gives those bytes too and takes an empty batch; and a run adds to mm2c_get_stats().launches exactly
the literal recorded here."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def _launches():
    import ctypes as C
    from mm2chain import _native as N
    st = N.Stats()
    N.load().mm2c_get_stats(C.byref(st))
    return int(st.launches)


def _b(*arrays):
    """the bytes of what a run or a host entry made"""
    return b"|".join(np.ascontiguousarray(a).tobytes() for a in arrays)


class Regs:
    launches = 3                                                               # regs_sort, regs_fill, regs_fill_reads

    def __init__(self):
        import regs_data
        import test_gpu_regs as T
        self.T, self.cs = T, regs_data.cases()[:3]
        Z = np.load(os.path.join(GOLDEN, "ref_regs.npz"))
        self.want = Z["regs"][:Z["reg_off"][3]]
        self.B = regs_data.batch(self.cs)

    def make(self):
        import mm2chain
        return mm2chain.RegPlan(len(self.cs), sum(c["u"].size for c in self.cs), sum(c["a"].shape[0] for c in self.cs))

    def zeros(self, plan):
        return [(plan.check(), 0)]

    def run(self, plan):
        got, self.checked = self.T._run_plan(plan, self.cs)
        self.T._assert_equal(got, self.want, self.cs, "RegPlan.run")
        return _b(got)

    def host(self):
        import mm2chain
        return _b(mm2chain.gen_regs_batch(*self.B))

    def host_empty(self):
        import mm2chain
        z = np.zeros(1, np.int64)
        assert mm2chain.gen_regs_batch(z, np.zeros(0, np.uint64), z, np.zeros((0, 2), np.uint64), np.zeros(0, np.int32), np.zeros(0, np.uint32)).size == 0


class Hits:
    launches = 1

    def __init__(self):
        import hits_data
        import hits_model
        import test_gpu_hits as T
        self.T, self.D, self.cs = T, hits_data, hits_data.cases()[:3]
        assert all(c["opt"] == hits_data.DEFAULT for c in self.cs)
        Z = np.load(os.path.join(GOLDEN, "ref_hits.npz"))
        self.want = [Z["hits"][Z["hit_off"][k]:Z["hit_off"][k + 1]].reshape(-1).view(hits_model.REG) for k in range(3)]

    def make(self):
        import mm2chain
        return mm2chain.HitPlan(len(self.cs), sum(c["regs"].size for c in self.cs))

    def zeros(self, plan):
        return [(plan.check(), 0)]

    def run(self, plan):
        got = self.T._run_plan(plan, self.D.DEFAULT, self.cs)                 # (checks inside that check()'s total is the sum of n_out)
        self.T._assert_equal(got, self.want, self.cs, "HitPlan.run")
        self.checked = sum(g.size for g in got)
        return _b(*got)

    def host(self):
        import mm2chain
        u_off, regs = self.D.batch(self.cs)
        out, n_out = mm2chain.select_hits_batch(self.T._opt(self.D.DEFAULT), u_off, regs)
        return _b(*[out[u_off[r]:u_off[r] + n_out[r]] for r in range(len(self.cs))])

    def host_empty(self):
        import mm2chain
        out, n_out = mm2chain.select_hits_batch(self.T._opt(self.D.DEFAULT), np.zeros(1, np.int64), np.zeros(0, mm2chain.REG_DTYPE))
        assert out.size == 0 and n_out.size == 0


class Mapq:
    launches = 2                                                               # mapq_join and, with anchors, mapq_gather

    def __init__(self):
        import mapq_data as D
        import mapq_model as M
        import test_gpu_mapq as T
        self.T = T
        self.o, idx = D.groups()[0]
        Z = np.load(os.path.join(GOLDEN, "ref_mapq.npz"))
        cs = D.cases()
        cut = lambda key, off, k: Z[key][Z[off][k]:Z[off][k + 1]]
        self.rs = [{"in": cut("hits_in", "in_off", k).reshape(-1).view(M.REG), "out": cut("hits_out", "out_off", k).reshape(-1).view(M.REG), "a": cut("a_out", "a_off", k),
                    "case": cs[k], "name": cs[k]["name"]} for k in idx[:3]]
        self.B = T._batch(self.rs)

    def make(self):
        import mm2chain
        return mm2chain.MapqPlan(len(self.rs), int(self.B["u_off"][-1]), int(self.B["b_off"][-1]))

    def zeros(self, plan):
        return [(plan.counts(), (0, 0, 0)), (plan.check(), 0)]

    def _defined(self, got, B):
        out, n_out, b_out, n_b_out = got
        k = range(len(self.rs))
        return _b(*[out[B["u_off"][r]:B["u_off"][r] + n_out[r]] for r in k], n_out[:len(self.rs)], *[b_out[B["b_off"][r]:B["b_off"][r] + n_b_out[r]] for r in k], n_b_out[:len(self.rs)])

    def run(self, plan):
        got = self.T._run(plan, self.o, self.B, True)
        self.checked = plan.check()
        for k, R in enumerate(self.rs):
            self.T._assert_read(got, self.B, k, R, "MapqPlan.run")
        return self._defined(got, self.B)

    def host(self):
        import mm2chain
        B = self.B
        h = mm2chain.join_mapq_batch(self.T._opt(self.o), B["u_off"], B["regs"], B["n_in"], B["b_off"], B["b"], B["qlen"], B["rep_len"], anchors=True)
        return self._defined((h[0].view(np.uint8).reshape(-1, 80), h[1], h[2], h[3]), B)

    def host_empty(self):
        import mm2chain
        z, i = np.zeros(1, np.int64), np.zeros(0, np.int32)
        h = mm2chain.join_mapq_batch(self.T._opt(self.o), z, np.zeros(0, mm2chain.REG_DTYPE), i, z, np.zeros((0, 2), np.uint64), i, i)
        assert h[0].size == 0 and h[1].size == 0 and h[2].size == 0 and h[3].size == 0


class EstErr:
    launches = 3                                                               # err_reads, err_walk, err_finish

    def __init__(self):
        import esterr_data as D
        import esterr_model as M
        import test_gpu_esterr as T
        self.T, self.rs = T, D.reference()[:3]
        for R in self.rs:
            c = R["case"]
            R["cnts"], R["avg_k"] = M.counts(R["in"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"])
        self.B = T._batch(self.rs, room=0)

    def make(self):
        import mm2chain
        B = self.B
        return mm2chain.EstErrPlan(len(self.rs), int(B["u_off"][-1]), int(B["b_off"][-1]), int(B["mini_off"][-1]))

    def zeros(self, plan):
        return [(plan.refused(), (0, 0)), (plan.check(), None)]

    def run(self, plan):
        err, avg = self.T._run(plan, self.B)
        self.checked = plan.refused()
        for k, R in enumerate(self.rs):
            self.T._assert_read((err, avg), self.B, k, R, "EstErrPlan.run")
        return _b(err[:int(self.B["u_off"][-1])], avg[:len(self.rs)])

    def host(self):
        import mm2chain
        B = self.B
        _, err, avg = mm2chain.est_err_batch(B["u_off"], B["regs"], B["n_in"], B["b_off"], B["b"], B["mini_off"], B["mini_pos"], B["qlen"], B["ref_len"])
        return _b(err, avg)

    def host_empty(self):
        import mm2chain
        z, i = np.zeros(1, np.int64), np.zeros(0, np.int32)
        regs, err, avg = mm2chain.est_err_batch(z, np.zeros(0, mm2chain.REG_DTYPE), i, z, np.zeros((0, 2), np.uint64), z, np.zeros(0, np.uint64), i, np.zeros(0, np.uint32))
        assert regs.size == 0 and err.size == 0 and avg.size == 0


class Segs:
    launches = 8                                                               # seg_count, two scans, seg_scatter, the three region kernels, seg_mark

    def __init__(self):
        import seg_data as D
        import test_gpu_seg as T
        ref = D.reference()
        assert ref is not None, "tests/golden/ref_seg.npz is absent"
        self.T, self.rs = T, [ref[k] for k in D.groups()[0][:3]]
        self.n_segs = self.rs[0]["case"]["n_segs"]
        assert all(R["case"]["n_segs"] == self.n_segs for R in self.rs)
        self.B = T._frag_batch(self.rs, len(self.rs), "sel")

    def make(self):
        import mm2chain
        return mm2chain.SegPlan(len(self.rs), self.n_segs, int(self.B["u_off"][-1]), int(self.B["b_off"][-1]))

    def zeros(self, plan):
        return [(plan.counts(), (0, 0, 0, 0)), (plan.check(), (0, 0))]

    def _defined(self, h):
        tu, ta = int(h["su_off"][-1]), int(h["sb_off"][-1])
        return _b(h["su_off"], h["sb_off"], h["su"][:tu], h["sb"][:ta], h["seg_regs"][:tu], h["seg_hash"], h["seg_rep_len"])

    def run(self, plan):
        h, self.checked = self.T._run_seg(plan, self.B)
        assert self.checked[:2] == (0, 0)
        self.T._assert_seg(h, self.rs, self.n_segs, "SegPlan.run")
        return self._defined(h)

    def host(self):
        import mm2chain
        B = self.B
        return self._defined(mm2chain.seg_gen_batch(self.n_segs, B["u_off"], B["regs"], B["n_in"], B["b_off"], B["b"], B["seg_len"], B["hash"], B["rep_len"]))

    def host_empty(self):
        import mm2chain
        z, i = np.zeros(1, np.int64), np.zeros(0, np.int32)
        h = mm2chain.seg_gen_batch(self.n_segs, z, np.zeros(0, mm2chain.REG_DTYPE), i, z, np.zeros((0, 2), np.uint64), i, np.zeros(0, np.uint32))
        assert h["su"].size == 0 and h["sb"].size == 0 and h["seg_regs"].size == 0 and h["su_off"].tolist() == [0]


class Ksw:
    launches = 1

    def __init__(self):
        import ksw_data as D
        import test_gpu_ksw as T
        fx = np.load(os.path.join(GOLDEN, "ref_ksw.npz"))
        cs = D.cases()
        ks = [k for k, c in enumerate(cs) if c["sc"] == "ont"][:3]
        assert [cs[k]["name"] for k in ks] == [fx["names"][k] for k in ks]
        self.T, self.D = T, D
        self.rs = [dict(case=cs[k], ez=fx["ez"][k], cigar=fx["cigar"][fx["cig_off"][k]:fx["cig_off"][k + 1]]) for k in ks]
        self.tk, self.seq, self.co = T.pack(self.rs)

    def make(self):
        import mm2chain
        return mm2chain.KswPlan(len(self.rs), self.seq.size, int(self.co[-1]), n_slots=2, slot_bytes=self.T.need_of(self.rs))

    def zeros(self, plan):
        return [(plan.counts(), (0, 0, 0)), (plan.check(), None)]

    def run(self, plan):
        _, rw, rv, cw, cv = self.T.run_plan(plan, "ont", self.rs, self.tk, self.seq, self.co)
        self.checked = plan.counts()
        res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
        self.T.check_out(self.rs, res, cig, self.co)
        assert self.T.guards_ok(rw, cw)
        return _b(res, cig)

    def host(self):
        import mm2chain
        res = np.full(len(self.rs) * 48, 0xee, np.uint8).view(mm2chain.KSW_RES_DTYPE); cigar = np.full(int(self.co[-1]), self.T.FILL, np.uint32)
        mm2chain.ksw_extd2_batch(self.D.score_set("ont"), self.tk, self.seq, self.co, res=res, cigar=cigar)
        return _b(res, cigar)

    def host_empty(self):
        import mm2chain
        res, cigar = mm2chain.ksw_extd2_batch(self.D.score_set("ont"), np.zeros(0, mm2chain.KSW_TASK_DTYPE), np.zeros(0, np.uint8), np.zeros(1, np.int64))
        assert res.size == 0 and cigar.size == 0


class Extra:
    launches = 1

    def __init__(self):
        import extra_data as D
        import test_gpu_extra as T
        f = np.load(os.path.join(GOLDEN, "ref_extra.npz"))
        us = D.update_cases()
        ks = [k for k, c in enumerate(us) if c["sc"] == "ont"][:3]
        assert [us[k]["name"] for k in ks] == [f["u_names"][k] for k in ks]
        off, cig = f["u_cig_off"], f["u_cigar"]
        self.T, self.D = T, D
        self.rs = [dict(case=us[k], res=f["u_res"][k], cigar=(cig[off[2 * k]:off[2 * k + 1]], cig[off[2 * k + 1]:off[2 * k + 2]])) for k in ks]
        self.p = T.pack(self.rs, 0)

    def make(self):
        import mm2chain
        return mm2chain.ExtraPlan(len(self.rs), self.p[1].size, self.p[3].size, int(self.p[4][-1]))

    def zeros(self, plan):
        return [(plan.counts(), (0, 0, 0)), (plan.check(), None)]

    def run(self, plan):
        rw, rv, cw, cv = self.T.run_update(plan, "ont", 0, self.rs, self.p)
        self.checked = plan.counts()
        res, cig = rv.cpu().numpy(), cv.cpu().numpy().view(np.uint32)
        self.T.check_out(self.rs, 0, res, cig, self.p[4])
        assert self.T.guards_ok(rw, cw)
        ms = plan.last_kernel_ms()
        assert ms[0] > 0 and ms[1] == 0.0, f"after update only: last_kernel_ms() = {ms}"
        return _b(res, cig)

    def host(self):
        import mm2chain
        tk, seq, io, ci, oo = self.p
        res = np.full(len(self.rs) * 32, 0xee, np.uint8).view(mm2chain.EXTRA_RES_DTYPE); out = np.full(int(oo[-1]), self.T.FILL, np.uint32)
        mm2chain.update_extra_batch(self.D.score_set("ont"), 0, tk, seq, io, ci, oo, res=res, cig_out=out)
        return _b(res, out)

    def host_empty(self):
        import mm2chain
        res, out = mm2chain.update_extra_batch(self.D.score_set("ont"), 0, np.zeros(0, mm2chain.EXTRA_TASK_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.int64),
                                               np.zeros(0, np.uint32), np.zeros(1, np.int64))
        assert res.size == 0 and out.size == 0


class Aln:
    launches = 4                                                               # aln_plan, aln_scan, aln_emit, aln_gather

    def __init__(self):
        import aln_data as D
        import aln_model as M
        import test_gpu_aln as T
        self.T, self.D = T, D
        self.o, reads = D.cached_batches()["ont"]
        self.c = D.csr(reads[:2])
        self.want = M.run(self.o, D.reference(), *self.c[:6], slot_words=T.SLOT_WORDS)
        self.ref = None

    def make(self):
        import mm2chain
        if self.ref is None:
            self.ref = mm2chain.RefSeq(*self.D.reference())
        return self.T.plan_for(self.c, self.want, slack=0)

    def zeros(self, plan):
        return [(plan.counts(), (0, 0, 0, (0, 0, 0, 0))), (plan.check(), (0, 0, 0, 0))]

    def _defined(self, got):
        return _b(*[got[k] for k in ("aln_regs", "items", "tasks", "cig_off", "pool", "b")], np.array(got["totals"], np.int64))

    def run(self, plan):
        got, guards = self.T.run_plan(plan, self.ref, self.T.opt_of(self.o), self.c)
        assert got["rc"] == 0 and guards
        self.T.same(got, self.want, "AlnPlan.run")
        self.checked = (got["rc"], got["n_refused"], got["n_too_big"], tuple(got["totals"]))
        return self._defined(got)

    def host(self):
        import mm2chain
        tot = self.want["totals"]
        got = mm2chain.align_tasks_batch(self.T.opt_of(self.o), *self.D.reference(), *self.c[:6], tot[0], tot[1], tot[3], fill=0xff)
        assert got["rc"] == 0
        return self._defined(got)

    def host_empty(self):
        import mm2chain
        z = np.zeros(1, np.int64)
        got = mm2chain.align_tasks_batch(self.T.opt_of(self.o), *self.D.reference(), z, np.zeros(0, mm2chain.REG_DTYPE), z, np.zeros((0, 2), np.uint64), z, np.zeros(0, np.uint8), 0, 0, 0)
        assert got["rc"] == 0 and got["aln_regs"].size == 0 and got["items"].size == 0 and got["tasks"].size == 0 and got["totals"] == (0, 0, 0, 0)

    def done(self):
        if self.ref is not None:
            self.ref.close()
            self.ref.close()                                                    # a RefSeq closes twice as well


PLANS = {"regs": Regs, "hits": Hits, "mapq": Mapq, "esterr": EstErr, "segs": Segs, "ksw": Ksw, "extra": Extra, "aln": Aln}


@pytest.mark.parametrize("name", list(PLANS))
def test_lifecycle(name):
    import mm2chain
    P = PLANS[name]()
    try:
        # a plan that never ran: zeros from the check accessors, refusals from the timing accessors, and it closes, closes again and dies
        plan = P.make()
        for got, want in P.zeros(plan):
            assert got == want, f"before any run: {got}, expected {want}"
        for timing in [getattr(plan, f) for f in ("last_ms", "last_kernel_ms") if hasattr(plan, f)]:      # (HitPlan has no last_kernel_ms)
            with pytest.raises(mm2chain.Mm2cError, match=r"code -2\).*has not been run"):
                timing()
        plan.close()
        assert plan.handle is None
        plan.close()
        del plan
        # two runs on one plan, then the host entry
        plan = P.make()
        at = _launches()
        first = P.run(plan)
        grown = _launches() - at
        print(f"{name}: launches per run {grown}")
        assert grown == P.launches, f"a run added {grown} to mm2c_get_stats().launches, the literal is {P.launches}"
        checked = P.checked
        assert plan.last_ms() > 0
        at = _launches()
        second = P.run(plan)
        assert _launches() - at == P.launches
        assert second == first, "the second run of the plan differs from the first"
        assert P.checked == checked, f"check() after the second run: {P.checked}, after the first {checked}"
        assert plan.last_ms() > 0
        plan.close()
        plan.close()
        del plan
        assert P.host() == first, "the host entry differs from the plan run"
        P.host_empty()
    finally:
        if hasattr(P, "done"):
            P.done()
