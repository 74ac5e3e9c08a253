"""Objects that are kept and run again on OTHER data: one ChainPlan over the sets of tests/reuse_data.py (whose differences tests/test_cpu_plan_reuse_data.py asserts
from the oracle), with the knobs flipped between the runs of one plan, through the segmented prepass of a long task; one SeedPlan over hit pools with and without equal
x, the heap order and skip_seed; one mm2c_read_result_t for calls of several sizes.  include/mm2chain.h promises that a plan "can be run many times" with the anchors
an argument of the run: every run here equals the oracle and says what a plan made for that run alone says."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_binding as ob
import reuse_data as rd
from helpers import assert_same, oracle_batch

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sketch.npz")
N_LIVE = sum(n > 0 for n in rd.SIZES)      # the cut makes no piece of a task without anchors


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture
def knobs():
    from helpers import knob_setter
    with knob_setter() as tune:
        yield tune


_CHAINS = {}


def _chains_ref(name):
    if name not in _CHAINS:
        P = rd.scalars()
        _CHAINS[name] = [ob.mm_chain_dp(P, 3, 40, t) for t in rd.get(name)]
    return _CHAINS[name]


class Kept:
    """one plan with its own output arrays, kept over the runs of a test"""

    def __init__(self, P, off):
        import mm2chain
        self.P, self.off = P, np.asarray(off, np.int64)
        self.plan = mm2chain.ChainPlan(P, self.off)
        total = int(self.off[-1])
        self.d_f = torch.empty(total, dtype=torch.int32, device="cuda")
        self.d_p = torch.empty_like(self.d_f)

    def run(self, a, f_ref, p_ref, what, chains=None, route=True):
        """runs the kept plan on `a` and checks it against the oracle and against a plan made for this run alone; returns the variant text"""
        import mm2chain
        d_a = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 2)).cuda()
        self.d_f.fill_(-77); self.d_p.fill_(-77)
        self.plan.run(d_a, self.d_f, self.d_p)
        torch.cuda.synchronize()
        v = self.plan.last_variant()
        assert_same(self.d_f.cpu().numpy(), self.d_p.cpu().numpy(), f_ref, p_ref, self.off, f"{what}: {v}")
        fresh = mm2chain.ChainPlan(self.P, self.off)
        d_f2 = torch.full_like(self.d_f, -77); d_p2 = torch.full_like(self.d_p, -77)
        fresh.run(d_a, d_f2, d_p2)
        torch.cuda.synchronize()
        assert_same(d_f2.cpu().numpy(), d_p2.cpu().numpy(), f_ref, p_ref, self.off, f"{what}, a plan of its own: {fresh.last_variant()}")
        kept_cls, own_cls = np.frombuffer(self.plan.last_classes(), np.uint8), np.frombuffer(fresh.last_classes(), np.uint8)
        assert np.array_equal(kept_cls, own_cls), f"{what}: class bytes {kept_cls} of the kept plan, {own_cls} of a plan of its own"
        assert v == fresh.last_variant(), f"{what}: {v} vs {fresh.last_variant()}"
        if route:
            assert self.plan.last_route() == fresh.last_route(), f"{what}: route {self.plan.last_route()} vs {fresh.last_route()}"
        fresh.close()
        if chains is not None:
            u_off, u, b_off, b = self.plan.chains(d_a, self.d_f, self.d_p, 3, 40)
            torch.cuda.synchronize()
            uo, bo = u_off.cpu().numpy(), b_off.cpu().numpy()
            u_h, b_h = u.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64)
            for k, (u_ref, b_ref) in enumerate(chains):
                assert np.array_equal(u_h[uo[k]:uo[k + 1]], u_ref) and np.array_equal(b_h[bo[k]:bo[k + 1]], b_ref), f"{what}: chains of task {k} differ"
        return v, kept_cls

    def run_set(self, name, what):
        f_ref, p_ref = rd.reference(name)
        return self.run(rd.anchors(name), f_ref, p_ref, f"{what}, set {name}", chains=_chains_ref(name))

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("coop_plans", [0, 2])
def test_one_plan_over_many_data_sets(coop_plans, knobs):
    """run order A B C D A E F B C on one plan: the packed side array, st[], the class bytes and their counters, the cut arena (two pieces of task 0 in D, three in E,
    none elsewhere) and the epilogue scratch all carry the run before"""
    knobs("coop_plans", coop_plans)
    kept = Kept(rd.scalars(), rd.OFF)
    live = np.array(rd.SIZES) > 0
    for n_run, name in enumerate(rd.ORDER):
        v, cls = kept.run_set(name, f"run {n_run} of {rd.ORDER}, coop_plans={coop_plans}")
        want = rd.expected_class_bits(rd.get(name))
        assert np.array_equal((cls & 10)[live], want[live]), (name, cls, want)
        assert "packed_fp=1" in v and "cut=1" in v, v
        pieces = kept.plan.last_route()[0]
        assert pieces == N_LIVE + len(rd.JUMPS.get(name, {}).get(0, ())), (name, pieces)                 # only task 0 reaches plan_cut_min
    kept.close()


@pytest.mark.parametrize("case", ["packed_fp", "plan_cut", "compact_ring", "cut_sizes"])
def test_knobs_flipped_between_the_runs_of_one_plan(case, knobs):
    """packed_fp 0 1 0 1 on A B A B (the side array appears with the second run and stays while the flag is off); plan_cut 1 0 1 on D E D; compact_ring 1 0 1 on
    A B A; seg_min / plan_cut_min (256, 8192) (64, 300) (256, 8192) on D E D (the cut arena is made again for another number of pieces).  One wave per piece, so that
    the variant text names the forms."""
    knobs("coop_plans", 0)
    kept = Kept(rd.scalars(), rd.OFF)
    if case == "packed_fp":
        for n_run, (pk, name) in enumerate(zip((0, 1, 0, 1), "ABAB")):
            knobs("packed_fp", pk)
            v, cls = kept.run_set(name, f"packed_fp={pk}, run {n_run}")
            assert f"packed_fp={pk}" in v and "compact=1" in v, v
            assert bool((cls & 8).any()) == bool(pk), cls
    elif case == "plan_cut":
        for n_run, (cut, name) in enumerate(zip((1, 0, 1), "DED")):
            knobs("plan_cut", cut)
            v, _ = kept.run_set(name, f"plan_cut={cut}, run {n_run}")
            assert f"cut={cut}" in v, v
            assert kept.plan.last_route()[0] == (N_LIVE + len(rd.JUMPS[name][0]) if cut else len(rd.SIZES))      # (a run that does not cut counts its tasks)
    elif case == "compact_ring":
        for n_run, (c, name) in enumerate(zip((1, 0, 1), "ABA")):
            knobs("compact_ring", c)
            v, cls = kept.run_set(name, f"compact_ring={c}, run {n_run}")
            assert f"compact={c}" in v and f"packed_fp={c}" in v, v
    else:
        for n_run, ((seg_min, cut_min), name) in enumerate(zip(((256, 8192), (64, 300), (256, 8192)), "DED")):
            knobs("seg_min", seg_min); knobs("plan_cut_min", cut_min)
            v, _ = kept.run_set(name, f"seg_min={seg_min}, plan_cut_min={cut_min}, run {n_run}")
            assert "cut=1" in v, v
            jumps = rd.JUMPS[name]
            n_cut = sum(len(j) for k, j in jumps.items() if rd.SIZES[k] >= cut_min)
            assert kept.plan.last_route()[0] == N_LIVE + n_cut, (kept.plan.last_route(), n_cut)
    kept.close()


_LONG = {}


def _long_sets():
    """[70000, 700, 3000]: n_tasks <= 512 and the longest task at least two prepass segments of 32768 anchors.  Set 1: compact q (the long task's q values span
    53 000), span 15; set 2: the mixed profile with span 23 (q over several 100 000: the 32-bit ring)"""
    if not _LONG:
        from mm2chain import params, synth
        P = params.map_ont()
        rng = np.random.default_rng(70)
        sizes = (70000, 700, 3000)
        one = [rd.chain_with_noise(rng, n, every, step=70 if n > 8192 else 450) for n, every in zip(sizes, (100, 40, 64))]
        two = [synth.make_stream("mixed", 1, n, seed=71 + k, q_span=23)[1].numpy().view(np.uint64) for k, n in enumerate(sizes)]
        for key, tasks in ((1, one), (2, two)):
            a, off = rd.batch(tasks)
            _LONG[key] = (a, off) + oracle_batch(P, off, a)
        bits = [rd.expected_class_bits(t, packed=False) for t in (one, two)]
        assert not (bits[0] & 2).any() and (bits[1][0] & 2), bits
        _LONG["P"] = P
    return _LONG


@pytest.mark.parametrize("coop_plans", [0, 2])
def test_a_long_task_through_the_segmented_prepass_again(coop_plans, knobs):
    """chain_window_start_t<true>: the segments of the long task add up its span sum, far tiles and q extremes in words that only the last segment of a run puts back
    to zero.  Sets 1, 2, 1 with seg_prepass 1, 0, 1: avg (through f / p) and the class bytes must be those of the run's own data"""
    L = _long_sets()
    knobs("coop_plans", coop_plans)
    kept = Kept(L["P"], L[1][1])
    cls = []
    for n_run, (key, seg) in enumerate(zip((1, 2, 1), (1, 0, 1))):
        knobs("seg_prepass", seg)
        a, off, f_ref, p_ref = L[key]
        cls.append(kept.run(a, f_ref, p_ref, f"long task, set {key}, seg_prepass={seg}, run {n_run}, coop_plans={coop_plans}")[1])
    assert np.array_equal(cls[0], cls[2]) and not np.array_equal(cls[0] & 2, cls[1] & 2), cls
    kept.close()


def _seed_pools():
    """13 reads over fixed match_off / anchor_off -- 12 of 200 to 6000 anchors and one of about 14 000 (the multi-wave replay class) -- and three hit pools with the same
    counts: every read full of equal x (positions out of 40), none at all (positions distinct within a read), and the reads alternating"""
    from test_gpu_seed_hits import _batch, _random_read
    rng = np.random.default_rng(1312)
    reads = []
    for n_matches in (80, 120, 250, 400, 500, 700, 900, 1100, 1300, 1500, 1700, 1900, 4400):
        qlen, m, h = _random_read(rng, n_matches, 6, 4, 1 << 24, qlen=60000)
        reads.append((qlen, m, h))
    sizes = [int(m["n"].sum()) for _, m, _ in reads]
    assert 150 < min(sizes) and max(sizes[:12]) <= 6144 and 12288 < sizes[12] <= 16384, sizes

    def redraw(m, kind):
        n = int(m["n"].sum())
        if kind == "ties":
            pos = rng.integers(0, 40, n).astype(np.uint64); rid = np.zeros(n, np.uint64); strand = np.zeros(n, np.uint64)
        else:
            pos = (rng.permutation(1 << 16)[:n].astype(np.uint64) << np.uint64(7)) | rng.integers(0, 128, n).astype(np.uint64)
            rid = rng.integers(0, 4, n).astype(np.uint64); strand = rng.integers(0, 2, n).astype(np.uint64)
        h = (rid << np.uint64(32)) | (pos << np.uint64(1)) | strand
        for c, k in zip(m["cr_off"], m["n"]):                        # ascending lists, as mm_idx_get hands them out
            h[int(c):int(c) + int(k)].sort()
        return h
    pools = {"ties": [(q, m, redraw(m, "ties")) for q, m, _ in reads], "none": [(q, m, redraw(m, "none")) for q, m, _ in reads]}
    pools["mixed"] = [pools["ties" if r % 2 else "none"][r] for r in range(len(reads))]
    return {k: (v, _batch(v)) for k, v in pools.items()}, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_a_seed_plan_run_again_on_other_hits():
    """status, has_ties, the replay stack, tie ids, the heap flag and the skip arguments of a seed plan are set "for the run it starts": ties, none, mixed, ties; the
    heap order on mixed and back on ties; skip_seed (NO_DIAG | NO_DUAL) and then a plain run, which keeps every anchor.  check() counts the reads with equal x of the
    run's own data"""
    import mm2chain
    pools, ao = _seed_pools()
    mo = pools["ties"][1][0]
    sp = mm2chain.SeedPlan(mo, ao)
    dev = {}
    for k, (reads, (mo_k, m, h, ql)) in pools.items():
        assert np.array_equal(mo_k, mo)
        dev[k] = (torch.from_numpy(m.view(np.uint8).copy()).cuda(), torch.from_numpy(h.view(np.int64)).cuda(), torch.from_numpy(ql).cuda())
    d_anchors = torch.empty((int(ao[-1]), 2), dtype=torch.int64, device="cuda")
    refs = {}

    def oracle(kind, heap):
        if (kind, heap) not in refs:
            refs[(kind, heap)] = [ob.collect_seed_hits(m, h, q, heap=heap) for q, m, h in pools[kind][0]]
        return refs[(kind, heap)]

    def plain(kind, heap, what):
        d_anchors.fill_(-77)
        sp.run(*dev[kind], anchors=d_anchors)
        n_tie_reads = sp.check()
        got = d_anchors.cpu().numpy().view(np.uint64)
        want_ties = 0
        for r, ref in enumerate(oracle(kind, heap)):
            assert ref.shape[0] == ao[r + 1] - ao[r], f"{what}: the plain run keeps every anchor"
            bad = np.nonzero((got[ao[r]:ao[r + 1]] != ref).any(axis=1))[0]
            assert bad.size == 0, f"{what}: read {r}: {bad.size} of {ref.shape[0]} anchors differ, first at {bad[0]}"
            want_ties += int((ref[1:, 0] == ref[:-1, 0]).any())
        assert n_tie_reads == want_ties, f"{what}: check() says {n_tie_reads} reads with equal x, the data has {want_ties}"
        return want_ties

    n_reads = len(ao) - 1
    seen = [plain(kind, False, f"run {k}, {kind}") for k, kind in enumerate(("ties", "none", "mixed", "ties"))]
    assert seen == [n_reads, 0, n_reads // 2, n_reads], seen
    sp.set_heap_sort(1)
    plain("mixed", True, "heap order, mixed")
    sp.set_heap_sort(0)
    plain("ties", False, "heap order off again, ties")
    # skip_seed: names as ranks; reads drop the hits on references that sort before them (NO_DUAL) and on their own diagonal (NO_DIAG)
    rank = np.array([2, 0, 3, 1], np.int32); ref_len = np.full(4, 60000, np.int32)
    q_lo = (np.arange(n_reads) % 5).astype(np.int32); q_eq = (np.arange(n_reads) % 2).astype(np.int32)
    flag = ob.F_NO_DIAG | ob.F_NO_DUAL
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()
    d_anchors.fill_(-77)
    _, d_off = sp.run_skip(*dev["mixed"], flag, i32(rank), i32(ref_len), i32(q_lo), i32(q_eq), anchors=d_anchors)
    sp.check()
    off = d_off.cpu().numpy(); got = d_anchors.cpu().numpy().view(np.uint64)
    kept = 0
    for r, (q, m, h) in enumerate(pools["mixed"][0]):
        ref = ob.collect_seed_hits(m, h, q, flag, rank, ref_len, int(q_lo[r]), int(q_eq[r]))
        assert off[r + 1] - off[r] == ref.shape[0] and np.array_equal(got[off[r]:off[r + 1]], ref), f"skip_seed: read {r} differs"
        kept += ref.shape[0]
    assert 0 < kept < ao[-1]                                         # some reads lost hits: the plain run below has more to keep than this run left
    plain("none", False, "plain run after skip_seed, none")
    plain("mixed", False, "plain run after skip_seed, mixed")
    sp.close()


def test_one_read_result_for_several_calls():
    """one mm2c_read_result_t serves mm2c_sketch_match_batch and then mm2c_read_chain_batch on 40 reads, 3 reads, a batch without minimizers and the 40 again: every
    field equals what a call with a result of its own returns, the counts follow the call, and what mm2c_read_chain_batch does not fill has count 0"""
    import mm2chain
    from mm2chain import params
    from mm2chain.batch import _arr, _reads_args
    z = np.load(FIX)
    so, seq = z["seq_off"], z["seq"]
    reads = [seq[so[r]:so[r + 1]].tobytes() for r in range(so.size - 1)]
    forty = reads + reads[1:11]
    assert len(forty) == 40
    k, w, hpc = (int(v) for v in z["map_ont_kwh"])
    pool = mm2chain.HitPool(z["map_ont_pool"])
    idx = mm2chain.MinimizerIndex(k, w, hpc, z["map_ont_keys"], z["map_ont_cr_off"], z["map_ont_n"], pool=pool)
    mid_occ = int(z["map_ont_mid_occ"][0])
    P = params.map_ont()
    lib = mm2chain.load()
    res = lib.mm2c_read_result_create()
    off40, seq40 = _reads_args(forty)
    assert lib.mm2c_sketch_match_batch(idx.handle, mid_occ, 40, off40.ctypes.data, seq40.ctypes.data, res) == 0
    assert res.contents.n_matches > 0 and res.contents.n_reads == 40
    batches = [forty, reads[1:4], [b"", b"ACG", b"N" * 60, b"ACGTACGTACGTAC"], forty]
    sizes = []
    for n_call, batch in enumerate(batches):
        own = mm2chain.read_chain_batch(P, 3, 40, batch, idx, mid_occ)
        off, sq = _reads_args(batch)
        nr = len(batch)
        assert lib.mm2c_read_chain_batch(C.byref(P), 3, 40, idx.handle, mid_occ, nr, off.ctypes.data, sq.ctypes.data, None, res) == 0, lib.mm2c_last_error()
        r = res.contents
        assert r.n_reads == nr and r.n_sketch == 0 and r.n_matches == 0 and r.n_rechained == 0, (n_call, r.n_reads, r.n_sketch, r.n_matches, r.n_rechained)
        got = {"anchor_off": _arr(r.anchor_off, nr + 1, np.int64), "u_off": _arr(r.u_off, nr + 1, np.int64), "u": _arr(r.u, r.n_u, np.uint64),
               "b_off": _arr(r.b_off, nr + 1, np.int64), "b": _arr(r.b, 2 * r.n_b, np.uint64).reshape(-1, 2), "rep_len": _arr(r.rep_len, nr, np.int32),
               "mini_off": _arr(r.mini_off, nr + 1, np.int64), "mini_pos": _arr(r.mini_pos, r.n_mini_pos, np.uint64)}
        for key, val in got.items():
            assert np.array_equal(val, own[key]), f"call {n_call}: {key} differs from a call with a result of its own"
        assert r.n_anchors == own["anchor_off"][-1] and r.n_u == own["u_off"][-1] and r.n_b == own["b_off"][-1] and r.n_mini_pos == own["mini_off"][-1]
        sizes.append((int(r.n_anchors), int(r.n_u), int(r.n_b), int(r.n_mini_pos)))
    assert sizes[2] == (0, 0, 0, 0) and sizes[0] == sizes[3] and all(a >= b for a, b in zip(sizes[0], sizes[1])) and sizes[0][3] > sizes[1][3] > 0 and sizes[0][1] > 0, sizes
    lib.mm2c_read_result_free(res)
    idx.close(); pool.close()
