"""The alignment-task plan on the device (csrc/align_tasks.hip: mm_align1, align.c:565-771, up to its ksw calls): every region of tests/aln_data.py through AlnPlan and
the host entry, equal in every byte -- region records, items, ksw tasks, cig_off, the sequence pool, the anchors' flag words -- to the model (tests/aln_model.py), and
through the model's reading of the record equal to what the reference's own mm_align1 called (tests/golden/ref_aln.npz): one batch per option set, the same in reverse
order through the same plan, the planted regions one per call, guard rows around every output array and fill behind the pool and the task list, each kind of refusal
with exact neighbours and untouched anchors, each capacity exceeded by one, a plan run again behind another kernel on the caller's stream, and the plan's device
outputs straight into a KswPlan.  Size classes: regions of 63 / 64 / 65 / 128 / 129 anchors around the wave steps; 2 048 long gaps in LDS and 2 049 in a scratch slot.
Everything is integer and compared with ==."""
import os

import numpy as np
import pytest
import torch

import aln_data as D
import aln_model as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD, SLACK = 3, 5
SLOT_WORDS = 2304


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "ref_aln.npz"))


@pytest.fixture(scope="module")
def ref():
    from mm2chain import RefSeq
    r = RefSeq(*D.reference())
    yield r
    r.close()


@pytest.fixture(scope="module")
def model():
    """the model's outputs of every option set, computed once"""
    out = {}
    for name, (o, reads) in D.cached_batches().items():
        c = D.csr(reads)
        out[name] = (o, c, M.run(o, D.reference(), *c[:6], slot_words=SLOT_WORDS))
    return out


def t(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    if a.dtype in (np.uint32, np.uint64):
        a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
    return torch.from_numpy(a).cuda()


def opt_of(o, **kw):
    from mm2chain import params
    v = params.aln_opts(**{k: o[k] for k in o if k not in ("q2", "sc_ambi")})
    v.update(kw)
    return v


def run_plan(plan, ref, o, c, stream=None, n_b=None):
    """one batch through the plan with guard rows around every output -> (dict in the model's layout, totals, return code, the guard verdict)"""
    from mm2chain import ALN_REG_DTYPE, ALN_ITEM_DTYPE, KSW_TASK_DTYPE
    u_off, regs, b_off, b, read_off, fwd = c[:6]
    n_reads, n_regs = len(u_off) - 1, int(u_off[-1])
    mk = lambda n, w, fill: torch.full((n + 2 * GUARD, w) if w else (n + 2 * GUARD,), fill, dtype=torch.uint8 if w else torch.int64, device="cuda")
    arw, itw, tkw = mk(max(n_regs, 1), ALN_REG_DTYPE.itemsize, 0xee), mk(max(plan.n_items_cap, 1), ALN_ITEM_DTYPE.itemsize, 0xff), mk(max(plan.n_tasks_cap, 1), KSW_TASK_DTYPE.itemsize, 0xff)
    cow = mk(plan.n_tasks_cap + 1, 0, -1)
    plw = torch.full((max(plan.pool_cap, 16) + 32,), 0xff, dtype=torch.uint8, device="cuda")
    pad = lambda v, n: v if v.numel() >= n else torch.cat([v, torch.zeros(n - v.numel(), dtype=v.dtype, device=v.device)])
    bd = pad(t(b).reshape(-1), 2 * plan.n_b_cap)
    plan.run(o, ref, n_reads, n_regs, t(u_off), t(regs), t(b_off), bd, t(read_off), pad(t(fwd), plan.reads_cap), n_b=n_b, aln_regs=arw[GUARD:GUARD + max(n_regs, 1)],
             items=itw[GUARD:GUARD + max(plan.n_items_cap, 1)], tasks=tkw[GUARD:GUARD + max(plan.n_tasks_cap, 1)], cig_off=cow[GUARD:GUARD + plan.n_tasks_cap + 1],
             pool=plw[16:16 + max(plan.pool_cap, 16)], stream=stream)
    rc, n_ref, n_big, tot = plan.counts()
    ar, it, tk, co, pl = arw.cpu().numpy(), itw.cpu().numpy(), tkw.cpu().numpy(), cow.cpu().numpy(), plw.cpu().numpy()
    guards = ((ar[:GUARD] == 0xee).all() and (ar[GUARD + max(n_regs, 1):] == 0xee).all() and (it[:GUARD] == 0xff).all() and (it[-GUARD:] == 0xff).all() and (tk[:GUARD] == 0xff).all() and
              (tk[-GUARD:] == 0xff).all() and (co[:GUARD] == -1).all() and (co[-GUARD:] == -1).all() and (pl[:16] == 0xff).all() and (pl[16 + plan.pool_cap:] == 0xff).all())
    out = dict(aln_regs=ar[GUARD:GUARD + n_regs].reshape(-1).view(ALN_REG_DTYPE), items=it[GUARD:GUARD + plan.n_items_cap].reshape(-1).view(ALN_ITEM_DTYPE),
               tasks=tk[GUARD:GUARD + plan.n_tasks_cap].reshape(-1).view(KSW_TASK_DTYPE), cig_off=co[GUARD:GUARD + plan.n_tasks_cap + 1], pool=pl[16:16 + plan.pool_cap],
               b=bd.cpu().numpy().view(np.uint64)[:2 * b.shape[0]].reshape(-1, 2), totals=tot, rc=rc, n_refused=n_ref, n_too_big=n_big)
    return out, bool(guards)


def same(got, want, what=""):
    """every output array equals the model's, the fill behind the used parts included (the model fills with 0xff as run_plan does)"""
    for k in ("aln_regs", "items", "tasks", "cig_off", "pool", "b"):
        g, w = got[k], want[k]
        n = min(g.size, w.size) if k != "b" else None
        if k == "b":
            assert np.array_equal(g, w), (what, k)
        else:
            assert g[:n].tobytes() == w[:n].tobytes(), (what, k, first_diff(g[:n], w[:n]))
            assert (g[n:].view(np.uint8) == 0xff).all() and (w[n:].view(np.uint8) == 0xff).all(), (what, k, "fill")
    assert tuple(got["totals"]) == tuple(want["totals"]), (what, got["totals"], want["totals"])


def first_diff(g, w):
    gb, wb = g.view(np.uint8).reshape(g.size, -1), w.view(np.uint8).reshape(w.size, -1)
    rows = np.nonzero((gb != wb).any(1))[0]
    return (int(rows[0]), g[rows[0]], w[rows[0]]) if rows.size else None


def plan_for(c, want, slack=SLACK, slot_words=SLOT_WORDS, **kw):
    from mm2chain import AlnPlan
    tot = want["totals"]
    return AlnPlan(max(int(c[0][-1]), 1), tot[0] + slack, tot[1] + slack, tot[3] + 8 * slack, c[3].shape[0], c[5].size, n_slots=64, slot_words=slot_words, **kw)


def reverse(c):
    """the reads and the regions of every read in reverse order; the anchors of a region stay where they are in their read"""
    u_off, regs, b_off, b, read_off, fwd, names = c
    n = len(u_off) - 1
    order = list(range(n))[::-1]
    rg = [regs[u_off[r]:u_off[r + 1]][::-1] for r in order]
    nm = [names[int(u_off[r]):int(u_off[r + 1])][::-1] for r in order]
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (off([x.size for x in rg]), np.concatenate(rg), off([b_off[r + 1] - b_off[r] for r in order]), np.concatenate([b[b_off[r]:b_off[r + 1]] for r in order]),
            off([read_off[r + 1] - read_off[r] for r in order]), np.concatenate([fwd[read_off[r]:read_off[r + 1]] for r in order]), [x for y in nm for x in y])


@pytest.mark.parametrize("name", sorted(D.OPTS))
def test_every_region_in_batches_both_orders(name, fx, ref, model):
    o, c, want = model[name]
    plan = plan_for(c, want)
    got, guards = run_plan(plan, ref, opt_of(o), c)
    assert got["rc"] == 0 and guards
    same(got, want, name)
    assert M.fixture_mismatches(name, got, fx, c[6]) == []                      # ... and what the device planned is what the reference's mm_align1 called
    rc_ = reverse(c)
    want_r = M.run(o, D.reference(), *rc_[:6], slot_words=SLOT_WORDS)
    got_r, guards = run_plan(plan, ref, opt_of(o), rc_)
    assert got_r["rc"] == 0 and guards
    same(got_r, want_r, name + " reversed")
    assert sorted(map(tuple, (M.task_records(got_r, g)[0] for g in range(len(rc_[6])))), key=str) == sorted(map(tuple, (M.task_records(got, g)[0] for g in range(len(c[6])))), key=str)
    ms = plan.last_kernel_ms()
    assert len(ms) == 3 and all(v >= 0 for v in ms)
    plan.close()


def repeat(c, k):
    """the reads of a batch k times over in one call"""
    u_off, regs, b_off, b, read_off, fwd, names = c
    off = lambda o: np.concatenate([[0], np.cumsum(np.tile(np.diff(o), k))]).astype(np.int64)
    return off(u_off), np.tile(regs, k), off(b_off), np.tile(b, (k, 1)), off(read_off), np.tile(fwd, k), list(names) * k


def test_more_regions_than_one_scan_chunk(ref, model):
    """the asm20 batch five times over in one call, 1 285 regions: aln_scan takes them in chunks of 1 024, so the offsets of the second chunk are the first chunk's
    totals plus its own prefix sums.  Every byte equals the model's, and every copy plans the tasks of the batch run once (which
    test_every_region_in_batches_both_orders holds against the reference's record)."""
    o, c, want1 = model["asm20"]
    c5 = repeat(c, 5)
    n = int(c5[0][-1])
    assert n > 1024 and n % 1024 != 0
    want = M.run(o, D.reference(), *c5[:6], slot_words=SLOT_WORDS)
    plan = plan_for(c5, want)
    got, guards = run_plan(plan, ref, opt_of(o), c5)
    assert got["rc"] == 0 and guards
    same(got, want, "asm20 x 5")
    n1 = int(c[0][-1])
    assert all(M.task_records(got, g) == M.task_records(want1, g % n1) for g in range(n))
    plan.close()


def one_region(c, g):
    """region g of a batch alone in a call, with its read"""
    u_off, regs, b_off, b, read_off, fwd, names = c
    r = int(np.searchsorted(u_off, g, side="right") - 1)
    return (np.array([0, 1], np.int64), regs[g:g + 1], np.array([0, b_off[r + 1] - b_off[r]], np.int64), b[b_off[r]:b_off[r + 1]], np.array([0, read_off[r + 1] - read_off[r]], np.int64),
            fwd[read_off[r]:read_off[r + 1]], [names[g]])


def test_planted_regions_one_per_call(ref, model):
    from mm2chain import AlnPlan
    plan = AlnPlan(1, 700, 700, 1 << 18, 4096, 1 << 17, n_slots=4, slot_words=SLOT_WORDS)
    seen = set()
    todo = [(o, c, want, g) for o, c, want in (model["ont"], model["ont_noflt"], model["hpc"], model["sr"]) for g, nm in enumerate(c[6]) if not nm.startswith("rand")]
    for o, c, want, g in todo:
        seen.add(c[6][g])
        c1 = one_region(c, g)
        got, guards = run_plan(plan, ref, opt_of(o), c1)
        assert got["rc"] == 0 and guards, c[6][g]
        assert M.task_records(got, 0) == M.task_records(want, g), c[6][g]
        f = ["as1", "cnt1", "rs", "qs", "re", "qe", "rs0", "qs0", "re0", "qe0", "n_items", "n_tasks", "status", "rev"]
        assert got["aln_regs"][f][0] == want["aln_regs"][f][g], c[6][g]
    assert {"cnt129", "gaps65", "lg2048", "lg2049", "short_span", "alt4", "tandem_last", "self_left", "rs_zero", "ctg_end", "inversion", "hp_q1_ctg0", "hp_first20_last2", "sr_equal", "sr_wave", "sr_n"} <= seen
    plan.close()


def test_host_entry(fx, model):
    from mm2chain import align_tasks_batch
    for name in ("asm20", "ont_sw"):
        o, c, want = model[name]
        tot = want["totals"]
        got = align_tasks_batch(opt_of(o), *D.reference(), *c[:6], tot[0], tot[1], tot[3], fill=0xff)
        assert got["rc"] == 0
        same(got, want, name)
        assert M.fixture_mismatches(name, got, fx, c[6]) == []


def test_plan_again_on_other_data_behind_another_kernel(ref, model):
    o, c, want = model["ont_g300"]
    o2, c2, want2 = model["asm20"]
    big = want if want["totals"][3] > want2["totals"][3] else want2
    from mm2chain import AlnPlan
    plan = AlnPlan(max(int(c[0][-1]), int(c2[0][-1])), max(want["totals"][0], want2["totals"][0]), max(want["totals"][1], want2["totals"][1]), big["totals"][3],
                   max(c[3].shape[0], c2[3].shape[0]), max(c[5].size, c2[5].size), n_slots=16)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        x = torch.randn(2048, 2048, device="cuda")
        y = x @ x                                                               # another kernel in front on the caller's stream
        got, guards = run_plan(plan, ref, opt_of(o), c, stream=st.cuda_stream)
        y = y @ x
        got2, guards2 = run_plan(plan, ref, opt_of(o2), c2, stream=st.cuda_stream)
    assert guards and guards2 and got["rc"] == 0 and got2["rc"] == 0 and y.numel() > 0
    for g_, w_, cc in ((got, want, c), (got2, want2, c2)):
        for g in range(len(cc[6])):
            assert M.task_records(g_, g) == M.task_records(w_, g)
        assert np.array_equal(g_["b"], w_["b"]) and tuple(g_["totals"]) == tuple(w_["totals"])
    plan.close()


def test_refusals(ref, model):
    """every kind of refusal: only the status is written, the anchors are untouched, the neighbours are exact"""
    from mm2chain import ALN_REFUSED, ALN_TOO_BIG
    o, c, want = model["ont"]
    reads = [r for r in D.cached_batches()["ont"][1] if r["name"] in ("cnt64", "fbs1", "alt2", "two_regions", "cnt3")]

    def variant(mutate):
        rs = [dict(r, a=r["a"].copy(), regs=r["regs"].copy()) for r in reads]
        mutate(rs[1])
        return D.csr(rs)
    n_seq = len(D.CONTIG_LENS)

    def set_x(r, i, x):
        r["a"][i, 0] = np.uint64(x)
    cases = {
        "as leaves the anchors": lambda r: r["regs"].__setitem__("as", -1),
        "cnt leaves the anchors": lambda r: r["regs"].__setitem__("cnt", r["a"].shape[0] + 1),
        "negative cnt": lambda r: r["regs"].__setitem__("cnt", -3),
        "another strand inside": lambda r: set_x(r, 5, int(r["a"][5, 0]) | (1 << 63)),
        "another contig inside": lambda r: set_x(r, 5, (int(r["a"][5, 0]) & 0xffffffff) | (1 << 32)),
        "rid beyond n_seq": lambda r: r["a"].__setitem__((slice(None), 0), (r["a"][:, 0] & np.uint64(0xffffffff)) | np.uint64(n_seq << 32)),
        "anchor beyond its contig": lambda r: set_x(r, r["a"].shape[0] - 1, (int(r["a"][-1, 0]) & ~0xffffffff) | D.CONTIG_LENS[5]),
        "anchor beyond its read": lambda r: r["a"].__setitem__((-1, 1), np.uint64((15 << 32) | r["fwd"].size)),
        "anchors running backwards": lambda r: set_x(r, 7, int(r["a"][6, 0]) - 1),
        "qs0 below 0 (:626)": lambda r: r["a"].__setitem__((0, 1), np.uint64((15 << 32) | 3)),
    }
    plan = plan_for(D.csr(reads), M.run(o, D.reference(), *D.csr(reads)[:6]), slack=64)
    for what, mutate in cases.items():
        cv = variant(mutate)
        got, guards = run_plan(plan, ref, opt_of(o), cv)
        wantv = M.run(o, D.reference(), *cv[:6])
        g_bad = int(cv[0][1])
        assert guards and got["rc"] == -2 and got["n_refused"] == 1 and got["aln_regs"]["status"][g_bad] == ALN_REFUSED, what
        assert wantv["aln_regs"]["status"][g_bad] == M.REFUSED and got["aln_regs"][g_bad].tobytes() == wantv["aln_regs"][g_bad].tobytes(), what
        assert np.array_equal(got["b"][cv[2][1]:cv[2][2]], cv[3][cv[2][1]:cv[2][2]]), what + ": the anchors of a refused region are touched"
        same(got, dict(wantv, totals=got["totals"]), what)
        assert tuple(got["totals"]) == tuple(wantv["totals"]), what
    # modes that are refused whole: splice; sr on an HPC index (:575)
    cv = D.csr(reads)
    for kw in (dict(flag=4), dict(flag=1, idx_flag=1)):
        got, guards = run_plan(plan, ref, opt_of(o, **kw), cv)
        assert guards and got["rc"] == -2 and got["n_refused"] == len(cv[6]) and (got["aln_regs"]["status"] == ALN_REFUSED).all() and np.array_equal(got["b"], cv[3]), kw
        assert (got["pool"] == 0xff).all() and (got["items"].view(np.uint8) == 0xff).all() and tuple(got["totals"]) == (0, 0, 0, 0), kw
    # offsets that leave a capacity
    bad_off = list(cv); bad_off[4] = cv[4].copy(); bad_off[4][2:] += 1 << 20
    got, guards = run_plan(plan, ref, opt_of(o), tuple(bad_off))
    assert guards and got["rc"] == -2 and got["n_refused"] >= 1 and got["aln_regs"]["status"][0] == 0
    plan.close()
    # more long gaps than LDS and slot: TOO_BIG, not run, anchors untouched; the 2 048 beside it is exact
    o = model["ont_noflt"][0]
    lg = [r for r in D.cached_batches()["ont_noflt"][1] if r["name"] in ("lg2048", "lg2049", "fbs1")]
    cl = D.csr(lg)
    wl = M.run(o, D.reference(), *cl[:6], slot_words=0)
    assert list(wl["aln_regs"]["status"]) == [M.TOO_BIG if nm == "lg2049" else 0 for nm in cl[6]]
    plan = plan_for(cl, wl, slot_words=0)
    got, guards = run_plan(plan, ref, opt_of(o), cl)
    assert guards and got["rc"] == -3 and got["n_too_big"] == 1 and got["n_refused"] == 0
    same(got, wl, "too big")
    g = cl[6].index("lg2049")
    assert got["aln_regs"]["status"][g] == ALN_TOO_BIG and np.array_equal(got["b"][cl[2][g]:cl[2][g + 1]], cl[3][cl[2][g]:cl[2][g + 1]])
    plan.close()


def test_each_capacity_exceeded_by_one(ref, model):
    from mm2chain import AlnPlan, ALN_OVER_CAP
    o, c, want = model["ont_noflt"]
    tot = want["totals"]
    last = len(c[6]) - 1
    assert want["aln_regs"]["n_items"][last] > 0 and want["aln_regs"]["n_tasks"][last] > 0
    for k, caps in enumerate(((tot[0] - 1, tot[1], tot[3]), (tot[0], tot[1] - 1, tot[3]), (tot[0], tot[1], tot[3] - 1))):
        wantc = M.run(o, D.reference(), *c[:6], caps=caps)
        assert wantc["aln_regs"]["status"][last] == M.OVER_CAP and (wantc["aln_regs"]["status"][:last] == 0).all()
        plan = AlnPlan(len(c[6]), caps[0], caps[1], caps[2], c[3].shape[0], c[5].size, n_slots=32, slot_words=SLOT_WORDS)
        got, guards = run_plan(plan, ref, opt_of(o), c)
        assert guards and got["rc"] == -3 and got["n_too_big"] == 1 and got["aln_regs"]["status"][last] == ALN_OVER_CAP, k
        same(got, wantc, "capacity %d" % k)
        assert tuple(got["totals"]) == tuple(tot)                               # what the batch takes is still told
        plan.close()


def test_chained_into_the_ksw_plan(fx, ref, model):
    """the plan's device outputs straight into KswPlan.run on the map-ont score set, no download between: the eleven ez fields of every first-pass task equal the
    reference's recorded ones, for the regions that ran to their end"""
    from mm2chain import AlnPlan, KswPlan, KSW_RES_DTYPE, KSW_TASK_DTYPE, ALN_REG_DTYPE, params
    name = "ont_g300"
    o, c, want = model[name]
    tot = want["totals"]
    u_off, regs, b_off, b, read_off, fwd = c[:6]
    plan = AlnPlan(len(c[6]), tot[0], tot[1], tot[3], b.shape[0], fwd.size, cig_shift=0, n_slots=64)
    ar, items, tasks, cig_off, pool = plan.run(opt_of(o), ref, len(u_off) - 1, len(c[6]), t(u_off), t(regs), t(b_off), t(b).reshape(-1), t(read_off), t(fwd))
    kp = KswPlan(tot[1], tot[3], tot[2], scratch_bytes=256 << 20)
    res, cigar = kp.run(params.ksw_scores("map-ont"), tot[1], tasks, pool, cig_off)
    plan.check(); kp.check()
    res = res.cpu().numpy().reshape(-1).view(KSW_RES_DTYPE)[:tot[1]]
    ar = ar.cpu().numpy().reshape(-1).view(ALN_REG_DTYPE)
    calls, call_off, dropped = fx[name + "_calls"], fx[name + "_call_off"], fx[name + "_dropped"]
    F = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "n_cigar", "reach_end")
    n = 0
    for g in range(len(c[6])):
        if dropped[g]:
            continue
        rec = calls[call_off[g]:call_off[g + 1]]
        assert rec.shape[0] == ar["n_tasks"][g]
        for j in range(rec.shape[0]):
            r = res[int(ar["task0"][g]) + j]
            assert r["status"] == 0 and [int(np.int32(r[f])) for f in F] == [int(v) for v in rec[j, 8:]], (c[6][g], j)
            n += 1
    assert n > 500
    kp.close(); plan.close()
