"""The cases of the fragment tests behind mm_gen_regs (mm_select_sub_multi pe.c:6-43, csrc/chain_hits.hip; mm_seg_gen hit.c:373-427, csrc/chain_segs.hip), made again
deterministically wherever they are needed.  A case is one fragment: {"name", "n_segs", "qlens", "hash", "u", "a", "hit" (mm2c_hit_opt_t), "multi" (pri1, pri2),
"gap_ref" (the fragment's max_chain_gap_ref), "mapq" (mm2c_mapq_opt_t), "rep_len"} -- chains with their anchors in the coordinates of the concatenated segments, the
segment of an anchor in bits 48-55 of y.  tests/golden/ref_seg.npz holds what the reference's own hit.o and pe.o make of them (tests/golden/make_ref_seg_fixtures.py).

Frag(...).chain(score, qs, qe, rs, ...) puts a chain whose region will be [qs, qe) on the fragment and [rs, re) on the reference; regions come out in descending
score (mm_gen_regs), so the scores of a case say who is region 0, 1, ...  A child is a chain over its parent's query interval.

The float products (pe.c:20, 26, 29: (float)score >= (float)pscore * ratio).  pscore * ratio is exact in double (24 x 24 bits).  Float and double can only decide
differently when the float product rounds onto an integer s that the exact product lies above (an integer is a float: a product at or below s never rounds above
it), that is for ratios that lie above their decimal: 0.2f = 0.2000000030 (pri1: 5 * 0.2f = 1.0000000149, in float 1.0f, so score 1 is kept), 0.8f (a pri_ratio
one may pass: 5 * 0.8f -> 4.0f) and 0.3f (10 * 0.3f -> 3.0f).  0.7f = 0.6999999881 lies below 0.7 and 0.5f is exact: for pri2 = 0.7f and pri_ratio = 0.5f NO score
exists on which float and double differ, and none is planted; "f32_pri2_03" plants the pri2 branch with 0.3f instead."""
import numpy as np

INT_MAX = 2**31 - 1
HIT_SR = dict(mask_level=0.5, mask_len=INT_MAX, hard_mask_level=0, pri_ratio=0.5, min_diff=0, best_n=20)      # options.c:123-132 (-x sr); min_diff is 2k = 42 there
MULTI = dict(pri1=0.2, pri2=0.7)                                                                            # map.c:254
MAPQ_SR = dict(do_join=0, max_join_long=20000, max_join_short=2000, min_join_flank_sc=1000, min_join_flank_ratio=0.5, min_cnt=2, min_chain_score=25)
SPAN = 15
FAR = 5000000                                                                  # "not close": another place on the reference


def hopt(**kw):
    o = dict(HIT_SR)
    o.update(kw)
    return o


class Frag:
    def __init__(self, name, qlens=(150, 150), hit=None, multi=None, gap_ref=500, mapq=None, rep_len=0):
        self.name, self.qlens, self.hit, self.multi, self.gap_ref = name, tuple(qlens), hit or hopt(), multi or dict(MULTI), gap_ref
        self.mapq, self.rep_len, self.chains = mapq or dict(MAPQ_SR), rep_len, []

    def chain(self, score, qs, qe, rs=10000, re=None, rid=0, rev=0, n=4, span=SPAN, sids=None, rev_bits=None):
        """n anchors from (rs, qs) to (re, qe), evenly; sids: the segment of every anchor (default: the segment the k-mer's first base lies in); rev_bits: the strand
        bit of every anchor (default rev; mm_gen_regs reads the first)"""
        qsum = sum(self.qlens)
        re = rs + (qe - qs) if re is None else re
        i = np.arange(n, dtype=np.int64)
        d = max(n - 1, 1)
        xs = (rs + span - 1) + (re - rs - span) * i // d
        y0, y1 = (qs + span - 1, qe - 1) if not rev else (qsum - qe + span - 1, qsum - qs - 1)
        ys = y0 + (y1 - y0) * i // d
        if sids is None:                                                        # the k-mer's first base on its own strand decides, so no coordinate goes below 0
            fwd = ys + 1 - span if not rev else qsum - 1 - (ys + 1 - span)
            acc = np.cumsum(self.qlens)
            sids = np.minimum(np.searchsorted(acc, fwd, side="right"), len(self.qlens) - 1)
        sids = np.asarray(sids, np.uint64)
        rb = np.full(n, rev, np.uint64) if rev_bits is None else np.asarray(rev_bits, np.uint64)
        assert sids.size == n and rb.size == n
        a = np.zeros((n, 2), np.uint64)
        a[:, 0] = (rb << np.uint64(63)) | (np.uint64(rid) << np.uint64(32)) | xs.astype(np.uint64)
        a[:, 1] = (sids << np.uint64(48)) | (np.uint64(span) << np.uint64(32)) | ys.astype(np.uint64)
        self.chains.append((int(score), a))
        return self

    def case(self):
        u = np.array([(s << 32) | a.shape[0] for s, a in self.chains], np.uint64)
        a = np.concatenate([a for _, a in self.chains]) if self.chains else np.zeros((0, 2), np.uint64)
        h = (sum(ord(c) * 31 ** k for k, c in enumerate(self.name)) * 2654435761) & 0xffffffff
        return {"name": self.name, "n_segs": len(self.qlens), "qlens": np.array(self.qlens, np.int32), "hash": h, "u": u, "a": np.ascontiguousarray(a),
                "hit": self.hit, "multi": self.multi, "gap_ref": self.gap_ref, "mapq": self.mapq, "rep_len": self.rep_len}


def random_frag(name, rng, n, qlen=2000, **kw):
    """n chains of distinct scores at random places of a 2 x qlen fragment, on two reference sequences and both strands, near enough to each other that some are close"""
    f = Frag(name, (qlen, qlen), **kw)
    for sc in rng.permutation(np.arange(30, 30 + 5 * n, 5)):
        ln = int(rng.integers(20, 60))
        qs = int(rng.integers(0, 2 * qlen - ln))
        f.chain(int(sc), qs, qs + ln, rs=int(rng.integers(10000, 14000)), rid=int(rng.integers(0, 2)), rev=int(rng.integers(0, 2)), n=int(rng.integers(2, 5)))
    return f


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    C = []
    add = lambda f: C.append(f.case())
    rng = np.random.default_rng(20261020)
    # ================= mm_select_sub_multi =================
    add(Frag("sel_primaries_only").chain(100, 0, 60).chain(90, 80, 140, rs=20000).chain(80, 160, 290, rs=30000, rev=1))
    for md in (70, 69):                                                         # kept by min_diff alone: 30 + 70 >= 100; one less and the ratio (not close: 0.5) drops it
        add(Frag(f"sel_min_diff_{md}", hit=hopt(min_diff=md)).chain(100, 0, 140).chain(30, 0, 140, rs=FAR))
    for pr in (0.0, -1.0):                                                      # pri_ratio <= 0: nothing beyond mm_set_parent, whatever would be dropped
        add(Frag(f"sel_pri_ratio_{pr}", hit=hopt(pri_ratio=pr)).chain(100, 0, 140).chain(30, 0, 140, rs=FAR).chain(20, 5, 140, rs=2 * FAR))
    # ---- the two distance compares: max_dist = 150 + 150 + 500 = 800.  Parent [10000, 10140) of score 100, child of score 30: close -> 0.2 keeps it, not close -> 0.5 drops it
    for D in (799, 800, 801):
        add(Frag(f"sel_dist_down_{D}").chain(100, 0, 140).chain(30, 0, 140, rs=10000 + D - 140))            # q->re - p->rs = D
        add(Frag(f"sel_dist_up_{D}").chain(100, 0, 140).chain(30, 0, 140, rs=10140 - D))                     # p->re - q->rs = D
    add(Frag("sel_dist_799_other_rev").chain(100, 0, 140).chain(30, 0, 140, rs=10000 + 799 - 140, rev=1))
    add(Frag("sel_dist_799_other_rid").chain(100, 0, 140).chain(30, 0, 140, rs=10000 + 799 - 140, rid=1))
    for g in (500, 499):                                                        # one geometry, two fragments of one batch whose gap_ref decides
        add(Frag(f"sel_gap_ref_{g}", gap_ref=g).chain(100, 0, 140).chain(30, 0, 140, rs=10000 + 799 - 140))
    add(Frag("sel_gap_ref_wraps", gap_ref=INT_MAX).chain(100, 0, 140).chain(30, 0, 140, rs=10000 + 100))     # 300 + INT_MAX wraps below zero: nothing is close
    # ---- is_par_both / is_chi_both: parent 100, child 60 (passes 0.5, fails 0.7), child far away.  Only (parent both, child not) takes pri2
    both = lambda name, p, c: add(Frag(name).chain(100, p[0], p[1]).chain(60, c[0], c[1], rs=FAR))
    both("sel_both_par0_chi0", (0, 140), (0, 130))
    both("sel_both_par1_chi1", (0, 300), (10, 290))
    both("sel_both_par0_chi1", (0, 150), (10, 160))
    both("sel_both_par1_chi0", (0, 300), (0, 150))
    both("sel_both_par_qs149", (149, 300), (150, 290)); both("sel_both_par_qs150", (150, 300), (150, 290))
    both("sel_both_par_qe150", (0, 150), (0, 140)); both("sel_both_par_qe151", (0, 151), (0, 140))
    both("sel_both_chi_qs149", (0, 300), (149, 290)); both("sel_both_chi_qs150", (0, 300), (150, 290))
    both("sel_both_chi_qe150", (0, 300), (10, 150)); both("sel_both_chi_qe151", (0, 300), (10, 151))
    # ---- n_segs = 3: max_dist = 0 (a neighbour 200 away is not close), and nobody spans "both"
    add(Frag("sel_three_segs_not_close", (100, 100, 100)).chain(100, 0, 90).chain(30, 0, 90, rs=10200))
    add(Frag("sel_three_segs_no_both", (100, 100, 100)).chain(100, 0, 300).chain(60, 0, 100, rs=FAR))
    # ---- the three ratios at, below and above the product
    for sc in (19, 20, 21):
        add(Frag(f"sel_pri1_{sc}").chain(100, 0, 140).chain(sc, 0, 140, rs=10200))
    for sc in (49, 50, 51):
        add(Frag(f"sel_pri_ratio_{sc}").chain(100, 0, 140).chain(sc, 0, 140, rs=FAR))
    for sc in (69, 70, 71):
        add(Frag(f"sel_pri2_{sc}").chain(100, 0, 300).chain(sc, 0, 150, rs=FAR))
    add(Frag("f32_pri1_5_1").chain(5, 0, 140).chain(1, 0, 140, rs=10200))                                    # 5 * 0.2f: 1.0f in float, above 1 in double
    add(Frag("f32_pri_ratio_08", hit=hopt(pri_ratio=0.8)).chain(5, 0, 140).chain(4, 0, 140, rs=FAR))         # 5 * 0.8f -> 4.0f
    add(Frag("f32_pri2_03", multi=dict(pri1=0.2, pri2=0.3)).chain(10, 0, 300).chain(3, 0, 150, rs=FAR))      # 10 * 0.3f -> 3.0f
    # ---- best_n: every secondary that passed counts, kept or not; one that failed does not
    kids = lambda f, scs: [f.chain(sc, 0, 140 - j, rs=FAR * (j + 1)) for j, sc in enumerate(scs)] and f
    for bn in (0, 1, 3):
        add(kids(Frag(f"sel_best_n_{bn}", hit=hopt(best_n=bn)).chain(100, 0, 140), (90, 80, 70)))
    # 90 passes (0.7), 65 fails (0.7) and does not count, 60 and 55 span both segments and pass (0.5): 60 is the second, 55 is dropped
    add(Frag("sel_best_n_2_one_fails", hit=hopt(best_n=2)).chain(100, 0, 300).chain(90, 0, 150, rs=FAR).chain(65, 0, 149, rs=2 * FAR).chain(60, 10, 290, rs=3 * FAR)
        .chain(55, 20, 280, rs=4 * FAR))
    # ---- no identical-hit test: the twin of the parent stays (mm_select_sub would drop it)
    add(Frag("sel_identical_kept").chain(100, 0, 140).chain(90, 0, 140))
    # ---- the parent's position overwritten by the compaction: regions A, k1 (dropped), B, C, k4 (child of B, judged against C, which lies at position 2 by then)
    ow = lambda name, B, C, k4: add(Frag(name).chain(500, 0, 90).chain(120, 0, 88, rs=FAR, rid=1).chain(B[0], 210, 290, rs=20000).chain(C[0], C[1], C[2], rs=30000, rev=C[3])
                                    .chain(k4[0], 215, 285, rs=k4[1], rid=k4[2]))
    ow("sel_overwritten_score", (110,), (60, 100, 140, 0), (40, FAR, 1))          # 40 < 55 against B, 40 >= 30 against C
    ow("sel_overwritten_rev", (110,), (105, 100, 140, 1), (30, 20100, 0))         # close to B (pri1: 30 >= 22); C is on the other strand: 0.5, 30 < 52.5
    ow("sel_overwritten_both", (110,), (100, 100, 200, 0), (60, FAR, 1))          # against B 0.5 (60 >= 55); C spans both segments: 0.7, 60 < 70
    # ---- sync: nothing dropped (ids and sam_pri untouched) / something dropped
    add(Frag("sel_nothing_dropped").chain(100, 0, 140).chain(90, 0, 130, rs=FAR).chain(80, 160, 290, rs=20000).chain(70, 160, 280, rs=2 * FAR))
    add(Frag("sel_first_child_dropped").chain(100, 0, 140).chain(20, 0, 130, rs=FAR).chain(80, 160, 290, rs=20000).chain(70, 160, 280, rs=2 * FAR))
    # ---- both table routes
    add(random_frag("sel_random40", rng, 40, hit=hopt(min_diff=10)))
    add(random_frag("sel_random128", rng, 128, hit=hopt(min_diff=10)))
    add(random_frag("sel_random129", rng, 129, hit=hopt(min_diff=10, best_n=5)))
    # ================= mm_seg_gen =================
    add(Frag("seg_which_segment", rep_len=40).chain(100, 5, 140).chain(90, 160, 290, rs=20000).chain(80, 100, 220, rs=30000, n=8))
    add(Frag("seg_reverse_spans").chain(100, 5, 140, rev=1, n=6).chain(90, 100, 220, rs=20000, rev=1, span=19, n=9).chain(80, 150, 295, rs=30000, rev=1, span=19, n=5)
        .chain(70, 20, 120, rs=40000, n=5, span=19))
    # the strand bit of the anchor itself turns y, not the region's: anchors of one chain with both bits (the region's rev is the first anchor's)
    add(Frag("seg_mixed_strand_bits").chain(100, 60, 240, n=8, rev_bits=[0, 1, 0, 1, 1, 0, 1, 0]).chain(90, 60, 240, rs=20000, rev=1, n=6, rev_bits=[1, 0, 0, 1, 0, 1]))
    add(Frag("seg_three_segs_middle", (100, 100, 100), rep_len=7).chain(100, 110, 190).chain(90, 20, 280, rs=20000, n=12).chain(80, 150, 290, rs=30000, rev=1, n=7))
    add(Frag("seg_zero_length_segment", (100, 0, 100)).chain(100, 10, 190, n=9).chain(90, 105, 195, rs=20000).chain(80, 20, 180, rs=30000, rev=1, n=6))
    # a dropped region: `as` has a hole behind the selection and its anchors appear nowhere; chains in a[] are not in score order either
    add(Frag("seg_dropped_region").chain(80, 160, 290, rs=20000, n=5).chain(20, 0, 130, rs=FAR, n=7).chain(100, 0, 140, n=6).chain(95, 100, 200, rs=30000, n=6))
    add(Frag("seg_empty_fragment"))
    # rows of 64 anchors
    big = (1000, 1000)
    for n in (63, 64, 65):
        add(Frag(f"seg_cnt_{n}", big).chain(300, 10, 1990, n=n))
    add(Frag("seg_change_63_64", big).chain(300, 10, 1990, n=130, sids=[0] * 64 + [1] * 66))
    add(Frag("seg_change_64_65", big).chain(300, 10, 1990, n=130, sids=[0] * 65 + [1] * 65))
    add(Frag("seg_alternating", big).chain(300, 10, 1990, n=100, sids=[j % 2 for j in range(100)]).chain(200, 10, 1900, rs=20000, rev=1, n=70, sids=[(j // 3) % 2 for j in range(70)]))
    add(Frag("seg_long_run", big).chain(300, 10, 1990, n=200, sids=[0] * 130 + [1] * 70))
    add(Frag("seg_three_alternating", (400, 400, 400)).chain(300, 10, 1190, n=150, sids=[(j * 7) % 3 for j in range(150)]))
    # a region across anchor 4096 of the fragment
    f = Frag("seg_across_4096", big)
    for j in range(14):
        f.chain(900 - 10 * j, 100 * j, 100 * j + 400, rs=10000 + 1000 * j, rev=j % 2, n=300)
    add(f)
    for n in (64, 65):                                                          # many regions
        f = Frag(f"seg_regions_{n}", (2000, 2000))
        for j in range(n):
            f.chain(500 - 3 * j, 60 * j, 60 * j + 50 + (50 if j % 9 == 0 else 0), rs=10000 + 300 * j, rev=j % 3 == 0, n=3 + j % 4)
        add(f)
    # equal sort keys: twins (same score, same anchors) give segment chains of equal z.x -- among more than 64 chains of a segment, where klib's sort is not stable
    f = Frag("seg_tied_keys_70", (2000, 2000), hit=hopt(min_diff=0))
    for j in range(60):                                                         # every anchor says segment 0, whatever its place: 70 chains in one segment read
        for _ in range(2 if j % 6 == 0 else 1):
            f.chain(500 - 3 * j, 60 * j, 60 * j + 50, rs=10000 + 300 * j, n=4, sids=[0, 0, 0, 0])
    add(f)
    add(Frag("seg_tied_keys_pair").chain(100, 100, 200, n=6).chain(100, 100, 200, n=6).chain(90, 0, 80, rs=20000))
    _CASES = C
    assert len({c["name"] for c in C}) == len(C)
    return C


def seg_len(cs):
    """-> int32 [sum n_segs] of cases with one n_segs: the qlens, fragment-major"""
    return np.concatenate([c["qlens"] for c in cs]).astype(np.int32) if cs else np.zeros(0, np.int32)


def group_key(c):
    return (c["n_segs"],) + tuple(sorted(c["hit"].items())) + tuple(sorted(c["multi"].items())) + tuple(sorted(c["mapq"].items()))


def groups(cs=None):
    """the cases grouped by equal n_segs and options -> [[index into cases()]]"""
    cs = cases() if cs is None else cs
    g = {}
    for k, c in enumerate(cs):
        g.setdefault(group_key(c), []).append(k)
    return list(g.values())


_REF = None


def reference():
    """-> per case {"name", "case", "sel": the array behind mm_select_sub_multi, "segs": per segment {"u", "a", "regs" (out of mm_seg_gen), "final" (behind
    mm_set_parent and mm_set_mapq)}, "libm"} from tests/golden/ref_seg.npz; None when the fixture is absent"""
    global _REF
    import os
    from regs_model import REG
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_seg.npz")
    if _REF is not None or not os.path.exists(path):
        return _REF
    Z = np.load(path)
    cs = cases()
    assert int(Z["reg_size"]) == REG.itemsize and [str(v) for v in Z["names"]] == [c["name"] for c in cs]
    out = []
    for k, c in enumerate(cs):
        segs = []
        for t in range(int(Z["sr_off"][k]), int(Z["sr_off"][k + 1])):
            u0, u1, b0, b1 = (int(v) for v in (Z["su_off"][t], Z["su_off"][t + 1], Z["sb_off"][t], Z["sb_off"][t + 1]))
            segs.append({"u": Z["su"][u0:u1], "a": Z["sb"][b0:b1], "regs": Z["seg_regs"][u0:u1].reshape(-1).view(REG), "final": Z["seg_final"][u0:u1].reshape(-1).view(REG)})
        out.append({"name": c["name"], "case": c, "sel": Z["sel"][Z["sel_off"][k]:Z["sel_off"][k + 1]].reshape(-1).view(REG), "segs": segs, "libm": str(Z["libm"])})
    _REF = out
    return out
