"""Cases for the pair plan (csrc/pair_ends.hip): the smallest shapes at which each rule of mm_pair and mm_set_pe_thru (pe.c:45-63, 76-177) can go
wrong.  cases(): one fragment each, dict(name, qlens, opt, regs [REG of mate 0, REG of mate 1], pext PEXT, gap (the fragment's max_gap_ref, or None for the
option's), max_log_arg (of the plan the case wants, when not the default), refuse: why the plan refuses the fragment, cases the reference is not run on).  p of a
region is 1 + the index of its record in the case's pext.  tests/golden/make_ref_pair_fixtures.py runs the reference's own pe.o on them (tests/golden/ref_pair.npz).
The planted cases run with flip = 0: the flip of map.c:455-466 is not in pe.o; flip_cases() are derived by hand."""
import numpy as np

from fin_model import PEXT
from regs_model import REG

LDS_CLASS = 128
MAX_LOG_ARG = 4096                                                             # of the plans the tests make
DEFAULT = dict(max_gap_ref=500, pe_bonus=33, sub_diff=12, match_sc=2, pe_ori=1, flip=0)   # -x sr (options.c:126, 56; a = 2, b = 8; map.c:311-313 with 2 x 150 bases)
REV, SAM_PRI, PROPER, THRU = 1 << 10, 1 << 12, 1 << 13, 1 << 14


def _hash(s, i):
    return ((2 * i + s + 1) * 2654435761) & 0xffffffff


def case(name, m0, m1, qlens=(150, 150), gap=None, max_log_arg=None, refuse=None, **opt):
    """m0, m1: one dict per region, in order.  A region: rid 0, rev 0, rs / re, qs 0 / qe = the read's length, dp (dp_max) 100, parent 0 (region 0 is the mate's
    primary and has sam_pri), mapq 0, hash by position"""
    o = dict(DEFAULT)
    assert not set(opt) - set(o)
    o.update(opt)
    regs, px = [], []
    for s, specs in enumerate((m0, m1)):
        r = np.zeros(len(specs), REG)
        for i, sp in enumerate(specs):
            sp = dict(sp)
            dp, rev, mapq, pri = sp.pop("dp", 100), sp.pop("rev", 0), sp.pop("mapq", 0), sp.pop("sam_pri", 1 if i == 0 else 0)
            rs = sp.pop("rs", 1000)
            v = dict(id=i, cnt=10, rid=0, score=dp, qs=0, qe=qlens[s], rs=rs, re=rs + qlens[s], parent=0, subsc=0, mlen=qlens[s] - 5, blen=qlens[s], n_sub=0, score0=dp,
                     hash=_hash(s, i), div=0.0)
            v["as"] = 7 * i
            nop = sp.pop("no_p", False)
            assert not set(sp) - set(v), set(sp) - set(v)
            v.update(sp)
            for k, x in v.items():
                r[k][i] = x
            r["flags"][i] = (mapq & 0xff) | (REV if rev else 0) | (SAM_PRI if pri else 0) | s << 16   # seg_id = the mate
            if not nop:
                px.append((dp - 3, dp, 0, 0, 3, 0, 10 * len(px)))
                r["p"][i] = len(px)
        regs.append(r)
    c = dict(name=name, qlens=tuple(qlens), opt=o, regs=regs, pext=np.array(px, PEXT).reshape(-1), gap=gap, refuse=refuse)
    if max_log_arg is not None:
        c["max_log_arg"] = max_log_arg
    return c


def _alternate(n0):
    """n0 regions of mate 0 alternate between two rs with equal dp_max and hash; one region of mate 1 follows the first group: every region of the first group makes
    the same score with it, and the winner is the one the sort left last"""
    m0 = [dict(rs=1000 if i % 2 == 0 else 5000, hash=77, parent=0) for i in range(n0)]
    return m0, [dict(rs=1200, hash=5)]


def _mixed(n0, n1, seed, n_rid=3):
    """random regions on both mates, both strands, n_rid references, positions so dense that most entries have several candidates and many keys are equal"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (n0, n1):
        m = []
        for i in range(n):
            m.append(dict(rid=int(rng.integers(0, n_rid)), rs=int(rng.integers(0, 40)) * 50, rev=int(rng.integers(0, 2)), dp=int(rng.integers(40, 160)),
                          hash=int(rng.integers(0, 1 << 32)), parent=int(rng.integers(0, max(1, min(n, 3)))), mapq=int(rng.integers(0, 61)) if i < 3 else 0))
        for i in range(min(n, 3)):
            m[i]["parent"] = i if i == 0 or rng.integers(0, 2) else 0
        out.append(m)
    return out


def cases():
    C = []
    one = [dict(rs=1000, mapq=30)]
    C.append(case("empty", [], []))
    C.append(case("one_end_mate0", one, []))
    C.append(case("one_end_mate1", [], [dict(rs=1001, mapq=30)]))
    # both ends, mate 1 in front of mate 0: its odd key meets no `last`; the two primaries lie through each other
    C.append(case("no_pair_pe_thru", [dict(rs=1000)], [dict(rs=999)]))
    C.append(case("pe_thru_re_2", [dict(rs=1000)], [dict(rs=999, re=1152)]))
    C.append(case("pe_thru_off_by_3", [dict(rs=1000)], [dict(rs=997)]))
    C.append(case("pe_thru_re_off_by_3", [dict(rs=1000)], [dict(rs=999, re=1153)]))
    C.append(case("pe_thru_clip", [dict(rs=1000, qs=1)], [dict(rs=999, qs=1)]))              # neither clip condition of pe.c:58
    C.append(case("pe_thru_second_clip", [dict(rs=1000, qs=3)], [dict(rs=999)]))              # q->qs == 0 && qlens[0] - p->qe == 0
    C.append(case("pe_thru_other_rev", [dict(rs=1000)], [dict(rs=999, rev=1)]))
    C.append(case("pe_thru_found", [dict(rs=1000)], [dict(rs=1001)]))                         # a pair is found as well
    # primaries counted behind the lifts: the winner of mate 0 is the secondary 1, which lies through mate 1; its old primary 0 lies on another reference
    C.append(case("lift_pe_thru", [dict(rid=1, rs=5000), dict(rs=1000)], [dict(rs=1001)]))
    C.append(case("two_primaries", [dict(rs=1000), dict(rs=9000, parent=1)], [dict(rs=999)]))
    C.append(case("single_floor2", [dict(rs=1000)], [dict(rs=1200)]))
    C.append(case("single_rev1", [dict(rs=1200, rev=1)], [dict(rs=1000, rev=1)]))             # mate 1 in front on the reverse strand
    C.append(case("wrong_order_rev1", [dict(rs=1000, rev=1)], [dict(rs=1200, rev=1)]))
    C.append(case("other_rev", [dict(rs=1000)], [dict(rs=1200, rev=1)]))
    C.append(case("blend_raises", [dict(rs=1000, mapq=60)], [dict(rs=1200)]))
    C.append(case("floor1", [dict(rs=1000, dp=100), dict(rs=1010, dp=99)], [dict(rs=1200)], pe_bonus=1000))
    C.append(case("equal_hi_no_floor", [dict(rs=1000), dict(rs=1010)], [dict(rs=1200)]))
    # the maximum occurs twice, a third candidate lies five below: the second-largest IS the maximum -- no floor
    C.append(case("max_twice", [dict(rs=1000, hash=9), dict(rs=1010, hash=9), dict(rs=1020, dp=95)], [dict(rs=1200, hash=1)], pe_bonus=1000))
    C.append(case("negative_alt", [dict(rs=1000, dp=100), dict(rs=1010, dp=99), dict(rs=1020, dp=99)], [dict(rs=1200)], pe_bonus=1000))
    C.append(case("alt_lowers", [dict(rs=1000, dp=100, mapq=60), dict(rs=1010, dp=88)], [dict(rs=1200)], pe_bonus=1000))
    C.append(case("sub_diff_eq", [dict(rs=1000, dp=100, mapq=60), dict(rs=1010, dp=88)], [dict(rs=1200)], pe_bonus=1000))
    C.append(case("sub_diff_plus1", [dict(rs=1000, dp=100, mapq=60), dict(rs=1010, dp=87)], [dict(rs=1200)], pe_bonus=1000))
    # the winner of mate 0 is a secondary: the old primary lies on another reference
    C.append(case("lift_mate0", [dict(rid=1, rs=1000, mapq=40), dict(rs=1000), dict(rs=7000, parent=0), dict(rs=8000, parent=3)], [dict(rs=1200, mapq=20)]))
    C.append(case("lift_mate1", [dict(rs=1000, mapq=20)], [dict(rid=1, rs=1200, mapq=40), dict(rs=9000, parent=0), dict(rs=1200)]))
    C.append(case("lift_both", [dict(rid=1, rs=1000, mapq=40), dict(rs=1000)], [dict(rid=2, rs=1200, mapq=35), dict(rs=1200)]))
    # the winner's parent is itself a secondary: only the regions that name it follow, and its mapq goes
    C.append(case("lift_chain", [dict(rid=1, rs=1000, mapq=40), dict(rid=1, rs=3000, parent=0, mapq=7), dict(rs=1000, parent=1), dict(rs=5000, parent=1)], [dict(rs=1200)]))
    # sam_pri elsewhere than on the primary that wins
    C.append(case("sam_pri_moved", [dict(rs=1000, sam_pri=0), dict(rs=9000, sam_pri=1, parent=1)], [dict(rs=1200)]))
    C.append(case("under_dp_thres", [dict(rs=1000, dp=100), dict(rs=1010, dp=20)], [dict(rs=1200)]))          # 120 < 200 - 33: one candidate, the floor 2
    C.append(case("pe_bonus_above_sum", [dict(rs=1000, dp=100), dict(rs=1010, dp=20)], [dict(rs=1200)], pe_bonus=1000))
    C.append(case("negative_bonus_no_pair", [dict(rs=1000)], [dict(rs=1200)], pe_bonus=-1))
    C.append(case("gap_eq", [dict(rs=1000)], [dict(rs=1650)]))                                                  # 1650 - 1150 == 500
    C.append(case("gap_plus1", [dict(rs=1000)], [dict(rs=1651)]))
    C.append(case("gap_per_fragment", [dict(rs=1000)], [dict(rs=1651)], gap=501))
    C.append(case("gap_per_fragment_less", [dict(rs=1000)], [dict(rs=1650)], gap=499))
    C.append(case("break_on_rid", [dict(rid=0, rs=1000), dict(rid=1, rs=1000)], [dict(rid=1, rs=1200)]))
    # break, not continue: the walk ends at the short region 1 (gap 580), the long region 2 in front of it would pass the test
    C.append(case("break_hides_long", [dict(rs=2050, dp=90), dict(rs=1500, re=1520, dp=100), dict(rs=1000, re=2100, dp=100)], [dict(rs=2100)], pe_bonus=1000))
    # a far `last`: the short region 1 is the latest even key, 990 in front; the long region 0 in front of it ends 100 before mate 1
    C.append(case("far_last_hides", [dict(rs=1500, re=2900), dict(rs=2000, re=2010)], [dict(rs=3000)]))
    C.append(case("far_last_alone", [dict(rs=1500, re=2900)], [dict(rs=3000)]))                                  # ... and without region 1 the pair is found
    C.append(case("equal_scores_j", [dict(rs=1000, hash=9), dict(rs=1100, hash=9), dict(rs=1050, hash=9)], [dict(rs=1300, hash=1)]))
    C.append(case("equal_scores_i", [dict(rs=1000, hash=9)], [dict(rs=1300, hash=4), dict(rs=1200, hash=4), dict(rs=1250, hash=4)]))
    C.append(case("hash_wraps", [dict(rs=1000, hash=0xffffffff), dict(rs=1010, hash=3)], [dict(rs=1200, hash=2)]))
    # 157 x 11 candidates, all counted: n_sub = 1727, the difference of the high words 56, match_sc 3: (int)(6.02f * 56 / 3 - 4.343f * logf(1727)) is 80, with the
    # product kept exact 79; the blend turns that into 64 and 63
    C.append(case("contraction", [dict(rs=1000 + i, dp=1000 if i == 0 else 900, mapq=200 if i == 0 else 0) for i in range(157)],
                  [dict(rs=1300 + i, dp=1000 if i == 2 else 944) for i in range(11)], pe_bonus=10 ** 6, sub_diff=2000, match_sc=3))
    for n0 in (63, 64, 70, 127, 128, 131, 299):
        m0, m1 = _alternate(n0)
        C.append(case(f"alternate_{n0 + 1}", m0, m1))
    for n0, n1 in ((3, 4), (30, 34), (33, 32), (64, 64), (60, 69), (150, 150)):
        m0, m1 = _mixed(n0, n1, 1000 + n0 + n1)
        C.append(case(f"mixed_{n0}_{n1}", m0, m1, pe_bonus=60))
    # ten candidates, all within sub_diff, and a plan whose table ends at 8: the reference's floor 1 on mate 1 is what the plan leaves out
    C.append(case("n_sub_beyond_table", [dict(rs=1000 + i, dp=100 - (i > 0), mapq=30 if i == 0 else 0) for i in range(10)], [dict(rs=1300)], pe_bonus=1000, max_log_arg=8))
    # refused
    C.append(case("refuse_no_p", [dict(rs=1000), dict(rs=1010, no_p=True)], [dict(rs=1200)], refuse="p == 0"))
    c = case("refuse_p_beyond", [dict(rs=1000)], [dict(rs=1200)], refuse="p names no record")
    c["regs"][1]["p"][0] = 1 << 40                                             # (beyond any batch the case may stand in)
    C.append(c)
    C.append(case("refuse_rid", [dict(rs=1000, rid=-1)], [dict(rs=1200)], refuse="rid < 0"))
    C.append(case("refuse_rs_negative", [dict(rs=-1)], [dict(rs=1200)], refuse="rs < 0"))
    C.append(case("refuse_rs_2_30", [dict(rs=1000)], [dict(rs=1 << 30)], refuse="rs >= 2^30"))
    C.append(case("refuse_id", [dict(rs=1000), dict(rs=1010, id=0)], [dict(rs=1200)], refuse="id is not the position"))
    C.append(case("refuse_parent", [dict(rs=1000)], [dict(rs=1200), dict(rs=1300, parent=2)], refuse="parent outside the mate"))
    C.append(case("refuse_parent_negative", [dict(rs=1000, parent=-1)], [dict(rs=1200)], refuse="parent outside the mate"))
    C.append(case("refuse_one_end", [dict(rs=1000, rid=-1)], [], refuse="rid < 0, one end only"))
    return C


def flip_cases():
    """hand-derived: (case, expected (qs, qe, rev) per region of either mate behind the flip; None: the mate is not flipped)"""
    F = []
    # pe_ori 1 (FR): mate 1 is flipped.  qlen 150: [0, 100) -> [50, 150), [20, 150) -> [0, 130); rev toggles
    c = case("flip_mate1", [dict(rs=1000, qs=5, qe=140)], [dict(rs=1200, qs=0, qe=100), dict(rs=9000, qs=20, qe=150, rev=1)], pe_ori=1, flip=1)
    F.append((c, [None, [(50, 150, 1), (0, 130, 0)]]))
    # pe_ori 2 (RF): mate 0, of length 120: [5, 100) -> [20, 115)
    c = case("flip_mate0", [dict(rs=1000, qs=5, qe=100)], [dict(rs=1200)], qlens=(120, 150), pe_ori=2, flip=1)
    F.append((c, [[(20, 115, 1)], None]))
    c = case("flip_both", [dict(rs=1000, qs=5, qe=100)], [dict(rs=1200, qs=1, qe=2)], qlens=(120, 150), pe_ori=3, flip=1)
    F.append((c, [[(20, 115, 1)], [(148, 149, 1)]]))
    c = case("flip_none_ff", [dict(rs=1000, qs=5, qe=100)], [dict(rs=1200, qs=1, qe=2)], pe_ori=0, flip=1)
    F.append((c, [None, None]))
    c = case("flip_off", [dict(rs=1000, qs=5, qe=100)], [dict(rs=1200, qs=1, qe=2)], pe_ori=3, flip=0)
    F.append((c, [None, None]))
    # one end only: mm_pair returns at once, the flip still runs
    c = case("flip_one_end", [], [dict(rs=1200, qs=0, qe=100)], pe_ori=1, flip=1)
    F.append((c, [None, [(50, 150, 1)]]))
    return F


def fixture():
    """tests/golden/ref_pair.npz -> (planted: name -> dict(case, out [mate 0, mate 1] behind mm_pair, kinds), real: one dict per simulated pair with qlens, rep_len,
    gap and the lists pre / in / out as [(REG, PEXT) of mate 0, of mate 1], kinds; libm)"""
    import os
    Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pair.npz"))
    cs = {c["name"]: c for c in cases()}
    o = Z["out_off"]
    planted = {}
    for k, name in enumerate(str(x) for x in Z["names"]):
        out = [Z["regs_out"][o[2 * k + s]:o[2 * k + s + 1]].copy().view(REG).reshape(-1) for s in range(2)]
        planted[name] = dict(case=cs[name], out=out, kinds=set(str(Z["kinds"][k]).split(",")) - {""})
    real = []
    L = {t: (Z[f"real_{t}_off"], Z[f"real_{t}_regs"], Z[f"real_{t}_poff"], Z[f"real_{t}_pext"]) for t in ("pre", "in", "out")}
    for f in range(Z["real_qlens"].shape[0]):
        d = dict(qlens=tuple(int(v) for v in Z["real_qlens"][f]), rep_len=int(Z["real_rep_len"][f]), gap=int(Z["real_gap"][f]), kinds=set(str(Z["real_kinds"][f]).split(",")) - {""})
        for t, (off, regs, poff, pext) in L.items():
            d[t] = [(regs[off[2 * f + s]:off[2 * f + s + 1]].copy().view(REG).reshape(-1), pext[poff[2 * f + s]:poff[2 * f + s + 1]].copy().view(PEXT).reshape(-1)) for s in range(2)]
        real.append(d)
    return planted, real, str(Z["libm"])


def real_case(d, which="in"):
    """a simulated pair's lists `which` as a case: one pext array for both mates, the p of mate 1 moved behind mate 0's records"""
    (r0, px0), (r1, px1) = d[which]
    r1 = r1.copy()
    r1["p"][r1["p"] != 0] += np.uint64(px0.size)
    return dict(name="real", qlens=d["qlens"], opt=dict(DEFAULT), regs=[r0.copy(), r1], pext=np.concatenate([px0, px1]), gap=d["gap"], refuse=None)
