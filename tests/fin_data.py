"""Cases for the finish plan (csrc/align_finish.hip): the smallest shapes at which each step of mm_filter_regs, mm_hit_sort, mm_set_parent,
mm_select_sub, mm_set_sam_pri and mm_set_mapq on regions with r->p can go wrong, and for mm_split_reg.  cases(): one read each, dict(name, qlen, rep_len, opt,
regs REG, pext PEXT; p of a region is 0 or 1 + the index of its record in the case's pext; refuse: why the plan refuses the read, cases the reference is not run on).
split_cases(): dict(name, reg, n, split_inv, qlen, a).  tests/golden/make_ref_fin_fixtures.py runs the reference's own hit.o on them (tests/golden/ref_fin.npz)."""
import numpy as np

from fin_model import PEXT, F, split_score, INV_BIT, IS_ALT_BIT, SEG_SPLIT_BIT
from regs_model import REG

INT32_MAX = 2 ** 31 - 1
LDS_CLASS = 128
MAX_LOG_ARG = 4096                                                             # of the plans the tests make; "beyond_table" holds a primary one past it
DEFAULT = dict(min_cnt=3, min_chain_score=40, min_dp_max=80, max_clip_ratio=1.0, mask_level=0.5, mask_len=INT32_MAX, hard_mask_level=0, sub_diff=8, pri_ratio=0.8,
               min_diff=30, best_n=5, match_sc=2, is_sr=0, all_chains=0)       # map-ont (options.c)


def _hash(i):
    return (i + 1) * 2654435761 & 0xffffffff


def case(name, specs, qlen=100000, rep_len=0, refuse=None, **opt):
    """specs: one dict per region, in input order; dp: its dp_max (None: no p)"""
    o = dict(DEFAULT)
    assert not set(opt) - set(o)
    o.update(opt)
    r = np.zeros(len(specs), REG)
    px = []
    for i, s in enumerate(specs):
        s = dict(s)
        dp = s.pop("dp", 200)
        qs, qe = s.pop("qs", 1000 * i), s.pop("qe", 1000 * i + 500)
        score = s.pop("score", 200)
        v = dict(id=i, cnt=20, rid=0, score=score, qs=qs, qe=qe, rs=qs + 5000, re=qe + 5000, parent=i, subsc=0, mlen=100, blen=120, n_sub=0, score0=score, flags=0,
                 hash=_hash(i), div=0.0)
        v["as"] = 100 * i
        dp2 = s.pop("dp2", 0)
        assert not set(s) - set(v), set(s) - set(v)
        v.update(s)
        for k, x in v.items():
            r[k][i] = x
        if dp is not None:
            px.append((dp, dp, dp2, 0, 3, 0, 10 * i))
            r["p"][i] = len(px)
    return dict(name=name, qlen=qlen, rep_len=rep_len, opt=o, regs=r, pext=np.array(px, PEXT).reshape(-1), refuse=refuse)


def _many(n, ties, seed, overlap=False):
    """n regions, disjoint on the query, dp_max 100 .. 611 and random hashes; `ties` of them share one key (a split child carries its parent's hash).  overlap: every
    tenth region lies on the one before it (a secondary), with another reference start"""
    rng = np.random.default_rng(seed)
    dp = rng.integers(100, 612, n)
    hs = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    if ties:
        at = rng.choice(n, ties, replace=False)
        dp[at] = 300; hs[at] = 0x9e3779b9
    specs = []
    for i in range(n):
        s = dict(dp=int(dp[i]), hash=int(hs[i]), qs=200 * i, qe=200 * i + 150, cnt=5 + i % 9)
        if overlap and i % 10 == 9:
            s.update(qs=200 * (i - 1), qe=200 * (i - 1) + 150, rs=7, re=157)
        specs.append(s)
    return specs


def cases():
    C = []
    C.append(case("empty", []))
    C.append(case("one", [dict(dp=300)]))                                      # mapq branch hit.c:494-496
    C.append(case("two_reordered", [dict(dp=150), dict(dp=400)]))
    C.append(case("all_filtered", [dict(cnt=2), dict(mlen=39), dict(dp=79)]))
    C.append(case("flt_min_cnt", [dict(cnt=2), dict(cnt=3), dict(cnt=2, flags=1 << SEG_SPLIT_BIT)]))
    C.append(case("flt_mlen", [dict(mlen=39), dict(mlen=40)]))
    C.append(case("flt_dp_max", [dict(dp=79), dict(dp=80)]))
    C.append(case("flt_clip", [dict(qs=101, qe=899), dict(qs=101, qe=900), dict(qs=100, qe=899)], qlen=1000, max_clip_ratio=0.1))   # both ends; one end each
    C.append(case("clip_float", [dict(qs=7, qe=12), dict(qs=0, qe=20, dp=90)], qlen=20, max_clip_ratio=0.35))
    C.append(case("tie_child", [dict(dp=200, hash=77, qs=0, qe=500), dict(dp=200, hash=77, qs=600, qe=900, id=-1, parent=-2), dict(dp=100, qs=1000, qe=1500)]))
    for n in (64, 65):
        C.append(case(f"n{n}_distinct", _many(n, 0, n)))
        C.append(case(f"n{n}_ties", _many(n, 10, 100 + n)))
    C.append(case("n128_ties", _many(128, 10, 228)))
    C.append(case("n129_ties", _many(129, 10, 229, overlap=True)))
    C.append(case("n300_ties", _many(300, 10, 300, overlap=True)))
    C.append(case("mixed_p", [dict(dp=300), dict(dp=None, score=250)], refuse="mixed"))
    C.append(case("all_no_p", [dict(dp=None, score=150), dict(dp=None, score=250), dict(dp=None, score=100, qs=1100, qe=1400)]))   # score as key; mapq branch :498
    # one primary, three children on it with other reference starts: dp_max2 is the maximum, in the order 100, 250, 180
    C.append(case("dp_max2_of_three", [dict(dp=300, qs=0, qe=1000), dict(dp=250, qs=0, qe=900, rs=9000, re=9900, cnt=3), dict(dp=180, qs=100, qe=1000, rs=3, re=903, cnt=3),
                                       dict(dp=100, qs=50, qe=950, rs=77, re=977, cnt=3)]))
    # two children of one primary, each counted (cnt not below the primary's): the second meets what the first left -- n_sub 1 -> 2, subsc stays 90, dp_max2 stays 250;
    # an update computed from the primary as it stood before either child would leave n_sub 1, or the second child's 60 and 180
    C.append(case("later_sees_update", [dict(dp=300, qs=0, qe=1000), dict(dp=250, qs=0, qe=900, rs=9000, re=9900, score=90), dict(dp=180, qs=100, qe=1000, rs=3, re=903, score=60)],
                  pri_ratio=0.0))
    # identical after DP: same rid, rs, re, and the overlap is the shorter one; dp_max within sub_diff, cnt below: neither dp_max2 nor n_sub; mm_select_sub drops it
    # as identical, and the p of the region behind it follows the survivors
    C.append(case("identical_after_dp", [dict(dp=300, qs=0, qe=1000), dict(dp=296, qs=0, qe=1000, rs=5000, re=6000, cnt=3), dict(dp=150, qs=2000, qe=2500)]))
    C.append(case("identical_but_rs", [dict(dp=300, qs=0, qe=1000), dict(dp=296, qs=0, qe=1000, rs=5001, re=6000, cnt=3), dict(dp=150, qs=2000, qe=2500)]))
    C.append(case("sub_diff_eq", [dict(dp=300, qs=0, qe=1000), dict(dp=292, qs=0, qe=900, rs=1, re=901, cnt=3)]))
    C.append(case("sub_diff_plus1", [dict(dp=300, qs=0, qe=1000), dict(dp=291, qs=0, qe=900, rs=1, re=901, cnt=3)]))
    C.append(case("best_n_0", [dict(dp=300, qs=0, qe=1000), dict(dp=290, qs=0, qe=900, rs=1, re=901)], best_n=0))
    C.append(case("pri_ratio_0", [dict(dp=300, qs=0, qe=1000), dict(dp=100, qs=0, qe=900, rs=1, re=901, score=10)], pri_ratio=0.0))
    C.append(case("dropped_by_ratio", [dict(dp=300, qs=0, qe=1000), dict(dp=100, qs=0, qe=900, rs=1, re=901, score=10), dict(dp=90, qs=2000, qe=2600)]))
    C.append(case("all_chains", [dict(dp=150, id=5, parent=5), dict(dp=300, qs=0, qe=400, id=-1, parent=-2), dict(dp=200, id=7, parent=5)], all_chains=1))
    C.append(case("sam_pri_nothing_dropped", [dict(dp=150, flags=1 << 12), dict(dp=300)]))
    # mapq: hit.c:484-491 with mapq_alt below (dp_max - dp_max2 small) and above, with and without is_sr
    for sr in (0, 1):
        C.append(case(f"alt_below_sr{sr}", [dict(dp=300, qs=0, qe=1000, score0=400), dict(dp=295, qs=0, qe=900, rs=1, re=901, cnt=3, score=20)], is_sr=sr))
        C.append(case(f"alt_above_sr{sr}", [dict(dp=300, qs=0, qe=1000, score0=400, cnt=4), dict(dp=90, qs=0, qe=900, rs=1, re=901, cnt=3, score=150)], is_sr=sr))
    # x = 109 * 273 / 300 / 148: 1.0f - x * x with the product rounded gives mapq 46, a fused multiply-add 45
    C.append(case("xx_not_fused", [dict(dp=300, qs=0, qe=1000, cnt=5, score0=148), dict(dp=109, qs=0, qe=900, rs=1, re=901, cnt=3, score=273)]))
    C.append(case("floor_504", [dict(dp=300, cnt=3, score=50)], rep_len=100000))
    C.append(case("cap_60", [dict(dp=4000, mlen=120)]))
    C.append(case("n_sub_none", [dict(dp=300, n_sub=0, cnt=3)]))
    C.append(case("n_sub_penalty", [dict(dp=300, n_sub=3, cnt=3)]))            # (int)(4.343f * logf(4) + .499f) = 6 less
    C.append(case("beyond_table", [dict(dp=MAX_LOG_ARG + 1), dict(dp=300)]))
    C.append(case("inv_region", [dict(dp=300), dict(dp=200, flags=1 << INV_BIT)], refuse="inv"))
    C.append(case("alt_region", [dict(dp=300, flags=1 << IS_ALT_BIT)], refuse="is_alt"))
    names = [c["name"] for c in C]
    assert len(set(names)) == len(names)
    return C


def anchors(n, rev, rid=3, x0=1000, y0=50, span=15, step=(40, 37)):
    """n chain anchors on one strand: x = rev << 63 | rid << 32 | pos, y = span << 32 | qpos"""
    a = np.zeros((n, 2), np.uint64)
    for i in range(n):
        a[i, 0] = (rev << 63) | (rid << 32) | (x0 + step[0] * i + (i * i) % 7)
        a[i, 1] = (span << 32) | (y0 + step[1] * i + (i * 3) % 5)
    return a


def float_double_score():
    """(score, cnt, n) on which (int32_t)(score * ((float)cnt2 / cnt) + .499) differs between a float and a double add"""
    for cnt in range(6, 16):                                                   # a float near 2^20 has no room for .499 behind a half
        for n in range(3, cnt - 2):
            for score in range((1 << 21) + 1, (1 << 21) + 40):
                if split_score(score, cnt - n, cnt) != split_score(score, cnt - n, cnt, "float"):
                    return score, cnt, n
    raise AssertionError("no such score")


def split_cases():
    S = []
    sc, cnt, n = float_double_score()
    for name, rev, parent, id_, split_inv, score, c, k in (("fwd_primary", 0, 4, 4, 0, 731, 12, 5), ("rev_secondary", 1, 2, 4, 0, 512, 9, 3), ("fwd_split_inv", 0, 0, 0, 1, 90, 6, 3),
                                                           ("float_double", 1, 1, 1, 0, sc, cnt, n)):
        a = anchors(c + 4, rev)
        r = np.zeros((), REG)
        r["id"], r["parent"], r["cnt"], r["score"], r["score0"], r["as"], r["rid"] = id_, parent, c, score, score + 5, 2, 3
        r["hash"], r["div"], r["subsc"], r["n_sub"], r["mlen"], r["blen"] = 0xabcdef01, 0.03125, 17, 2, 111, 222
        r["flags"] = (rev << 10) | (1 << 12) | (1 << 24) | (2 << 8 if name == "rev_secondary" else 0)      # sam_pri and split_inv set: the child clears them
        r["qs"], r["qe"], r["rs"], r["re"], r["p"] = 1, 2, 3, 4, 0
        S.append(dict(name=name, reg=r, n=k, split_inv=split_inv, qlen=5000, a=a))
    return S


REAL_OPT = {"ont": dict(DEFAULT),                                              # map-ont, asm20 and sr of options.c, as params.fin_opts has them
            "asm20": dict(DEFAULT, min_dp_max=200, best_n=50, sub_diff=6, min_diff=38, match_sc=1),
            "sr": dict(DEFAULT, min_cnt=2, min_chain_score=25, min_dp_max=40, pri_ratio=0.5, best_n=20, sub_diff=12, min_diff=42, is_sr=1)}
_REAL = {}


def real_reads(name):
    """The reads of tests/cig_data.ref_batches()[name] as mm_align_skeleton holds them behind its loop, rebuilt from the reference's own record of mm_align1
    (tests/golden/ref_cig.npz): per read the regions of the recorded rounds, every child directly behind its parent (mm_insert_reg; NAME_c1_parent / NAME_c2_parent give
    the order), each as mm_align1 left it -- hd's rs, re, qs, qe, blen, mlen and r->p, and for a split region cnt, score and split as mm_split_reg left them, the child
    made from the chain-level region by cig_ref.split_reg.  -> cases in the format of cases(), one per read, with `where`: (round, index in the round) of every region."""
    if name in _REAL:
        return _REAL[name]
    import cig_ref
    fx = cig_ref.fixture()
    o, u_off, regs, b_off, b, read_off, fwd, names = cig_ref.inputs(name, 0)
    hd = [fx[cig_ref.prefix(name, lv) + "hd"] for lv in range(3)]
    child = [{int(p): k for k, p in enumerate(fx[cig_ref.prefix(name, lv + 1) + "parent"])} for lv in range(2)] + [{}]
    out = []
    for rd in range(len(u_off) - 1):
        a = np.asarray(b, np.uint64).reshape(-1, 2)[int(b_off[rd]):int(b_off[rd + 1])]
        qlen = int(read_off[rd + 1] - read_off[rd])
        lst, px, where = [], [], []

        def emit(lv, g, R):
            h = hd[lv][g]
            O = np.array(R, REG).reshape(()).copy()
            if h[12] > 0:                                                      # hit.c:119-122 on the parent
                O["cnt"] = int(R["cnt"]) - int(h[12]); O["score"] = int(R["score"]) - int(h[24]); O["flags"] = int(R["flags"]) | 1 << 8
            assert int(O["flags"]) >> 8 & 3 == int(h[22]), (name, lv, g)
            O["rs"], O["re"], O["qs"], O["qe"], O["p"] = h[1], h[2], h[3], h[4], 0
            if h[5]:
                O["blen"], O["mlen"] = h[8], h[9]
                px.append((h[6], h[7], 0, h[10], h[11], 0, 0))
                O["p"] = len(px)
            lst.append(O); where.append((lv, g))
            if h[12] > 0:
                assert g in child[lv], (name, lv, g, "a split whose child the record does not hold")
                emit(lv + 1, child[lv][g], cig_ref.split_reg(R, int(h[13]) - int(R["as"]), int(h[14]), qlen, a))
        for g in range(int(u_off[rd]), int(u_off[rd + 1])):
            emit(0, g, regs[g])
        out.append(dict(name=f"{name}_read{rd}", qlen=qlen, rep_len=0, opt=dict(REAL_OPT[name]), regs=np.array(lst, REG).reshape(-1), pext=np.array(px, PEXT).reshape(-1),
                        refuse=None, where=where))
    _REAL[name] = out
    return out


def real_cases():
    return [c for name in ("ont", "asm20", "sr") for c in real_reads(name)]
