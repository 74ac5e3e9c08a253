"""The inputs of the regions-to-hits tests (mm_set_parent + mm_select_sub; csrc/chain_hits.hip), made again deterministically wherever they are needed: the fixture
tests/golden/ref_hits.npz stores only what the reference made of them.  A case is {"name", "opt" (the fields of mm2c_hit_opt_t), "regs" (REG array)}.  The regions are
built directly -- the reference does not need them in score order -- with the constant fields as mm_gen_regs leaves them (parent -1, subsc 0, n_sub 0, div -1, p 0).

The float-edge family (hit.c:165): one primary [s, s + M) and one region [0, L) per pair, so uncov_len = L - ol; ol is searched beside the real solution of
ol / min - (L - ol) / max = mask_level, and pairs are kept where the float result and the real one disagree about `>` ("f32_yes": float says greater, the real
value does not; "f32_no": the reverse).  For mask_level 0.5f the real value can equal the level (EQ_05: pairs whose float value is 0.5 too, and pairs whose float
value falls below it).  The side "f32_yes" has no pair at 0.5f: of all 92 380 pairs of lengths in [50, 30000) whose real value is exactly 1/2 none has a float value
above it, and 4 * 10^7 pairs drawn beside the level held none either -- the search below finds "f32_no" only, and that is the state of the data, not an omission.
For 0.3f the real value cannot equal the level: 0.3f is an odd number over 2^24, the
real value a fraction over lcm(min, max), and no two lengths below 2^24 have a common multiple divisible by 2^24 -- the geometry admits no "eq" pair there.
FLOAT_EDGE lists what was planted; a side on which the search finds nothing shows up there as missing (test_cpu_hits_model.py prints and checks it)."""
import numpy as np

from regs_model import REG

LDS_CLASS = 128                                                                # MM2C_HIT_LDS_REGIONS
INT_MAX = 2**31 - 1
DEFAULT = dict(mask_level=0.5, mask_len=INT_MAX, hard_mask_level=0, pri_ratio=0.8, min_diff=30, best_n=5)


def opt(**kw):
    o = dict(DEFAULT)
    o.update(kw)
    return o


def reg(qs, qe, score, cnt=10, rid=0, rs=None, re=None, rev=0, hash_=0):
    r = np.zeros(1, REG)
    rs = qs + 100000 if rs is None else rs
    re = rs + (qe - qs) if re is None else re
    r["id"], r["cnt"], r["rid"], r["score"], r["qs"], r["qe"], r["rs"], r["re"] = -7, cnt, rid, score, qs, qe, rs, re
    r["parent"], r["as"], r["mlen"], r["blen"], r["score0"] = -1, 3 * cnt, (qe - qs) // 2, qe - qs, score
    r["flags"], r["hash"], r["div"] = rev << 10, hash_, -1.0
    return r


def cat(*rs):
    out = np.concatenate(rs) if rs else np.zeros(0, REG)
    out["id"] = np.arange(out.size)                                            # as mm_gen_regs numbers them
    out["hash"] = (np.arange(out.size, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xffffffff)).astype(np.uint32)
    return out


def disjoint(n, step=100, length=50, score0=5000):
    return [reg(step * j, step * j + length, score0 - j, cnt=5 + j % 7) for j in range(n)]


def random_read(rng, n, qlen=20000):
    """regions of random extent in descending score, as a real read has them: a mix of primaries, children, identical hits and equal scores"""
    sc = np.sort(rng.integers(40, 4000, n))[::-1]
    rs = []
    for j in range(n):
        if j and rng.random() < 0.15:                                           # the same query and reference interval as an earlier region
            q = rs[int(rng.integers(0, j))]
            r = reg(int(q["qs"][0]), int(q["qe"][0]), int(sc[j]), int(rng.integers(3, 60)), int(q["rid"][0]), int(q["rs"][0]), int(q["re"][0]), int(rng.integers(0, 2)))
        else:
            ln = int(rng.integers(30, qlen // 4)) if rng.random() < 0.3 else int(rng.integers(30, 600))
            s = int(rng.integers(0, qlen - ln))
            r = reg(s, s + ln, int(sc[j]), int(rng.integers(3, 60)), int(rng.integers(0, 3)), int(rng.integers(0, 1 << 20)), None, int(rng.integers(0, 2)))
        rs.append(r)
    return cat(*rs)


EQ_05 = [("eq", 100, 100, 25), ("eq", 4004, 4004, 1001), ("eq", 900, 1800, 300), ("eq", 1400, 700, 700), ("eq", 60, 140, 21), ("eq", 54, 675, 25)]   # real value exactly 1/2: (L, M, uncov)


def float_edges(mask_level, seed, per_kind=3, tries=400000):
    """-> [(kind, L, M, s)]: kind "f32_yes" (float says > while the real value does not), "f32_no" (the reverse), "eq" (the real value equals the level)"""
    from fractions import Fraction
    rng = np.random.default_rng(seed)
    ml = np.float32(mask_level)
    L = rng.integers(50, 30000, tries); M = rng.integers(50, 30000, tries)
    mn, mx = np.minimum(L, M), np.maximum(L, M)
    ol = np.rint((float(ml) + L / mx) / (1.0 / mn + 1.0 / mx)).astype(np.int64) + rng.integers(-1, 2, tries)
    f = (ol.astype(np.float32) / mn.astype(np.float32) - (L - ol).astype(np.float32) / mx.astype(np.float32)) > ml
    near = np.abs(ol / mn - (L - ol) / mx - float(ml)) < 4e-7                   # (in double: only these can disagree)
    found = {"f32_yes": [], "f32_no": []}
    lvl = Fraction(float(ml))
    for t in np.nonzero((ol >= 1) & (ol <= mn) & near)[0]:
        v = Fraction(int(ol[t]), int(mn[t])) - Fraction(int(L[t] - ol[t]), int(mx[t]))
        kind = "f32_yes" if f[t] and v <= lvl else "f32_no" if (not f[t]) and v > lvl else None
        if kind and len(found[kind]) < per_kind:
            found[kind].append((kind, int(L[t]), int(M[t]), int(L[t] - ol[t])))     # the primary starts at L - ol and reaches to L or beyond
        if all(len(v_) == per_kind for v_ in found.values()):
            break
    return found["f32_yes"] + found["f32_no"] + (EQ_05 if float(ml) == 0.5 else [])


def edge_read(edges):
    """every pair at its own place on the query: primary [base + s, base + s + M), then the region [base, base + L)"""
    prim, kids = [], []
    for t, (_, L, M, s) in enumerate(edges):
        base = 100000 * t
        prim.append(reg(base + s, base + s + M, 9000 - t, cnt=20))
        kids.append(reg(base, base + L, 800 - t, cnt=20))
    return cat(*(prim + kids))


FLOAT_EDGE = {}
_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(20241)
    C = []
    add = lambda name, o, regs: C.append({"name": name, "opt": o, "regs": regs})
    add("empty", opt(), cat())
    add("one", opt(), cat(reg(10, 500, 300)))
    for n in (64, 65, 129):
        add(f"disjoint{n}", opt(), cat(*disjoint(n)))
    # only the 65th primary passes; then one more primary and a child of the first
    add("child_of_65th", opt(), cat(*(disjoint(65) + [reg(6400, 6450, 90, cnt=30), reg(7000, 7050, 80), reg(0, 48, 70, cnt=1)])))
    # the first overlapping primary fails (1/3 of the shorter), the second passes
    add("first_overlap_fails", opt(), cat(reg(0, 1000, 500), reg(900, 1100, 400), reg(950, 1100, 300), reg(5000, 5100, 200)))
    # both primaries pass for region 2; the first in w order takes it, not the one of higher score
    add("first_not_best", opt(), cat(reg(0, 1000, 500), reg(600, 1600, 900), reg(500, 1100, 450, cnt=30), reg(520, 1090, 440)))
    short = lambda ln: [reg(100 * j, 100 * j + ln, 3000 - j, cnt=8 + j % 5) for j in range(100)]
    add("long_over_100_primary", opt(), cat(*(short(40) + [reg(0, 10000, 2000, cnt=12)])))             # uncov 6000: 1 - 0.6 < 0.5
    add("long_over_100_child", opt(), cat(*(short(90) + [reg(0, 10000, 2950, cnt=10)])))               # uncov 1000: 1 - 0.1 > 0.5, child of the first
    # primaries that overlap each other below the level: the union is not the sum
    un = [reg(0, 1000, 900), reg(600, 1600, 800), reg(500, 1100, 790), reg(400, 1800, 780), reg(2000, 2100, 50)]
    add("union_not_sum", opt(), cat(*un))
    add("union_hard_mask_level", opt(hard_mask_level=1), cat(*un))                                      # uncov stays 0: region 3 goes to the first primary
    # mask_len decides: uncov 150 against 100 / 150 / 149
    ml = [reg(0, 1000, 900), reg(0, 1150, 850), reg(3000, 4000, 800), reg(2900, 4000, 700), reg(2850, 4000, 690)]
    for v in (100, 150, 149):
        add(f"mask_len_{v}", opt(mask_len=v), cat(*ml))
    for lvl, seed in ((0.5, 11), (0.3, 12)):
        E = float_edges(lvl, seed)
        FLOAT_EDGE[lvl] = E
        add(f"float_edge_{lvl}", opt(mask_level=lvl), edge_read(E))
        add(f"float_edge_{lvl}_keepall", opt(mask_level=lvl, pri_ratio=0.0), edge_read(E))
    # n_sub with cnt equal, above and below; subsc raised twice, then not
    ns = [reg(0, 1000, 100, cnt=20), reg(0, 900, 50, cnt=20), reg(10, 950, 70, cnt=25), reg(20, 940, 60, cnt=5), reg(2000, 2500, 40, cnt=9), reg(2000, 2400, 39, cnt=9)]
    add("n_sub_subsc", opt(), cat(*ns))
    add("n_sub_subsc_pri0", opt(pri_ratio=0.0), cat(*ns))
    # best_n reached exactly, identical hits among the candidates (they do not count)
    P = reg(0, 1000, 100, rid=1, rs=5000, re=6000)
    same = lambda sc: reg(0, 1000, sc, rid=1, rs=5000, re=6000)
    bn = [P, same(99), reg(0, 990, 98, rid=1), reg(5, 1000, 97, rid=2), same(96), reg(0, 1000, 95, rid=1, rs=5000, re=6001), reg(0, 1000, 94, rid=2, rs=5000, re=6000),
          same(93), reg(1, 1000, 92)]
    for v in (3, 4, 2):
        add(f"best_n_{v}", opt(best_n=v), cat(*bn))
    # the two branches of hit.c:263 alone, and the float product
    br = [reg(0, 1000, 100), reg(0, 990, 80), reg(0, 980, 79), reg(0, 970, 70), reg(0, 960, 69)]
    add("pri_ratio_alone", opt(min_diff=0), cat(*br))
    add("min_diff_alone", opt(min_diff=30, pri_ratio=0.99), cat(*br))
    add("min_diff_30", opt(min_diff=30), cat(*br))
    add("five_four", opt(min_diff=0), cat(reg(0, 1000, 5), reg(0, 990, 4), reg(3000, 4000, 10), reg(3000, 3990, 8), reg(3000, 3980, 7)))
    # hit.c:262: the compaction overwrites a parent's position.  0 primary, 1 dropped, 2 primary, 3 primary, 4 child of 2 -- judged against old region 3
    ow = lambda s3, r4: cat(reg(0, 800, 500), reg(0, 790, 100), reg(1000, 2000, 100), reg(1400, 2600, s3, rid=2, rs=700, re=1900), r4, reg(5000, 5100, 30))
    add("overwritten_keep_to_drop", opt(min_diff=5), ow(200, reg(1400, 2600, 90, rid=2, rs=701, re=1901)))          # 90 >= 80 against region 2, 90 < 160 against region 3
    add("overwritten_drop_to_keep", opt(min_diff=5), ow(60, reg(1400, 2600, 50, rid=2, rs=701, re=1901)))           # 50 < 80 against region 2, 50 >= 48 against region 3
    add("overwritten_identity_drop", opt(min_diff=5), ow(95, reg(1400, 2600, 90, rid=2, rs=700, re=1900)))          # identical to region 3, not to its parent
    add("overwritten_identity_keep", opt(min_diff=5), ow(95, reg(1000, 2000, 90)))                                  # identical to its parent (100000-based rs), not to region 3
    # nothing dropped: ids and parents are mm_set_parent's and sam_pri stays 0
    add("nothing_dropped", opt(), cat(reg(0, 1000, 100), reg(0, 990, 95), reg(2000, 3000, 90), reg(2000, 2990, 85)))
    add("first_dropped_only", opt(), cat(reg(0, 1000, 100), reg(0, 990, 20), reg(2000, 3000, 90), reg(2000, 2990, 85)))
    add("pri_ratio_zero", opt(pri_ratio=0.0), random_read(rng, 90))
    add("pri_ratio_negative", opt(pri_ratio=-1.0), random_read(rng, 20))
    # at the LDS class and beyond it
    for n in (30, 70, LDS_CLASS, LDS_CLASS + 1, 700):
        add(f"random{n}", opt(), random_read(rng, n))
    add(f"random{LDS_CLASS}_asm", opt(best_n=50, min_diff=38), random_read(rng, LDS_CLASS))
    add(f"random{LDS_CLASS + 1}_sr", opt(best_n=20, min_diff=42, pri_ratio=0.5), random_read(rng, LDS_CLASS + 1))
    add(f"disjoint{LDS_CLASS}", opt(), cat(*disjoint(LDS_CLASS)))
    add(f"disjoint{LDS_CLASS + 1}_child", opt(), cat(*(disjoint(LDS_CLASS + 1) + [reg(100 * LDS_CLASS, 100 * LDS_CLASS + 50, 60)])))
    add("long_over_300_beyond", opt(), cat(*([reg(100 * j, 100 * j + 90, 3000 - j, cnt=8 + j % 5) for j in range(300)] + [reg(0, 30000, 2600, cnt=10), reg(50, 29000, 100)])))
    add("random1500_hard", opt(hard_mask_level=1, mask_level=0.4), random_read(rng, 1500, qlen=60000))
    _CASES = C
    return C


def opt_key(o):
    return tuple(o[k] for k in ("mask_level", "mask_len", "hard_mask_level", "pri_ratio", "min_diff", "best_n"))


def groups(cs=None):
    """the cases grouped by equal options -> [(opt, [index into cases()])]"""
    cs = cases() if cs is None else cs
    g = {}
    for k, c in enumerate(cs):
        g.setdefault(opt_key(c["opt"]), (c["opt"], []))[1].append(k)
    return list(g.values())


def batch(cs):
    """-> (u_off int64, regs REG) of the cases one after another"""
    n = np.array([c["regs"].size for c in cs], np.int64)
    u_off = np.zeros(len(cs) + 1, np.int64)
    u_off[1:] = np.cumsum(n)
    return u_off, (np.concatenate([c["regs"] for c in cs]) if cs else np.zeros(0, REG))
