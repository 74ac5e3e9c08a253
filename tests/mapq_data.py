"""The cases of the hits-to-mapping-quality tests (mm_join_long hit.c:295-371, mm_set_mapq hit.c:463-508; csrc/chain_mapq.hip), made again deterministically wherever
they are needed.  A case is {"name", "hash", "qlen", "u", "a", "hit" (mm2c_hit_opt_t), "mapq" (mm2c_mapq_opt_t), "rep_len"}: chains with their anchors, so that regions
and anchors agree; tests/golden/ref_mapq.npz holds what the reference's own hit.o makes of them (tests/golden/make_ref_mapq_fixtures.py): the hits in front of
mm_join_long (the plan's input), the final regions and the final a[].

A read is a list of chains in the order they lie in a[].  Read(...).chain(score, ref_len, q_len, n, gap=(gx, gq)) puts a chain of n anchors whose region is ref_len by
q_len long, its first anchor gx / gq behind the last anchor of the chain before it; at=(x, y) places it freely instead (a secondary over an earlier chain's query
interval).  The defaults (options.c:38-41: max_join_long 20000, max_join_short 2000, min_join_flank_sc 1000, min_join_flank_ratio 0.5) give
sc_thres = (int)(0.05f * max_gap + .499) and min_flank_len = max_gap / 2.

sc_thres, float against exact (SC_EDGE): under the default options no max_gap <= 20000 exists at which (int)(fl(fl(1000/20000) * max_gap) + .499) differs from the
exact (int)(max_gap / 20 + .499), or at which adding .499f in float differs from adding .499 in double -- all 20001 values were tried (sc_edges() below, and
test_cpu_mapq_model.py repeats it).  Other options have such gaps: the search below walks min_join_flank_sc over a few odd values and keeps, for each kind, the
first max_gap found; the cases "sc_exact_*" (float product and exact product on different sides of an integer) and "sc_f499_*" (the float add rounds up to the next
integer, the double add does not) put r0's score at the larger of the two thresholds minus one and r1's above both, so that exactly one of the two
computations joins.

One ulp of logf (ULP_EDGE): scores and rep_len at which (int)(pen_cm * 40 * (1 - x) * L) changes when L moves by one ulp, found with L = (float)log((double)score),
which does not depend on the host's libm; a dozen of them are single-chain reads "ulp_<score>_<rep_len>"."""
import numpy as np

from hits_data import DEFAULT as HIT_DEFAULT

LDS_CLASS = 128                                                                # MM2C_HIT_LDS_REGIONS: the tables of mapq_join are in LDS up to here
MAPQ_DEFAULT = dict(do_join=1, max_join_long=20000, max_join_short=2000, min_join_flank_sc=1000, min_join_flank_ratio=0.5, min_cnt=3, min_chain_score=40)
SPAN = 15
QLEN = 4000000
SMALL_TABLE = 4096                                                             # the max_log_arg of the plan the table-range cases run on


def mopt(**kw):
    o = dict(MAPQ_DEFAULT)
    o.update(kw)
    return o


def hopt(**kw):
    o = dict(HIT_DEFAULT)
    o.update(kw)
    return o


class Read:
    def __init__(self, name, rid=0, rev=0, x=50000, y=300, hit=None, mapq=None, rep_len=0, qlen=QLEN):
        self.name, self.rid, self.rev, self.x, self.y = name, rid, rev, x, y
        self.hit, self.mapq, self.rep_len, self.qlen = hit or hopt(), mapq or mopt(), rep_len, qlen
        self.chains = []

    def chain(self, score, ref_len=12000, q_len=12000, n=5, gap=(500, 500), at=None, rid=None, rev=None, span=SPAN):
        rid = self.rid if rid is None else rid
        rev = self.rev if rev is None else rev
        x0, y0 = (self.x + gap[0], self.y + gap[1]) if at is None else at
        i = np.arange(n, dtype=np.int64)
        xs = x0 + (ref_len - span) * i // max(n - 1, 1)
        ys = y0 + (q_len - span) * i // max(n - 1, 1)
        a = np.zeros((n, 2), np.uint64)
        a[:, 0] = (np.uint64(rev) << np.uint64(63)) | (np.uint64(rid) << np.uint64(32)) | xs.astype(np.uint64)
        a[:, 1] = (np.uint64(span) << np.uint64(32)) | ys.astype(np.uint64)
        self.chains.append((int(score), a))
        if at is None:
            self.x, self.y = int(xs[-1]), int(ys[-1])
        return self

    def case(self):
        u = np.array([(s << 32) | a.shape[0] for s, a in self.chains], np.uint64)
        a = np.concatenate([a for _, a in self.chains]) if self.chains else np.zeros((0, 2), np.uint64)
        h = (sum(ord(c) * 31 ** k for k, c in enumerate(self.name)) * 2654435761) & 0xffffffff
        return {"name": self.name, "hash": h, "qlen": self.qlen, "u": u, "a": np.ascontiguousarray(a), "hit": self.hit, "mapq": self.mapq, "rep_len": self.rep_len}


def sc_thres_variants(fsc, mjl, max_gap):
    """(reference, .499f added in float, exact) for arrays of max_gap"""
    pr = (np.float32(fsc) / np.float32(mjl)) * max_gap.astype(np.float32)
    ref = (pr.astype(np.float64) + 0.499).astype(np.int64)
    f32 = (pr + np.float32(0.499)).astype(np.int64)
    exact = (int(fsc) * max_gap.astype(np.int64) * 1000 + 499 * int(mjl)) // (1000 * int(mjl))
    return ref, f32, exact


def sc_edges():
    """-> {"default": (n float-add edges, n exact edges) under the default options, "exact": (fsc, mjl, gap) or None, "f499": (fsc, mjl, gap) or None}"""
    g = np.arange(1, 20001)
    ref, f32, exact = sc_thres_variants(1000, 20000, g)
    out = {"default": (int((ref != f32).sum()), int((ref != exact).sum())), "exact": None, "f499": None}
    for fsc in (1001, 33333, 700001, 1999999, 2999999):
        ref, f32, exact = sc_thres_variants(fsc, 20000, g)
        keep = ref < (1 << 21)                                                 # scores stay below the default table
        for kind, other in (("exact", exact), ("f499", f32)):
            at = np.nonzero((ref != other) & keep)[0]
            if out[kind] is None and at.size:
                out[kind] = (fsc, 20000, int(g[at[0]]))
    return out


def ulp_edges(want=12):
    """-> [(score, rep_len)]: one ulp of L = logf(score) changes (int)(uniq_ratio * 40 * (1 - 40f / score) * L) for a lone primary of more than 10 anchors
    (pen_cm = pen_s1 = uniq_ratio = score / (score + rep_len), subsc at min_chain_score, n_sub 0).  About one input in 10^5 is such an edge: 10^7 are tried."""
    s = np.arange(101, 160000)
    sf = s.astype(np.float32)
    L = np.log(s.astype(np.float64)).astype(np.float32)
    lo, hi = np.nextafter(L, np.float32(0)), np.nextafter(L, np.float32(np.inf))
    one_x = np.float32(1) - np.float32(40) / sf
    out = []
    for k in range(3, 70):
        rep = s * k + 7 * k
        base = (sf / (s + rep).astype(np.float32)) * np.float32(40) * one_x
        q = [(base * v).astype(np.int64) for v in (lo, L, hi)]
        for t in np.nonzero(((q[0] != q[1]) | (q[2] != q[1])) & (q[1] < 60) & (q[0] > 0))[0]:
            out.append((int(s[t]), int(rep[t])))
    out.sort()
    step = max(len(out) // want, 1)
    return out[::step][:want]


SC_EDGE = {}
ULP_EDGE = []
_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    C = []
    add = lambda r: C.append(r.case())
    BIG = 12000

    def pair(name, gx=500, gq=500, s0=3000, s1=2900, l0=(BIG, BIG), l1=(BIG, BIG), rid1=None, rev=0, rev1=None, mapq=None, hit=None, n=5):
        r = Read(name, rev=rev, mapq=mapq, hit=hit)
        r.chain(s0, l0[0], l0[1], n).chain(s1, l1[0], l1[1], n, gap=(gx, gq), rid=rid1, rev=rev1)
        add(r)

    # ---- n = 0, 1, 2 ----
    add(Read("n0"))
    add(Read("n1").chain(500, 600, 600, 6))
    # a lone hit whose as is not 0: the chain before it is a secondary that mm_select_sub dropped (n < 2: no squeeze, as stays)
    add(Read("n1_as_nonzero").chain(100, 900, 900, 4, at=(900000, 1000), rid=3).chain(3000, 1000, 1000, 7, at=(60000, 1000)))
    pair("n2_no_join", gx=30000, gq=30000)
    pair("n2_join")
    pair("n2_join_off", mapq=mopt(do_join=0))
    # do_join = 0 with a dropped chain in front: no squeeze, the as stay
    add(Read("no_join_no_squeeze", mapq=mopt(do_join=0)).chain(100, 900, 900, 4, at=(900000, 400), rid=3).chain(3000).chain(2900))
    # ---- adjacency in squeezed coordinates ----
    # A, D, B: D is a secondary of A that mm_select_sub drops: A and B become adjacent and join
    add(Read("adjacent_by_drop").chain(3000).chain(100, 900, 900, 4, at=(900000, 1000), rid=3).chain(2900))
    # A, S, B: S is a secondary of A that stays: A and B are candidates next to each other but not adjacent
    add(Read("adjacency_broken_by_secondary").chain(3000).chain(2800, 11000, 11000, 6, at=(900000, 600), rid=3).chain(2900))
    # ---- the refusals of hit.c:336-348, both sides ----
    pair("rid_differs", rid1=1)
    pair("strand_differs", rev1=1)
    pair("x_equal", gx=0); pair("x_one_more", gx=1)
    pair("y_equal", gq=0); pair("y_one_more", gq=1)
    pair("max_gap_at", gx=20000, gq=1000); pair("max_gap_above", gx=20001, gq=1000)
    pair("max_gap_q_at", gx=1000, gq=20000); pair("max_gap_q_above", gx=1000, gq=20001)
    pair("min_gap_at", gx=2000, gq=5000); pair("min_gap_above", gx=2001, gq=5000)
    pair("min_gap_q_at", gx=5000, gq=2000); pair("min_gap_q_above", gx=5000, gq=2001)
    g = 10000                                                                   # sc_thres 500, min_flank_len 5000
    pair("score0_at", gx=g, gq=1500, s0=500); pair("score0_below", gx=g, gq=1500, s0=499)
    pair("score1_at", gx=g, gq=1500, s1=500); pair("score1_below", gx=g, gq=1500, s1=499)
    for k, which in enumerate(("r0_ref", "r0_query", "r1_ref", "r1_query")):
        for d, word in ((0, "at"), (-1, "below")):
            ln = [[BIG, BIG], [BIG, BIG]]
            ln[k // 2][k % 2] = 5000 + d
            pair(f"flank_{which}_{word}", gx=g, gq=1500, l0=tuple(ln[0]), l1=tuple(ln[1]))
    # ---- sc_thres: float product against exact product, float add against double add ----
    SC_EDGE.update(sc_edges())
    for kind in ("exact", "f499"):
        if SC_EDGE[kind]:
            fsc, mjl, gap = SC_EDGE[kind]
            ref, f32, exact = (int(v[0]) for v in sc_thres_variants(fsc, mjl, np.array([gap])))
            sc = max(ref, exact if kind == "exact" else f32) - 1
            o = mopt(min_join_flank_sc=fsc, max_join_long=mjl, min_join_flank_ratio=0.01)
            pair(f"sc_{kind}_{fsc}_{gap}", gx=gap, gq=min(gap, 1500), s0=sc, s1=sc + 5, mapq=o)
    # ---- the mlen pair term: span, tl, ql, and tl == ql ----
    for gx, gq in ((100, 200), (10, 200), (200, 10), (10, 10), (15, 15), (16, 16)):
        pair(f"mlen_pair_{gx}_{gq}", gx=gx, gq=gq)
    # ---- the reverse strand ----
    pair("rev_join", rev=1)
    pair("rev_no_join", rev=1, gx=30000, gq=300)
    add(Read("rev_adjacent_by_drop", rev=1).chain(3000).chain(100, 900, 900, 4, at=(900000, QLEN - 1500), rid=3, rev=0).chain(2900))
    # ---- three chains: A joins B only because B has absorbed C (B alone: score 300 < 500, 1600 long < 5000) ----
    add(Read("grown_r1").chain(600).chain(300, 1600, 1600, 4, gap=(10000, 1500)).chain(310, 1600, 1600, 4, gap=(2000, 2000)))
    add(Read("grown_r1_not_enough").chain(600).chain(300, 1600, 1600, 4, gap=(10000, 1500)).chain(190, 1600, 1600, 4, gap=(2000, 2000)))
    add(Read("grown_r1_rev", rev=1).chain(600).chain(300, 1600, 1600, 4, gap=(10000, 1500)).chain(310, 1600, 1600, 4, gap=(2000, 2000)))
    # ---- the hierarchy fix (hit.c:360-367): four chains joined back to front and a secondary S of the fourth ----
    # fourth outranks third: S ends with the dropped second as its parent (UNSET after the sync); third outranks fourth: S reaches the kept first
    for name, s3, s4 in (("hier_fourth_outranks_third", 2000, 2500), ("hier_third_outranks_fourth", 2500, 2000)):
        r = Read(name).chain(5000, 3000, 3000).chain(4000, 3000, 3000).chain(s3, 3000, 3000).chain(s4, 3000, 3000)
        y4 = r.y - 3000 + SPAN
        r.chain(int(s4 * 0.9), 2900, 2900, 6, at=(700000, y4 + 50), rid=2)
        add(r)
    # ---- filtering (hit.c:368) only behind a join: a chain below min_cnt stays in a read without a join ----
    add(Read("min_cnt_no_join").chain(3000).chain(900, 600, 600, 2, gap=(30000, 900)).chain(800, 600, 600, 3, gap=(30000, 900)))
    add(Read("min_cnt_with_join").chain(3000).chain(2900).chain(900, 600, 600, 2, gap=(30000, 900)).chain(800, 600, 600, 3, gap=(30000, 900)))
    add(Read("min_cnt_5_with_join", mapq=mopt(min_cnt=5)).chain(3000, n=3).chain(2900, n=2).chain(900, 600, 600, 4, gap=(30000, 900)).chain(800, 600, 600, 5, gap=(30000, 900)))
    # ---- many hits: the LDS class and the candidate rounds ----
    rng = np.random.default_rng(20261020)

    def many(name, n_pri, n_kept_sec, n_drop_sec):
        r = Read(name)
        sec = {int(v): "keep" for v in rng.choice(n_pri, n_kept_sec, replace=False)}
        for v in rng.choice([v for v in range(n_pri) if v not in sec], n_drop_sec, replace=False):
            sec[int(v)] = "drop"
        scores = rng.permutation(np.arange(400, 400 + 7 * n_pri, 7))
        for k in range(n_pri):
            gap = [(400, 400), (400, 400), (30000, 400), (400, 3000), (700, 900)][int(rng.integers(0, 5))]
            r.chain(int(scores[k]), 600, 600, int(rng.integers(3, 6)), gap=gap, rid=int(rng.integers(0, 4) == 0))
            if k in sec:
                f = 0.93 if sec[k] == "keep" else 0.3
                r.chain(int(scores[k] * f), 590, 590, 4, at=(3000000 + 1000 * k, r.y - 600 + SPAN + 5), rid=2)
        add(r)
    many("cand64", 64, 2, 3)
    many("cand65", 65, 2, 3)
    many(f"hits{LDS_CLASS}", LDS_CLASS - 3, 3, 6)
    many(f"hits{LDS_CLASS + 1}", LDS_CLASS - 2, 3, 6)
    many("hits300", 297, 3, 20)
    # all of one read's chains joined into one, 70 of them
    r = Read("cascade70")
    for k in range(70):
        r.chain(4000 - 13 * k, 600, 600, 3, gap=(400, 400))
    add(r)
    # ---- mapping quality ----
    for sc in (100, 101):
        for cnt in (10, 11):
            add(Read(f"mapq_score{sc}_cnt{cnt}", rep_len=9 * sc * (cnt - 10)).chain(sc, 600, 600, cnt))             # cnt 10: capped; cnt 11: uniq_ratio 0.1 decides
    for sub in (39, 40, 41):                                                    # subsc below, at and above min_chain_score; uniq_ratio 0.1 keeps the result below the cap
        add(Read(f"mapq_subsc{sub}", rep_len=900).chain(100, 2000, 2000, 8).chain(sub, 1900, 1900, 5, at=(800000, 850), rid=1))
    add(Read("mapq_subsc900").chain(1000, 2000, 2000, 8).chain(900, 1900, 1900, 5, at=(800000, 850), rid=1))
    add(Read("mapq_subsc_above_score0", mapq=mopt(min_chain_score=5000)).chain(1000, 2000, 2000, 8))
    add(Read("mapq_subsc_equals_score0").chain(1000, 2000, 2000, 8).chain(1000, 1900, 1900, 5, at=(800000, 850), rid=1))
    add(Read("mapq_cap_60").chain(5000, 9000, 9000, 50))
    for n_sub in (1, 63):
        r = Read(f"mapq_n_sub{n_sub}", hit=hopt(best_n=3)).chain(9000, 3000, 3000, 6)
        for k in range(n_sub):
            r.chain(8000 - k, 2900 - k, 2900 - k, 6 + k % 2, at=(500000 + 5000 * k, 850), rid=1 + k % 3)
        add(r)
    add(Read("mapq_n_sub_smaller_cnt").chain(9000, 3000, 3000, 6).chain(8000, 2900, 2900, 5, at=(500000, 850), rid=1))   # cnt below the primary's: n_sub stays 0
    for rep in (0, 700, 100000):
        add(Read(f"mapq_rep_len{rep}", rep_len=rep).chain(300, 900, 900, 7).chain(250, 900, 900, 12, gap=(40000, 400)))
    add(Read("mapq_several_primaries", rep_len=55).chain(90, 700, 700, 4).chain(150, 700, 700, 9, gap=(40000, 300)).chain(3000, 5000, 5000, 30, gap=(40000, 300), rid=1)
        .chain(101, 700, 700, 11, gap=(90, 300), rev=1))
    add(Read("mapq_after_join_score0", rep_len=10).chain(120, BIG, BIG, 6).chain(110, BIG, BIG, 4).chain(100, 11000, 11000, 5, at=(800000, 400), rid=1))
    ULP_EDGE[:] = ulp_edges()
    for sc, rep in ULP_EDGE:
        add(Read(f"ulp_{sc}_{rep}", rep_len=rep).chain(sc, 600, 600, 12))
    # ---- the table's range on a plan with max_log_arg = SMALL_TABLE ----
    add(Read(f"table_score{SMALL_TABLE}").chain(SMALL_TABLE, 600, 600, 4))
    add(Read(f"table_score{SMALL_TABLE + 1}").chain(SMALL_TABLE + 1, 600, 600, 4).chain(500, 600, 600, 4, gap=(40000, 300)))
    _CASES = C
    return C


def opt_key(c):
    return tuple(c["mapq"][k] for k in ("do_join", "max_join_long", "max_join_short", "min_join_flank_sc", "min_join_flank_ratio", "min_cnt", "min_chain_score"))


def groups(cs=None):
    """the cases grouped by equal mapq options -> [(opt, [index into cases()])]"""
    cs = cases() if cs is None else cs
    g = {}
    for k, c in enumerate(cs):
        g.setdefault(opt_key(c), (c["mapq"], []))[1].append(k)
    return list(g.values())
