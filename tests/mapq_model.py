"""NumPy / Python restatement of mm_join_long (hit.c:315-371, with mm_squeeze_a hit.c:295-313, mm_filter_regs hit.c:274-293 and mm_sync_regs hit.c:231-253) and
mm_set_mapq (hit.c:463-508) on REG arrays whose p, inv and is_alt are 0, for reads mapped without CIGAR.  The logarithm is the host's own logf, called through
ctypes: the function the reference's hit.o calls on this machine.  If this model stops reproducing tests/golden/ref_mapq.npz on the "ulp_*" cases only, the
machine's libm is not the fixture's (its version string is in the fixture).

A join is made WITHOUT a walk over the anchors (what csrc/chain_mapq.hip relies on): cnt and score add, rs / re and qs / qe come from the two regions by strand,
and mlen / blen from the two regions and the one junction pair of anchors, in wrapping int.  Equality with the fixture shows these identities.

The keyword variants restate a step the "natural" way; the tests use them to show that the planted cases tell the difference:
  fp499="float"        sc_thres adds .499f in float instead of .499 in double
  hier="parallel"      the hierarchy fix reads every regs[parent].parent as it stood before the fix
  filter_always=True   mm_filter_regs / mm_sync_regs also when nothing was joined
  x_from="score"       mm_set_mapq's x = subsc / score instead of subsc / score0
  adj="unsqueezed"     the adjacency test r0->as + r0->cnt != r1->as on the as in front of mm_squeeze_a
  log="np"             np.log in double in place of logf (log may also be a function of the integer argument)"""
import ctypes
import ctypes.util

import numpy as np

from hits_model import SAM_PRI_BIT
from regs_model import REG, M64, s32

MM_SEED_LONG_JOIN = 1 << 40                                                    # mmpriv.h:17
F = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(v):
    """the host's logf((float)v)"""
    return F(_libm.logf(float(F(v))))


def squeeze(r, a):
    """mm_squeeze_a: -> (the new a[] prefix, its length); r["as"] is renumbered in place"""
    order = sorted(range(r.size), key=lambda i: (int(r["as"][i]) << 32) | i)
    out, as_ = [], 0
    for i in order:
        out.append(a[int(r["as"][i]):int(r["as"][i]) + int(r["cnt"][i])])
        r["as"][i] = as_
        as_ += int(r["cnt"][i])
    return (np.concatenate(out) if out else np.zeros((0, 2), np.uint64)), as_


def sync_regs(r, n_old):
    """mm_sync_regs + mm_set_sam_pri (hit.c:220-253) behind the filter.  tmp[] covers every id in front of the filter (n_old), so a parent that was dropped
    reads -1 wherever its id lies; the reference sizes tmp[] by the largest id that is left and reads beyond it for a dropped parent above that"""
    tmp = np.full(n_old, -1, np.int64)
    for i in range(r.size):
        tmp[r["id"][i]] = i
    n_pri = 0
    for i in range(r.size):
        p = int(r["parent"][i])
        r["id"][i] = i
        r["parent"][i] = i if p == -2 else tmp[p] if p >= 0 and tmp[p] >= 0 else -1
        r["flags"][i] &= ~np.uint32(1 << SAM_PRI_BIT)
        if r["parent"][i] == i:
            n_pri += 1
            if n_pri == 1:
                r["flags"][i] |= np.uint32(1 << SAM_PRI_BIT)


def join_long(regs, a, qlen, o, fp499="double", hier="sequential", filter_always=False, adj="squeezed"):
    """-> (regs behind mm_join_long, a[] as the reference leaves its first n_b_out entries, n joined)"""
    r = regs.copy()
    a = np.asarray(a, np.uint64).reshape(-1, 2).copy()
    n = r.size
    if n < 2:
        return r, a, 0
    as_old = r["as"].copy()
    a, _ = squeeze(r, a)
    as_adj = as_old if adj == "unsqueezed" else r["as"]
    aux = sorted(((int(r["as"][i]) << 32) | i) for i in range(n) if r["parent"][i] == i or r["parent"][i] < 0)
    aux = [v & 0xffffffff for v in aux]
    n_drop = 0
    for i in range(len(aux) - 1, 0, -1):
        i0, i1 = aux[i - 1], aux[i]
        r0, r1 = r[i0], r[i1]
        if int(as_adj[i0]) + int(r0["cnt"]) != int(as_adj[i1]):
            continue
        rev0, rev1 = (int(r0["flags"]) >> 10) & 1, (int(r1["flags"]) >> 10) & 1
        if r0["rid"] != r1["rid"] or rev0 != rev1:
            continue
        x0, y0 = (int(v) for v in a[int(r0["as"]) + int(r0["cnt"]) - 1])
        x1, y1 = (int(v) for v in a[int(r1["as"])])
        if x1 <= x0 or s32(y1) <= s32(y0):
            continue
        d = s32(s32(y1) - s32(y0))
        max_gap = d if ((x0 + d) & M64) > x1 else s32(x1 - x0)                 # hit.c:340-342: uint64 + int, compared and subtracted unsigned
        min_gap = d if ((x0 + d) & M64) < x1 else s32(x1 - x0)
        if max_gap > o["max_join_long"] or min_gap > o["max_join_short"]:
            continue
        pr = F(o["min_join_flank_sc"]) / F(o["max_join_long"]) * F(max_gap)    # float quotient, float product ...
        sc_thres = int(np.float64(pr) + 0.499) if fp499 == "double" else int(F(pr + F(0.499)))   # ... then a double add
        if r0["score"] < sc_thres or r1["score"] < sc_thres:
            continue
        min_flank_len = int(F(max_gap) * F(o["min_join_flank_ratio"]))
        if r0["re"] - r0["rs"] < min_flank_len or r0["qe"] - r0["qs"] < min_flank_len:
            continue
        if r1["re"] - r1["rs"] < min_flank_len or r1["qe"] - r1["qs"] < min_flank_len:
            continue
        a[int(r1["as"]), 1] |= np.uint64(MM_SEED_LONG_JOIN)
        span = y1 >> 32 & 0xff
        tl, ql = s32(s32(x1) - s32(x0)), d
        r0["cnt"] = s32(int(r0["cnt"]) + int(r1["cnt"]))
        r0["score"] = s32(int(r0["score"]) + int(r1["score"]))
        r0["re"] = r1["re"]
        if rev0:
            r0["qs"] = r1["qs"]
        else:
            r0["qe"] = r1["qe"]
        r0["blen"] = s32(int(r0["blen"]) + int(r1["blen"]) - span + max(tl, ql))
        r0["mlen"] = s32(int(r0["mlen"]) + int(r1["mlen"]) - span + (span if tl > span and ql > span else min(tl, ql)))
        r1["cnt"] = 0
        r1["parent"] = r0["id"]
        n_drop += 1
    if n_drop > 0 or filter_always:
        if n_drop > 0:
            before = r["parent"].copy()
            for i in range(n):
                p = int(r["parent"][i])
                if p >= 0 and r["id"][i] != p:
                    pp = int((before if hier == "parallel" else r["parent"])[p])
                    if pp >= 0 and pp != p:
                        r["parent"][i] = pp
        r = r[[i for i in range(n) if not r["cnt"][i] < o["min_cnt"]]].copy()   # mm_filter_regs: p, inv and seg_split are 0
        sync_regs(r, n)
    return r, a, n_drop


def set_mapq(regs, min_chain_sc, rep_len, x_from="score0", log="logf", beyond=None):
    """beyond: max_log_arg -- a primary whose score or n_sub + 1 lies beyond the table gets mapq 0 (what the plan does; the reference has no table)"""
    r = regs.copy()
    if r.size == 0:
        return r
    lg = logf if log == "logf" else log if callable(log) else (lambda v: np.log(np.float64(v)))
    sum_sc = sum(int(s) for s, p, i in zip(r["score"], r["parent"], r["id"]) if p == i)
    with np.errstate(divide="ignore", invalid="ignore"):
        uniq_ratio = F(sum_sc) / F(sum_sc + rep_len)
    for i in range(r.size):
        mapq = 0
        score, cnt, n_sub = int(r["score"][i]), int(r["cnt"][i]), int(r["n_sub"][i])
        if r["parent"][i] == r["id"][i] and not (beyond is not None and (score > beyond or n_sub + 1 > beyond)):
            pen_s1 = (F(1) if score > 100 else F(0.01) * F(score)) * uniq_ratio
            pen_cm = F(1) if cnt > 10 else F(0.1) * F(cnt)
            pen_cm = pen_s1 if pen_s1 < pen_cm else pen_cm
            subsc = max(int(r["subsc"][i]), min_chain_sc)
            x = F(subsc) / F(int(r[x_from][i]))
            mapq = int(pen_cm * F(40) * (F(1) - x) * lg(score))
            mapq -= int(F(4.343) * lg(n_sub + 1) + F(0.499))
            mapq = min(max(mapq, 0), 60)
        r["flags"][i] = (int(r["flags"][i]) & ~0xff) | mapq
    return r


def join_mapq(regs, a, qlen, o, rep_len, beyond=None, **variant):
    """the hits in front of mm_join_long and the read's a[] -> (final regions, a[] of n_b_out anchors, n joined); o: the fields of mm2c_mapq_opt_t"""
    jv = {k: v for k, v in variant.items() if k in ("fp499", "hier", "filter_always", "adj")}
    mv = {k: v for k, v in variant.items() if k in ("x_from", "log")}
    r, a = np.asarray(regs, REG).copy(), np.asarray(a, np.uint64).reshape(-1, 2)
    n_j = 0
    if o["do_join"]:
        r, a, n_j = join_long(r, a, qlen, o, **jv)
    return set_mapq(r, o["min_chain_score"], rep_len, beyond=beyond, **mv), a, n_j
