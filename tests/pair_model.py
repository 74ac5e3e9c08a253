"""Python restatement of what the pair plan computes (csrc/pair_ends.hip) on the two REG arrays of a fragment whose p is 1 + the index of a PEXT
record: pair(): mm_pair (pe.c:76-177) with mm_set_pe_thru (pe.c:45-63), then the flip of map.c:455-466.  Float steps are evaluated in np.float32 one by one as the C
expressions are; the logarithm is the host's own logf through ctypes (mapq_model.logf).  klib's radix_sort_pair is regs_model's replay of ksort.h.  The keyword
variants restate a step the "natural" way; the tests use them to show that the planted cases tell the difference:
  sort="stable"         a stable sort above 64 records too
  winner="ge"           >= for the winner: the last in scan order among equal scores
  stop="continue"       continue in the place of the break of pe.c:120
  first_test=False      no first test against a[last] (pe.c:115)
  n_sub="others"        n_sub without the optimal pair
  second="distinct"     the second-largest among distinct values
  lift_mapq="keep"      a lift that keeps the old primary's mapq
  pe_thru="before"      mm_set_pe_thru's primaries counted before the lifts
  fp="fused"            the mapq expressions with fused multiply-adds"""
from fractions import Fraction

import numpy as np

from fin_model import PEXT
from mapq_model import logf
from regs_model import REG
import regs_model

F = np.float32
REV_BIT, SAM_PRI_BIT, PROPER_FRAG_BIT, PE_THRU_BIT = 10, 12, 13, 14
OPT_FIELDS = ("max_gap_ref", "pe_bonus", "sub_diff", "match_sc", "pe_ori", "flip")
M32, M64 = 0xffffffff, 0xffffffffffffffff


class Refused(Exception):
    """the plan refuses the fragment: nothing of it is written but its status"""


def s32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def _r32(x):
    """a Fraction rounded once to float32 (through the nearest double)"""
    return F(float(x))


def check(regs, pext):
    """what pair_select refuses, mate by mate"""
    for r in regs:
        for i in range(r.size):
            p, rs = int(r["p"][i]), int(r["rs"][i])
            if p == 0 or p - 1 >= pext.size or r["rid"][i] < 0 or rs < 0 or rs >= 1 << 30 or r["id"][i] != i or not 0 <= r["parent"][i] < r.size:
                raise Refused


def radix_sort_pair(keys, sort="klib"):
    """the arrangement klib's radix_sort_pair leaves: -> order, order[t] = index of the record at ascending position t"""
    n = len(keys)
    stable = sorted(range(n), key=lambda i: (keys[i], i))
    if n <= 64 or sort == "stable" or len(set(keys)) == n:
        return stable
    z = [(int(k), i) for i, k in enumerate(keys)]
    regs_model.radix_sort_128x(z)
    return [i for _, i in z]


def set_pe_thru(qlens, regs):
    n_pri, pri = [0, 0], [-1, -1]
    for s in range(2):
        for i in range(regs[s].size):
            if regs[s]["id"][i] == regs[s]["parent"][i]:
                n_pri[s] += 1; pri[s] = i
    if n_pri == [1, 1]:
        p, q = regs[0][pri[0]], regs[1][pri[1]]
        rev = lambda r: int(r["flags"]) >> REV_BIT & 1
        if (p["rid"] == q["rid"] and rev(p) == rev(q) and abs(int(p["rs"]) - int(q["rs"])) < 3 and abs(int(p["re"]) - int(q["re"])) < 3 and
                ((p["qs"] == 0 and qlens[1] - int(q["qe"]) == 0) or (q["qs"] == 0 and qlens[0] - int(p["qe"]) == 0))):
            return pri
    return None


def pair(regs0, regs1, pext, qlens, opt, gap=None, max_log_arg=1 << 16, sort="klib", winner="gt", stop="break", first_test=True, n_sub="all", second="multiset",
         lift_mapq="zero", pe_thru="after", fp="ieee"):
    """-> (regs0, regs1 behind mm_pair, mm_set_pe_thru and the flip (copies), info); info: found, n_sc, n_sub, beyond (n_sub beyond the table), lifted, winners (input
    indices per mate), order (the sorted arrangement as (mate, index)).  Raises Refused."""
    regs = [np.array(regs0, REG, copy=True), np.array(regs1, REG, copy=True)]
    check(regs, pext)
    max_gap_ref = int(opt["max_gap_ref"]) if gap is None else int(gap)
    info = dict(found=False, n_sc=0, n_sub=0, beyond=False, lifted=[False, False], winners=None, order=None, thru=False)
    if regs[0].size and regs[1].size:                                          # pe.c:97-100
        a, dp_thres = [], 0
        for s in range(2):
            mx = 0
            for i in range(regs[s].size):
                r = regs[s][i]
                rev = int(r["flags"]) >> REV_BIT & 1
                key = (int(r["rid"]) << 32 | int(r["rs"]) << 1 | (s ^ rev)) & M64
                dm = int(pext["dp_max"][int(r["p"]) - 1])
                a.append(dict(s=s, i=i, rev=rev, key=key, rid=int(r["rid"]), rs=int(r["rs"]), re=int(r["re"]), dp=dm, hash=int(r["hash"])))
                mx = max(mx, dm)
            dp_thres += mx
        dp_thres = max(dp_thres - int(opt["pe_bonus"]), 0)
        a = [a[k] for k in radix_sort_pair([e["key"] for e in a], sort)]
        info["order"] = [(e["s"], e["i"]) for e in a]
        thru_before = set_pe_thru(qlens, regs) if pe_thru == "before" else None
        mx, max_idx, last, sc = -1, [-1, -1], [-1, -1], []
        for i, e in enumerate(a):
            if e["key"] & 1:
                L = last[e["rev"]]
                if L < 0:
                    continue
                q = a[L]
                if first_test and (e["rid"] != q["rid"] or e["rs"] - q["re"] > max_gap_ref):
                    continue
                for j in range(L, -1, -1):
                    q = a[j]
                    if q["rev"] != e["rev"] or q["s"] == e["s"]:
                        continue
                    if e["rid"] != q["rid"] or e["rs"] - q["re"] > max_gap_ref:
                        if stop == "break":
                            break
                        continue
                    sm = s32(e["dp"] + q["dp"])
                    if sm < dp_thres:
                        continue
                    score = sm * (1 << 32) | ((e["hash"] + q["hash"]) & M32)   # (int64_t)sum << 32 | uint32 sum
                    if score > mx or (winner == "ge" and score >= mx):
                        mx = score; max_idx[q["s"]] = j; max_idx[e["s"]] = i
                    sc.append(score & M64)
            else:
                last[e["rev"]] = i
        sc.sort()                                                              # radix_sort_64: distinct orders of equal values cannot be told apart
        info["n_sc"] = len(sc)
        if sc and mx > 0:                                                      # pe.c:134
            info["found"] = True
            w = [a[max_idx[0]]["i"], a[max_idx[1]]["i"]]
            info["winners"] = w
            for s in range(2):
                R = regs[s]
                R["flags"][w[s]] |= 1 << PROPER_FRAG_BIT
                if R["id"][w[s]] != R["parent"][w[s]]:
                    p = int(R["parent"][w[s]])
                    pid = int(R["id"][p])
                    for i in range(R.size):
                        if R["parent"][i] == pid:
                            R["parent"][i] = R["id"][w[s]]
                    if lift_mapq == "zero":
                        R["flags"][p] &= ~np.uint32(0xff)
                    info["lifted"][s] = True
                if not int(R["flags"][w[s]]) >> SAM_PRI_BIT & 1:
                    R["flags"] &= ~np.uint32(1 << SAM_PRI_BIT)
                    R["flags"][w[s]] |= 1 << SAM_PRI_BIT
            q = [int(regs[s]["flags"][w[s]]) & 0xff for s in range(2)]
            mapq_pe = max(q)
            maxhi = (mx & M64) >> 32
            cnt = sum(1 for v in sc if (v >> 32) + int(opt["sub_diff"]) >= maxhi)
            if n_sub == "others":
                cnt -= 1
            info["n_sub"] = cnt
            sec = None
            if len(sc) > 1:
                sec = sc[-2] >> 32
                if second == "distinct":
                    d = sorted(set(sc))
                    sec = d[-2] >> 32 if len(d) > 1 else d[-1] >> 32
                if not 0 <= cnt <= max_log_arg:
                    info["beyond"] = True
                elif cnt == 0:                                                 # only the n_sub="others" variant: logf(0) is -inf, the cast is undefined
                    mapq_pe = min(mapq_pe, 1 << 30)
                else:
                    diff = F((maxhi - sec) & M64)                              # int64 - uint64 is uint64, then to float
                    lg = logf(cnt)
                    if fp == "fused":
                        t = F(F(6.02) * diff) / F(int(opt["match_sc"]))
                        alt = int(_r32(Fraction(float(t)) - Fraction(float(F(4.343))) * Fraction(float(lg))))
                    else:
                        alt = int(F(F(F(6.02) * diff) / F(int(opt["match_sc"]))) - F(F(4.343) * lg))
                    mapq_pe = min(mapq_pe, alt)
            if not info["beyond"]:
                for s in range(2):
                    if q[s] < mapq_pe:
                        if fp == "fused":
                            t = _r32(Fraction(float(F(.8))) * mapq_pe + Fraction(float(F(F(.2) * F(q[s])))))
                            q[s] = int(F(t + F(.499)))
                        else:
                            q[s] = int(F(F(F(.2) * F(q[s])) + F(F(.8) * F(mapq_pe))) + F(.499))
                if len(sc) == 1:
                    q = [max(v, 2) for v in q]
                elif maxhi > sec:
                    q = [max(v, 1) for v in q]
                for s in range(2):
                    regs[s]["flags"][w[s]] = (int(regs[s]["flags"][w[s]]) & ~0xff) | (q[s] & 0xff)
        pri = thru_before if pe_thru == "before" else set_pe_thru(qlens, regs)
        if pri is not None:
            info["thru"] = True
            for s in range(2):
                regs[s]["flags"][pri[s]] |= 1 << PE_THRU_BIT
    if opt["flip"]:                                                            # map.c:455-466
        for j in range(2):
            if (j == 0 and int(opt["pe_ori"]) >> 1 & 1) or (j == 1 and int(opt["pe_ori"]) & 1):
                R = regs[j]
                qs = R["qs"].copy()
                R["qs"] = qlens[j] - R["qe"]
                R["qe"] = qlens[j] - qs
                R["flags"] ^= np.uint32(1 << REV_BIT)
    return regs[0], regs[1], info


def pair_case(c, **variant):
    """pair() on a case of pair_data"""
    return pair(c["regs"][0], c["regs"][1], c["pext"], c["qlens"], c["opt"], gap=c.get("gap"), max_log_arg=c.get("max_log_arg", 1 << 16), **variant)
