"""NumPy / Python restatement of mm_select_sub_multi (pe.c:6-43, with mm_sync_regs hit.c:220-253) and mm_seg_gen (hit.c:373-427) on REG arrays whose p, is_alt and
inv are 0, and of the fragment path they stand in (map.c:344, 252-254, 365-370).  `int` arithmetic wraps; the score tests are evaluated in np.float32 step by step
as the C expressions are.  mm_set_parent, mm_gen_regs and mm_set_mapq are the models of the steps before (hits_model, regs_model, mapq_model).
The keyword variants restate a step the "natural" way; the tests use them to show that the planted cases tell the difference:
  fp=np.float64        the three score tests in double
  strict=True          score > pscore * ratio in place of >=
  dist_le=True         <= max_dist in place of < in the two closeness tests
  in_place=False       the parent is read from the untouched array instead of from the array being compacted
  identical_drop=True  mm_select_sub's identical-hit test kept
  max_dist_any=True    max_dist = qlens[0] + qlens[1] + max_gap_ref for any n_segs >= 2
  count_all=True       n_2nd counts every secondary, whether it passed its test or not
  turn_by="region"     hit.c:414 turned by the region's rev instead of the anchor's own strand bit
  forget_qlen=True     the reverse shift without qlens[sid]
  order="as"           a segment's anchors in the order the chains lie in a[] instead of region order"""
import numpy as np

import hits_model
import mapq_model
import regs_model
from regs_model import REG, M64, s32

F = np.float32
SEG_SPLIT_BIT, SEG_ID_SHIFT, REV_BIT = 15, 16, 10


def select_sub_multi(regs, pri_ratio, pri1, pri2, max_gap_ref, min_diff, best_n, n_segs, qlens, fp=np.float32, strict=False, dist_le=False, in_place=True,
                     identical_drop=False, max_dist_any=False, count_all=False):
    """-> the kept regions (a new array of *n_ entries)"""
    r = regs.copy()
    n = r.size
    if not (F(pri_ratio) > 0 and n > 0):
        return r
    two = n_segs == 2
    max_dist = s32(int(qlens[0]) + int(qlens[1]) + max_gap_ref) if (two or (max_dist_any and n_segs >= 2)) else 0
    q0 = int(qlens[0])
    rev = lambda x: (int(x["flags"]) >> REV_BIT) & 1
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    lt = (lambda a, b: a <= b) if dist_le else (lambda a, b: a < b)
    k = n_2nd = 0
    for i in range(n):
        p = int(r["parent"][i])
        keep = p == i
        if not keep:
            rp = r[p] if in_place else regs[p]
            q = r[i]
            sc, scp = int(q["score"]), int(rp["score"])
            if s32(sc + min_diff) >= scp:
                keep = True
            else:
                if rev(rp) == rev(q) and rp["rid"] == q["rid"] and lt(s32(int(q["re"]) - int(rp["rs"])), max_dist) and lt(s32(int(rp["re"]) - int(q["rs"])), max_dist):
                    ratio = pri1
                else:
                    par_both = two and rp["qs"] < q0 and rp["qe"] > q0
                    chi_both = two and q["qs"] < q0 and q["qe"] > q0
                    ratio = pri_ratio if chi_both or chi_both == par_both else pri2
                keep = bool(ge(fp(sc), fp(scp) * fp(F(ratio))))
            if keep and identical_drop and all(q[f] == rp[f] for f in ("qs", "qe", "rid", "rs", "re")):
                keep = False
            if keep or count_all:                                               # pe.c:35: n_2nd++ for every secondary that passed, kept or not
                if n_2nd >= best_n:
                    keep = False
                n_2nd += 1
        if keep:
            r[k] = r[i]; k += 1
    out = r[:k].copy()
    if k != n:
        hits_model.sync_regs(out)
    return out


def seg_gen(hash_, n_segs, qlens, regs0, a, turn_by="anchor", forget_qlen=False, order="region", sort=None):
    """-> [(u uint64 [n_u], a uint64 [n_a, 2], regs REG [n_u])] per segment: seg[s].u, seg[s].a and regs[s] of hit.c:419-424"""
    a = np.asarray(a, np.uint64).reshape(-1, 2)
    qlens = [int(v) for v in qlens]
    acc = [0] * n_segs
    for s in range(1, n_segs):
        acc[s] = s32(acc[s - 1] + qlens[s - 1])
    qlen_sum = s32(acc[n_segs - 1] + qlens[n_segs - 1])
    u = [[(int(r["score"]) << 32) & M64 for r in regs0] for _ in range(n_segs)]
    sa = [[] for _ in range(n_segs)]
    walk = range(regs0.size) if order == "region" else sorted(range(regs0.size), key=lambda i: int(regs0["as"][i]))
    for i in range(regs0.size):
        r = regs0[i]
        for j in range(int(r["cnt"])):
            sid = int(a[int(r["as"]) + j, 1]) >> 48 & 0xff
            u[sid][i] = (u[sid][i] + 1) & M64
    for i in walk:
        r = regs0[i]
        for j in range(int(r["cnt"])):
            x, y = int(a[int(r["as"]) + j, 0]), int(a[int(r["as"]) + j, 1])
            sid = y >> 48 & 0xff
            turned = (int(r["flags"]) >> REV_BIT) & 1 if turn_by == "region" else x >> 63
            d = s32(qlen_sum - ((0 if forget_qlen else qlens[sid]) + acc[sid])) if turned else acc[sid]
            sa[sid].append((x, (y - d) & M64))                                   # hit.c:414: a 64-bit subtraction of a sign-extended int
    out = []
    for s in range(n_segs):
        us = np.array([v for v in u[s] if s32(v) != 0], np.uint64)
        as_ = np.array(sa[s], np.uint64).reshape(-1, 2)
        regs = regs_model.gen_regs(hash_, qlens[s], us, as_, sort=sort)
        regs["flags"] |= np.uint32(1 << SEG_SPLIT_BIT | s << SEG_ID_SHIFT)
        out.append((us, as_, regs))
    return out


def frag_hits(c, **variant):
    """a case of seg_data -> the array behind mm_gen_regs -> mm_set_parent -> mm_select_sub_multi"""
    h, m = c["hit"], c["multi"]
    r = regs_model.gen_regs(c["hash"], int(c["qlens"].sum()), c["u"], c["a"])
    r = hits_model.set_parent(r, h["mask_level"], h["mask_len"], h["hard_mask_level"])
    return select_sub_multi(r, h["pri_ratio"], m["pri1"], m["pri2"], c["gap_ref"], h["min_diff"], h["best_n"], c["n_segs"], c["qlens"], **variant)


def seg_final(c, regs):
    """regs[s] -> what map.c:368-370 leave: mm_set_parent, mm_set_mapq"""
    h = c["hit"]
    r = hits_model.set_parent(regs, h["mask_level"], h["mask_len"], h["hard_mask_level"])
    return mapq_model.set_mapq(r, c["mapq"]["min_chain_score"], c["rep_len"])
