"""NumPy / Python restatement of mm_set_parent (hit.c:125-186) and mm_select_sub (hit.c:255-272, with mm_sync_regs / mm_set_sam_pri hit.c:220-253) on REG_DTYPE
arrays, for regions whose p, is_alt and inv are 0 (what mm_gen_regs makes).  The float tests are evaluated in np.float32 step by step as the C expressions are.
The keyword variants restate the step the "natural" way instead; the tests use them to show that the planted cases tell the difference:
  pick="best"      the passing primary of highest score instead of the first in w order
  in_place=False   mm_select_sub reads the parent from the untouched array instead of from the array it is compacting
  fp=np.float64    the two float tests in double
  always_sync=True mm_sync_regs (ids, parents, sam_pri) even when nothing was dropped
  uncov=f          uncov_len by f(si, ei, prim) instead of the sorted sweep: uncov_by_gaps (the kernel's way, equal to the sweep) and its two wrong forms,
                   uncov_by_gaps_round_lost and uncov_by_gaps_every_end (tests/hits_limit_data.py holds the cases that tell them from the reference)"""
import numpy as np

from regs_model import REG

SAM_PRI_BIT = 12                                                               # minimap.h:96: mapq:8, split:2, rev:1, inv:1, sam_pri:1
MM_PARENT_UNSET, MM_PARENT_TMP_PRI = -1, -2


def uncov_len(si, ei, prim):
    """hit.c:138-156: the sorted sweep over the clipped overlaps; prim: [(qs, qe)] of the primaries in w order"""
    cov = []
    for sj, ej in prim:
        if ej <= si or sj >= ei:
            continue
        cov.append((max(sj, si), min(ej, ei)))
    if not cov:
        return 0, 0
    cov.sort()
    x, un = si, 0
    for s, e in cov:
        if s > x:
            un += s - x
        x = max(x, e)
    if ei > x:
        un += ei - x
    return un, len(cov)


def uncov_by_gaps(si, ei, prim, round_lost=False, every_end=False):
    """the same measure as the kernel finds it (csrc/chain_hits.hip): every candidate gap start g -- si or the end of a clipped interval -- opens a gap if no interval
    holds g, g < ei and no earlier interval ends there too; the gap reaches to the nearest interval start beyond g, or ei.
    The candidates are taken 64 at a time and si is candidate number n_cov; round_lost: the rounds stop at t0 < n_cov, so si is lost when n_cov is a multiple of 64;
    every_end: every interval that ends at g opens the gap, not only the first"""
    cov = [(max(sj, si), min(ej, ei)) for sj, ej in prim if not (ej <= si or sj >= ei)]
    if not cov:
        return 0
    un = 0
    for t in range(len(cov) + 1):
        if round_lost and t == len(cov) and t % 64 == 0:
            continue
        g = cov[t][1] if t < len(cov) else si
        if g >= ei or any(a <= g < b for a, b in cov) or (not every_end and any(cov[q][1] == g for q in range(min(t, len(cov))))):
            continue
        un += min([a for a, _ in cov if a > g] + [ei]) - g
    return un


def uncov_by_gaps_round_lost(si, ei, prim):
    return uncov_by_gaps(si, ei, prim, round_lost=True)


def uncov_by_gaps_every_end(si, ei, prim):
    return uncov_by_gaps(si, ei, prim, every_end=True)


def passes(si, ei, sj, ej, un, mask_level, mask_len, fp=np.float32):
    """hit.c:160-165 for one overlapping primary"""
    mn, mx = min(ej - sj, ei - si), max(ej - sj, ei - si)
    ol = (0 if ei < sj else ei - sj if ei < ej else ej - sj) if si < sj else (0 if ej < si else ej - si if ej < ei else ei - si)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = fp(ol) / fp(mn) - fp(un) / fp(mx)
        return bool(v > fp(np.float32(mask_level))) and un <= mask_len


def set_parent(regs, mask_level, mask_len, hard_mask_level, fp=np.float32, pick="first", uncov=None):
    r = regs.copy()
    n = r.size
    if n <= 0:
        return r
    r["id"] = np.arange(n)
    w = [0]
    r["parent"][0] = 0
    for i in range(1, n):
        si, ei = int(r["qs"][i]), int(r["qe"][i])
        prim = [(int(r["qs"][j]), int(r["qe"][j])) for j in w]
        un = 0 if hard_mask_level else uncov_len(si, ei, prim)[0] if uncov is None else uncov(si, ei, prim)
        hit = []
        for j in w:
            sj, ej = int(r["qs"][j]), int(r["qe"][j])
            if ej <= si or sj >= ei:
                continue
            if passes(si, ei, sj, ej, un, mask_level, mask_len, fp):
                hit.append(j)
                if pick == "first":
                    break
        if hit:
            j = hit[0] if pick == "first" else max(hit, key=lambda q: int(r["score"][q]))
            r["parent"][i] = r["parent"][j]
            r["subsc"][j] = max(int(r["subsc"][j]), int(r["score"][i]))
            if r["cnt"][i] >= r["cnt"][j]:
                r["n_sub"][j] += 1
        else:
            w.append(i)
            r["parent"][i] = i
            r["n_sub"][i] = 0
    return r


def sync_regs(r):
    """hit.c:231-253 on the kept regions"""
    n = r.size
    if n <= 0:
        return
    tmp = np.full(int(r["id"].max()) + 1, -1, np.int64)
    for i in range(n):
        if r["id"][i] >= 0:
            tmp[r["id"][i]] = i
    n_pri = 0
    for i in range(n):
        p = int(r["parent"][i])
        r["id"][i] = i
        if p == MM_PARENT_TMP_PRI:
            r["parent"][i] = i
        elif p >= 0 and tmp[p] >= 0:
            r["parent"][i] = tmp[p]
        else:
            r["parent"][i] = MM_PARENT_UNSET
    for i in range(n):
        r["flags"][i] &= ~np.uint32(1 << SAM_PRI_BIT)
        if r["id"][i] == r["parent"][i]:
            n_pri += 1
            if n_pri == 1:
                r["flags"][i] |= np.uint32(1 << SAM_PRI_BIT)


def select_sub(regs, pri_ratio, min_diff, best_n, fp=np.float32, in_place=True, always_sync=False):
    """-> the kept regions (a new array of *n_ entries)"""
    r = regs.copy()
    n = r.size
    if not (np.float32(pri_ratio) > 0 and n > 0):
        return r
    k = n_2nd = 0
    for i in range(n):
        p = int(r["parent"][i])
        if p == i:
            r[k] = r[i]; k += 1
            continue
        rp = r[p] if in_place else regs[p]
        sc, scp = int(r["score"][i]), int(rp["score"])
        if (fp(sc) >= fp(scp) * fp(np.float32(pri_ratio)) or sc + min_diff >= scp) and n_2nd < best_n:
            if not all(r[f][i] == rp[f] for f in ("qs", "qe", "rid", "rs", "re")):
                r[k] = r[i]; k += 1; n_2nd += 1
    out = r[:k].copy()
    if k != n or always_sync:
        sync_regs(out)
    return out


def select_hits(regs, opt, **variant):
    """opt: dict with the fields of mm2c_hit_opt_t -> the array the reference holds after mm_set_parent + mm_select_sub"""
    sp = {k: v for k, v in variant.items() if k in ("fp", "pick", "uncov")}
    ss = {k: v for k, v in variant.items() if k in ("fp", "in_place", "always_sync")}
    r = set_parent(np.asarray(regs, REG), opt["mask_level"], opt["mask_len"], opt["hard_mask_level"], **sp)
    return select_sub(r, opt["pri_ratio"], opt["min_diff"], opt["best_n"], **ss)
