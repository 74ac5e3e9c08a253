"""NumPy / Python restatement of what the finish plan computes (csrc/align_finish.hip) on REG arrays whose p is 0 or 1 + the index of a PEXT record:
apply(): what mm_align1 leaves in a region, with mm_split_reg (align.c:757-760, 781-783; hit.c:108-123); finish(): mm_filter_regs (hit.c:274-293), mm_hit_sort
(hit.c:188-218), mm_set_parent (hit.c:125-186), mm_select_sub (hit.c:255-272), mm_set_sam_pri (hit.c:220-229) and mm_set_mapq (hit.c:463-506).  Float steps are
evaluated in np.float32 one by one as the C expressions are; the logarithm is the host's own logf through ctypes (mapq_model.logf).  klib's radix_sort_128x is
replay_model's.  The keyword variants restate a step the "natural" way; the tests use them to show that the planted cases tell the difference:
  clip="double"         the clip test of hit.c:284 in double
  sort="stable"         a stable sort above 64 records too
  key="score"           the sort key from r->score under p
  dp2_identical=True    dp_max2 / cnt_sub without the exclusion of pairs identical after DP
  sam_pri="on_drop"     sam_pri only recomputed when mm_select_sub dropped something
  xx="fused"            1 - x * x with the product kept exact (a fused multiply-add)
  alt_under_sr=True     mapq_alt also under is_sr
  split_fp="float"      the split score's + .499 in float"""
import numpy as np

from hits_model import SAM_PRI_BIT, uncov_len, passes, sync_regs
from mapq_model import logf
from regs_model import REG

F = np.float32
PEXT = np.dtype([("dp_score", "<i4"), ("dp_max", "<i4"), ("dp_max2", "<i4"), ("ambi_strand", "<u4"), ("n_cigar", "<i4"), ("reserved", "<i4"), ("cig0", "<i8")])
CIG_REG = np.dtype([(n, "<i4") for n in ("status", "n_used", "dropped", "drop_item", "zdrop_code", "split_n", "split_inv", "has_p", "n_cigar", "dp_score", "rs1", "re1",
                                         "qs1", "qe1", "r_qs", "r_qe")] + [("cig0", "<i8")])
EXTRA_RES = np.dtype([(n, "<i4") for n in ("n_cigar", "qshift", "tshift", "blen", "mlen", "n_ambi", "dp_max", "status")])
INV_BIT, SEG_SPLIT_BIT, SPLIT_INV_BIT, IS_ALT_BIT, REV_BIT = 11, 15, 24, 25, 10
REFUSED, INCOMPLETE, OVER_CAP = 1, 2, 3
OPT_FIELDS = ("min_cnt", "min_chain_score", "min_dp_max", "max_clip_ratio", "mask_level", "mask_len", "hard_mask_level", "sub_diff", "pri_ratio", "min_diff", "best_n",
              "match_sc", "is_sr", "all_chains")


class Refused(Exception):
    """the plan refuses the read: nothing of it is written"""


def radix_sort_128x(keys, sort="klib"):
    """the arrangement klib's radix_sort_128x leaves: -> order, order[i] = index of the record at ascending position i"""
    n = len(keys)
    stable = sorted(range(n), key=lambda i: (keys[i], i))
    if n <= 64 or sort == "stable" or len(set(keys)) == n:
        return stable
    import regs_model
    z = [(int(k), i) for i, k in enumerate(keys)]
    regs_model.radix_sort_128x(z)
    return [i for _, i in z]


def split_score(score, cnt2, cnt, fp="double"):
    part = F(score) * (F(cnt2) / F(cnt))
    return int(F(part + F(.499))) if fp == "float" else int(float(part) + .499)


def split_reg(r, n, split_inv, qlen, a, split_fp="double"):
    """mm_split_reg: -> (r after it, r2); a: the read's anchors uint64 [., 2]"""
    import cig_ref
    r2 = cig_ref.split_reg(r, n, split_inv, qlen, a)
    r2["score"] = split_score(int(r["score"]), int(r2["cnt"]), int(r["cnt"]), split_fp)
    r1 = r.copy()
    r1["cnt"] = int(r["cnt"]) - int(r2["cnt"])
    r1["score"] = int(r["score"]) - int(r2["score"])
    r1["flags"] = int(r["flags"]) | (1 << 8)
    return r1, r2


def apply(u_off, regs, b_off, b, read_off, cig_regs, extra_reg, extra_res, out_off, n_child_cap, split_fp="double"):
    """-> dict(regs, pext, status, child, child_of, n_child, counts=(refused, incomplete, beyond)); entries the plan does not write are None / absent"""
    n = len(regs)
    out, pext, status = [None] * n, [None] * n, np.zeros(n, np.int32)
    child, child_of = [], []
    k_of = {int(g): k for k, g in enumerate(extra_reg)}
    bb = np.asarray(b, np.uint64).reshape(-1, 2)
    for rd in range(len(u_off) - 1):
        a = bb[int(b_off[rd]):int(b_off[rd + 1])]
        qlen = int(read_off[rd + 1] - read_off[rd])
        for g in range(int(u_off[rd]), int(u_off[rd + 1])):
            R, C = regs[g], cig_regs[g]
            st = 0 if C["status"] == 0 else REFUSED if C["status"] == 1 else INCOMPLETE
            E = None
            if st == 0 and C["has_p"]:
                if g not in k_of:
                    st = REFUSED
                else:
                    E = extra_res[k_of[g]]
                    st = 0 if E["status"] == 0 else REFUSED if E["status"] == 1 else INCOMPLETE
            split = 0 < int(C["split_n"]) < int(R["cnt"])
            if st == 0 and split and not (0 <= int(R["as"]) + int(C["split_n"]) and int(R["as"]) + int(R["cnt"]) <= len(a)):
                st = REFUSED
            status[g] = st
            if st:
                continue
            O = R.copy()
            if split:
                O, r2 = split_reg(R, int(C["split_n"]), int(C["split_inv"]), qlen, a, split_fp)
                child.append(r2); child_of.append(g)
            O["rs"], O["re"], O["qs"], O["qe"] = C["rs1"], C["re1"], C["r_qs"], C["r_qe"]
            P = np.zeros((), PEXT)
            O["p"] = 0
            if C["has_p"]:
                O["rs"] += E["tshift"]
                if int(R["flags"]) >> REV_BIT & 1:
                    O["qe"] -= E["qshift"]
                else:
                    O["qs"] += E["qshift"]
                O["blen"], O["mlen"], O["p"] = E["blen"], E["mlen"], g + 1
                P["dp_score"], P["dp_max"], P["ambi_strand"], P["n_cigar"], P["cig0"] = C["dp_score"], E["dp_max"], int(E["n_ambi"]) & 0x3fffffff, E["n_cigar"], out_off[k_of[g]]
            out[g], pext[g] = O, P
    n_child = len(child)
    for k in range(n_child_cap, n_child):
        status[child_of[k]] = OVER_CAP
    return dict(regs=out, pext=pext, status=status, child=child[:n_child_cap], child_of=child_of[:n_child_cap], n_child=n_child,
                counts=(int((status == REFUSED).sum()), int((status == INCOMPLETE).sum()), max(n_child - n_child_cap, 0)))


def filter_regs(r, pext, qlen, o, clip="float"):
    keep = []
    for i in range(r.size):
        fl = int(r["flags"][i])
        flt = not (fl >> INV_BIT & 1) and not (fl >> SEG_SPLIT_BIT & 1) and int(r["cnt"][i]) < o["min_cnt"]
        if r["p"][i]:
            qs, qe = int(r["qs"][i]), int(r["qe"][i])
            if clip == "double":
                lim = qlen * float(F(o["max_clip_ratio"]))
                clipped = qs > lim and qlen - qe > lim
            else:
                lim = F(qlen) * F(o["max_clip_ratio"])
                clipped = bool(F(qs) > lim) and bool(F(qlen - qe) > lim)
            if int(r["mlen"][i]) < o["min_chain_score"] or int(pext["dp_max"][int(r["p"][i]) - 1]) < o["min_dp_max"] or clipped:
                flt = True
        if not flt:
            keep.append(i)
    return keep


def hit_sort(r, pext, keep, sort="klib", key="dp_max"):
    """-> the input indices in the order mm_hit_sort leaves them"""
    if len(keep) <= 1:
        return keep
    aux = [i for i in keep if (int(r["flags"][i]) >> INV_BIT & 1) or int(r["cnt"][i]) > 0]
    has = any(r["p"][i] != 0 for i in aux)
    no = any(r["p"][i] == 0 for i in aux)
    if int(has) + int(no) != 1:
        raise Refused("hit.c:210")
    keys = []
    for i in aux:
        sc = int(pext["dp_max"][int(r["p"][i]) - 1]) if r["p"][i] and key == "dp_max" else int(r["score"][i])
        keys.append(((sc & 0xffffffff) << 32) | int(r["hash"][i]))
    order = radix_sort_128x(keys, sort)
    return [aux[order[i]] for i in range(len(aux) - 1, -1, -1)]


def set_parent(r, dpm, dpm2, o, dp2_identical=False):
    """mm_set_parent with hit.c:171-176 on r (in place); dpm / dpm2: dp_max and dp_max2 per region (None without p)"""
    n = r.size
    if n <= 0:
        return
    r["id"] = np.arange(n)
    w = [0]
    r["parent"][0] = 0
    for i in range(1, n):
        si, ei = int(r["qs"][i]), int(r["qe"][i])
        prim = [(int(r["qs"][j]), int(r["qe"][j])) for j in w]
        un = 0 if o["hard_mask_level"] else uncov_len(si, ei, prim)[0]
        hit = None
        for j in w:
            sj, ej = int(r["qs"][j]), int(r["qe"][j])
            if ej <= si or sj >= ei:
                continue
            if passes(si, ei, sj, ej, un, o["mask_level"], o["mask_len"]):
                hit = j
                break
        if hit is None:
            w.append(i)
            r["parent"][i] = i
            r["n_sub"][i] = 0
            continue
        j = hit
        sj, ej = int(r["qs"][j]), int(r["qe"][j])
        mn = min(ej - sj, ei - si)
        ol = (0 if ei < sj else ei - sj if ei < ej else ej - sj) if si < sj else (0 if ej < si else ej - si if ej < ei else ei - si)
        r["parent"][i] = r["parent"][j]
        r["subsc"][j] = max(int(r["subsc"][j]), int(r["score"][i]))
        cnt_sub = r["cnt"][i] >= r["cnt"][j]
        if dpm[j] is not None and dpm[i] is not None and (dp2_identical or r["rid"][j] != r["rid"][i] or r["rs"][j] != r["rs"][i] or r["re"][j] != r["re"][i] or ol != mn):
            dpm2[j] = max(dpm2[j], dpm[i])
            if dpm[j] - dpm[i] <= o["sub_diff"]:
                cnt_sub = True
        if cnt_sub:
            r["n_sub"][j] += 1


def select_sub(r, o):
    """-> (the kept positions, whether mm_sync_regs ran)"""
    n = r.size
    if not (F(o["pri_ratio"]) > 0 and n > 0):
        return list(range(n)), False
    src, n_2nd = [], 0
    for i in range(n):
        p = int(r["parent"][i])
        if p == i:
            src.append(i)
            continue
        pp = src[p] if len(src) > p else p                                     # what lies at position p by now
        sc, scp = int(r["score"][i]), int(r["score"][pp])
        if (F(sc) >= F(scp) * F(o["pri_ratio"]) or sc + o["min_diff"] >= scp) and n_2nd < o["best_n"]:
            if not all(r[f][i] == r[f][pp] for f in ("qs", "qe", "rid", "rs", "re")):
                src.append(i); n_2nd += 1
    return src, len(src) != n


def set_mapq(r, dpm, dpm2, o, rep_len, max_log_arg=None, xx="plain", alt_under_sr=False):
    """mm_set_mapq on r (in place) -> primaries beyond the table"""
    beyond = 0
    if r.size == 0:
        return 0
    sum_sc = sum(int(r["score"][i]) for i in range(r.size) if r["parent"][i] == r["id"][i])
    with np.errstate(divide="ignore", invalid="ignore"):
        uniq = F(sum_sc) / F(sum_sc + rep_len)
    for i in range(r.size):
        mapq = 0
        if r["parent"][i] == r["id"][i]:
            score, cnt, n_sub1 = int(r["score"][i]), int(r["cnt"][i]), int(r["n_sub"][i]) + 1
            larg = dpm[i] if dpm[i] is not None else score
            if max_log_arg is not None and not (0 <= larg <= max_log_arg and 0 <= n_sub1 <= max_log_arg):
                beyond += 1
            else:
                pen_s1 = (F(1.0) if score > 100 else F(0.01) * F(score)) * uniq
                pen_cm = F(1.0) if cnt > 10 else F(0.1) * F(cnt)
                pen_cm = pen_s1 if pen_s1 < pen_cm else pen_cm
                subsc = max(int(r["subsc"][i]), o["min_chain_score"])
                with np.errstate(divide="ignore", invalid="ignore"):
                    if dpm[i] is not None:
                        identity = F(int(r["mlen"][i])) / F(int(r["blen"][i]))
                        lg = F(logf(F(dpm[i]) / F(o["match_sc"])))
                    if dpm[i] is not None and dpm2[i] > 0 and dpm[i] > 0:
                        x = F(dpm2[i]) * F(subsc) / F(dpm[i]) / F(int(r["score0"][i]))
                        one = F(1.0 - float(x) * float(x)) if xx == "fused" else F(1.0) - x * x
                        mapq = int(identity * pen_cm * F(40.0) * one * lg)
                        if not o["is_sr"] or alt_under_sr:
                            alt = int(F(6.02) * identity * identity * F(dpm[i] - dpm2[i]) / F(o["match_sc"]) + F(.499))
                            mapq = min(mapq, alt)
                    else:
                        x = F(subsc) / F(int(r["score0"][i]))
                        if dpm[i] is not None:
                            mapq = int(identity * pen_cm * F(40.0) * (F(1.0) - x) * lg)
                        else:
                            mapq = int(pen_cm * F(40.0) * (F(1.0) - x) * logf(score))
                    mapq -= int(F(4.343) * logf(n_sub1) + F(.499))
                mapq = min(max(mapq, 0), 60)
                if dpm[i] is not None and dpm[i] > dpm2[i] and mapq == 0:
                    mapq = 1
        r["flags"][i] = (int(r["flags"][i]) & ~0xff) | mapq
    return beyond


def finish(regs, pext, qlen, rep_len, o, max_log_arg=None, clip="float", sort="klib", key="dp_max", dp2_identical=False, sam_pri="always", xx="plain", alt_under_sr=False):
    """one read -> dict(regs: the reference's array behind map.c:361, idx: the input index of every survivor, pext: the records with dp_max2 updated, beyond)
    regs: REG in the order mm_align_skeleton holds them; pext: PEXT; p of a region: 0 or 1 + the index of its record.  Raises Refused."""
    r = np.asarray(regs, REG).copy()
    px = np.asarray(pext, PEXT).copy()
    fl = r["flags"].astype(np.int64)
    if ((fl >> INV_BIT & 1) | (fl >> IS_ALT_BIT & 1)).any():
        raise Refused("inv or is_alt")
    if ((r["p"] != 0) & (r["p"].astype(np.int64) - 1 >= px.size)).any():
        raise Refused("p names no record")
    keep = filter_regs(r, px, qlen, o, clip)
    idx = hit_sort(r, px, keep, sort, key)
    out = r[idx].copy() if idx else np.zeros(0, REG)
    dpm = [int(px["dp_max"][int(p) - 1]) if p else None for p in out["p"]]
    dpm2 = [int(px["dp_max2"][int(p) - 1]) if p else 0 for p in out["p"]]
    synced = False
    if not o["all_chains"]:
        set_parent(out, dpm, dpm2, o, dp2_identical)
        src, synced = select_sub(out, o)
        out, idx, dpm, dpm2 = out[src].copy(), [idx[s] for s in src], [dpm[s] for s in src], [dpm2[s] for s in src]
        if synced:
            sync_regs(out)
        if sam_pri == "always" or synced:                                      # mm_set_sam_pri (map.c:267)
            n_pri = 0
            for i in range(out.size):
                out["flags"][i] &= ~np.uint32(1 << SAM_PRI_BIT)
                if out["id"][i] == out["parent"][i]:
                    n_pri += 1
                    if n_pri == 1:
                        out["flags"][i] |= np.uint32(1 << SAM_PRI_BIT)
        for i in range(out.size):
            if dpm[i] is not None:
                px["dp_max2"][int(out["p"][i]) - 1] = dpm2[i]
    beyond = set_mapq(out, dpm, dpm2, o, rep_len, max_log_arg, xx, alt_under_sr)
    return dict(regs=out, idx=idx, pext=px, beyond=beyond)
