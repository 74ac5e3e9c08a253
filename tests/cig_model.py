"""NumPy restatement of what mm_align1 does with its ksw results (align.c:698-705, 736-764, 772-783; include/mm2chain.h, the mm2c_cigplan_t section): the list of
second passes, the cut behind the first dropped gap item, mm_append_cigar with its merge at the boundary, the dp_score sums, rs1 / qs1 / re1 / qe1 and the split
decision.  Plain loops over records; `variant` names one deliberate mistake (VARIANTS), which the CPU test shows to differ on a planted case."""
import numpy as np

from aln_model import ALN_REG_DTYPE, ALN_ITEM_DTYPE, KSW_TASK_DTYPE, REG_DTYPE

KSW_RES_DTYPE = np.dtype([("max", "<u4"), ("zdropped", "<i4"), ("max_q", "<i4"), ("max_t", "<i4"), ("mqe", "<i4"), ("mqe_t", "<i4"), ("mte", "<i4"), ("mte_q", "<i4"),
                          ("score", "<i4"), ("n_cigar", "<i4"), ("reach_end", "<i4"), ("status", "<i4")])
ZDROP_RES_DTYPE = np.dtype([("max_zdrop", "<i4"), ("t0", "<i4"), ("t1", "<i4"), ("q0", "<i4"), ("q1", "<i4"), ("code", "<i4"), ("inv_cand", "<i4"), ("status", "<i4")])
EXTRA_TASK_DTYPE = np.dtype([("q_off", "<i8"), ("t_off", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"), ("n_cigar", "<i4"), ("rev", "<i4")])
CIG_OPT_DTYPE = np.dtype([(n, "<i4") for n in ("zdrop", "zdrop_inv", "bw_ext", "min_cnt", "flag", "cig_shift")])
CIG_REG_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_used", "dropped", "drop_item", "zdrop_code", "split_n", "split_inv", "has_p", "n_cigar", "dp_score", "rs1", "re1",
                                               "qs1", "qe1", "r_qs", "r_qe")] + [("cig0", "<i8")])
REFUSED, INCOMPLETE, OVER_CAP, NO_ROOM, LOST = 1, 2, 3, -2, -3
LEFT, GAP, RIGHT, UNGAPPED, OVER = 0, 1, 2, 3, 16
F_SR = 1
APPROX_MAX = 0x08
VARIANTS = ("no_boundary_merge", "merge_inside_items", "ext_score_for_max", "max_t_under_reach_end", "j_lt", "no_j_clamp", "split_gt", "right_behind_drop", "drop_score_for_max",
            "first_pass_ez", "zdrop_for_inv", "no_strand_flip", "append_behind_drop")


def i32(v):
    v = int(v) & 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def slot_of(s, shift):
    return min(s, (s >> shift) + 16)


def sr_test(q, t, mat, zdrop):
    """mm_test_zdrop on one M word: the running maximum starts at INT32_MIN, every point lies on one diagonal"""
    score, mx, best = 0, -(1 << 31), 0
    for a, b in zip(t, q):
        score += int(mat[min(int(a), 4) * 5 + min(int(b), 4)])
        if score < mx:
            best = max(best, mx - score)
        else:
            mx = score
    return 1 if best > zdrop else 0


def second_pass(opt, aregs, items, tasks, zres, pool, mat, n_tasks2_cap=1 << 30, cigar2_cap=1 << 60, variant=None):
    """-> dict(tasks2, cig_off2, second_of, totals, n_over)"""
    second_of = np.full(len(items), -1, np.int32)
    t2, co2 = [], [0]
    n_over = n_lost = 0
    tot_t = tot_c = 0
    for R in aregs:
        if R["status"] != 0:
            continue
        mine = []
        for k in range(int(R["item0"]), int(R["item0"]) + int(R["n_items"])):
            it = items[k]
            if it["kind"] == GAP and it["task"] >= 0:
                z = zres[it["task"]]
                if z["status"] == 0 and z["code"] in (1, 2):
                    T = tasks[it["task"]].copy()
                    T["flag"] &= ~APPROX_MAX
                    T["zdrop"] = opt["zdrop_inv"] if z["code"] == 2 and variant != "zdrop_for_inv" else opt["zdrop"]
                    mine.append((k, T))
            elif it["kind"] == UNGAPPED and (opt["flag"] & F_SR):
                qo, to = int(R["q_off"]) + int(it["qs"] - R["qs0"]), int(R["t_off"]) + int(it["rs"] - R["rs0"])
                n = int(it["qe"] - it["qs"])
                nt = int(it["re"] - it["rs"])
                if n < 0 or nt < 0 or qo < 0 or to < 0 or qo + n > len(pool) or to + nt > len(pool) or n > nt:
                    second_of[k] = LOST                                            # its bases leave the pool
                    n_lost += 1
                    continue
                if sr_test(pool[qo:qo + n], pool[to:to + n], mat, opt["zdrop"]):
                    T = np.zeros((), KSW_TASK_DTYPE)
                    T["q_off"], T["t_off"], T["qlen"], T["tlen"], T["w"], T["zdrop"], T["end_bonus"], T["flag"] = qo, to, n, int(it["re"] - it["rs"]), opt["bw_ext"], opt["zdrop"], -1, 0
                    mine.append((k, T))
        words = [slot_of(int(T["qlen"]) + int(T["tlen"]), opt["cig_shift"]) for _, T in mine]
        room = not mine or (tot_t + len(mine) <= n_tasks2_cap and tot_c + sum(words) <= cigar2_cap)
        if not room:
            n_over += 1
        for n, (k, T) in enumerate(mine):
            if room:
                second_of[k] = tot_t + n
                t2.append((tot_t + n, T, tot_c + sum(words[:n])))
            else:
                second_of[k] = NO_ROOM
        tot_t += len(mine)
        tot_c += sum(words)
    tasks2 = np.zeros(tot_t, KSW_TASK_DTYPE)
    cig_off2 = np.zeros(tot_t + 1, np.int64)
    written = np.zeros(tot_t, bool)                                                # the tasks of a region without room are not written
    for idx, T, c in t2:
        tasks2[idx] = T
        cig_off2[idx] = c
        written[idx] = True
    cig_off2[tot_t] = tot_c
    return dict(tasks2=tasks2, cig_off2=cig_off2, second_of=second_of, totals=(tot_t, tot_c), n_over=n_over, written=written, n_lost=n_lost)


def eff(k, items, cig_off, res, cigar, zres, second_of, cig_off2, res2, cigar2, variant=None):
    """the effective ez of item k: dict(n, words, zdropped, max, max_q, max_t, mqe_t, score, reach_end, code, bad)"""
    it = items[k]
    E = dict(n=0, words=[], zdropped=0, max=0, max_q=0, max_t=0, mqe_t=0, score=0, reach_end=0, code=0, bad=0)
    base = int(it["kind"]) & 15
    if it["kind"] & OVER:
        E.update(zdropped=1, max_q=-1, max_t=-1, mqe_t=-1)
        return E
    s, t = int(second_of[k]), int(it["task"])
    if base == UNGAPPED:
        if s == NO_ROOM:
            E["bad"] = INCOMPLETE
            return E
        if s == LOST:
            E["bad"] = REFUSED
            return E
        if s < 0:
            E.update(n=1, words=[(int(it["qe"] - it["qs"]) << 4) & 0xffffffff], score=int(it["score"]))
            return E
        E["code"] = 1
    else:
        if t < 0 or t >= len(res):
            E["bad"] = REFUSED
            return E
        if base == GAP:
            z = zres[t]
            if z["status"] != 0 or not 0 <= z["code"] <= 2 or (z["code"] == 0 and s >= 0):
                E["bad"] = REFUSED
                return E
            if z["code"] != 0 and s < 0:
                E["bad"] = INCOMPLETE
                return E
            E["code"] = int(z["code"])
        elif s >= 0 or base not in (LEFT, RIGHT):
            E["bad"] = REFUSED
            return E
    if s >= 0 and variant != "first_pass_ez":
        if s >= len(res2):
            E["bad"] = REFUSED
            return E
        r, c0, c1, buf = res2[s], int(cig_off2[s]), int(cig_off2[s + 1]), cigar2
    else:
        r, c0, c1, buf = res[t], int(cig_off[t]), int(cig_off[t + 1]), cigar
    if c0 < 0 or c1 < c0 or c1 > len(buf):
        E["bad"] = REFUSED
        return E
    if r["status"] != 0 or r["n_cigar"] < 0 or r["n_cigar"] > c1 - c0:
        E["bad"] = INCOMPLETE
        return E
    n = int(r["n_cigar"])
    E.update(n=n, words=[int(w) for w in buf[c0:c0 + n]], zdropped=int(r["zdropped"]), max=i32(r["max"]), max_q=int(r["max_q"]), max_t=int(r["max_t"]), mqe_t=int(r["mqe_t"]),
             score=int(r["score"]), reach_end=int(r["reach_end"]))
    return E


def append(cig, words, variant=None):
    """mm_append_cigar (:288-311)"""
    if not words:
        return
    words = list(words)
    if variant == "merge_inside_items":
        m = []
        for w in words:
            if m and (m[-1] & 0xf) == (w & 0xf):
                m[-1] = (m[-1] + (w >> 4 << 4)) & 0xffffffff
            else:
                m.append(w)
        words = m
    if cig and (cig[-1] & 0xf) == (words[0] & 0xf) and variant != "no_boundary_merge":
        cig[-1] = (cig[-1] + (words[0] >> 4 << 4)) & 0xffffffff
        cig.extend(words[1:])
    else:
        cig.extend(words)


def region(opt, r, R, a, qlen, items, E_of, variant=None):
    """one region -> (CIG_REG record without cig0, its CIGAR words)"""
    O = np.zeros((), CIG_REG_DTYPE)
    refuse = lambda s: (np.array((s,) + (0,) * 16, CIG_REG_DTYPE), None)
    if R["status"] != 0:
        return refuse(REFUSED)
    if R["cnt1"] == 0 and R["n_items"] == 0:
        O["rs1"], O["re1"], O["r_qs"], O["r_qe"] = r["rs"], r["re"], r["qs"], r["qe"]
        return O, []
    i0, n = int(R["item0"]), int(R["n_items"])
    if n < 0 or i0 < 0 or i0 + n > len(items) or R["as1"] < 0 or R["cnt1"] < 1 or int(R["as1"]) + int(R["cnt1"]) > len(a):
        return refuse(REFUSED)
    as1, cnt1 = int(R["as1"]), int(R["cnt1"])
    cig, dp = [], 0
    rs1, qs1 = int(R["rs"]), int(R["qs"])
    re1, qe1 = int(R["rs"]), int(R["qs"])
    dropped, drop_item, code, split_n, split_inv, n_used = 0, -1, 0, 0, 0, 0
    bad = 0
    for k in range(n):
        it = items[i0 + k]
        base = int(it["kind"]) & 15
        if dropped and not (variant == "right_behind_drop" and base == RIGHT) and variant != "append_behind_drop":
            continue                                                               # everything behind the drop is cut, the right extension too
        E = E_of(i0 + k)
        if dropped:                                                                # only a wrong variant comes here
            if E["bad"]:
                continue
            if variant == "append_behind_drop":
                append(cig, E["words"], variant)
                continue
        else:
            n_used += 1
        if E["bad"]:
            bad = E["bad"] if bad != REFUSED else bad
            continue
        if base == LEFT:
            if E["n"] > 0:
                append(cig, E["words"], variant)
                dp += E["score"] if variant == "ext_score_for_max" else E["max"]
            under = E["max_t"] if variant == "max_t_under_reach_end" else E["mqe_t"]
            rs1 = int(it["re"]) - (under + 1 if E["reach_end"] else E["max_t"] + 1)
            qs1 = int(it["qe"]) - (int(it["qe"] - it["qs"]) if E["reach_end"] else E["max_q"] + 1)
        elif base in (GAP, UNGAPPED):
            append(cig, E["words"], variant)
            if E["zdropped"]:
                dropped, drop_item, code = 1, k, E["code"]
                dp += E["score"] if variant == "drop_score_for_max" else E["max"]
                re1, qe1 = int(it["rs"]) + E["max_t"] + 1, int(it["qs"]) + E["max_q"] + 1
                i = int(it["anchor"]) - as1
                if i < 0 or i >= cnt1:
                    return refuse(REFUSED)
                thr = int(it["rs"]) + E["max_t"]
                j = i - 1
                while j >= 0:
                    x = i32(int(a[as1 + j][0]) & 0xffffffff)
                    if (x < thr) if variant == "j_lt" else (x <= thr):
                        break
                    j -= 1
                if j < 0 and variant != "no_j_clamp":
                    j = 0
                rest = cnt1 - (j + 1)
                if (rest > opt["min_cnt"]) if variant == "split_gt" else (rest >= opt["min_cnt"]):
                    split_n, split_inv = as1 + j + 1 - int(r["as"]), int(code == 2)
            else:
                dp += E["score"]
                re1, qe1 = int(it["re"]), int(it["qe"])
        elif base == RIGHT:
            if E["n"] > 0:
                append(cig, E["words"], variant)
                dp += E["score"] if variant == "ext_score_for_max" else E["max"]
            under = E["max_t"] if variant == "max_t_under_reach_end" else E["mqe_t"]
            re1 = int(it["rs"]) + (under + 1 if E["reach_end"] else E["max_t"] + 1)
            qe1 = int(it["qs"]) + (int(it["qe"] - it["qs"]) if E["reach_end"] else E["max_q"] + 1)
        else:
            return refuse(REFUSED)
    if bad:
        return refuse(bad)
    has_p = int(bool(cig) or dropped)
    if variant is None:
        ql = sum(w >> 4 for w in cig if (w & 0xf) <= 1)
        tl = sum(w >> 4 for w in cig if (w & 0xf) in (0, 2, 3))
        if has_p and (ql != qe1 - qs1 or tl != re1 - rs1):
            return refuse(REFUSED)
        if qs1 < 0 or rs1 < 0 or qe1 > qlen or re1 - rs1 > int(R["re0"]) - int(R["rs0"]):
            return refuse(REFUSED)
    O["n_used"], O["dropped"], O["drop_item"], O["zdrop_code"], O["split_n"], O["split_inv"], O["has_p"] = n_used, dropped, drop_item, code, split_n, split_inv, has_p
    O["n_cigar"], O["dp_score"] = len(cig), i32(dp)
    O["rs1"], O["re1"], O["qs1"], O["qe1"] = rs1, re1, qs1, qe1
    flip = R["rev"] and variant != "no_strand_flip"
    O["r_qs"], O["r_qe"] = (qlen - qe1, qlen - qs1) if flip else (qs1, qe1)
    return O, cig


def assemble(opt, u_off, regs, b_off, b, read_off, aregs, items, cig_off, res, cigar, zres, second_of, cig_off2, res2, cigar2, words_cap=1 << 60, extra_cap=1 << 60, variant=None):
    """-> dict(cig_regs, cigs (a list per region, None where none is written), cig_out, in_off, extra_tasks, extra_reg, totals, counts (refused, incomplete, over_cap))"""
    n_reads = len(u_off) - 1
    out = np.zeros(int(u_off[-1]), CIG_REG_DTYPE)
    cigs = [None] * len(out)
    E_of = lambda k: eff(k, items, cig_off, res, cigar, zres, second_of, cig_off2, res2, cigar2, variant)
    for rd in range(n_reads):
        a = np.asarray(b[int(b_off[rd]):int(b_off[rd + 1])], np.uint64).reshape(-1, 2)
        qlen = int(read_off[rd + 1] - read_off[rd])
        for g in range(int(u_off[rd]), int(u_off[rd + 1])):
            out[g], cigs[g] = region(opt, regs[g], aregs[g], a, qlen, items, E_of, variant)
    words, k = 0, 0
    cig_out, in_off, extra, extra_reg = [], [], [], []
    counts = [int((out["status"] == REFUSED).sum()), int((out["status"] == INCOMPLETE).sum()), 0]
    for g in range(len(out)):
        if out[g]["status"] != 0:
            continue
        n = int(out[g]["n_cigar"])
        if n > 0 and (words + n > words_cap or k >= extra_cap):
            out[g]["status"] = OVER_CAP                                            # the record keeps what the region came to; only its words are not written
            cigs[g] = None
            counts[2] += 1
        else:
            out[g]["cig0"] = words
            if n > 0:
                R, O = aregs[g], out[g]
                in_off.append(words); extra_reg.append(g)
                extra.append((int(R["q_off"]) + int(O["qs1"] - R["qs0"]), int(R["t_off"]) + int(O["rs1"] - R["rs0"]), int(O["qe1"] - O["qs1"]), int(O["re1"] - O["rs1"]), n, int(R["rev"])))
                cig_out.extend(cigs[g])
        words += n
        k += n > 0
    in_off.append(words)
    return dict(cig_regs=out, cigs=cigs, cig_out=np.array(cig_out, np.uint32), in_off=np.array(in_off, np.int64), extra_tasks=np.array(extra, EXTRA_TASK_DTYPE).reshape(-1),
                extra_reg=np.array(extra_reg, np.int32), totals=(words, k), counts=tuple(counts))
