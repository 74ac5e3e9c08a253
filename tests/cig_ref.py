"""The reference's own record of mm_align1 (tests/golden/ref_cig.npz, made by tests/golden/make_ref_cig_fixtures.py) laid out as the arrays the CIGAR-join plan
takes: per option set of tests/cig_data.ref_batches() the model of the alignment-task plan (tests/aln_model.py) gives regions, items, tasks and the pool; every recorded ksw
call, both passes, becomes the ksw result and CIGAR of its item's task (a task the reference never called, behind a drop, gets ksw status 1 and a refused z-drop
record: the join must not look at it); the z-drop code of a gap item is read off the record (a second pass exists iff it is not 0, its zdrop argument tells 2 from
1).  expect(): what the record says the join must give."""
import os

import numpy as np

import aln_data as AD
import aln_model as AM
import cig_data as D
import cig_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
APPROX_MAX = 0x08
_CACHE = {}


def fixture():
    if "fx" not in _CACHE:
        _CACHE["fx"] = np.load(os.path.join(GOLDEN, "ref_cig.npz"))
    return _CACHE["fx"]


def split_reg(r, n, split_inv, qlen, a):
    """mm_split_reg (hit.c:106-123) with mm_reg_set_coor and mm_cal_fuzzy_len: the region r2 that r splits off behind its first n anchors, as the record of REG_DTYPE
    mm_align1 is called on next; the score in float32 arithmetic as the reference's (int32_t)(r->score * ((float)r2->cnt / r->cnt) + .499).  a: the read's anchors"""
    r2 = r.copy()
    cnt2 = int(r["cnt"]) - n
    assert 0 < n < int(r["cnt"])
    r2["id"] = -1
    r2["cnt"] = cnt2
    r2["score"] = int(float(np.float32(np.float32(int(r["score"])) * np.float32(np.float32(cnt2) / np.float32(int(r["cnt"]))))) + .499)
    r2["as"] = int(r["as"]) + n
    if r["parent"] == r["id"]:
        r2["parent"] = -2                                                       # MM_PARENT_TMP_PRI
    k = int(r2["as"])
    lo = lambda v: int(v) & 0xffffffff
    i32 = lambda v: v - (1 << 32) if v & 0x80000000 else v
    x = [i32(lo(v)) for v in a[k:k + cnt2, 0]]
    y = [i32(lo(v)) for v in a[k:k + cnt2, 1]]
    sp = [int(v) >> 32 & 0xff for v in a[k:k + cnt2, 1]]
    rev = int(a[k, 0]) >> 63
    r2["rid"] = int(a[k, 0]) << 1 >> 33 & 0x7fffffff
    r2["rs"], r2["re"] = (x[0] + 1 - sp[0] if x[0] + 1 > sp[0] else 0), x[-1] + 1
    r2["qs"], r2["qe"] = (qlen - (y[-1] + 1), qlen - (y[0] + 1 - sp[0])) if rev else (y[0] + 1 - sp[0], y[-1] + 1)
    mlen = blen = sp[0]
    for t in range(1, cnt2):
        tl, ql = x[t] - x[t - 1], y[t] - y[t - 1]
        blen += max(tl, ql)
        mlen += sp[t] if tl > sp[t] and ql > sp[t] else min(tl, ql)
    r2["mlen"], r2["blen"] = mlen, blen
    f = int(r["flags"]) & ~((1 << 12) | (1 << 24) | (1 << 10))                    # sam_pri and split_inv cleared, rev from the anchors
    r2["flags"] = f | (rev << 10) | (int(bool(split_inv)) << 24) | (2 << 8)       # split |= 2
    return r2


def prefix(name, level):
    return name + ("_c%d" % level if level else "") + "_"


def inputs(name, level):
    """the batch of one level: the regions of cig_data.ref_batches(), or (level 1, 2) the regions the level above split off, made by split_reg from the model's join of
    that level, with the anchors as that level's alignment-task plan left them (the flags of its filters).  -> (o, u_off, regs, b_off, b, read_off, fwd, names)"""
    o, reads = D.cached_ref_batches()[name]
    c = AD.csr(reads)
    if level == 0:
        return (o,) + tuple(c)
    B, names = batch(name, level - 1)
    m = model_of(name, level - 1)
    u_off, b_off, read_off = B["u_off"], B["b_off"], B["read_off"]
    regs, nm, per = [], [], np.zeros(len(u_off) - 1, np.int64)
    for rd in range(len(u_off) - 1):
        a = B["b"][int(b_off[rd]):int(b_off[rd + 1])]
        for g in range(int(u_off[rd]), int(u_off[rd + 1])):
            O = m["cig_regs"][g]
            if O["status"] == 0 and O["split_n"] > 0:
                regs.append(split_reg(B["regs"][g], int(O["split_n"]), int(O["split_inv"]), int(read_off[rd + 1] - read_off[rd]), a))
                nm.append(names[g] + "+"); per[rd] += 1
    regs = np.array(regs, AD.REG_DTYPE).reshape(-1) if regs else np.zeros(0, AD.REG_DTYPE)
    return o, np.concatenate([[0], np.cumsum(per)]).astype(np.int64), regs, b_off, B["b"], read_off, c[5], nm


def model_of(name, level=0):
    key = ("m", name, level)
    if key not in _CACHE:
        _CACHE[key] = D.model(batch(name, level)[0])
    return _CACHE[key]


def batch(name, level=0):
    """-> (B in the layout of cig_data.build, names of the regions)"""
    if (name, level) in _CACHE:
        return _CACHE[name, level]
    fx = fixture()
    pf = prefix(name, level)
    o, u_off, regs, b_off, b, read_off, fwd, names = inputs(name, level)
    assert len(regs) == len(fx[pf + "hd"]), (name, level, "the regions are not the recorded ones")
    if level:                                                                  # the Python mm_split_reg made the region the reference called mm_align1 on
        up = fx[prefix(name, level - 1) + "hd"][fx[pf + "parent"]]
        for g, r in enumerate(regs):
            got = tuple(int(r[f]) for f in ("cnt", "as", "rs", "re", "qs", "qe", "score", "mlen", "blen", "parent")) + (int(r["flags"]) >> 24 & 1,)
            assert got == tuple(int(v) for v in up[g][[12, 13, 15, 16, 17, 18, 24, 25, 26, 27, 14]]), (name, level, g, got, up[g][12:28])
    A = AM.run(o, AD.reference(), u_off, regs, b_off, b, read_off, fwd, slot_words=2304)
    aregs, items, tasks, cig_off = A["aln_regs"], A["items"], A["tasks"], A["cig_off"]
    n_items, n_tasks = A["totals"][0], A["totals"][1]
    items, tasks, cig_off = items[:n_items], tasks[:n_tasks], cig_off[:n_tasks + 1]
    sr = bool(o["flag"] & 1)
    opt = dict(zdrop=o["zdrop"], zdrop_inv=o["zdrop_inv"], bw_ext=int(o["bw"] * 1.5 + 1.), min_cnt=o["min_cnt"], flag=o["flag"], cig_shift=0)
    mat = D.mat_of(o["a"], o["b"], o["sc_ambi"])
    calls, call_off, cw, cw_off, hd = fx[pf + "calls"], fx[pf + "call_off"], fx[pf + "cw"], fx[pf + "cw_off"], fx[pf + "hd"]
    assert (aregs["as1"] == hd[:, 28]).all() and (aregs["cnt1"] == hd[:, 29]).all() or (aregs["status"] != 0).any()
    res, zres = np.zeros(n_tasks, M.KSW_RES_DTYPE), np.zeros(n_tasks, M.ZDROP_RES_DTYPE)
    res["status"] = 1; zres["status"] = 1                                      # until the record names a call for the task
    cigar = np.full(int(cig_off[-1]), 0xdeadbee0, np.uint32)
    F = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "n_cigar", "reach_end")

    def put(r, rec):
        for f, v in zip(F, rec[8:]):
            r[f] = int(v) & 0xffffffff if f == "max" else int(v)

    second = {}                                                                # item -> index of its second-pass call
    for g in range(len(aregs)):
        R = aregs[g]
        j, end = int(call_off[g]), int(call_off[g + 1])
        if R["status"] != 0:
            continue
        for k in range(int(R["item0"]), int(R["item0"]) + int(R["n_items"])):
            it = items[k]
            base = int(it["kind"]) & 15
            if it["kind"] & M.OVER:
                continue
            if base == M.UNGAPPED:
                if j < end and calls[j, 5] == 0 and calls[j, 4] == -1:
                    second[k] = j; j += 1
                continue
            t = int(it["task"])
            if j >= end:
                continue                                                       # behind the drop: never called
            rec = calls[j]
            T = tasks[t]
            assert (int(T["qlen"]), int(T["tlen"]), int(T["w"]), int(T["end_bonus"]), int(T["flag"])) == tuple(int(x) for x in rec[[0, 1, 2, 4, 5]]), (name, g, k)
            put(res[t], rec)
            res[t]["status"] = 0
            w = cw[int(cw_off[j]):int(cw_off[j + 1])]
            assert w.size <= cig_off[t + 1] - cig_off[t]
            cigar[int(cig_off[t]):int(cig_off[t]) + w.size] = w
            zres[t]["status"] = 0
            j += 1
            if base == M.GAP and j < end and rec[5] & APPROX_MAX and calls[j, 5] == rec[5] & ~APPROX_MAX and (calls[j, :2] == rec[:2]).all() and (calls[j, 6:8] == rec[6:8]).all():
                zres[t]["code"] = 2 if calls[j, 3] == o["zdrop_inv"] else 1      # every non-sr option set has zdrop != zdrop_inv
                second[k] = j; j += 1
        assert j == end, (name, g, "calls the items do not account for")
    B = dict(opt=opt, mat=mat, u_off=u_off, regs=regs, b_off=b_off, b=A["b"], read_off=read_off, aregs=aregs, items=items, tasks=tasks, cig_off=cig_off, res=res, cigar=cigar,
             zres=zres, pool=A["pool"][:A["totals"][3]])
    S = M.second_pass(opt, aregs, items, tasks, zres, B["pool"], mat)
    assert sorted(int(k) for k in np.nonzero(S["second_of"] >= 0)[0]) == sorted(second), (name, "the second passes are not the recorded ones")
    res2 = np.zeros(len(S["tasks2"]), M.KSW_RES_DTYPE)
    cigar2 = np.full(int(S["cig_off2"][-1]), 0xfeedfac0, np.uint32)
    for k, j in second.items():
        s = int(S["second_of"][k])
        T, rec = S["tasks2"][s], calls[j]
        # the second list's task is the call the reference made: lengths, band, zdrop, end_bonus, flag
        assert (int(T["qlen"]), int(T["tlen"]), int(T["w"]), int(T["zdrop"]), int(T["end_bonus"]), int(T["flag"])) == tuple(int(x) for x in rec[:6]), (name, k)
        put(res2[s], rec)
        w = cw[int(cw_off[j]):int(cw_off[j + 1])]
        cigar2[int(S["cig_off2"][s]):int(S["cig_off2"][s]) + w.size] = w
    B.update(tasks2=S["tasks2"], cig_off2=S["cig_off2"], second_of=S["second_of"], res2=res2, cigar2=cigar2, second=S)
    _CACHE[name, level] = (B, names)
    return _CACHE[name, level]


def mismatches(name, B, cig_regs, cigs, level=0):
    """what of the join's output differs from the record: the CIGAR and dp_score in front of mm_update_extra, has_p, the split and r2, and, through extra_model's
    mm_update_extra on the pool's sequences, the final r->rs / re / qs / qe, blen, mlen, n_ambi, dp_max and CIGAR"""
    import extra_model
    fx = fixture()
    pf = prefix(name, level)
    hd, pre, pre_off, fin, fin_off = fx[pf + "hd"], fx[pf + "pre"], fx[pf + "pre_off"], fx[pf + "fin"], fx[pf + "fin_off"]
    o = D.cached_ref_batches()[name][0]
    bad = []
    for g in range(len(cig_regs)):
        R, O, h = B["aregs"][g], cig_regs[g], hd[g]
        if R["status"] != 0:
            continue
        if O["status"] != 0:
            bad.append((g, "status", int(O["status"]))); continue
        cig = [int(w) for w in cigs[g]]
        if int(O["has_p"]) != int(h[5]):
            bad.append((g, "has_p"))
        if h[19]:
            if int(O["dp_score"]) != int(h[20]) or cig != [int(w) for w in pre[int(pre_off[g]):int(pre_off[g + 1])]]:
                bad.append((g, "dp_score or the appended CIGAR", int(O["dp_score"]), int(h[20])))
        elif h[5] or cig:
            bad.append((g, ":787 not reached"))
        r = B["regs"][g]
        if (int(O["split_n"]) > 0) != (h[12] > 0) or (h[12] > 0 and (int(r["as"]) + int(O["split_n"]), int(r["cnt"]) - int(O["split_n"]), int(O["split_inv"])) != (int(h[13]), int(h[12]), int(h[14]))):
            bad.append((g, "split", int(O["split_n"]), int(O["split_inv"]), [int(x) for x in h[12:15]]))
        if not h[5]:
            continue
        q0, t0 = int(R["q_off"]) + int(O["qs1"] - R["qs0"]), int(R["t_off"]) + int(O["rs1"] - R["rs0"])
        try:
            X = extra_model.update_extra(B["pool"][q0:q0 + int(O["qe1"] - O["qs1"])], B["pool"][t0:t0 + int(O["re1"] - O["rs1"])], cig, B["mat"], o["q"], o["e"], 0)
        except (extra_model.Undefined, IndexError) as e:                       # the assert of :284 would fire, or the walk leaves the sequences
            bad.append((g, "mm_update_extra is not defined on it", str(e))); continue
        rs, re = int(O["rs1"]) + X["tshift"], int(O["re1"])
        qs, qe = (int(O["r_qs"]), int(O["r_qe"]) - X["qshift"]) if R["rev"] else (int(O["r_qs"]) + X["qshift"], int(O["r_qe"]))
        got = (rs, re, qs, qe, int(O["dp_score"]), X["dp_max"], X["blen"], X["mlen"], X["n_ambi"], X["n_cigar"])
        want = tuple(int(x) for x in (h[1], h[2], h[3], h[4], h[6], h[7], h[8], h[9], h[10], h[11]))
        if got != want or X["cigar"].tolist() != fin[int(fin_off[g]):int(fin_off[g + 1])].tolist():
            bad.append((g, "the final region", got, want))
    return bad
