"""Seeded inputs of the CIGAR-join tests (tests/test_cpu_cig_model.py, tests/test_gpu_cig.py): regions described by the ez and the CIGAR words of their items, laid
out as the arrays the alignment-task plan, the ksw plan and the z-drop entry leave (aln_regs, items, tasks, cig_off, res, cigar, zres) with a batch around them
(u_off, regs, b_off, b, read_off) whose coordinates follow from the words, so that the length check of align.c:284 holds.  No sequences but for sr."""
import numpy as np

import cig_model as M

OPS = "MIDN"
OPT = dict(zdrop=400, zdrop_inv=200, bw_ext=751, min_cnt=3, flag=0, cig_shift=0)
OPT_SR = dict(zdrop=100, zdrop_inv=100, bw_ext=151, min_cnt=2, flag=1, cig_shift=0)
SR_SCORE = (2, 8, 12, 2, 1)               # a, b, q, e, sc_ambi of the sr preset
K2 = 7                                    # k >> 1 of mm_adjust_minier


def mat_of(a, b, amb):
    m = np.full(25, -b, np.int8)
    for i in range(4):
        m[i * 5 + i] = a
    m[4::5] = -amb
    m[20:] = -amb
    return m


def words(s):
    """'5M2I' -> BAM words"""
    out, n = [], ""
    for ch in s:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | OPS.index(ch)); n = ""
    return out


def lens(ws):
    return sum(w >> 4 for w in ws if (w & 0xf) <= 1), sum(w >> 4 for w in ws if (w & 0xf) in (0, 2, 3))


def ez(cig="", zdropped=0, reach_end=0, score=None, mx=None, second=None, code=None, over=False, status=0, zstatus=0, slot=None, n_cigar=None, anchors=1):
    """one item: its (first-pass) CIGAR as text or words, its scalars, and `second`, another ez, if a second pass replaces it (code 1 or 2).  anchors: how many
    anchors the item spans (gap items).  status: the ksw status; zstatus: the z-drop record's; slot: words of its CIGAR slot; n_cigar: a count that differs from the words"""
    ws = words(cig) if isinstance(cig, str) else list(cig)
    ql, tl = lens(ws)
    return dict(words=ws, zdropped=zdropped, reach_end=reach_end, score=2 * ql - 3 if score is None else score, max=2 * ql + 1 if mx is None else mx, second=second,
                code=(code if code is not None else (0 if second is None else 1)), over=over, status=status, zstatus=zstatus, slot=slot, n_cigar=n_cigar, anchors=anchors)


def region(gaps, left=None, right=None, rev=0, pre=0, post=0, pin_eq=False, sr=None, as_status=0):
    """gaps: list of ez; left / right: ez or None; pre / post: anchors of the read's region in front of as1 and behind as1 + cnt1; pin_eq: the anchor in front of the
    dropped item's gets x == rs + max_t exactly; sr: dict(n, bad=(start, count)) for one ungapped item of n bases with a run of mismatches instead of `gaps`"""
    return dict(gaps=gaps, left=left, right=right, rev=rev, pre=pre, post=post, pin_eq=pin_eq, sr=sr, as_status=as_status)


def build(regions, opt=OPT, per_read=1, seed=5):
    """-> dict of every array of a batch, and `E`: per item the spec it came from"""
    rng = np.random.default_rng(seed)
    sr = bool(opt["flag"] & M.F_SR)
    mat = mat_of(SR_SCORE[0], SR_SCORE[1], SR_SCORE[4]) if sr else mat_of(2, 4, 1)
    n = len(regions)
    aregs, regs = np.zeros(n, M.ALN_REG_DTYPE), np.zeros(n, M.REG_DTYPE)
    items, tasks, res, zres, cigar, cig_off, specs = [], [], [], [], [], [0], []
    b, b_off, read_off, u_off = [], [0], [0], [0]
    pool = []
    cur_a, cur_qlen = [], 0
    for g, S in enumerate(regions):
        R = aregs[g]
        eff = lambda e: e["second"] if e is not None and e["second"] is not None else e
        qs0, rs0 = 11, 1000 + 13 * g
        item0 = len(items)
        R["item0"], R["task0"], R["cig0"], R["rev"], R["status"] = item0, len(tasks), cig_off[-1], S["rev"], S["as_status"]
        R["q_off"] = len(pool)

        def put(kind, anchor, rs, re, qs, qe, e, score=0):
            over = e is not None and e["over"]
            t = -1
            if e is not None and not over:
                t = len(tasks)
                T = np.zeros((), M.KSW_TASK_DTYPE)
                T["q_off"], T["t_off"], T["qlen"], T["tlen"], T["w"], T["zdrop"], T["end_bonus"] = R["q_off"] + (qs - qs0), R["q_off"] + 100000 + (rs - rs0), qe - qs, re - rs, opt["bw_ext"], opt["zdrop"], -1
                T["flag"] = {M.LEFT: 0xc2, M.GAP: M.APPROX_MAX, M.RIGHT: 0x40}[kind]
                tasks.append(T)
                r, z = np.zeros((), M.KSW_RES_DTYPE), np.zeros((), M.ZDROP_RES_DTYPE)
                ql, tl = lens(e["words"])
                r["n_cigar"] = len(e["words"]) if e["n_cigar"] is None else e["n_cigar"]
                r["zdropped"], r["reach_end"], r["score"], r["max"], r["status"] = e["zdropped"], e["reach_end"], e["score"], e["max"], e["status"]
                r["max_q"], r["max_t"], r["mqe_t"], r["mqe"], r["mte"], r["mte_q"] = ql - 1, tl - 1, tl - 1, 77, 78, 79
                if e["reach_end"]:
                    r["max_t"] = tl + 3                                            # under reach_end mqe_t counts, max_t is another number
                    r["max_q"] = ql + 2
                z["code"], z["status"], z["max_zdrop"] = e["code"], e["zstatus"], 5
                res.append(r); zres.append(z)
                slot = M.slot_of(int(qe - qs) + int(re - rs), opt["cig_shift"]) if e["slot"] is None else e["slot"]
                cigar.extend((e["words"] + [0xdeadbee0] * slot)[:slot])
                cig_off.append(cig_off[-1] + slot)
            items.append((g, kind | (M.OVER if over else 0), anchor, rs, re, qs, qe, t, score, 0))
            specs.append(e)

        L, Rt = S["left"], S["right"]
        qs, rs = qs0, rs0
        if L is not None:
            ql, tl = lens(eff(L)["words"]) if not L["over"] else (40, 40)
            qs, rs = qs0 + ql + (0 if eff(L)["reach_end"] else 7), rs0 + tl + 9
        else:
            qs0 = rs0 = 0
            qs, rs = 0, 1000 + 13 * g
            rs0 = rs
        R["qs0"], R["rs0"], R["qs"], R["rs"] = qs0, rs0, qs, rs
        as1 = S["pre"]
        a = [[rs0 + 1 + i, 0] for i in range(S["pre"])]                            # anchors the alignment-task plan trimmed off the front
        a.append([rs + K2, 0])
        if L is not None:
            put(M.LEFT, as1, rs0, rs, qs0, qs, L)
        cq, ct = qs, rs
        pin = None
        if S["sr"] is not None:
            nb = S["sr"]["n"]
            q = rng.integers(0, 4, nb).astype(np.uint8)
            t = q.copy()
            st, cnt = S["sr"].get("bad", (0, 0))
            t[st:st + cnt] = (t[st:st + cnt] + 1) & 3
            score = int(sum(int(mat[int(x) * 5 + int(y)]) for x, y in zip(t, q)))
            e = S["gaps"][0] if S["gaps"] else None
            for i in range(3):
                a.append([ct + (i + 1) * nb // 4, 0])
            a.append([ct + nb - 1, 0])
            S["_seq"] = (q, t, cq - qs0, ct - rs0)
            put(M.UNGAPPED, as1 + len(a) - S["pre"] - 1, ct, ct + nb, cq, cq + nb, None, score)
            specs[-1] = e                                                          # the second pass of the ungapped item, if its test gives 1
            if e is not None and e["zdropped"]:
                ql, tl = lens(e["words"])
            cq, ct = cq + nb, ct + nb
        else:
            for e in S["gaps"]:
                f = eff(e)
                ql, tl = (0, 0) if e["over"] else lens(f["words"])
                dropped = e["over"] or f["zdropped"]
                span_q, span_t = (ql + 30, tl + 30) if dropped else (ql, tl)
                if e["over"]:
                    span_q = span_t = 5000
                for i in range(1, e["anchors"]):
                    a.append([ct + K2 + 1 + i * max(span_t, 1) // e["anchors"], 0])
                if dropped and S["pin_eq"] and pin is None:
                    pin = (len(a) - 1, ct + (tl - 1))
                a.append([ct + span_t + K2, 0])
                put(M.GAP, as1 + len(a) - S["pre"] - 1, ct, ct + span_t, cq, cq + span_q, e)
                cq, ct = cq + span_q, ct + span_t
        if pin is not None:
            a[pin[0]][0] = pin[1]
        cnt1 = len(a) - S["pre"]
        R["qe"], R["re"] = cq, ct
        qe0, re0 = cq, ct
        if Rt is not None:
            ql, tl = lens(eff(Rt)["words"]) if not Rt["over"] else (40, 40)
            qe0, re0 = cq + ql + (0 if eff(Rt)["reach_end"] else 7), ct + tl + 9
            put(M.RIGHT, as1 + cnt1 - 1, ct, re0, cq, qe0, Rt)
        for i in range(S["post"]):
            a.append([re0 + 50 + i, 0])
        R["qe0"], R["re0"], R["as1"], R["cnt1"], R["n_items"], R["n_tasks"] = qe0, re0, as1, cnt1, len(items) - item0, len(tasks) - R["task0"]
        R["t_off"] = R["q_off"] + 100000
        if S["sr"] is not None:
            q, t, dq, dt = S["_seq"]
            pool.extend([4] * ((qe0 - qs0 + 15) // 16 * 16)); pool.extend([4] * ((re0 - rs0 + 15) // 16 * 16))
            R["t_off"] = R["q_off"] + (qe0 - qs0 + 15) // 16 * 16
            pool[R["q_off"] + dq:R["q_off"] + dq + len(q)] = q.tolist()
            pool[R["t_off"] + dt:R["t_off"] + dt + len(t)] = t.tolist()
        regs[g]["as"], regs[g]["cnt"], regs[g]["rs"], regs[g]["re"], regs[g]["qs"], regs[g]["qe"] = 0, len(a), rs, ct, qs, cq
        for i, v in enumerate(a):                                                  # x: strand and rid 0 above the position; y: a span of 15 and some query position
            v[0] = (S["rev"] << 63) | (v[0] & 0xffffffff)
            v[1] = (15 << 32) | (qs + i)
        # regions of one read share its anchors: each region's as / as1 are shifted to where its anchors start
        regs[g]["as"] = len(cur_a)
        R["as1"] += len(cur_a)
        for k in range(item0, len(items)):
            items[k] = items[k][:2] + (items[k][2] + len(cur_a),) + items[k][3:]
        cur_a.extend(a)
        cur_qlen = max(cur_qlen, qe0 + 17)
        if (g + 1) % per_read == 0 or g == n - 1:
            b.extend(cur_a); b_off.append(len(b)); read_off.append(read_off[-1] + cur_qlen); u_off.append(g + 1)
            cur_a, cur_qlen = [], 0
    D = dict(opt=dict(opt), mat=mat, u_off=np.array(u_off, np.int64), regs=regs, b_off=np.array(b_off, np.int64), b=np.array(b, np.uint64).reshape(-1, 2),
             read_off=np.array(read_off, np.int64), aregs=aregs, items=np.array(items, M.ALN_ITEM_DTYPE).reshape(-1), tasks=np.array(tasks, M.KSW_TASK_DTYPE).reshape(-1),
             cig_off=np.array(cig_off, np.int64), res=np.array(res, M.KSW_RES_DTYPE).reshape(-1), cigar=np.array(cigar, np.uint32), zres=np.array(zres, M.ZDROP_RES_DTYPE).reshape(-1),
             pool=np.array(pool, np.uint8), specs=specs)
    return with_second(D)


def with_second(D, n_tasks2_cap=1 << 30):
    """the second list as the model makes it, and its ksw results from the specs"""
    S = M.second_pass(D["opt"], D["aregs"], D["items"], D["tasks"], D["zres"], D["pool"], D["mat"], n_tasks2_cap)
    res2 = np.zeros(len(S["tasks2"]), M.KSW_RES_DTYPE)
    cigar2 = np.full(int(S["cig_off2"][-1]), 0xfeedfac0, np.uint32)
    for k, s in enumerate(S["second_of"]):
        if s < 0:
            continue
        e = D["specs"][k]
        e = e["second"] if e is not None and e["second"] is not None else e
        assert e is not None, f"item {k} got a second pass the case did not plan"
        ql, tl = lens(e["words"])
        r = res2[s]
        r["n_cigar"] = len(e["words"]) if e["n_cigar"] is None else e["n_cigar"]
        r["zdropped"], r["reach_end"], r["score"], r["max"], r["status"] = e["zdropped"], e["reach_end"], e["score"], e["max"], e["status"]
        r["max_q"], r["max_t"], r["mqe_t"] = ql - 1, tl - 1, tl - 1
        c0, c1 = int(S["cig_off2"][s]), int(S["cig_off2"][s + 1])
        w = (e["words"] + [0xfeedfac0] * (c1 - c0))[:c1 - c0]
        cigar2[c0:c1] = w
    return dict(D, tasks2=S["tasks2"], cig_off2=S["cig_off2"], second_of=S["second_of"], res2=res2, cigar2=cigar2, second=S)


def model(D, variant=None, **caps):
    return M.assemble(D["opt"], D["u_off"], D["regs"], D["b_off"], D["b"], D["read_off"], D["aregs"], D["items"], D["cig_off"], D["res"], D["cigar"], D["zres"], D["second_of"],
                      D["cig_off2"], D["res2"], D["cigar2"], variant=variant, **caps)


def planted():
    """name -> region: one case per rule, and per wrong variant of cig_model.VARIANTS one on which it differs"""
    drop = lambda cig="30M", **kw: ez(cig, zdropped=1, **kw)
    P = {
        "both_ext": region([ez("50M2I40M"), ez("3D60M")], left=ez("20M1D5M"), right=ez("33M")),
        "no_left": region([ez("50M"), ez("2I60M")], right=ez("33M")),
        "no_right": region([ez("50M"), ez("2I60M")], left=ez("12M")),
        "left_reach_end": region([ez("50M")], left=ez("20M1D5M", reach_end=1), right=ez("9M", reach_end=1)),
        "ext_empty": region([ez("50M")], left=ez(""), right=ez("")),
        "merge": region([ez("50M"), ez("60M"), ez("2I8M")], left=ez("4M")),
        "no_merge": region([ez("50M2I"), ez("3D60M"), ez("8M")]),
        "inside_item": region([ez(words("5M") + words("6M") + words("2I")), ez("8M")]),   # two M words inside one item stay two words
        "run65": region([ez("10M") for _ in range(70)]),
        "drop_split": region([ez("50M", anchors=2), drop("30M", anchors=2), ez("9M", anchors=3), ez("9M", anchors=3)], left=ez("4M"), right=ez("7M")),
        "drop_no_split": region([ez("50M"), ez("40M"), drop("30M"), ez("9M")], right=ez("7M")),
        "drop_exact_min_cnt": region([ez("50M"), drop("30M"), ez("9M"), ez("9M")]),               # cnt1 - (j + 1) == min_cnt
        "drop_first": region([drop("30M"), ez("9M", anchors=4)], left=ez("4M")),
        "drop_last": region([ez("50M"), ez("40M"), drop("30M")], right=ez("7M")),
        "j_clamp": region([drop(""), ez("9M", anchors=5)]),                                         # max_t = -1: no anchor at or below rs - 1
        "j_eq": region([ez("50M", anchors=2), ez("40M", anchors=2), drop("30M", anchors=3), ez("9M", anchors=3)], pin_eq=True),
        "code1": region([ez("50M"), ez("3M", second=ez("40M1I9M"), score=1), ez("9M")]),
        "code2_split_inv": region([ez("50M"), ez("3M", second=drop("20M", code=2), code=2), ez("9M", anchors=4)]),
        "second_differs": region([ez("50M"), ez("17M", second=drop("20M", mx=55, score=-9), mx=99)]),
        "over_left": region([ez("50M")], left=ez(over=True), right=ez("7M")),
        "over_gap": region([ez("50M"), ez(over=True), ez("9M", anchors=4)], right=ez("7M")),
        "over_right": region([ez("50M")], left=ez("4M"), right=ez(over=True)),
        "rev": region([ez("50M2I40M"), ez("3D60M")], left=ez("20M"), right=ez("33M"), rev=1),
        "rev_drop": region([ez("50M"), drop("30M"), ez("9M", anchors=4)], left=ez("20M"), rev=1, pre=2, post=3),
        "bad_behind_cut": region([ez("50M"), drop("30M"), ez("9M", status=1), ez("9M", zstatus=1, anchors=3)], right=ez("7M", status=2)),
    }
    return P


# the planted case on which each wrong variant of the model differs
DIFFERS = {"no_boundary_merge": "merge", "merge_inside_items": "inside_item", "ext_score_for_max": "both_ext", "max_t_under_reach_end": "left_reach_end", "j_lt": "j_eq",
           "no_j_clamp": "j_clamp", "split_gt": "drop_exact_min_cnt", "right_behind_drop": "drop_last", "drop_score_for_max": "drop_split", "first_pass_ez": "second_differs",
           "zdrop_for_inv": "code2_split_inv", "no_strand_flip": "rev", "append_behind_drop": "drop_first"}


def planted_batch(names=None, per_read=3, opt=OPT):
    P = planted()
    names = [k for k in P if P[k] is not None] if names is None else names
    return names, build([P[k] for k in names], opt=opt, per_read=per_read)


def sr_batch():
    """sr: an ungapped item whose test gives 0, one whose test gives 1 (14 mismatches in a row: 14 * (2 + 8) > 100) with a second pass, one with a dropped second pass"""
    regs = [region([], left=ez("5M"), right=ez("6M"), sr=dict(n=150)),
            region([ez("150M", score=123)], left=ez("5M"), sr=dict(n=150, bad=(60, 14))),
            region([ez("70M", zdropped=1, mx=140)], right=ez("6M"), sr=dict(n=150, bad=(70, 14)), rev=1),
            region([], sr=dict(n=131, bad=(3, 9)))]
    return build(regs, opt=OPT_SR, per_read=2)


def limits(opt=OPT):
    """name -> batch: the sizes at which the kernels change steps"""
    out = {}
    rng = np.random.default_rng(11)
    # regions of 0 (cnt == 0), 1, 2, 63, 64, 65 and 129 items
    fills = lambda n: [ez(f"{3 + i % 5}M{1 + i % 2}{'ID'[i % 2]}{2 + i % 3}M") for i in range(n)]
    regs = [region([ez("7M")])] + [region(fills(n)) for n in (1, 2, 63, 64, 65, 129)] + [region(fills(n - 2), left=ez("4M"), right=ez("7M")) for n in (63, 64, 65, 129)]
    out["items"] = build(regs, opt=opt, per_read=4)
    out["items"]["aregs"][0] = np.zeros((), M.ALN_REG_DTYPE)                       # a region with cnt == 0 (:578)
    # appended CIGARs of 1, 255, 256 and 257 words (the gather's piece), from one item and from several
    mk = lambda n: words("".join(f"{2 + i % 7}{'MIMD'[i % 4]}" for i in range(n)))
    regs = [region([ez(mk(n))]) for n in (1, 255, 256, 257, 700)] + [region([ez(mk(100)), ez(mk(155)), ez(mk(1)), ez(mk(300))]), region([ez(mk(255)), ez("3I5M")]),
                                                                      region([ez(mk(127)), ez(mk(129)), ez("3M")])]
    out["words"] = build(regs, opt=opt, per_read=1)
    # merges across lanes 63 / 64, across a piece boundary, and a run longer than a piece (of items and of words)
    one = lambda n: [ez(f"{1 + i % 9}M") for i in range(n)]
    regs = [region([ez(mk(63)[:-1] + words("4M"))] + one(3)), region([ez(mk(255)[:-1] + words("4M"))] + one(3) + [ez("2I3M")]), region(one(300) + [ez("2I3M")] + one(5)),
            region([ez(mk(250))] + one(20) + [ez(mk(9))]), region(one(600)), region([ez("2I5M")] + one(255) + [ez("5M2D"), ez("3D")] + one(258))]
    out["merges"] = build(regs, opt=opt, per_read=2)
    # a drop at item 63 and at item 64 (with and without a left extension), j in the first and in the last anchor of a 129-anchor region
    d = lambda n, **kw: region([ez("6M") for _ in range(n)] + [ez("30M", zdropped=1)] + [ez("5M") for _ in range(3)], **kw)
    regs = [d(63), d(64), d(62, left=ez("4M")), d(63, left=ez("4M"), right=ez("5M")), d(127), d(128),
            region([ez("8M", zdropped=1, anchors=128)]), region([ez("6M", anchors=127), ez("30M", zdropped=1)]), region([ez("900M", zdropped=1, anchors=128)])]
    out["drops"] = build(regs, opt=opt, per_read=3)
    return out


# ---- reads for the reference's own mm_align1 (tests/golden/make_ref_cig_fixtures.py): the regions of tests/aln_data.py and, on top, regions planted so that the
# reference itself drops, splits, runs second passes, meets items over max_sw_mat in every position and appends long runs of one-word fills ----
def ref_opts():
    """the option sets of aln_data.OPTS, all with q != q2; asm20 gets zdrop != zdrop_inv, so that a second pass's zdrop argument tells code 2 from code 1 in every
    non-sr set"""
    import aln_data as AD
    O = {k: dict(v) for k, v in AD.OPTS.items()}
    O["asm20"]["zdrop_inv"] = 100
    assert all(o["q"] != o["q2"] and (o["flag"] & 1 or o["zdrop"] != o["zdrop_inv"]) for o in O.values())
    return O


def ref_batches():
    import aln_data as AD
    B = AD.batches()
    O = ref_opts()
    B = {name: (O[name], reads) for name, (_, reads) in B.items()}
    G = AD.genome()
    rng = np.random.default_rng(4242)

    def new(opt, name, rev=0):
        return AD.Read(name, rng, G, O[opt]["k"], rev)

    def mid(opt, name, rid, start, l1, n_junk, l2, rev=0, pos1=None, pos2=None, step=(20, 60), sub=0.02):
        """one region over two pieces of the contig with n_junk unrelated bases between them, in the read and in the contig alike: a diverging middle stretch"""
        r = new(opt, name, rev).junk(40)
        r.piece(rid, start, l1, at_pos=pos1, step=step, sub=sub, region=False)
        r.junk(n_junk)
        r.piece(rid, start + l1 + n_junk, l2, at_pos=pos2, step=step, sub=sub, region=False)
        r.regs.append((0, len(r.a), rid, 0, rev)); r.names.append(name)
        B[opt][1].append(r.junk(40).done())

    for opt in ("ont", "asm20"):
        mid(opt, "cig_drop_split", 5, 2000, 1500, 900, 1500)
        mid(opt, "cig_drop_split_rev", 6, 3000, 1500, 900, 1500, rev=1)
        mid(opt, "cig_drop_nosplit", 3, 2000, 1500, 900, 160, pos2=[40, 110])
        mid(opt, "cig_drop_nosplit_rev", 3, 6000, 1500, 900, 160, rev=1, pos2=[40, 110])
        mid(opt, "cig_drop_first", 5, 8000, 60, 900, 1800, pos1=[30])
        mid(opt, "cig_drop_last", 6, 9000, 1800, 900, 60, pos2=[40])
        mid(opt, "cig_drop_twice", 6, 20000, 1200, 900, 1200)                   # its child drops again: a second level
    # the split test at its edge (three and four anchors behind the drop, min_cnt = 3) and an anchor that ends on the last matching base (x == rs + max_t unless the
    # junk happens to go on matching)
    for n in (3, 4):
        mid("ont", "cig_split_eq%d" % n, 5, 14000 + 3000 * n, 1500, 900, 260, pos2=[40, 110, 170, 230][:n], sub=0.0)
    for j in range(6):
        mid("ont", "cig_j_eq%d" % j, 5, 24000 + 2600 * j, 1000, 900, 900, pos1=[14 + 58 * t for t in range(17)] + [999], sub=0.0)
    r = new("ont", "cig_drop_twice2").junk(40)
    r.piece(6, 30000, 1200, region=False).junk(900).piece(6, 32100, 1200, region=False).junk(900).piece(6, 34200, 1200, region=False)
    r.regs.append((0, len(r.a), 6, 0, 0)); r.names.append("cig_drop_twice2")
    B["ont"][1].append(r.junk(40).done())
    # the read ends with the last anchor.  Without sr the last fill ends k / 2 in front of it (mm_adjust_minier), so a right extension of k / 2 bases is made all the
    # same; under sr the fill ends behind the anchor and there is none
    B["ont"][1].append(new("ont", "cig_read_end").junk(40).piece(5, 12000, 1000, sub=0.0, at_pos=[14 + 41 * t for t in range(24)] + [999]).done())
    B["sr"][1].append(new("sr", "cig_sr_no_right").junk(5).piece(1, 2300, 150, sub=0.0, at_pos=[29 + 10 * t for t in range(13)]).done())
    # a perfect match: every fill is one M word, 70 of them and more merge into one
    for rev in (0, 1):
        r = new("ont", "cig_run%d" % rev, rev).junk(30).piece(6, 40000 + 50 * rev, 15000, sub=0.0, at_pos=[14 + 100 * t for t in range(149)]).junk(30)
        B["ont"][1].append(r.done())
    # max_sw_mat = 200 * 200: extensions over it on both sides; a fill over it in the middle; one as the first fill (max_t = -1: the j clamp)
    pos = [14 + 100 * t for t in range(13)]
    B["ont_sw"][1].append(new("ont_sw", "cig_over_ext").junk(450).piece(2, 6500, 1300, sub=0.0, at_pos=pos).junk(450).done())
    B["ont_sw"][1].append(new("ont_sw", "cig_over_ext_rev", 1).junk(450).piece(2, 8000, 1300, sub=0.0, at_pos=pos).junk(450).done())
    B["ont_sw"][1].append(new("ont_sw", "cig_over_gap").junk(10).piece(2, 9500, 1900, sub=0.0, at_pos=[14 + 100 * t for t in range(7)] + [914 + 100 * t for t in range(9)]).junk(10).done())
    B["ont_sw"][1].append(new("ont_sw", "cig_over_first").junk(10).piece(2, 3000, 1900, sub=0.0, at_pos=[14] + [314 + 100 * t for t in range(14)]).junk(10).done())
    return B


_REF = {}


def cached_ref_batches():
    if "b" not in _REF:
        _REF["b"] = ref_batches()
    return _REF["b"]
