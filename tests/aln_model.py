"""A NumPy / Python restatement of DESIGN 3.19: final regions -> the ksw tasks mm_align1 (align.c:565-771) issues when no task drops, the items, cig_off and the
sequence pool, in the plan's own layout.  run(opt, ref, csr arrays, cig_shift, variant=None) -> dict of the plan's output arrays; `variant` names one deliberately
wrong rule (VARIANTS), each of which tests/test_cpu_aln_model.py requires to differ on a named planted case."""
import numpy as np

REG_DTYPE = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0")] +
                     [("flags", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("p", "<u8")])
ALN_REG_DTYPE = np.dtype([(n, "<i4") for n in ("as1", "cnt1", "rs", "qs", "re", "qe", "rs0", "qs0", "re0", "qe0", "n_items", "n_tasks", "status", "rev")] +
                         [(n, "<i8") for n in ("item0", "task0", "cig0", "q_off", "t_off", "left_off")])
ALN_ITEM_DTYPE = np.dtype([(n, "<i4") for n in ("reg", "kind", "anchor", "rs", "re", "qs", "qe", "task", "score", "reserved")])
KSW_TASK_DTYPE = np.dtype([("q_off", "<i8"), ("t_off", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"), ("w", "<i4"), ("zdrop", "<i4"), ("end_bonus", "<i4"), ("flag", "<i4")])
LONG_JOIN, IGNORE, TANDEM, SELF = 1 << 40, 1 << 41, 1 << 42, 1 << 43
LEFT, GAP, RIGHT, UNGAPPED, OVER = 0, 1, 2, 3, 16
REFUSED, TOO_BIG, OVER_CAP = 1, 2, 3
F_SR, F_NO_END_FLT, F_SPLICE, I_HPC = 1, 2, 4, 1
EXTZ_ONLY, RIGHT_ALIGN, REV_CIGAR, APPROX_MAX = 0x40, 0x02, 0x80, 0x08
VARIANTS = ("fix_ends_ignores_long_join", "max_ext_cnt_off_by_one", "flush_only_at_end", "rs0_without_final_min", "nearby_counts_ge", "bw1_not_widened", "tandem_skips_last",
            "target_word_aligned", "hpc_walk_to_zero", "max_stretch_ge")


def lo(v):
    v &= 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def span(y):
    return y >> 32 & 0xff


def r16(n):
    return (n + 15) & ~15


def cdiv(a, b):
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def gap_at(a, i):
    return lo((a[i][1] - a[i - 1][1]) - (a[i][0] - a[i - 1][0]))


def long_gaps(a, as1, cnt1, min_gap):
    K = [i for i in range(1, cnt1) if not -min_gap <= gap_at(a, as1 + i) <= min_gap]
    return K if len(K) > 1 else None


def filter_bad_seeds(a, as1, cnt1, min_gap, diff_thres, max_ext_len, max_ext_cnt, variant):
    K = long_gaps(a, as1, cnt1, min_gap)
    if K is None:
        return
    n, mx, max_st, max_en, k = len(K), 0, -1, -1, 0
    if variant == "max_ext_cnt_off_by_one":
        max_ext_cnt -= 1
    while True:
        if k == n or (k >= max_en and variant != "flush_only_at_end"):
            if max_en > 0:
                for i in range(K[max_st], K[max_en]):
                    a[as1 + i][1] |= IGNORE
            mx, max_st, max_en = 0, -1, -1
            if k == n:
                break
        n_ins = n_del = max_diff = 0
        max_diff_l = -1
        i = K[k]
        gap = gap_at(a, as1 + i)
        if gap > 0:
            n_ins += gap
        else:
            n_del -= gap
        qs, rs = lo(a[as1 + i - 1][1]), lo(a[as1 + i - 1][0])
        l = k + 1
        while l < n and l <= k + max_ext_cnt:
            j = K[l]
            if lo(a[as1 + j][1]) - qs > max_ext_len or lo(a[as1 + j][0]) - rs > max_ext_len:
                break
            gap = gap_at(a, as1 + j)
            if gap > 0:
                n_ins += gap
            else:
                n_del -= gap
            diff = n_ins + n_del - abs(n_ins - n_del)
            if max_diff < diff:
                max_diff, max_diff_l = diff, l
            l += 1
        if max_diff > diff_thres and max_diff > mx:
            mx, max_st, max_en = max_diff, k, max_diff_l
        k += 1


def filter_bad_seeds_alt(a, as1, cnt1, min_gap, max_ext):
    K = long_gaps(a, as1, cnt1, min_gap)
    if K is None:
        return
    n, k = len(K), 0
    while k < n:
        i = K[k]
        gap1 = abs(gap_at(a, as1 + i))
        re1, qe1 = lo(a[as1 + i][0]), lo(a[as1 + i][1])
        l = k + 1
        while l < n:
            j = K[l]
            if lo(a[as1 + j][1]) - qe1 > max_ext or lo(a[as1 + j][0]) - re1 > max_ext:
                break
            gap2 = abs(gap_at(a, as1 + j))
            sp = span(a[as1 + j - 1][1])
            rs2, qs2 = lo(a[as1 + j - 1][0]) + sp, lo(a[as1 + j - 1][1]) + sp
            if min(rs2 - re1, qs2 - qe1) > gap1 + gap2:
                break
            re1, qe1, gap1 = lo(a[as1 + j][0]), lo(a[as1 + j][1]), gap2
            l += 1
        if l > k + 1:
            end = K[l - 1]
            for j in range(K[k], end):
                a[as1 + j][1] |= IGNORE
            a[as1 + end][1] |= LONG_JOIN
        k = l


def fix_bad_ends(r_as, r_cnt, mlen, a, bw, min_match, variant):
    as1, cnt1 = r_as, r_cnt
    if r_cnt < 3:
        return as1, cnt1
    honour = variant != "fix_ends_ignores_long_join"
    m = l = span(a[r_as][1])
    for i in range(r_as + 1, r_as + r_cnt - 1):
        if honour and a[i][1] & LONG_JOIN:
            break
        lr, lq = lo(a[i][0]) - lo(a[i - 1][0]), lo(a[i][1]) - lo(a[i - 1][1])
        mn, mx = min(lr, lq), max(lr, lq)
        if mx - mn > l >> 1:
            as1 = i
        l += mn
        m += min(mn, span(a[i][1]))
        if l >= bw << 1 or (m >= min_match and m >= bw) or m >= mlen >> 1:
            break
    cnt1 = r_as + r_cnt - as1
    m = l = span(a[r_as + r_cnt - 1][1])
    for i in range(r_as + r_cnt - 2, as1, -1):
        if honour and a[i + 1][1] & LONG_JOIN:
            break
        lr, lq = lo(a[i + 1][0]) - lo(a[i][0]), lo(a[i + 1][1]) - lo(a[i][1])
        mn, mx = min(lr, lq), max(lr, lq)
        if mx - mn > l >> 1:
            cnt1 = i + 1 - as1
        l += mn
        m += min(mn, span(a[i + 1][1]))
        if l >= bw << 1 or (m >= min_match and m >= bw) or m >= mlen >> 1:
            break
    return as1, cnt1


def adjust_minier(o, v, fwd, ref, rid, variant=None):
    """mm_adjust_minier (:350-365) -> (r, q); the HPC form walks the query homopolymer down to i > 0 as written, the target one down to the contig's first base"""
    if not o["idx_flag"] & I_HPC:
        return lo(v[0]) - (o["k"] >> 1), lo(v[1]) - (o["k"] >> 1)
    n = len(fwd)
    base = (lambda i: (3 - int(fwd[n - 1 - i]) if fwd[n - 1 - i] < 4 else 4)) if v[0] >> 63 else (lambda i: int(fwd[i]))
    y = lo(v[1])
    c, i, stop = base(y), y - 1, -1 if variant == "hpc_walk_to_zero" else 0
    while i > stop and base(i) == c:
        i -= 1
    q = i + 1
    off, _, S = ref
    get = lambda p: int(S[p >> 3]) >> ((p & 7) << 2) & 0xf
    off0 = int(off[rid]); at = off0 + lo(v[0])
    ct, j = get(at), at - 1
    while j >= off0 and get(j) == ct:
        j -= 1
    return lo(v[0]) + 1 - (at - j), q


def max_stretch(r_as, cnt, a, variant=None):
    """mm_max_stretch (:495-521): the first stretch of anchors on one diagonal with the strictly largest score"""
    if cnt < 2:
        return r_as, cnt
    max_score, max_i, max_len = -1, -1, 0
    score, ln = span(a[r_as][1]), 1
    for i in range(r_as + 1, r_as + cnt + 1):
        if i < r_as + cnt:
            lr, lq, sp = lo(a[i][0]) - lo(a[i - 1][0]), lo(a[i][1]) - lo(a[i - 1][1]), span(a[i][1])
            if lq == lr:
                score += min(lq, sp); ln += 1
                continue
        if score > max_score or (variant == "max_stretch_ge" and score >= max_score):
            max_score, max_len, max_i = score, ln, i - ln
        if i < r_as + cnt:
            score, ln = sp, 1
    return max_i, max_len


def plan_region(o, r, a, qlen, n_seq, ref_len, variant=None, slot_words=1 << 30, lds_gaps=2048, fwd=None, ref=None):
    """-> (status, dict of the region's scalars or None, [item tuples (kind, anchor, rs, re, qs, qe, w, zdrop, end_bonus, flag)]).  Writes the flags into a."""
    is_sr = bool(o["flag"] & F_SR)
    if o["flag"] & F_SPLICE or (is_sr and o["idx_flag"] & I_HPC):                       # :575
        return REFUSED, None, []
    cnt, r_as = int(r["cnt"]), int(r["as"])
    if cnt == 0:
        return 0, None, []
    if cnt < 0 or r_as < 0 or r_as + cnt > len(a):
        return REFUSED, None, []
    a0, aN = a[r_as], a[r_as + cnt - 1]
    key, rid = a0[0] >> 32, a0[0] >> 32 & 0x7fffffff
    if rid >= n_seq:
        return REFUSED, None, []
    tlen = int(ref_len[rid])
    for i in range(r_as, r_as + cnt):
        x, y = lo(a[i][0]), lo(a[i][1])
        if a[i][0] >> 32 != key or x < 0 or x >= tlen or y < 0 or y >= qlen or (i > r_as and (x < lo(a[i - 1][0]) or y < lo(a[i - 1][1]))):
            return REFUSED, None, []
    as1, cnt1 = max_stretch(r_as, cnt, a, variant) if is_sr else (r_as, cnt) if o["flag"] & F_NO_END_FLT else fix_bad_ends(r_as, cnt, int(r["mlen"]), a, o["bw"], o["min_chain_score"] * 2, variant)
    if cnt1 <= 0:
        return REFUSED, None, []
    rs, qs = adjust_minier(o, a[as1], fwd, ref, rid, variant)
    re, qe = adjust_minier(o, a[as1 + cnt1 - 1], fwd, ref, rid, variant)
    if is_sr:                                                                            # :584-587
        aL = a[as1 + cnt1 - 1]
        rs, qs, re, qe = lo(a[as1][0]) + 1 - span(a[as1][1]), lo(a[as1][1]) + 1 - span(a[as1][1]), lo(aL[0]) + 1, lo(aL[1]) + 1
    if is_sr:                                                                            # :613-620
        ext = lambda l: l + (cdiv(l * o["a"] + o["end_bonus"] - o["q"], o["e"]) if l * o["a"] + o["end_bonus"] > o["q"] else 0)
        qs0, qe0 = 0, qlen
        rs0 = max(rs - ext(qs), 0)
        re0 = min(re + ext(qlen - qe), tlen)
    else:
        rs0, qs0 = lo(a0[0]) + 1 - span(a0[1]), lo(a0[1]) + 1 - span(a0[1])
        rs0 = max(rs0, 0)
        if qs0 < 0:
            return REFUSED, None, []
        rs1 = qs1 = l = 0
        i = r_as - 1
        while i >= 0 and a[i][0] >> 32 == key:
            x, y = lo(a[i][0]) + 1 - span(a[i][1]), lo(a[i][1]) + 1 - span(a[i][1])
            if x < rs0 and y < qs0:
                l += 1
                if l > o["min_cnt"] or (variant == "nearby_counts_ge" and l >= o["min_cnt"]):
                    l = max(rs0 - x, qs0 - y)
                    rs1, qs1 = max(rs0 - l, 0), qs0 - l
                    break
            i -= 1
        if qs > 0 and rs > 0:
            l = min(qs, o["max_gap"])
            qs1 = max(qs1, qs - l)
            qs0 = min(qs0, qs1)
            l += cdiv(l * o["a"] - o["q"], o["e"]) if l * o["a"] > o["q"] else 0
            l = min(l, o["max_gap"], rs)
            rs1 = max(rs1, rs - l)
            rs0 = min(rs0, rs1)
            if variant != "rs0_without_final_min":
                rs0 = min(rs0, rs)
        else:
            rs0, qs0 = rs, qs
        re0, qe0 = lo(aN[0]) + 1, lo(aN[1]) + 1
        re1, qe1, l = tlen, qlen, 0
        i = r_as + cnt
        while i < len(a) and a[i][0] >> 32 == key:
            x, y = lo(a[i][0]) + 1, lo(a[i][1]) + 1
            if x > re0 and y > qe0:
                l += 1
                if l > o["min_cnt"] or (variant == "nearby_counts_ge" and l >= o["min_cnt"]):
                    l = max(x - re0, y - qe0)
                    re1, qe1 = re0 + l, qe0 + l
                    break
            i += 1
        if qe < qlen and re < tlen:
            l = min(qlen - qe, o["max_gap"])
            qe1 = min(qe1, qe + l)
            qe0 = max(qe0, qe1)
            l += cdiv(l * o["a"] - o["q"], o["e"]) if l * o["a"] > o["q"] else 0
            l = min(l, o["max_gap"], tlen - re)
            re1 = min(re1, re + l)
            re0 = max(re0, re1)
        else:
            re0, qe0 = re, qe
    if a0[1] & SELF:
        r_qs, r_qe, r_rs, r_re = int(r["qs"]), int(r["qe"]), int(r["rs"]), int(r["re"])
        me = abs(r_qs - r_rs)
        if r_rs - rs0 > me:
            rs0 = r_rs - me
        if r_qs - qs0 > me:
            qs0 = r_qs - me
        me = abs(r_qe - r_re)
        if re0 - r_re > me:
            re0 = r_re + me
        if qe0 - r_qe > me:
            qe0 = r_qe + me
    if not re0 > rs0 or qs0 < 0 or rs0 < 0 or qs0 > qs or rs0 > rs or qe > qe0 or re > re0 or qe0 > qlen or re0 > tlen:
        return REFUSED, None, []
    n10 = 0 if is_sr else sum(1 for i in range(1, cnt1) if not -10 <= gap_at(a, as1 + i) <= 10)
    if n10 > lds_gaps and n10 > slot_words:
        return TOO_BIG, None, []
    if is_sr and qe - qs != re - rs:                                                    # :725
        return REFUSED, None, []
    if not is_sr:
        filter_bad_seeds(a, as1, cnt1, 10, 40, o["max_gap"] >> 1, 10, variant)
        filter_bad_seeds_alt(a, as1, cnt1, 30, o["max_gap"] >> 1)
    R = dict(as1=as1, cnt1=cnt1, rs=rs, qs=qs, re=re, qe=qe, rs0=rs0, qs0=qs0, re0=re0, qe0=qe0, rev=a0[0] >> 63, rid=rid)
    items = []
    split_inv = int(r["flags"]) >> 24 & 1
    crs, cqs = rs, qs
    if qs > 0 and rs > 0:
        items.append((LEFT, as1, rs0, rs, qs0, qs, o["bw_ext"], o["zdrop_inv"] if split_inv else o["zdrop"], o["end_bonus"], EXTZ_ONLY | RIGHT_ALIGN | REV_CIGAR))
    if is_sr:                                                                            # :724-731: the ungapped fill of the whole stretch, no ksw task
        items.append((UNGAPPED, as1 + cnt1 - 1, rs, re, qs, qe, 0, 0, 0, 0))
    for i in range(1, 0 if is_sr else cnt1):
        y = a[as1 + i][1]
        last = i == cnt1 - 1
        if y & (IGNORE | TANDEM) and (not last or variant == "tandem_skips_last"):
            continue
        e_r, e_q = adjust_minier(o, a[as1 + i], fwd, ref, rid, variant)
        if last or y & LONG_JOIN or (e_q - cqs >= o["min_ksw_len"] and e_r - crs >= o["min_ksw_len"]):
            bw1 = max(e_q - cqs, e_r - crs) if y & LONG_JOIN and variant != "bw1_not_widened" else o["bw_ext"]
            items.append((GAP, as1 + i, crs, e_r, cqs, e_q, bw1, o["zdrop"], -1, APPROX_MAX))
            crs, cqs = e_r, e_q
    if qe < qe0 and re < re0:
        items.append((RIGHT, as1 + cnt1 - 1, re, re0, qe, qe0, o["bw_ext"], o["zdrop"], o["end_bonus"], EXTZ_ONLY))
    return 0, R, items


def unpack(S, off, ref_len, rid, st, en, variant=None):
    """mm_idx_getseq (index.c:152-162)"""
    o0 = int(off[rid])
    if variant == "target_word_aligned":
        o0 &= ~7
    p = np.arange(o0 + st, o0 + en, dtype=np.int64)
    return (S[p >> 3] >> ((p & 7) << 2).astype(np.uint32) & 0xf).astype(np.uint8)


def run(opt, ref, u_off, regs, b_off, b, read_off, reads, cig_shift=0, variant=None, caps=None, slot_words=1 << 30):
    """the plan on one batch.  ref = (offset, len, S); b uint64 [n, 2].  Returns dict(aln_regs, items, tasks, cig_off, pool, b (with flags), totals).  caps = (items,
    tasks, pool) marks regions beyond them OVER_CAP and writes nothing of theirs.  The pool's unwritten bytes are 0xff."""
    off, ref_len, S = ref
    o = dict(opt)
    o.setdefault("bw_ext", int(o["bw"] * 1.5 + 1.))
    n_reads, n_regs = len(u_off) - 1, int(u_off[-1])
    A = [[[int(x), int(y)] for x, y in b[b_off[r]:b_off[r + 1]]] for r in range(n_reads)]
    aregs = np.zeros(n_regs, ALN_REG_DTYPE)
    per = []
    for r in range(n_reads):
        qlen = int(read_off[r + 1] - read_off[r])
        for g in range(int(u_off[r]), int(u_off[r + 1])):
            st, R, items = plan_region(o, regs[g], A[r], qlen, len(ref_len), ref_len, variant, slot_words, fwd=reads[read_off[r]:read_off[r + 1]], ref=ref)
            per.append((r, st, R, items))
    def strand_of(r, rev):
        fwd = reads[read_off[r]:read_off[r + 1]]
        return np.where(fwd[::-1] < 4, 3 - fwd[::-1], 4).astype(np.uint8) if rev else fwd
    it = tk = cig = pool_at = 0
    items_out, tasks_out, chunks = [], [], []
    for g, (r, st, R, items) in enumerate(per):
        ar = aregs[g]
        ar["status"] = st
        if R is None:
            continue
        for f in ("as1", "cnt1", "rs", "qs", "re", "qe", "rs0", "qs0", "re0", "qe0", "rev"):
            ar[f] = R[f]
        left = R["qs"] > 0 and R["rs"] > 0
        nq, nt, nlq, nlt = R["qe0"] - R["qs0"], R["re0"] - R["rs0"], (R["qs"] - R["qs0"]) if left else 0, (R["rs"] - R["rs0"]) if left else 0
        q_off = pool_at; t_off = q_off + r16(nq); left_off = t_off + r16(nt)
        pool_n = r16(nq) + r16(nt) + r16(nlq) + r16(nlt)
        mine_i, mine_t, c0, i0, t0 = [], [], cig, it, tk
        for (kind, anchor, irs, ire, iqs, iqe, w, zd, eb, fl) in items:
            ql, tl = iqe - iqs, ire - irs
            if kind == UNGAPPED:
                sq, tq = strand_of(r, R["rev"])[iqs:iqe].astype(np.int64), unpack(S, off, ref_len, R["rid"], irs, ire, variant).astype(np.int64)
                sc = int(np.where((sq >= 4) | (tq >= 4), o["e2"], np.where(sq == tq, o["a"], -o["b"])).sum())
                mine_i.append((g, kind, anchor, irs, ire, iqs, iqe, -1, sc, 0))
                it += 1
                continue
            over = o["max_sw_mat"] > 0 and tl * ql > o["max_sw_mat"]
            mine_i.append((g, kind | (OVER if over else 0), anchor, irs, ire, iqs, iqe, -1 if over else tk, 0, 0))
            it += 1
            if over:
                continue
            if kind == LEFT:
                qo, to = left_off, left_off + r16(nlq)
            else:
                qo, to = q_off + (iqs - R["qs0"]), t_off + (irs - R["rs0"])
            mine_t.append((qo, to, ql, tl, w, zd, eb, fl))
            tk += 1
            cig += min(ql + tl, ((ql + tl) >> cig_shift) + 16)
        ar["n_items"], ar["n_tasks"], ar["item0"], ar["task0"], ar["cig0"], ar["q_off"], ar["t_off"], ar["left_off"] = len(mine_i), len(mine_t), i0, t0, c0, q_off, t_off, left_off
        pool_at += pool_n
        if caps is not None and (it > caps[0] or tk > caps[1] or pool_at > caps[2]):
            ar["status"] = OVER_CAP
            continue
        items_out.append((i0, mine_i)); tasks_out.append((t0, mine_t))
        # the pool: spans, then the reversed left copies; padding is code 4
        fwd = reads[read_off[r]:read_off[r + 1]]
        strand = np.where(fwd[::-1] < 4, 3 - fwd[::-1], 4).astype(np.uint8) if R["rev"] else fwd
        tspan = unpack(S, off, ref_len, R["rid"], R["rs0"], R["re0"], variant)
        seg = np.full(pool_n, 4, np.uint8)
        seg[:nq] = strand[R["qs0"]:R["qe0"]]
        seg[r16(nq):r16(nq) + nt] = tspan
        if left:
            lo_ = r16(nq) + r16(nt)
            seg[lo_:lo_ + nlq] = strand[R["qs0"]:R["qs"]][::-1]
            seg[lo_ + r16(nlq):lo_ + r16(nlq) + nlt] = tspan[:nlt][::-1]
        chunks.append((q_off, seg))
    n_items_cap = caps[0] if caps else it
    n_tasks_cap = caps[1] if caps else tk
    pool_cap = caps[2] if caps else pool_at
    items_a = np.full(n_items_cap * ALN_ITEM_DTYPE.itemsize, 0xff, np.uint8).view(ALN_ITEM_DTYPE)
    tasks_a = np.full(n_tasks_cap * KSW_TASK_DTYPE.itemsize, 0xff, np.uint8).view(KSW_TASK_DTYPE)
    cig_a = np.full((n_tasks_cap + 1) * 8, 0xff, np.uint8).view(np.int64)
    pool = np.full(pool_cap, 0xff, np.uint8)
    for i0, rows in items_out:
        for j, row in enumerate(rows):
            items_a[i0 + j] = row
    for t0, rows in tasks_out:
        for j, row in enumerate(rows):
            tasks_a[t0 + j] = row
    # cig_off is written per task at its own index; the entry behind the last task holds the total if it fits
    for g, (r, st, R, items) in enumerate(per):
        ar = aregs[g]
        if R is None or ar["status"] != 0:
            continue
        c = int(ar["cig0"])
        for j in range(int(ar["n_tasks"])):
            cig_a[int(ar["task0"]) + j] = c
            t = tasks_a[int(ar["task0"]) + j]
            s = int(t["qlen"]) + int(t["tlen"])
            c += min(s, (s >> cig_shift) + 16)
    if tk <= n_tasks_cap:
        cig_a[tk] = cig
    for q_off, seg in chunks:
        pool[q_off:q_off + seg.size] = seg
    bb = np.array([xy for rd in A for xy in rd], np.uint64).reshape(-1, 2)
    return dict(aln_regs=aregs, items=items_a, tasks=tasks_a, cig_off=cig_a, pool=pool, b=bb, totals=(it, tk, cig, pool_at))


def fnv(s):
    h = 2166136261
    for c in bytes(s):
        h = ((h ^ c) * 16777619) & 0xffffffff
    return h - (1 << 32) if h & 0x80000000 else h


def task_records(out, g):
    """the planned calls of region g as the fixture records them: [qlen, tlen, w, zdrop, end_bonus, flag, hash_q, hash_t] per task, and the kinds of ALL its items"""
    ar = out["aln_regs"][g]
    rows = []
    for j in range(int(ar["task0"]), int(ar["task0"]) + int(ar["n_tasks"])):
        t = out["tasks"][j]
        q = out["pool"][int(t["q_off"]):int(t["q_off"]) + int(t["qlen"])]
        tt = out["pool"][int(t["t_off"]):int(t["t_off"]) + int(t["tlen"])]
        rows.append([int(t["qlen"]), int(t["tlen"]), int(t["w"]), int(t["zdrop"]), int(t["end_bonus"]), int(t["flag"]), fnv(q), fnv(tt)])
    kinds = [int(k) for k in out["items"]["kind"][int(ar["item0"]):int(ar["item0"]) + int(ar["n_items"])]]
    return rows, kinds


def fixture_mismatches(name, out, fx, names):
    """regions of option set `name` whose plan disagrees with the reference's record (tests/golden/ref_aln.npz): as1 / cnt1, the anchor flags afterwards, and the calls.
    A region that ran to its end: its calls equal the planned tasks one for one; a dropped one: the planned list's prefix up to and including the dropped task; one
    with a gap item over max_sw_mat (the reference sets zdropped there, :323-325, and makes no call): the tasks in front of that item."""
    bad = []
    calls, call_off, ends, dropped = fx[name + "_calls"], fx[name + "_call_off"], fx[name + "_ends"], fx[name + "_dropped"]
    assert list(fx[name + "_names"]) == list(names)
    if not np.array_equal((out["b"][:, 1] >> np.uint64(40)).astype(np.uint8), fx[name + "_flags"]):
        bad.append("<anchor flags>")
    for g, nm in enumerate(names):
        ar = out["aln_regs"][g]
        rows, kinds = task_records(out, g)
        rec = calls[call_off[g]:call_off[g + 1], :8].tolist()
        if GAP | OVER in kinds:
            cut = kinds.index(GAP | OVER)
            rows = rows[:sum(1 for k in kinds[:cut] if not k & OVER)]
        elif dropped[g]:
            ok = len(rec) >= 1 and len(rec) <= len(rows)
            rows = rows[:len(rec)] if ok else None
        if ar["status"] != 0 or (int(ar["as1"]), int(ar["cnt1"])) != tuple(int(v) for v in ends[g][:2]) or rows != rec:
            bad.append(nm)
        elif UNGAPPED in kinds and not dropped[g] and int(ends[g][2]) != -(1 << 31):
            # the ungapped score has no call of its own: it is the region's dp_score less the extensions' maxima (:700, 762, 774; an extension without a CIGAR adds nothing)
            full = calls[call_off[g]:call_off[g + 1]]
            it = out["items"][int(ar["item0"]):int(ar["item0"]) + int(ar["n_items"])]
            if int(it["score"][kinds.index(UNGAPPED)]) != int(ends[g][2]) - sum(int(c[8]) for c in full if c[17] > 0):
                bad.append(nm + " <ungapped score>")
    return bad
