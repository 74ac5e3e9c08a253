"""Seeded cases of the alignment-task plan (mm_align1, align.c:565-771): a small multi-contig genome whose contig lengths are no multiples of 8, packed
as mm_idx_t packs it; reads cut from it on both strands with substitutions and real indels; anchors along the true alignment (x = strand << 63 | rid << 32 | last
reference base, y = span << 32 | last read base on the anchors' strand), thinned, plus planted ones; regions over them with the fields the plan reads.
batches(): {option set name: (opt dict, [read])}; a read is dict(name, fwd uint8, a uint64 [n, 2], regs REG_DTYPE, names [one per region]).  Everything is made again
from the seeds; tests/golden/ref_aln.npz holds only what the reference made of it."""
import numpy as np

REG_DTYPE = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0")] +
                     [("flags", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("p", "<u8")])
LONG_JOIN, IGNORE, TANDEM, SELF = 1 << 40, 1 << 41, 1 << 42, 1 << 43
CONTIG_LENS = (3001, 5003, 12007, 20011, 999, 40013, 60013, 13, 4001)      # the last: planted homopolymers (HP_RUNS)
HP_RUNS = ((0, 20), (300, 2), (500, 20), (900, 2), (1500, 20), (2100, 2), (2500, 1))   # (start, length) in the last contig; a run's base differs from both neighbours

# option sets: the fields of mm2c_aln_opt_t that differ from map-ont (params.aln_opts) -- written out here so that the fixture does not depend on the package
BASE = dict(a=2, b=4, q=4, e=2, q2=24, e2=1, bw=500, min_chain_score=40, max_gap=5000, min_cnt=3, min_ksw_len=200, end_bonus=-1, zdrop=400, zdrop_inv=200, max_sw_mat=0, flag=0,
            idx_flag=0, k=15, sc_ambi=1)
OPTS = {
    "ont": dict(BASE),
    "asm20": dict(BASE, a=1, b=4, q=6, e=2, q2=26, e2=1, zdrop=200, zdrop_inv=200, k=19),
    "ont_noflt": dict(BASE, flag=2),                               # MM2C_ALN_F_NO_END_FLT
    "ont_g300": dict(BASE, max_gap=300),
    "ont_sw": dict(BASE, max_sw_mat=40000),
    "sr": dict(BASE, b=8, q=12, bw=100, min_chain_score=25, max_gap=100, min_cnt=2, end_bonus=10, zdrop=100, zdrop_inv=100, flag=1, k=21),   # the sr preset: MM2C_ALN_F_SR
    "hpc": dict(BASE, idx_flag=1, k=19),                           # map-pb: MM2C_ALN_I_HPC
}


def genome():
    rng = np.random.default_rng(20250)
    out = []
    for n in CONTIG_LENS:
        s = rng.integers(0, 4, n).astype(np.uint8)
        if n > 4000:                                               # a few ambiguous bases
            for p in rng.integers(100, n - 100, 3):
                s[p:p + int(rng.integers(1, 4))] = 4
        if n == 4001:
            for st, ln in HP_RUNS:
                s[st:st + ln] = 0
                s[st + ln] = 1
                if st:
                    s[st - 1] = 2
        out.append(s)
    return out


def pack(contigs):
    """offset uint64, len uint32, S uint32: the contigs one behind the other (index.c: offset = the bases before), 8 bases a word, base i in bits 4 (i & 7) on"""
    ln = np.array([c.size for c in contigs], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
    allb = np.concatenate(contigs).astype(np.uint32)
    pad = (-allb.size) % 8
    allb = np.concatenate([allb, np.zeros(pad, np.uint32)]).reshape(-1, 8)
    S = np.zeros(allb.shape[0], np.uint32)
    for j in range(8):
        S |= allb[:, j] << np.uint32(4 * j)
    return off, ln, S


def revcomp(s):
    return np.where(s[::-1] < 4, 3 - s[::-1], 4).astype(np.uint8)


def mutate(rng, ref, indels, sub):
    """ref piece -> (read piece, m): m[i] = index of reference base i in the read piece, -1 if deleted.  indels: sorted (pos, size): size > 0 inserts that many random
    bases in front of reference base pos, size < 0 deletes -size reference bases from pos on."""
    out, m, at, i = [], np.full(ref.size, -1, np.int64), 0, 0
    for pos, size in indels:
        seg = ref[i:pos].copy()
        m[i:pos] = at + np.arange(pos - i)
        out.append(seg); at += seg.size; i = pos
        if size > 0:
            out.append(rng.integers(0, 4, size).astype(np.uint8)); at += size
        else:
            i = min(ref.size, pos - size)
    seg = ref[i:].copy()
    m[i:] = at + np.arange(ref.size - i)
    out.append(seg)
    s = np.concatenate(out)
    hit = rng.random(s.size) < sub
    s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4 if hit.any() else s[hit]
    s[s > 4] = 4
    return s.astype(np.uint8), m


class Read:
    """a read on the anchors' strand, built piece by piece; anchors and regions in the order the pieces come"""

    def __init__(self, name, rng, G, k, rev=0):
        self.name, self.rng, self.G, self.k, self.rev = name, rng, G, k, rev
        self.s, self.a, self.regs, self.names = [], [], [], []
        self.at = 0

    def junk(self, n):
        self.s.append(self.rng.integers(0, 4, n).astype(np.uint8)); self.at += n
        return self

    def piece(self, rid, start, length, indels=(), sub=0.02, step=(20, 60), cnt=None, region=True, name=None, at_pos=None, split_inv=0):
        """ref[rid][start : start + length] with the indels; anchors at reference positions `at_pos` (piece coordinates of a k-mer's last base) or every `step` bases,
        thinned to `cnt` if given; they form a region unless region is False (then they are stray anchors the `nearby seeds` loops meet)"""
        k, rng = self.k, self.rng
        rev = self.rev
        s, m = mutate(rng, self.G[rid][start:start + length], sorted(indels), sub)
        if at_pos is None:
            at_pos, p = [], k - 1 + int(rng.integers(0, 8))
            while p < length:
                at_pos.append(p); p += int(rng.integers(step[0], step[1] + 1))
        pos = [p for p in at_pos if m[p] >= 0 and self.at + m[p] >= k - 1]
        if cnt is not None:
            assert len(pos) >= cnt, (self.name, len(pos), cnt)
            keep = np.sort(rng.choice(len(pos), cnt, replace=False)) if cnt > 2 else np.arange(cnt)
            pos = [pos[j] for j in keep]
        a0 = len(self.a)
        for p in pos:
            self.a.append([(rev << 63) | (rid << 32) | (start + p), (k << 32) | (self.at + int(m[p]))])
        if region and pos:
            self.regs.append((a0, len(pos), rid, split_inv, rev)); self.names.append(self.name if name is None else self.name + "/" + name)
        self.s.append(s); self.at += s.size
        return self

    def stray(self, rid, x, y, sp):
        """an anchor of no region, given outright"""
        self.a.append([(self.rev << 63) | (rid << 32) | x, (sp << 32) | y])
        return self

    def span(self, idx, sp):
        self.a[idx][1] = (self.a[idx][1] & ~(0xff << 32)) | (sp << 32)
        return self

    def flag(self, idx, bit):
        self.a[idx][1] |= bit
        return self

    def done(self):
        s = np.concatenate(self.s) if self.s else np.zeros(0, np.uint8)
        qlen = s.size
        a = np.array(self.a, np.uint64).reshape(-1, 2)
        regs = np.zeros(len(self.regs), REG_DTYPE)
        for g, (a0, cnt, rid, split_inv, rev) in enumerate(self.regs):
            x, y, k = a[a0:a0 + cnt, 0].astype(np.int64) & 0x7fffffff, a[a0:a0 + cnt, 1].astype(np.int64) & 0x7fffffff, self.k
            qs, qe = int(y[0]) + 1 - k, int(y[-1]) + 1
            r = regs[g]
            r["id"], r["cnt"], r["rid"], r["as"], r["parent"] = g, cnt, rid, a0, g
            r["rs"], r["re"] = int(x[0]) + 1 - k, int(x[-1]) + 1
            r["qs"], r["qe"] = (qlen - qe, qlen - qs) if rev else (qs, qe)
            r["mlen"] = r["blen"] = k + int(np.minimum(np.minimum(np.diff(x), np.diff(y)), k).sum())
            r["score"] = r["score0"] = r["mlen"]
            r["flags"] = (rev << 10) | (split_inv << 24)
        fwd = revcomp(s) if self.rev else s                          # the plan gets forward codes; the anchors of a read are all on one strand here
        return dict(name=self.name, fwd=np.ascontiguousarray(fwd), a=a, regs=regs, names=self.names)


def _indel_row(start, n, size, gap, alternate=True):
    return [(start + j * gap, size if (not alternate or j % 2 == 0) else -size) for j in range(n)]


def batches():
    G = genome()
    rng = np.random.default_rng(777)
    B = {name: (dict(o), []) for name, o in OPTS.items()}

    def new(opt, name, rev=0):
        r = Read(name, rng, G, OPTS[opt]["k"], rev)
        B[opt][1].append(r)
        return r

    # region sizes around the wave steps
    for cnt in (1, 2, 3, 63, 64, 65, 128, 129):
        new("ont", "cnt%d" % cnt, cnt & 1).junk(40).piece(5, 1000 + cnt, 40 * cnt + 300, cnt=cnt).junk(30)
    # long-gap counts around collect_long_gaps' `n <= 1` and one wave step
    for n in (0, 1, 2, 11, 12, 65):
        new("ont", "gaps%d" % n, n & 1).junk(25).piece(6, 2000, 120 * n + 900, indels=_indel_row(300, n, 14, 120), step=(25, 50)).junk(25)
    # mm_filter_bad_seeds: insertion / deletion pairs; a later, larger window overrides an earlier one or not
    for j, sizes in enumerate(((30, -30), (30, -30, 60, -60), (60, -60, 25, -25), (25, -30, 40, -45, 50, -20), (22, -22, 22, -22, 22, -22, 22, -22, 22, -22, 22, -22, 22, -22),
                               (12,) * 10 + (-60,))):      # the last: only the tenth gap on from the first makes a difference (max_ext_cnt)
        ind = [(400 + 90 * t, sz) for t, sz in enumerate(sizes)]
        new("ont", "fbs%d" % j).junk(30).piece(3, 500, 3000, indels=ind, step=(20, 40)).junk(30)
        new("ont_noflt", "fbs%d" % j, 1).junk(30).piece(3, 500, 3000, indels=ind, step=(20, 40)).junk(30)
    # mm_filter_bad_seeds_alt: chains of 1, 2 and 4 joins (insertions only, so the first filter sees no difference)
    for joins in (1, 2, 4):
        ind = [(600 + 70 * t, 45) for t in range(joins + 1)]
        new("ont", "alt%d" % joins).junk(30).piece(5, 3000, 2500, indels=ind, step=(20, 35)).junk(30)
    # an inbound LONG_JOIN at the second and at the second-to-last anchor, with an indel right behind / in front that mm_fix_bad_ends would trim at
    pos = [14 + 30 * t for t in range(40)]
    new("ont", "lj_second").junk(30).piece(3, 7000, 1300, indels=[(50, 40)], at_pos=pos).flag(1, LONG_JOIN).junk(30)
    new("ont", "lj_second_to_last").junk(30).piece(3, 7000, 1300, indels=[(14 + 30 * 36 + 8, -40)], at_pos=pos).flag(38, LONG_JOIN).junk(30)
    new("ont", "lj_none").junk(30).piece(3, 7000, 1300, indels=[(50, 40)], at_pos=pos).junk(30)
    # TANDEM on a middle and on the last anchor; SELF with the clamp
    new("ont", "tandem_mid").junk(30).piece(2, 3000, 1500, at_pos=[14 + 110 * t for t in range(13)]).flag(4, TANDEM).flag(5, TANDEM).junk(30)
    new("ont", "tandem_last").junk(30).piece(2, 3000, 1500, at_pos=[14 + 110 * t for t in range(13)]).flag(12, TANDEM).junk(30)
    new("ont", "self_left").junk(60).piece(2, 80, 1500).flag(0, SELF).junk(60)
    # the only way the final `rs0 < rs ? rs0 : rs` of :649 binds on a defined input: a first anchor whose span is below k / 2, more than min_cnt seeds right in front
    # of it, and mm_fix_bad_ends moving the start one base on across an insertion (so that qs0 stays in front of qs)
    r = new("ont", "short_span").junk(50)
    for _ in range(4):
        r.stray(2, 4013, 63, 5)
    r.piece(2, 4000, 900, sub=0.0, indels=[(15, 49)], at_pos=[14, 15] + [55 + 40 * t for t in range(18)]).span(4, 5).junk(40)
    # the contig's first and last bases: rs == 0 through the `rs0 < 0` clamp (x = k >> 1 gives rs = 0); a span ending at the contig's last base
    new("ont", "rs_zero").junk(50).piece(1, 0, 900, at_pos=[7] + [40 + 45 * t for t in range(18)]).junk(20)
    new("ont", "ctg_end").junk(20).piece(1, 5003 - 800, 800).junk(300)
    new("ont", "ctg_end_rev", 1).junk(20).piece(0, 3001 - 700, 700).junk(300)
    new("ont", "ctg_start_midword").junk(200).piece(4, 0, 999).junk(200)
    # max_gap binding on both sides and on the target side only (ont_g300: max_gap = 300; the target reach is never below the query's, :644, so the query alone cannot bind)
    new("ont_g300", "gapq").junk(900).piece(0, 100, 1200).junk(900)
    new("ont_g300", "gapt").junk(250).piece(3, 4000, 1200).junk(100)
    new("ont_g300", "gapqt", 1).junk(900).piece(3, 4000, 1200).junk(900)
    # nearby seeds: exactly min_cnt and min_cnt + 1 stray anchors in front and behind, on the same and on another x >> 32
    for n in (3, 4):
        new("ont", "near_front%d" % n).junk(30).piece(5, 8000, 60 * n + 20, at_pos=[20 + 50 * t for t in range(n)], region=False).junk(400).piece(5, 9000, 1000).junk(50)
        new("ont", "near_back%d" % n).junk(30).piece(5, 9000, 1000).junk(400).piece(5, 10500, 60 * n + 20, at_pos=[20 + 50 * t for t in range(n)], region=False).junk(50)
        new("ont", "near_other%d" % n).junk(30).piece(3, 8000, 60 * n + 20, at_pos=[20 + 50 * t for t in range(n)], region=False).junk(400).piece(5, 9000, 1000).junk(50)
    new("ont", "two_regions").junk(30).piece(5, 20000, 1500, name="a").junk(700).piece(5, 23000, 1500, name="b").junk(30)
    new("ont", "two_regions_rev", 1).junk(30).piece(5, 20000, 1500, name="a").junk(700).piece(5, 23000, 1500, name="b").junk(30)
    # rs0 at every residue of the packed position mod 8 (the test asserts that all eight occur)
    for j in range(8):
        new("asm20", "res%d" % j, j & 1).junk(33).piece(3, 9000 + j, 700).junk(33)
    # an item exactly at and one above max_sw_mat = 200 * 200 (ont_sw): anchors 100 apart, one single-base insertion
    new("ont_sw", "sw_at").junk(10).piece(2, 5000, 1300, sub=0.0, at_pos=[14 + 100 * t for t in range(12)]).junk(10)
    new("ont_sw", "sw_above").junk(10).piece(2, 5000, 1300, sub=0.0, indels=[(500, 1)], at_pos=[14 + 100 * t for t in range(12)]).junk(10)
    # the last LDS-class and the first scratch-class region: 2 048 and 2 049 long gaps (without the end filter, which would trim some of them away)
    for n in (2048, 2049):
        new("ont_noflt", "lg%d" % n).junk(20).piece(6, 1000, 26 * n + 400, indels=_indel_row(60, n, 12, 26), at_pos=[50 + 26 * t for t in range(n + 1)], sub=0.0).junk(20)
    # the prefix rule: 2 kb of unrelated sequence spliced in; a real inversion
    r = new("ont", "spliced_in").junk(30)
    r.piece(5, 30000, 3000, indels=[(1500, 2000)], sub=0.01).junk(30)
    r = new("ont", "inversion").junk(30)
    s0 = G[5][33000:33400]
    r.piece(5, 32000, 1000, name="x")
    # the inverted stretch belongs to the same region's read: the region's anchors go on behind it
    r.regs.pop(); r.names.pop()
    r.s.append(revcomp(s0)); r.at += s0.size
    a0 = 0
    r.piece(5, 33400, 1000, region=False)
    r.regs.append((a0, len(r.a), 5, 0, 0)); r.names.append("inversion")
    r.junk(30)
    # the HPC form of mm_adjust_minier: homopolymers of 1, 2 and 20 under the first and the last anchor (anchors inside the runs of the last contig); a run that reaches
    # the read's position 0 (the walk stops at i > 0, so q = 1) at the contig's first base (the target walk stops at the offset, so r = 0)
    new("hpc", "hp_q1_ctg0").piece(8, 0, 1200, sub=0.0, at_pos=[18] + [60 + 45 * t for t in range(24)]).junk(40)
    new("hpc", "hp_first20_last2").junk(40).piece(8, 450, 500, sub=0.0, at_pos=[65] + [110 + 30 * t for t in range(11)] + [451]).junk(40)          # 515 in the run at 500, 901 in the run at 900
    new("hpc", "hp_first2_last20", 1).junk(40).piece(8, 250, 1300, sub=0.0, at_pos=[51] + [100 + 40 * t for t in range(28)] + [1262]).junk(40)   # 301 in the run at 300, 1512 in the run at 1500
    new("hpc", "hp_first1_last1").junk(40).piece(8, 2080, 500, sub=0.0, at_pos=[21] + [60 + 40 * t for t in range(8)] + [420]).junk(40)            # 2101 is the second base of a run of 2; 2500 a run of 1
    for j in range(40):
        rd = new("hpc", "hrand%d" % j, j & 1).junk(int(rng.integers(0, 80)))
        for t in range(2):
            rid = int(rng.choice([2, 3, 5, 8]))
            L = int(rng.integers(200, 1200))
            rd.piece(rid, int(rng.integers(0, CONTIG_LENS[rid] - L)), L, indels=[(L // 2, int(rng.choice([-25, 14, 33])))], sub=0.01, step=(15, 60), name="r%d" % t).junk(int(rng.integers(0, 200)))
    # sr (mm_max_stretch): the longest stretch on one diagonal at the chain's start, middle and end, two stretches of equal score (the first wins), one anchor, two
    pos = [20 + 10 * t for t in range(12)]
    new("sr", "sr_start").junk(5).piece(1, 1000, 150, sub=0.0, indels=[(95, 1), (115, -1)], at_pos=pos).junk(5)
    new("sr", "sr_middle", 1).junk(5).piece(1, 1200, 150, sub=0.0, indels=[(45, 1), (115, -1)], at_pos=pos).junk(5)
    new("sr", "sr_end").junk(5).piece(1, 1400, 150, sub=0.0, indels=[(35, 1), (55, 2)], at_pos=pos).junk(5)
    new("sr", "sr_equal").junk(5).piece(1, 1600, 150, sub=0.01, indels=[(75, 1)], at_pos=pos).junk(5)
    new("sr", "sr_one").junk(5).piece(1, 1800, 150, at_pos=[60]).junk(5)
    new("sr", "sr_two", 1).junk(5).piece(1, 2000, 150, indels=[(70, 3)], at_pos=[50, 90]).junk(5)
    new("sr", "sr_n").junk(5).piece(5, int(np.nonzero(G[5] == 4)[0][0]) - 70, 150, sub=0.02, at_pos=pos).junk(5)       # an ambiguous base inside the ungapped fill
    new("sr", "sr_wave").junk(5).piece(3, 3000, 1500, sub=0.0, indels=[(400, 1), (1190, -1)], at_pos=[20 + 10 * t for t in range(140)]).junk(5)   # a stretch across the 64-anchor steps
    for j in range(60):
        L = int(rng.integers(100, 251))
        rid = int(rng.choice([1, 2, 3, 5]))
        ind = [(int(rng.integers(30, L - 30)), int(rng.choice([-2, -1, 1, 2])))] if j % 3 else []
        new("sr", "srand%d" % j, j & 1).junk(int(rng.integers(0, 12))).piece(rid, int(rng.integers(0, CONTIG_LENS[rid] - L)), L, indels=ind, sub=float(rng.choice([0.0, 0.01, 0.03])), step=(5, 30)).junk(int(rng.integers(0, 12)))
    # about a thousand random regions
    for j in range(330):
        opt = ("ont", "asm20", "ont_noflt", "ont_g300")[j % 4]
        rd = new(opt, "rand%d" % j, int(rng.integers(0, 2))).junk(int(rng.integers(0, 120)))
        for t in range(3):
            rid = int(rng.choice([0, 1, 2, 3, 5, 6]))
            L = int(rng.integers(150, 1500))
            st = int(rng.integers(0, CONTIG_LENS[rid] - L))
            n_ind = int(rng.integers(0, 5))
            ind = [(int(p), int(rng.choice([-60, -35, -20, -12, -3, 2, 11, 20, 33, 50]))) for p in np.sort(rng.choice(np.arange(40, L - 80, 70), min(n_ind, (L - 120) // 70), replace=False))] if L > 300 else []
            rd.piece(rid, st, L, indels=ind, sub=float(rng.choice([0.0, 0.01, 0.04])), step=(15, int(rng.integers(30, 120))), name="r%d" % t)
            rd.junk(int(rng.integers(0, 300)))
    out = {}
    for name, (o, reads) in B.items():
        out[name] = (o, [r.done() for r in reads])
    return out


_CACHE = {}


def cached_batches():
    if "b" not in _CACHE:
        _CACHE["b"] = batches()
    return _CACHE["b"]


def reference():
    if "g" not in _CACHE:
        _CACHE["g"] = pack(genome())
    return _CACHE["g"]


def csr(reads):
    """the arrays of one batch: u_off, regs, b_off, b, read_off, reads (forward codes), names"""
    u_off = np.concatenate([[0], np.cumsum([r["regs"].size for r in reads])]).astype(np.int64)
    b_off = np.concatenate([[0], np.cumsum([r["a"].shape[0] for r in reads])]).astype(np.int64)
    read_off = np.concatenate([[0], np.cumsum([r["fwd"].size for r in reads])]).astype(np.int64)
    regs = np.concatenate([r["regs"] for r in reads]) if reads else np.zeros(0, REG_DTYPE)
    b = np.concatenate([r["a"] for r in reads]) if reads else np.zeros((0, 2), np.uint64)
    fwd = np.concatenate([r["fwd"] for r in reads]) if reads else np.zeros(0, np.uint8)
    names = [n for r in reads for n in r["names"]]
    return u_off, regs, b_off, np.ascontiguousarray(b), read_off, np.ascontiguousarray(fwd), names
