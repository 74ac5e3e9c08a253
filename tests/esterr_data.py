"""The cases of the chain-anchor divergence tests (mm_est_err map.c:357, esterr.c; csrc/chain_esterr.hip), made again deterministically wherever they are needed.
A case is a case of mapq_data ({"name", "hash", "qlen", "u", "a", "hit", "mapq", "rep_len"}: chains with their anchors) plus "mini_pos" (uint64: q_span << 32 | q_pos,
ascending) and "ref_len" (uint32 per reference sequence).  tests/golden/ref_esterr.npz holds what the reference's own hit.o and esterr.o make of them
(tests/golden/make_ref_esterr_fixtures.py): the final regions with div and the final a[].

ERead(name, qlen, ref_len) is a mapq_data.Read; .walk(fpos, ...) adds a chain given by the FORWARD query positions of its anchors in walk order (esterr.c:55: for
a reverse chain the walk runs from the back of a[]), so a case says directly what the walk meets.  .minis(...) sets mini_pos: by default every anchor position of
every chain with its span, minus `drop`, plus `extra`.  Chains of a read lie 100000 apart on the reference, so nothing joins unless a case asks for it (it then
uses Read.chain, whose gaps join under the default options)."""
import numpy as np

from mapq_data import Read, SPAN

SLICE = 4096                                                                   # ERR_SLICE of csrc/chain_esterr.h: the anchors of one workgroup step
LEAD = 60                                                                      # anchors in front of the long region of a slice case: no wave and no slice starts with it
_CASES = None


class ERead(Read):
    def __init__(self, name, qlen=100000, ref_len=(10000000,), **kw):
        super().__init__(name, qlen=qlen, **kw)
        self.ref_len, self.mini = np.array(ref_len, np.uint32), None
        self.n_walks = 0

    def walk(self, fpos, score=None, rev=0, rid=0, spans=SPAN, x0=None, flip=()):
        """fpos: forward query positions in walk order; flip: walk indices whose anchor carries the other strand bit than the chain's first"""
        fpos = np.asarray(fpos, np.int64)
        n = fpos.size
        spans = np.broadcast_to(np.asarray(spans, np.int64), (n,)).copy()
        bit = np.full(n, rev, np.int64)
        bit[list(flip)] ^= 1
        y = np.where(bit == 1, self.qlen - 1 - fpos + spans - 1, fpos)          # get_for_qpos backwards
        if rev:
            y, spans, bit = y[::-1], spans[::-1], bit[::-1]
        x = (1000 + 100000 * self.n_walks if x0 is None else x0) + 20 * np.arange(n)
        a = np.zeros((n, 2), np.uint64)
        a[:, 0] = (bit.astype(np.uint64) << np.uint64(63)) | (np.uint64(rid) << np.uint64(32)) | x.astype(np.uint64)
        a[:, 1] = (spans.astype(np.uint64) << np.uint64(32)) | (y.astype(np.uint64) & np.uint64(0xffffffff))
        self.chains.append((int(5000 - 7 * self.n_walks if score is None else score), a))
        self.n_walks += 1
        return self

    def anchor_minis(self):
        """(forward position, span) of every anchor of every chain"""
        out = []
        for _, a in self.chains:
            for ax, ay in a:
                ax, ay = int(ax), int(ay)
                span, y = (ay >> 32) & 0xff, ay & 0xffffffff
                out.append((self.qlen - 1 - (y + 1 - span) if ax >> 63 else y, span))
        return out

    def minis(self, drop=(), extra=(), only=None):
        seen = {}
        for pos, span in (self.anchor_minis() if only is None else list(only)) + [(p, s) for p, s in extra]:
            if pos not in drop and 0 <= pos < (1 << 31):
                seen.setdefault(int(pos), int(span))
        self.mini = np.array([(s << 32) | p for p, s in sorted(seen.items())], np.uint64)
        return self

    def case(self):
        if self.mini is None:
            self.minis()
        c = super().case()
        c["mini_pos"], c["ref_len"] = self.mini, self.ref_len
        return c


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    C = []
    add = lambda r: C.append(r.case())
    P = lambda n, lo=1000, step=50: lo + step * np.arange(n)                   # n forward positions
    # ---- trivial sizes ----
    add(ERead("no_mini").walk(P(5)).minis(only=[]))
    add(ERead("no_regions").minis(only=[(500, 15), (900, 15)]))
    add(ERead("one_mini_cnt1").walk([1000]))
    add(ERead("one_mini_absent").walk([1000]).minis(only=[(2000, 15)]))
    add(ERead("cnt1").walk([1500]).minis(extra=[(1000, 15), (2000, 15)]))
    # ---- search edges ----
    add(ERead("first_absent").walk(P(5)).minis(drop=[1000]))
    add(ERead("first_at_0").walk(P(5)).minis(extra=[(3000, 15)]))
    add(ERead("first_at_n_minus_1_cnt1").walk([5000]).minis(extra=[(1000, 15), (2000, 15)]))
    add(ERead("first_at_n_minus_1_rest_absent").walk([5000, 5100, 5200]).minis(drop=[5100, 5200], extra=[(1000, 15)]))
    # ---- every anchor matched ----
    add(ERead("all_matched_extras_between").walk(P(6)).minis(extra=[(1010, 15), (1060, 15), (1070, 15), (1240, 15), (1300, 15)]))
    # ---- where the walk stops ----
    add(ERead("middle_absent").walk(P(7)).minis(drop=[1150]))
    add(ERead("middle_absent_extras").walk(P(7)).minis(drop=[1150], extra=[(1020, 15), (1160, 15), (1290, 15)]))
    add(ERead("last_absent").walk(P(5)).minis(drop=[1200]))
    add(ERead("second_absent").walk(P(5)).minis(drop=[1050]))
    add(ERead("j_reaches_n").walk([1000, 1050, 9000, 9050]).minis(drop=[9000]))
    add(ERead("repeated_position").walk([1000, 1050, 1050, 1100, 1150]))
    add(ERead("decreasing_position").walk([1000, 1100, 1050, 1150, 1200]))
    add(ERead("decreasing_below_first").walk([1000, 900, 1050]))
    # ---- strand ----
    add(ERead("reverse").walk(P(6), rev=1).minis(extra=[(1020, 15)]))
    add(ERead("reverse_middle_absent").walk(P(6), rev=1).minis(drop=[1100]))
    add(ERead("both_strands").walk(P(6)).walk(P(5, 4000), rev=1).minis(drop=[4100], extra=[(1120, 15)]))
    add(ERead("reverse_spans_15_19").walk(P(6), rev=1, spans=[15, 19, 15, 19, 19, 15]))
    add(ERead("reverse_spans_15_19_forward_twin").walk(P(6), spans=[15, 19, 15, 19, 19, 15]))
    add(ERead("anchor_strand_differs").walk(P(6), flip=[2, 3]))                 # the anchors' own bits turn positions 2 and 3; r->rev says forward
    add(ERead("anchor_strand_differs_rev").walk(P(6), rev=1, flip=[1]))
    # ---- flank tests: a lone anchor of span 10 among minimizers that set avg_k ----
    def flank(name, qs, rs, tail_q, tail_r, other, a_span=10, cnt=1):
        """one region with qs, rs, qlen - qs = tail_q and l_ref - re = tail_r; `other`: spans of the other minimizers (in front of position 0 there is none:
        they lie behind the region)"""
        f0 = qs + a_span - 1
        fp = f0 + 40 * np.arange(cnt)
        qlen = qs + tail_q
        x0 = rs + a_span - 1
        re = x0 + 20 * (cnt - 1) + 1
        r = ERead(name, qlen=qlen, ref_len=(re + tail_r,)).walk(fp, spans=a_span, x0=x0)
        r.minis(extra=[(int(fp[-1]) + 1 + k, s) for k, s in enumerate(other)])
        add(r)
    flank("all_matched_no_flanks", 5, 5, 200, 3, [], a_span=15, cnt=5)          # n_match == n_tot: 0.0f
    for d in (-1, 0, 1):                                                        # avg_k = 15: spans 10 and 20
        flank(f"flank_qs_{15 + d}", 15 + d, 100, 100, 100, [20])
        flank(f"flank_rs_{15 + d}", 100, 15 + d, 100, 100, [20])
        flank(f"flank_qtail_{15 + d}", 5, 5, 15 + d, 100, [20])
        flank(f"flank_rtail_{15 + d}", 5, 5, 100, 15 + d, [20])                # ref_len at re + avg_k - 1, + 0, + 1
    for qs in (15, 16):
        flank(f"avg_int_all15_qs{qs}", qs, 100, 5, 5, [15, 15], a_span=15)
        flank(f"avg_15_333_qs{qs}", qs, 100, 5, 5, [15, 16], a_span=15)         # (15 + 15 + 16) / 3 = 15.333334f
        flank(f"avg_15_5_qs{qs}", qs, 100, 5, 5, [16], a_span=15)               # 15.5
    # qlen - qs = 52 > 15 but qlen - qe = 2: the second flank counts only because the reference reads qs
    flank("qs_not_qe", 5, 5, 52, 100, [20], cnt=2)
    # ---- reference sequences ----
    add(ERead("two_rids", ref_len=(1000 + 20 * 4 + 1 + 5, 101000 + 20 * 4 + 1 + 50)).walk(P(5)).walk(P(5, 4000), rid=1))
    # ---- after a join ----
    j = ERead("joined", qlen=40000, ref_len=(10000000, 1, 2, 2000000)).chain(3000).chain(100, 900, 900, 4, at=(900000, 1000), rid=3).chain(2900)
    add(j.minis(extra=[(700, 15), (12500, 15)]))
    j = ERead("joined_rev", qlen=40000, rev=1).chain(3000).chain(2900)
    add(j.minis(extra=[(20000, 15)], drop=[j.anchor_minis()[7][0]]))
    add(ERead("unsqueezed_as_nonzero", qlen=40000, ref_len=(10000000, 1, 2, 2000000)).chain(100, 900, 900, 4, at=(900000, 1000), rid=3)
        .chain(3000, 1000, 1000, 7, at=(60000, 1000)).minis(extra=[(1500, 15)]))
    # ---- many regions ----
    for n in (128, 129):
        r = ERead(f"regions{n}", qlen=400000, ref_len=(20000000, 14000000))
        for k in range(n):
            r.walk(P(3 + k % 3, 2000 * k + 500, 40), rev=k % 2, rid=k % 2, x0=1000 + 100000 * ((k * 37) % n))
        add(r.minis(drop=[2000 * k + 540 for k in range(0, n, 5)], extra=[(2000 * k + 555, 15) for k in range(0, n, 3)]))
    # ---- wave and slice edges ----
    for n in (63, 64, 65):
        add(ERead(f"cnt{n}").walk(P(n, 1000, 20)).minis(extra=[(1010, 15)]))
        add(ERead(f"minis{n}").walk(P(n - 2, 1000, 20)).minis(extra=[(500, 15), (990, 15)]))
    # failing lanes in two neighbouring waves of one region, away from any slice edge: the per-wave minimum and the per-region atomicMin meet
    add(ERead("wave_missing_63_64_65").walk(P(200, 1000, 20)).minis(drop=[1000 + 20 * k for k in (63, 64, 65)]))
    add(ERead("wave_missing_64_130").walk(P(200, 1000, 20)).minis(drop=[1000 + 20 * k for k in (64, 130)]))
    add(ERead("wave_missing_130_64_rev").walk(P(200, 1000, 20), rev=1).minis(drop=[1000 + 20 * k for k in (199 - 130, 199 - 64)]))
    for n in (SLICE - 1, SLICE, SLICE + 1):
        add(ERead(f"slice_cnt{n}", qlen=300000).walk(P(LEAD, 1000, 20)).walk(P(n, 100000, 20)).minis(extra=[(150007, 15)]))
    for at in (SLICE - 1, SLICE, SLICE + 1):                                    # the anchor at this position of the read's a[] is missing
        add(ERead(f"slice_missing_at{at}", qlen=300000).walk(P(LEAD, 1000, 20)).walk(P(SLICE + 200, 100000, 20)).minis(drop=[100000 + 20 * (at - LEAD)]))
    n = SLICE + 200                                                             # reverse: the anchor at position SLICE of a[] is walk index n - 1 - (SLICE - LEAD)
    add(ERead("slice_missing_at_rev", qlen=300000).walk(P(LEAD, 1000, 20)).walk(P(n, 100000, 20), rev=1).minis(drop=[100000 + 20 * (n - 1 - (SLICE - LEAD))]))
    # ---- libm sensitivity: n_tot large, one mismatch ----
    for n in (500, 1000, 2047, 3001):
        add(ERead(f"libm_{n}", qlen=300000).walk(P(n, 1000, 20)).minis(extra=[(1000 + 20 * (n // 2) + 7, 15)]))
    # ---- fractional avg_k under a pow: where (double)sum_k / n in place of the float shows, if it shows anywhere ----
    for n in (3, 5, 7, 11, 13, 17, 19, 23):
        add(ERead(f"avgk_frac_{n}").walk(P(n)).minis(extra=[(1010, 16)]))
    _CASES = C
    return C


def reference():
    """-> per case {"name", "case", "out": the reference's final regions (div included), "in": the same with div as mm_gen_regs leaves it (-1.0f, hit.c:83): what the
    mapq plan hands on, "a": the final a[], "libm"}"""
    import os
    from regs_model import REG
    Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_esterr.npz"))
    cs = cases()
    assert int(Z["reg_size"]) == REG.itemsize and [str(v) for v in Z["names"]] == [c["name"] for c in cs]
    out = []
    for k, c in enumerate(cs):
        w = Z["regs_out"][Z["out_off"][k]:Z["out_off"][k + 1]].reshape(-1).view(REG)
        r0 = w.copy()
        r0["div"] = -1.0
        out.append({"name": c["name"], "case": c, "out": w, "in": r0, "a": Z["a_out"][Z["a_off"][k]:Z["a_off"][k + 1]], "libm": str(Z["libm"])})
    return out
