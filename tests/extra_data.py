"""Seeded inputs for the extra plan (mm_update_extra and mm_test_zdrop, align.c): the inputs behind tests/golden/ref_extra.npz.  The fixture stores outputs only;
update_cases() and zdrop_cases() make the same inputs again, for the generator, the model's test and the GPU tests.
An update case is one call of mm_update_extra: query and target as codes 0..4 (already cut to the region), a CIGAR (uint32 words len << 4 | op), rev and a score
set; the generator and the tests run each with is_eqx 0 and 1.  A z-drop case is one call of mm_test_zdrop: query, target, CIGAR, score set; it runs under the two
threshold sets of ZD_THR."""
import os
import re

import numpy as np

import ksw_data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPS = "MIDN"
# a, b, q, e, sc_ambi: map-ont, asm20, sr, and one whose ambiguous bases score 0
SCORES = {"ont": (2, 4, 4, 2, 1), "asm20": (1, 4, 6, 2, 1), "sr": (2, 8, 12, 2, 1), "amb0": (2, 4, 4, 2, 0)}
# zdrop, zdrop_inv, max_gap, flag: map-ont's own (options.c), and a set tight enough that code 1 and the inversion test both occur
ZD_THR = ((400, 200, 5000, 0), (12, 6, 40, 0))
LDS_WORDS = 2048                      # MM2C_EXTRA_LDS_WORDS
RUN_LANE = 16                         # MM2C_EXTRA_RUN_LANE


def score_set(name):
    """(mat int8 [25], q, e, q2, e2) of a name of SCORES or of ksw_data.SCORES; q2, e2 are not read by the extra plan"""
    if name in SCORES:
        a, b, q, e, amb = SCORES[name]
        return ksw_data.gen_mat(a, b, amb), q, e, 24, 1
    return ksw_data.score_set(name)


def words(s):
    """'6M1I5M' -> uint32 words"""
    if isinstance(s, str):
        return np.array([int(n) << 4 | OPS.index(o) for n, o in re.findall(r"(\d+)([MIDN])", s)], np.uint32)
    return np.asarray(s, np.uint32)


def text(w):
    return "".join("%d%s" % (int(x) >> 4, "MIDN??? =X"[int(x) & 0xf] if int(x) & 0xf < 9 else "?") for x in w)


def seqs_for(rng, cig, mis=0.0):
    """a target of random bases and the query the CIGAR makes of it: M copied (a base changed with probability mis), I random, D and N passed over"""
    q, t = [], []
    for w in words(cig):
        op, n = int(w) & 0xf, int(w) >> 4
        seg = rng.integers(0, 4, n).astype(np.uint8)
        if op == 0:
            t.append(seg)
            qq = seg.copy()
            flip = rng.random(n) < mis
            qq[flip] = (qq[flip] + 1 + rng.integers(0, 3, int(flip.sum()))) % 4
            q.append(qq)
        elif op == 1:
            q.append(seg)
        else:
            t.append(seg)
    cat = lambda x: np.concatenate(x).astype(np.uint8) if x else np.zeros(0, np.uint8)
    return cat(q), cat(t)


def edit_region(rng, n_cols, gap_lo=8, gap_hi=13, mis=0.04, amb=0.002, repeat=0.6, runs=0.03):
    """An ONT-like region from a seeded edit script: M stretches of gap_lo .. gap_hi - 1 bases with mismatches, between them an insertion or a deletion that, with
    probability `repeat`, repeats the bases in front of it (so that it stands at the right end of its repeat and left alignment moves it), with probability `runs` an
    I and a D side by side.  -> (query, target, CIGAR words)"""
    q, t, cig = [], [], []

    def push(op, n):
        if cig and cig[-1][0] == op:
            cig[-1][1] += n
        else:
            cig.append([op, n])
    done = 0
    while True:
        n = int(rng.integers(gap_lo, gap_hi))
        kind = rng.random()
        if kind < 0.15:
            seg = np.full(n, rng.integers(0, 4))                 # a homopolymer
        elif kind < 0.3:
            seg = np.tile(rng.integers(0, 4, 2), n)[:n]          # a dinucleotide repeat
        else:
            seg = rng.integers(0, 4, n)
        seg = seg.astype(np.uint8)
        qq = seg.copy()
        flip = rng.random(n) < mis
        qq[flip] = (qq[flip] + 1 + rng.integers(0, 3, int(flip.sum()))) % 4
        qq[rng.random(n) < amb] = 4
        tt = seg.copy()
        tt[rng.random(n) < amb] = 4
        q.extend(qq); t.extend(tt); push(0, n); done += n
        if done >= n_cols:
            break
        k = int(min(rng.geometric(0.5), 8)) if rng.random() < 0.97 else int(rng.integers(20, 60))
        for op in ((1, 2) if rng.random() < runs else ((1,) if rng.random() < 0.5 else (2,))):
            own = q if op == 1 else t
            if rng.random() < repeat and len(own) >= k:
                seg = np.array(own[-k:], np.uint8)
            else:
                seg = rng.integers(0, 4, k).astype(np.uint8)
            own.extend(seg); push(op, k)
    return np.array(q, np.uint8), np.array(t, np.uint8), np.array([n << 4 | op for op, n in cig], np.uint32)


def _case(name, q, t, cig, sc="ont", rev=0):
    return dict(name=name, q=np.asarray(q, np.uint8), t=np.asarray(t, np.uint8), cigar=words(cig), sc=sc, rev=int(rev))


def update_planted():
    rng = np.random.default_rng(20261021)
    cs = []

    def add(name, q, t, cig, scs=("ont", "asm20", "sr", "amb0"), revs=(0,)):
        for sc in scs:
            for rev in revs:
                cs.append(_case("%s/%s/r%d" % (name, sc, rev), q, t, cig, sc, rev))

    def auto(name, cig, mis=0.0, **kw):
        q, t = seqs_for(rng, cig, mis)
        add(name, q, t, cig, **kw)
    Z = np.zeros

    def hp(name, cig, **kw):
        """both sequences one base throughout: every indel can move as far as its cap lets it"""
        ln, op = words(cig) >> 4, words(cig) & 0xf
        add(name, Z(int(ln[op <= 1].sum())), Z(int(ln[op != 1].sum())), cig, **kw)
    # n_cigar 0 .. 3, one empty word, one word I: the return of :97 comes before the leading-I/D step
    add("n0", [], [], "")
    auto("n1_M", "7M", 0.3)
    add("n1_0M", [], [], "0M")
    auto("n1_I", "5I")
    auto("n1_D", "4D")
    add("n1_0I", [], [], "0I")
    auto("n2_MI", "6M3I"); auto("n2_IM", "3I6M", revs=(0, 1)); auto("n2_DM", "2D6M", revs=(0, 1)); auto("n2_MM", "3M4M")
    auto("n3", "5M2I6M", 0.2); auto("n3_D", "5M2D6M", 0.2)
    # the issue's own example: an insertion at the right end of a repeat
    add("repeat_6M1I5M", [0, 1, 2, 3, 1, 1, 1, 2, 3, 0, 2, 0], [0, 1, 2, 3, 1, 1, 2, 3, 0, 2, 0], "6M1I5M")
    # an indel first and one last are never shifted; an indel between M and D is not either
    hp("indel_first_last", "2I4M2D4M2I2D")
    hp("indel_M_D", "4M2I2D4M"); hp("indel_M_I_D_M", "4M2I3D6M")
    # l == prev_len: the M in front becomes empty, is squeezed, and a leading indel appears and is stripped
    hp("lead_appears_I", "3M2I4M", revs=(0, 1)); hp("lead_appears_D", "3M3D4M", revs=(0, 1))
    hp("prev_eaten_merge", "2I3M2I4M3M")            # 2I 0M 2I 7M... the I words merge into the next
    # M I M I M: the second cap is reached only through the first shift
    hp("cap_through_shift", "4M1I2M2I4M"); hp("cap_through_shift_D", "4M2D2M2D4M")
    add("cap_through_shift_stop", [1] + [0] * 12, [1] + [0] * 9, "5M1I2M2I3M")
    # shifts around the lane's own walk and the wave's steps, in a homopolymer: RUN_LANE, 63, 64, 65, 16 + 64 k, > 256
    for n in (15, 16, 17, 63, 64, 65, 79, 80, 81, 143, 144, 145, 300):
        add("homo_shift_%d" % n, [1] + [0] * (n + 2 + 8), [1] + [0] * (n + 8), "%dM2I8M" % (n + 1), scs=("ont",))
        add("homo_shift_all_%d" % n, [0] * (n + 3 + 8), [0] * (n + 8), "%dM3I8M" % n, scs=("ont",), revs=(0, 1))
        add("homo_shift_D_%d" % n, [2] + [3] * (n + 8), [2] + [3] * (n + 2 + 8), "%dM2D8M" % (n + 1), scs=("ont",))
    # the 5I6D7I repair
    auto("run2_untouched", "5M2I3D5M", revs=(0, 1)); auto("run3", "5M2I3D1I5M"); auto("run4", "5M2I3D1I2D5M"); auto("run3_DID", "5M2D3I1D5M")
    add("run_zero_inside", *seqs_for(rng, "5M2I3D5M"), "5M2I0M3D0I5M"); add("run_zero_inside3", *seqs_for(rng, "5M3I3D5M"), "5M2I0M3D0D1I5M")
    add("run_zero_M_between", *seqs_for(rng, "5M2I3D4I5M"), "5M2I3D0M4I5M")
    auto("run_IID", "5M2I1I3D5M"); auto("run_IIDI", "5M2I1I3D2I5M"); auto("run_only_I", "5M2I1I3I5M")
    auto("N_then_M", "5M20N6M2I3D2I4M"); auto("N_D_I", "5M20N2D3I2D4M"); auto("I_N", "5M2I20N3D4M")
    auto("run_second_behind", "5M2I3D1I4M2D3I2D5M"); auto("run_second_behind_short", "5M2I3D1I4M2D3I5M"); auto("run_second_one_M", "4M1I2D1I1M2D1I2D4M")
    auto("run_at_end", "5M2I3D1I"); auto("run_at_end_short", "5M2I3D"); auto("run_at_start", "2I3D1I5M", revs=(0, 1)); auto("run_last_two", "5M2I1M3D2I")
    auto("run_all", "2I3D1I", revs=(0, 1))
    hp("run_after_shift", "3M2I0M2D2I5M")
    # N words, and ambiguous bases in M, I and D on either sequence
    auto("N_words", "6M30N7M2D100N4M", 0.2); auto("N_first", "10N6M"); auto("N_last", "6M10N")
    q, t = seqs_for(rng, "8M3I6M3D8M")
    q[2] = 4; t[3] = 4; q[9] = 4; t[15] = 4; q[20] = 4; t[20] = 4
    add("ambi", q, t, "8M3I6M3D8M")
    add("ambi_both", [4, 4, 0, 1, 4], [4, 0, 0, 4, 4], "5M"); add("ambi_all", [4] * 9, [4] * 8, "3M2I3M1D1M")
    # dp_max: clamps at 0 and recovers; a maximum in front of a long gap; a maximum in the last base
    q, t = seqs_for(rng, "40M")
    q[10:22] = (q[10:22] + 1) % 4
    add("dp_clamp_recover", q, t, "40M")
    auto("dp_max_before_gap", "30M60D3M"); auto("dp_max_before_ins", "30M90I3M")
    q, t = seqs_for(rng, "30M")
    q[:12] = (q[:12] + 2) % 4
    add("dp_max_last_base", q, t, "30M")
    add("dp_all_mismatch", Z(10), np.ones(10), "10M"); auto("dp_gap_first", "9I4M", revs=(0, 1))
    # EQX: all-match and all-mismatch M words, alternating single bases, N against N
    add("eqx_all_match", [0, 1, 2, 3], [0, 1, 2, 3], "4M"); add("eqx_all_mismatch", [0, 0, 0], [1, 1, 1], "3M")
    add("eqx_mismatch_words", [0, 0, 0, 2, 2, 1, 1], [0, 0, 0, 3, 3, 0, 2], "3M1I2M1D1M")     # every M word is one run: in place, `=` for a mismatch
    add("eqx_alternate", [0, 1, 0, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0], "7M"); add("eqx_alternate_x", [1, 0, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0], "6M")
    add("eqx_N_N", [0, 4, 4, 1], [0, 4, 4, 1], "4M"); add("eqx_N_A", [0, 4, 0, 1], [0, 0, 4, 1], "4M")
    auto("eqx_mixed", "9M2I7M2D30N8M", 0.3)
    # CIGARs of 63 .. 129 words, and on either side of the LDS class (MM2C_EXTRA_LDS_WORDS words at entry)
    for n in (63, 64, 65, 127, 128, 129, LDS_WORDS, LDS_WORDS + 1):
        cig = "".join("%d%s" % (3 + k % 4, "M" if k % 2 == 0 else "ID"[k // 2 % 2]) for k in range(n))
        q, t = seqs_for(rng, cig, 0.1)
        add("words_%d" % n, q, t, cig, scs=("ont",))
    return cs


def update_limits():
    """one region of 10^5 bases, and edit-script regions whose CIGARs lie on either side of the LDS class"""
    rng = np.random.default_rng(99)
    cs = []
    q, t, cig = edit_region(rng, 100000, 30, 70, mis=0.01, repeat=0.5)
    cs.append(_case("big_1e5", q, t, cig))
    q, t, cig = edit_region(rng, 12000, 8, 13)
    cs.append(_case("ont_12k", q, t, cig, rev=1))
    return cs


def update_randoms(n=2000):
    rng = np.random.default_rng(777)
    names = list(SCORES)
    cs = []
    for i in range(n):
        q, t, cig = edit_region(rng, int(rng.integers(10, 220)), int(rng.integers(1, 9)), int(rng.integers(9, 16)), mis=float(rng.choice([0.0, 0.05, 0.3])),
                                amb=float(rng.choice([0.0, 0.02])), repeat=float(rng.choice([0.3, 0.9])), runs=float(rng.choice([0.0, 0.2])))
        cs.append(_case("rnd%04d" % i, q, t, cig, str(rng.choice(names)), int(rng.integers(0, 2))))
    return cs


def update_from_ksw():
    """the CIGARs ksw_extd2 made (tests/golden/ref_ksw.npz) that consume both sequences whole: the function's real inputs"""
    fx = np.load(os.path.join(GOLDEN, "ref_ksw.npz"))
    off, cig = fx["cig_off"], fx["cigar"]
    cs = []
    for k, c in enumerate(ksw_data.cases()):
        if c["sc"] in ("ret", "mis12", "swap", "eeq", "asm5", "asm10") or k % 3:
            continue
        g = cig[off[k]:off[k + 1]]
        ln, op = g >> 4, g & 0xf
        if g.size and int(ln[op != 2].sum()) == c["q"].size and int(ln[op != 1].sum()) == c["t"].size:
            cs.append(_case("ksw/" + c["name"], c["q"], c["t"], g, c["sc"], k & 1))
    return cs


def zdrop_planted():
    rng = np.random.default_rng(5150)
    cs = []

    def add(name, q, t, cig, sc="ont"):
        cs.append(dict(name=name, q=np.asarray(q, np.uint8), t=np.asarray(t, np.uint8), cigar=words(cig), sc=sc))
    Z, O = (lambda n: [0] * n), (lambda n: [1] * n)

    def hp(name, cig, spare=0):
        ln, op = words(cig) >> 4, words(cig) & 0xf
        add(name, Z(int(ln[op <= 1].sum()) + spare), Z(int(ln[op != 1].sum()) + spare), cig)
    hp("none", "20M"); add("empty", Z(5), Z(5), "")
    add("deep_diag", Z(30) + O(20) + Z(10), Z(60), "60M")
    add("deep_off_diag", Z(30) + O(20) + Z(10), Z(70), "30M10D30M"); add("deep_off_diag_I", Z(30) + [2] * 12 + O(20) + Z(10), Z(60), "30M12I30M")
    add("max_tie_later_wins", Z(10) + [1, 1, 0, 0, 0, 0] + O(12), Z(28), "28M")      # score 20 at base 9 and again at base 15; the drop is measured from the later
    add("max_tie_gap", Z(10) + [1, 1, 0, 0, 0, 0] + O(12), Z(10) + [0, 0, 0, 0, 0, 0] + Z(7) + Z(12), "16M7D12M")
    add("two_equal_drops", Z(10) + O(3) + Z(30) + O(3) + Z(5), Z(51), "51M")         # 12 below the maximum twice: the earlier keeps it
    add("two_equal_drops_reset", Z(10) + O(3) + Z(6) + O(3) + Z(5), Z(27), "27M")
    add("drop_ends_in_gap", Z(20) + O(6), Z(20) + O(0) + Z(6) + Z(9), "26M9D"); add("drop_ends_in_ins", Z(20) + O(6) + Z(9), Z(26), "26M9I")
    hp("only_gaps", "4I5D5I7D"); hp("only_gaps_N", "4I30N10D")
    add("first_base_negative", O(1) + Z(12), Z(13), "13M"); hp("first_gap", "2I10M")
    add("all_negative", O(15), Z(15), "15M")
    hp("partial", "10M3D10M", spare=17)                                        # an extension: the CIGAR ends inside both sequences
    q, t = seqs_for(rng, "50M4I30M6D40M", 0.15)
    q[60:75] = 4
    add("ambi_stretch", q, t, "50M4I30M6D40M", sc="amb0")
    for n in (63, 64, 65, 129, LDS_WORDS, LDS_WORDS + 1):
        cig = "".join("%d%s" % (3 + k % 4, "M" if k % 2 == 0 else "ID"[k // 2 % 2]) for k in range(n))
        q, t = seqs_for(rng, cig, 0.25)
        add("words_%d" % n, q, t, cig)
    q, t, cig = edit_region(rng, 30000, 8, 13, mis=0.08)
    q[9000:9400] = rng.integers(0, 4, 400)
    add("ont_30k_bad_stretch", q, t, cig)
    return cs


def zdrop_from_ksw():
    """every case of tests/ksw_data.py with the CIGAR of tests/golden/ref_ksw.npz: the function's real inputs (score-only tasks have none)"""
    fx = np.load(os.path.join(GOLDEN, "ref_ksw.npz"))
    off, cig = fx["cig_off"], fx["cigar"]
    return [dict(name="ksw/" + c["name"], q=c["q"], t=c["t"], cigar=cig[off[k]:off[k + 1]], sc=c["sc"], ksw=k) for k, c in enumerate(ksw_data.cases())]


_CACHE = {}


def update_cases():
    if "u" not in _CACHE:
        _CACHE["u"] = update_planted() + update_limits() + update_from_ksw() + update_randoms()
    return _CACHE["u"]


def zdrop_cases():
    if "z" not in _CACHE:
        _CACHE["z"] = zdrop_planted() + zdrop_from_ksw()
    return _CACHE["z"]
