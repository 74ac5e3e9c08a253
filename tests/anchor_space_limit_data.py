"""Batch layouts for the two anchor-parallel kernels, mapq_gather (csrc/chain_mapq.hip) and err_walk (csrc/chain_esterr.hip), at the limits of their traversal of the
batch's b index space: slices of SLICE positions, lanes LANES apart with a memo of the hit / table entry found last, a grid of at most GRID_CAP workgroups that takes
positions from TURN on in a second turn, and the read-by-read path behind a refusal.

A read is an esterr_data.ERead (so also a mapq_data.Read): cases() gives every read of the module once, by name, and tests/golden/ref_mapq_limits.npz /
ref_esterr_limits.npz hold what the reference's own hit.o and esterr.o make of each (make_ref_mapq_fixtures.py / make_ref_esterr_fixtures.py with this module's name).
A layout is {"name", "reads": [names, in batch order], "b_off0": position of the batch's first anchor, "at": {"what", "read", "q", "p"} or None, "plants": [...],
"gpu_only"}: "at" names one anchor -- position q of read number `read` of the layout -- and p, the batch position it lands on, computed here from the lengths of the
reads in front of it.  A plant is (kernel, read, q, what the lane does there): "hit" or "miss" of its memo, "copy" (mapq: not a squeezed read) or "k0" (esterr: a
first walk anchor), which the trace of tests/anchor_space_model.py must show.

Filler reads fill<n> are one chain of n anchors with every minimizer present: one hit, so MAPQ_READ_COPY, and nothing fails in them.  All reads run under the default
options.  NAMED = 40 is the position inside its read of every named anchor of the slice-edge layouts, so three small fillers serve them all."""
import numpy as np

from esterr_data import ERead

SLICE, LANES, GRID_CAP = 4096, 256, 2048                                       # MAPQ_SLICE = ERR_SLICE, the workgroup, the grid cap of the two launchers
TURN = GRID_CAP * SLICE                                                        # 8 388 608: the first position of a workgroup's second turn
NAMED = 40
BIG_FILL = 3900
MEMO_SIZES = (255, 256, 257, 512, 513)
DROP4 = dict(score=100, ref_len=900, q_len=900, n=4, at=(900000, 1000), rid=3)  # a secondary of the chain over query 800..12800 that mm_select_sub drops
REFS = (10000000, 1, 2, 2000000)
_READS = None
_CASES = None
_LAYOUTS = None

P = lambda n, lo=1000, step=20: lo + step * np.arange(n)


def _make_reads():
    R = {}

    def add(r):
        assert r.name not in R
        R[r.name] = r
    E = lambda name, qlen=100000: ERead(name, qlen=qlen, ref_len=REFS)
    for n in (BIG_FILL, 155, 156, 157, 116, 117, 41):
        add(E(f"fill{n}", 300000).walk(P(n)))
    add(E("empty").minis(only=[(500, 15)]))
    # ---- the named anchors of the slice-edge layouts, each at position NAMED of its read ----
    add(E("absorbed").chain(3000, n=NAMED).chain(2900, n=40))                                           # joined: a[NAMED] carries MM_SEED_LONG_JOIN
    add(E("dropped").chain(3000, n=NAMED).chain(**DROP4).chain(2900, n=40, gap=(30000, 30000)))          # no join: from dst NAMED on src = dst + 4; 4 anchors of tail
    add(E("failing").walk(P(100)).minis(drop=[1000 + 20 * NAMED]))
    add(E("k0").walk(P(NAMED, 5000)).walk(P(60, 1000)))                         # the second region's first anchor lies BELOW its a[] neighbour: walked, it would fail
    add(E("rev_pred").walk(P(100), rev=1).minis(drop=[1000 + 20 * (99 - NAMED)]))                        # a[NAMED] is walk anchor 59; its predecessor is a[NAMED + 1]
    # ---- the lane memo inside a read ----
    for c in MEMO_SIZES:
        add(E(f"memo_join{c}").chain(3000, n=c).chain(2900, n=c))                                        # one region of 2c anchors, the flag at a[c]
        add(E(f"memo_adjoin{c}").chain(3000, n=c).chain(**DROP4).chain(2900, n=c, gap=(30000, 30000)))   # two hits that adjoin at dst c; src = dst + 4 behind it
        add(E(f"ewalk{c}").walk(P(c), rev=1).walk(P(c, 20000)))                                          # a reverse and a forward region that adjoin at a[c]
    # ---- the lane memo across reads ----
    add(E("hit300").chain(3000, n=300).chain(2900, n=40, gap=(30000, 30000)))                            # squeezed, hits (dst 0, cnt 300), (300, 40)
    add(E("drop4_front").chain(**DROP4).chain(3000, n=300, at=(60000, 800)).chain(2900, n=40, at=(102000, 42800)))   # squeezed: (src 4, dst 0, cnt 300), (304, 300, 40)
    add(E("copy_as4").chain(**DROP4).chain(3000, n=300, at=(60000, 800)))       # one hit with as = 4: copy state, the 4 anchors in front are copied too
    add(E("copy340").chain(3000, n=340))
    add(E("e_fwd").walk(P(300)).walk(P(40, 20000)))
    add(E("e_rev_other", 77777).walk(P(300, 50001), rev=1).walk(P(40, 70001)))  # another qlen, the other strand, positions that e_fwd's mini_pos does not hold
    add(E("e_k0", 88888).walk(P(300, 30001)).walk(P(40, 60001)))                # a[0] is k == 0, a[256] lies in the same region
    # ---- failures ----
    add(E("fail_a").walk(P(400)).minis(drop=[1000 + 20 * 395]))
    add(E("fail_b").walk(P(300)).minis(drop=[1000 + 20 * 3]))
    add(E("fail_2reg").walk(P(150)).walk(P(150, 20000)).minis(drop=[1000 + 20 * 140, 20000 + 20 * 5]))   # a[140] and a[155]: two regions' failures in one wave
    return R


def reads():
    """-> {name: ERead}"""
    global _READS
    if _READS is None:
        _READS = _make_reads()
    return _READS


def cases():
    """every read of the module once, as the case dicts of esterr_data (what the fixture generators run)"""
    global _CASES
    if _CASES is None:
        _CASES = [r.case() for r in reads().values()]
    return _CASES


def length(name):
    """the anchors of a read's input a[]"""
    return sum(a.shape[0] for _, a in reads()[name].chains)


def b_off(layout):
    return np.concatenate([[0], np.cumsum([length(n) for n in layout["reads"]])]).astype(np.int64) + int(layout["b_off0"])


def _layout(name, rs, at=None, plants=(), b_off0=0, gpu_only=False):
    L = {"name": name, "reads": list(rs), "b_off0": b_off0, "at": None, "plants": list(plants), "gpu_only": gpu_only}
    if at is not None:
        what, k, q = at
        L["at"] = {"what": what, "read": k, "q": q, "p": int(b_off(L)[k]) + q}
    return L


SECOND_TURN = ["fill3900", "absorbed", "dropped", "memo_join513", "rev_pred", "failing", "memo_adjoin512", "ewalk257", "hit300", "drop4_front", "fill3900", "e_fwd",
               "e_rev_other", "e_k0", "memo_join256", "ewalk512", "empty", "copy_as4", "fail_2reg", "memo_adjoin257", "fill3900", "absorbed"]
SECOND_TURN_B_OFF0 = TURN - 6000
SECOND_TURN_CAP = TURN + 4 * SLICE
BY_READ = ["memo_join256", "hit300", "fail_a", "fail_b", "drop4_front", "memo_adjoin512", "ewalk512", "fail_2reg"]
BY_READ_CAP = 2 * SLICE + 1                                                    # three workgroups for eight reads
BY_READ_REFUSALS = {"offset": 7, "hit": 5}                                     # b_off[8] beyond n_b_cap refuses read 7; a hit's as beyond the read's anchors refuses read 5


def layouts():
    global _LAYOUTS
    if _LAYOUTS is not None:
        return _LAYOUTS
    Ls = []
    # ---- slice edges: [fill3900, a small filler, the read of interest, a read behind it] ----
    named = (("absorbed", "mapq: the flagged first anchor of an absorbed chain"), ("dropped", "mapq: the first anchor behind a dropped secondary"),
             ("failing", "esterr: a failing anchor"), ("k0", "esterr: a region's first walk anchor"), ("rev_pred", "esterr: reverse region, the predecessor is a[q + 1]"))
    for at in (SLICE - 1, SLICE, SLICE + 1):
        small = at - BIG_FILL - NAMED
        for rd, what in named:
            Ls.append(_layout(f"edge_{rd}_{at}", [f"fill{BIG_FILL}", f"fill{small}", rd, "fill41"], at=(what, 2, NAMED)))
        Ls.append(_layout(f"edge_last_{at}", [f"fill{BIG_FILL}", f"fill{small}", "fill41", "dropped"], at=("mapq: the last anchor of a read", 2, 40)))
    # ---- a read boundary at exactly SLICE, with e empty reads on it, in front of the batch and behind it; batches that end at SLICE, SLICE + 1, 2 * SLICE ----
    for e in (0, 1, 2):
        Ls.append(_layout(f"boundary_empty{e}", ["empty"] * e + [f"fill{BIG_FILL}", "fill116", "absorbed"] + ["empty"] * e + ["dropped", "fill41"] + ["empty"] * e,
                          at=("the first anchor behind the boundary", e + 3 + e, 0)))
    Ls.append(_layout(f"end_{SLICE}", [f"fill{BIG_FILL}", "fill116", "absorbed"], at=("the batch's last anchor", 2, 79)))
    Ls.append(_layout(f"end_{SLICE + 1}", [f"fill{BIG_FILL}", "fill117", "absorbed"], at=("the batch's last anchor", 2, 79)))
    Ls.append(_layout(f"end_{2 * SLICE}", [f"fill{BIG_FILL}", "fill116", "absorbed"] * 2, at=("the batch's last anchor", 5, 79)))
    # ---- the lane memo inside a read: the read starts the batch, so lane t visits q = t, t + 256, t + 512, ... ----
    inside = {255: [(256, "miss")], 256: [(256, "miss")], 257: [(256, "hit")], 512: [(256, "hit"), (512, "miss")], 513: [(256, "hit"), (512, "hit"), (768, "miss")]}
    # (the reverse region's first walk anchor is its LAST a[] anchor, c - 1; the forward region's is c)
    walks = {255: [(254, "k0"), (255, "k0"), (256, "miss")], 256: [(255, "k0"), (256, "k0")], 257: [(256, "k0"), (257, "k0")], 512: [(256, "hit"), (511, "k0"), (512, "k0")],
             513: [(256, "hit"), (512, "k0"), (513, "k0"), (768, "miss")]}
    for c in MEMO_SIZES:
        pl = inside[c]
        Ls.append(_layout(f"memo_join{c}", [f"memo_join{c}"], at=("the flagged anchor", 0, c), plants=[("mapq", 0, q, o) for q, o in pl] + [("mapq", 0, c, "miss")]))
        Ls.append(_layout(f"memo_adjoin{c}", [f"memo_adjoin{c}"], at=("src = dst + 4 begins", 0, c), plants=[("mapq", 0, q, o) for q, o in pl] + [("mapq", 0, c, "miss")]))
        Ls.append(_layout(f"ewalk{c}", [f"ewalk{c}"], at=("the forward region's k == 0", 0, c), plants=[("esterr", 0, q, o) for q, o in walks[c]]))
    # ---- the lane memo across reads: the first read is 340 long, so lane 84 goes from q = 84 of it to q = 0 of the next and lane 85 to q = 1 ----
    Ls.append(_layout("across_sq_sq", ["hit300", "drop4_front"], at=("dst 0 of the second read", 1, 0), plants=[("mapq", 0, 84, "miss"), ("mapq", 1, 0, "miss"), ("mapq", 1, 256, "hit")]))
    Ls.append(_layout("across_sq_copy", ["hit300", "copy_as4"], at=("q 0 of the copied read", 1, 0), plants=[("mapq", 0, 84, "miss"), ("mapq", 1, 0, "copy")]))
    # (a copy read sets no memo, so the memo that reaches drop4_front is hit300's: lane 168 goes from q = 168 of hit300 over q = 84 of copy340 to q = 0 of drop4_front)
    Ls.append(_layout("across_copy_sq", ["hit300", "copy340", "drop4_front"], at=("dst 0 of the third read", 2, 0),
                      plants=[("mapq", 0, 168, "miss"), ("mapq", 1, 84, "copy"), ("mapq", 2, 0, "miss"), ("mapq", 2, 256, "hit")]))
    Ls.append(_layout("across_err_other", ["e_fwd", "e_rev_other"], at=("q 1 of the second read", 1, 1), plants=[("esterr", 0, 85, "miss"), ("esterr", 1, 1, "miss"), ("esterr", 1, 257, "hit")]))
    Ls.append(_layout("across_err_k0", ["e_fwd", "e_k0"], at=("k == 0 of the second read", 1, 0), plants=[("esterr", 1, 0, "k0"), ("esterr", 1, 256, "hit")]))
    # ---- eight reads on a plan of three workgroups: as a sound batch here (fail_a and fail_b fail in one wave), read by read behind a refusal in the GPU and model tests ----
    Ls.append(_layout("by_read", BY_READ, at=("fail_a's failing anchor", 2, 395)))
    # ---- the second turn: reads straddle TURN, and the batch's first anchor lies far behind position 0 ----
    Ls.append(_layout("second_turn", SECOND_TURN, b_off0=SECOND_TURN_B_OFF0, at=("the first position of the second turn", 6, 6000 - 5290), gpu_only=True))
    _LAYOUTS = Ls
    return Ls


def reference():
    """-> {name: {"case", "hits": the hits in front of mm_join_long (the mapq plan's input), "mid": the final regions with div as mm_gen_regs leaves it (what the mapq
    plan hands on), "out": the final regions with div, "a": the final a[], "mapq_out" / "mapq_a": the same two from the mapq fixture, "libm"}} from the two fixtures"""
    import os
    from regs_model import REG
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    Zm, Ze = np.load(os.path.join(g, "ref_mapq_limits.npz")), np.load(os.path.join(g, "ref_esterr_limits.npz"))
    cs = cases()
    for Z in (Zm, Ze):
        assert int(Z["reg_size"]) == REG.itemsize and [str(v) for v in Z["names"]] == [c["name"] for c in cs], "the fixtures are not of this module's reads"
    cut = lambda Z, key, off, k: Z[key][Z[off][k]:Z[off][k + 1]]
    out = {}
    for k, c in enumerate(cs):
        w = cut(Ze, "regs_out", "out_off", k).reshape(-1).view(REG)
        mid = w.copy()
        mid["div"] = -1.0
        out[c["name"]] = {"name": c["name"], "case": c, "hits": cut(Zm, "hits_in", "in_off", k).reshape(-1).view(REG), "mapq_out": cut(Zm, "hits_out", "out_off", k).reshape(-1).view(REG),
                          "mapq_a": cut(Zm, "a_out", "a_off", k), "mid": mid, "out": w, "a": cut(Ze, "a_out", "a_off", k), "libm": str(Ze["libm"])}
    return out
