"""Seeded data and the CPU side for the fragment path at the shapes the fixture (tests/golden/ref_frag.npz) is too small for: shared by
tests/test_cpu_frag_shapes.py (which asserts, from the model alone, that every shape occurred) and tests/test_gpu_frag_e2e.py (which compares the library with
the model).  The CPU side is frag_model.map_frag over an index_model.build_index table; nothing here calls the library except FragCpu.gpu_index().

The sets (DATA[name]() -> FragCpu, built once per process):
  a    the re-chain decision at wave width: 100 diverged copies of one source, so that a fragment has about one chain per reference and the chain's index in u
       follows the reference number; fragments cut from a copy of their own, with exact windows of it planted in chosen references
  b    compaction beyond one block: 700 pairs of 2 x 100-150 bases, arranged by the model's decision into long runs of flagged and unflagged fragments
  c    segment boundaries inside a tandem array and inside a member of a repeat family; N runs, lowercase, an empty and a tiny segment
  d    pairs from inside 1 400 near-identical copies of a 150-base unit: nothing to seed with mid_occ 1000, tens of thousands of anchors with max_occ 5000
  e_a, e_c   a and c with the HPC sketch (k 19, w 10)

What cannot occur, for any input (and so is asserted the other way round in test_cpu_frag_shapes.py): collect_minimizers shifts the positions of segment i by
the lengths of the segments before it, so along a chain, whose query positions strictly increase (decrease on the reverse strand), the segment number never
comes back: a best chain reading 0,1,0 does not exist, the count of changes plus one IS the number of distinct segments.  Set a has a chain reading 0,2 in its
place.  For the same reason a repetitive interval of one segment can touch that of the next (st == rep_en, the merging branch) but never overlap it, and a
fragment's rep_len always equals the sum over its segments; set c has the touching intervals."""
import numpy as np

import frag_model as fm
import index_model as im
import sketch_model as sm
from test_gpu_read_chain_e2e import ACGT, Cpu, _chunks, _diverge

SEG_SHIFT = np.uint64(fm.SEG_SHIFT)
KEYS = ("mini_off", "mini_pos", "rep_len", "anchor_off", "u_off", "u", "b_off", "b", "rechained", "n_rechained")


def txt(s):
    return ACGT[np.asarray(s, np.uint8)].tobytes()


def params_of(h, gap_scale=1.0):
    from mm2chain import params
    return params.make_params(max_dist_x=h[0], max_dist_y=h[1], bw=h[2], max_skip=h[3], max_iter=h[4], gap_scale=gap_scale, is_cdna=h[7], n_segs=h[8])


def seg_ids(b):
    """the segment of every anchor of a chain (or of all of b)"""
    return ((b[:, 1] & np.uint64(fm.SEG_MASK)) >> SEG_SHIFT).astype(np.int64)


def best_chain(u, b):
    """(index in u, score, its anchors) of the first chain with the strictly largest score, as map.c:321-326 picks it"""
    sc = (u >> np.uint64(32)).astype(np.int64)
    i = int(np.argmax(sc))                                     # argmax: the first of equals
    cnt = (u & np.uint64(0xFFFFFFFF)).astype(np.int64)
    off = int(cnt[:i].sum())
    return i, int(sc[i]), b[off:off + int(cnt[i])]


def chain_of(u, b, i):
    cnt = (u & np.uint64(0xFFFFFFFF)).astype(np.int64)
    off = int(cnt[:i].sum())
    return b[off:off + int(cnt[i])]


def frag_chunks(frags, chunk_bases):
    """the host's rule over whole fragments (mm2c_frag_chain_batch): the rule of the reads, with a fragment's bases those of its segments"""
    return _chunks([range(sum(len(s) for s in f)) for f in frags], chunk_bases)


def chunk_bases_for(frags, sizes=(2, 3)):
    """a read_chunk_bases under which every chunk holds two or three fragments"""
    tot = [sum(len(s) for s in f) for f in frags]
    cands = sorted({sum(tot[i:i + n]) for n in (2, 3) for i in range(len(tot) - n + 1)})
    for cb in cands:
        if all(r1 - r0 in sizes for r0, r1 in frag_chunks(frags, cb)):
            return cb
    raise AssertionError(f"no read_chunk_bases cuts fragments of {tot} bases into chunks of {sizes}")


class FragCpu(Cpu):
    """a set: references, fragments in groups that may share a call (one n_segs, one set of scalars), and the model's result per (mid_occ, max_occ, heap)"""

    def __init__(self, refs, frags, names, k, w, hpc, groups, mid_occ, max_occ, extra=None):
        self.refs, self.frags, self.names, self.k, self.w, self.hpc = refs, frags, names, k, w, hpc
        self.groups, self.mid_occ, self.max_occ, self.extra = groups, mid_occ, max_occ, extra or {}
        self.keys, self.cr_off, self.n, self.pool = im.build_index(refs, k, w, hpc)
        self.lookup = sm.table_lookup(self.keys, self.cr_off, self.n)
        self.h_of = {g: h for h, ids in groups for g in ids}
        self.cache, self.mini = {}, {}
        assert sorted(g for _, ids in groups for g in ids) == list(range(len(frags)))

    def one(self, g, mid_occ, max_occ, heap=True):
        """frag_model.map_frag of fragment g; its minimizers are made once (the sketch is a Python loop per base) and handed to the later calls"""
        h, made = self.h_of[g], fm.collect_minimizers

        def once(segs, w, k, is_hpc=False):
            if g not in self.mini:
                self.mini[g] = made(segs, w, k, is_hpc)
            return self.mini[g]
        fm.collect_minimizers = once
        try:
            return fm.map_frag(self.frags[g], self.w, self.k, self.lookup, self.pool, params_of(h), h[5], h[6], mid_occ, max_occ, is_hpc=bool(self.hpc), heap=heap)
        finally:
            fm.collect_minimizers = made

    def run(self, heap=True):
        """the model per fragment with the set's mid_occ and max_occ; ["first"] of each is the result of a call with max_occ = mid_occ"""
        key = (self.mid_occ, self.max_occ, bool(heap))
        if key not in self.cache:
            self.cache[key] = [self.one(g, self.mid_occ, self.max_occ, heap) for g in range(len(self.frags))]
        return self.cache[key]

    def by_name(self, name, heap=True):
        return self.run(heap)[self.names.index(name)]


def compare(got, want, ids, names, what, first=False):
    """a frag_chain_batch result against the model's fragments `ids`, bit for bit; the message names the fragment and the field"""
    flags = [0 if first else int(want[g]["rechained"]) for g in ids]
    want = [want[g]["first"] if first else want[g] for g in ids]
    assert got["rep_len"].size == len(ids), f"{what}: {got['rep_len'].size} fragments out, {len(ids)} in"
    for j, (g, r) in enumerate(zip(ids, want)):
        at = f"{what}: fragment {g} ({names[g]})"
        assert int(got["rechained"][j]) == flags[j], f"{at}: rechained {int(got['rechained'][j])}, the model {flags[j]}"
        assert int(got["rep_len"][j]) == int(r["rep_len"]), f"{at}: rep_len {int(got['rep_len'][j])}, the model {int(r['rep_len'])}"
        m0, m1 = int(got["mini_off"][j]), int(got["mini_off"][j + 1])
        assert m1 - m0 == r["mini_pos"].size, f"{at}: mini_off gives {m1 - m0} kept minimizers, the model {r['mini_pos'].size}"
        assert np.array_equal(got["mini_pos"][m0:m1], r["mini_pos"]), f"{at}: mini_pos differs"
        na = int(got["anchor_off"][j + 1] - got["anchor_off"][j])
        assert na == r["n_anchors"], f"{at}: {na} kept anchors, the model {r['n_anchors']}"
        u, b = got["chains"][j]
        assert np.array_equal(u, r["u"]), f"{at}: u differs ({u.size} chains, the model {r['u'].size})"
        assert np.array_equal(b, r["b"]), f"{at}: b differs ({b.shape[0]} anchors in chains, the model {r['b'].shape[0]})"
    assert got["n_rechained"] == sum(flags), f"{what}: n_rechained {got['n_rechained']}, the model {sum(flags)}"


# ---- (a) the decision at wave width ---------------------------------------------------------------------------------------------------------------------------

A_L, A_R, A_MOTIF = 1600, 100, (760, 800)
A_H = lambda n_segs: (5000, 5000, 500, 25, 5000, 3, 40, 0, n_segs)
A_K, A_W, A_MID, A_MAX = 15, 10, 200, 1000


_LOCAL = {}


def _local_first_pass(segs, ref, h, motif_mini):
    """the first pass of `segs` against an index of `ref` and the motif's reference alone: what one reference contributes to the fragment's chains"""
    if ref not in _LOCAL:
        _LOCAL.clear()                                         # (the searches below ask for the same reference many times in a row)
        keys, cr, n, pool = im.build_from_minimizers(np.concatenate([im.sketch_refs([ref], A_K, A_W), motif_mini]))
        _LOCAL[ref] = (sm.table_lookup(keys, cr, n), pool)
    lookup, pool = _LOCAL[ref]
    return fm.map_frag(segs, A_W, A_K, lookup, pool, params_of(h), h[5], h[6], A_MID, A_MID, heap=True)["first"]


def _set_a():
    rng = np.random.default_rng(20261018)
    S = rng.integers(0, 4, A_L, dtype=np.uint8)
    motif = rng.integers(0, 4, 40, dtype=np.uint8)

    def copy_of(d):
        s = _diverge(rng, S, d)
        s[A_MOTIF[0]:A_MOTIF[1]] = motif                      # the planted repeat: every copy and every fragment holds it once, a reference of its own 250 times
        return s
    refs = [copy_of(0.03) for _ in range(A_R)]
    motif_mini = sm.sketch_array(txt(np.tile(motif, 250)), A_W, A_K)
    motif_mini[:, 1] |= np.uint64(1) << np.uint64(32)
    rand = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    frags, names, plan = [], [], {}

    def whole(r, F, lo=100, hi=1300):
        refs[r][lo:hi] = F[lo:hi]

    def alone(r, F, windows):
        """reference r: random but for F's windows, in place -- its chain cannot run on outside them"""
        s = rand(A_L)
        for lo, hi in windows:
            s[lo:hi] = F[lo:hi]
        refs[r] = s

    def add(name, F, cuts):
        frags.append([txt(F[lo:hi]) for lo, hi in cuts]); names.append(name)

    two = [(100, 700), (700, 1300)]
    three = [(100, 500), (500, 900), (900, 1300)]
    # best chain at an index of 64 or more, among 65 chains or more
    F = copy_of(0.10); whole(90, F); add("best_hi", F, two)
    # a change of segment late in the best chain
    F = copy_of(0.10); whole(15, F); add("change_late", F, two)
    # a change exactly between anchors 63 and 64: segment 0 begins where the chain holds 64 of its anchors
    F = copy_of(0.10); whole(30, F)
    ref = txt(F[40:1400])
    for s0 in range(390, 300, -1):
        r = _local_first_pass([txt(F[s0:700]), txt(F[700:1300])], ref, A_H(2), motif_mini)
        seg = seg_ids(best_chain(r["u"], r["b"])[2]) if r["u"].size else np.zeros(0)
        if seg.size > 65 and (seg == 0).sum() == 64 and seg[63] == 0 and seg[64] == 1:
            break
    else:
        raise AssertionError("no start of segment 0 leaves 64 of its anchors in the best chain")
    add("change_63_64", F, [(s0, 700), (700, 1300)])
    # a change between anchors 0 and 1: segment 0 gives the best chain its first anchor and nothing else
    F = copy_of(0.10); whole(50, F)
    ref = txt(F[40:1400])
    for t in range(24, 60):
        r = _local_first_pass([txt(F[700 - t:700]), txt(F[700:1300])], ref, A_H(2), motif_mini)
        seg = seg_ids(best_chain(r["u"], r["b"])[2]) if r["u"].size else np.zeros(0)
        if seg.size > 65 and (seg == 0).sum() == 1:
            break
    else:
        raise AssertionError("no segment 0 gives the best chain exactly one anchor")
    add("change_0_1", F, [(700 - t, 700), (700, 1300)])

    # two chains of equal, strictly largest score: X over both segments (a window across the boundary), Y inside segment 1 alone, each alone in its reference
    def tie(name, r_x, r_y):
        F = copy_of(0.10)
        segs = [txt(F[lo:hi]) for lo, hi in two]
        alone(r_x, F, [(450, 950)])
        x = _local_first_pass(segs, txt(refs[r_x]), A_H(2), motif_mini)
        want = best_chain(x["u"], x["b"])[1]
        assert set(seg_ids(best_chain(x["u"], x["b"])[2])) == {0, 1}
        flank = rand(A_L)
        for lo in range(705, 745):
            for hi in range(lo + want - 4, 1295):
                s = flank.copy(); s[lo:hi] = F[lo:hi]
                y = _local_first_pass(segs, txt(s[lo - 80:hi + 80]), A_H(2), motif_mini)
                sc = best_chain(y["u"], y["b"])[1] if y["u"].size else 0
                if sc == want:
                    refs[r_y] = s
                    y = _local_first_pass(segs, txt(s), A_H(2), motif_mini)
                    if y["u"].size == 1 and best_chain(y["u"], y["b"])[1] == want and set(seg_ids(y["b"])) == {1}:
                        frags.append(segs); names.append(name); plan[name] = (r_x, r_y)
                        return
                if sc > want:
                    break
        raise AssertionError(f"{name}: no window inside segment 1 scores {want}")
    tie("tie_lanes", 20, 5)                                    # Y first: both below 64, different lanes
    tie("tie_same_lane", 10, 75)                               # X first: chains 10 and 74, the same lane (one reference below gives no chain)
    tie("tie_low_lane_later", 70, 40)                          # Y first at 40; X at 70, lane 6
    n2 = len(frags)

    F = copy_of(0.10); whole(80, F); add("three_best_hi", F, three)
    F = copy_of(0.10); alone(60, F, [(150, 880)]); add("three_reads_0_1", F, three)
    F = copy_of(0.10); alone(45, F, [(150, 480), (920, 1280)]); add("three_reads_0_2", F, three)
    F = copy_of(0.10); whole(25, F); add("three_plain", F, three)
    refs = refs + [np.tile(motif, 250)]
    groups = [(A_H(2), list(range(n2))), (A_H(3), list(range(n2, len(frags))))]
    return FragCpu([txt(s) for s in refs], frags, names, A_K, A_W, 0, groups, A_MID, A_MAX, {"plan": plan})


# ---- (b) compaction beyond one block ---------------------------------------------------------------------------------------------------------------------------

B_H = (500, 300, 100, 25, 5000, 2, 25, 0, 2)


def _set_b():
    rng = np.random.default_rng(20261019)
    rand = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    unique = rand(25_000)
    unit = rand(300)
    parts, at, pos = [], [], 0
    for _ in range(60):                                       # the family: 60 copies at 1.5 %, 150 unique bases between them
        sp = rand(150)
        at.append(pos); parts += [sp, _diverge(rng, unit, 0.015)]; pos += 450
    fam = np.concatenate(parts)
    cands = []
    ln = lambda: int(rng.integers(100, 151))
    for _ in range(300):                                      # proper pairs from the unique sequence
        p = int(rng.integers(0, unique.size - 500)); a, b = ln(), ln()
        cands.append([txt(unique[p:p + a]), txt(unique[p + 440 - b:p + 440])])
    for i in range(400):
        c = at[int(rng.integers(1, 58))]
        kind, a, b = (0, 0, 0, 3, 3, 3, 1, 2)[i % 8], ln(), ln()
        r1 = fam[c + 90:c + 90 + a]                            # 60 unique bases, then into the copy
        if kind == 0:                                          # the mate is nowhere: the chain misses a segment
            cands.append([txt(r1), txt(rand(b))])
        elif kind == 1:                                        # both inside a copy: little or nothing to seed
            cands.append([txt(fam[c + 160:c + 160 + a]), txt(fam[c + 450 - b:c + 450])])
        elif kind == 2:                                        # the mate in the next spacer: repetitive bases and a chain over both
            cands.append([txt(r1), txt(fam[c + 450:c + 450 + b])])
        else:                                                  # the mate first
            cands.append([txt(rand(b)), txt(r1)])
    cpu = FragCpu([txt(unique), txt(fam)], cands, ["pair"] * len(cands), 15, 10, 0, [(B_H, list(range(len(cands))))], 20, 200)
    res = cpu.run(True)
    flagged = [g for g, r in enumerate(res) if r["rechained"]]
    plain = [g for g, r in enumerate(res) if not r["rechained"]]
    assert len(flagged) >= 300 and len(plain) >= 300, (len(flagged), len(plain))
    mixed = [g for pair in zip(flagged[262:], plain[260:]) for g in pair]
    rest = flagged[262 + len(mixed) // 2:] + plain[260 + len(mixed) // 2:]
    order = flagged[:1] + plain[:260] + mixed + rest + flagged[1:262]
    assert sorted(order) == list(range(len(cands)))
    cpu.frags = [cands[g] for g in order]
    cpu.cache = {key: [v[g] for g in order] for key, v in cpu.cache.items()}
    cpu.mini = {j: cpu.mini[g] for j, g in enumerate(order)}
    return cpu


# ---- (c) segment boundaries -----------------------------------------------------------------------------------------------------------------------------------

C_H = (5000, 5000, 500, 25, 5000, 3, 40, 0, 3)
C_K, C_W = 15, 10


def _set_c():
    rng = np.random.default_rng(20261020)
    rand = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    unit = rand(45)                                            # the tandem array: 12 exact copies, below mid_occ
    member = rand(600)                                         # the family: 40 copies at 1 %, above it
    other = np.concatenate([np.concatenate([rand(200), _diverge(rng, member, 0.01)]) for _ in range(39)])
    arr0, mem0 = 3000, 6540
    locus = np.concatenate([rand(arr0), np.tile(unit, 12), rand(mem0 - arr0 - 540), _diverge(rng, member, 0.01), rand(12_000 - mem0 - 600)])
    assert locus.size == 12_000
    # the smallest minimizer of the array's unit: a segment that ends with its k-mer keeps it as its last minimizer, one that begins with it as its first
    m = sm.sketch_array(txt(locus[arr0:arr0 + 540]), C_W, C_K)
    inner = m[(m[:, 1] >> np.uint64(1) & np.uint64(0xFFFFFFFF)) > 100]
    kmin = inner[np.argmin(inner[:, 0])]
    e = int(kmin[1] >> np.uint64(1) & np.uint64(0xFFFFFFFF)) % 45 + arr0 + 1          # one past the k-mer's last base, in the array's first units
    while e < arr0 + 90:
        e += 45
    t_end, t_start = e, e + 3 * 45 - C_K                                               # seg s ends after the k-mer; seg s+1 begins with it, three units on
    # inside the family member: segment 1 ends with the k-mer of one of its minimizers and segment 2 begins with the k-mer of a later one
    mm = sm.sketch_array(txt(locus[mem0:mem0 + 600]), C_W, C_K)
    pos = (mm[:, 1] >> np.uint64(1) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    order = np.argsort(mm[:, 0])
    lo = [int(pos[i]) for i in order if 200 < pos[i] < 300][0]                         # small hashes: they stay minimizers at a segment's edge
    hi = [int(pos[i]) for i in order if 320 < pos[i] < 420][0]
    m_end, m_start = mem0 + lo + 1, mem0 + hi + 1 - C_K
    frags, names = [], []

    def add(name, segs):
        frags.append([s if isinstance(s, bytes) else txt(s) for s in segs]); names.append(name)
    add("array_and_member", [locus[500:t_end], locus[t_start:m_end], locus[m_start:m_start + 2600]])
    s = [bytearray(txt(locus[700:t_end])), bytearray(txt(locus[t_start:m_end])), bytearray(txt(locus[m_start:m_start + 2400]))]
    s[0][900:1100] = b"N" * 200; s[1][1500:1530] = b"n" * 30; s[2][:900] = bytes(s[2][:900]).lower(); s[0][:300] = bytes(s[0][:300]).lower()
    add("n_runs_lowercase", [bytes(x) for x in s])
    add("empty_middle", [locus[300:t_end], b"", locus[t_start:t_start + 5200]])       # the array's boundary with an empty segment between
    add("tiny_middle", [locus[1000:t_end], locus[t_start:t_start + 10], locus[m_start:m_start + 5400]])
    add("two_members", [other[100:2300], locus[mem0 - 2000:mem0 + 800], other[9000:12500]])
    add("plain", [locus[200:2600], locus[4000:m_end], locus[9000:11900]])
    refs = [txt(locus), txt(other)]
    cpu = FragCpu(refs, frags, names, C_K, C_W, 0, [(C_H, list(range(len(frags))))], 20, 100)
    return cpu


# ---- (d) a fragment the first pass cannot seed ----------------------------------------------------------------------------------------------------------------

D_H = (500, 300, 100, 25, 5000, 2, 25, 0, 2)


def _set_d():
    rng = np.random.default_rng(20261021)
    unit = rng.integers(0, 4, 150, dtype=np.uint8)
    family = np.concatenate([_diverge(rng, unit, 0.002) for _ in range(1400)])
    unique = rng.integers(0, 4, 5000, dtype=np.uint8)
    cons = np.tile(unit, 4)
    deep = [[txt(cons[o:o + 100]), txt(cons[o + 170:o + 270])] for o in (7, 61, 118)]
    plain = [[txt(unique[p:p + 120]), txt(unique[p + 300:p + 420])] for p in (100, 900, 1700, 2500, 3300)]
    frags = [plain[0], deep[0], plain[1], plain[2], deep[1], deep[2], plain[3], plain[4]]
    names = ["plain", "deep", "plain", "plain", "deep", "deep", "plain", "plain"]
    return FragCpu([txt(family), txt(unique)], frags, names, 15, 10, 0, [(D_H, list(range(len(frags))))], 1000, 5000)


# ---- (e) HPC --------------------------------------------------------------------------------------------------------------------------------------------------

def _set_e_a():
    a = get("a")                                               # 92 of the copies and the motif's reference
    return FragCpu(a.refs[:92] + a.refs[-1:], a.frags, a.names, 19, 10, 1, a.groups, a.mid_occ, a.max_occ)


def _set_e_c():
    c = get("c")
    return FragCpu(c.refs, c.frags, c.names, 19, 10, 1, c.groups, c.mid_occ, c.max_occ)


_MAKERS = {"a": _set_a, "b": _set_b, "c": _set_c, "d": _set_d, "e_a": _set_e_a, "e_c": _set_e_c}
_SETS = {}


def get(name):
    """the set, built once per process"""
    if name not in _SETS:
        _SETS[name] = _MAKERS[name]()
    return _SETS[name]
