"""Forests that put the device epilogue (csrc/chain_epilogue.hip) at the limits of its keys, sorts and LDS classes (tests/test_gpu_epilogue_limits.py runs them;
tests/test_cpu_epilogue_limit_data.py asserts, from the oracle alone, that each one reaches the limit it names).  No DP produced these f[] / p[]: ob.backtrack and
ChainPlan.chains take any f[] / p[] with p[i] < i, so every count below is set by construction.

The brick is a COMB: C independent paths, anchor t of every path in round t and the rounds one after the other, so that the parent of an anchor is the anchor of
its own path in the round before (with paths of one length: exactly C anchors back).  f rises along a path: the leaf is the peak, the path is one chain, its score
is f[leaf].  A path may HANG on an anchor of another path (a branch): its chain stops there and scores f[leaf] - f[stop].  `rows` lays the paths out one after the
other instead (parent = i - 1).  x never falls with the index and y holds the index: every anchor of a task is distinct, every order is visible.

A case is a dict: name, a (uint64 [n, 2]), f, p (int32), min_cnt, min_sc, facts.  facts = what the case claims:
  n, nu (chain ends: anchors without a child whose maximum of f over itself and its ancestors is >= min_sc), top / low (the largest and the smallest peak score
  among the chain ends) -- computed here from f[] / p[] alone -- and nk (kept chains), ties (equal neighbours among the first x of the kept chains, in the order of
  the output), by the builder's own arithmetic."""
import numpy as np

FUSE_S, FUSE_L = 5120, 7680     # chain_epilogue.hip:150  the two LDS size classes of epi_fused (CAP); longer tasks take kernels A / B / C
ENDS_MAX = 1024                 # chain_epilogue.hip:152,494  2 * FNT: the most chain ends the sort-free form holds (two per thread)
RANK_MAX = 768                  # chain_epilogue.hip:153  the most keys ordered by counting (:648 kept chains, :667 chain ends, :807 kept chains)
TS_MAX = 4096                   # chain_epilogue.hip:862  the most chains whose tie replay keeps its index array in LDS
W = 256                         # chain_epilogue.hip:148  anchors per chunk of kernels A / B / C
WIDE = 1 << 19                  # chain_epilogue.hip:475  peak scores in [1, 2^19) fit the one-word owner key f[peak] << 13 | peak

U = np.uint64
SPAN = 15
X0 = (1 << 32) | (1 << 20)
F_MAX = 1 << 30                 # every |f| stays at or below this, so every f[peak] - f[stop] is an int32


# ---- layout -------------------------------------------------------------------------------------------------------------------------------------------------------
def assemble(paths, layout="comb", tie_first=0):
    """paths: [(f values from the root to the leaf, None or (path, position) of the anchor the root hangs on)]; a path hangs on an earlier path only.
    comb: anchor t of a path stands in round start + t (start = one round behind the anchor it hangs on, else 0), rounds in order, paths in order inside a round;
    rows: path after path.  tie_first: the first so many anchors have pairwise equal x (0 1 | 2 3 | ...).  Returns a, f, p."""
    lens = np.array([len(fv) for fv, _ in paths], np.int64)
    first = np.cumsum(lens) - lens                                    # flat position of every path's root
    start = np.zeros(len(paths), np.int64)
    hang_at = np.full(len(paths), -1, np.int64)
    for k, (_, hang) in enumerate(paths):
        if hang is not None:
            j, m = hang
            assert j < k and 0 <= m < lens[j]
            start[k] = start[j] + m + 1
            hang_at[k] = first[j] + m
    pid = np.repeat(np.arange(len(paths)), lens)
    t = np.arange(int(lens.sum())) - np.repeat(first, lens)
    order = np.lexsort((pid, start[pid] + t)) if layout == "comb" else np.arange(pid.size)
    assert layout in ("comb", "rows")
    where = np.empty(pid.size, np.int64)
    where[order] = np.arange(pid.size)                                # flat position -> index in the task
    parent_flat = np.where(t > 0, np.arange(pid.size) - 1, hang_at[pid])
    p_flat = np.where(parent_flat >= 0, where[np.maximum(parent_flat, 0)], -1)
    f_flat = np.concatenate([np.asarray(fv, np.int64) for fv, _ in paths])
    f, p = f_flat[order], p_flat[order]
    n = f.size
    assert np.all(p < np.arange(n)) and np.abs(f).max() <= F_MAX
    step = np.ones(n, np.int64)
    step[1:tie_first:2] = 0
    a = np.empty((n, 2), U)
    a[:, 0] = U(X0) + np.cumsum(step).astype(U)
    a[:, 1] = (U(SPAN) << U(32)) | np.arange(n).astype(U)
    return a, f.astype(np.int32), p.astype(np.int32)


def rising(top, length, gain=15):
    """f along a path of `length` anchors that ends at `top`"""
    return top - gain * np.arange(length - 1, -1, -1, dtype=np.int64)


# ---- what a task reaches, from f[] / p[] alone -----------------------------------------------------------------------------------------------------------------
def fill_v(f, p):
    """v[i] = the maximum of f over i and its ancestors (chain.c:106-111), by pointer jumping"""
    v = np.asarray(f, np.int64).copy()
    ptr = np.asarray(p, np.int64).copy()
    while (ptr >= 0).any():
        has = ptr >= 0
        q = np.maximum(ptr, 0)
        v = np.where(has, np.maximum(v, v[q]), v)
        ptr = np.where(has, ptr[q], -1)
    return v


def chain_ends(f, p, min_sc):
    """indices of the chain ends (chain.c:349-354) and their peak scores (f[peak] = v[end], chain.c:360-361)"""
    n = len(f)
    child = np.zeros(n, bool)
    child[np.asarray(p)[np.asarray(p) >= 0]] = True
    v = fill_v(f, p)
    ends = np.nonzero(~child & (v >= min_sc))[0]
    return ends, v[ends]


def _case(name, afp, min_cnt, min_sc, nk, ties=0):
    a, f, p = afp
    ends, peak_sc = chain_ends(f, p, min_sc)
    facts = dict(n=int(f.size), nu=int(ends.size), top=int(peak_sc.max()), low=int(peak_sc.min()), nk=int(nk), ties=int(ties))
    for arr in (a, f, p):
        arr.setflags(write=False)
    return dict(name=name, a=a, f=f, p=p, min_cnt=int(min_cnt), min_sc=int(min_sc), facts=facts)


def _tops(rng, count, lo=60, hi=5000):
    return rng.integers(lo, hi, count).astype(np.int64)


def comb(name, seed, lengths, min_cnt, min_sc=40, tie_first=0, tops=None, layout="comb", hi=5000):
    """independent paths of the given lengths, leaf scores drawn in [60, hi) (or `tops`): every leaf is a chain end, a chain is kept when its path is long enough"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    tops = _tops(rng, lengths.size, hi=hi) if tops is None else np.asarray(tops, np.int64)
    gain = np.minimum(15, (tops - min_sc) // lengths)
    assert tops.min() >= min_sc + 15 and gain.min() >= 1
    afp = assemble([(rising(int(s), int(L), int(g)), None) for s, L, g in zip(tops, lengths, gain)], layout, tie_first)
    kept = lengths >= min_cnt
    # the first tie_first anchors are the roots of the first paths, in pairs of one x: a pair counts when both its chains are kept
    pairs = sum(1 for k in range(0, min(tie_first, lengths.size) - 1, 2) if kept[k] and kept[k + 1]) if layout == "comb" else 0
    return _case(name, afp, min_cnt, min_sc, int(kept.sum()), pairs)


def _mixed_lengths(C, n):
    """C paths of one or two anchors, n anchors in all; the paths of two come first"""
    assert C <= n <= 2 * C
    return np.array([2] * (n - C) + [1] * (2 * C - n))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------------
MIN_SC = 40
SCORE_19 = (WIDE - 1, WIDE, WIDE + 1)


def score_19():
    """the best chain's peak score at 2^19 - 1, 2^19, 2^19 + 1 (nothing else differs); two branches stop at an anchor of that chain whose f is 2^19 - 2 000, one
    scores exactly min_sc (kept), the other min_sc - 1 (dropped); 300 ordinary chains of three anchors around them"""
    out = []
    for top in SCORE_19:
        rng = np.random.default_rng(1900)
        best = np.concatenate((WIDE - 4000 + 100 * np.arange(39), [top]))
        stop = int(best[20])
        assert stop == WIDE - 2000
        paths = [(rising(int(s), 3), None) for s in _tops(rng, 150)]
        paths.append((best, None))
        paths.append(([stop + 10, stop + 20, stop + MIN_SC], (150, 20)))
        paths.append(([stop + 9, stop + 19, stop + MIN_SC - 1], (150, 20)))
        paths += [(rising(int(s), 3), None) for s in _tops(rng, 150)]
        out.append(_case(f"score_19/top-{top}", assemble(paths), 2, MIN_SC, nk=302))
    return out


def score_nonpositive():
    """min_sc = -5: a chain whose peak score is 0, one whose peak score is -2, one whose peak score (-10) is below min_sc, thirty ordinary chains, and a peak with two
    leaves under it (both leaves list that peak: the second listing keeps the taken peak alone, chain.c:381-383).  The same task under min_cnt = 2 and min_cnt = 1."""
    rng = np.random.default_rng(500)
    paths = [(rising(int(s), 3), None) for s in _tops(rng, 15, 20, 300)]
    paths.append(([-3, 0], None))
    paths.append(([-4, -2], None))
    paths.append(([-20, -10], None))
    paths.append(([20, 50], None))                                    # path 18: the peak ...
    paths.append(([45], (18, 1)))                                     # ... and its two leaves
    paths.append(([44], (18, 1)))
    paths += [(rising(int(s), 3), None) for s in _tops(rng, 15, 20, 300)]
    afp = assemble(paths)
    # chain ends: 30 ordinary, the two at 0 and -2, the two leaves; kept under min_cnt = 2: all but the second listing (one anchor)
    return [_case("score_nonpositive/min_cnt-2", afp, 2, -5, nk=33), _case("score_nonpositive/min_cnt-1", tuple(x.copy() for x in afp), 1, -5, nk=34)]


BYTE_EDGES = tuple(v for b in (8, 16, 19, 24, 30) for v in ((1 << b) - 1, 1 << b))


def score_bytes():
    """peak scores 2^b - 1 and 2^b for b = 8, 16, 19, 24, 30 among scores drawn evenly over the bit lengths 7 .. 30: the keys differ in every byte of the score.
    Paths of two anchors; one branch that stops on the path of 2^30.  Once with 700 chains (counting), once with 1 100 (the radix sort)."""
    out = []
    for C in (700, 1100):
        rng = np.random.default_rng(800 + C)
        bits = rng.integers(7, 31, C - 1 - len(BYTE_EDGES))
        tops = np.concatenate((BYTE_EDGES, (1 << (bits - 1)) + rng.integers(0, 64, bits.size) * (1 << (bits - 7)))).astype(np.int64)
        tops = tops[rng.permutation(tops.size)]
        paths = [(rising(int(s), 2, gain=20), None) for s in tops]
        at = int(np.nonzero(tops == F_MAX)[0][0])
        paths[at] = ([F_MAX - 1000, F_MAX - 500, F_MAX], None)
        paths.append(([F_MAX - 450, F_MAX - 400], (at, 1)))             # the branch: stops at f = 2^30 - 500 and scores 100
        out.append(_case(f"score_bytes/chains-{C}", assemble(paths), 2, MIN_SC, nk=C))
    return out


def ends_1024():
    out = [comb(f"ends_1024/all-kept-{C}", 1024 + C, [2] * C, 2) for C in (ENDS_MAX, ENDS_MAX + 1)]
    for C in (ENDS_MAX, ENDS_MAX + 1):
        lengths = np.ones(C, np.int64)
        lengths[np.linspace(3, C - 4, 25).astype(np.int64)] = 12       # 25 long paths among the one-anchor paths
        out.append(comb(f"ends_1024/few-kept-{C}", 2048 + C, lengths, 2))
    return out


def rank_768_by_key():
    return [comb(f"rank_768_by_key/{C}", 768 + C, [2] * C, 2) for C in (RANK_MAX, RANK_MAX + 1)]


def rank_768_general():
    out = []
    for C in (RANK_MAX, RANK_MAX + 1):
        rng = np.random.default_rng(7680 + C)
        tops = _tops(rng, C)
        tops[C // 3] = WIDE + 77                                        # one score beyond the one-word key: the general form
        out.append(comb(f"rank_768_general/{C}", 0, [2] * C, 2, tops=tops))
    return out


HALF_CAP = ((FUSE_S // 2, FUSE_S), (FUSE_S // 2 + 1, FUSE_S), (FUSE_L // 2, FUSE_L), (FUSE_L // 2 + 1, FUSE_L))


def half_cap():
    """nu at CAP / 2 and one beyond, in tasks that fill their class: paths of two anchors and, for the odd counts, two paths of one anchor (min_cnt = 1)"""
    return [comb(f"half_cap/nu-{C}-n-{n}", 2560 + C, _mixed_lengths(C, n), 1) for C, n in HALF_CAP]


THIRD_CAP = ((FUSE_S // 3, 2 * (FUSE_S // 3)), (FUSE_S // 3 + 1, 2 * (FUSE_S // 3 + 1)), (FUSE_L // 3, FUSE_S + 1), (FUSE_L // 3 + 1, FUSE_S + 2))


def third_cap():
    """not in the kernel's list of named constants, but a switch all the same (chain_epilogue.hip:817): in the general form the sort of more than RANK_MAX kept
    chains by first x runs inside the cells' LDS up to CAP / 3 chains.  nk = nu at CAP / 3 and one beyond in both classes; paths of two anchors, one of three where
    the task has to be longer than 5 120"""
    out = []
    for C, n in THIRD_CAP:
        lengths = np.full(C, 2)
        lengths[C // 2] += n - 2 * C
        out.append(comb(f"third_cap/nk-{C}-n-{n}", 1700 + C, lengths, 2))
    return out


def ties_4096():
    """4 096 and 4 097 kept chains whose first x are equal in pairs: (a) in exactly 7 680 anchors, (b) in more (kernels A / B / C), (c) 4 097 roots and nothing else"""
    out = []
    for C in (TS_MAX, TS_MAX + 1):
        out.append(comb(f"ties_4096/a-fused-{C}", 4096 + C, _mixed_lengths(C, FUSE_L), 1, tie_first=C))
    for C in (TS_MAX, TS_MAX + 1):
        out.append(comb(f"ties_4096/b-chunked-{C}", 8192 + C, [2] * C, 1, tie_first=C))
    out.append(comb(f"ties_4096/c-roots-{TS_MAX + 1}", 12288, [1] * (TS_MAX + 1), 1, tie_first=TS_MAX + 1))
    return out


CHUNK_SIZES = (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1)
CHUNK_LINKS = (W - 1, W, W + 1)


def chunk_256():
    out = [comb(f"chunk_256/path-{n}", 256 + n, [n], 2, tops=[60 + 15 * n], layout="rows") for n in CHUNK_SIZES]
    out += [comb(f"chunk_256/link-{C}", 512 + C, [5] * C, 2, hi=900) for C in CHUNK_LINKS]
    return out


ONE_PATH = (FUSE_S, FUSE_S + 1, FUSE_L, FUSE_L + 1)


def one_path():
    """one path: the depth counters and the length field of u at their largest; the two sizes that fill an LDS class also with a peak score beyond 2^19 (the depths
    of the general form)"""
    out = [comb(f"one_path/{n}", n, [n], 2, tops=[60 + 15 * n], layout="rows") for n in ONE_PATH]
    return out + [comb(f"one_path/{n}-wide", n, [n], 2, tops=[WIDE + n], layout="rows") for n in (FUSE_S, FUSE_L)]


_CASES = []


def forest_cases():
    """every case, built once and handed out read-only; in the order of the batch, which is not by size"""
    if not _CASES:
        s19, neg, byt, e1k, rk, rg, hc, t4k, ch, op, tc = (score_19(), score_nonpositive(), score_bytes(), ends_1024(), rank_768_by_key(), rank_768_general(),
                                                           half_cap(), ties_4096(), chunk_256(), one_path(), third_cap())
        _CASES.extend([ch[0], t4k[1], s19[0], op[2], rk[0], e1k[3], hc[0], ch[6], neg[0], tc[2], t4k[2], byt[1], ch[4], s19[1], op[1], rg[1], e1k[0], hc[3],
                       ch[1], tc[1], op[4], t4k[4], rk[1], neg[1], ch[7], op[3], e1k[1], hc[1], byt[0], ch[5], s19[2], tc[3], t4k[0], rg[0], ch[2], e1k[2], op[0], ch[8],
                       hc[2], op[5], tc[0], t4k[3], ch[3]])
        assert len({c["name"] for c in _CASES}) == len(_CASES) == 43
    return _CASES


EMPTY_AT = (5, 19, 34)          # positions of the three empty tasks in the batch


def batch(cases, empty_at=()):
    """CSR batch of the cases with empty tasks in front of the given positions: returns off, a, f, p and the task number of every case"""
    sizes, task_of_case = [], []
    for k, c in enumerate(cases):
        if k in empty_at:
            sizes.append(0)
        task_of_case.append(len(sizes))
        sizes.append(c["f"].size)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    return (off, np.ascontiguousarray(np.concatenate([c["a"] for c in cases])), np.ascontiguousarray(np.concatenate([c["f"] for c in cases])),
            np.ascontiguousarray(np.concatenate([c["p"] for c in cases])), task_of_case)


def groups(cases):
    """the distinct (min_cnt, min_sc) of the cases"""
    return sorted({(c["min_cnt"], c["min_sc"]) for c in cases})


# boundary pairs (and triples): the cases on either side of one switch, run alone in a batch of their own
PAIRS = {
    "score_19": ["score_19/top-%d" % s for s in SCORE_19],
    "score_nonpositive": ["score_nonpositive/min_cnt-2", "score_nonpositive/min_cnt-1"],
    "score_bytes": ["score_bytes/chains-700", "score_bytes/chains-1100"],
    "ends_1024-all-kept": ["ends_1024/all-kept-1024", "ends_1024/all-kept-1025"],
    "ends_1024-few-kept": ["ends_1024/few-kept-1024", "ends_1024/few-kept-1025"],
    "rank_768_by_key": ["rank_768_by_key/768", "rank_768_by_key/769"],
    "rank_768_general": ["rank_768_general/768", "rank_768_general/769"],
    "half_cap-5120": ["half_cap/nu-2560-n-5120", "half_cap/nu-2561-n-5120"],
    "half_cap-7680": ["half_cap/nu-3840-n-7680", "half_cap/nu-3841-n-7680"],
    "third_cap-5120": ["third_cap/nk-1706-n-3412", "third_cap/nk-1707-n-3414"],
    "third_cap-7680": ["third_cap/nk-2560-n-5121", "third_cap/nk-2561-n-5122"],
    "ties_4096-a": ["ties_4096/a-fused-4096", "ties_4096/a-fused-4097"],
    "ties_4096-b": ["ties_4096/b-chunked-4096", "ties_4096/b-chunked-4097"],
    "ties_4096-c": ["ties_4096/c-roots-4097"],
    "chunk_256-paths": ["chunk_256/path-%d" % n for n in CHUNK_SIZES],
    "chunk_256-links": ["chunk_256/link-%d" % C for C in CHUNK_LINKS],
    "one_path-5120": ["one_path/5120", "one_path/5121", "one_path/5120-wide"],
    "one_path-7680": ["one_path/7680", "one_path/7681", "one_path/7680-wide"],
}


def by_name(name):
    return next(c for c in forest_cases() if c["name"] == name)


_REF = {}


def reference(case, min_cnt=None, min_sc=None):
    """the oracle's (u, b) of a case under its own thresholds (or the given ones), computed once and handed out read-only"""
    import oracle_binding as ob
    key = (case["name"], case["min_cnt"] if min_cnt is None else min_cnt, case["min_sc"] if min_sc is None else min_sc)
    if key not in _REF:
        u, b = ob.backtrack(key[1], key[2], case["a"], case["f"], case["p"])
        u.setflags(write=False); b.setflags(write=False)
        _REF[key] = (u, b)
    return _REF[key]


# ---- tasks that go through the real DP -------------------------------------------------------------------------------------------------------------------------
DP_SCORE_19 = (2056, 2057, 2058)          # 255 * n = 524 280 / 524 535 / 524 790: below, above, above 2^19


def dp_score_19():
    """(P, tasks): strictly colinear chains of span 255 and 2 056, 2 057, 2 058 anchors (every link gains the whole span: f of the last anchor is 255 n) under
    the map-ont scalars, and an ordinary task of 300 anchors between them"""
    from limit_data import _colinear255
    from mm2chain import params, synth
    rng = np.random.default_rng(1919)
    col = [_colinear255(rng, n, lo=256) for n in DP_SCORE_19]
    plain = synth.make_stream("mixed", 1, 300, seed=1920)[1].numpy().view(np.uint64).reshape(-1, 2)
    return params.map_ont(), [col[0], col[1], plain, col[2]]
