"""Seeded reads that put the seed-hit path (csrc/seed_hits.hip, csrc/radix_replay.h) at the limits of its size classes, key widths, run lengths and bucket
forms (tests/test_gpu_seed_limits.py runs them; tests/test_cpu_seed_limit_data.py asserts, from the oracle alone, that each one reaches the limit it names and that a
plain stable sort would NOT pass where the reference's unstable sort reorders).

A read is (qlen, matches, hits) as `_batch` of tests/test_gpu_seed_hits.py takes it.  Every builder starts from the x values it wants IN FILL ORDER (the order
collect_seed_hits writes a[], map.c:222-243) and makes one match with one hit per anchor, at strictly increasing query positions: the anchor count is exact, and anchors
with equal x always differ in y, so every order among them is visible.  A case is a dict:
  name, read, na                 the exact anchor count
  runs                           None or [(start, length)]: every run of >= 2 equal x in the sorted list, by the builder's own arithmetic
  kb, idb                        None or the widths the builder aimed at
  reorder                        the run lengths inside which the reference's order must differ from the stable sort's (() = it must differ somewhere);
                                 None: the reference cannot reorder this read, the two orders must be EQUAL
  top                            set D: (shift, {digit: size}) of the first pass that has more than one occupied digit;  nodes: further (shift, {digit: size}) to find

x = strand << 63 | rid << 32 | pos (pos < 2^31, rid < 2^31), map.c:232-238."""
import numpy as np

import oracle_binding as ob

U = np.uint64
SPAN = 15


def mk_x(strand, rid, pos):
    return (np.asarray(strand, U) << U(63)) | (np.asarray(rid, U) << U(32)) | np.asarray(pos, U)


def read_from_x(x_fill, seed):
    """one match with one hit per anchor; the strand of the query minimizer is random, the hit's strand bit follows from the wanted x"""
    x = np.ascontiguousarray(x_fill, U)
    n = x.size
    rng = np.random.default_rng(seed)
    qs = rng.integers(0, 2, n).astype(U)
    qpos = (SPAN - 1 + 3 * np.arange(n) + rng.integers(0, 3, n)).astype(U)
    m = np.zeros(n, ob.MATCH_DTYPE)
    m["n"] = 1
    m["cr_off"] = np.arange(n)
    m["q_pos"] = ((qpos << U(1)) | qs).astype(np.uint32)
    m["q_span"] = SPAN
    m["seg_tandem"] = rng.integers(0, 2, n)
    hits = (x & U(0x7fffffff00000000)) | ((x & U(0x7fffffff)) << U(1)) | ((x >> U(63)) ^ qs)
    return int(qpos[-1]) + 20 if n else 100, m, hits


def fill_anchors(read, for_only=False):
    """map.c:222-243 in NumPy: the anchors of a read in the order collect_seed_hits fills a[], before the sort (for_only: MM_F_FOR_ONLY, map.c:137-143)"""
    qlen, m, h = read
    cnt = m["n"].astype(np.int64)
    idx = np.repeat(np.arange(m.size), cnt)
    k = np.arange(idx.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    r = np.asarray(h, U)[m["cr_off"][idx] + k]
    qp, span, st = m["q_pos"][idx].astype(np.int64), m["q_span"][idx].astype(np.int64), m["seg_tandem"][idx].astype(U)
    fwd = (r & U(1)).astype(np.int64) == (qp & 1)
    x = (r & U(0xffffffff00000000)) | ((r & U(0xffffffff)) >> U(1)) | np.where(fwd, U(0), U(1) << U(63))
    qe = qp >> 1
    ylow = np.where(fwd, qe, int(qlen) - (qe + 1 - span) - 1) & 0xffffffff
    y = (span.astype(U) << U(32)) | ylow.astype(U) | ((st >> U(1)) << U(48)) | ((st & U(1)) << U(42))
    a = np.stack((x, y), 1)
    return a[fwd] if for_only else a


_REF = {}


def reference(case):
    """the oracle's anchor list of a case, computed once and handed out read-only"""
    if case["name"] not in _REF:
        qlen, m, h = case["read"]
        a = ob.collect_seed_hits(m, h, qlen, case.get("flag", 0), heap=case.get("heap", False))
        a.setflags(write=False)
        _REF[case["name"]] = a
    return _REF[case["name"]]


# ---- what a read reaches, from the oracle's sorted x ------------------------------------------------------------------------------------------------------------
def widths(x):
    """kb = the differing bits of x squeezed (bit lengths of the differing position bits and target-id bits, plus the strand), idb = the bits of an index"""
    x = np.asarray(x, U)
    diff = int(np.bitwise_or.reduce(x) ^ np.bitwise_and.reduce(x)) if x.size else 0
    kb = (diff & 0xffffffff).bit_length() + ((diff >> 32) & 0x7fffffff).bit_length() + (diff >> 63)
    return kb, max(1, (int(x.size) - 1).bit_length())


def runs_of(x_sorted):
    """[(start, length)] of the maximal runs of >= 2 equal x"""
    x = np.asarray(x_sorted, U)
    if x.size == 0:
        return []
    edge = np.concatenate(([0], np.nonzero(x[1:] != x[:-1])[0] + 1, [x.size]))
    return [(int(s), int(e - s)) for s, e in zip(edge[:-1], edge[1:]) if e - s >= 2]


def bucket_tree(x_sorted, lo=0, hi=None, shift=56):
    """every call of rs_sort the reference makes on more than 64 records (ksort.h:101-151), as (shift, lo, hi, {digit: size}): a bucket is a range of positions of
    the sorted array, so the sorted x alone gives the tree"""
    x = np.asarray(x_sorted, U)
    hi = x.size if hi is None else hi
    if hi - lo <= 64:
        return []
    dig, size = np.unique((x[lo:hi] >> U(shift)) & U(255), return_counts=True)
    out = [(shift, lo, hi, {int(d): int(s) for d, s in zip(dig, size)})]
    if shift:
        at = lo
        for s in size:
            out += bucket_tree(x, at, at + int(s), shift - 8 if shift > 8 else 0)
            at += int(s)
    return out


def first_split(tree):
    return next(((sh, dg) for sh, _, _, dg in tree if len(dg) > 1), None)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------------------------------
def _sites(rng, n, b0=26, b1=2, bs=1, ends=False):
    """n distinct x in ascending order from positions below 2^b0, target ids below 2^b1 and bs + 1 strands; ends: with the smallest and the largest of them, so that
    x_or ^ x_and has exactly the bits of the three fields"""
    space = 1 << (b0 + b1 + bs)
    assert n <= space and (not ends or n >= 2 or space == 1)
    got = np.zeros(0, U)
    if ends:
        got = mk_x([0, bs], [0, (1 << b1) - 1], [0, (1 << b0) - 1])
    while True:
        k = 2 * n + 16
        got = np.unique(np.concatenate((got, mk_x(rng.integers(0, bs + 1, k), rng.integers(0, 1 << b1, k), rng.integers(0, 1 << b0, k)))))
        if got.size >= n:
            break
    if got.size > n:
        keep = np.ones(got.size, bool)
        inner = np.arange(1, got.size - 1) if ends else np.arange(got.size)
        keep[rng.choice(inner, got.size - n, replace=False)] = False
        got = got[keep]
    return got


def _case(name, seed, sites, mult, **kw):
    """sites[k] taken mult[k] times, in a random fill order"""
    rng = np.random.default_rng(seed)
    mult = np.asarray(mult, np.int64)
    assert sites.size == mult.size and np.all(sites[1:] > sites[:-1])
    xs = np.repeat(sites, mult)
    starts = np.cumsum(mult) - mult
    case = dict(name=name, read=read_from_x(rng.permutation(xs), seed + 1), na=int(xs.size), runs=[(int(s), int(c)) for s, c in zip(starts, mult) if c >= 2],
                kb=None, idb=None, reorder=())
    case.update(kw)
    return case


def run_case(name, seed, lengths, gaps, lead=0, tail=0, **kw):
    """sorted layout: `lead` single anchors, then a run of lengths[k] anchors of one x followed by gaps[k] single anchors (the last run by `tail`)"""
    assert len(gaps) == len(lengths) - 1
    mult = [1] * lead
    for k, L in enumerate(lengths):
        mult += [L] + [1] * (gaps[k] if k < len(gaps) else tail)
    rng = np.random.default_rng(seed)
    return _case(name, seed + 7, _sites(rng, len(mult)), mult, reorder=tuple(sorted(set(lengths))), **kw)


def _tie_mult(rng, na):
    """multiplicities that add up to exactly na, about a third of the anchors in runs of 2 .. 4"""
    mult = rng.choice([1, 1, 1, 1, 1, 1, 2, 3, 4], na)
    mult = mult[:int(np.searchsorted(np.cumsum(mult), na, side="left")) + 1]
    mult[-1] -= int(mult.sum()) - na
    assert mult.sum() == na and mult.min() >= 1
    return mult


def ties_case(name, seed, na, **kw):
    """exactly na anchors, about a third of them in runs of 2 .. 4 equal x"""
    rng = np.random.default_rng(seed)
    mult = _tie_mult(rng, na)
    return _case(name, seed + 7, _sites(rng, mult.size), mult, **kw)


# ---- A: runs of equal x -------------------------------------------------------------------------------------------------------------------------------------------
def set_a_223():
    """Runs of 223 = RUN_MAX - 1 positions, the longest the windowed fix-up takes: reads of about 3 300 anchors whose first run starts at position 0 and whose last ends at
    position na - 1, gaps of 1 .. 64 single anchors chosen so that the run starts of the reads together cover every residue modulo 64 (a read of at most 5 120 anchors holds
    13 such runs, so the 64 residues take six reads; the last read is filled up with random residues)."""
    rng = np.random.default_rng(2230)
    todo = list(rng.permutation(np.arange(1, 64)))
    cases = []
    while todo:
        at, gaps = 0, []
        for _ in range(12):
            g = (int(todo.pop() if todo else rng.integers(0, 64)) - at - 223) % 64
            g = g if g else 64
            gaps.append(g)
            at += 223 + g
        cases.append(run_case(f"A-L223-{len(cases)}", 2231 + 10 * len(cases), [223] * (len(gaps) + 1), gaps))
    return cases


def _spaced(seed, L, n_runs):
    rng = np.random.default_rng(seed)
    return dict(lengths=[L] * n_runs, gaps=[int(g) for g in rng.integers(1, 65, n_runs - 1)], lead=int(rng.integers(1, 65)), tail=int(rng.integers(1, 65)))


def set_a_lengths():
    cases = [run_case(f"A-L{L}", 3000 + L, **_spaced(L, L, max(2, 3000 // (L + 32)))) for L in (222, 224, 225, 447, 1000)]
    mix = _spaced(5, 223, 12)
    mix["lengths"] = [223, 224] * 6
    return cases + [run_case("A-L223+224", 3999, **mix)]


def set_a_long():
    """the same run lengths in the two-wave class (5 121 .. 12 288 anchors) and the eight-wave class (12 289 .. 65 536)"""
    return [run_case(f"A-L{L}-{n // 1000}k", 4000 + L + n, **_spaced(L + n, L, n // (L + 32))) for n in (9000, 20000) for L in (223, 224)]


def set_a_one_x():
    """every anchor with one x (kb = 0): each pass of the reference sees one bucket and moves nothing, so the list stays in fill order"""
    return [_case(f"A-one-x-{n}", 4500 + n, mk_x([1], [2], [123456]), [n], kb=0, reorder=None) for n in (65, 300, 5121, 20000)]


# ---- B: size classes ------------------------------------------------------------------------------------------------------------------------------------------------
BOUNDS = (64, 2560, 5120, 12288, 16384, 65536, 131072)


def size_case(na):
    # 64 anchors or fewer: the reference sorts by insertion (ksort.h:149), which is stable
    return ties_case(f"B-{na}", 5000 + na, na, reorder=None if na <= 64 else ())


def set_b_batches():
    """n and n + 1 anchors at every boundary, in two batches with short reads between them, not in order of size"""
    short = [ties_case(f"B-short-{k}", 5900 + k, n) for k, n in enumerate((300, 70, 1500, 900, 130, 2000))]
    one = [short[0], size_case(2560), size_case(131072), short[1], size_case(64), size_case(5121), size_case(12288), size_case(16385), short[2], size_case(65536)]
    two = [size_case(12289), short[3], size_case(131073), size_case(65), size_case(2561), short[4], size_case(5120), size_case(16384), short[5], size_case(65537)]
    return one, two


def skip_case(cap, kept):
    """capacity against count: `cap` hits of which exactly `kept` are on the forward strand -- what MM_F_FOR_ONLY keeps (map.c:137-143) --, with equal x among the kept"""
    rng = np.random.default_rng(6000 + cap + kept)
    mult = _tie_mult(rng, kept)
    fwd_x = rng.permutation(np.repeat(_sites(rng, mult.size, bs=0), mult))
    rev_x = mk_x(1, rng.integers(0, 4, cap - kept), rng.integers(0, 1 << 26, cap - kept))
    where = rng.permutation(cap)
    x_fill = np.empty(cap, U)
    x_fill[np.sort(where[:kept])] = fwd_x
    x_fill[where[kept:]] = rev_x
    starts = np.cumsum(mult) - mult
    return dict(name=f"B-cap{cap}-keep{kept}", read=read_from_x(x_fill, 6200 + cap + kept), na=kept, cap=cap, flag=ob.F_FOR_ONLY,
                runs=[(int(s), int(c)) for s, c in zip(starts, mult) if c >= 2], kb=None, idb=None, reorder=None if kept <= 64 else ())


SKIP_CASES = ((16385, 64), (16385, 65), (16385, 2561), (16385, 5121), (131073, 12289))


def heap_case(n_matches):
    """exactly n_matches matches of 1 .. 3 hits each, every list ascending as mm_idx_get hands them out, on so few positions that many x are equal"""
    rng = np.random.default_rng(7000 + n_matches)
    m = np.zeros(n_matches, ob.MATCH_DTYPE)
    m["n"] = rng.integers(1, 4, n_matches)
    m["q_pos"] = ((SPAN - 1 + 3 * np.arange(n_matches)).astype(np.uint32) << 1) | rng.integers(0, 2, n_matches).astype(np.uint32)
    m["q_span"] = SPAN
    m["cr_off"] = np.cumsum(m["n"].astype(np.int64)) - m["n"]
    lists = [np.sort((rng.integers(0, 900, int(n)).astype(U) << U(1)) | rng.integers(0, 2, int(n)).astype(U)) for n in m["n"]]
    return dict(name=f"B-heap-{n_matches}", read=(3 * n_matches + 40, m, np.concatenate(lists)), na=int(m["n"].sum()), heap=True, runs=None, kb=None, idb=None, reorder=None)


# ---- C: key widths --------------------------------------------------------------------------------------------------------------------------------------------------
def width_case(na, b0, b1, bs, long_run=0, tag=""):
    """na anchors whose x differ in exactly b0 position bits, b1 target-id bits and bs strand bits; long_run: one run of that many anchors, every other run short"""
    kb = b0 + b1 + bs
    rng = np.random.default_rng(8000 + 100 * kb + na + long_run)
    n_sites = min(1 << kb, max(2, int(0.7 * (na - long_run))))
    sites = _sites(rng, n_sites, b0, b1, bs, ends=True)
    mult = np.ones(n_sites, np.int64)
    if long_run:
        mult[n_sites // 2] = long_run
    extra = na - int(mult.sum())
    assert extra >= 0
    others = np.delete(np.arange(n_sites), n_sites // 2) if long_run else np.arange(n_sites)
    np.add.at(mult, rng.choice(others, extra), 1)
    return _case(f"C-kb{kb}-na{na}{tag}", 8500 + 100 * kb + na + long_run, sites, mult, kb=kb, idb=max(1, (na - 1).bit_length()),
                 reorder=(long_run,) if long_run else ())


KB_FIELDS = {1: (1, 0, 0), 8: (8, 0, 0), 9: (8, 0, 1), 16: (16, 0, 0), 17: (16, 0, 1), 24: (22, 2, 0), 25: (22, 2, 1), 31: (29, 2, 0), 32: (29, 2, 1), 33: (29, 3, 1)}


def set_c_kb():
    return [width_case(3000, *KB_FIELDS[kb]) for kb in sorted(KB_FIELDS)] + [width_case(16384, 31, 0, 1), width_case(16384, 31, 1, 1)]


def set_c_sum():
    """kb + idb = 64 and 65: the last one-word key and the first read sorted as whole anchors.  About 2 000 anchors (idb 11) and about 20 000 (idb 15); 65 with every run
    shorter than 224 and with one run of 224; 2 048 against 2 049 anchors, where one more anchor moves idb from 11 to 12"""
    return [width_case(2000, 31, 21, 1), width_case(2000, 31, 22, 1), width_case(2000, 31, 22, 1, long_run=224, tag="-run224"),
            width_case(20000, 31, 17, 1), width_case(20000, 31, 18, 1), width_case(20000, 31, 18, 1, long_run=224, tag="-run224"),
            width_case(2048, 31, 21, 1), width_case(2049, 31, 21, 1)]


# ---- D: bucket structure, from the bytes of x --------------------------------------------------------------------------------------------------------------------
def xb(*bytes_hi_to_lo):
    """x from its eight bytes, highest first (byte 3 holds position bits 24 .. 30: below 128)"""
    assert len(bytes_hi_to_lo) == 8 and bytes_hi_to_lo[4] < 128
    v = 0
    for b in bytes_hi_to_lo:
        v = v << 8 | int(b)
    return v


def _d_case(name, seed, x_fill, **kw):
    x_fill = np.array(x_fill, U)
    case = dict(name=name, read=read_from_x(x_fill, seed), na=int(x_fill.size), runs=runs_of(np.sort(x_fill)), kb=None, idb=None, reorder=())
    case.update(kw)
    return case


def _low(rng, top, n, k):
    """n x with the top byte `top` and a lowest byte below k, at random: equal keys found at the lowest byte only"""
    return [xb(top, 0, 0, 0, 0, 0, 0, int(b)) for b in rng.integers(0, k, n)]


def set_d():
    rng = np.random.default_rng(9000)
    cases = []
    for third in (False, True):
        tag, extra, dg = ("three", [xb(0x40, 0, 0, 0, 0, 0, 0, 9)], {0x40: 1}) if third else ("two", [], {})
        # one side holds a single record, standing in the middle of the other side's range
        a = _low(rng, 0, 400, 6)
        fill = a[:200] + [xb(0x80, 0, 0, 0, 0, 0, 0, 1)] + extra + a[200:]
        cases.append(_d_case(f"D-{tag}-single", 9010 + third, fill, top=(56, {0: 400, 0x80: 1, **dg})))
        # no record misplaced, one x on either side: the reference has nothing to reorder
        fill = [xb(0, 0, 0, 0, 0, 0, 0, 5)] * 200 + extra + [xb(0x80, 0, 0, 0, 0, 0, 0, 5)] * 150
        cases.append(_d_case(f"D-{tag}-none", 9020 + third, fill, top=(56, {0: 200, 0x80: 150, **dg}), reorder=None))
        # every record misplaced: the upper side first
        fill = _low(rng, 0x80, 300, 6) + extra + _low(rng, 0, 300, 6)
        cases.append(_d_case(f"D-{tag}-all", 9030 + third, fill, top=(56, {0: 300, 0x80: 300, **dg})))
    # sub-buckets of exactly 64 and 65 records with equal keys inside
    fill = _low(rng, 0, 64, 3) + _low(rng, 1, 65, 3) + [xb(2, 0, 0, 0, 0, 0, 1, b) for b in range(30)] + _low(rng, 3, 150, 4)
    cases.append(_d_case("D-sub-64-65", 9040, rng.permutation(np.array(fill, U)), top=(56, {0: 64, 1: 65, 2: 30, 3: 150}), nodes=[(0, {0: None, 1: None, 2: None})]))
    # keys that differ in the lowest byte only: the first pass that moves anything has shift 0
    fill = [xb(0x80, 0, 0, 1, 2, 3, 4, int(b)) for b in rng.integers(0, 256, 1000)]
    cases.append(_d_case("D-low-byte", 9050, fill, top=(0, None)))
    # digit 255 occupied, digit 0 empty, long gaps of empty digits between 3, 130 and 255
    fill = _low(rng, 3, 170, 8) + _low(rng, 130, 160, 8) + _low(rng, 255, 170, 8)
    cases.append(_d_case("D-digit-255", 9060, rng.permutation(np.array(fill, U)), top=(56, {3: 170, 130: 160, 255: 170})))
    # equal keys only inside one bucket of 65 records at the lowest byte, under differing bytes at every level above
    main = [xb(1, 1, 1, 1, 1, 1, 1, int(b)) for b in rng.integers(0, 3, 65)]
    side = []
    for level in range(7):                                                       # byte 7 (level 0) .. byte 1: forty records that leave the main group at that byte
        for k in range(40):
            b = [1] * level + [2] + [0] * (6 - level) + [k]
            side.append(xb(*b))
    nodes = [(56 - 8 * level, {1: 65 + 40 * (6 - level), 2: 40}) for level in range(7)]
    cases.append(_d_case("D-deep", 9070, rng.permutation(np.array(main + side, U)), top=nodes[0], nodes=nodes[1:] + [(0, {0: None, 1: None, 2: None})]))
    return cases


# ---- E: encoding --------------------------------------------------------------------------------------------------------------------------------------------------
def _enc_read(qlen, rows, seed):
    """rows: (end position of the minimizer, strand, span, segment id, tandem bit); two hits each, one per strand, at random reference positions"""
    rng = np.random.default_rng(seed)
    m = np.zeros(len(rows), ob.MATCH_DTYPE)
    for k, (end, strand, span, seg, tandem) in enumerate(rows):
        assert 0 <= end - span + 1 and end < qlen
        m[k] = (2 * k, 2, end << 1 | strand, span, seg << 1 | tandem)
    pos = rng.integers(0, 400, 2 * len(rows)).astype(U)                          # few positions: equal x under different spans and segments
    hits = (U(1) << U(32)) | (pos << U(1)) | (np.arange(2 * len(rows)).astype(U) & U(1))
    return qlen, m, hits


def set_e():
    big = 2**31 - 1
    rng = np.random.default_rng(9500)
    segs = [(s, t) for s in (0, 1, 127, 255) for t in (0, 1)]
    rows = []
    for span in range(1, 256):
        seg, tandem = segs[span % 8]
        rows.append((int(rng.integers(span - 1, big)), span & 1, span, seg, tandem))
    for strand in (0, 1):
        for k, span in enumerate((1, 15, 255)):
            rows.append((span - 1, strand, span, *segs[(k + strand) % 8]))       # the minimizer that starts at the first query position
            rows.append((big - 1, strand, span, *segs[(k + 3 + strand) % 8]))    # the one that ends at the last
    rows.sort()
    one = (40, np.array([(0, 1, 20 << 1 | 1, 15, 0)], ob.MATCH_DTYPE), np.array([5 << 32 | 77 << 1], U))
    reads = [_enc_read(big, rows, 9501), _enc_read(1, [(0, 0, 1, 255, 1), (0, 1, 1, 1, 0)], 9502),
             _enc_read(15, [(0, 0, 1, 0, 0), (14, 0, 15, 127, 1), (14, 1, 15, 1, 1), (14, 1, 1, 255, 0)], 9503), one]
    return [dict(name=f"E-{k}", read=r, na=int(r[1]["n"].sum()), runs=None, kb=None, idb=None, reorder=None) for k, r in enumerate(reads)]


# ---- the epilogue's use of the same replay: chains that start at equal x ------------------------------------------------------------------------------------------
def tandem_task(n_chains, seed):
    """n_chains chains of four anchors, two (once three, for an odd count) at each locus sharing their reference positions -- a tandem repeat in the query: the same x,
    query positions 6 000 apart --, so that chains start at equal x; loci 20 000 apart"""
    rng = np.random.default_rng(seed)
    copies = [2] * (n_chains // 2 - 1) + [2 + n_chains % 2]
    x, y = [], []
    for g, c in enumerate(copies):
        for k in range(c):
            q0 = 1000 + k * 6000 + int(rng.integers(0, 50))
            for s in range(4):
                x.append(1 << 32 | (100000 + g * 20000 + 20 * s))
                y.append(SPAN << 32 | (q0 + 20 * s))
    a = np.stack((np.array(x, U), np.array(y, U)), 1)
    return np.ascontiguousarray(a[np.argsort(a[:, 0], kind="stable")])


TANDEM_CHAINS = (64, 65, 768, 769)
