"""Reads, lookup tables and sequence lists that put the device sketch, the minimizer lookups (csrc/sketch.hip) and the index build (csrc/index_build.hip,
build_index / cal_max_occ in csrc/mm2chain_sketch.cpp) at the limits of their lanes (tests/test_gpu_sketch_limits.py runs them;
tests/test_cpu_sketch_limit_data.py asserts, from the models alone, that each one reaches the limit it names).  Seeded and deterministic.

The lanes.  sk_push / sk_slots give a lane CH = 64 positions; the k-mer registers and the step counter l of a later lane exist only through two segmented
scans (PushOp, LOp).  sk_select gives a lane SC = 256 SLOTS (an ambiguous base, or a step whose k-mer is not symmetric), and rebuilds min / min_pos from the w
slots before its first.  The HPC span walks back over the bases and is cut at SPAN_CUT = 256.  lk_reads folds rep_len ROUND = 64 minimizers at a time.  The index
build's first sort takes y_bits(n_seqs) bits of y.

A sketch case is a dict: name, family, reads (bytes each), kwh = (k, w, hpc), facts (which limit it reaches, computed while building it).  cases(setting) are
the cases of one (k, w, hpc); batch(setting) is all their reads in one list with the range of every case.  lookup_cases() carry a key table each, index_lists()
the sequence lists of the build, occ_tables() the made indexes of cal_max_occ.

`lanes_sketch`, `collect_matches_v`, `build_index_v` and `max_occ_v` restate the device's way of computing (per lane, per round, per sort) in Python with ONE
deliberate error switched on at a time (ERRORS): the CPU test names, for every error, the cases whose output it changes.  Without an error they equal the
literal models (sketch_model.py, index_model.py), which stay untouched.

Three things the reading for these cases settled, each asserted by the CPU test:
  * an LOp that does not saturate l changes nothing below 2^32 steps: sk_slots caps l again at the lane's first step ('l_unsat' is caught by no case);
  * '>=' for '>' in the rep_len fold changes nothing: touching intervals have the same total merged or apart ('rep_ge' is caught by no case), so the
    error that the round cases guard against is the fold's state lost between two rounds of 64 ('rep_round_reset');
  * two minimizers of one key have one t, so a kept minimizer cannot have a repetitive equal neighbour; the case kept instead is a kept minimizer whose
    neighbours in the KEPT list share its key while its neighbours in the unfiltered list do not (tandem == 0).
With w = 255, k = 28 no slot before 281 can have l == w + k - 1: that setting has the first-window slots 511, 512, 513 only.  A period of 100 repeated 30
times over every offset 0 ... 255 would alone exceed the batch cap; it takes every 16th offset, the period of 3 every offset.  A period of 3 repeated 40
times is the minimum of a 255-slot window only by luck (none of 256 random reads had a tie across a lane): there the unit is the one of the 64 whose k-mers
hash lowest and the flanks are drawn so that no k-mer of theirs hashes below it.  b"AT" * n under even k has k - 1 slots, not none: the registers are not
symmetric before they are full.  With w = 1 the k-mer before an N is never pushed, so two consecutive minimizers are never exactly one base apart: the
'apart' pairs are minimizers j - k - 1 and j."""
import functools
import itertools

import numpy as np

import index_model as im
import sketch_model as sm

CH, SC, SPAN_CUT, ROUND = 64, 256, 256, 64
ALL1 = sm.ALL1
INT32_MAX = 2**31 - 1
SETTINGS = [(15, 10, 0), (16, 10, 0), (28, 255, 0), (19, 5, 1), (5, 3, 1), (15, 1, 0)]
CAP_BASES = 400_000
ACGT = np.frombuffer(b"ACGT", np.uint8)
NT4 = bytes(sm.nt4(b) for b in range(256))
ERRORS = ("clear_at_n", "span_255", "span_257", "rebuild_gt", "no_first_window", "l_noreset", "l_unsat",
          "tandem_across_reads", "rep_ge", "rep_round_reset", "mid_le", "y_bits_short", "occ_rank_up", "occ_rank_down")


def y_bits(n_seqs):
    """the bits of y that the build's first sort takes: 32 + max(bits_for(n_seqs - 1), 1)"""
    return 32 + max(int(n_seqs - 1).bit_length(), 1)


# ---- the device's way, restated with one error at a time ----------------------------------------------------------------------------------------------------------
def slots(seq, k, w, hpc, err=None, light=False):
    """sk_push + sk_slots: x, y, l of every slot of one read and the position that wrote it.  l at a lane's first position is what LOp's scan hands over.
    light: l and the positions only (x = y = all ones)"""
    s = bytes(seq).translate(NT4)
    n = len(s)
    mask, shift1, cap = (1 << 2 * k) - 1, 2 * (k - 1), w + k
    cut = {"span_255": 255, "span_257": 257}.get(err, SPAN_CUT)
    km0 = km1 = l = carried = lane_l = 0
    lane_reset = True
    X, Y, L, P = [], [], [], []
    for i in range(n):
        if i % CH == 0:
            if i > 0:
                if err == "l_noreset":
                    carried = min(carried + lane_l, cap)
                elif err == "l_unsat":
                    carried = lane_l if lane_reset else carried + lane_l
                else:
                    carried = lane_l if lane_reset else min(carried + lane_l, cap)
                l = carried
            lane_l, lane_reset = 0, i == 0
        c = s[i]
        if hpc and c < 4 and i + 1 < n and s[i + 1] == c:
            continue
        x = y = ALL1
        if c < 4:
            km0 = (km0 << 2 | c) & mask
            km1 = km1 >> 2 | (3 ^ c) << shift1
            if km0 == km1:
                continue
            l = min(l + 1, cap)
            lane_l = min(lane_l + 1, cap)
            if l >= k and not light:
                span = k
                if hpc:
                    runs, cc, span, q = 1, c, 0, i
                    while q >= 0 and span < cut:
                        cq = s[q]
                        if cq >= 4:
                            break
                        if cq != cc:
                            runs += 1
                            if runs > k:
                                break
                            cc = cq
                        span += 1
                        q -= 1
                if span < cut:
                    z = 0 if km0 < km1 else 1
                    x = sm.hash64(km1 if z else km0, mask) << 8 | span
                    y = (i & 0xFFFFFFFF) << 1 | z
        else:
            l = lane_l = 0
            lane_reset = True
            if err == "clear_at_n":
                km0 = km1 = 0
        X.append(x); Y.append(y); L.append(l); P.append(i)
    return X, Y, L, P


def select(X, Y, L, w, k, err=None):
    """sk_select: every lane of SC slots rebuilds min / min_pos from the w slots before it and runs the loop of sketch.c:109-137 over its own"""
    ns, wk, out = len(X), w + k, []
    for a in range(0, ns, SC):
        b = min(a + SC, ns)
        mx = my = ALL1
        mpos = 0
        if a > 0:
            for t in range(a - w, a):
                x = ALL1 if t < 0 else X[t]
                if (mx > x) if err == "rebuild_gt" else (mx >= x):
                    mx, my, mpos = x, (ALL1 if t < 0 else Y[t]), t % w
        for t in range(a, b):
            bp, ix, iy, l = t % w, X[t], Y[t], L[t]

            def buf(jj):
                q = t - (bp - jj) % w
                return (ALL1, ALL1) if q < 0 else (X[q], Y[q])
            if l == wk - 1 and mx != ALL1 and not (err == "no_first_window" and t == a and a > 0):
                for jj in itertools.chain(range(bp + 1, w), range(0, bp)):
                    e = buf(jj)
                    if mx == e[0] and e[1] != my:
                        out.append(e)
            if ix <= mx:
                if l >= wk and mx != ALL1:
                    out.append((mx, my))
                mx, my, mpos = ix, iy, bp
            elif bp == mpos:
                if l >= wk - 1 and mx != ALL1:
                    out.append((mx, my))
                mx = ALL1
                for jj in itertools.chain(range(bp + 1, w), range(0, bp + 1)):
                    e = buf(jj)
                    if mx >= e[0]:
                        mx, my, mpos = e[0], e[1], jj
                if l >= wk - 1 and mx != ALL1:
                    for jj in itertools.chain(range(bp + 1, w), range(0, bp + 1)):
                        e = buf(jj)
                        if mx == e[0] and my != e[1]:
                            out.append(e)
        if b == ns and mx != ALL1:
            out.append((mx, my))
    return out


def lanes_sketch(seq, k, w, hpc, err=None):
    """the sketch of one read the device's way: uint64 [n, 2]"""
    X, Y, L, _ = slots(seq, k, w, hpc, err)
    return np.array([(x & ALL1, y) for x, y in select(X, Y, L, w, k, err)], dtype=np.uint64).reshape(-1, 2)


def collect_matches_v(minis, lookup, mid_occ, err=None):
    """lk_lookup / lk_emit / lk_reads over a batch (minis: one uint64 [n, 2] per read): [(matches, rep_len, mini_pos)] per read, as sm.collect_matches"""
    out = []
    flat = [int(m[i][0]) >> 8 for m in minis for i in range(len(m))]
    at = 0
    for m in minis:
        n = len(m)
        rep_st = rep_en = rep_len = 0
        matches, mini_pos = [], []
        for i in range(n):
            x, y = int(m[i][0]), int(m[i][1])
            q_pos, q_span = y & 0xFFFFFFFF, x & 0xFF
            cr, t = lookup(x >> 8)
            if err == "rep_round_reset" and i % ROUND == 0 and i > 0:
                rep_len += rep_en - rep_st
                rep_st = rep_en = 0
            if not ((t <= mid_occ) if err == "mid_le" else (t < mid_occ)):
                en = (q_pos >> 1) + 1
                st = en - q_span
                if (st >= rep_en) if err == "rep_ge" else (st > rep_en):
                    rep_len += rep_en - rep_st
                    rep_st, rep_en = st, en
                else:
                    rep_en = en
            else:
                g = at + i
                lo, hi = (0, len(flat)) if err == "tandem_across_reads" else (at, at + n)
                tandem = int((g > lo and flat[g - 1] == x >> 8) or (g < hi - 1 and flat[g + 1] == x >> 8))
                matches.append((cr if t else 0, t, q_pos, q_span, (y >> 32) << 1 | tandem))
                mini_pos.append(q_span << 32 | q_pos >> 1)
        out.append((matches, rep_len + rep_en - rep_st, mini_pos))
        at += n
    return out


def build_index_v(mini, n_seqs, err=None):
    """index_sort + the grouping: two stable sorts, on the low y_bits(n_seqs) bits of y, then on the key.  mini: index_model.sketch_refs' rows"""
    bits = y_bits(n_seqs) - (1 if err == "y_bits_short" else 0)
    key, y = mini[:, 0] >> np.uint64(8), mini[:, 1]
    o1 = np.argsort(y & np.uint64((1 << bits) - 1), kind="stable")
    o2 = np.argsort(key[o1], kind="stable")
    key, y = key[o1][o2], y[o1][o2]
    keys, first, n = np.unique(key, return_index=True, return_counts=True)
    return keys.astype(np.uint64), first.astype(np.int64), n.astype(np.uint32), np.ascontiguousarray(y, dtype=np.uint64)


def max_occ_v(n, frac, err=None):
    """cal_max_occ: the rank (uint32_t)((1. - f) * n_keys), f a float widened to double, of the sorted counts, plus 1"""
    n = np.asarray(n)
    if not frac > 0 or n.size == 0:
        return INT32_MAX
    i = int((1.0 - float(np.float32(frac))) * n.size) + {"occ_rank_up": 1, "occ_rank_down": -1}.get(err, 0)
    i = min(max(i, 0), n.size - 1)
    return min(int(np.sort(n.astype(np.int64))[i]) + 1, INT32_MAX)


# ---- building blocks ----------------------------------------------------------------------------------------------------------------------------------------------
def _rng(S, *more):
    return np.random.default_rng([2031, *S, *more])


def rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def nohp(rng, n, not_first=None):
    """n random bases without two equal neighbours (under HPC every base is then a step); the first one is not `not_first` (a code 0-3)"""
    out = np.empty(n, np.int64)
    prev = not_first
    for i in range(n):
        c = int(rng.integers(0, 4))
        while c == prev:
            c = int(rng.integers(0, 4))
        out[i] = prev = c
    return ACGT[out].tobytes()


def code(b):
    return sm.nt4(b)


def revcomp(s):
    return bytes(s)[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def _flank(S, rng, n, not_first=None):
    return nohp(rng, n, not_first) if S[2] else rnd(rng, n)


def _unit(S, rng, p):
    """a tandem unit of period p; under HPC without equal neighbours, also across the junction"""
    if not S[2] and p > 2:
        return rnd(rng, p)
    while True:
        u = nohp(rng, p)
        if u[0] != u[-1]:
            return u


def n_slots(seq, S):
    return len(slots(seq, *S, light=True)[0])


def lane_pushes(seq, hpc):
    """nucleotides pushed into the registers by every lane of CH positions"""
    s = bytes(seq).translate(NT4)
    out = [0] * ((len(s) + CH - 1) // CH)
    for i, c in enumerate(s):
        if c < 4 and not (hpc and i + 1 < len(s) and s[i + 1] == c):
            out[i // CH] += 1
    return out


_SK = {}


def sk(S, r):
    """sketch_model.sketch of one read under a setting, computed once: the facts below and model(S) share it"""
    r = bytes(r)
    if (S, r) not in _SK:
        _SK[S, r] = sm.sketch(r, S[1], S[0], S[2])
    return _SK[S, r]


def tail_differs(read, tail, S):
    """does the model's sketch of `tail` inside `read` (its last len(tail) bases) differ from the sketch of `tail` alone -- what registers cleared at the
    ambiguous run before it would give"""
    k, w, hpc = S
    off = len(read) - len(tail)
    a = [(x, y) for x, y in sk(S, read) if y >> 1 >= off]
    b = [(x, y + 2 * off) for x, y in sm.sketch(tail, w, k, hpc)]
    return a != b


def straddles(mini, P, every=SC):
    """equal-x minimizers whose slots lie on both sides of a multiple of `every`: the number of such x.  P: the position of every slot"""
    slot_of = {p: t for t, p in enumerate(P)}
    by_x = {}
    for x, y in mini:
        by_x.setdefault(int(x), []).append(slot_of[int(y) >> 1])
    return sum(1 for v in by_x.values() if len(v) > 1 and min(v) // every != max(v) // every)


def _case(name, family, reads, S, facts):
    return {"name": name, "family": family, "reads": [bytes(r) for r in reads], "kwh": S, "facts": facts}


# ---- the sketch families -----------------------------------------------------------------------------------------------------------------------------------------
def fam_registers(S):
    k, w, hpc = S
    rng, out = _rng(S, 1), []
    if not hpc:
        for run in (1, 63, 64, 65, 128, 200):
            for off in (0, 1, 62, 63):
                pre = rnd(rng, 3 * CH + off)
                out.append(_case(f"n_run_{run}_at_{off}", "registers", [pre + b"N" * run + rnd(rng, 200 + (w if w > 200 else 0))], S,
                                 {"run": run, "in_lane": len(pre) % CH}))
        if k == 28:                                                        # lanes that push fewer than k, k and more than k nucleotides, in every order
            for perm in itertools.permutations((27, 28, 29)):
                body = b"".join(b"N" * (CH - c) + rnd(rng, c) for c in perm)
                r = rnd(rng, 2 * CH) + body + rnd(rng, 400)
                out.append(_case("push_%d_%d_%d" % perm, "registers", [r], S, {"pushes": lane_pushes(r, 0)[2:5]}))
    else:
        for run in (64, 65, 128, 129):
            r = nohp(rng, 2 * CH, 0)[::-1] + b"A" * run + nohp(rng, 300, 0)
            out.append(_case(f"hp_run_{run}", "registers", [r], S, {"run": run, "silent_lanes": sum(1 for c in lane_pushes(r, 1) if c == 0)}))
    return out


PAL_SEED = {(16, 1): 1, (28, 1): 192, (28, 64): 98, (28, 70): 65, (28, 130): 104}                                                              # (k, m): where the search below is known to end


def fam_palindrome(S):
    k, w, hpc = S
    out = []
    if k % 2 or hpc:
        return out
    for m in (1, 64, 70, 130):
        for t in range(PAL_SEED.get((k, m), 0), 200):
            rng = _rng(S, 2, m, t)
            pre, h, post = rnd(rng, 100), rnd(rng, k // 2), rnd(rng, w + k + 150)
            tail = revcomp(h) + post
            h2 = ACGT[[(code(h[0]) + 1) % 4]].tobytes() + h[1:]
            r, c = pre + h + b"N" * m + tail, pre + h2 + b"N" * m + tail
            if tail_differs(r, tail, S) and not tail_differs(c, tail, S):
                break
        out.append(_case(f"palindrome_across_{m}", "palindrome", [r], S, {"m": m, "tail": len(tail), "seed": t, "tail_differs": tail_differs(r, tail, S)}))
        out.append(_case(f"palindrome_control_{m}", "palindrome", [c], S, {"m": m, "tail": len(tail), "tail_differs": tail_differs(c, tail, S)}))
    return out


def _first_l(seq, S, after, v):
    """(position, slot) of the first slot behind position `after` whose l is v"""
    _, _, L, P = slots(seq, *S, light=True)
    for t, (l, p) in enumerate(zip(L, P)):
        if p > after and l == v:
            return p, t
    return -1, -1


def fam_l_edges(S):
    k, w, hpc = S
    rng, out = _rng(S, 3), []
    for name, v in (("k", k), ("wk1", w + k - 1), ("wk", w + k)):
        if (w == 1 and name == "wk1"):
            continue                                                       # w + k - 1 == k
        for e in (CH - 1, 0):
            q = 2 * CH + (e - v) % CH
            r = _flank(S, rng, q) + b"N" + _flank(S, rng, v + 300)
            p, _ = _first_l(r, S, q, v)
            out.append(_case(f"l_{name}_at_{e}", "l_edges", [r], S, {"l": v, "in_lane": p % CH}))
    return out


def fam_first_window(S):
    """an N w + k - 1 steps before slot 255, 256, 257 (511, 512, 513): the first-window loop (l == w + k - 1) runs there, over a tandem repeat"""
    k, w, hpc = S
    rng, out = _rng(S, 4), []
    targets = [s for s in (255, 256, 257) if s - (w + k - 1) >= 0] + ([511, 512, 513] if S == (28, 255, 0) else [])
    p = 3 if w == 255 else 2
    for s in targets:
        q = s - (w + k - 1)
        for _ in range(50):                                                # a unit whose smallest k-mer stands more than once in the first window
            r = _flank(S, rng, q) + b"N" + _unit(S, rng, p) * max(40, (w + k) // p + 20) + _flank(S, rng, 100)
            X, _, L, P = slots(r, *S)
            t = next((t for t in range(len(X)) if P[t] > q and L[t] == w + k - 1), -1)
            first = X[max(t - w + 1, 0):t]                                 # the slots in buf when the loop runs at slot t
            ties = first.count(min(first)) - 1 if first and min(first) != ALL1 else 0
            if ties > 0 or w == 1:
                break
        out.append(_case(f"first_window_at_{s}", "first_window", [r], S, {"slot": t, "window_ties": ties}))
    return out


N_SLOTS = {(15, 10, 0): (255, 256, 257, 512, 65_535, 65_536, 65_537), (19, 5, 1): (255, 256, 257, 512, 65_536)}


def fam_lag(S):
    k, w, hpc = S
    rng, out = _rng(S, 5), []
    lag = []
    if k % 2 == 0 and not hpc:
        lag = [("at_only", b"AT" * 700), ("at_flanked", rnd(rng, 100) + b"AT" * 600 + rnd(rng, 100))]
    if hpc:
        lag = [("two_runs", nohp(rng, 60, 0)[::-1] + b"A" * 500 + b"C" * 500 + nohp(rng, 60, 1))]
    for name, r in lag:
        ns = n_slots(r, S)
        out.append(_case("lag_" + name, "lag", [r], S, {"n_slots": ns, "bases": len(r), "empty_tail_lanes": -(-len(r) // SC) - -(-ns // SC)}))
    for n in N_SLOTS.get(S, (255, 256, 257, 512)):
        long_enough = rnd(rng, n * 3 // 2 + 64 if (hpc or k % 2 == 0) else n)
        P = slots(long_enough, *S, light=True)[3]
        r = long_enough[:P[n - 1] + 1]                                     # cut behind the step that writes slot n - 1
        out.append(_case(f"slots_{n}", "lag", [r], S, {"n_slots": n_slots(r, S), "bases": len(r)}))
    r = b"N" * 256
    out.append(_case("all_n_256", "lag", [r], S, {"n_slots": n_slots(r, S), "minimizers": len(sk(S, r))}))
    return out


PERIODS = {(15, 10, 0): (7, 2), (16, 10, 0): (7,), (28, 255, 0): (3, 100), (19, 5, 1): (2,), (5, 3, 1): (2,), (15, 1, 0): ()}


def _canon_hash(kmer, k):
    """the hash of a k-mer's smaller strand, as the x of its minimizer holds it"""
    a = b = 0
    for c in bytes(kmer).translate(NT4):
        a = (a << 2 | c) & ((1 << 2 * k) - 1)
        b = b >> 2 | (3 ^ c) << 2 * (k - 1)
    return sm.hash64(min(a, b), (1 << 2 * k) - 1)


def _floor(s, k):
    """the lowest hash among the k-mers of s"""
    return min(_canon_hash(s[i:i + k], k) for i in range(len(s) - k + 1))


def _quiet_flank(rng, n, before, k, floor):
    """`before` and n random bases behind it, drawn again wherever a k-mer that ends in them would hash at or below `floor`: with w = 255 a short repeat
    is the window's minimum only where its neighbourhood stays above it"""
    s = bytearray(before)
    for _ in range(n):
        for _ in range(8):
            c = b"ACGT"[int(rng.integers(0, 4))]
            if len(s) + 1 < k or _canon_hash(bytes(s[len(s) + 1 - k:]) + bytes([c]), k) > floor:
                break
        s.append(c)
    return bytes(s)


def fam_ties(S):
    """a tandem unit whose first base stands at 230 + o: every alignment of the repeat against slot 256, l saturated (no N)"""
    k, w, hpc = S
    rng, out = _rng(S, 6), []
    for p in PERIODS[S]:
        unit = _unit(S, rng, p)
        reps = 30 if p == 100 else 40
        quiet = S == (28, 255, 0) and p == 3
        if quiet:                                                          # of the 64 units the one whose k-mers hash lowest
            unit = min((bytes(u) for u in itertools.product(b"ACGT", repeat=3)), key=lambda u: _floor(u * 20, k))
        for o in range(0, max(w, 30) + 1, 16 if p == 100 else 1):
            if quiet:
                r = _quiet_flank(rng, 230 + o, b"", k, _floor(unit * 20, k)) + unit * reps
                r = _quiet_flank(rng, 60, r, k, _floor(unit * 20, k))
            else:
                r = _flank(S, rng, 230 + o) + unit * reps + _flank(S, rng, 60)
            out.append(_case(f"ties_p{p}_o{o}", "ties", [r], S, {"start": 230 + o, "straddles": straddles(sk(S, r), slots(r, *S, light=True)[3])}))
    return out


def fam_span(S):
    """the last k runs sum to T = 255, 256, 257: one long run and k - 1 single-base runs behind it"""
    k, w, hpc = S
    rng, out = _rng(S, 7), []
    if not hpc:
        return out

    def window(r, end):
        """the model's minimizers at the k steps whose last k runs hold the long run: their spans"""
        return sorted(int(x) & 0xFF for x, y in sk(S, r) if end <= y >> 1 < end + k)
    for T in (255, 256, 257):
        for off in (0, 1, 63):
            pre, singles = nohp(rng, 2 * CH + off, 0)[::-1], nohp(rng, k - 1, 0)
            r = pre + b"A" * (T - k + 1) + singles + nohp(rng, 120, code(singles[-1]))
            end = len(pre) + T - k
            out.append(_case(f"span_{T}_at_{off}", "span", [r], S, {"T": T, "in_lane": len(pre) % CH, "spans": window(r, end)}))
    pre, singles = nohp(rng, 2 * CH + 5, 0)[::-1], nohp(rng, k - 1, 0)
    r = pre + b"N" + b"A" * (255 - k + 1) + singles + nohp(rng, 120, code(singles[-1]))          # exactly k runs since the N at the last single
    out.append(_case("span_255_n_before_run", "span", [r], S, {"T": 255, "spans": window(r, len(pre) + 1 + 255 - k)}))
    r = pre + b"A" * (255 - k + 1) + singles[:k - 2] + b"N" + nohp(rng, 120)                     # the N comes before the k-th run
    out.append(_case("span_255_n_cuts_walk", "span", [r], S, {"T": 255, "spans": window(r, len(pre) + 255 - k)}))
    return out


def fam_boundary(S):
    k, w, hpc = S
    rng = _rng(S, 8)
    choice = [0, 1, k - 1, k, w + k - 2, w + k - 1, w + k, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    lens = [0, 0, 0] + [int(v) for v in rng.choice(choice, 594)] + [0, 0, 0]
    for i in (255, 256, 257):
        lens[i] = 300
    reads = [rnd(rng, L) for L in lens]
    mini = [len(sk(S, r)) for r in reads]
    facts = {"reads": len(reads), "markers": [len(reads[i]) for i in (255, 256, 257)], "lengths": len(set(lens) - {300}),
             "empty": sum(1 for L in lens if L == 0), "without_minimizers": sum(1 for m in mini if m == 0)}
    return [_case("boundary_reads", "boundary", reads, S, facts)]


FAMILIES = (fam_registers, fam_palindrome, fam_l_edges, fam_first_window, fam_lag, fam_ties, fam_span, fam_boundary)


def _long_read(S, small):
    """the other cases one after another until the slots pass 65 536 with structure around them"""
    parts = [r for c in small if c["family"] != "boundary" for r in c["reads"] if len(r) < 5000]
    target = 100_000 if (S[2] or S == (16, 10, 0)) else 75_000
    out, i = [], 0
    while sum(len(p) for p in out) < target:
        out.append(parts[i % len(parts)]); i += 1
    r = b"".join(out)
    return _case("long_read", "long", [r], S, {"bases": len(r), "n_slots": n_slots(r, S), "parts": len(out)})


@functools.lru_cache(maxsize=None)
def cases(S):
    out = [c for fam in FAMILIES for c in fam(S)]
    return out + [_long_read(S, out)]


def families(S):
    return sorted({c["family"] for c in cases(S)})


def by_name(S, name):
    return next(c for c in cases(S) if c["name"] == name)


@functools.lru_cache(maxsize=None)
def batch(S):
    """every read of the setting in one list: (reads, {case name: (first, last + 1)})"""
    reads, where = [], {}
    for c in cases(S):
        where[c["name"]] = (len(reads), len(reads) + len(c["reads"]))
        reads += c["reads"]
    return reads, where


@functools.lru_cache(maxsize=None)
def model(S):
    """sketch_model over batch(S), once: one uint64 [n, 2] per read"""
    return [np.array(sk(S, r), dtype=np.uint64).reshape(-1, 2) for r in batch(S)[0]]


def fragments(S, n_segs):
    """batch(S) cut into fragments of n_segs consecutive reads (the last one takes what is left)"""
    reads = batch(S)[0]
    return [reads[i:i + n_segs] for i in range(0, len(reads), n_segs)]


# ---- lookups ------------------------------------------------------------------------------------------------------------------------------------------------------
def _table(counts):
    """{key: n} -> (keys, cr_off, n, hits) as MinimizerIndex takes them (n = 0 rows are left out: an absent key)"""
    keys = np.array(sorted(key for key, n in counts.items() if n > 0), np.uint64)
    n = np.array([counts[int(key)] for key in keys], np.uint32)
    cr = np.concatenate([[0], np.cumsum(n.astype(np.int64))[:-1]]).astype(np.int64) if keys.size else np.zeros(0, np.int64)
    return keys, cr, n, np.arange(max(int(n.astype(np.int64).sum()), 1), dtype=np.uint64)


def _keys_of(reads, S):
    k, w, hpc = S
    return [[int(x) >> 8 for x, _ in sm.sketch(r, w, k, hpc)] for r in reads]


def lookup_model(c):
    """sm.collect_matches per read of a lookup case: [(matches, rep_len, mini_pos)]"""
    k, w, hpc = c["kwh"]
    look = sm.table_lookup(*c["table"][:3])
    return [sm.collect_matches(sm.sketch_array(r, w, k, hpc), look, c["mid_occ"]) for r in c["reads"]]


def _lookup_case(name, S, reads, counts, mid_occ, facts):
    return {"name": name, "kwh": S, "reads": [bytes(r) for r in reads], "table": _table(counts), "mid_occ": mid_occ, "facts": facts}


def _tandem_edges():
    S = (15, 10, 0)
    k, w, _ = S
    for t in range(200):
        rng = _rng(S, 10, t)
        u = rnd(rng, w + k - 1)                                            # one window: the read's first and its last minimizer are this window's
        r = u + rnd(rng, 300) + u
        keys = _keys_of([r], S)[0]
        if keys[0] == keys[-1] and keys[0] != keys[1] and keys[-1] != keys[-2]:
            break
    unit = rnd(rng, 7)
    reads = [r, r, r[:len(r) // 2], r, rnd(rng, 200) + unit * 30, unit * 30 + rnd(rng, 200), rnd(rng, k), rnd(rng, k + w + 1)]
    all_keys = _keys_of(reads, S)
    c = _lookup_case("tandem_edges", S, reads, {key: 1 for ks in all_keys for key in ks}, 2, {})
    res = lookup_model(c)
    c["facts"] = {
        "group_cut": len(reads[0]) + len(reads[1]),                        # read_chunk_bases that cuts the batch inside the [r, r, r[:len//2], r] group
        "edge_pairs": sum(1 for a, b, ra, rb in zip(all_keys, all_keys[1:], res, res[1:])
                          if a and b and a[-1] == b[0] and ra[0][-1][4] & 1 == 0 and rb[0][0][4] & 1 == 0),
        "edge_tandems": [res[4][0][-1][4] & 1, res[5][0][0][4] & 1],
        "minimizers_of_short": [len(all_keys[6]), len(all_keys[7])]}
    return c


def _tandem_unfiltered():
    """minimizers A B A B ... with B repetitive: A's neighbours in the kept list are A, in the unfiltered list B; tandem == 0"""
    S = (15, 10, 0)
    for p in range(11, 20):
        for t in range(20):
            rng = _rng(S, 11, p, t)
            r = rnd(rng, 100) + rnd(rng, p) * 20 + rnd(rng, 100)
            keys = _keys_of([r], S)[0]
            alt = [i for i in range(1, len(keys) - 3) if keys[i] == keys[i + 2] != keys[i + 1] and keys[i + 1] == keys[i + 3]]
            if len(alt) >= 4:
                b = keys[alt[0] + 1]
                c = _lookup_case("tandem_unfiltered", S, [r], {key: (2 if key == b else 1) for key in keys}, 2, {})
                m = lookup_model(c)[0][0]
                a_key = keys[alt[0]]
                kept = [key for key in keys if key != b]
                lone = [j for j in range(1, len(kept) - 1) if kept[j] == a_key == kept[j - 1] == kept[j + 1]]
                c["facts"] = {"kept_neighbours_equal": len(lone), "their_tandem": sorted({m[j][4] & 1 for j in lone}), "repetitive": keys.count(b)}
                return c
    raise AssertionError("no alternating pair of minimizers found")


def _mid_occ_cases():
    S = (15, 10, 0)
    rng = _rng(S, 12)
    reads = [rnd(rng, 400) for _ in range(6)] + [rnd(rng, 100) + rnd(rng, 7) * 30 + rnd(rng, 100), b"", rnd(rng, 14)]
    keys = _keys_of(reads, S)
    out = []
    for mid_occ, made_for in ((1, 1), (2, 2), (50, 50), (0, 1), (INT32_MAX, 50)):
        counts = {key: (made_for if key % 3 == 0 else made_for - 1) for ks in keys for key in ks}
        c = _lookup_case(f"mid_occ_{mid_occ}", S, reads, counts, mid_occ, {})
        ts = [counts[key] for ks in keys for key in ks]
        res = lookup_model(c)
        c["facts"] = {"at_mid_occ": sum(1 for t in ts if t == mid_occ), "one_below": sum(1 for t in ts if t == mid_occ - 1),
                      "kept": sum(len(m) for m, _, _ in res), "minimizers": len(ts), "rep_len": sum(rl for _, rl, _ in res)}
        out.append(c)
    return out


def _rep_len_rounds():
    """w = 1: minimizer i of a read without N ends at base i + k.  Pairs of repetitive minimizers whose later one is minimizer j of the read"""
    S = (15, 1, 0)
    k = S[0]
    rng = _rng(S, 13)
    reads, chosen, design = [], [], []
    for j in (63, 64, 65, 128):
        for kind, first in (("touch", j - k), ("overlap", j - 1), ("apart", j - k - 1)):
            reads.append(rnd(rng, 200)); chosen.append({first, j}); design.append((kind, j))
    for n in (63, 64, 65, 129):
        reads.append(rnd(rng, n + k - 1)); chosen.append(set(range(n))); design.append(("all", n))
    reads.append(rnd(rng, 150)); chosen.append(set()); design.append(("none", 0))
    keys = _keys_of(reads, S)
    counts = {key: 1 for ks in keys for key in ks}
    for ks, ch in zip(keys, chosen):
        for i in ch:
            counts[ks[i]] = 2
    c = _lookup_case("rep_len_rounds", S, reads, counts, 2, {})
    rel = []                                                               # per read: the repetitive minimizers and st - rep_en at the last of them
    for r, ks, ch in zip(reads, keys, chosen):
        rep = [i for i, key in enumerate(ks) if counts[key] >= 2]
        mini = sm.sketch(r, 1, k)
        gap = None
        if len(rep) >= 2:
            (xa, ya), (xb, yb) = mini[rep[-2]], mini[rep[-1]]
            gap = ((yb >> 1) + 1 - (xb & 0xFF)) - ((ya >> 1) + 1)
        rel.append((rep == sorted(ch), len(ks), gap))
    c["facts"] = {"design": design, "as_designed": [a for a, _, _ in rel], "minimizers": [n for _, n, _ in rel], "gap": [g for _, _, g in rel],
                  "rep_len": [rl for _, rl, _ in lookup_model(c)]}
    return c


@functools.lru_cache(maxsize=None)
def lookup_cases():
    return [_tandem_edges(), _tandem_unfiltered()] + _mid_occ_cases() + [_rep_len_rounds()]


def lookup_by_name(name):
    return next(c for c in lookup_cases() if c["name"] == name)


# ---- index build --------------------------------------------------------------------------------------------------------------------------------------------------
N_SEQS = (1, 2, 3, 4, 5, 8, 9, 256, 257, 65_536, 65_537)


@functools.lru_cache(maxsize=None)
def plant(S):
    return _flank(S, _rng(S, 20), 60)


@functools.lru_cache(maxsize=None)
def seq_list(n_seqs, S=(15, 10, 0)):
    """n_seqs sequences, all but about 40 empty or shorter than k; plant(S) in sequence 0, in the last one and in 2^m - 1 and 2^m for the top m of the list,
    at a smaller offset the larger the number: a sort that drops y's top bit puts a later sequence's hit first"""
    k = S[0]
    rng = _rng(S, 21, n_seqs)
    seqs = [b""] * n_seqs
    for i in rng.choice(n_seqs, min(n_seqs, 200), replace=False):
        seqs[int(i)] = rnd(rng, int(rng.integers(1, k)))
    for i in rng.choice(n_seqs, min(n_seqs, 36), replace=False):
        seqs[int(i)] = _flank(S, rng, int(rng.integers(80, 200)))
    at = {}
    if n_seqs > 2:
        m = int(n_seqs - 1).bit_length() - 1
        at[(1 << m) - 1], at[1 << m] = 30, 20
    at[0] = 40
    if n_seqs > 1:
        at[n_seqs - 1] = 10
    for i, off in at.items():
        seqs[i] = _flank(S, rng, off) + plant(S) + _flank(S, rng, 30)
    return tuple(seqs), tuple(sorted(at))


@functools.lru_cache(maxsize=None)
def list_minimizers(n_seqs, S=(15, 10, 0)):
    k, w, hpc = S
    return im.sketch_refs(seq_list(n_seqs, S)[0], k, w, hpc)


def planted_keys(S):
    k, w, hpc = S
    return sorted({int(x) >> 8 for x, _ in sm.sketch(plant(S), w, k, hpc)})


def list_facts(n_seqs, S=(15, 10, 0)):
    keys, cr, n, pool = im.build_from_minimizers(list_minimizers(n_seqs, S))
    spanning = ascending = 0
    for key in planted_keys(S):
        i = int(np.searchsorted(keys, np.uint64(key)))
        if i < keys.size and int(keys[i]) == key:
            rid = (pool[cr[i]:cr[i] + n[i]] >> np.uint64(32)).astype(np.int64)
            if rid[0] == 0 and rid[-1] == n_seqs - 1:
                spanning += 1
                ascending += bool(np.all(np.diff(rid) >= 0))
    lens = [len(s) for s in seq_list(n_seqs, S)[0]]
    return {"planted_in": list(seq_list(n_seqs, S)[1]), "spanning_keys": spanning, "ascending": ascending, "keys": int(keys.size), "hits": int(pool.size),
            "with_minimizers": sum(1 for L in lens if L >= S[0]), "y_bits": y_bits(n_seqs)}


def chunks(lens, lim):
    """the host's rule (build_index): a chunk takes whole sequences while its bases stay within lim, at least one sequence.  [(first, last + 1, bases)]"""
    off = np.concatenate([[0], np.cumsum(lens)])
    out, r0 = [], 0
    while r0 < len(lens):
        r1 = r0 + 1
        while r1 < len(lens) and off[r1 + 1] - off[r0] <= lim:
            r1 += 1
        out.append((r0, r1, int(off[r1] - off[r0])))
        r0 = r1
    return out


CHUNKINGS = (("a chunk of empty sequences only", 20), ("every sequence with bases its own chunk", 1), ("default", 1 << 27))


def hpc_build_seqs():
    """(19, 5, 1) over the HPC sketch cases: every read of the families, the boundary reads and the long reads left out"""
    S = (19, 5, 1)
    return [r for c in cases(S) if c["family"] not in ("boundary", "long") for r in c["reads"] if len(r) < 5000]


OCC_KEYS = (1, 2, 3, 4999, 5000, 5001, 9999, 10000, 10001)
OCC_FRACS = (2e-4, 0.25, 0.5, 1.0, 0.0)


def occ_table(n_keys):
    """a made index of n_keys keys whose counts are a permutation of 1 ... n_keys (every row starts at hit 0 of one pool of n_keys hits)"""
    rng = np.random.default_rng([2031, 30, n_keys])
    keys = (np.arange(n_keys, dtype=np.uint64) * np.uint64(7) + np.uint64(1))[rng.permutation(n_keys)]
    return keys, np.zeros(n_keys, np.int64), (rng.permutation(n_keys) + 1).astype(np.uint32), np.arange(n_keys, dtype=np.uint64)


def occ_rank(n_keys, frac):
    return int((1.0 - float(np.float32(frac))) * n_keys)
