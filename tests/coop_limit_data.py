"""Seeded inputs that put anchors AT the limits of the several-waves DP (csrc/chain_dp_coop.h): the rank test of its short cut, the window edge of its pair rows, the
dealing of rows to its helper waves and the wrap of its candidate rings, ties between candidates in different parts of its look-back, and runs of equal x across a
tile edge.  tests/test_gpu_coop_limits.py runs them against the oracle; tests/test_cpu_coop_limit_data.py shows, from the oracle and tests/coop_model.py alone, that
each one holds the anchors it names.  Every builder returns (P, [tasks], info).

Two ways of making an anchor nobody's candidate are used throughout (chain.c:202-203: dq <= 0 or dq > max_dist_y fails):
  fillers   q far above every other anchor's (2^28 and falling by one per filler): they occupy indices -- tile phases, depths of look-back -- and have f = span, p = -1;
  falling q a stream whose q falls as x rises: no anchor is a predecessor of a later one.  A BEACON B in such a stream is an anchor whose q lies below the stream's, on
            the diagonal of the stream anchor `focus` indices after it: the stream anchors behind it see it with dq > 0 and |dr - dq| growing by 2 .. 4 per anchor
            of distance from that focus -- so each beacon is the best candidate of the anchors about `focus` behind it, wherever in their window that is."""
import numpy as np

from reuse_data import task_of

INT32_MAX = 2**31 - 1
SPAN = 15
FILL_Q = 1 << 28
OWN, BEFORE, DEEP = 0, 1, 2


class _Lay:
    """anchors appended in index order with x never falling; fillers and padding to a tile phase"""
    def __init__(self, x0=1 << 20):
        self.x, self.q, self.s = [], [], []
        self.xc = x0

    @property
    def n(self):
        return len(self.x)

    def put(self, x, q, span=SPAN):
        assert x >= self.xc and q >= 0
        self.x.append(int(x)); self.q.append(int(q)); self.s.append(int(span)); self.xc = int(x)
        return self.n - 1

    def fill(self, k):
        for _ in range(k):
            self.put(self.xc + 1, FILL_Q - self.n)

    def pad_to(self, phase, origin=0):
        self.fill((phase - (self.n - origin)) % 64)

    def task(self):
        t = task_of(self.x, self.q, self.s)
        assert np.array_equal((t[:, 0] & np.uint64(0xffffffff)).astype(np.int64), np.array(self.x))      # (already in order: indices stay)
        return t


# ---- 1. the rank test
RANK_SKIPS = (0, 1, 3, 25)
RANK_CHAIN = 40            # anchors of the main chain: f[B] = 600, above any decoy chain's (at most 28 decoys: 420)
RANK_REPS = 5


def _rank_unit(L, rng, r, where, piece_relative, last, lone=False):
    """gap | padding | main chain .. B | fillers (DEEP) | r decoys | T | padding to the end of T's tile.  B = (xb, qb); decoy k = (xb + F + 16 k, qb + F + 16 k + 2 d): a chain of
    its own, 2 d > bw off the main chain's diagonal; T = (xb + a, qb + a + d) with a = F + 16 r + d + 20: d off B's diagonal and d off the decoys', behind all of them.
    lone: the main chain's last link is 4 900 long, so that B is the only anchor of it within T's reach -- T has r + 1 candidates and B is the farthest (the bound that the
    kernel has on the rank of a deep candidate, the candidate count less one, is then the rank itself)."""
    d = int(rng.integers(251, 501))
    F = int(rng.integers(128, 150)) if where == DEEP else 0
    kT = int(rng.integers(r + 1, 63)) if where == OWN else int(rng.integers(0, r + 1)) if where == BEFORE else int(rng.integers(0, 63))
    L.xc += 6000                                                   # beyond max_dist_x: the unit's first anchor has an empty window
    origin = L.n if piece_relative else 0                          # tiles counted from the piece that a cut at the empty window starts
    L.pad_to(kT - (RANK_CHAIN + F + r), origin)
    qb0 = 1000
    for k in range(1, RANK_CHAIN + 1):
        step = 4900 if lone and k == RANK_CHAIN else 20
        qb0 += step - 20
        L.put(L.xc + step, qb0 + 20 * k)
    B, xb, qb = L.n - 1, L.xc, qb0 + 20 * RANK_CHAIN
    L.fill(F)
    for k in range(1, r + 1):
        L.put(xb + F + 16 * k, qb + F + 16 * k + 2 * d)
    a = F + 16 * r + d + 20
    T = L.put(xb + a, qb + a + d)
    assert (T - origin) % 64 == kT
    if not last:
        L.pad_to(0, origin)
    return T, B, origin


def rank_case(max_skip, piece_relative=False):
    """Three tasks -- B in T's own tile, in the tile before, two or more tiles back -- of RANK_REPS units for each r = max_skip .. max_skip + 3 decoys; the last unit of a
    task has r = max_skip + 3 and ends the task inside a tile; in every other unit of the third task B is the farthest of T's candidates.  piece_relative: ONE task of all of them, tile phases counted from each unit's first anchor (where a cut
    on the device starts a piece), preceded by 37 fillers so that no piece starts at a multiple of 64.  info: per task the arrays T, B, r, where, origin."""
    from mm2chain import params
    rng = np.random.default_rng(9100 + max_skip + (50 if piece_relative else 0))
    P = params.make_params(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=max_skip, max_iter=5000)
    tasks, info = [], []
    L = _Lay()
    if piece_relative:
        L.fill(37)
    rows = []
    for where in (OWN, BEFORE, DEEP):
        if not piece_relative:
            L, rows = _Lay(), []
        rs = [max_skip + k for _ in range(RANK_REPS) for k in range(4)]
        for u, r in enumerate(rs):
            T, B, origin = _rank_unit(L, rng, r, where, piece_relative, last=u == len(rs) - 1 and (where == DEEP or not piece_relative),
                                      lone=where == DEEP and (u // 4) % 2 == 1)
            rows.append((T, B, r, where, origin))
        if not piece_relative:
            assert L.n % 64 != 0
            tasks.append(L.task()); info.append({k: np.array([row[c] for row in rows]) for c, k in enumerate(("T", "B", "r", "where", "origin"))})
    if piece_relative:
        tasks.append(L.task()); info.append({k: np.array([row[c] for row in rows]) for c, k in enumerate(("T", "B", "r", "where", "origin"))})
    return P, tasks, info


# ---- falling-q streams with beacons
def _stream(rng, n, extra, q0):
    """x rising by 1 .. 3, q falling by 1, for n + extra anchors (the extra ones only place beacons whose focus lies behind the task's end)"""
    x = (1 << 20) + np.cumsum(rng.integers(1, 4, n + extra))
    q = q0 - np.arange(n + extra)
    return x, q


def _beacon_q(x, q, b, focus):
    """q of a beacon at index b on the diagonal of stream anchor b + focus, with dq == dr there"""
    return q[b + focus] - (x[b + focus] - x[b])


# ---- 2. the window edge
EDGE_ITERS = (1, 3, 4, 5, 63, 64, 65, 66, 67, 127, 128, 129)
EDGE_BW = (500, (1 << 20) - 1, 1 << 20)
EDGE_BEACONS = 12


def edge_case(max_iter, bw, seed=0):
    """One task: a falling-q stream (every window is bounded by max_iter: max_dist_x = 2^20 + 2 is wider than the task) with EDGE_BEACONS major beacons of span 255 and
    focus max_iter + 1 -- the stream anchor max_iter + 1 behind a beacon passes every pair filter with it (dd = 0, dq = dr) and has it one anchor before its window,
    the one max_iter behind has it as the last anchor inside -- and minor beacons of span 15 with any focus, kept only where no beacon is another's candidate:
    every beacon has f = span.  info: B (the majors), out = B + max_iter + 1, inside = B + max_iter."""
    from mm2chain import params
    rng = np.random.default_rng(9200 + 7 * max_iter + seed * 1000 + bw % 13)
    P = params.make_params(max_dist_x=(1 << 20) + 2, max_dist_y=(1 << 20) + 2, bw=bw, max_skip=INT32_MAX, max_iter=max_iter)
    gaps = max_iter + 2 + rng.integers(3, 60, EDGE_BEACONS)
    B = 5 + np.cumsum(gaps) - gaps[0]
    n = int(B[-1]) + max_iter + 2 + int(rng.integers(1, 50))
    x, q = _stream(rng, n, max_iter + 2, 40000)
    span = np.full(n, SPAN)
    for b in B:
        q[b] = _beacon_q(x, q, b, max_iter + 1); span[b] = 255
    taken = set(B.tolist()) | set((B + max_iter).tolist()) | set((B + max_iter + 1).tolist())
    beacons = sorted(B.tolist())
    for b in np.nonzero(rng.random(n) < 0.2)[0]:
        if int(b) in taken:
            continue
        qb = _beacon_q(x, q, b, int(rng.integers(1, max_iter + 2)))
        near = [c for c in beacons if 0 < b - c <= max_iter + 1 or 0 < c - b <= max_iter + 1]
        # (kept only if it is nobody's predecessor among the beacons and has none among them: q not above an earlier beacon's, not below a later one's)
        if all((qb <= q[c]) if c < b else (q[c] <= qb) for c in near):
            q[b] = qb; beacons.append(int(b)); beacons.sort()
    t = task_of(x[:n], q[:n], span)
    return P, [t], {"B": B, "out": B + max_iter + 1, "inside": B + max_iter}


# ---- 3. the dealing of rows
DEAL_SMALL = tuple(64 + k for k in (0, 1, 7, 8, 9, 37, 38, 79, 80, 81))
DEAL_LARGE = (959, 960, 961, 1215, 1216, 1217, 1279, 1280, 1281)
DEAL_EXTRA = (200, 500)    # with eight waves none of the sizes above splits an EDGE segment at the rings' wrap (the counter's groups end on multiples of eight there); these do
DEAL_N = 4369              # 68 tiles and 17 anchors: ranges of every kind on both sides of 2 048 and 4 096


def deal_focuses(wn):
    """the focuses the beacons of deal_case take in turn: the window's last anchor and the anchors around it, then down the window in steps of 120 (a beacon is the
    best candidate of the anchors up to about 160 on either side of its focus)"""
    return [wn + 2, wn, wn + 1, wn - 1] + ([wn - 120 * m for m in range(1, wn // 120 + 1) if wn - 120 * m > 0] if wn >= 300 else [wn // 2 + 1, wn // 4 + 1, 3])


def deal_case(wn):
    """One task of DEAL_N anchors with uniform windows of wn anchors (max_iter = wn; x rises by 1 .. 3, max_dist_x = 5 000 is wider than 1 281 * 3): a falling-q stream with a
    beacon for every 230 anchors or so, the focuses of deal_focuses in turn, so that the best candidate of an anchor lies now at the far end of its window -- the last anchor
    inside, then one anchor outside -- now anywhere down to its near end, for runs of consecutive anchors (every lane of a tile).  A beacon that would be another's
    candidate is left out: every beacon has f = span.  max_skip = INT_MAX: no anchor fails the rank test."""
    from mm2chain import params
    rng = np.random.default_rng(9300 + wn)
    P = params.make_params(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=INT32_MAX, max_iter=wn)
    x, q = _stream(rng, DEAL_N, wn + 3, 30000)
    focuses, kept = deal_focuses(wn), []
    for k, target in enumerate(range(70, DEAL_N + wn - 100, 230)):
        focus = focuses[k % len(focuses)]
        b = target + int(rng.integers(0, 64)) - focus
        if b < 0 or b >= DEAL_N or b in kept:
            continue
        qb = _beacon_q(x, q, b, focus)
        rel = [(x[max(b, c)] - x[min(b, c)], (qb - q[c]) if c < b else (q[c] - qb)) for c in kept if abs(b - c) <= wn + 1]
        if all(dq <= 0 or dq > 5000 or abs(dr - dq) > 500 for dr, dq in rel):
            q[b] = qb; kept.append(b)
    assert q[:DEAL_N].min() > 0
    return P, [task_of(x[:DEAL_N], q[:DEAL_N], np.full(DEAL_N, SPAN))], {"beacons": np.array(sorted(kept))}


# ---- 4. ties
TIE_ITER = 1000            # uniform windows of 1 000 anchors: 936 rows of phase A1 per tile -- static blocks of 44 (sixteen waves) / 100 (eight), the rest from the counter
TIE_PLACES = ("own-own", "own-older", "before-deeper", "two-blocks", "same-block", "counter-group")
TIE_REPS = 3


def tie_case():
    """One task, x rising by exactly 1 (dr = distance in anchors), fillers everywhere but for the units: a target T and its candidates, each unit's q 20 000 below the unit
    before it (no pair across units passes).  Spans 15, bw = 40.
      tied pair   candidates at distance a1 on the diagonal d above T's (dq = a1 + d) and at a2 on the one d below (dq = a2 - d >= 15), 20 < d <= 40: both isolated
                  (2 d > bw apart), both give T 15 + 15 - gap(d); placed by TIE_PLACES relative to T's tile start t0 and to j1 = t0 - 64
      span tie    one candidate of span 3 (f = 3) at |dr - dq| = 14: 3 + 15 - gap(14) = 15 == span, p stays -1
      plus one    one candidate of span 1 on T's diagonal at a distance of 15 or more: f + span = 1 + 15 == best + 1, the last row the score bound may not skip
    info: list of (kind, T, near candidate, far candidate or -1)."""
    from mm2chain import params
    rng = np.random.default_rng(9400)
    P = params.make_params(max_dist_x=5000, max_dist_y=5000, bw=40, max_skip=25, max_iter=TIE_ITER)
    cells, units = {}, []
    qbase = [3000000]

    def unit(kind, t0, kT, cands):
        """cands: (distance from T, diagonal offset: dq = dr + off, span); a distance whose index is taken moves one further back"""
        T = t0 + kT
        qT = qbase[0]; qbase[0] -= 20000
        assert T not in cells
        cells[T] = (qT, SPAN)
        js = []
        for a, off, span in cands:
            while T - a in cells:
                a += 1
            assert a + off >= (15 if span == SPAN else 1) and T - a >= 0
            cells[T - a] = (qT - (a + off), span); js.append(T - a)
        units.append((kind, T, js[0], js[1] if len(js) > 1 else -1))

    t0 = 64 * 17
    for rep in range(TIE_REPS):
        for kind in TIE_PLACES:
            d = int(rng.integers(21, 41)) * (1 if rng.random() < 0.5 else -1)       # which of the two is on the upper diagonal (dq = dr + |d|)
            j1 = t0 - 64
            kT = 63 if kind == "own-own" else int(rng.integers(58, 64)) if kind == "own-older" else int(rng.integers(0, 64))
            near, far = {"own-own": (t0 + 47 - rep, t0 + 3 + rep), "own-older": (t0 + 1 + rep, t0 - 30), "before-deeper": (t0 - 30 + rep, j1 - 100),
                         "two-blocks": (j1 - 10 - rep, j1 - 150), "same-block": (j1 - 10, j1 - 30 - rep), "counter-group": (j1 - 10 - rep, j1 - 800 - 9 * rep)}[kind]
            a1, a2 = t0 + kT - near, t0 + kT - far
            if d < 0 and a1 < 16 - d:                                                # (the one on the lower diagonal needs dq = dr - |d| >= 15)
                d = -d
            assert a1 >= 16 and a2 >= 16 + abs(d)
            unit(kind, t0, kT, [(a1, d, SPAN), (a2, -d, SPAN)])
            t0 += 128
    # span ties: a candidate of span 3 (f = 3) at |dr - dq| = 14, dq >= 15: 3 + 15 - gap(14) = 3 + 15 - 3 == 15
    for kind, kT, a in (("span-tie-own", 40, 30), ("span-tie-before", 5, 35), ("span-tie-block", 9, 9 + 64 + 20), ("span-tie-counter", 9, 9 + 64 + 800)):
        unit(kind, t0, kT, [(a, -14, 3)])
        t0 += 128
    for kind, a in (("plus-one-own", 20), ("plus-one-before", 40), ("plus-one-block", 64 + 10 + 30), ("plus-one-counter", 64 + 800 + 30), ("plus-one-edge", TIE_ITER)):
        unit(kind, t0, 30, [(a, 0, 1)])
        t0 += 128
    n = t0 - 64 + 23
    x = (1 << 20) + np.arange(n)
    q = FILL_Q - np.arange(n)
    span = np.full(n, SPAN)
    for idx, (qq, ss) in cells.items():
        q[idx] = qq; span[idx] = ss
    return P, [task_of(x, q, span)], {"units": units}


# ---- 5. equal x across a tile edge
EQX_RUNS = (2, 3, 17, 40, 64, 65, 70, 2, 33, 70)


def eqx_case():
    """One task of units: gap | padding | a chain of 20 anchors (steps of 20, span 15) to E | a run of m anchors of span 255 with ONE x, 200 behind E, and q rising by 20 from
    200 behind E's | five more chain anchors.  The run starts in one tile and ends in the next.  Anchor k of the run gets f[E] + 200 - gap(20 k) from E (nothing from k > 25:
    beyond bw) -- and would get f[k - 1] - gap(20), far more, from the run anchor before it if dr == 0 did not fail chain.c:202.  info: first, m per run."""
    from mm2chain import params
    rng = np.random.default_rng(9500)
    P = params.make_params(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000)
    L = _Lay()
    first = []
    for m in EQX_RUNS:
        ks = int(rng.integers(65 - m, 64)) if m <= 64 else int(rng.integers(0, 128 - m))
        L.xc += 6000
        L.pad_to(ks - 20)
        q0 = 1000
        for k in range(1, 21):
            L.put(L.xc + 20, q0 + 20 * k)
        xe, qe = L.xc, q0 + 400
        first.append(L.n)
        assert L.n % 64 == ks and (L.n + m - 1) // 64 == L.n // 64 + 1
        for k in range(m):
            L.put(xe + 200, qe + 200 + 20 * k, 255)
        for k in range(1, 6):
            L.put(xe + 200 + 20 * k, qe + 200 + 20 * (m - 1) + 20 * k)
    return P, [L.task()], {"first": np.array(first), "m": np.array(EQX_RUNS)}


# ---- one long task for the cut on the device
def cut_rank_case(max_skip):
    """rank_case as ONE task whose units are pieces of their own (every unit starts behind an x jump beyond max_dist_x), tile phases counted from the piece"""
    return rank_case(max_skip, piece_relative=True)


CUT_PARTS = 5


def cut_edge_case(max_iter, bw, parts=CUT_PARTS):
    """`parts` edge tasks of one (max_iter, bw), drawn with seeds of their own, as ONE task: each part 2^20 + 3 + a few in x behind the part before it (beyond max_dist_x), at
    offsets that are no multiples of 64.  info: B / out / inside in the task's indices, and the parts' first anchors."""
    P = None
    ts, info, starts, base = [], {"B": [], "out": [], "inside": []}, [], 0
    for s in range(parts):
        P, (t,), i = edge_case(max_iter, bw, seed=s + 1)
        while (base + t.shape[0]) % 64 == 0:
            t = t[:-1]
        t = t.copy()
        t[:, 0] += np.uint64(s * ((1 << 21) + 11))
        keep = i["out"] < t.shape[0]
        for k in info:
            info[k].append(i[k][keep] + base)
        starts.append(base)
        ts.append(t); base += t.shape[0]
    assert all(s % 64 for s in starts[1:])
    x = np.concatenate(ts)[:, 0]
    assert np.all(np.diff(x.astype(np.int64)) > 0) and int(x.max() & np.uint64(0xffffffff)) < (1 << 31)
    return P, [np.concatenate(ts)], dict({k: np.concatenate(v) for k, v in info.items()}, starts=np.array(starts))
