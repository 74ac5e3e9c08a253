"""Seeded inputs for the parts of the tile kernel's hand-written loop (csrc/chain_dp_tile.h) that count older tiles in anchors and make the log term of the gap cost
in two instructions.  tests/test_gpu_loop_trim.py runs them through the library; every claim made here about an input is asserted there from the oracle alone.
All of them chain under ONE set of scalars (map-ont's, max_skip 3: the fold drivers' setting), so one batch and one oracle run serve every case."""
import numpy as np

from reuse_data import task_of

NX, NF = 16, 4
MAX_SKIP = 3
BW = 500
FILL_SPAN = 15
T_TILE, T_POS = 18, 30
DEPTH_T = 64 * T_TILE + T_POS

# (whole older tiles inside the window, lanes of the partly covered tile behind them).  With NX - 1 whole tiles the ring is full: a partly covered tile behind them,
# and everything of the two cases with NX and NX + 1 whole tiles, comes from memory (the far form), where the depth goes on counting in anchors.
DEPTH_CASES = [(m, part) for m in (0, 1, NF, NF + 1, NX - 1) for part in (0, 1, 63)] + [(NX, 20), (NX + 1, 0)]


def depth_task(m, part):
    """(task, info).  x rises by one per anchor from anchor lo = 64 (T_TILE - m) - part on and lies 10 000 lower before it, so the window of every anchor of tile T_TILE
    starts exactly at lo (max_dist_x = 5 000): it holds the anchor's own-tile predecessors, m whole older tiles and `part` lanes of the tile before those.  T, at position
    T_POS of the tile, is the only anchor with candidates: one at position 10 of its own tile, one at position 40 of every whole older tile, and -- the deepest -- the
    LAST anchor of the window (lane part - 1 of the partly covered tile, or anchor lo itself: lane 63 of the deepest whole tile when part is 0, position 0 of the own tile
    when there is no older tile).  The candidates share one q, dq = 0 between them, so none sees another: each is lone, f = its span, p = -1 (no stamp, no mark, no `break`).
    That q lies C = dr(deepest) - 1 below T's: the deepest has dd = 1 and no gap cost, a nearer one dd = C - dr and a smaller span, and one more than bw off T's diagonal is
    filtered.  The deepest is T's best, every scored chunk on the way raises the best with its one lane (fold B0), and p[T] is made from the depth the scan has reached.
    Every other anchor is a filler: q falls by one per anchor from above everything else (nobody's successor: dq < 0; nobody's predecessor: dq > max_dq)."""
    T, i0 = DEPTH_T, 64 * T_TILE
    lo = i0 - 64 * m - part
    assert lo >= 0
    n = T + 40
    x = (1 << 20) + np.arange(n)
    x[:lo] -= 10000
    qT = 100000
    q = qT + n + 6000 - np.arange(n)
    span = np.full(n, FILL_SPAN)
    q[T] = qT
    span[T] = 40
    cands = [(0, i0 + 10)] + [(d, i0 - 64 * d + 40) for d in range(1, m + 1)]
    deepest = (m + 1 if part else m, lo)
    cands = [c for c in cands if c[1] > lo] + [deepest]
    C = (T - lo) - 1
    for d, j in cands:
        q[j] = qT - C
        span[j] = 20 + 10 * d
    return task_of(x, q, span), dict(T=T, lo=lo, cands=cands, deepest=lo, depth=deepest[0])


# ---- folds B1 and B1M (one / several lanes beat the best, no mark, no skip so far) at a chosen depth
PAIR_CASES = [(m, kind) for m in (0, 1, NF + 1) for kind in ("b1", "b1m")]


def pair_task(m, kind):
    """(task, info).  depth_task(m, 0) with two candidates only, the last two anchors of the window (lanes 62 and 63 of the deepest whole tile; positions 1 and 0 of the
    own tile for m = 0).  j2, the deeper, is the deepest of depth_task: dd = 1, span 100.  j1, the nearer and so the first surviving lane of the chunk, lies 40 further
    from T's diagonal (a gap cost of 6 to 8) and does not see j2 (dq < 0).  "b1": j1 has span 2 and scores below T's own span of 40 -- one lane beats the best and it is not
    the first: fold B1.  "b1m": j1 has span 50 and beats the best, j2 beats j1: two candidates, the first not the maximum -- the prefix maximum without marks (Lb1m).
    p[T] = j2 either way."""
    assert kind in ("b1", "b1m")
    T, i0 = DEPTH_T, 64 * T_TILE
    lo = i0 - 64 * m
    n = T + 40
    x = (1 << 20) + np.arange(n)
    x[:lo] -= 10000
    qT = 100000
    q = qT + n + 6000 - np.arange(n)
    span = np.full(n, FILL_SPAN)
    q[T] = qT
    span[T] = 40
    C = (T - lo) - 1
    q[lo] = qT - C; span[lo] = 100
    q[lo + 1] = qT - C - 40; span[lo + 1] = 2 if kind == "b1" else 50
    return task_of(x, q, span), dict(T=T, j1=lo + 1, j2=lo)


# ---- pairs at chosen distances from the diagonal
DD_VALUES = (0, 1, 2, 3, 4, 8, 16, 32, 64, 128, 256, BW - 1, BW, BW + 1)     # every power of two up to bw, bw itself, and one beyond it (filtered)


DD_SPAN_J = 200        # f[j]: above any gap cost inside the band, so that T takes j at every dd <= bw


def dd_task():
    """(task, pairs): pairs = [(T, j, dd, sign)].  Groups 20 000 apart in x (far more than max_dist_x: a window never leaves its group).  A group is j, then `fill` fillers, then
    T, with dr = 600 between j and T and dq = 600 + sign * dd; fill = 0 puts j next to T (own tile, unless a tile boundary falls between them), fill = 70 at least one tile
    boundary between them (a ring tile).  Fillers as in depth_task.  j is lone with f = DD_SPAN_J: f[T] = DD_SPAN_J + min(dq, dr, span) - cost(dd) and p[T] = j for dd <= bw; f[T] = span, p[T] = -1 for dd = bw + 1."""
    xs, qs, spans, pairs, at = [], [], [], [], 0
    for g, (dd, sign, fill) in enumerate((dd, sign, fill) for fill in (0, 70) for dd in DD_VALUES for sign in ((1,) if dd == 0 else (1, -1))):
        x0 = (1 << 20) + 20000 * g
        xs += [x0] + [x0 + 1 + k for k in range(fill)] + [x0 + 600]
        qs += [1000] + [40000 - k for k in range(fill)] + [1000 + 600 + sign * dd]
        spans += [DD_SPAN_J] + [FILL_SPAN] * (fill + 1)
        pairs.append((at + fill + 1, at, dd, sign))
        at += fill + 2
    return task_of(np.array(xs), np.array(qs), np.array(spans)), pairs


def gap_cost(dd, avg, gap_scale=1.0):
    """chain.c:209,218-219 for one segment"""
    lg = int(dd).bit_length() - 1 if dd else 0
    c = int(np.float32(dd) * np.float32(avg)) + (lg >> 1)
    return c if gap_scale == 1.0 else int(float(c) * float(np.float32(gap_scale)) + .499)


# ---- an equal-x run that reaches back over a tile boundary
EQ_RUN = (126, 130)


def eq_run_task():
    """A dense locus of 300 anchors in which anchors 126 .. 130 share one x.  127 (position 63 of tile 1) has a run of one behind it, inside its tile: the loop takes it
    and drops that lane.  128, 129 and 130 (positions 0 .. 2 of tile 2) end runs that reach into the tile before: the loop hands each to the C++ scan and takes over
    again at 131."""
    import score_exit_data as sx
    t = sx._stream("dense", 1, 300, seed=4711, locus=12000)[0].copy()
    t[EQ_RUN[0]:EQ_RUN[1] + 1, 0] = t[EQ_RUN[0], 0]
    assert np.all(np.diff(t[:, 0].astype(np.int64)) >= 0)
    return t


SHORT_SIZES = (1, 63, 64, 65, 128, 129)


def short_tasks():
    import score_exit_data as sx
    return [sx._stream("dense", 1, n, seed=300 + n, locus=max(40 * n, 2000))[0] for n in SHORT_SIZES]


def exit_then_stamp_task():
    """one mixed read of 700 anchors: in it a fold B0 leaves through the score-bound exit before any stamp of its chunk and the NEXT anchor, in the same tile, has a chunk
    that stamps (tests/test_gpu_loop_trim.py asserts it from the model's events)"""
    import score_exit_data as sx
    return sx._stream("mixed", 1, 700, seed=5)[0]


def all_tasks():
    """(tasks, index): index names the first task of each group in the batch"""
    from tile_loop_harness import label_tasks
    tasks, index = [], {}
    index["depth"] = len(tasks); tasks += [depth_task(m, part)[0] for m, part in DEPTH_CASES]
    index["pair"] = len(tasks); tasks += [pair_task(m, kind)[0] for m, kind in PAIR_CASES]
    index["dd"] = len(tasks); tasks.append(dd_task()[0])
    index["fold"] = len(tasks); tasks += label_tasks()[1]
    index["short"] = len(tasks); tasks += short_tasks()
    index["eq"] = len(tasks); tasks.append(eq_run_task())
    index["exit"] = len(tasks); tasks.append(exit_then_stamp_task())
    return tasks, index
