"""Seeded inputs for the score-bound exit of the tile kernel's hand-written loop (csrc/chain_dp_tile.h, MM2C_EXIT_TEST; the model: tests/tile_model.py).
tests/test_cpu_score_exit.py shows on the CPU, from the oracle and the model alone, that each input holds what it is named for; tests/test_gpu_score_exit.py runs
the same inputs through the library."""
import numpy as np

from reuse_data import task_of

SPAN = 15
FILL_Q = 1 << 28
SKIPS = (1, 3, 25)
FORMS = {"32-bit ring of 8 tiles": (False, 8), "compact ring of 16 tiles": (True, 16)}


def _stream(profile, n_reads, n_per, seed, **kw):
    from mm2chain import synth
    off, a = synth.make_stream(profile, n_reads, n_per, seed=seed, **kw)
    off, a = off.numpy(), a.numpy().view(np.uint64)
    return [a[off[k]:off[k + 1]] for k in range(n_reads)]


def fold_and_stream_tasks():
    """the inputs of test_model_of_the_hand_written_loop_reaches_every_label (tests/test_cpu_oracle.py): the fold drivers, two mixed reads, one dense window"""
    from helpers import fold_driver_tasks
    rng = np.random.default_rng(4242)
    tasks = fold_driver_tasks(rng, shapes=((1100, 4, 0.05, 0.15), (2000, 3, 0.0, 0.3), (700, 12, 0.2, 0.15), (500, 40, 0.0, 0.2)))
    return tasks + _stream("mixed", 2, 700, seed=5) + _stream("dense", 1, 1600, seed=8, locus=5000)


def tile_path_tasks(seed=27502):
    """the generator of test_tile_kernel_paths (tests/test_gpu_parity.py) at its shorter shapes: runs of equal x shorter and longer than a tile, spans 8 - 40"""
    rng = np.random.default_rng(seed)
    tasks = []
    for n, dup, dens in [(700, 0.0, 1), (900, 0.3, 1), (1300, 0.9, 2), (130, 0.97, 1), (1000, 0.2, 10)]:
        step = np.where(rng.random(n) < dup, 0, rng.integers(1, 12 * dens + 2, n))
        pos = (1 << 22) + np.cumsum(step)
        q = 50 + np.cumsum(np.where(rng.random(n) < 0.15, rng.integers(-400, 400, n), rng.integers(0, 14 * dens, n)))
        span = np.where(rng.random(n) < 0.5, 15, rng.integers(8, 40, n))
        tasks.append(task_of(pos, np.maximum(q, 1), span))
    return tasks


def standard_tasks():
    return fold_and_stream_tasks() + tile_path_tasks()


# ---- the equality edge.  x rises by exactly 3 per anchor (a window of max_dist_x = 5000 holds 1 666 anchors: beyond a ring of 16 tiles), every anchor but the named
# ones is a filler (q far above everything and falling: nobody's candidate, f = span = 15, p = -1).  T (span 15) sits at position 30 of tile 17; c, six anchors before
# it in the same tile, lies 10 off T's diagonal (dr = 18, dq = 28: gap cost g = (int)(10 avg) + (ilog2(10) >> 1) = 1 + 1 for any avg in [0.1, 0.2)); j, in an older
# tile, lies ON T's diagonal, is nobody's successor and has span 30 = f[j].  c sees j 10 off its own diagonal: f[c] = 30 + span_c - 2, and T gets f[c] + 15 - 2 through c.
#   "fires"   span_c = 4: best = 45 through c == f[j] + 15, and f[j] is the largest f before T's tile: the exit is taken at equality.  Scanned, j would score exactly
#             45 and lose the tie to the nearer c (chain.c:226 is strict): f / p are what they were.
#   "holds"   span_c = 3: best = 44 through c, f[j] + 15 == best + 1 and the pair scores it (dd = 0, dr = dq >= 15): p[T] = j.  A filler of span 31 before T's tile
#             keeps the bound above the best after j is taken as well (31 + 15 > 45), so T never leaves early.
# near: j in the tile before T's (40 anchors back); far: 1 000 anchors back (dr = 3 000), beyond the ring of either form.
EDGE_T = 64 * 17 + 30
EDGE_CASES = [(kind, far) for kind in ("fires", "holds") for far in (False, True)]


def edge_case(kind, far):
    """(P, task, info): info = dict(T, c, j, best)"""
    from mm2chain import params
    assert kind in ("fires", "holds")
    P = params.make_params(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000)
    n = EDGE_T + 40
    x = (1 << 20) + 3 * np.arange(n)
    q = FILL_Q - np.arange(n)
    span = np.full(n, SPAN)
    T, c, j = EDGE_T, EDGE_T - 6, EDGE_T - (1000 if far else 40)
    qT = 3000000
    q[T] = qT
    q[c] = qT - (3 * 6 + 10); span[c] = 4 if kind == "fires" else 3
    q[j] = qT - 3 * (T - j); span[j] = 30
    if kind == "holds":
        span[T - 50] = 31
    return P, task_of(x, q, span), dict(T=T, c=c, j=j, best=45)


# ---- first tile, short last tile
def short_tasks():
    """tasks shorter than one tile, of exactly 64 / 65 / 128 anchors, and with a last tile of 1 .. 63 anchors (dense loci: every anchor has candidates)"""
    sizes = [1, 2, 40, 63, 64, 65, 127, 128, 129, 191, 200, 64 * 5 + 1, 64 * 6 + 63]
    return [_stream("dense", 1, n, seed=300 + n, locus=max(40 * n, 2000))[0] for n in sizes]


# ---- negative gap_scale: the gap cost is a gain, a pair can score more than f[j] + span, the bound does not hold and the host leaves the exit off
def negative_gap_case():
    """(P, tasks, info).  gap_scale = -2.  The first task is the far layout of the equality edge with j moved 495 off T's diagonal, to the side on which c (10 off
    it the other way, now of span 60 and lone) is 505 from j's diagonal and does not see it (bw = 500): j's gap cost to T, 78 at avg 0.15, turns into a gain of 155,
    so T scores 30 + 15 + 155 through j -- far above f[j] + span_T = 45, which the best through c (60 + 15 + 3) has long passed when the scan gets there."""
    from mm2chain import params
    P = params.make_params(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, gap_scale=-2.0)
    _, t, info = edge_case("fires", True)
    t = t.copy()
    t[info["j"], 1] += np.uint64(495)
    t[info["c"], 1] = (np.uint64(60) << np.uint64(32)) | (t[info["c"], 1] & np.uint64(0xffffffff))
    return P, [t] + _stream("mixed", 2, 900, seed=77), dict(T=info["T"], c=info["c"], j=info["j"])


# ---- a task that the plan cuts into pieces on the device (chain_cut: at least 8192 anchors, cut where a window is empty, pieces of at least 256 anchors)
CUT_SEG_MIN, CUT_MIN_ANCHORS = 256, 8192


def cut_task():
    """(P, task): eleven loci of 700 - 1 000 anchors, 10^6 apart in x (far more than max_dist_x), 9 000 anchors in all"""
    from mm2chain import params
    P = params.map_ont()
    parts, base = [], 1 << 20
    sizes = [700, 1000, 800, 900, 750, 850, 700, 1000, 800, 700, 800]
    for k, n in enumerate(sizes):
        t = _stream("mixed" if k % 2 else "dense", 1, n, seed=500 + k)[0]
        pos = (t[:, 0] & np.uint64(0xffffffff)).astype(np.int64)
        parts.append((pos - pos.min() + base, (t[:, 1] & np.uint64(0xffffffff)).astype(np.int64), ((t[:, 1] >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)))
        base = int(parts[-1][0].max()) + 1000000
    task = task_of(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
    assert task.shape[0] == sum(sizes) >= CUT_MIN_ANCHORS
    return P, task


def cut_pieces(P, task, seg_min=CUT_SEG_MIN, min_anchors=CUT_MIN_ANCHORS):
    """chain_cut (csrc/chain_kernel.hip) on the CPU: [(start, end)] of the pieces of one task -- cut at the first empty window (st[i] == i) that leaves at least
    seg_min anchors behind, then again from there"""
    n = task.shape[0]
    x64 = task[:, 0]
    D = np.uint64(P.max_dist_x)
    st = np.maximum(np.searchsorted(x64, np.where(x64 >= D, x64 - D, np.uint64(0)), side="left"), np.arange(n) - P.max_iter)
    if n < min_anchors:
        return [(0, n)]
    pieces, s0 = [], 0
    for i in range(1, n):
        if st[i] == i and i >= s0 + seg_min:
            pieces.append((s0, i)); s0 = i
    pieces.append((s0, n))
    return pieces
