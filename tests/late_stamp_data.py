"""Seeded inputs for the fold order of the tile kernel's hand-written loop (csrc/chain_dp_tile.h: a chunk stamps only once its fold knows that the scan goes on; the
model: tests/tile_model.py).  tests/test_cpu_late_stamps.py shows on the CPU, from the oracle and the model alone, that each input holds what it is named
for; tests/test_gpu_late_stamps.py runs the same inputs through the library."""
import numpy as np

from reuse_data import task_of

SPAN = 15
SKIPS = (0, 1, 25)
FORMS = {"32-bit ring of 8 tiles": (False, 8, 2), "compact ring of 16 tiles, pairs": (True, 16, 2), "compact ring of 16 tiles, packed f / p": (True, 16, 4)}   # compact, NX, NF


def standard_tasks():
    import score_exit_data as sx
    return sx.standard_tasks()


# ---- windows that end a given number of tiles before the anchor's own.  x rises by exactly 1 per anchor and max_dist_x = 30 + 64 m + part: the window of T, at
# position 30 of tile 9, holds its 30 own-tile predecessors, m whole older tiles and the `part` nearest anchors of the tile before those.  Every anchor but the
# named ones is a filler: q falls by one per anchor from a value above everything else (a filler is nobody's successor, dq < 0, and nobody's predecessor, dq >
# max_dq), f = span, p = -1.  Each older tile of T's window holds ONE candidate; all candidates share one q (dq = 0 between them, chain.c:203: none sees another, each
# is lone with f = its span), C = max_dq - 1 below T's, so T sees every one of them (dd = C - dr <= bw) at a gap cost that falls with the depth while the spans
# rise with it: the DEEPEST candidate is T's best.  The scan scores a tile on either side of every tile boundary it crosses, raises the best in each (fold B0, one
# surviving lane), and makes p[T] from the depth it has reached.  The q values of a task span less than 2 000: every ring form takes it.
DEPTH_T = 64 * 9 + 30
DEPTH_CASES = [(m, part) for m in (1, 2, 3, 4, 5, 6) for part in (0, 20)]


def depth_case(m, part, gap_scale=1.0):
    """(P, task, info): info = dict(T, cands = [(depth, j)] nearest first)"""
    from mm2chain import params
    T = DEPTH_T
    D = 30 + 64 * m + part
    P = params.make_params(max_dist_x=D, max_dist_y=5000, bw=min(500, D - 1), max_skip=25, max_iter=5000, gap_scale=gap_scale)   # (max_dq - 1 >= bw: the hand-written loop's filter)
    n = T + 40
    C = D - 1
    qT = 100000
    x = (1 << 20) + np.arange(n)
    q = qT + n + D + 10 - np.arange(n)
    span = np.full(n, SPAN)
    q[T] = qT
    span[T] = 40
    cands = []
    i0 = T - 30
    for d in range(1, m + 2):
        if d == m + 1 and part == 0:
            break
        j = i0 - 64 * d + (40 if d <= m else 64 - 3)      # (the partly covered tile: inside the part that the window covers)
        assert 40 <= T - j <= D and C - (T - j) <= P.bw
        q[j] = qT - C
        span[j] = 100 + 22 * d
        cands.append((d, j))
    return P, task_of(x, q, span), dict(T=T, cands=cands)
