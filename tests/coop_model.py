"""What the several-waves DP (csrc/chain_dp_coop.h) has to get right, anchor by anchor, from the oracle's f and the reference's definitions alone: the window of
chain.c:192-193, the candidates that pass chain.c:202-205, the best of them (the highest f[j] + score, nearest on ties), how many candidates lie nearer than it, and
in which tile of 64 anchors it lies.  The kernel's short cut takes that best candidate whenever at most max_skip candidates are nearer; the reference's scan may
`break` before it gets there.  tests/test_cpu_coop_limit_data.py uses this to show that tests/coop_limit_data.py puts anchors AT the boundaries; the model takes no
part in any expected value -- those are the oracle's.

deal() restates the arithmetic by which the kernel hands the rows of phase A1 (candidates of the tiles two or more back) to its helper waves -- static blocks of
`per` rows, groups of eight from a counter, either split at `jm` into rows inside every window and edge rows, every range split where the candidate rings of 2 048
anchors wrap -- only so that the CPU test can count the ranges of each kind that cross the wrap."""
import numpy as np

from wave_model import _pair_score

OWN, BEFORE, DEEP = 0, 1, 2
NX, FAR_TILES, RING = 16, 4, 2048              # csrc/chain_dp_coop.h: COOP_NX, COOP_FAR_TILES, 64 * COOP_NC


def fields(task):
    t = np.ascontiguousarray(task).view(np.uint64).reshape(-1, 2)
    x = t[:, 0].astype(np.int64)                                   # (strand and reference id above bit 32: one value, as chain.c compares it)
    q = (t[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
    span = ((t[:, 1] >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    return x, q, span


def window_starts(P, x):
    """chain.c:192-193: the first j with x[i] <= x[j] + max_dist_x, and never more than max_iter anchors back"""
    i = np.arange(x.shape[0])
    return np.maximum(np.searchsorted(x, x - P.max_dist_x, side="left"), np.maximum(i - P.max_iter, 0))


def avg_of(span):
    return float(np.float32(.01 * float(np.float32(span.sum())) / span.shape[0]))      # chain.c:48-49


def classify(P, task, f, tile0=0, extend=0, allow_dr0=False):
    """Per anchor of one task (f: the oracle's): st, argmax (-1: no candidate beats the span), near (candidates nearer than argmax), ncand, nmax (candidates at the
    best score), tie_span (some candidate's score EQUALS the span while none beats it), where (OWN / BEFORE / DEEP, -1 without argmax; tiles of 64 counted from
    anchor tile0).  extend: the window opened by so many anchors beyond its start; allow_dr0: without the test dr > 0 of chain.c:202."""
    x, q, span = fields(task)
    n = x.shape[0]
    avg = avg_of(span)
    st = window_starts(P, x)
    out = {k: np.full(n, -1, np.int64) for k in ("argmax", "where")}
    out.update({k: np.zeros(n, np.int64) for k in ("near", "ncand", "nmax")})
    out["tie_span"] = np.zeros(n, bool)
    out["st"] = st
    f = np.asarray(f, np.int64)
    for i in range(n):
        lo = max(int(st[i]) - extend, 0)
        if lo >= i:
            continue
        j = np.arange(i - 1, lo - 1, -1)                           # nearest first
        dr, dq = x[i] - x[j], q[i] - q[j]
        same = np.ones(j.shape[0], bool)
        ok, sc = _pair_score(P, avg, dr, dq, same, span[i])
        if allow_dr0:
            ok = ok | ((dr == 0) & (dq > 0) & (dq <= min(P.max_dist_x, P.max_dist_y)) & (np.abs(dr - dq) <= P.bw))
        if not ok.any():
            continue
        tot = np.where(ok, f[j] + sc, -(1 << 40))
        best = int(tot.max())
        out["ncand"][i] = int(ok.sum())
        if best <= span[i]:
            out["tie_span"][i] = best == span[i]
            continue
        k = int(np.argmax(tot == best))                            # the nearest of equal scores
        out["argmax"][i] = j[k]
        out["near"][i] = int(ok[:k].sum())
        out["nmax"][i] = int((tot == best).sum())
        ti, tj = (i - tile0) // 64, (int(j[k]) - tile0) // 64
        out["where"][i] = OWN if tj == ti else BEFORE if tj == ti - 1 else DEEP
    return out


def short_cut_holds(P, c):
    """the anchors whose best candidate is among the first max_skip + 1 of the scan (or that have none): the short cut is exact for them"""
    return (c["argmax"] < 0) | (c["near"] <= P.max_skip)


def eligible(n, st, max_iter):
    """per anchor: the kernel may try the short cut at all -- the window does not reach behind the NX - 1 + FAR_TILES tiles whose candidates phase A deals"""
    i = np.arange(n)
    i0 = i & ~63
    far = max_iter > 64 * (NX - 1)
    return ~(far & (st < i0 - 64 * (NX - 1) - 64 * FAR_TILES) & (st < i))


def deal(n, st, max_iter, W):
    """The row ranges of phase A1 for every tile t0 >= 128 of a task of n anchors with window starts st, W waves per task: a list of
    (t0, kind, unit, ja, jz, edge) for the rows [jz, ja), kind "block" (unit: the helper wave) or "group" (unit: the counter's value), and per tile (t0, per, n_all).  Ranges are listed before the split at the rings' wrap."""
    nw = W - 1
    far = max_iter > 64 * (NX - 1)
    ranges, tiles = [], []
    for t0 in range(64, n, 64):
        i0 = t0 - 64
        last = min(t0 + 63, n - 1)
        lo_first, lo_max = min(int(st[t0]), t0), min(int(st[last]), last)
        j0 = max(lo_first, t0 - 64 * (NX - 1 + (FAR_TILES if far else 0)), 0)
        j1 = i0
        if j0 >= j1:
            continue
        jm = min(max(lo_max, j0), j1)
        n_all = j1 - j0
        per = ((n_all * 3 // 4) // nw) & ~3
        jq = j1 - per * nw
        tiles.append((t0, per, n_all))

        def split(kind, unit, ja, jz):
            if ja > max(jz, jm):
                ranges.append((t0, kind, unit, ja, max(jz, jm), False))
            if min(ja, jm) > jz:
                ranges.append((t0, kind, unit, min(ja, jm), jz, True))
        for me in range(nw if per > 0 else 0):
            split("block", me, j1 - me * per, j1 - me * per - per)
        for g in range((jq - j0 + 7) >> 3):
            split("group", g, jq - 8 * g, max(jq - 8 * g - 8, j0))
    return ranges, tiles


def crosses_wrap(ja, jz):
    """rows [jz, ja) lie on both sides of a multiple of the ring size (the kernel reads them as two segments)"""
    return ((ja - 1) & ~(RING - 1)) > jz
