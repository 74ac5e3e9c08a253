"""tests/coop_limit_data.py does what it says: asserted from the oracle's f / p and tests/coop_model.py alone, without a GPU.  These are conditions on the inputs of
tests/test_gpu_coop_limits.py -- an input that does not put an anchor AT the limit it names tests nothing."""
import time

import numpy as np
import pytest

import coop_limit_data as cd
import coop_model as cm
from helpers import oracle_batch
from reuse_data import batch


def _oracle(P, tasks):
    a, off = batch(tasks)
    f, p = oracle_batch(P, off, a)
    return [(f[off[k]:off[k + 1]], p[off[k]:off[k + 1]]) for k in range(len(tasks))]


def check_tasks(tasks, n_max=6000):
    for t in tasks:
        assert t.dtype == np.uint64 and 0 < t.shape[0] <= n_max and t.shape[1] == 2
        assert np.all(t[1:, 0] >= t[:-1, 0]), "a task must be sorted by x"


# ---- 1. the rank test
def _rank_conditions(P, t, f, p, info, max_skip):
    """per unit: near_T == r, argmax_T == B where the builder says it is, p == argmax up to r = max_skip + 1; returns the targets where the `break` fired first, and those
    of them with max_skip + 2 nearer candidates whose B is the farthest candidate of all"""
    T, B, r, where, origin = (info[k] for k in ("T", "B", "r", "where", "origin"))
    broke, lone = [], []
    for o in np.unique(origin):                                      # (one origin per task, or one per unit when tiles are counted from the pieces)
        m = origin == o
        end = int(T[m].max()) + 1
        c = cm.classify(P, t[o:end], f[o:end], tile0=0)
        Tm, Bm = T[m] - o, B[m] - o
        assert np.array_equal(c["near"][Tm], r[m]), (max_skip, c["near"][Tm], r[m])
        assert np.array_equal(c["argmax"][Tm], Bm) and np.array_equal(c["where"][Tm], where[m])
        ok = r[m] <= max_skip + 1
        pp = np.where(p[o:end] >= 0, p[o:end] - o, -1)                # (p counts from the task's start)
        assert np.array_equal(pp[Tm[ok]], Bm[ok]), "up to max_skip + 1 nearer candidates the scan reaches the best one"
        differs = pp[Tm] != c["argmax"][Tm]
        assert np.array_equal(differs, ~ok), "from max_skip + 2 on the break fires first"
        others = np.setdiff1d(np.nonzero(~cm.short_cut_holds(P, c))[0], Tm)
        assert others.size == 0, "only the targets fail the rank test"
        broke += list(T[m][differs])
        lone += list(T[m][differs & (c["ncand"][Tm] == r[m] + 1) & (r[m] == max_skip + 2)])
    return np.array(broke), np.array(lone)


@pytest.mark.parametrize("max_skip", cd.RANK_SKIPS)
def test_rank_case_puts_targets_on_both_sides_of_max_skip_plus_one(max_skip):
    P, tasks, info = cd.rank_case(max_skip)
    check_tasks(tasks)
    assert P.max_skip == max_skip and P.max_skip < P.max_iter and len(tasks) == 3
    for where, (t, (f, p), I) in enumerate(zip(tasks, _oracle(P, tasks), info)):
        assert (I["where"] == where).all() and sorted(set(I["r"] - max_skip)) == [0, 1, 2, 3]
        broke, lone = _rank_conditions(P, t, f, p, I, max_skip)
        assert broke.size >= 8, (where, broke.size)                  # per position: targets whose p differs from the window's best
        assert where != cd.DEEP or lone.size >= 2                    # deep, and the candidate count less one IS the rank: max_skip + 2 there
        n = t.shape[0]
        per_tile = np.bincount(broke // 64, minlength=(n + 63) // 64)
        full = per_tile[:n // 64]
        assert (full == 1).sum() >= 1                                # a full tile of 63 anchors that pass and one that does not (the straight-line pushes hand it to the walk)
        assert n % 64 != 0 and per_tile[-1] == 1                     # ... and a partial last tile that holds one


@pytest.mark.parametrize("max_skip", cd.RANK_SKIPS)
def test_rank_case_as_one_task_counts_tiles_from_each_piece(max_skip):
    P, (t,), (I,) = cd.cut_rank_case(max_skip)
    check_tasks([t], 12000)
    (f, p), = _oracle(P, [t])
    x = cm.fields(t)[0]
    starts = 1 + np.nonzero(np.diff(x) > P.max_dist_x)[0]            # where a cut at every empty window starts a piece
    assert np.isin(I["origin"], starts).all() and (starts % 64 != 0).all() and starts.size == I["T"].size
    broke, lone = _rank_conditions(P, t, f, p, I, max_skip)
    assert lone.size >= 2
    for where in (cd.OWN, cd.BEFORE, cd.DEEP):
        assert np.isin(broke, I["T"][I["where"] == where]).sum() >= 8


# ---- 2. the window edge
@pytest.mark.parametrize("bw", cd.EDGE_BW)
@pytest.mark.parametrize("max_iter", cd.EDGE_ITERS)
def test_edge_case_has_a_best_candidate_one_anchor_outside_and_the_last_one_inside(max_iter, bw):
    P, (t,), I = cd.edge_case(max_iter, bw)
    check_tasks([t])
    assert (P.max_iter, P.bw, P.max_dist_x) == (max_iter, bw, (1 << 20) + 2) and min(P.max_dist_x, P.max_dist_y) - 1 >= bw
    (f, p), = _oracle(P, [t])
    x, q, span = cm.fields(t)
    n = t.shape[0]
    assert np.array_equal(cm.window_starts(P, x), np.maximum(np.arange(n) - max_iter, 0)), "every window is bounded by max_iter"
    B, out, inside = I["B"], I["out"], I["inside"]
    assert B.size >= 8 and out.max() < n
    assert (np.diff(np.sort(B % 64)) > 0).sum() >= 5                 # the beacons' tile phases differ
    c0, c1 = cm.classify(P, t, f), cm.classify(P, t, f, extend=1)
    # the last anchor inside: it is the window's best and the oracle takes it
    assert np.array_equal(p[inside], B) and np.array_equal(c0["argmax"][inside], B) and np.array_equal(c0["st"][inside], B)
    # one anchor outside: it passes every pair filter (the window opened by one anchor takes it), the oracle does not
    assert np.array_equal(c1["argmax"][out], B) and np.array_equal(c0["st"][out], B + 1)
    assert (p[out] != B).all() and (c1["argmax"][out] != p[out]).sum() >= 8


# ---- 3. the dealing of rows
DEAL_ALL = cd.DEAL_SMALL + cd.DEAL_LARGE + cd.DEAL_EXTRA


@pytest.mark.parametrize("wn", DEAL_ALL)
def test_deal_case_best_candidates_lie_in_every_part_of_the_window(wn):
    P, (t,), I = cd.deal_case(wn)
    check_tasks([t])
    n = t.shape[0]
    assert n >= 4300 and P.max_iter == wn and P.max_skip >= wn
    x = cm.fields(t)[0]
    st = cm.window_starts(P, x)
    assert np.array_equal(st, np.maximum(np.arange(n) - wn, 0)), "uniform windows"
    (f, p), = _oracle(P, [t])
    i = np.nonzero(p >= 0)[0]
    dist = i - p[i]
    assert (f[I["beacons"]] == cd.SPAN).all() and I["beacons"].size >= 12
    assert (dist == wn).sum() >= 4, "the last anchor of a window is the best of several anchors"
    lanes = np.unique((i % 64)[dist > wn - 64])
    assert lanes.size >= 40, "... and the anchors at the far end of a window are the best ones of most lanes of a tile"
    assert np.unique((dist - 1) * 8 // wn).size == 8, "best candidates in every eighth of the window"
    c1 = cm.classify(P, t, f, extend=1)
    assert ((c1["argmax"] != p) & (c1["argmax"] == c1["st"] - 1)).sum() >= 2, "an anchor one before the window that would be the best"
    for W in (16, 8):
        ranges, tiles = cm.deal(n, st, wn, W)
        per = np.array([pr for _, pr, _ in tiles])
        full = [n_all for t0, _, n_all in tiles if t0 >= wn]
        rows_full = min(wn, 64 * (cm.NX - 1 + (cm.FAR_TILES if wn > 960 else 0))) - 64     # rows of phase A1 for a tile whose windows lie inside the task
        assert set(full) == ({rows_full} if rows_full else set()), (wn, W)
        first_block = 38 if W == 8 else 80                           # rows at which a helper's static block reaches a group of four
        assert ((per > 0).any()) == (wn - 64 >= first_block), (wn, W, per.max())
        if wn - 64 < first_block:
            assert (per == 0).all()                                  # every row from the counter
        # every row of every tile is dealt exactly once
        for t0, _, n_all in tiles[:3] + tiles[-3:]:
            rows = np.concatenate([np.arange(jz, ja) for tt, _, _, ja, jz, _ in ranges if tt == t0])
            assert rows.size == n_all and np.unique(rows).size == n_all


def test_deal_cases_cross_the_wrap_of_the_candidate_rings_with_every_kind_of_range():
    for W in (16, 8):
        seen = set()
        mixed = {}
        pers = set()
        for wn in DEAL_ALL:
            n = cd.DEAL_N
            st = np.maximum(np.arange(n) - wn, 0)
            ranges, tiles = cm.deal(n, st, wn, W)
            pers |= {pr > 0 for _, pr, _ in tiles}
            for t0, kind, unit, ja, jz, edge in ranges:
                if cm.crosses_wrap(ja, jz):
                    seen.add((kind, edge))
            el = cm.eligible(n, st, wn)[:n // 64 * 64].reshape(-1, 64)
            mixed[wn] = int((el.any(1) & ~el.all(1)).sum())
        assert ("block", False) in seen and ("group", False) in seen, (W, seen)
        assert ("block", True) in seen or ("group", True) in seen, (W, seen)           # an edge segment
        assert pers == {True, False}
        assert mixed[1217] > 0 and mixed[1279] > 0 and mixed[1216] == 0 and mixed[1280] == 0, mixed
        assert all(mixed[wn] == 0 for wn in cd.DEAL_SMALL + (959, 960, 961, 1215))


# ---- 4. ties
def test_tie_case_places_equal_scores_in_every_pair_of_places():
    P, (t,), I = cd.tie_case()
    check_tasks([t])
    (f, p), = _oracle(P, [t])
    n = t.shape[0]
    x = cm.fields(t)[0]
    st = cm.window_starts(P, x)
    assert np.array_equal(st, np.maximum(np.arange(n) - cd.TIE_ITER, 0)) and np.array_equal(np.diff(x), np.ones(n - 1, np.int64))
    c = cm.classify(P, t, f)
    deals = {W: cm.deal(n, st, cd.TIE_ITER, W)[0] for W in (16, 8)}

    def owner(W, T, j):
        t0 = T & ~63
        if j >= t0: return ("own",)
        if j >= t0 - 64: return ("before",)
        hit = [(kind, unit) for tt, kind, unit, ja, jz, _ in deals[W] if tt == t0 and jz <= j < ja]
        assert len(hit) == 1, (W, T, j, hit)
        return hit[0]
    kinds = [u[0] for u in I["units"]]
    assert all(kinds.count(k) == cd.TIE_REPS for k in cd.TIE_PLACES)
    for kind, T, near, far in I["units"]:
        if kind in cd.TIE_PLACES:
            assert c["nmax"][T] == 2 and c["ncand"][T] == 2 and p[T] == near == c["argmax"][T] and near > far, (kind, T)
            assert f[near] == f[far] == cd.SPAN and f[T] > cd.SPAN
            for W in (16, 8):
                a, b = owner(W, T, near), owner(W, T, far)
                want = {"own-own": a == b == ("own",), "own-older": a == ("own",) and b == ("before",), "before-deeper": a == ("before",) and b[0] == "block",
                        "two-blocks": a[0] == b[0] == "block" and a != b, "same-block": a[0] == "block" and a == b, "counter-group": a[0] == "block" and b[0] == "group"}[kind]
                assert want, (kind, W, a, b)
        elif kind.startswith("span-tie"):
            assert p[T] == -1 and f[T] == cd.SPAN and c["tie_span"][T] and c["ncand"][T] == 1, (kind, T)
            for W in (16, 8):
                assert owner(W, T, near)[0] == {"own": "own", "before": "before", "block": "block", "counter": "group"}[kind[9:]], (kind, W)
        else:
            assert kind.startswith("plus-one")
            assert p[T] == near and f[T] == cd.SPAN + 1 and f[near] == 1 and c["ncand"][T] == 1, (kind, T, f[T])     # f[j] + span == span + 1: beats the span by exactly one
            if kind == "plus-one-edge":
                assert near == st[T]
    assert sum(k.startswith("span-tie") for k in kinds) >= 3 and sum(k.startswith("plus-one") for k in kinds) >= 4


# ---- 5. equal x across a tile edge
def test_eqx_case_runs_cross_a_tile_edge_and_would_chain_without_the_dr_test():
    P, (t,), I = cd.eqx_case()
    check_tasks([t])
    (f, p), = _oracle(P, [t])
    x = cm.fields(t)[0]
    for first, m in zip(I["first"], I["m"]):
        assert 2 <= m <= 70 and (x[first:first + m] == x[first]).all() and x[first - 1] < x[first] and x[first + m] > x[first]
        assert (first + m - 1) // 64 == first // 64 + 1, "the run starts in one tile and ends in the next"
    c = cm.classify(P, t, f, allow_dr0=True)
    differs = np.nonzero(c["argmax"] != p)[0]
    assert differs.size >= 8
    in_run = np.zeros(t.shape[0], bool)
    for first, m in zip(I["first"], I["m"]):
        in_run[first + 1:first + m] = True
    assert in_run[differs].all() and (x[c["argmax"][differs]] == x[differs]).all()      # ... each time the equal-x anchor before it
    assert np.array_equal(cm.classify(P, t, f)["argmax"] != p, np.zeros(t.shape[0], bool))  # (with the test in place the window's best is what the oracle takes: no break here)


# ---- the long tasks of the device cut
@pytest.mark.parametrize("bw", cd.EDGE_BW)
def test_edge_case_as_one_task_of_parts_behind_x_jumps(bw):
    for max_iter in cd.EDGE_ITERS:
        P, (t,), I = cd.cut_edge_case(max_iter, bw)
        check_tasks([t], 20000)
        x = cm.fields(t)[0]
        starts = 1 + np.nonzero(np.diff(x) > P.max_dist_x)[0]
        assert np.array_equal(starts, I["starts"][1:]) and (starts % 64 != 0).all() and starts.size == cd.CUT_PARTS - 1
        (f, p), = _oracle(P, [t])
        assert np.array_equal(p[I["inside"]], I["B"]) and (p[I["out"]] != I["B"]).all() and I["B"].size >= 8 * (cd.CUT_PARTS - 1)
        assert np.array_equal(cm.window_starts(P, x)[I["out"]], I["B"] + 1)          # (one anchor outside, in every part)


def test_zz_the_module_builds_in_under_twenty_seconds():
    """every builder once more, from nothing, and the oracle over the largest input"""
    t0 = time.perf_counter()
    for ms in cd.RANK_SKIPS:
        P, tasks, _ = cd.rank_case(ms)
        cd.cut_rank_case(ms)
    _oracle(P, tasks)
    for mi in cd.EDGE_ITERS:
        for bw in cd.EDGE_BW:
            cd.edge_case(mi, bw)
            cd.cut_edge_case(mi, bw)
    for wn in cd.DEAL_SMALL + cd.DEAL_LARGE + cd.DEAL_EXTRA:
        P, tasks, _ = cd.deal_case(wn)
    _oracle(P, tasks)
    cd.tie_case(); cd.eqx_case()
    took = time.perf_counter() - t0
    print(f"coop limit data: every builder in {took:.1f} s")
    assert took < 20.0, took
