"""The several-waves DP (csrc/chain_dp_coop.h) at the limits of its forms: the rank test of the short cut at max_skip + 1 / + 2 nearer candidates, the window edge of its pair
rows (hand-written below bw = 2^20, C++ at it), the dealing of rows to helper waves at the 38 / 80-row thresholds of the static blocks and at 960 / 1 216 / 1 280 anchors
of look-back, the wrap of the candidate rings at multiples of 2 048 anchors, ties between candidates in different parts of the look-back, and runs of equal x across
a tile edge.  The inputs are tests/coop_limit_data.py's; tests/test_cpu_coop_limit_data.py shows from the oracle alone that each holds the anchors it names.
Everything is compared element for element with the CPU oracle, sixteen and eight waves per task, with the gap-cost table (C++ rows for the tile before and the
edges) and without (hand-written rows), and the variant text says which kernel ran."""
import numpy as np
import pytest
import torch

import coop_limit_data as cd
import oracle_binding as ob
from helpers import assert_same, gpu_batch, knobs, oracle_batch  # noqa: F401 (knobs: a fixture)
from reuse_data import batch

pytestmark = pytest.mark.gpu

FORMS = [(16, 0), (16, 1), (8, 0), (8, 1)]
FORM_IDS = ["w16", "w16-tab", "w8", "w8-tab"]


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


_CASES = {}


def case(name, *args):
    """(P, tasks, anchors, offsets, f_ref, p_ref) of one builder call: built and run through the oracle once per process, handed out read-only"""
    key = (name,) + args
    if key not in _CASES:
        P, tasks = getattr(cd, name)(*args)[:2]
        a, off = batch(tasks)
        f, p = oracle_batch(P, off, a)
        for arr in (a, off, f, p):
            arr.setflags(write=False)
        _CASES[key] = (P, tasks, a, off, f, p)
    return _CASES[key]


def run_form(knobs, c, W, tab, what):
    """one case through the cooperative kernel of W waves per task, with or without the gap-cost table; f / p against the oracle, and the kernel named"""
    P, tasks, a, off, f_ref, p_ref = c
    assert not tab or P.bw <= 511, "the table holds |dr - dq| up to 511"
    knobs("coop_plans", 1)
    knobs("coop_w8_above", 0 if W == 8 else 256)
    knobs("force_tab", tab)
    v = []
    f, p = gpu_batch(P, off, a, variant=v)
    assert_same(f, p, f_ref, p_ref, off, f"{what}, {W} waves, table {tab}: {v[0]}")
    assert v[0].startswith(f"chain_dp_coop<W={W},") and f"FAR={int(P.max_iter > 960)}," in v[0] and f"TAB={tab}>" in v[0] and "loop=asm" in v[0], (what, v)


# ---- 1. the rank test
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("max_skip", cd.RANK_SKIPS)
def test_rank_test_at_max_skip_plus_one_and_plus_two(max_skip, form, knobs):
    """targets whose best candidate B has max_skip .. max_skip + 3 candidates nearer than itself (a decoy chain; B in the target's tile, in the tile before, deeper): up to
    max_skip the short cut takes B, at max_skip + 1 the exact scan still reaches it, from max_skip + 2 on the reference's `break` fires first and p is NOT the window's
    best.  One such target among 63 anchors that pass sends a whole tile from the straight-line pushes to the walk; the last one sits in a partial tile."""
    run_form(knobs, case("rank_case", max_skip), *form, f"rank test, max_skip {max_skip}")


# ---- 2. the window edge
EDGE_FORMS = [(bw, form) for bw in cd.EDGE_BW for form in FORMS if not (form[1] and bw > 511)]      # (the table holds |dr - dq| up to 511: beyond, the plain form only)


@pytest.mark.parametrize("bw,form", EDGE_FORMS, ids=[f"{bw}-{FORM_IDS[FORMS.index(form)]}" for bw, form in EDGE_FORMS])
def test_window_edge_one_anchor_outside_and_the_last_one_inside(bw, form, knobs):
    """windows bounded by max_iter = 1 .. 129 (every lane its own start; the tile before holds 1 .. 64 rows of them: whole groups of four and tails of one, two, three): a
    beacon of f = 255 that passes every pair filter lies exactly one anchor before the window of some anchors and is the last one inside for their neighbours.  bw = 500
    and 2^20 - 1: the hand-written rows carry the window test in the filter's third operand; bw = 2^20: the C++ rows."""
    for max_iter in cd.EDGE_ITERS:
        run_form(knobs, case("edge_case", max_iter, bw), *form, f"window edge, max_iter {max_iter}, bw {bw}")


# ---- 3. the dealing of rows
@pytest.mark.parametrize("wn", cd.DEAL_SMALL + cd.DEAL_LARGE + cd.DEAL_EXTRA)
def test_rows_dealt_to_the_helper_waves_and_split_at_the_rings_wrap(wn, knobs):
    """uniform windows of wn anchors over 4 369 anchors: wn - 64 rows per tile for the helpers -- none, fewer than a static block needs (38 rows with seven helpers, 80 with
    fifteen: everything from the counter), just enough -- up to the x / q ring (960), the tiles phase A deals (1 216) and the bound of the short cut (1 280: lanes of
    one tile on both sides of it); ranges of every kind cross anchor 2 048 and 4 096, where the candidate rings wrap.  The best candidate of an anchor lies anywhere in
    its window, for runs of anchors at its last row, and one row behind it."""
    for form in FORMS:
        run_form(knobs, case("deal_case", wn), *form, f"dealing, windows of {wn}")


# ---- 4. ties, 5. equal x
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_equal_scores_take_the_nearer_candidate_and_never_replace_the_span(form, knobs):
    """two candidates of exactly one score in the own tile, own tile / tile before, tile before / deeper, two static blocks, one block, a block and a counter group: p is the
    nearer one; a candidate whose score EQUALS the span: p stays -1; a candidate with f + span == best + 1: the last row the score bound may not skip"""
    run_form(knobs, case("tie_case"), *form, "ties")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_runs_of_equal_x_across_a_tile_edge(form, knobs):
    """runs of 2 .. 70 anchors with one x that start in one tile and end in the next: the equal-x anchor before each has the highest f and passes dq, and is nobody's candidate"""
    run_form(knobs, case("eqx_case"), *form, "equal x")


# ---- (a) cut on the device
def _plan_run(P, off, a):
    import mm2chain
    d_a = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 2)).cuda()
    d_f = torch.full((a.shape[0],), -77, dtype=torch.int32, device="cuda"); d_p = torch.full_like(d_f, -77)
    plan = mm2chain.ChainPlan(P, off)
    plan.run(d_a, d_f, d_p)
    torch.cuda.synchronize()
    route, variant = plan.last_route(), plan.last_variant()
    plan.close()
    return d_f.cpu().numpy(), d_p.cpu().numpy(), route, variant


def _cut_and_compare(knobs, c, pieces, what):
    P, tasks, a, off, f_ref, p_ref = c
    knobs("plan_cut", 1); knobs("plan_cut_min", 1000); knobs("seg_min", 1)
    for w8 in (256, 0):
        knobs("coop_w8_above", w8)
        f, p, route, variant = _plan_run(P, off, a)                  # (the default route: decided on the device, after the cut)
        assert_same(f, p, f_ref, p_ref, off, f"{what}, cut on the device, coop_w8_above {w8}: {variant}, route {route}")
        assert route == (pieces, 0, pieces), (what, route, variant)  # a piece per part, every piece with several waves


@pytest.mark.parametrize("max_skip", cd.RANK_SKIPS)
def test_rank_test_in_pieces_cut_on_the_device(max_skip, knobs):
    """the rank units as ONE task, each behind an x jump beyond max_dist_x at an offset that is no multiple of 64: a piece each, tiles counted from the piece, window
    starts from the task"""
    c = case("cut_rank_case", max_skip)
    _cut_and_compare(knobs, c, 1 + 3 * 4 * cd.RANK_REPS, f"rank test, max_skip {max_skip}")


@pytest.mark.parametrize("bw", cd.EDGE_BW)
def test_window_edge_in_pieces_cut_on_the_device(bw, knobs):
    """five edge tasks of one (max_iter, bw) as ONE task, each part behind an x jump beyond max_dist_x = 2^20 + 2"""
    for max_iter in cd.EDGE_ITERS:
        _cut_and_compare(knobs, case("cut_edge_case", max_iter, bw), cd.CUT_PARTS, f"window edge, max_iter {max_iter}, bw {bw}")


# ---- (b) the per-read entry
def _per_read(P, t, f_ref, p_ref, what):
    import mm2chain
    from mm2chain import params
    assert t.shape[0] <= 7168
    Pr = params.make_params(P.max_dist_x, P.max_dist_y, P.bw, P.max_skip, P.max_iter, P.gap_scale, P.is_cdna, P.n_segs, P.q_span_override, P.flags | mm2chain.MM2C_F_IGNORE_SEG)
    avg = ob.avg_qspan(t)
    for single in (1, 0, 1):
        with mm2chain.tuned(single_launch=single):
            f, p = mm2chain.chain_task(Pr, t, avg)
            v = mm2chain.last_host_variant()
        assert_same(f, p, f_ref, p_ref, None, f"{what}, per-read entry, single_launch {single}: {v}")
        assert v.startswith("chain_dp_coop<W=16,") and f"FAR={int(P.max_iter > 960)},TAB=0>" in v and "loop=asm" in v, (what, v)


@pytest.mark.parametrize("max_skip", cd.RANK_SKIPS)
def test_rank_test_through_the_per_read_entry(max_skip, knobs):
    """one call per task, as run_chaining_on_hw's caller makes them: the kernel makes the window starts itself, as one launch and behind stage_in"""
    P, tasks, a, off, f_ref, p_ref = case("rank_case", max_skip)
    knobs("single_launch", 1)
    for k, t in enumerate(tasks):
        _per_read(P, t, f_ref[off[k]:off[k + 1]], p_ref[off[k]:off[k + 1]], f"rank test, max_skip {max_skip}, task {k}")


@pytest.mark.parametrize("bw", cd.EDGE_BW)
def test_window_edge_through_the_per_read_entry(bw, knobs):
    knobs("single_launch", 1)
    for max_iter in cd.EDGE_ITERS:
        P, (t,), a, off, f_ref, p_ref = case("edge_case", max_iter, bw)
        _per_read(P, t, f_ref, p_ref, f"window edge, max_iter {max_iter}, bw {bw}")
