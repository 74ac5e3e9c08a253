"""The tile kernel's hand-written loop (csrc/chain_dp_tile.h) with its older tiles counted in anchors, the per-anchor word in the loop's layout, the two-instruction
log term and the packed f / p word left packed on the lean form's way to the stamps: the inputs of tests/loop_trim_data.py through ChainPlan.run and chain_task, f / p
compared element for element with the CPU oracle -- over ring_class 0 .. 4, the ring forms of the tile kernel (compact_ring, packed_fp, far_ring), the computed and
the tabulated gap cost (gap_scale 1.0 / 0.8) and the knob score_bound_exit on and off.

What each input holds is asserted here from the oracle (and, for the order of an exit and a stamp, from the model's events).  Which fold a chunk takes is not visible
in f / p; for the record, a copy of tests/tile_model.py with a counter per fold and depth gave, for NX 16 / NF 4 at max_skip 3:
  fold drivers (label_tasks)     B0 at depth 0 / 1 / beyond NF: 2 419 / 153 / 16;   general folds with marks or skips (Lb2): 1 528 / 249 / 37;   no B1
  pair_task(m, "b1")             exactly one fold B1, at depth m (0, 1, NF + 1);     pair_task(m, "b1m"): one Lslow2 -> Lb1m at depth m
  depth_task(m, part)            one fold B0 per scored chunk, the last at the depth of the deepest candidate"""
import numpy as np
import pytest

from tile_loop_harness import RING_FORMS, _init, knobs, ref  # noqa: F401 (the fixtures)

pytestmark = pytest.mark.gpu
_REFS = {}
GAP_SCALES = [1.0, 0.8]


def _params(gap_scale):
    import loop_trim_data as lt
    from mm2chain import params
    return params.make_params(max_skip=lt.MAX_SKIP, gap_scale=gap_scale)


def _batch(gap_scale):
    """(tasks, index, anchors, offsets, oracle f, oracle p) of the whole batch at one gap_scale, made once"""
    import loop_trim_data as lt
    if ("tasks",) not in _REFS:
        _REFS[("tasks",)] = lt.all_tasks()
    tasks, index = _REFS[("tasks",)]
    return (tasks, index) + tuple(ref(_REFS, ("all", gap_scale), _params(gap_scale), tasks))


@pytest.mark.parametrize("gap_scale", GAP_SCALES)
def test_inputs_hold_what_they_are_named_for(gap_scale):
    """from the oracle alone: the deepest candidate is the best at every depth, every dd scores its own gap cost, the short tasks have their sizes"""
    import loop_trim_data as lt
    import oracle_binding as ob
    tasks, index, a, off, f_ref, p_ref = _batch(gap_scale)
    for k, (m, part) in enumerate(lt.DEPTH_CASES):
        t, info = lt.depth_task(m, part)
        o = off[index["depth"] + k]
        assert np.array_equal(t, tasks[index["depth"] + k])
        assert info["T"] - info["lo"] == lt.T_POS + 64 * m + part and info["depth"] == m + (part > 0)
        assert p_ref[o + info["T"]] == info["deepest"], (m, part)
        assert all(p_ref[o + j] == -1 for _, j in info["cands"])
    for k, (m, kind) in enumerate(lt.PAIR_CASES):
        _, info = lt.pair_task(m, kind)
        o = off[index["pair"] + k]
        assert p_ref[o + info["T"]] == info["j2"] and p_ref[o + info["j1"]] == -1 and p_ref[o + info["j2"]] == -1, (m, kind)
    t, pairs = lt.dd_task()
    o, avg = off[index["dd"]], ob.avg_qspan(t)
    assert {dd for _, _, dd, _ in pairs} >= {0, 1, 2, 3, 4, lt.BW} | {1 << b for b in range(9)}
    for T, j, dd, sign in pairs:
        if dd <= lt.BW:
            assert p_ref[o + T] == j and f_ref[o + T] == lt.DD_SPAN_J + lt.FILL_SPAN - lt.gap_cost(dd, avg, gap_scale), (T, j, dd, sign)
        else:
            assert p_ref[o + T] == -1 and f_ref[o + T] == lt.FILL_SPAN
    assert tuple(tasks[index["short"] + k].shape[0] for k in range(len(lt.SHORT_SIZES))) == lt.SHORT_SIZES == (1, 63, 64, 65, 128, 129)
    x = tasks[index["eq"]][:, 0]
    assert len(set(x[lt.EQ_RUN[0]:lt.EQ_RUN[1] + 1].tolist())) == 1 and x[lt.EQ_RUN[0] - 1] < x[lt.EQ_RUN[0]] and x[lt.EQ_RUN[1] + 1] > x[lt.EQ_RUN[1]]
    assert lt.EQ_RUN[0] // 64 < lt.EQ_RUN[1] // 64 and lt.EQ_RUN[1] % 64 < 62


def test_an_exit_before_the_stamps_is_followed_by_a_stamping_chunk_in_the_same_tile():
    """from the model (== oracle on this task): an anchor whose fold B0 leaves before any stamp of its chunk, and the next anchor, in the same tile, reads a mark in its own
    tile -- so it stamped there"""
    import loop_trim_data as lt
    from tile_loop_harness import run_model, same
    o, mdl, st, ex, ev = run_model(_params(1.0), lt.exit_then_stamp_task(), NX=lt.NX, NF=lt.NF, compact=True)
    assert same(o, mdl)
    left, stamped = {i for i, _ in ev["unstamped"]}, set(ev["own_marks"])
    assert [i for i in left if (i + 1) // 64 == i // 64 and i + 1 in stamped], (len(left), len(stamped))


def _run_both_knob_values(knobs, gap_scale, what, want_asm):
    from helpers import assert_same, gpu_batch
    tasks, index, a, off, f_ref, p_ref = _batch(gap_scale)
    for ex in (1, 0):
        knobs("score_bound_exit", ex)
        v = []
        f, p = gpu_batch(_params(gap_scale), off, a, variant=v)
        assert_same(f, p, f_ref, p_ref, off, f"{what}, gap_scale={gap_scale}, score_bound_exit={ex}: {v[0]}")
        if want_asm:
            assert "loop=asm" in v[0] and f"score_exit={ex}" in v[0], v


@pytest.mark.parametrize("gap_scale", GAP_SCALES)
@pytest.mark.parametrize("ring_class", [0, 1, 2, 3, 4])
def test_ring_classes(ring_class, gap_scale, knobs):
    import mm2chain
    with mm2chain.tuned(ring_class=ring_class):
        _run_both_knob_values(knobs, gap_scale, f"ring_class={ring_class}", want_asm=ring_class >= 3)


@pytest.mark.parametrize("gap_scale", GAP_SCALES)
@pytest.mark.parametrize("compact,packed,far_ring", RING_FORMS)
def test_ring_forms(compact, packed, far_ring, gap_scale, knobs):
    knobs("compact_ring", compact); knobs("packed_fp", packed); knobs("far_ring", far_ring)
    _run_both_knob_values(knobs, gap_scale, f"compact={compact} packed={packed} far_ring={far_ring}", want_asm=True)


@pytest.mark.parametrize("gap_scale", GAP_SCALES)
def test_pieces_cut_on_the_device(gap_scale, knobs):
    import score_exit_data as sx
    from tile_loop_harness import both_knob_values
    from mm2chain import params
    _, t = sx.cut_task()
    P = params.make_params(gap_scale=gap_scale)
    assert len(sx.cut_pieces(P, t)) > 1
    import loop_trim_data as lt
    tasks = [t, lt.depth_task(lt.NF + 1, 63)[0], lt.dd_task()[0]]
    both_knob_values(_REFS, ("cut", gap_scale), P, tasks, knobs, f"device-cut task, gap_scale={gap_scale}", extra=("cut=1",))


@pytest.mark.parametrize("gap_scale", GAP_SCALES)
def test_chain_task(gap_scale, knobs):
    import mm2chain
    import oracle_binding as ob
    from helpers import assert_same
    tasks, index, a, off, f_ref, p_ref = _batch(gap_scale)
    P = _params(gap_scale)
    for ex in (1, 0):
        knobs("score_bound_exit", ex)
        for k, t in enumerate(tasks):
            f, p = mm2chain.chain_task(P, t, ob.avg_qspan(t))
            assert_same(f, p, f_ref[off[k]:off[k + 1]], p_ref[off[k]:off[k + 1]], None,
                        f"chain_task, task {k} of {t.shape[0]} anchors, gap_scale={gap_scale}, score_bound_exit={ex}: {mm2chain.last_host_variant()}")
