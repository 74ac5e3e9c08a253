"""The score-bound exit of the tile kernel's hand-written loop (csrc/chain_dp_tile.h, MM2C_EXIT_TEST) on the GPU: the inputs of tests/test_cpu_score_exit.py
(tests/score_exit_data.py) through ChainPlan.run and chain_task, f / p compared element for element with the CPU oracle, over the ring forms (compact_ring,
packed_fp, far_ring), the computed and the tabulated gap cost (gap_scale 1.0 / 0.8) and the knob score_bound_exit on and off; and the exits the REAL instruction
sequence takes, counted by the label-counting build (bit 31 of its label counters; tests/tile_loop_harness.py runs it), against the model's for the same inputs."""
import pytest

from tile_loop_harness import RING_FORMS, VARIANT, _init, both_knob_values, knobs, label_bit, label_hits, label_tasks  # noqa: F401 (the fixtures)

pytestmark = pytest.mark.gpu
_REFS = {}


@pytest.mark.parametrize("gap_scale", [1.0, 0.8])
@pytest.mark.parametrize("compact,packed,far_ring", RING_FORMS)
def test_standard_inputs_over_the_ring_forms(compact, packed, far_ring, gap_scale, knobs):
    import score_exit_data as sx
    from mm2chain import params
    knobs("compact_ring", compact); knobs("packed_fp", packed); knobs("far_ring", far_ring)
    tasks = sx.standard_tasks()
    for max_skip in sx.SKIPS:
        P = params.make_params(max_skip=max_skip, gap_scale=gap_scale)
        both_knob_values(_REFS, ("std", max_skip, gap_scale), P, tasks, knobs, f"standard inputs, max_skip={max_skip} gap_scale={gap_scale} compact={compact} packed={packed} far_ring={far_ring}",
                         extra=(f"compact={compact}", f"packed_fp={packed}", f"TAB={int(gap_scale != 1.0)}"))


@pytest.mark.parametrize("compact", [1, 0])
def test_equality_edge(compact, knobs):
    import score_exit_data as sx
    knobs("compact_ring", compact)
    cases = [sx.edge_case(kind, far) for kind, far in sx.EDGE_CASES]
    P = cases[0][0]
    f_ref, p_ref = both_knob_values(_REFS, "edge", P, [c[1] for c in cases], knobs, f"equality edge, compact={compact}")
    base = 0
    for (kind, far), (_, t, info) in zip(sx.EDGE_CASES, cases):
        T = base + info["T"]
        assert f_ref[T] == info["best"] and p_ref[T] == (info["c"] if kind == "fires" else info["j"]), (kind, far)   # (p is relative to the task)
        base += t.shape[0]


def test_first_tile_and_short_last_tile(knobs):
    import score_exit_data as sx
    from mm2chain import params
    both_knob_values(_REFS, "short", params.map_ont(), sx.short_tasks(), knobs, "short tasks")


def test_negative_gap_scale_runs_without_the_exit(knobs):
    import score_exit_data as sx
    P, tasks, info = sx.negative_gap_case()
    f_ref, p_ref = both_knob_values(_REFS, "neg", P, tasks, knobs, "gap_scale = -2", want_exit=0, extra=("TAB=1",))
    assert p_ref[info["T"]] == info["j"]                          # the link the forced exit loses (tests/test_cpu_score_exit.py, D)


def test_pieces_cut_on_the_device(knobs):
    import score_exit_data as sx
    P, t = sx.cut_task()
    tasks = [t] + sx.fold_and_stream_tasks()[:2]
    assert len(sx.cut_pieces(P, t)) > 1
    both_knob_values(_REFS, "cut", P, tasks, knobs, "device-cut task", extra=("cut=1",))


def test_chain_task(knobs):
    import mm2chain
    import oracle_binding as ob
    import score_exit_data as sx
    from helpers import assert_same
    from mm2chain import params
    P = params.make_params(max_skip=3)
    tasks = sx.fold_and_stream_tasks()[:3] + [sx.edge_case(kind, far)[1] for kind, far in sx.EDGE_CASES] + sx.short_tasks()[3:7]
    for ex in (1, 0):
        knobs("score_bound_exit", ex)
        for k, t in enumerate(tasks):
            avg = ob.avg_qspan(t)
            f_ref, p_ref, _ = ob.chain_fpv(P, t, avg)
            f, p = mm2chain.chain_task(P, t, avg)
            assert_same(f, p, f_ref, p_ref, None, f"chain_task, task {k} of {t.shape[0]} anchors, score_bound_exit={ex}: {mm2chain.last_host_variant()}")


def test_exits_counted_on_the_real_loop_equal_the_models(tmp_path):
    import oracle_binding as ob
    from tile_model import chain_tile_model
    hits = label_hits(tmp_path)
    P, tasks = label_tasks()
    model = 0
    for t in tasks:
        st = {}
        chain_tile_model(P, t, ob.avg_qspan(t), NX=16, NF=4, compact=True, stats=st, late_stamps=False)
        model += st["exits"]
    rec = dict(lib=hits["lib"], model=model, on=label_bit(hits["on"], 31), off=label_bit(hits["off"], 31))
    print(rec)
    assert rec["lib"] == VARIANT and rec["model"] > 0
    assert rec["on"] == rec["model"], rec
    assert rec["off"] == 0, rec
