"""The fold order of the tile kernel's hand-written loop (csrc/chain_dp_tile.h: stamps and marks of a scored chunk behind the fold's decision) on the GPU: the
inputs of tests/test_cpu_late_stamps.py (tests/late_stamp_data.py, tests/score_exit_data.py) through ChainPlan.run and chain_task, f / p compared element for
element with the CPU oracle, over the ring forms (compact_ring, packed_fp, far_ring), the computed and the tabulated gap cost (gap_scale 1.0 / 0.8) and the knob
score_bound_exit on and off; and the chunks that the REAL instruction sequence leaves before stamping, counted by the label-counting build, against the model's.
In that build (tests/tile_loop_harness.py runs it) bit 4 (Lhf) counts the chunks that write their stamps; bits 1 and 3 count the scored own-tile and ring chunks:
the difference is what left before."""
import pytest

from tile_loop_harness import RING_FORMS, VARIANT, _init, both_knob_values, knobs, label_bit, label_hits, label_tasks  # noqa: F401 (the fixtures)

pytestmark = pytest.mark.gpu
_REFS = {}


@pytest.mark.parametrize("gap_scale", [1.0, 0.8])
@pytest.mark.parametrize("compact,packed,far_ring", RING_FORMS)
def test_standard_inputs_over_the_ring_forms(compact, packed, far_ring, gap_scale, knobs):
    """max_skip 0, 1 and 25: a fold B0 that stays stamps late and still reaches the `break` (tests/test_cpu_late_stamps.py, A)"""
    import late_stamp_data as ls
    from mm2chain import params
    knobs("compact_ring", compact); knobs("packed_fp", packed); knobs("far_ring", far_ring)
    tasks = ls.standard_tasks()
    for max_skip in ls.SKIPS:
        P = params.make_params(max_skip=max_skip, gap_scale=gap_scale)
        both_knob_values(_REFS, ("std", max_skip, gap_scale), P, tasks, knobs, f"standard inputs, max_skip={max_skip} gap_scale={gap_scale} compact={compact} packed={packed} far_ring={far_ring}",
                         extra=(f"compact={compact}", f"packed_fp={packed}", f"TAB={int(gap_scale != 1.0)}"))


@pytest.mark.parametrize("gap_scale", [1.0, 0.8])
@pytest.mark.parametrize("compact,packed", [(1, 1), (1, 0), (0, 0)])
def test_windows_around_the_end_of_the_fp_ring(compact, packed, gap_scale, knobs):
    """1 .. 6 whole older tiles with and without a partly covered one, the best candidate in the deepest (tests/test_cpu_late_stamps.py, B)"""
    import late_stamp_data as ls
    knobs("compact_ring", compact); knobs("packed_fp", packed)
    for m, part in ls.DEPTH_CASES:
        P, t, info = ls.depth_case(m, part, gap_scale)
        f_ref, p_ref = both_knob_values(_REFS, ("depth", m, part, gap_scale), P, [t], knobs, f"window of {m} older tiles + {part} anchors, gap_scale={gap_scale} compact={compact} packed={packed}",
                                        extra=(f"compact={compact}", f"packed_fp={packed}"))
        assert p_ref[info["T"]] == info["cands"][-1][1]


def test_first_tile_and_short_last_tile(knobs):
    import score_exit_data as sx
    from mm2chain import params
    both_knob_values(_REFS, "short", params.map_ont(), sx.short_tasks(), knobs, "short tasks")


def test_pieces_cut_on_the_device(knobs):
    import score_exit_data as sx
    P, t = sx.cut_task()
    tasks = [t] + sx.fold_and_stream_tasks()[:2]
    assert len(sx.cut_pieces(P, t)) > 1
    both_knob_values(_REFS, "cut", P, tasks, knobs, "device-cut task", extra=("cut=1",))


def test_chain_task(knobs):
    import late_stamp_data as ls
    import mm2chain
    import oracle_binding as ob
    import score_exit_data as sx
    from helpers import assert_same
    from mm2chain import params
    work = [(params.make_params(max_skip=s), t) for s in ls.SKIPS for t in sx.fold_and_stream_tasks()[:3]]
    work += [ls.depth_case(m, part)[:2] for m, part in ls.DEPTH_CASES]
    for ex in (1, 0):
        knobs("score_bound_exit", ex)
        for k, (P, t) in enumerate(work):
            avg = ob.avg_qspan(t)
            f_ref, p_ref, _ = ob.chain_fpv(P, t, avg)
            f, p = mm2chain.chain_task(P, t, avg)
            assert_same(f, p, f_ref, p_ref, None, f"chain_task, task {k} of {t.shape[0]} anchors, score_bound_exit={ex}: {mm2chain.last_host_variant()}")


def test_chunks_left_before_stamping_on_the_real_loop_equal_the_models(tmp_path):
    import oracle_binding as ob
    from tile_model import chain_tile_model
    hits = label_hits(tmp_path)
    P, tasks = label_tasks()
    rec = dict(lib=hits["lib"], model={})
    for knob, mode in (("on", "auto"), ("off", "off")):
        rec["model"][knob] = dict(unstamped=0, stamped=0)
        for t in tasks:
            st = {}
            chain_tile_model(P, t, ob.avg_qspan(t), NX=16, NF=4, compact=True, stats=st, score_exit=mode)
            rec["model"][knob]["unstamped"] += st["exits_unstamped"]
            rec["model"][knob]["stamped"] += st["stamped_chunks"]
        scored, stamped = label_bit(hits[knob], 1) + label_bit(hits[knob], 3), label_bit(hits[knob], 4)
        rec[knob] = dict(unstamped=scored - stamped, stamped=stamped)
    print(rec)
    assert rec["lib"] == VARIANT and rec["model"]["on"]["unstamped"] > 0
    for knob in ("on", "off"):
        assert rec[knob] == rec["model"][knob], rec
    assert rec["off"]["unstamped"] == 0, rec
