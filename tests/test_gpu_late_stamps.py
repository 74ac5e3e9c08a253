"""The fold order of the tile kernel's hand-written loop (csrc/chain_dp_tile.h: stamps and marks of a scored chunk behind the fold's decision) on the GPU: the
inputs of tests/test_cpu_late_stamps.py (tests/late_stamp_data.py, tests/score_exit_data.py) through ChainPlan.run and chain_task, f / p compared element for
element with the CPU oracle, over the ring forms (compact_ring, packed_fp, far_ring), the computed and the tabulated gap cost (gap_scale 1.0 / 0.8) and the knob
score_bound_exit on and off; and the chunks that the REAL instruction sequence leaves before stamping, counted by the label-counting build, against the model's.
In that build bit 4 (Lhf) counts the chunks that write their stamps; bits 1 and 3 count the scored own-tile and ring chunks: the difference is what left before.

Run as a program (the label-counter case starts it in a fresh child process under MM2C_LIB_PATH = variants/labelcount.so): writes the counts with the knob on and
off, and the model's, to the JSON file named on the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "minimap2-fpga_amd", "variants", "labelcount.so")
LABEL_SKIP = 3            # max_skip of the label-counter case
RING_FORMS = [(1, 1, 0), (1, 1, 2), (1, 0, 0), (1, 0, 2), (0, 0, 0), (0, 0, 2)]   # compact_ring, packed_fp, far_ring

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    import torch
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture
def knobs():
    import helpers
    import mm2chain

    def tune(key, val):
        if key == "coop_plans":
            helpers.PINNED_ROUTE = val
        return mm2chain.tune(key, val)
    yield tune
    helpers.PINNED_ROUTE = None
    for key, val in (("score_bound_exit", 1), ("compact_ring", 1), ("packed_fp", 1), ("far_ring", 1), ("coop_plans", 2)):
        mm2chain.tune(key, val)


_REFS = {}


def _ref(key, P, tasks):
    """oracle f / p of a batch, computed once per module"""
    from helpers import oracle_batch
    from reuse_data import batch
    if key not in _REFS:
        a, off = batch(tasks)
        _REFS[key] = (a, off) + tuple(oracle_batch(P, off, a))
    return _REFS[key]


def _both_knob_values(key, P, tasks, knobs, what, extra=()):
    """GPU == oracle with score_bound_exit 1 and 0; the variant text says which ran.  Returns the oracle's (f, p)."""
    from helpers import assert_same, gpu_batch
    a, off, f_ref, p_ref = _ref(key, P, tasks)
    for ex in (1, 0):
        knobs("score_bound_exit", ex)
        v = []
        f, p = gpu_batch(P, off, a, variant=v)
        assert_same(f, p, f_ref, p_ref, off, f"{what}, score_bound_exit={ex}: {v[0]}")
        assert "loop=asm" in v[0] and f"score_exit={ex}" in v[0] and all(w in v[0] for w in extra), v
    return f_ref, p_ref


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
        _both_knob_values(("std", max_skip, gap_scale), P, tasks, knobs, f"standard inputs, max_skip={max_skip} gap_scale={gap_scale} compact={compact} packed={packed} far_ring={far_ring}",
                          extra=(f"compact={compact}", f"packed_fp={packed}", f"TAB={int(gap_scale != 1.0)}"))


@pytest.mark.parametrize("gap_scale", [1.0, 0.8])
@pytest.mark.parametrize("compact,packed", [(1, 1), (1, 0), (0, 0)])
def test_windows_around_the_end_of_the_fp_ring(compact, packed, gap_scale, knobs):
    """1 .. 6 whole older tiles with and without a partly covered one, the best candidate in the deepest (tests/test_cpu_late_stamps.py, B)"""
    import late_stamp_data as ls
    knobs("compact_ring", compact); knobs("packed_fp", packed)
    for m, part in ls.DEPTH_CASES:
        P, t, info = ls.depth_case(m, part, gap_scale)
        f_ref, p_ref = _both_knob_values(("depth", m, part, gap_scale), P, [t], knobs, f"window of {m} older tiles + {part} anchors, gap_scale={gap_scale} compact={compact} packed={packed}",
                                         extra=(f"compact={compact}", f"packed_fp={packed}"))
        assert p_ref[info["T"]] == info["cands"][-1][1]


def test_first_tile_and_short_last_tile(knobs):
    import score_exit_data as sx
    from mm2chain import params
    _both_knob_values("short", params.map_ont(), sx.short_tasks(), knobs, "short tasks")


def test_pieces_cut_on_the_device(knobs):
    import score_exit_data as sx
    P, t = sx.cut_task()
    tasks = [t] + sx.fold_and_stream_tasks()[:2]
    assert len(sx.cut_pieces(P, t)) > 1
    _both_knob_values("cut", P, tasks, knobs, "device-cut task", extra=("cut=1",))


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
    assert os.path.exists(VARIANT), "minimap2-fpga_amd/variants/labelcount.so is built by `make -C minimap2-fpga_amd` (__graft_entry__.build())"
    out = str(tmp_path / "unstamped.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, MM2C_LIB_PATH=VARIANT), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, "the label-counting run failed:\n" + r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.load(open(out))
    print(rec)
    assert rec["lib"] == VARIANT and rec["model"]["on"]["unstamped"] > 0
    for knob in ("on", "off"):
        assert rec[knob] == rec["model"][knob], rec
    assert rec["off"]["unstamped"] == 0, rec


def _child(out_path):
    """fold-driver tasks once with the knob on, once off, one wave per piece: scored chunks (bits 1 and 3) less stamped chunks (bit 4), summed over the rows that ran,
    and the model's"""
    for p in (os.path.join(ROOT, "minimap2-fpga_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import ctypes as C
    import torch
    import mm2chain
    import oracle_binding as ob
    from helpers import fold_driver_tasks
    from mm2chain import _native as N, params
    from reuse_data import batch
    from tile_model_late_stamps import chain_tile_model_late_stamps
    tasks = fold_driver_tasks(np.random.default_rng(4242), shapes=((1100, 4, 0.05, 0.15), (2000, 3, 0.0, 0.3), (700, 12, 0.2, 0.15), (500, 40, 0.0, 0.2)))
    P = params.make_params(max_skip=LABEL_SKIP)
    a, off = batch(tasks)
    f_ref, p_ref, _ = ob.chain_batch(P, off, a, n_threads=4)
    model = {}
    for name, mode in (("on", "auto"), ("off", "off")):
        model[name] = dict(unstamped=0, stamped=0)
        for t in tasks:
            st = {}
            chain_tile_model_late_stamps(P, t, ob.avg_qspan(t), NX=16, NF=4, compact=True, stats=st, score_exit=mode)
            model[name]["unstamped"] += st["exits_unstamped"]
            model[name]["stamped"] += st["stamped_chunks"]
    mm2chain.init()
    mm2chain.tune("coop_plans", 0)
    lib = N.load()
    d_a = torch.from_numpy(a.view(np.int64).reshape(-1, 2)).cuda()
    counted = {}
    for name, ex in (("on", 1), ("off", 0)):
        mm2chain.tune("score_bound_exit", ex)
        hits = (C.c_ulonglong * 256)()
        N.check(lib.mm2c_debug_label_hits(hits, 1), "mm2c_debug_label_hits")          # (reset)
        d_f = torch.empty(a.shape[0], dtype=torch.int32, device="cuda"); d_p = torch.empty_like(d_f)
        plan = mm2chain.ChainPlan(P, off)
        plan.run(d_a, d_f, d_p)
        torch.cuda.synchronize()
        variant = plan.last_variant()
        plan.close()
        assert np.array_equal(d_f.cpu().numpy(), f_ref) and np.array_equal(d_p.cpu().numpy(), p_ref), variant
        assert "loop=asm" in variant and f"score_exit={ex}" in variant, variant
        N.check(lib.mm2c_debug_label_hits(hits, 0), "mm2c_debug_label_hits")
        scored = int(sum(hits[row * 32 + 1] + hits[row * 32 + 3] for row in range(8)))
        stamped = int(sum(hits[row * 32 + 4] for row in range(8)))
        counted[name] = dict(unstamped=scored - stamped, stamped=stamped)
    mm2chain.shutdown()
    json.dump(dict(lib=N.LIB_PATH, model=model, **counted), open(out_path, "w"))


if __name__ == "__main__":
    _child(sys.argv[1])
