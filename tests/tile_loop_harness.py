"""What the tests of the tile kernel's hand-written loop (csrc/chain_dp_tile.h, MM2C_SCAN_TILE_ASM) share: the model held against the oracle (run_model, same) for
tests/test_cpu_score_exit.py and tests/test_cpu_late_stamps.py; the fixtures, the oracle cache and the run over both values of the knob score_bound_exit for
tests/test_gpu_score_exit.py and tests/test_gpu_late_stamps.py; and the label-counter run.

Run as a program (label_hits starts it in a fresh child process under MM2C_LIB_PATH = variants/labelcount.so): the fold-driver tasks once with the knob on, once
off, one wave per piece; writes the library's path and the whole table of 256 label counters of either run to the JSON file named on the command
line.  Which bits mean what is the business of the test that reads them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import knobs  # noqa: F401 (a fixture, handed on to the modules that import this one's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "minimap2-fpga_amd", "variants", "labelcount.so")
LABEL_SKIP = 3            # max_skip of the label-counter case
RING_FORMS = [(1, 1, 0), (1, 1, 2), (1, 0, 0), (1, 0, 2), (0, 0, 0), (0, 0, 2)]   # compact_ring, packed_fp, far_ring


def run_model(P, t, **kw):
    """(oracle f, p), (model f, p), stats, anchors that left early, events"""
    import oracle_binding as ob
    from tile_model import chain_tile_model
    avg = ob.avg_qspan(t)
    f, p, _ = ob.chain_fpv(P, t, avg)
    st, ex, ev = {}, [], dict(unstamped=[], own_marks=[])
    fm, pm = chain_tile_model(P, t, avg, stats=st, exit_anchors=ex, events=ev, **kw)
    return (f, p), (fm, pm), st, ex, ev


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module", autouse=True)
def _init():
    import torch
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def ref(refs, key, P, tasks):
    """oracle f / p of a batch, computed once per module (refs: the module's cache)"""
    from helpers import oracle_batch
    from reuse_data import batch
    if key not in refs:
        a, off = batch(tasks)
        refs[key] = (a, off) + tuple(oracle_batch(P, off, a))
    return refs[key]


def both_knob_values(refs, key, P, tasks, knobs, what, want_exit=1, extra=()):
    """GPU == oracle with score_bound_exit 1 and 0; the variant text says which ran.  Returns the oracle's (f, p)."""
    from helpers import assert_same, gpu_batch
    a, off, f_ref, p_ref = ref(refs, key, P, tasks)
    for ex in (1, 0):
        knobs("score_bound_exit", ex)
        v = []
        f, p = gpu_batch(P, off, a, variant=v)
        assert_same(f, p, f_ref, p_ref, off, f"{what}, score_bound_exit={ex}: {v[0]}")
        assert "loop=asm" in v[0] and f"score_exit={ex and want_exit}" in v[0] and all(w in v[0] for w in extra), v
    return f_ref, p_ref


def label_tasks():
    """(P, tasks) of the label-counter case: the fold drivers of test_model_of_the_hand_written_loop_reaches_every_label (tests/test_cpu_oracle.py)"""
    from helpers import fold_driver_tasks
    from mm2chain import params
    tasks = fold_driver_tasks(np.random.default_rng(4242), shapes=((1100, 4, 0.05, 0.15), (2000, 3, 0.0, 0.3), (700, 12, 0.2, 0.15), (500, 40, 0.0, 0.2)))
    return params.make_params(max_skip=LABEL_SKIP), tasks


def label_hits(tmp_path):
    """{"lib", "on", "off"}: the label counters of the real loop over label_tasks() with the knob on and off (256 each: label_bit), counted in a fresh process"""
    assert os.path.exists(VARIANT), "minimap2-fpga_amd/variants/labelcount.so is built by `make -C minimap2-fpga_amd` (__graft_entry__.build())"
    out = str(tmp_path / "label_hits.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, MM2C_LIB_PATH=VARIANT), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, "the label-counting run failed:\n" + r.stdout[-3000:] + r.stderr[-3000:]
    return json.load(open(out))


def label_bit(hits, bit):
    """one bit of the label counters summed over the rows that ran"""
    return int(sum(hits[row * 32 + bit] for row in range(8)))


def _child(out_path):
    sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))
    import ctypes as C
    import torch
    import mm2chain
    import oracle_binding as ob
    from mm2chain import _native as N
    from reuse_data import batch
    P, tasks = label_tasks()
    a, off = batch(tasks)
    f_ref, p_ref, _ = ob.chain_batch(P, off, a, n_threads=4)
    mm2chain.init()
    mm2chain.tune("coop_plans", 0)
    lib = N.load()
    d_a = torch.from_numpy(a.view(np.int64).reshape(-1, 2)).cuda()
    rec = dict(lib=N.LIB_PATH)
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
        rec[name] = [int(h) for h in hits]
    mm2chain.shutdown()
    json.dump(rec, open(out_path, "w"))


if __name__ == "__main__":
    _child(sys.argv[1])
