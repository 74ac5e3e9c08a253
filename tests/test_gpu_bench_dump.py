"""`bench.py --dump-outputs DIR`: f[] and p[] of the last timed step as float64 .npy files, the same rows from run to run (a plain run and a --full
run alike), equal to the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 1 024 reads of 2 500 anchors: 2.56e6 rows, more than bench.DUMP_ROWS, so the seeded sample is what is written
ARGS = ["--steps", "3", "--warmup", "1", "--reads", "1024", "--distinct", "128", "--anchors-per-read", "2500", "--cpu-seconds", "0", "--no-secondary"]


def _bench(out_dir, full):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir)] + ARGS + (["--full"] if full else []),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3
    if full:
        assert line["verified_vs_oracle"] is True
    else:                                       # a plain run does not check against the oracle: that is --full's
        assert "verified_vs_oracle" not in line
    return {k: np.load(os.path.join(out_dir, k + ".npy")) for k in ("index", "f", "p")}


def test_dumped_outputs_are_a_fixed_sample_equal_to_the_oracle(tmp_path):
    from mm2chain import params, synth
    a, b = _bench(tmp_path / "a", full=False), _bench(tmp_path / "b", full=True)
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float64 and a[k].shape == (1 << 21,)
        assert np.array_equal(a[k], b[k]), k
    idx = a["index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < 1024 * 2500
    # the batch is the 128 distinct reads tiled 8 times: row r holds the anchors of row r mod (128 x 2500) of the distinct reads
    off1, a1 = synth.make_stream("mixed", 128, 2500, seed=20240)
    f_ref, p_ref, _ = ob.chain_batch(params.map_ont(), off1.numpy(), a1.numpy().view(np.uint64), 4)
    rows = idx % int(off1[-1])
    assert np.array_equal(a["f"], f_ref[rows].astype(np.float64)) and np.array_equal(a["p"], p_ref[rows].astype(np.float64))
