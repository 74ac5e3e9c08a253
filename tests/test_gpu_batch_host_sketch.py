"""The batched host (examples/batch_host/batch_driver.c) with MM2_BATCH_GPU_SKETCH=1: the mini-batch's sequences go to the library and mm_sketch, the lookups,
seed hits, DP and epilogue all run on the GPU (mm2c_read_chain_batch).  Its PAF must be the reference's (the MT pair's md5 of SURVEY.md section 4, the t-inv
lines of ref_host_paf_observed.txt) and byte-identical to the default batched host on a synthetic genome with repeats."""
import hashlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_EXE = os.path.join(ROOT, "oracle", "_ref", "mm2_batchhost")
DATA = os.path.join(ROOT, "tests", "golden", "ref_testdata")
MT_MD5 = "f49a6331f92e6f24acc73485827a2eba"


def _run(ref, qry, gpu_sketch, threads=2, extra=None):
    if not os.path.exists(BATCH_EXE):
        pytest.skip("oracle/_ref/mm2_batchhost not built (needs /root/reference at build time: __graft_entry__.build())")
    env = dict(os.environ)
    env.pop("MM2_BATCH_GPU_SKETCH", None)
    if gpu_sketch:
        env["MM2_BATCH_GPU_SKETCH"] = "1"
    env.update(extra or {})
    r = subprocess.run([BATCH_EXE, "-t", str(threads), ref, qry], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_gpu_sketch_prints_the_reference_paf():
    out = _run(os.path.join(DATA, "MT-human.fa"), os.path.join(DATA, "MT-orang.fa"), True)
    assert hashlib.md5(out.encode()).hexdigest() == MT_MD5, out
    lines = _run(os.path.join(DATA, "t-inv.fa"), os.path.join(DATA, "q-inv.fa"), True)
    want = open(os.path.join(ROOT, "tests", "golden", "ref_host_paf_observed.txt")).read().split("# t-inv.fa q-inv.fa\n")[1].split("#")[0]
    assert lines == want
    assert _run(os.path.join(DATA, "t2.fa"), os.path.join(DATA, "q2.fa"), True) == ""


def test_gpu_sketch_equals_default_on_a_synthetic_genome(tmp_path):
    prefix = str(tmp_path / "syn")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), prefix, "--genome-mb", "4", "--reads", "300", "--seed", "21"],
                          stdout=subprocess.DEVNULL)
    ref, qry = prefix + ".ref.fa", prefix + ".reads.fa"
    small = {"MM2_MINI_BATCH": "400000"}                              # several mini-batches in flight
    base = _run(ref, qry, False, threads=4, extra=small)
    assert base.count("\n") > 200
    assert _run(ref, qry, True, threads=4, extra=small) == base
    assert _run(ref, qry, True, threads=4) == base
