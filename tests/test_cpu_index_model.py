"""The NumPy key table (tests/index_model.py) against the reference's own index (tests/golden/ref_sketch.npz, map_ont_* and ava_ont_*): the fixture's reference
set is rebuilt as make_ref_sketch_fixtures.py assembles it -- the two test-data FASTAs, the seeded synthetic genome, and the two repeat units drawn by
replaying its generator -- and every key, every key's hit list in order, and mid_occ must equal what mm_idx_build and mm_idx_cal_max_occ gave."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import index_model as im

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "ref_sketch.npz")
DATA = os.path.join(HERE, "golden", "ref_testdata")


def _generator():
    spec = importlib.util.spec_from_file_location("make_ref_sketch_fixtures", os.path.join(HERE, "golden", "make_ref_sketch_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """the reference sequences of the fixture's index, in its order: MT-human, t-inv, the synthetic chromosomes, repeats, repeats2"""
    g = _generator()
    tmp = tmp_path_factory.mktemp("syn")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), str(tmp / "syn"), "--genome-mb", "0.05",
                           "--reads", "6", "--read-len", "4000", "--seed", "5"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(2026)
    g.adversarial(rng)                                         # the draws before the repeat units
    unit = rng.choice(np.frombuffer(b"ACGT", np.uint8), 150).tobytes()
    unit2 = rng.choice(np.frombuffer(b"ACGT", np.uint8), 24).tobytes()
    seqs = []
    for p in (os.path.join(DATA, "MT-human.fa"), os.path.join(DATA, "t-inv.fa"), str(tmp / "syn.ref.fa")):
        seqs += g.read_fasta(p)
    return seqs + [unit * 80, unit2 * 300]


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["map_ont", "ava_ont"])
def test_key_table_equals_the_reference_index(refs, fx, name):
    k, w, hpc = (int(v) for v in fx[name + "_kwh"])
    keys, cr_off, n, pool = im.build_index(refs, k, w, hpc)
    assert np.array_equal(keys, fx[name + "_keys"]), f"{name}: {keys.size} keys, the reference {fx[name + '_keys'].size}"
    assert np.array_equal(n, fx[name + "_n"])
    assert pool.size == int(n.sum())
    ref_pool, ref_cr = fx[name + "_pool"], fx[name + "_cr_off"]
    for i in range(keys.size):                                 # the offsets differ (singletons live in the reference's hash table); the hits do not
        a, b, c = int(cr_off[i]), int(ref_cr[i]), int(n[i])
        assert np.array_equal(pool[a:a + c], ref_pool[b:b + c]), f"{name}: key {int(keys[i]):#x} ({c} hits) differs"
    assert (n > 1).sum() > 500 and n.max() >= fx[name + "_mid_occ"][0], "the fixture's index has multi-hit keys and keys at or above mid_occ"
    assert im.cal_max_occ(n) == int(fx[name + "_mid_occ"][0])


def test_hits_within_a_key_are_in_ascending_y(refs, fx):
    """the order the reference's radix_sort_64 leaves: a key whose hits span several sequences and both strands is what makes this more than by-position"""
    keys, cr_off, n, pool = im.build_index(refs, 15, 10)
    multi = np.nonzero(n > 1)[0]
    mixed = 0
    for i in multi:
        h = pool[cr_off[i]:cr_off[i] + n[i]]
        assert np.all(h[1:] > h[:-1])
        mixed += len(set((h >> np.uint64(32)).tolist())) > 1
    assert mixed > 10


def test_cal_max_occ_rule():
    """hand-made counts: 10 000 keys, the count at index int(0.9998 * 10 000) = 9 998 of the sorted counts (50) plus 1"""
    n = np.ones(10000, np.uint32)
    n[-3:] = [50, 7, 9000]
    assert im.cal_max_occ(n) == 51
    assert im.cal_max_occ(n, 0.0) == 2**31 - 1
    assert im.cal_max_occ(np.array([5], np.uint32)) == 6
