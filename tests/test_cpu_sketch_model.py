"""The Python restatement of mm_sketch / collect_matches (tests/sketch_model.py) against the reference's own output on every fixture read
(tests/golden/ref_sketch.npz, make_ref_sketch_fixtures.py, which pins each read's output by count and SHA-256): the model the GPU tests compare random
batches with is itself pinned to the reference."""
import os

import numpy as np
import pytest

import sketch_model as sm

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sketch.npz")
CONFIGS = ["map_ont", "ava_ont", "asm20", "sr", "map_pb", "ava_pb", "even_k16", "w1", "w255"]


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


def reads(fx):
    off, seq = fx["seq_off"], fx["seq"]
    return [seq[off[r]:off[r + 1]].tobytes() for r in range(off.size - 1)]


@pytest.mark.parametrize("name", CONFIGS)
def test_model_sketch_equals_reference(fx, name):
    k, w, hpc = (int(v) for v in fx[name + "_kwh"])
    off, digest = fx[name + "_off"], fx[name + "_sha"]
    for r, s in enumerate(reads(fx)):
        got = sm.sketch_array(s, w, k, hpc)
        assert got.shape[0] == off[r + 1] - off[r], f"{name}: read {r} ({len(s)} bases): {got.shape[0]} minimizers, the reference {off[r + 1] - off[r]}"
        assert np.array_equal(sm.sha(got), digest[r]), f"{name}: read {r} ({len(s)} bases) differs"


def test_fixture_reaches_the_corners(fx):
    """the adversarial reads do what they are there for: the HPC span cut drops minimizers, even k skips symmetric k-mers, reads shorter than
    w + k - 1 still end in the final push"""
    rs = reads(fx)
    hp = [i for i, s in enumerate(rs) if b"A" * 300 in s][0]
    spans = [int(x) & 0xFF for x, _ in sm.sketch(rs[hp], 10, 19, True)]
    assert max(spans) < 256 and len(spans) > 0
    sym = [i for i, s in enumerate(rs) if s.startswith(b"AT" * 300)][0]
    assert len(sm.sketch(rs[sym], 10, 16)) < len(sm.sketch(rs[sym], 10, 15))
    short = [s for s in rs if 0 < len(s) < 15 + 10 - 1 and len(s) >= 15]
    assert all(len(sm.sketch(s, 10, 15)) == 1 for s in short)
    assert any(len(s) >= 100_000 for s in rs)


@pytest.mark.parametrize("name", ["map_ont", "ava_ont"])
def test_model_matches_equal_reference(fx, name):
    k, w, hpc = (int(v) for v in fx[name + "_kwh"])
    look = sm.table_lookup(fx[name + "_keys"], fx[name + "_cr_off"], fx[name + "_n"])
    mid_occ = int(fx[name + "_mid_occ"][0])
    mo = fx[name + "_match_off"]
    n_rep = n_absent = n_hit = 0
    for r, s in enumerate(reads(fx)):
        m, rep_len, mini_pos = sm.collect_matches(sm.sketch_array(s, w, k, hpc), look, mid_occ)
        ma = sm.match_array(m)
        assert ma.size == mo[r + 1] - mo[r] and np.array_equal(sm.sha(ma), fx[name + "_match_sha"][r]), f"{name}: matches of read {r} differ"
        assert rep_len == int(fx[name + "_rep_len"][r])
        assert np.array_equal(sm.sha(np.array(mini_pos, np.uint64)), fx[name + "_mini_pos_sha"][r])
        n_rep += rep_len > 0
        n_absent += int((ma["n"] == 0).sum())
        n_hit += int((ma["n"] > 0).sum())
    assert n_rep > 0 and n_absent > 0 and n_hit > 0, "the fixture reaches repetitive minimizers, absent keys and hits"
