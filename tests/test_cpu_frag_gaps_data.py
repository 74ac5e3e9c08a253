"""CPU checks of tests/golden/ref_frag_gaps.npz (per-fragment chaining distances as the reference's mm_map_frag applied them): the assertions its maker made
hold for the committed file -- enough distinct pairs, re-chained fragments with different pairs, and fragments whose chains come out differently when the
fixture's most common pair is used in the place of their own, so that a build which ignored the per-fragment values could not pass the GPU tests -- and the
NumPy restatement of map.c:305-314 (tests/frag_gaps_model.py) gives exactly the pairs the reference recorded."""
import importlib.util
import os

import numpy as np
import pytest

import frag_gaps_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "ref_frag_gaps.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


def test_fixture_holds_what_its_maker_asserted(fx, oracle):
    spec = importlib.util.spec_from_file_location("make_ref_frag_gaps_fixtures", os.path.join(HERE, "golden", "make_ref_frag_gaps_fixtures.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    mk.check_fixture(fx)
    assert os.path.getsize(FIX) < (1 << 20)


def test_planted_fragments_need_their_own_pair(fx, oracle):
    """both directions: long mates (own max_dist_x below the common one) and short mates (above it)"""
    import oracle_binding as ob
    from mm2chain import params
    common = tuple(int(v) for v in fx["common"])
    below = above = 0
    for g in fx["planted"]:
        h = [int(v) for v in fx["par"][g]]
        a = fx["heap_a"][fx["heap_a_off"][g]:fx["heap_a_off"][g + 1]]
        mk = lambda x, y: params.make_params(max_dist_x=x, max_dist_y=y, bw=h[2], max_skip=h[3], max_iter=h[4], gap_scale=1.0, is_cdna=h[7], n_segs=h[8])
        own, other = ob.mm_chain_dp(mk(h[0], h[1]), h[5], h[6], a), ob.mm_chain_dp(mk(*common), h[5], h[6], a)
        assert np.array_equal(own[0], fx["heap_u"][fx["heap_u_off"][g]:fx["heap_u_off"][g + 1]])           # the oracle is the reference's mm_chain_dp
        assert np.array_equal(own[1], fx["heap_b"][fx["heap_b_off"][g]:fx["heap_b_off"][g + 1]])
        if not (np.array_equal(own[0], other[0]) and np.array_equal(own[1], other[1])):
            below += h[0] < common[0]
            above += h[0] > common[0]
    assert below >= 4 and above >= 4


def test_gap_formula_equals_the_recorded_pairs(fx):
    q = gm.qlen_sums(fx["frag_off"], fx["seq_off"])
    got = gm.frag_dists(q, *[int(v) for v in fx["gaps"]])
    assert np.array_equal(got, fx["par"][:, :2])
    assert (got[:, 0] == 100).any() and (got[:, 1] == 100).any() and (got[:, 0] > 100).any() and (got[:, 1] > 100).any()


def test_gap_formula_variants():
    q = np.array([0, 50, 100, 101, 699, 700, 701, 5000, 2**31 - 1])
    assert np.array_equal(gm.frag_dists(q, 1, 100, -1, 800)[:, 0], [800, 750, 700, 699, 101, 100, 100, 100, 100])
    assert np.array_equal(gm.frag_dists(q, 1, 100, -1, 800)[:, 1], [100, 100, 100, 101, 699, 700, 701, 5000, 2**31 - 1])
    assert np.array_equal(gm.frag_dists(q, 0, 100, -1, 800)[:, 1], [100] * 9)                      # not sr: max_gap
    assert np.array_equal(gm.frag_dists(q, 1, 100, 350, 800)[:, 0], [350] * 9)                     # max_gap_ref is always honoured
    assert np.array_equal(gm.frag_dists(q, 1, 100, 0, 0)[:, 0], [100] * 9)                         # no max_frag_len: max_gap
    assert np.array_equal(gm.frag_dists(q, 1, 100, -5, -1)[:, 0], [100] * 9)
