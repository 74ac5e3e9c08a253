"""CPU tests of the fragment model (tests/frag_model.py) against what the reference's own mm_map_frag did with n_segs = 2 and 3 under -x sr
(tests/golden/ref_frag.npz, made by tests/golden/make_ref_frag_fixtures.py): collect_minimizers, collect_matches over the joined list, the re-chain
decision of map.c:318-331 and, through the oracle's seed hits and mm_chain_dp, the chains themselves.  All comparisons are bit for bit."""
import os

import numpy as np
import pytest

import frag_model as fm
import sketch_model as sm

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_frag.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


def _segs(fx, g):
    fo, so, seq = fx["frag_off"], fx["seq_off"], fx["seq"]
    return [seq[so[s]:so[s + 1]].tobytes() for s in range(fo[g], fo[g + 1])]


def _par(fx, g):
    from mm2chain import params
    h = fx["par"][g]
    return params.make_params(max_dist_x=int(h[0]), max_dist_y=int(h[1]), bw=int(h[2]), max_skip=int(h[3]), max_iter=int(h[4]), gap_scale=float(fx["gap_scale"][g]),
                              is_cdna=int(h[7]), n_segs=int(h[8])), int(h[5]), int(h[6])


def test_fixture_holds_every_kind():
    z = np.load(FIX)
    n_segs = np.diff(z["frag_off"])
    for c in "abcdef":
        for n in (2, 3):
            assert (n_segs[z["kind_" + c]] == n).sum() >= 3, (c, n)
    assert (z["heap_rechained"][z["kind_a"]] == 1).all() and (z["heap_rechained"][z["kind_b"]] == 1).all()
    assert (z["heap_rechained"][z["kind_c"]] == 0).all() and (z["rep_len1"][z["kind_c"]] > 0).all() and (z["rep_len1"][z["kind_d"]] == 0).all()
    assert int(z["max_occ"]) > int(z["mid_occ"])


@pytest.mark.parametrize("hpc", [0, 1])
def test_collect_minimizers_and_matches(fx, hpc):
    p = "hpc_" if hpc else ""
    k, w, mid_occ = int(fx["k"]), int(fx["w"]), int(fx["mid_occ"])
    lookup = sm.table_lookup(fx[p + "keys"], fx[p + "cr_off"], fx[p + "n"])
    mo, fo = fx[p + "mini_off"], fx[p + "match_off"]
    for g in range(fx["frag_off"].size - 1):
        mini = fm.collect_minimizers(_segs(fx, g), w, k, bool(hpc))
        assert np.array_equal(mini, fx[p + "mini"][mo[g]:mo[g + 1]]), f"fragment {g}: minimizers"
        m, rep_len, mini_pos = sm.collect_matches(mini, lookup, mid_occ)
        assert np.array_equal(sm.match_array(m), fx[p + "matches"][fo[g]:fo[g + 1]]), f"fragment {g}: matches"
        assert rep_len == fx[p + "rep_len1"][g] and np.array_equal(np.array(mini_pos, np.uint64), fx[p + "mini_pos1"][fo[g]:fo[g + 1]]), f"fragment {g}"


def test_boundary_minimizer_is_tandem_on_both_sides(fx):
    """kind (e): the same minimizer last in one segment and first in the next -- both matches carry the tandem bit, with different segment ids"""
    mo, fo = fx["mini_off"], fx["match_off"]
    lookup = sm.table_lookup(fx["keys"], fx["cr_off"], fx["n"])
    for g in fx["kind_e"]:
        mini = fx["mini"][mo[g]:mo[g + 1]]
        j = np.nonzero((mini[1:, 0] >> np.uint64(8) == mini[:-1, 0] >> np.uint64(8)) & (mini[1:, 1] >> np.uint64(32) != mini[:-1, 1] >> np.uint64(32)))[0]
        assert j.size
        m = fx["matches"][fo[g]:fo[g + 1]]
        kept = [i for i in range(mini.shape[0]) if lookup(int(mini[i, 0]) >> 8)[1] < int(fx["mid_occ"])]
        for i in j:
            if i in kept and i + 1 in kept:
                a, b = m[kept.index(i)], m[kept.index(i + 1)]
                assert a["seg_tandem"] & 1 and b["seg_tandem"] & 1 and a["seg_tandem"] >> 1 != b["seg_tandem"] >> 1


@pytest.mark.parametrize("variant,heap,flag", [("heap", True, 0), ("radix", False, 0), ("heap_for", True, 0x100000)])
def test_rechain_decision_and_chains(fx, variant, heap, flag):
    k, w, mid_occ, max_occ = int(fx["k"]), int(fx["w"]), int(fx["mid_occ"]), int(fx["max_occ"])
    lookup = sm.table_lookup(fx["keys"], fx["cr_off"], fx["n"])
    v = lambda name: fx[variant + "_" + name]
    for g in range(fx["frag_off"].size - 1):
        par, min_cnt, min_sc = _par(fx, g)
        r = fm.map_frag(_segs(fx, g), w, k, lookup, fx["pool"], par, min_cnt, min_sc, mid_occ, max_occ, heap=heap, flag=flag)
        assert r["rechained"] == bool(v("rechained")[g]), f"fragment {g}: re-chain decision"
        assert r["rep_len"] == v("rep_len")[g] and r["n_anchors"] == v("na")[g]
        assert np.array_equal(r["mini_pos"], v("mini_pos")[v("mp_off")[g]:v("mp_off")[g + 1]])
        assert np.array_equal(r["u"], v("u")[v("u_off")[g]:v("u_off")[g + 1]]) and np.array_equal(r["b"], v("b")[v("b_off")[g]:v("b_off")[g + 1]]), f"fragment {g}: chains"
        f = r["first"]
        assert f["n_anchors"] == v("na1")[g] and np.array_equal(f["u"], v("u1")[v("u1_off")[g]:v("u1_off")[g + 1]])
        assert np.array_equal(f["b"], v("b1")[v("b1_off")[g]:v("b1_off")[g + 1]])
        if variant == "heap":
            assert np.array_equal(r["anchors"], fx["heap_a"][fx["heap_a_off"][g]:fx["heap_a_off"][g + 1]])


def test_best_chain_is_the_first_of_the_largest():
    """map.c:322-325: `max < score` from 0 keeps the FIRST chain among equals"""
    seg = lambda s: np.uint64(s << 48)
    u = np.array([50 << 32 | 2, 50 << 32 | 2], np.uint64)
    b = np.array([[1, seg(0) | 10], [2, seg(0) | 40], [3, seg(0) | 10], [4, seg(1) | 200]], np.uint64)
    assert fm.n_chained_segs(u, b) == 1 and fm.rechain(8, 40, 5, 2, u, b)
    assert fm.n_chained_segs(u[::-1], b[[2, 3, 0, 1]]) == 2 and not fm.rechain(8, 40, 5, 2, u, b[[2, 3, 0, 1]])
    assert not fm.rechain(8, 8, 5, 2, u, b) and not fm.rechain(8, 40, 0, 2, u, b) and fm.rechain(8, 40, 5, 2, u[:0], b[:0])
