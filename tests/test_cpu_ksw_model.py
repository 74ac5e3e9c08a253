"""The NumPy restatement of ksw_extd2_sse (tests/ksw_model.py) against what the reference's own ksw2_extd2_sse.o made of every case of tests/ksw_data.py
(tests/golden/ref_ksw.npz): equal in all eleven ez fields and every CIGAR word.  Then the eight mistakes a kernel that computes "the band" would make, each of which
must differ from the fixture on a planted case named here -- so the fixture can tell such a kernel from the reference."""
import os

import numpy as np
import pytest

import ksw_data as D
import ksw_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    path = os.path.join(GOLDEN, "ref_ksw.npz")
    assert os.path.exists(path), "tests/golden/ref_ksw.npz is absent"
    fx = np.load(path)
    cs = D.cases()
    assert [c["name"] for c in cs] == list(fx["names"])
    return cs, fx["ez"], fx["cig_off"], fx["cigar"]


def _same(ref, k, variant=None):
    cs, ez, off, cig = ref
    e, g = M.run_case(cs[k], D.score_set, variant)
    return np.array_equal(e, ez[k]) and np.array_equal(g, cig[off[k]:off[k + 1]])


def test_fixture_covers_what_it_claims(ref):
    cs, ez, off, cig = ref
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names) and sum(n.startswith("rnd") for n in names) == 2000
    assert {c["flag"] for c in cs if c["name"].startswith("len_17_17/")} == set(D.ALL_FLAGS) and len(set(D.ALL_FLAGS)) == 64
    assert all(c["flag"] & ~D.SUPPORTED == 0 for c in cs)
    zd, reach = ez[:, 1] == 1, ez[:, 10] == 1
    assert zd.sum() > 100 and reach.sum() > 10
    closes = [k for k, c in enumerate(cs) if c["name"].startswith("band_closes") and not c["flag"] & D.SCORE_ONLY]
    assert all(ez[k, 1] == 1 for k in closes)                                    # zdropped without a z-drop
    ret = [k for k, c in enumerate(cs) if c["sc"] == "ret"]
    assert ret and all(tuple(ez[k]) == (0, 0, -1, -1, M.NEG_INF, -1, M.NEG_INF, -1, M.NEG_INF, 0, 0) for k in ret)
    ops = np.bincount(cig & 0xf, minlength=3)
    assert ops[0] > 0 and ops[1] > 0 and ops[2] > 0
    assert any((cig[off[k]:off[k + 1]] >> 4).max(initial=0) >= 60 for k, c in enumerate(cs) if c["name"].startswith(("ins60/", "del60/")))


def test_planted_and_limit_cases(ref):
    cs = ref[0]
    bad = [cs[k]["name"] for k in range(len(cs)) if not cs[k]["name"].startswith("rnd") and not _same(ref, k)]
    assert not bad, bad[:10]


def test_random_cases(ref):
    cs = ref[0]
    bad = [cs[k]["name"] for k in range(len(cs)) if cs[k]["name"].startswith("rnd") and not _same(ref, k)]
    assert not bad, bad[:10]


# the planted case on which each mistake shows (found by running the variant over the planted cases; any one suffices)
CAUGHT_BY = {
    "real_only": "len_17_17/f00",
    "s_exact": "w_1/f00",
    "tie_low_t": "tie_lanes_141/f00",
    "mte_q_en0": "len_17_17/f00",
    "off_unpadded": "w_2/f00",
    "right_as_left": "len_16_16/f02",
    "reach_ge": "extz_equal_eb0/f40",
    "no_clamp": "sc_asm10_N/f00",
}


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_wrong_variant_differs_on_its_planted_case(ref, variant):
    cs = ref[0]
    k = [c["name"] for c in cs].index(CAUGHT_BY[variant])
    assert not cs[k]["name"].startswith("rnd")
    assert _same(ref, k) and not _same(ref, k, variant)


def test_planted_cases_reach_what_their_names_say(ref):
    """the backtracks of the leave_band_right cases take force_state 1, those of the leave_band_left cases force_state 2; the row cases walk padded rows of the stated widths; the LDS corner fills the image"""
    cs = ref[0]
    by = {c["name"]: c for c in cs}

    def stats(name):
        st = {}
        M.run_case(by[name], D.score_set, stats=st)
        return st
    for name in ("leave_band_right_16/f00", "leave_band_right_16/f40", "leave_band_right_17/f00", "leave_band_right_17/f40"):
        assert stats(name).get("force") == {1}, name
    for name, want in (("leave_band_left_156/f00", {1, 2}), ("leave_band_left_575/f00", {2}), ("leave_band_left_1054/f00", {2}), ("leave_band_left_575/f80", {2})):
        assert stats(name).get("force") == want, name
    assert {64, 80} <= stats("row_64_lanes")["widths"] and max(stats("row_64_lanes")["widths"]) == 80
    assert {64, 80, 96} <= stats("row_65_lanes")["widths"] and max(stats("row_65_lanes")["widths"]) == 96
    assert {128, 144} <= stats("row_129_lanes")["widths"] and max(stats("row_129_lanes")["widths"]) == 144
    c = by["lds_last_both_2304"]
    assert c["q"].size == 2304 and c["t"].size == 2304 and 12 * 2304 + 32 + 2304 + 16 == 30000
    assert all(by["p_over_4mib_%d" % k]["w"] == 2000 for k in range(3))
