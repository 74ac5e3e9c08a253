"""CPU test of the rules of DESIGN 3.18: tests/extra_model.py reproduces every byte the reference's own mm_update_extra and mm_test_zdrop gave on the cases of
tests/extra_data.py (tests/golden/ref_extra.npz), and each wrong variant of the model differs from the fixture on the planted case named here.  Three variants
cannot differ on any input the reference is defined on (extra_model's docstring says why); for them the test asserts that they agree everywhere."""
import os

import numpy as np
import pytest

import extra_data as D
import extra_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UF = ("n_cigar", "qshift", "tshift", "blen", "mlen", "n_ambi", "dp_max")


@pytest.fixture(scope="module")
def fx():
    path = os.path.join(GOLDEN, "ref_extra.npz")
    assert os.path.exists(path), "tests/golden/ref_extra.npz is absent"
    f = np.load(path)
    us, zs = D.update_cases(), D.zdrop_cases()
    assert [c["name"] for c in us] == list(f["u_names"]) and [c["name"] for c in zs] == list(f["z_names"])
    return dict(us=us, zs=zs, u_res=f["u_res"], u_off=f["u_cig_off"], u_cig=f["u_cigar"], z_res=f["z_res"])


def u_equal(fx, k, x, wrong=None):
    c = fx["us"][k]
    mat, q, e = D.score_set(c["sc"])[:3]
    got = M.update_extra(c["q"], c["t"], c["cigar"], mat, q, e, x, wrong)
    ref = fx["u_res"][k, x]
    want = fx["u_cig"][fx["u_off"][2 * k + x]:fx["u_off"][2 * k + x + 1]]
    return [got[f] for f in UF] == [int(v) for v in ref[:7]] and np.array_equal(got["cigar"], want)


def z_equal(fx, k, wrong=None):
    c = fx["zs"][k]
    mat, q, e = D.score_set(c["sc"])[:3]
    ref = fx["z_res"][k]
    for s, thr in enumerate(D.ZD_THR):
        g = M.test_zdrop(c["q"], c["t"], c["cigar"], mat, q, e, thr[0], thr[1], thr[2], thr[3] != 0, wrong)
        if s == 0:
            ok = (g["max_zdrop"], g["t0"], g["t1"] - g["t0"], g["q1"] - g["q0"]) == tuple(int(v) for v in ref[:4]) and M.revcomp_hash(c["q"], g["q0"], g["q1"]) == int(ref[4]) & 0xffffffff
            if not ok:
                return False
        if (g["code"], g["inv_cand"]) != (int(ref[5 + 2 * s]), int(ref[6 + 2 * s])):
            return False
    return True


def test_the_issues_example(fx):
    k = [c["name"] for c in fx["us"]].index("repeat_6M1I5M/ont/r0")
    assert D.text(fx["u_cig"][fx["u_off"][2 * k]:fx["u_off"][2 * k + 1]]) == "4M1I7M" and [int(v) for v in fx["u_res"][k, 0, 3:7]] == [12, 11, 0, 16]


def test_model_reproduces_update_extra(fx):
    bad = [(fx["us"][k]["name"], x) for k in range(len(fx["us"])) for x in (0, 1) if not u_equal(fx, k, x)]
    assert not bad, bad[:10]
    r = fx["u_res"]
    assert (r[:, :, 1] > 0).any() and (r[:, :, 2] > 0).any() and (r[:, 1, 0] > r[:, 0, 0]).any() and (r[:, :, 5] > 0).any()


def test_model_reproduces_test_zdrop(fx):
    bad = [fx["zs"][k]["name"] for k in range(len(fx["zs"])) if not z_equal(fx, k)]
    assert not bad, bad[:10]
    z = fx["z_res"]
    assert (z[:, 5] == 1).any() and (z[:, 6] == 1).any() and (z[:, 7] == 1).any() and (z[:, 8] == 1).any() and (z[:, 0] == 0).any()


WRONG_UPDATE = {                      # variant -> (planted case, is_eqx)
    "cap_no_shift": ("cap_through_shift/ont/r0", 0),
    "skip_twice": ("run_second_behind/ont/r0", 0),
    "strip_before_return": ("n1_I/ont/r0", 0),
    "mismatch_X": ("eqx_mismatch_words/ont/r0", 1),
}
WRONG_ZDROP = {"tie_earliest": "max_tie_later_wins", "drop_latest": "two_equal_drops"}


@pytest.mark.parametrize("wrong", sorted(WRONG_UPDATE))
def test_wrong_update_variant_differs_on_its_planted_case(fx, wrong):
    name, x = WRONG_UPDATE[wrong]
    k = [c["name"] for c in fx["us"]].index(name)
    assert u_equal(fx, k, x) and not u_equal(fx, k, x, wrong)


@pytest.mark.parametrize("wrong", sorted(WRONG_ZDROP))
def test_wrong_zdrop_variant_differs_on_its_planted_case(fx, wrong):
    k = [c["name"] for c in fx["zs"]].index(WRONG_ZDROP[wrong])
    assert z_equal(fx, k) and not z_equal(fx, k, wrong)


@pytest.mark.parametrize("wrong", ["no_skip", "nm_ignored", "merge_prev"])
def test_variants_that_cannot_differ_agree_on_planted_and_random_cases(fx, wrong):
    ks = [k for k, c in enumerate(fx["us"]) if not c["name"].startswith(("ksw/", "big_", "ont_", "words_", "homo_"))]
    assert all(u_equal(fx, k, x, wrong) for k in ks for x in (0, 1))


def test_undefined_inputs_are_named():
    mat, q, e = D.score_set("ont")[:3]
    for cig, ql, tl in (([5 << 4 | 4], 5, 5), ([3 << 4, 0 << 4 | 3, 3 << 4], 6, 6), ([0, 1, 2], 0, 0), ([5 << 4, 2 << 4 | 1], 6, 5), ([5 << 4, 2 << 4 | 2, 3 << 4], 8, 9)):
        with pytest.raises(M.Undefined):
            M.update_extra(np.zeros(ql, np.uint8), np.zeros(tl, np.uint8), cig, mat, q, e, 0)
