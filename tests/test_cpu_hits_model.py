"""CPU tests of the regions-to-hits model (tests/hits_model.py: mm_set_parent hit.c:125-186, mm_select_sub hit.c:255-272) and of the cases of tests/hits_data.py:
the model reproduces every byte the reference's own hit.o made of every case (tests/golden/ref_hits.npz), every family reaches the boundary it is named for, and the
"natural" restatements -- best primary instead of first, the parent read out of place, double instead of float, sam_pri always set -- give another output on the
planted cases, so the fixture can tell them from the reference."""
import os

import numpy as np
import pytest

import hits_data as D
import hits_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    Z = np.load(os.path.join(GOLDEN, "ref_hits.npz"))
    return {k: Z[k] for k in Z.files}


@pytest.fixture(scope="module")
def by_name():
    return {c["name"]: c for c in D.cases()}


def _want(ref, k):
    return ref["hits"][ref["hit_off"][k]:ref["hit_off"][k + 1]].reshape(-1).view(M.REG)


def test_fixture_matches_the_cases(ref):
    cs = D.cases()
    assert int(ref["reg_size"]) == M.REG.itemsize == 80
    assert [str(s) for s in ref["names"]] == [c["name"] for c in cs] and len(set(c["name"] for c in cs)) == len(cs)
    assert np.array_equal(ref["n_in"], [c["regs"].size for c in cs])
    assert np.array_equal(ref["opts"], np.array([D.opt_key(c["opt"]) for c in cs], np.float64))
    assert os.path.getsize(os.path.join(GOLDEN, "ref_hits.npz")) < (1 << 20)


def test_model_reproduces_every_byte_of_every_case(ref):
    for k, c in enumerate(D.cases()):
        got, want = M.select_hits(c["regs"], c["opt"]), _want(ref, k)
        assert got.size == int(ref["n_out"][k]) == want.size, f"{c['name']}: n = {got.size}, the reference {int(ref['n_out'][k])}"
        bad = [i for i in range(got.size) if got[i].tobytes() != want[i].tobytes()]
        assert not bad, f"{c['name']}: {len(bad)} of {got.size} hits differ, first at {bad[0]}:\n got {got[bad[0]]}\nwant {want[bad[0]]}"


def test_gap_measure_equals_the_sorted_sweep():
    """the kernel finds uncov_len as a measure, without klib's sort: equal keys of radix_sort_64 are equal values, so any exact union length is the reference's"""
    rng = np.random.default_rng(3)
    for _ in range(400):
        n = int(rng.integers(1, 12))
        s = rng.integers(0, 60, n)
        prim = [(int(a), int(a + b)) for a, b in zip(s, rng.integers(1, 30, n))]
        si = int(rng.integers(0, 50)); ei = si + int(rng.integers(1, 40))
        assert M.uncov_by_gaps(si, ei, prim) == M.uncov_len(si, ei, prim)[0], (si, ei, prim)
    for c in D.cases():                                                         # ... and on the primaries of every case
        r = M.set_parent(c["regs"], c["opt"]["mask_level"], c["opt"]["mask_len"], 0)
        prim = [(int(q["qs"]), int(q["qe"])) for q in r[r["parent"] == r["id"]]][:200]
        for q in r[::max(r.size // 40, 1)]:
            assert M.uncov_by_gaps(int(q["qs"]), int(q["qe"]), prim) == M.uncov_len(int(q["qs"]), int(q["qe"]), prim)[0]


def test_families_reach_their_boundaries(by_name):
    sp = lambda c: M.set_parent(c["regs"], c["opt"]["mask_level"], c["opt"]["mask_len"], c["opt"]["hard_mask_level"])
    assert by_name["empty"]["regs"].size == 0 and by_name["one"]["regs"].size == 1
    for n in (64, 65, 129, D.LDS_CLASS):
        r = sp(by_name[f"disjoint{n}"])
        assert r.size == n and np.array_equal(r["parent"], np.arange(n))
    r = sp(by_name["child_of_65th"])
    assert r["parent"][65] == 64 and r["parent"][66] == 66 and r["parent"][67] == 0 and r["subsc"][64] == 90 and r["n_sub"][64] == 1 and r["n_sub"][0] == 0
    r = sp(by_name["first_overlap_fails"])
    assert r["parent"][2] == 1 and r["parent"][1] == 1                          # region 2 overlaps primary 0 first, which fails
    r = sp(by_name["first_not_best"])
    assert list(r["parent"]) == [0, 1, 0, 0] and r["score"][1] > r["score"][0]
    for name, child in (("long_over_100_primary", False), ("long_over_100_child", True)):
        c = by_name[name]
        prim = [(int(q["qs"]), int(q["qe"])) for q in c["regs"][:100]]
        un, n_cov = M.uncov_len(0, 10000, prim)
        r = sp(c)
        assert n_cov == 100 and un == (1000 if child else 6000) and r["parent"][100] == (0 if child else 100)
    c = by_name["long_over_300_beyond"]
    assert M.uncov_len(0, 30000, [(int(q["qs"]), int(q["qe"])) for q in c["regs"][:300]])[1] == 300 and c["regs"].size > D.LDS_CLASS
    c = by_name["union_not_sum"]
    un, n_cov = M.uncov_len(400, 1800, [(0, 1000), (600, 1600)])
    assert (un, n_cov) == (200, 2) and 1400 - (600 + 1000) != un                 # the clipped intervals add up to more than their union
    assert list(sp(c)["parent"]) == [0, 1, 0, 1, 4] and list(sp(by_name["union_hard_mask_level"])["parent"]) == [0, 1, 0, 0, 4]
    assert [list(sp(by_name[f"mask_len_{v}"])["parent"]) for v in (100, 150, 149)] == [[0, 1, 2, 2, 4], [0, 0, 2, 2, 2], [0, 1, 2, 2, 4]]
    r = sp(by_name["n_sub_subsc"])
    assert r["n_sub"][0] == 2 and r["subsc"][0] == 70 and list(r["parent"][:4]) == [0, 0, 0, 0]    # cnt equal and above count, below does not; 50, then 70, not 60
    for v, kept in ((3, [100, 98, 97, 95]), (4, [100, 98, 97, 95, 94]), (2, [100, 98, 97])):
        assert list(M.select_hits(by_name[f"best_n_{v}"]["regs"], by_name[f"best_n_{v}"]["opt"])["score"]) == kept
    assert list(M.select_hits(by_name["pri_ratio_alone"]["regs"], by_name["pri_ratio_alone"]["opt"])["score"]) == [100, 80]
    assert list(M.select_hits(by_name["min_diff_alone"]["regs"], by_name["min_diff_alone"]["opt"])["score"]) == [100, 80, 79, 70]
    out = M.select_hits(by_name["nothing_dropped"]["regs"], by_name["nothing_dropped"]["opt"])
    assert out.size == 4 and not (out["flags"] >> M.SAM_PRI_BIT & 1).any()
    out = M.select_hits(by_name["first_dropped_only"]["regs"], by_name["first_dropped_only"]["opt"])
    assert out.size == 3 and list(out["flags"] >> M.SAM_PRI_BIT & 1) == [1, 0, 0] and list(out["parent"]) == [0, 1, 1] and list(out["id"]) == [0, 1, 2]
    for name in ("pri_ratio_zero", "pri_ratio_negative"):
        c = by_name[name]
        out = M.select_hits(c["regs"], c["opt"])
        assert out.size == c["regs"].size and (out["parent"] != out["id"]).any() and out.tobytes() == sp(c).tobytes()
    sizes = sorted(c["regs"].size for c in D.cases())
    assert D.LDS_CLASS in sizes and D.LDS_CLASS + 1 in sizes and sizes[-1] <= 4000


def test_float_edges_are_planted(by_name):
    """hit.c:165 at the level: pairs whose real value equals mask_level, and pairs on which float and real arithmetic disagree about `>`"""
    from fractions import Fraction
    D.cases()
    print("planted:", D.FLOAT_EDGE)
    kinds = {lvl: [e[0] for e in E] for lvl, E in D.FLOAT_EDGE.items()}
    assert kinds[0.5].count("eq") == len(D.EQ_05) and kinds[0.5].count("f32_no") == 3 and "f32_yes" not in kinds[0.5]   # (none exists: see hits_data)
    assert kinds[0.3].count("f32_yes") >= 1 and kinds[0.3].count("f32_no") == 3 and "eq" not in kinds[0.3]
    for lvl, E in D.FLOAT_EDGE.items():
        ml = np.float32(lvl)
        for kind, L, Mm, s in E:
            ol, mn, mx = L - s, min(L, Mm), max(L, Mm)
            real = Fraction(ol, mn) - Fraction(s, mx)
            f32 = np.float32(ol) / np.float32(mn) - np.float32(s) / np.float32(mx)
            assert abs(float(real) - float(ml)) < 2 ** -22                      # within an ulp or two of the level
            if kind == "eq":
                assert real == Fraction(float(ml)) and not f32 > ml
            else:
                assert (f32 > ml) == (kind == "f32_yes") and (real > Fraction(float(ml))) == (kind == "f32_no")
        c = by_name[f"float_edge_{lvl}"]
        r = M.set_parent(c["regs"], c["opt"]["mask_level"], c["opt"]["mask_len"], 0)
        n = len(E)
        assert [int(r["parent"][n + t]) == t for t in range(n)] == [e[0] == "f32_yes" for e in E]


def test_five_four_is_kept_in_float(by_name):
    c = by_name["five_four"]
    assert np.float32(4) >= np.float32(5) * np.float32(0.8) and not 4.0 >= 5.0 * float(np.float32(0.8))
    assert list(M.select_hits(c["regs"], c["opt"])["score"]) == [5, 4, 10, 8]


VARIANTS = {"pick": ({"pick": "best"}, ["first_not_best"]),
            "in_place": ({"in_place": False}, ["overwritten_keep_to_drop", "overwritten_drop_to_keep", "overwritten_identity_drop", "overwritten_identity_keep"]),
            "double": ({"fp": np.float64}, ["float_edge_0.5", "float_edge_0.3", "float_edge_0.3_keepall", "five_four", "pri_ratio_alone"]),
            "always_sync": ({"always_sync": True}, ["nothing_dropped", "disjoint64", "one"])}


@pytest.mark.parametrize("which", sorted(VARIANTS))
def test_natural_variants_differ_on_the_planted_cases(which, by_name, ref):
    kw, names = VARIANTS[which]
    idx = {c["name"]: k for k, c in enumerate(D.cases())}
    for name in names:
        c = by_name[name]
        assert M.select_hits(c["regs"], c["opt"], **kw).tobytes() != _want(ref, idx[name]).tobytes(), f"{name} does not tell `{which}` from the reference"


def test_overwritten_parent_flips_as_described(by_name):
    for name, n_ref, n_out_of_place in (("overwritten_keep_to_drop", 4, 5), ("overwritten_drop_to_keep", 5, 4), ("overwritten_identity_drop", 4, 5),
                                        ("overwritten_identity_keep", 5, 4)):
        c = by_name[name]
        r = M.set_parent(c["regs"], c["opt"]["mask_level"], c["opt"]["mask_len"], 0)
        assert list(r["parent"]) == [0, 0, 2, 3, 2, 5]
        assert M.select_hits(c["regs"], c["opt"]).size == n_ref and M.select_hits(c["regs"], c["opt"], in_place=False).size == n_out_of_place
