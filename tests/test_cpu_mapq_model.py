"""CPU test of tests/mapq_model.py against the reference's own hit.o (tests/golden/ref_mapq.npz): every byte of the final regions and of a[] for every case of
tests/mapq_data.py, with the host's logf; the planted cases are what they claim to be; and each natural wrong variant differs from the reference on the cases
planted for it."""
import os

import numpy as np
import pytest

import mapq_data as D
import mapq_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    Z = np.load(os.path.join(GOLDEN, "ref_mapq.npz"))
    cs = D.cases()
    assert int(Z["reg_size"]) == M.REG.itemsize and [str(v) for v in Z["names"]] == [c["name"] for c in cs]
    cut = lambda key, off, k: Z[key][Z[off][k]:Z[off][k + 1]]
    return {c["name"]: {"in": cut("hits_in", "in_off", k).reshape(-1).view(M.REG), "out": cut("hits_out", "out_off", k).reshape(-1).view(M.REG),
                        "a": cut("a_out", "a_off", k), "case": c, "libm": str(Z["libm"])} for k, c in enumerate(cs)}


def _model(R, **variant):
    c = R["case"]
    return M.join_mapq(R["in"], c["a"], c["qlen"], c["mapq"], c["rep_len"], **variant)


def _differs(R, **variant):
    return _model(R, **variant)[0].tobytes() != R["out"].tobytes()


def test_model_reproduces_every_byte_of_the_fixture(ref):
    bad = []
    for name, R in ref.items():
        r, a, _ = _model(R)
        if r.tobytes() != R["out"].tobytes() or a.tobytes() != R["a"].tobytes():
            bad.append(name)
    only_ulp = bad and all(n.startswith("ulp_") for n in bad)
    assert not bad, f"{len(bad)} case(s) differ: {bad[:8]}" + (f" -- only the one-ulp cases: this machine's libm is not the fixture's ({next(iter(ref.values()))['libm']})" if only_ulp else "")


def test_planted_cases_are_what_they_claim(ref):
    n_in = lambda name: ref[name]["in"].size
    n_cand = lambda name: int(((ref[name]["in"]["parent"] == np.arange(n_in(name))) | (ref[name]["in"]["parent"] < 0)).sum())
    assert (n_in("n0"), n_in("n1"), n_in("n2_join")) == (0, 1, 2) and ref["n2_join"]["out"].size == 1 and ref["n2_no_join"]["out"].size == 2
    assert n_in("n1_as_nonzero") == 1 and ref["n1_as_nonzero"]["out"]["as"][0] == 4 and ref["n1_as_nonzero"]["a"].shape[0] == 11   # no squeeze: as and a[] stay
    assert ref["no_join_no_squeeze"]["out"]["as"].min() == 4 and ref["no_join_no_squeeze"]["out"].size == 2
    assert n_in(f"hits{D.LDS_CLASS}") == D.LDS_CLASS and n_in(f"hits{D.LDS_CLASS + 1}") == D.LDS_CLASS + 1 and n_in("hits300") == 300
    assert n_cand("cand64") == 64 and n_cand("cand65") == 65
    assert ref["cascade70"]["out"].size == 1 and ref["cascade70"]["out"]["cnt"][0] == 210
    for at, off in (("x_one_more", "x_equal"), ("y_one_more", "y_equal"), ("max_gap_at", "max_gap_above"), ("max_gap_q_at", "max_gap_q_above"), ("min_gap_at", "min_gap_above"),
                    ("min_gap_q_at", "min_gap_q_above"), ("score0_at", "score0_below"), ("score1_at", "score1_below"), ("n2_join", "rid_differs"), ("n2_join", "strand_differs"),
                    ("rev_join", "rev_no_join"), ("adjacent_by_drop", "adjacency_broken_by_secondary"), ("grown_r1", "grown_r1_not_enough")) + \
            tuple((f"flank_{w}_at", f"flank_{w}_below") for w in ("r0_ref", "r0_query", "r1_ref", "r1_query")):
        assert ref[at]["out"].size == ref[at]["in"].size - (2 if at.startswith("grown") else 1), at
        assert ref[off]["out"].size == ref[off]["in"].size - (1 if off.startswith("grown") else 0), off
    # the join bit sits on the first anchor of the absorbed chain, in squeezed coordinates, and nowhere else
    bit = lambda name: np.nonzero(ref[name]["a"][:, 1] & np.uint64(M.MM_SEED_LONG_JOIN))[0].tolist()
    assert bit("n2_join") == [5] and bit("adjacent_by_drop") == [5] and bit("grown_r1") == [5, 9] and bit("n2_no_join") == [] and bit("n2_join_off") == []
    assert ref["adjacent_by_drop"]["a"].shape[0] == 10 and D.cases()[[c["name"] for c in D.cases()].index("adjacent_by_drop")]["a"].shape[0] == 14
    # the three branches of the mlen pair term give three different mlen behind the same two chains
    assert len({int(ref[f"mlen_pair_{g}"]["out"]["mlen"][0]) - 0 for g in ("100_200", "10_200", "200_10")}) >= 2
    # hierarchy: the secondary of the fourth chain ends without a parent in one order and with the kept first chain in the other
    assert ref["hier_fourth_outranks_third"]["out"]["parent"].tolist() == [0, -1] and ref["hier_third_outranks_fourth"]["out"]["parent"].tolist() == [0, 0]
    # filtering only behind a join
    assert ref["min_cnt_no_join"]["out"]["cnt"].min() == 2 and ref["min_cnt_with_join"]["out"]["cnt"].min() >= 3
    assert ref["min_cnt_5_with_join"]["out"]["cnt"].tolist() == [5, 5]
    # mapq: the cap, zero above score0, the values below the cap
    q = lambda name: (ref[name]["out"]["flags"] & 0xff).tolist()
    assert q("mapq_cap_60") == [60] and q("mapq_subsc_above_score0") == [0] and q("mapq_subsc39") == q("mapq_subsc40") != q("mapq_subsc41")
    assert ref["mapq_n_sub63"]["out"]["n_sub"][0] == 63 and ref["mapq_n_sub1"]["out"]["n_sub"][0] == 1 and ref["mapq_n_sub_smaller_cnt"]["out"]["n_sub"][0] == 0
    assert q("mapq_rep_len0") != q("mapq_rep_len100000") and 0 < q("mapq_after_join_score0")[0] < 60
    assert ref["mapq_after_join_score0"]["out"]["score"][0] != ref["mapq_after_join_score0"]["out"]["score0"][0]
    assert ref[f"table_score{D.SMALL_TABLE}"]["out"]["score"][0] == D.SMALL_TABLE and ref[f"table_score{D.SMALL_TABLE + 1}"]["out"]["score"].max() == D.SMALL_TABLE + 1


def test_sc_thres_edges_exist_only_under_other_options():
    e = D.sc_edges()
    assert e["default"] == (0, 0), "the default options have a max_gap at which float and exact (or float and double add) disagree: plant it"
    assert e["exact"] and e["f499"] and e == D.SC_EDGE or not D.SC_EDGE
    for kind in ("exact", "f499"):
        fsc, mjl, gap = e[kind]
        r, f, x = (int(v[0]) for v in D.sc_thres_variants(fsc, mjl, np.array([gap])))
        assert r != (x if kind == "exact" else f)
        assert any(c["name"] == f"sc_{kind}_{fsc}_{gap}" for c in D.cases())


def test_one_ulp_of_logf_changes_the_dozen(ref):
    names = [n for n in ref if n.startswith("ulp_")]
    assert len(names) == 12 == len(D.ULP_EDGE)
    base = lambda v: np.float32(np.log(np.float64(v)))
    for n in names:
        got = {_model(ref[n], log=lambda v, d=d: np.nextafter(base(v), np.float32(d)) if d is not None else base(v))[0].tobytes() for d in (None, 0, np.inf)}
        assert len(got) >= 2, f"{n}: one ulp of the logarithm does not change the result"


@pytest.mark.parametrize("variant,planted", [
    (dict(fp499="float"), ["sc_f499_"]),
    (dict(hier="parallel"), ["hier_third_outranks_fourth"]),
    (dict(filter_always=True), ["min_cnt_no_join"]),
    (dict(x_from="score"), ["mapq_after_join_score0"]),
    (dict(adj="unsqueezed"), ["adjacent_by_drop", "rev_adjacent_by_drop"]),
    (dict(log="np"), ["ulp_"]),
])
def test_natural_variants_differ_on_their_planted_cases(ref, variant, planted):
    for prefix in planted:
        names = [n for n in ref if n.startswith(prefix)]
        assert names and any(_differs(ref[n], **variant) for n in names), f"{variant} gives the reference's bytes on {names}"
        if not prefix.endswith("_"):
            assert all(_differs(ref[n], **variant) for n in names)


def test_beyond_the_table_only_the_primary_concerned_changes(ref):
    R = ref[f"table_score{D.SMALL_TABLE + 1}"]
    c = R["case"]
    r = M.set_mapq(M.join_mapq(R["in"], c["a"], c["qlen"], c["mapq"], c["rep_len"])[0], 40, 0, beyond=D.SMALL_TABLE)
    assert (r["flags"] & 0xff).tolist() == [0, int(R["out"]["flags"][1]) & 0xff] and (R["out"]["flags"][0] & 0xff) == 60
    at = ref[f"table_score{D.SMALL_TABLE}"]
    assert M.set_mapq(at["out"], 40, 0, beyond=D.SMALL_TABLE).tobytes() == at["out"].tobytes()
