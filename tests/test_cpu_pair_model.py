"""The Python model of the pair plan (tests/pair_model.py) against the reference's own mm_pair (tests/golden/ref_pair.npz, made by make_ref_pair_fixtures.py from
pe.o): every planted case and every simulated pair byte for byte, every required kind reached by the reference, every natural wrong variant told apart by the case
planted for it, the flip of map.c:455-466 against values derived by hand, and what the plan does where the reference has no counterpart (the table's end, refusals).
The fixture's mapq values are its build host's logf (its version string is `libm` in the file): if this file fails on mapq alone after a change of the C library,
the fixture is made again by the committed script."""
import numpy as np
import pytest

import pair_data as D
import pair_model as M

PLANTED, REAL, LIBM = D.fixture()
REQUIRED = ("one_end_only", "no_pair_pe_thru", "single_floor2", "floor1", "equal_hi_no_floor", "lift_mate0", "lift_mate1", "old_primary_mapq_zeroed", "sam_pri_moved",
            "under_dp_thres", "pe_bonus_above_sum", "gap_eq_accepted", "gap_plus1_rejected", "break_on_rid", "far_last_hides", "equal_scores_first_wins", "hash_wraps",
            "sub_diff_counted", "sub_diff_not_counted", "alt_lowers", "negative_alt", "blend_raises", "contraction", "pe_thru_off_by_3", "two_primaries", "n64", "n65",
            "ties_gt64_not_stable", "lds_128", "scratch_129", "n300", "n_sub_beyond_table")
REQUIRED_REAL = ("real_one_candidate", "real_several_candidates", "real_one_end_only", "real_both_no_pair")


def same(got, want):
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_fixture_holds_every_case_and_kind():
    assert set(PLANTED) == {c["name"] for c in D.cases() if not c["refuse"]}
    reached = set().union(*(e["kinds"] for e in PLANTED.values()))
    assert not [k for k in REQUIRED if k not in reached]
    rreached = set().union(*(d["kinds"] for d in REAL))
    assert not [k for k in REQUIRED_REAL if k not in rreached]
    assert 100 <= len(REAL) <= 400


def test_model_is_the_reference_on_the_planted_cases():
    bad = []
    for name, e in PLANTED.items():
        m0, m1, _ = M.pair(e["case"]["regs"][0], e["case"]["regs"][1], e["case"]["pext"], e["case"]["qlens"], e["case"]["opt"], gap=e["case"]["gap"])
        if not same((m0, m1), e["out"]):
            only_mapq = all((g["flags"] | 0xff == w["flags"] | 0xff).all() and g["parent"].tobytes() == w["parent"].tobytes() for g, w in zip((m0, m1), e["out"]))
            bad.append((name, "mapq alone" if only_mapq else "more than mapq"))
    assert not bad, f"{bad}" + (f" -- this machine's libm may not be the fixture's ({LIBM})" if all(b[1] == "mapq alone" for b in bad) else "")


def test_model_is_the_reference_on_the_simulated_pairs():
    for f, d in enumerate(REAL):
        c = D.real_case(d)
        m0, m1, info = M.pair_case(c)
        m1["p"] = d["in"][1][0]["p"]
        assert same((m0, m1), (d["out"][0][0], d["out"][1][0])), f"simulated pair {f}"
        assert not (m0["flags"] >> M.PROPER_FRAG_BIT & 1).any() or "real_one_candidate" in d["kinds"] or "real_several_candidates" in d["kinds"]


def test_only_the_named_fields_change():
    """parent and the four bit groups of flags; nothing else of a region, and nothing at all of a fragment with one end only"""
    mask = np.uint32(0xff | 1 << M.SAM_PRI_BIT | 1 << M.PROPER_FRAG_BIT | 1 << M.PE_THRU_BIT)
    for name, e in PLANTED.items():
        for s in range(2):
            a, b = e["case"]["regs"][s].copy(), e["out"][s].copy()
            if min(r.size for r in e["case"]["regs"]) == 0:
                assert a.tobytes() == b.tobytes(), name
            a["parent"] = b["parent"] = 0
            a["flags"] &= ~mask; b["flags"] &= ~mask
            assert a.tobytes() == b.tobytes(), name


VARIANTS = [   # (variant, the case planted for it, cases on which it must still be the reference)
    (dict(sort="stable"), "alternate_71", ("alternate_64",)),
    (dict(sort="stable"), "alternate_132", ()),
    (dict(sort="stable"), "alternate_65", ()),
    (dict(winner="ge"), "equal_scores_j", ("single_floor2",)),
    (dict(winner="ge"), "equal_scores_i", ()),
    (dict(stop="continue"), "break_hides_long", ("far_last_hides", "break_on_rid")),
    (dict(stop="continue", first_test=False), "far_last_hides", ()),
    (dict(n_sub="others"), "sub_diff_eq", ("single_floor2",)),
    (dict(second="distinct"), "max_twice", ("floor1", "equal_hi_no_floor")),
    (dict(lift_mapq="keep"), "lift_mate0", ("single_floor2",)),
    (dict(lift_mapq="keep"), "lift_mate1", ()),
    (dict(pe_thru="before"), "lift_pe_thru", ("no_pair_pe_thru",)),
    (dict(fp="fused"), "contraction", ("blend_raises", "alt_lowers")),
]


@pytest.mark.parametrize("variant,name,still", VARIANTS, ids=[f"{'-'.join(f'{k}={v}' for k, v in v.items())}@{n}" for v, n, _ in VARIANTS])
def test_wrong_variant_differs_on_its_case(variant, name, still):
    e = PLANTED[name]
    assert not same(M.pair_case(e["case"], **variant)[:2], e["out"]), f"{variant} is the reference on {name}"
    for other in still:
        assert same(M.pair_case(PLANTED[other]["case"], **variant)[:2], PLANTED[other]["out"]), f"{variant} differs on {other}"


def test_first_test_alone_is_implied_by_the_walk():
    """pe.c:115 tests a[last] exactly as the walk's first step does (a[last] has r's rev and the other mate: its key is even, r's is odd), so leaving it out
    changes nothing on its own; it is the walk's break that it repeats.  With `continue` in the walk it is what still hides the nearer candidate."""
    for name, e in PLANTED.items():
        assert same(M.pair_case(e["case"], first_test=False)[:2], M.pair_case(e["case"])[:2]), name
    e = PLANTED["far_last_hides"]
    assert same(M.pair_case(e["case"], stop="continue")[:2], e["out"])


def test_sort_matches_the_issue_s_check():
    """70 regions of mate 0 alternating between two rs, one region of mate 1 behind the first group: the reference marks input index 34, a stable sort 68; at 131
    it marks 66, not 130; at 63 the stable answer 62 is right"""
    w = lambda name: int(np.nonzero(PLANTED[name]["out"][0]["flags"] >> M.PROPER_FRAG_BIT & 1)[0][0])
    assert (w("alternate_71"), w("alternate_132"), w("alternate_64")) == (34, 66, 62)
    assert M.pair_case(PLANTED["alternate_71"]["case"], sort="stable")[2]["winners"][0] == 68
    assert M.pair_case(PLANTED["alternate_132"]["case"], sort="stable")[2]["winners"][0] == 130


def test_flip_by_hand():
    for c, want in D.flip_cases():
        m = M.pair_case(c)[:2]
        noflip = M.pair(c["regs"][0], c["regs"][1], c["pext"], c["qlens"], dict(c["opt"], flip=0))[:2]
        for s in range(2):
            if want[s] is None:
                assert m[s].tobytes() == noflip[s].tobytes(), c["name"]
                continue
            got = [(int(r["qs"]), int(r["qe"]), int(r["flags"]) >> M.REV_BIT & 1) for r in m[s]]
            assert got == want[s], c["name"]
            a, b = m[s].copy(), noflip[s].copy()
            for r in (a, b):
                r["qs"] = r["qe"] = 0
                r["flags"] &= ~np.uint32(1 << M.REV_BIT)
            assert a.tobytes() == b.tobytes(), c["name"]


def test_beyond_the_table_leaves_the_winners_mapq():
    e = PLANTED["n_sub_beyond_table"]
    c = e["case"]
    m0, m1, info = M.pair_case(c)
    assert info["beyond"] and info["n_sub"] == 10 > c["max_log_arg"] and info["found"]
    w = info["winners"]
    for s, m in enumerate((m0, m1)):
        assert int(m["flags"][w[s]]) & 0xff == int(c["regs"][s]["flags"][w[s]]) & 0xff
        a, b = m.copy(), e["out"][s].copy()
        a["flags"][w[s]] &= ~np.uint32(0xff); b["flags"][w[s]] &= ~np.uint32(0xff)
        assert a.tobytes() == b.tobytes()                                      # everything else is the reference's
    assert not same((m0, m1), e["out"])


def test_refused_cases():
    ref = [c for c in D.cases() if c["refuse"]]
    assert len(ref) >= 8
    for c in ref:
        with pytest.raises(M.Refused):
            M.pair_case(c)


def test_chain_of_models_on_the_simulated_pairs():
    """the finish model on the lists in front of mm_filter_regs gives the lists in front of mm_pair (regions and the records their p names): the fixture's three
    recordings hang together, and the GPU chain FinPlan -> PairPlan has a host-side twin"""
    import fin_model as FM
    from mm2chain import params
    o = params.fin_opts("sr")
    od = {k: getattr(o, k) for k in FM.OPT_FIELDS}
    for f, d in enumerate(REAL):
        for s in range(2):
            r, px = d["pre"][s]
            m = FM.finish(r, px, d["qlens"][s], d["rep_len"], od, max_log_arg=1 << 20)
            w, wpx = d["in"][s]
            g, w = m["regs"].copy(), w.copy()
            assert g.size == w.size, f"pair {f} mate {s}"
            if g.size:
                assert m["pext"][g["p"].astype(int) - 1].tobytes() == wpx[w["p"].astype(int) - 1].tobytes(), f"pair {f} mate {s}"
            g["p"] = w["p"] = 0
            assert g.tobytes() == w.tobytes(), f"pair {f} mate {s}"
