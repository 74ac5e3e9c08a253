"""CPU test of tests/seg_model.py against the reference's own hit.o and pe.o (tests/golden/ref_seg.npz): every byte of the array behind mm_select_sub_multi, of every
segment's chains, anchors and regions out of mm_seg_gen, and of the final per-segment regions, for every case of tests/seg_data.py; the planted cases are what they
claim to be; and each natural wrong variant differs from the reference on the cases planted for it."""
import numpy as np
import pytest

import regs_model
import seg_data as D
import seg_model as M


@pytest.fixture(scope="module")
def ref():
    R = D.reference()
    if R is None:
        pytest.skip("tests/golden/ref_seg.npz is absent (tests/golden/make_ref_seg_fixtures.py makes it from the reference's objects)")
    return {r["name"]: r for r in R}


def _sel_differs(ref, names, **variant):
    return [n for n in names if M.frag_hits(ref[n]["case"], **variant).tobytes() != ref[n]["sel"].tobytes()]


def _seg_differs(ref, names, **variant):
    bad = []
    for n in names:
        R, c = ref[n], ref[n]["case"]
        got = M.seg_gen(c["hash"], c["n_segs"], c["qlens"], R["sel"], c["a"], **variant)
        if any(u.tobytes() != S["u"].tobytes() or a.tobytes() != S["a"].tobytes() or r.tobytes() != S["regs"].tobytes() for (u, a, r), S in zip(got, R["segs"])):
            bad.append(n)
    return bad


def test_model_reproduces_every_byte_of_the_fixture(ref):
    assert not _sel_differs(ref, list(ref)), "mm_select_sub_multi"
    assert not _seg_differs(ref, list(ref)), "mm_seg_gen"
    bad = []
    for n, R in ref.items():
        for S in R["segs"]:
            if M.seg_final(R["case"], S["regs"]).tobytes() != S["final"].tobytes():
                bad.append(n)
    assert not bad, f"final regions differ in {bad[:8]}; logf is the host's: the fixture was made with {next(iter(ref.values()))['libm']}"


def test_planted_cases_are_what_they_claim(ref):
    n_out = lambda n: ref[n]["sel"].size
    n_in = lambda n: ref[n]["case"]["u"].size
    assert n_out("sel_primaries_only") == 3 and n_out("sel_min_diff_70") == 2 and n_out("sel_min_diff_69") == 1
    assert n_out("sel_pri_ratio_0.0") == 3 and n_out("sel_pri_ratio_-1.0") == 3 and not (ref["sel_pri_ratio_0.0"]["sel"]["flags"] >> 12 & 1).any()
    for side in ("down", "up"):
        assert [n_out(f"sel_dist_{side}_{D_}") for D_ in (799, 800, 801)] == [2, 1, 1]
    assert n_out("sel_dist_799_other_rev") == 1 and n_out("sel_dist_799_other_rid") == 1
    assert n_out("sel_gap_ref_500") == 2 and n_out("sel_gap_ref_499") == 1 and n_out("sel_gap_ref_wraps") == 1
    assert [n_out(f"sel_both_par{p}_chi{c}") for p, c in ((0, 0), (1, 1), (0, 1), (1, 0))] == [2, 2, 2, 1]
    assert [n_out(f"sel_both_{n}") for n in ("par_qs149", "par_qs150", "par_qe150", "par_qe151", "chi_qs149", "chi_qs150", "chi_qe150", "chi_qe151")] == [1, 2, 2, 1, 2, 1, 1, 2]
    assert n_out("sel_three_segs_not_close") == 1 and n_out("sel_three_segs_no_both") == 2
    for fam, scs in (("pri1", (19, 20, 21)), ("pri_ratio", (49, 50, 51)), ("pri2", (69, 70, 71))):
        assert [n_out(f"sel_{fam}_{s}") for s in scs] == [1, 2, 2], fam
    assert n_out("f32_pri1_5_1") == 2 and n_out("f32_pri_ratio_08") == 2 and n_out("f32_pri2_03") == 2
    assert [n_out(f"sel_best_n_{b}") for b in (0, 1, 3)] == [1, 2, 4] and n_out("sel_best_n_2_one_fails") == 3
    assert n_out("sel_identical_kept") == 2
    assert n_out("sel_overwritten_score") == 4 and n_out("sel_overwritten_rev") == 3 and n_out("sel_overwritten_both") == 3
    nd = ref["sel_nothing_dropped"]["sel"]
    assert nd.size == 4 and not (nd["flags"] >> 12 & 1).any() and (ref["sel_first_child_dropped"]["sel"]["flags"] >> 12 & 1).tolist() == [1, 0, 0]
    assert n_in("sel_random128") == 128 and n_in("sel_random129") == 129 and 1 < n_out("sel_random128") < 128 and 1 < n_out("sel_random129") < 129
    # mm_seg_gen
    seg_n = lambda n: [(S["u"].size, S["a"].shape[0]) for S in ref[n]["segs"]]
    assert seg_n("seg_which_segment") == [(2, 8), (2, 8)] and seg_n("seg_empty_fragment") == [(0, 0), (0, 0)]
    assert seg_n("seg_zero_length_segment")[1] == (0, 0) and all(nu > 0 for nu, _ in seg_n("seg_three_segs_middle"))
    assert ref["seg_dropped_region"]["sel"].size == 3 and sum(na for _, na in seg_n("seg_dropped_region")) == 17
    # a segment said by the anchor, not by its place: y - acc borrows from the upper word, the 64-bit subtraction hit.c:414 is
    assert any(int(S["regs"]["qs"].min()) < 0 for S in ref["seg_change_63_64"]["segs"])
    assert seg_n("seg_change_63_64") == [(1, 64), (1, 66)] and seg_n("seg_change_64_65") == [(1, 65), (1, 65)] and seg_n("seg_long_run") == [(1, 130), (1, 70)]
    assert [sum(na for _, na in seg_n(f"seg_cnt_{n}")) for n in (63, 64, 65)] == [63, 64, 65]
    as_, cnt = ref["seg_across_4096"]["sel"]["as"], ref["seg_across_4096"]["sel"]["cnt"]
    assert ((as_ < 4096) & (as_ + cnt > 4096)).any()
    assert ref["seg_regions_64"]["sel"].size == 64 and ref["seg_regions_65"]["sel"].size == 65
    tied = 0
    for S in ref["seg_tied_keys_70"]["segs"]:
        zx = [z[0] for z in regs_model.keys(ref["seg_tied_keys_70"]["case"]["hash"], S["u"], S["a"])]
        tied += len(zx) - len(set(zx))
    assert [S["u"].size for S in ref["seg_tied_keys_70"]["segs"]] == [70, 0] and tied == 10
    c = ref["seg_tied_keys_70"]["case"]                                         # ... and klib's order among them is not the stable one
    assert any(M.seg_gen(c["hash"], 2, c["qlens"], ref["seg_tied_keys_70"]["sel"], c["a"], sort=regs_model.stable_sort)[s][2].tobytes() != S["regs"].tobytes()
               for s, S in enumerate(ref["seg_tied_keys_70"]["segs"]))


def test_wrong_variants_differ_on_their_planted_cases(ref):
    sel = [n for n in ref if n.startswith(("sel_", "f32_"))]
    d = lambda **v: set(_sel_differs(ref, sel, **v))
    assert {"f32_pri1_5_1", "f32_pri_ratio_08", "f32_pri2_03"} <= d(fp=np.float64)
    assert {"sel_pri1_20", "sel_pri_ratio_50", "sel_pri2_70"} <= d(strict=True)
    assert {"sel_dist_down_800", "sel_dist_up_800"} <= d(dist_le=True)
    assert {"sel_overwritten_score", "sel_overwritten_rev", "sel_overwritten_both"} <= d(in_place=False)
    assert "sel_identical_kept" in d(identical_drop=True)
    assert d(max_dist_any=True) == {"sel_three_segs_not_close"}
    assert "sel_best_n_2_one_fails" in d(count_all=True)
    seg = [n for n in ref if n.startswith("seg_")]
    assert "seg_mixed_strand_bits" in _seg_differs(ref, seg, turn_by="region") and "seg_reverse_spans" not in _seg_differs(ref, seg, turn_by="region")
    assert {"seg_reverse_spans", "seg_three_segs_middle"} <= set(_seg_differs(ref, seg, forget_qlen=True))
    assert "seg_dropped_region" in _seg_differs(ref, seg, order="as")
