"""CPU test of the model of the CIGAR join against the reference's own mm_align1 (tests/golden/ref_cig.npz): per option set of tests/cig_data.ref_batches() the recorded
ksw calls, both passes with their CIGAR words, go through cig_model as the join's inputs; the second list is the calls the reference made, and the join reproduces
the region's CIGAR and dp_score in front of mm_update_extra, has_p, the split with r2's as, cnt and split_inv, and -- through extra_model's mm_update_extra -- the final
rs, re, qs, qe, dp_max, blen, mlen, n_ambi and CIGAR of r and r->p.  A split region goes through a Python mm_split_reg in float32 and a second and third round equal
the records of the regions the reference split off.  Every wrong variant of the model differs from the record on at least one region."""
import numpy as np
import pytest

import aln_data as AD
import cig_data as D
import cig_model as M
import cig_ref

KINDS = ("undropped_both_ext", "no_left", "no_right", "left_reach_end_1", "left_reach_end_0", "right_reach_end_1", "right_reach_end_0", "ext_n_cigar_0", "dropped_split",
         "dropped_no_split", "j_clamp", "drop_first", "drop_last", "code1", "code2_split_inv", "second_differs", "over_left", "over_gap", "over_right", "merge", "no_merge",
         "run65", "sr_test_0", "sr_test_1", "rev_undropped", "rev_dropped", "child")


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(AD.OPTS))
def test_model_reproduces_the_reference(name, level):
    B, names = cig_ref.batch(name, level)
    m = cig_ref.model_of(name, level)
    bad = cig_ref.mismatches(name, B, m["cig_regs"], m["cigs"], level)
    assert not bad, (name, level, len(bad), [(names[x[0]],) + tuple(x[1:]) for x in bad[:5]])
    assert m["counts"] == (int((B["aregs"]["status"] != 0).sum()), 0, 0)


def test_fixture_reaches_every_kind():
    """the conditions the generator refuses to write without hold on the committed fixture: every kind reached by the reference alone, at most half the regions dropped,
    children on two levels"""
    fx = cig_ref.fixture()
    assert sorted(fx["kinds_reached"].tolist()) == sorted(KINDS)
    n, d = fx["counts"].tolist()
    assert n == sum(len(fx[cig_ref.prefix(k, l) + "hd"]) for k in AD.OPTS for l in range(3)) and 0 < 2 * d <= n
    assert sum(len(fx[k + "_c1_hd"]) for k in AD.OPTS) >= 10 and sum(len(fx[k + "_c2_hd"]) for k in AD.OPTS) >= 2
    assert all(o["flag"] & 1 or o["zdrop"] != o["zdrop_inv"] for o in D.ref_opts().values())


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_each_wrong_variant_differs_from_the_record(variant):
    """on the reference's own regions, not only on the planted ones: some region of the record is not reproduced by the wrong variant"""
    n_bad = 0
    for name in sorted(AD.OPTS):
        for level in (0, 1):
            B, _ = cig_ref.batch(name, level)
            if variant == "zdrop_for_inv":                                     # the second list's zdrop argument is the recorded call's: batch() asserts it
                S = M.second_pass(B["opt"], B["aregs"], B["items"], B["tasks"], B["zres"], B["pool"], B["mat"], variant=variant)
                n_bad += int((S["tasks2"]["zdrop"] != B["tasks2"]["zdrop"]).sum())
                continue
            w = D.model(B, variant=variant)
            n_bad += len(cig_ref.mismatches(name, B, w["cig_regs"], [c if c is not None else [] for c in w["cigs"]], level))
    if variant in ("merge_inside_items", "append_behind_drop"):
        # no input reaches these: ksw_push_cigar merges equal neighbouring ops itself, so the reference never holds two words of one op inside an item; and the
        # reference makes no call behind a drop, so the record has no ez a wrong join could append there (those tasks carry ksw status 1 here; a right
        # extension over max_sw_mat behind a drop is the one item that needs no call, and `right_behind_drop` does differ on it).  The two variants are equal on the
        # record; the planted regions of tests/cig_data.py (`inside_item`, `drop_first`) tell them apart
        assert n_bad == 0, variant
    else:
        assert n_bad > 0, variant
