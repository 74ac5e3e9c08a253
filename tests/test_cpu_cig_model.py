"""CPU test of the model of the CIGAR join (tests/cig_model.py) on the planted regions of tests/cig_data.py: every planted region comes to what its case says (the
appended CIGAR spelled out, the cut, the split decision, the coordinates), the second list holds the passes the z-drop codes ask for, the model's output goes through
extra_model's mm_update_extra with lengths that add up, and each wrong variant of cig_model.VARIANTS differs on its named planted case."""
import numpy as np
import pytest

import cig_data as D
import cig_model as M
import extra_model


@pytest.fixture(scope="module")
def planted():
    names, B = D.planted_batch()
    return names, B, D.model(B)


def text(ws):
    return "".join(f"{w >> 4}{D.OPS[w & 0xf]}" for w in ws)


def test_planted_regions_come_to_what_they_plant(planted):
    names, B, m = planted
    r = {k: (m["cig_regs"][i], text(m["cigs"][i])) for i, k in enumerate(names)}
    assert m["counts"] == (0, 0, 0) and all(x[0]["status"] == 0 for x in r.values())
    # mm_append_cigar: the left extension's last M takes the first fill's M; a run of one-word fills is one word; words inside an item stay
    assert r["both_ext"][1] == "20M1D55M2I40M3D93M" and r["merge"][1] == "114M2I8M" and r["no_merge"][1] == "50M2I3D68M" and r["inside_item"][1] == "5M6M2I8M"
    assert r["run65"][1] == "700M" and r["run65"][0]["n_used"] == 70 and r["ext_empty"][1] == "50M"
    # dp_score: max of an extension that has words, score of a fill, max of the dropped fill (cig_data.ez: score = 2 ql - 3, max = 2 ql + 1)
    assert r["both_ext"][0]["dp_score"] == (2 * 25 + 1) + (2 * 92 - 3) + (2 * 60 - 3) + (2 * 33 + 1)
    assert r["drop_split"][0]["dp_score"] == (2 * 4 + 1) + (2 * 50 - 3) + (2 * 30 + 1)
    # the cut: everything behind the dropped item is gone, the right extension too
    for k in ("drop_split", "drop_no_split", "drop_last", "drop_first", "rev_drop", "over_gap", "bad_behind_cut"):
        assert r[k][0]["dropped"] == 1 and r[k][0]["n_used"] == r[k][0]["drop_item"] + 1
    assert r["drop_last"][1] == "120M" and r["drop_first"][1] == "34M" and r["over_gap"][1] == "50M"
    # the split decision: cnt1 - (j + 1) >= min_cnt, the clamp, <=
    assert r["drop_split"][0]["split_n"] == 3 and r["drop_no_split"][0]["split_n"] == 0 and r["drop_exact_min_cnt"][0]["split_n"] == 2
    assert r["j_clamp"][0]["split_n"] == 1 and r["j_clamp"][0]["has_p"] == 1 and r["j_clamp"][0]["n_cigar"] == 0 and r["j_eq"][0]["split_n"] == 7
    assert r["code2_split_inv"][0]["split_inv"] == 1 and r["code2_split_inv"][0]["zdrop_code"] == 2 and r["second_differs"][0]["zdrop_code"] == 1
    # the second pass replaces the first: its words and its scalars
    assert r["code1"][1] == "90M1I18M" and r["second_differs"][0]["dp_score"] == (2 * 50 - 3) + 55
    # the strand flip of :782
    q = r["rev"][0]
    i = names.index("rev")
    rd = int(np.searchsorted(B["u_off"], i, side="right") - 1)
    qlen = int(B["read_off"][rd + 1] - B["read_off"][rd])
    assert (q["r_qs"], q["r_qe"]) == (qlen - q["qe1"], qlen - q["qs1"]) and r["both_ext"][0]["r_qs"] == r["both_ext"][0]["qs1"]
    # reach_end: qs1 = qs0 and mqe_t, not max_t
    L = r["left_reach_end"][0]
    g = names.index("left_reach_end")
    assert L["qs1"] == B["aregs"][g]["qs0"] and L["qe1"] == B["aregs"][g]["qe0"]


def test_second_list(planted):
    names, B, m = planted
    S = B["second"]
    assert S["totals"][0] == 3 and S["n_over"] == 0
    k = [int(B["aregs"][names.index(n)]["item0"]) + 1 for n in ("code1", "code2_split_inv", "second_differs")]
    assert [int(S["second_of"][i]) for i in k] == [0, 1, 2] and (np.delete(S["second_of"], k) == -1).all()
    assert [int(x) for x in S["tasks2"]["zdrop"]] == [400, 200, 400] and (S["tasks2"]["flag"] & M.APPROX_MAX == 0).all()
    for n, i in enumerate(k):
        T0, T2 = B["tasks"][B["items"][i]["task"]], S["tasks2"][n]
        assert all(T0[f] == T2[f] for f in ("q_off", "t_off", "qlen", "tlen", "w", "end_bonus"))
        assert S["cig_off2"][n + 1] - S["cig_off2"][n] == M.slot_of(int(T2["qlen"]) + int(T2["tlen"]), 0)
    # sr: the ungapped item's own test
    R = D.sr_batch()
    assert [int(x) for x in R["second_of"] if x >= 0] == [0, 1] and R["second"]["totals"][0] == 2
    assert all(int(T["flag"]) == 0 and int(T["end_bonus"]) == -1 and int(T["w"]) == 151 and int(T["zdrop"]) == 100 for T in R["tasks2"])
    mr = D.model(R)["cig_regs"]
    assert [int(x) for x in mr["zdrop_code"]] == [0, 0, 1, 0] and [int(x) for x in mr["dropped"]] == [0, 0, 1, 0] and mr["status"].tolist() == [0, 0, 0, 0]
    assert M.sr_test([0] * 20, [0] * 10 + [1] * 10, D.mat_of(2, 8, 1), 79) == 1 and M.sr_test([0] * 20, [0] * 10 + [1] * 10, D.mat_of(2, 8, 1), 80) == 0


def test_output_goes_through_update_extra(planted):
    """the extra tasks carry the lengths the appended CIGAR consumes (the assert of :284), so extra_model.update_extra takes every one"""
    names, B, m = planted
    rng = np.random.default_rng(3)
    mat = D.mat_of(2, 4, 1)
    for k, g in enumerate(m["extra_reg"]):
        T = m["extra_tasks"][k]
        c0 = int(m["in_off"][k])
        cig = m["cig_out"][c0:c0 + int(T["n_cigar"])]
        assert D.lens([int(w) for w in cig]) == (int(T["qlen"]), int(T["tlen"])), names[g]
        q, t = rng.integers(0, 4, int(T["qlen"])).astype(np.uint8), rng.integers(0, 4, int(T["tlen"])).astype(np.uint8)
        out = extra_model.update_extra(q, t, cig, mat, 4, 2, 0)
        assert out is not None


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_each_wrong_variant_differs_on_its_planted_case(planted, variant):
    names, B, m = planted
    g = names.index(D.DIFFERS[variant])
    if variant == "zdrop_for_inv":
        S = M.second_pass(B["opt"], B["aregs"], B["items"], B["tasks"], B["zres"], B["pool"], B["mat"], variant=variant)
        k = int(B["second_of"][int(B["aregs"][g]["item0"]) + 1])
        assert S["tasks2"][k]["zdrop"] != B["tasks2"][k]["zdrop"] and (np.delete(S["tasks2"], k) == np.delete(B["tasks2"], k)).all()
        return
    w = D.model(B, variant=variant)
    assert w["cig_regs"][g] != m["cig_regs"][g] or w["cigs"][g] != m["cigs"][g], (variant, names[g])


def test_limits_are_what_their_names_say():
    L = D.limits()
    m = {k: D.model(b) for k, b in L.items()}
    assert all(x["counts"] == (0, 0, 0) for x in m.values())
    assert [int(x) for x in m["items"]["cig_regs"]["n_used"]] == [0, 1, 2, 63, 64, 65, 129, 63, 64, 65, 129]
    assert [int(x) for x in m["words"]["cig_regs"]["n_cigar"][:4]] == [1, 255, 256, 257]
    assert [int(x) for x in m["drops"]["cig_regs"]["drop_item"][:6]] == [63, 64, 63, 64, 127, 128]
    d = m["drops"]["cig_regs"]
    assert int(d[6]["split_n"]) == 1 and int(d[7]["split_n"]) == 0 and int(d[8]["dropped"]) == 1   # j is anchor 0 of 129 at the end of the scan; j is the last anchor in front
    assert int(m["merges"]["cig_regs"][4]["n_cigar"]) == 1 and int(m["merges"]["cig_regs"][4]["n_used"]) == 600
