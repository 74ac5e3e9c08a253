"""CPU tests of the regions-to-hits cases at the kernel's own limits (tests/hits_limit_data.py, tests/golden/ref_hits_limits.npz): the model reproduces every byte
the reference's hit.o made of them, every family reaches the population condition it is named for (n_cov, the region's start covered or not, equal ends in different
rounds of 64 candidates, the w index of the passing primary, kept), the kernel's gap measure equals the sorted sweep on every region, and the two wrong forms of the
measure -- the round of the region's start lost, every equal end opening the gap -- change the cases named for them and no other family."""
import os

import numpy as np
import pytest

import hits_limit_data as L
import hits_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    Z = np.load(os.path.join(GOLDEN, "ref_hits_limits.npz"))
    return {k: Z[k] for k in Z.files}


@pytest.fixture(scope="module")
def by_name():
    return {c["name"]: c for c in L.cases()}


def _want(ref, k):
    return ref["hits"][ref["hit_off"][k]:ref["hit_off"][k + 1]].reshape(-1).view(M.REG)


def _sp(c, **kw):
    return M.set_parent(c["regs"], c["opt"]["mask_level"], c["opt"]["mask_len"], c["opt"]["hard_mask_level"], **kw)


_WALKS = {}


def _walk(c):
    if c["name"] not in _WALKS:
        _WALKS[c["name"]] = _walk_once(c)
    return _WALKS[c["name"]]


def _walk_once(c):
    """mm_set_parent with its inner state: per region (n_cov, un of the sweep, clipped intervals in w order, w indices of the primaries that pass)"""
    r, o = c["regs"], c["opt"]
    w, out = [0], [None]
    for i in range(1, r.size):
        si, ei = int(r["qs"][i]), int(r["qe"][i])
        prim = [(int(r["qs"][j]), int(r["qe"][j])) for j in w]
        un, n_cov = M.uncov_len(si, ei, prim)
        cov = [(max(a, si), min(b, ei)) for a, b in prim if not (b <= si or a >= ei)]
        ok = [t for t, (a, b) in enumerate(prim) if not (b <= si or a >= ei) and M.passes(si, ei, a, b, un, o["mask_level"], o["mask_len"])]
        out.append((n_cov, un, cov, ok))
        if not ok:
            w.append(i)
    return out


def test_fixture_matches_the_cases(ref):
    cs = L.cases()
    assert int(ref["reg_size"]) == M.REG.itemsize == 80
    assert [str(s) for s in ref["names"]] == [c["name"] for c in cs]
    assert np.array_equal(ref["n_in"], [c["regs"].size for c in cs])
    assert np.array_equal(ref["opts"], np.array([L.opt_key(c["opt"]) for c in cs], np.float64))
    assert os.path.getsize(os.path.join(GOLDEN, "ref_hits_limits.npz")) < 1000000
    assert max(c["regs"].size for c in cs) <= 4000


def test_model_reproduces_every_byte_of_every_case(ref):
    for k, c in enumerate(L.cases()):
        got, want = M.select_hits(c["regs"], c["opt"]), _want(ref, k)
        assert got.size == int(ref["n_out"][k]) == want.size, f"{c['name']}: n = {got.size}, the reference {int(ref['n_out'][k])}"
        bad = [i for i in range(got.size) if got[i].tobytes() != want[i].tobytes()]
        assert not bad, f"{c['name']}: {len(bad)} of {got.size} hits differ, first at {bad[0]}:\n got {got[bad[0]]}\nwant {want[bad[0]]}"


def test_gap_measure_equals_the_sorted_sweep_on_every_region():
    for c in L.cases():
        r = c["regs"]
        w = [0]
        par = _sp(c)["parent"]
        for i in range(1, r.size):
            prim = [(int(r["qs"][j]), int(r["qe"][j])) for j in w]
            si, ei = int(r["qs"][i]), int(r["qe"][i])
            assert M.uncov_by_gaps(si, ei, prim) == M.uncov_len(si, ei, prim)[0], (c["name"], i)
            if par[i] == i:
                w.append(i)


def test_pairs_pin_uncov_len_from_both_sides(by_name):
    """at mask_len = un the pinned region is a child, at un - 1 a primary, and un is what the sweep gives"""
    assert L.cases() and len(L.PIN) == 2 * len(L.GAP_N) + 5
    for stem, (i, un) in L.PIN.items():
        kid, pri = by_name[stem + "_child"], by_name[stem + "_primary"]
        assert kid["regs"].tobytes() == pri["regs"].tobytes() and kid["regs"].size == i + 1
        assert kid["opt"]["mask_len"] == un and pri["opt"]["mask_len"] == un - 1
        assert _walk(kid)[i][1] == un and _walk(pri)[i][1] == un
        assert _sp(kid)["parent"][i] != i and _sp(pri)["parent"][i] == i, stem


def test_families_reach_their_populations(by_name):
    for n in L.GAP_N:
        for fam, covered in (("start_gap", False), ("start_covered", True)):
            c = by_name[f"{fam}_{n}_child"]
            n_cov, un, cov, ok = _walk(c)[n]
            si = int(c["regs"]["qs"][n])
            assert n_cov == n and c["regs"].size == n + 1 and any(a <= si < b for a, b in cov) == covered and ok and ok[0] == 0
            assert all(_walk(c)[i][0] == 0 for i in range(1, n))                # the primaries are disjoint: all of them are in w
    assert {n for n in L.GAP_N if n % L.ROUND == 0} == {64, 128, 192} and 127 + 1 == L.LDS_CLASS
    for stem, at in (("equal_ends", (0, 1)), ("equal_ends_across_rounds", (0, 65)), ("equal_ends_triple", (0, 1, 2))):
        c = by_name[stem + "_child"]
        i = L.PIN[stem][0]
        n_cov, un, cov, ok = _walk(c)[i]
        ei = int(c["regs"]["qe"][i])
        assert n_cov == i and _sp(c)["parent"][:i].tolist() == list(range(i))   # everything before the pinned region is a primary
        g = cov[0][1]
        assert [t for t in range(n_cov) if cov[t][1] == g] == list(at) and g < ei and not any(a <= g < b for a, b in cov)   # the equal ends, and a gap behind them
    assert 65 // L.ROUND != 0 // L.ROUND                                        # ... in different rounds of candidates
    c = by_name["equal_ends_child"]
    v = np.float32(500) / np.float32(500) - np.float32(500) / np.float32(1000)
    assert v == np.float32(0.5) and _sp(c)["parent"][1] == 1                    # the second primary: its value is the level, not above it
    c = by_name["equal_ends_triple_child"]
    assert _walk(c)[2][1] == 300 > c["opt"]["mask_len"] and _sp(c)["parent"][2] == 2
    c = by_name["clipped_to_end_child"]
    n_cov, un, cov, ok = _walk(c)[2]
    assert n_cov == 2 and all(b == int(c["regs"]["qe"][2]) for _, b in cov) and sum(int(q["qe"]) > int(c["regs"]["qe"][2]) for q in c["regs"][:2]) == 2 and un == 100
    for n in (65, 129):
        c = by_name[f"tiled_{n}"]
        W = _walk(c)
        assert [W[n][0], W[n][1], W[n + 1][0], W[n + 1][1]] == [n, 0, n, 0] and n > L.ROUND and c["opt"]["mask_len"] == 0
        assert _sp(c)["parent"][n:].tolist() == [0, 1]
    for k in L.PASS_AT:
        c = by_name[f"passing_at_{k}"]
        W, r = _walk(c), _sp(c)
        assert W[k + 1][3] == [k] and W[k + 1][0] == 1 and r["parent"][k + 1:].tolist() == [k, k + 2, 0] and r["subsc"][k] == 90 and r["n_sub"][k] == 1
    for k in (63, 127):
        c = by_name[f"passing_at_{k}_and_{k + 1}"]
        assert _walk(c)[k + 2][3] == [k, k + 1] and k // L.ROUND != (k + 1) // L.ROUND and _sp(c)["parent"][k + 2] == k
        c = by_name[f"passing_at_{k - 1}_and_{k}"]
        assert _walk(c)[k + 2][3] == [k - 1, k] and (k - 1) // L.ROUND == k // L.ROUND and _sp(c)["parent"][k + 2] == k - 1
    c = by_name["sole_overlap_round3_child"]
    n_cov, un, cov, ok = _walk(c)[130]
    assert n_cov == 1 and ok == [129] and 129 // L.ROUND == 2 and cov[0][1] - cov[0][0] == 40 and c["regs"].size > L.LDS_CLASS
    for name, kept in (("kept_1_of_130", 1), ("kept_129_of_130", 129)):
        c = by_name[name]
        r, out = _sp(c), M.select_hits(c["regs"], c["opt"])
        assert c["regs"].size == 130 > L.LDS_CLASS and (r["parent"] == 0).all() and out.size == kept
        assert out["id"].tolist() == list(range(kept)) and (out["flags"] >> M.SAM_PRI_BIT & 1).tolist() == [1] + [0] * (kept - 1)
    assert 100 not in M.select_hits(by_name["kept_129_of_130"]["regs"], by_name["kept_129_of_130"]["opt"])["score"][1:] and by_name["kept_129_of_130"]["regs"]["score"][66] == 100
    c = by_name["best_n_0"]
    r, out = _sp(c), M.select_hits(c["regs"], c["opt"])
    assert (r["parent"] != r["id"]).sum() == 4 and out["score"].tolist() == [100, 97] and (out["parent"] == out["id"]).all()
    assert M.select_hits(c["regs"], dict(c["opt"], best_n=1)).size == 3         # (the scores would keep them)


WRONG = {"round_lost": (M.uncov_by_gaps_round_lost, [f"start_gap_{n}_primary" for n in (64, 128, 192)]),
         "every_end": (M.uncov_by_gaps_every_end, ["equal_ends_child", "equal_ends_across_rounds_child", "equal_ends_triple_child"])}


@pytest.mark.parametrize("which", sorted(WRONG))
def test_wrong_measures_change_the_cases_named_for_them_and_no_other_family(which, ref):
    f, names = WRONG[which]
    changed = [c["name"] for k, c in enumerate(L.cases()) if M.select_hits(c["regs"], c["opt"], uncov=f).tobytes() != _want(ref, k).tobytes()]
    assert changed == names                                                    # these, and no case of any other family
    fams = {L.FAMILY[n] for n in names}
    assert len(fams) == (1 if which == "round_lost" else 3)
    for k, c in enumerate(L.cases()):                                          # the kernel's measure itself changes nothing
        if L.FAMILY[c["name"]] in fams:
            assert M.select_hits(c["regs"], c["opt"], uncov=M.uncov_by_gaps).tobytes() == _want(ref, k).tobytes()
