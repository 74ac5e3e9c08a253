"""CPU tests of the finish-plan model (tests/fin_model.py) and of the cases of tests/fin_data.py: the model reproduces every byte the reference's own hit.o made of
every case (tests/golden/ref_fin.npz: mm_filter_regs, mm_hit_sort, mm_set_parent, mm_select_sub, mm_set_sam_pri, mm_set_mapq on regions with r->p, and
mm_split_reg), with the stages in between; and each "natural" restatement gives another output on the case planted for it and on nothing it should not.
The fixture's mapq values are its build host's logf; the model calls this host's (mapq_model.logf)."""
import os

import numpy as np
import pytest

import fin_data as D
import fin_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    Z = np.load(os.path.join(GOLDEN, "ref_fin.npz"))
    return {k: Z[k] for k in Z.files}


@pytest.fixture(scope="module")
def cases():
    return [c for c in D.cases() if not c["refuse"]]


def want(ref, k):
    lo, hi = int(ref["out_off"][k]), int(ref["out_off"][k + 1])
    return ref["hits_out"][lo:hi].reshape(-1).view(M.REG), ref["out_idx"][lo:hi], ref["out_dp_max2"][lo:hi]


def run(c, **kw):
    return M.finish(c["regs"], c["pext"], c["qlen"], c["rep_len"], c["opt"], **kw)


def test_fixture_matches_the_cases(ref, cases):
    assert int(ref["reg_size"]) == M.REG.itemsize == 80 and M.PEXT.itemsize == 32
    assert [str(s) for s in ref["names"]] == [c["name"] for c in cases]
    assert [str(s) for s in ref["split_names"]] == [s["name"] for s in D.split_cases()]
    assert os.path.getsize(os.path.join(GOLDEN, "ref_fin.npz")) < (1 << 20)
    reached = set(",".join(str(k) for k in ref["kinds"]).split(","))
    for kind in ("ties_gt64_not_stable", "tie_le64_later_first", "clip_float_keeps", "identical_no_dp_max2", "floor_504", "mapq_p_dp2", "mapq_p_no_dp2", "mapq_no_p",
                 "scratch_129", "lds_128", "n300", "sam_pri_rewritten_without_drop", "p_follows_survivors"):
        assert kind in reached


def test_model_reproduces_every_byte_of_every_case(ref, cases):
    for k, c in enumerate(cases):
        got = run(c)
        hits, idx, dp2 = want(ref, k)
        keep = M.filter_regs(c["regs"], c["pext"], c["qlen"], c["opt"])
        assert keep == list(ref["flt_idx"][int(ref["flt_off"][k]):int(ref["flt_off"][k + 1])]), c["name"]
        assert M.hit_sort(c["regs"], c["pext"], keep) == list(ref["srt_idx"][int(ref["srt_off"][k]):int(ref["srt_off"][k + 1])]), c["name"]
        assert got["idx"] == list(idx), c["name"]
        bad = [i for i in range(hits.size) if got["regs"][i].tobytes() != hits[i].tobytes()]
        assert not bad, f"{c['name']}: {len(bad)} of {hits.size} hits differ, first at {bad[0]}:\n got {got['regs'][bad[0]]}\nwant {hits[bad[0]]}"
        for t, i in enumerate(idx):
            if c["regs"]["p"][i]:
                assert int(got["pext"]["dp_max2"][int(c["regs"]["p"][i]) - 1]) == int(dp2[t]), (c["name"], t)


def test_refused_cases_are_refused():
    for c in D.cases():
        if c["refuse"]:
            with pytest.raises(M.Refused):
                run(c)


def test_split_reg_is_the_references(ref):
    for k, s in enumerate(D.split_cases()):
        r1, r2 = M.split_reg(s["reg"], s["n"], s["split_inv"], s["qlen"], s["a"])
        w1, w2 = ref["split_r"][k].view(M.REG)[0], ref["split_r2"][k].view(M.REG)[0]
        r2["flags"] = (int(r2["flags"]) & ~(1 << M.SPLIT_INV_BIT))                 # align.c:759 sets split_inv behind mm_split_reg
        assert r2.tobytes() == w2.tobytes(), (s["name"], r2, w2)
        for f in ("cnt", "score", "id", "parent", "as", "hash", "subsc", "n_sub", "score0"):   # (the parent's coordinates and lengths are overwritten by align.c:781-783)
            assert r1[f] == w1[f], (s["name"], f)
        assert int(r1["flags"]) >> 8 & 3 == int(w1["flags"]) >> 8 & 3
    s = [s for s in D.split_cases() if s["name"] == "float_double"][0]
    assert M.split_reg(s["reg"], s["n"], 0, s["qlen"], s["a"], split_fp="float")[1]["score"] != ref["split_r2"][3].view(M.REG)[0]["score"]


def _two_sorted_with_p(c):
    """the key of hit.c:203 matters: more than one region reaches the sort, with p (the cases' chain scores are all alike, so a key from them orders by hash)"""
    keep = M.filter_regs(c["regs"], c["pext"], c["qlen"], c["opt"])
    return len(keep) > 1 and bool(c["regs"]["p"][keep].any())


def _hits_without_a_drop(c):
    """mm_set_sam_pri of map.c:267 is the only one that runs: hits are left, mm_select_sub dropped none, and map.c:265-267 are not skipped"""
    m = run(c)
    return not c["opt"]["all_chains"] and m["regs"].size > 0 and m["regs"].size == len(M.hit_sort(c["regs"], c["pext"], M.filter_regs(c["regs"], c["pext"], c["qlen"], c["opt"])))


# variant -> (keywords, the cases it must differ on, where else it may: a list of names or a predicate of the case); on every other case it must not differ
VARIANTS = {"clip_double": (dict(clip="double"), ["clip_float"], []),
            "stable_sort": (dict(sort="stable"), ["n65_ties", "n128_ties", "n129_ties", "n300_ties"], []),
            "key_score": (dict(key="score"), ["two_reordered", "tie_child"], _two_sorted_with_p),
            "dp2_identical": (dict(dp2_identical=True), ["identical_after_dp"], []),
            "sam_pri_on_drop": (dict(sam_pri="on_drop"), ["sam_pri_nothing_dropped"], _hits_without_a_drop),
            "xx_fused": (dict(xx="fused"), ["xx_not_fused"], []),
            "alt_under_sr": (dict(alt_under_sr=True), ["alt_below_sr1"], ["alt_above_sr1"]),
            }


@pytest.mark.parametrize("which", sorted(VARIANTS))
def test_natural_variants_differ_on_the_planted_cases(which, ref, cases):
    kw, must, may = VARIANTS[which]
    differs = [c["name"] for k, c in enumerate(cases) if run(c, **kw)["regs"].tobytes() != want(ref, k)[0].tobytes()]
    print(which, "differs on", differs)
    assert set(must) <= set(differs), f"`{which}` is not told from the reference by {sorted(set(must) - set(differs))}"
    allowed = set(must) | (set(c["name"] for c in cases if may(c)) if callable(may) else set(may))
    assert set(differs) <= allowed, f"`{which}` differs where it should not: {sorted(set(differs) - allowed)}"


def test_model_reproduces_the_reads_rebuilt_from_the_alignment_record(ref):
    """ont, asm20 and sr as mm_align_skeleton holds them behind its loop (fin_data.real_cases), against what the reference's hit.o made of them"""
    rc = D.real_cases()
    assert [str(s) for s in ref["real_names"]] == [c["name"] for c in rc] and len(rc) > 300
    reached = set(",".join(str(k) for k in ref["real_kinds"]).split(","))
    assert {"real_child_kept", "real_grandchild_kept", "real_filtered", "real_sort_reorders", "real_all_gone"} <= reached
    for k, c in enumerate(rc):
        lo, hi = int(ref["real_out_off"][k]), int(ref["real_out_off"][k + 1])
        got = run(c)
        assert got["idx"] == list(ref["real_out_idx"][lo:hi]), c["name"]
        assert got["regs"].tobytes() == ref["real_hits_out"][lo:hi].tobytes(), c["name"]
        assert [int(got["pext"]["dp_max2"][int(c["regs"]["p"][i]) - 1]) for i in got["idx"]] == list(ref["real_out_dp_max2"][lo:hi]), c["name"]


def test_interleave_rounds_makes_the_rebuilt_lists():
    """mm2chain.interleave_rounds on what the apply entry writes round by round (here made from the reference's record, p = index in the round + 1) gives every read's
    list as fin_data.real_reads rebuilds it: a child directly behind its parent, p renumbered into the rounds' concatenated records; and it refuses a child_of that
    does not name the next round's regions in order"""
    import cig_ref
    import mm2chain
    fx = cig_ref.fixture()
    for name in ("ont", "asm20", "sr"):
        o, u_off, regs, b_off, b, read_off, fwd, names = cig_ref.inputs(name, 0)
        bb = np.asarray(b, np.uint64).reshape(-1, 2)
        made, cur = [], np.array(regs, M.REG)
        for lv in range(3):
            hd = fx[cig_ref.prefix(name, lv) + "hd"]
            if len(hd) == 0:
                break
            out, px, kids, of = cur.copy(), np.zeros(len(hd), M.PEXT), [], []
            for g, h in enumerate(hd):
                rd = int(np.searchsorted(u_off, g, side="right") - 1)
                if h[12] > 0:
                    out["cnt"][g] -= h[12]; out["score"][g] -= h[24]; out["flags"][g] |= 1 << 8
                    kids.append(cig_ref.split_reg(cur[g], int(h[13]) - int(cur[g]["as"]), int(h[14]), int(read_off[rd + 1] - read_off[rd]), bb[int(b_off[rd]):int(b_off[rd + 1])]))
                    of.append(g)
                out["rs"][g], out["re"][g], out["qs"][g], out["qe"][g] = h[1], h[2], h[3], h[4]
                if h[5]:
                    out["blen"][g], out["mlen"][g], out["p"][g] = h[8], h[9], g + 1
                    px[g] = (h[6], h[7], 0, h[10], h[11], 0, 0)
            made.append(dict(u_off=u_off, regs=out, pext=px, child_of=np.array(of, np.int32)))
            per = np.bincount(np.searchsorted(u_off, of, side="right") - 1, minlength=len(u_off) - 1) if of else np.zeros(len(u_off) - 1, np.int64)
            u_off, cur = np.concatenate([[0], np.cumsum(per)]).astype(np.int64), (np.array(kids, M.REG).reshape(-1) if kids else np.zeros(0, M.REG))
        f_off, L, LP = mm2chain.interleave_rounds(made)
        rc = D.real_reads(name)
        assert f_off.size == len(rc) + 1 and L.size == LP.size == sum(m["regs"].size for m in made)
        for rd, c in enumerate(rc):
            g, w = L[f_off[rd]:f_off[rd + 1]].copy(), c["regs"].copy()
            assert g.size == w.size, c["name"]
            gp, wp = g["p"].astype(np.int64), w["p"].astype(np.int64)
            g["p"] = 0; w["p"] = 0
            assert g.tobytes() == w.tobytes() and np.array_equal(gp != 0, wp != 0), c["name"]
            assert LP[gp[gp != 0] - 1].tobytes() == c["pext"][wp[wp != 0] - 1].tobytes(), c["name"]
        if len(made) > 1:
            bad = [dict(m) for m in made]
            bad[0]["child_of"] = bad[0]["child_of"][::-1].copy()
            with pytest.raises(ValueError):
                mm2chain.interleave_rounds(bad)
            bad[0]["child_of"] = made[0]["child_of"][:-1]
            with pytest.raises(ValueError):
                mm2chain.interleave_rounds(bad)
    e = mm2chain.interleave_rounds([])
    assert e[0].tolist() == [0] and e[1].size == 0 and e[2].size == 0
