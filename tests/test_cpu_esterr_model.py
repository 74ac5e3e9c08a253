"""CPU test of tests/esterr_model.py against the reference's own esterr.o (tests/golden/ref_esterr.npz): every byte of the final regions, div included, for every case
of tests/esterr_data.py, with the host's pow; the parallel identity csrc/chain_esterr.hip relies on against the literal loop, on the fixture and on seeded random
inputs; the planted cases are what they claim to be; and each natural wrong variant differs from the reference on the cases planted for it."""
import numpy as np
import pytest

import esterr_data as D
import esterr_model as M


@pytest.fixture(scope="module")
def ref():
    return {R["name"]: R for R in D.reference()}


def _model(R, **variant):
    c = R["case"]
    return M.est_err(R["in"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"], **variant)


def _differ(ref, names, **variant):
    return [n for n in names if _model(ref[n], **variant).tobytes() != ref[n]["out"].tobytes()]


def test_model_reproduces_every_byte_of_the_fixture(ref):
    bad = [n for n, R in ref.items() if _model(R).tobytes() != R["out"].tobytes()]
    only_libm = bad and all(n.startswith(("libm_", "avgk_frac_")) for n in bad)
    assert not bad, f"{len(bad)} case(s) differ: {bad[:8]}" + (f" -- only the libm-sensitive cases: this machine's libm is not the fixture's ({next(iter(ref.values()))['libm']})" if only_libm else "")


def test_parallel_identity_on_the_fixture(ref):
    for n, R in ref.items():
        c = R["case"]
        a, b = (M.counts(R["in"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"], walk=w) for w in ("loop", "parallel"))
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), n


def test_parallel_identity_on_random_inputs():
    """small reads with missing, repeated and decreasing anchor positions, both strands, spans that vary, first anchors that are absent, regions of one anchor, reads
    of one minimizer: the counts by the parallel identity equal the literal loop's"""
    rng = np.random.default_rng(20261021)
    n_cases = n_stop = n_first = 0
    for t in range(3000):
        qlen = int(rng.integers(200, 400))
        n_mini = int(rng.integers(1, 30))
        pos = np.sort(rng.choice(np.arange(20, qlen - 20), n_mini, replace=False))
        mini = np.array([(int(rng.integers(10, 20)) << 32) | int(p) for p in pos], np.uint64)
        regs, chains = [], []
        at = 0
        for _ in range(int(rng.integers(1, 4))):
            cnt, rev = int(rng.integers(1, 9)), int(rng.integers(0, 2))
            kind = int(rng.integers(0, 4))
            start = int(rng.integers(0, n_mini))
            fp = [int(pos[min(start + k, n_mini - 1)]) if kind == 3 else int(pos[(start + k) % n_mini]) if kind == 2 else int(pos[start + k]) if start + k < n_mini else qlen + k
                  for k in range(cnt)]
            for k in range(cnt):                                               # some anchors off the minimizers
                if rng.integers(0, 6) == 0:
                    fp[k] += 1
            spans = rng.integers(10, 20, cnt)
            y = [qlen - 1 - p + int(s) - 1 if rev else p for p, s in zip(fp, spans)]
            order = range(cnt - 1, -1, -1) if rev else range(cnt)
            chains += [((rev << 63) | (1000 + 10 * i), (int(spans[k]) << 32) | (y[k] & 0xffffffff)) for i, k in enumerate(order)]
            g = np.zeros(1, M.REG)
            g["cnt"], g["as"], g["flags"], g["qs"], g["rs"], g["re"] = cnt, at, rev << 10, int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(900, 1100))
            regs.append(g)
            at += cnt
        regs, a = np.concatenate(regs), np.array(chains, np.uint64)
        ref_len = np.array([int(rng.integers(900, 1200))], np.uint32)
        lo, pa = (M.counts(regs, a, mini, qlen, ref_len, walk=w) for w in ("loop", "parallel"))
        assert np.array_equal(lo[0], pa[0]), f"input {t}: loop {lo[0].tolist()}, parallel {pa[0].tolist()}"
        n_cases += regs.size
        n_stop += int(((lo[0][:, 0] > 0) & (lo[0][:, 0] < regs["cnt"])).sum())
        n_first += int((lo[0][:, 0] == 0).sum())
    assert n_cases > 4000 and n_stop > 500 and n_first > 100, (n_cases, n_stop, n_first)


def test_planted_cases_are_what_they_claim(ref):
    d = lambda n: ref[n]["out"]["div"].tolist()
    cn = lambda n: M.counts(ref[n]["in"], ref[n]["a"], ref[n]["case"]["mini_pos"], ref[n]["case"]["qlen"], ref[n]["case"]["ref_len"])[0].tolist()
    assert d("no_mini") == [-1.0] and cn("no_mini") == [[-1, 0]] and ref["no_regions"]["out"].size == 0        # mm_gen_regs leaves -1 (hit.c:83), esterr.c:36 returns
    assert d("first_absent") == [-1.0] and d("one_mini_absent") == [-1.0] and cn("first_absent") == [[0, 0]]
    assert d("all_matched_no_flanks") == [0.0] and cn("all_matched_no_flanks") == [[5, 5]]
    assert cn("all_matched_extras_between") == [[6, 12]] and cn("middle_absent") == [[3, 5]] and cn("j_reaches_n") == [[2, 4]]
    assert cn("repeated_position") == [[2, 4]] and cn("decreasing_position") == [[2, 5]] and cn("reverse_middle_absent") == [[2, 4]]
    assert ref["first_at_n_minus_1_cnt1"]["case"]["mini_pos"].size == 3 and cn("first_at_n_minus_1_cnt1") == [[1, 3]]
    for w in ("qs", "rs", "qtail", "rtail"):                                    # at avg_k and one below: not counted; one above: counted
        assert cn(f"flank_{w}_14")[0][1] == cn(f"flank_{w}_15")[0][1] == cn(f"flank_{w}_16")[0][1] - 1, w
    assert cn("avg_15_333_qs15") == [[1, 1]] and cn("avg_15_333_qs16") == [[1, 2]] and cn("avg_15_5_qs15") == [[1, 1]] and cn("avg_15_5_qs16") == [[1, 2]]
    assert ref["joined"]["out"].size == 1 and ref["joined"]["out"]["cnt"][0] == 10 and ref["joined"]["case"]["a"].shape[0] == 14 and ref["joined"]["a"].shape[0] == 10
    assert ref["unsqueezed_as_nonzero"]["out"]["as"].tolist() == [4] and ref["regions128"]["out"].size == 128 and ref["regions129"]["out"].size == 129
    assert ref["minis64"]["case"]["mini_pos"].size == 64 and ref["minis65"]["case"]["mini_pos"].size == 65
    for n in (D.SLICE - 1, D.SLICE, D.SLICE + 1):
        r = ref[f"slice_cnt{n}"]["out"]
        assert sorted(zip(r["as"].tolist(), r["cnt"].tolist())) == [(0, D.LEAD), (D.LEAD, n)]
        assert sorted(v[0] for v in cn(f"slice_missing_at{n}")) == [D.LEAD, n - D.LEAD]       # the walk stops at position n of the read's a[]
    assert cn("wave_missing_63_64_65") == [[63, 65]] and cn("wave_missing_64_130") == [[64, 66]]          # a[] positions 63-65 / 64 and 130: waves 0, 1 and 2
    assert cn("wave_missing_130_64_rev")[0][0] == 199 - 130                                                # the walk from the back stops at a[] position 130
    assert sorted(v[0] for v in cn("slice_missing_at_rev")) == [D.LEAD, D.SLICE + 200 - 1 - (D.SLICE - D.LEAD)]
    two = ref["two_rids"]["out"]
    assert sorted(two["rid"].tolist()) == [0, 1] and len(set(two["div"].tolist())) == 2
    assert all(0 < ref[f"libm_{n}"]["out"]["div"][0] < 1e-3 for n in (500, 1000, 2047, 3001))


@pytest.mark.parametrize("variant,planted", [
    (dict(flank="qe"), ["qs_not_qe"]),
    (dict(strand="region"), ["anchor_strand_differs", "anchor_strand_differs_rev"]),
    (dict(avg="int"), ["avg_15_5_qs16", "avg_15_333_qs16"]),
    (dict(cmp="ge"), ["flank_qs_15", "flank_rs_15", "flank_qtail_15", "flank_rtail_15", "avg_int_all15_qs15"]),
    (dict(prefix="skip"), ["middle_absent", "second_absent", "reverse_middle_absent", "slice_missing_at4096"]),
    (dict(en="last"), ["middle_absent", "j_reaches_n", "repeated_position"]),
])
def test_wrong_variants_differ_on_their_planted_cases(ref, variant, planted):
    got = _differ(ref, planted, **variant)
    assert got == planted, f"{variant}: differs only on {got} of {planted}"


def test_avg_k_in_double_differs_somewhere_on_its_planted_family(ref):
    """on these cases (double)sum_k / n changes no flank compare: with a few minimizers no integer lies between the float quotient and the double one (with some
    10^6 minimizers the float quotient can round up to an integer, which no case here reaches).  So it shows only through pow, in the last bit of some results and
    not of others: the family avgk_frac_* and the fractional flank cases are planted for it, and at least one of them tells"""
    fam = [n for n in ref if n.startswith("avgk_frac_")] + ["avg_15_333_qs16", "qs_not_qe"]
    got = _differ(ref, fam, avg="double")
    print("avg_k in double differs on", got)
    assert got, "no planted case tells avg_k in double from avg_k in float"
    assert not _differ(ref, [n for n in ref if n.startswith("flank_")], avg="double")


def test_reverse_conversion_depends_on_the_span(ref):
    """spans 15 and 19 in one reverse read: with one span for all the anchors' forward positions move and the walk stops"""
    R = ref["reverse_spans_15_19"]
    a = R["a"].copy()
    a[:, 1] = (a[:, 1] & np.uint64(0xffffffff)) | (np.uint64(15) << np.uint64(32))
    c = R["case"]
    assert M.est_err(R["in"], a, c["mini_pos"], c["qlen"], c["ref_len"]).tobytes() != R["out"].tobytes()
