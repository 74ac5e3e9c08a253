"""tests/seed_limit_data.py does what it says: asserted from the oracle alone (collect_seed_hits, radix_sort_128x), without a GPU.  These are conditions on the inputs of
tests/test_gpu_seed_limits.py -- a limit input that does not reach its limit tests nothing, and a tie test that a plain stable sort would pass tests nothing either.

The size classes, RUN_MAX and the key-width thresholds below are written out here from the issue's table, not read from the kernel source."""
import numpy as np
import pytest

import oracle_binding as ob
import seed_limit_data as sd

U = np.uint64


def _rows(a):
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def check_case(case):
    """counts, the encoding, runs, widths and the sensitivity of one case; returns (reference list, stable list)"""
    qlen, m, h = case["read"]
    ref = sd.reference(case)
    fill = sd.fill_anchors(case["read"], for_only=case.get("flag", 0) == ob.F_FOR_ONLY)
    assert ref.shape[0] == case["na"] == fill.shape[0], (case["name"], ref.shape[0], case["na"], fill.shape[0])
    assert int(m["n"].sum()) == case.get("cap", case["na"]) and m.size == int((m["n"] >= 0).sum())
    # the reference's list is radix_sort_128x of the list in fill order (map.c:245), and the same anchors
    if not case.get("heap"):
        assert np.array_equal(ob.radix_sort_128x(fill), ref), case["name"]
    assert np.array_equal(_rows(fill), _rows(ref)), case["name"]
    stable = fill[np.argsort(fill[:, 0], kind="stable")]
    x = ref[:, 0]
    assert np.array_equal(x, stable[:, 0]) and np.all(x[1:] >= x[:-1])
    runs = sd.runs_of(x)
    for s, n in runs:                                                             # equal x never share y: every order among them is visible
        assert np.unique(ref[s:s + n, 1]).size == n, (case["name"], s)
    if case["runs"] is not None:
        assert runs == case["runs"], (case["name"], runs[:4], case["runs"][:4])
    kb, idb = sd.widths(x)
    if case["kb"] is not None:
        assert kb == case["kb"], (case["name"], kb)
    if case["idb"] is not None:
        assert idb == case["idb"], (case["name"], idb)
    moved = (ref != stable).any(axis=1)
    if case["reorder"] is None:
        assert not moved.any(), f"{case['name']}: the reference should leave the stable order"
    else:
        assert moved.any(), f"{case['name']}: a stable sort would pass"
        for L in case["reorder"]:
            hit = [s for s, n in runs if n == L and moved[s:s + n].any()]
            assert hit, f"{case['name']}: no run of {L} is reordered by the reference"
    return ref, stable


def test_runs_of_223_start_at_every_residue_and_at_both_ends():
    """the L = 223 set: six reads of at most 5 120 anchors (one read of that class holds 13 runs of 223, the 64 residues need 64 run starts), each with a run at position 0
    and a run that ends at position na - 1; gaps between 1 and 64; the run starts together cover every residue modulo 64, hence every lane and every window step"""
    cases = sd.set_a_223()
    residues, gaps = set(), set()
    for c in cases:
        check_case(c)
        assert 2560 < c["na"] <= 5120 and all(n == 223 for _, n in c["runs"])
        starts = [s for s, _ in c["runs"]]
        assert starts[0] == 0 and starts[-1] + 223 == c["na"]
        residues |= {s % 64 for s in starts}
        gaps |= {b - a - 223 for a, b in zip(starts[:-1], starts[1:])}
        assert any(s // 512 != (s + 222) // 512 for s in starts), "a run straddles a multiple of 512"
    assert residues == set(range(64)) and min(gaps) >= 1 and max(gaps) <= 64, (sorted(residues), sorted(gaps))


@pytest.mark.parametrize("which", ["lengths", "long"])
def test_runs_of_every_named_length(which):
    cases = sd.set_a_lengths() if which == "lengths" else sd.set_a_long()
    lengths = set()
    for c in cases:
        check_case(c)
        got = {n for _, n in c["runs"]}
        assert got == set(c["reorder"]) and len(c["runs"]) >= 2
        gaps = [b[0] - a[0] - a[1] for a, b in zip(c["runs"][:-1], c["runs"][1:])]
        assert min(gaps) >= 1 and max(gaps) <= 64 and c["runs"][0][0] >= 1 and c["runs"][-1][0] + c["runs"][-1][1] < c["na"]
        lengths |= got
        if which == "lengths":
            assert 64 < c["na"] <= 5120, c["na"]
        else:
            lo, hi = (5120, 12288) if c["name"].endswith("-9k") else (16384, 65536)
            assert lo < c["na"] <= hi, (c["name"], c["na"])
    assert lengths == ({222, 223, 224, 225, 447, 1000} if which == "lengths" else {223, 224})


def test_reads_of_one_x_stay_in_fill_order():
    """kb = 0: every pass of the reference sees one occupied digit and moves nothing (ksort.h:117-131), so the list is the fill order -- the reference cannot
    reorder these reads and a stable sort gives the same list"""
    cases = sd.set_a_one_x()
    assert [c["na"] for c in cases] == [65, 300, 5121, 20000]
    for c in cases:
        ref, _ = check_case(c)
        assert sd.widths(ref[:, 0])[0] == 0 and c["runs"] == [(0, c["na"])]
        assert np.array_equal(ref, sd.fill_anchors(c["read"]))


def test_size_class_batches_hold_n_and_n_plus_1_at_every_boundary():
    """64 anchors or fewer are sorted by insertion (ksort.h:149, stable): for the 64-anchor read the two orders must be equal; every other read is reordered"""
    one, two = sd.set_b_batches()
    sizes = sorted(c["na"] for c in one + two if not c["name"].startswith("B-short"))
    assert sizes == sorted([n for b in sd.BOUNDS for n in (b, b + 1)])
    assert sd.BOUNDS == (64, 2560, 5120, 12288, 16384, 65536, 131072)
    for batch in (one, two):
        order = [c["na"] for c in batch]
        assert order != sorted(order) and order != sorted(order, reverse=True)
        assert sum(c["name"].startswith("B-short") for c in batch) == 3
        for c in batch:
            check_case(c)
            assert len(c["runs"]) > c["na"] // 20


def test_capacity_and_count_fall_into_different_classes():
    for cap, kept in sd.SKIP_CASES:
        c = sd.skip_case(cap, kept)
        ref, _ = check_case(c)
        assert int(c["read"][1]["n"].sum()) == cap and ref.shape[0] == kept and not (ref[:, 0] >> U(63)).any()
        assert sd.reference(dict(c, name=c["name"] + "-all", flag=0)).shape[0] == cap
    assert sd.SKIP_CASES == ((16385, 64), (16385, 65), (16385, 2561), (16385, 5121), (131073, 12289))


def test_heap_reads_have_the_match_counts_around_the_heap_capacity():
    for nm in (2047, 2048, 2049):
        c = sd.heap_case(nm)
        qlen, m, h = c["read"]
        assert m.size == nm and (m["n"] > 0).all()
        assert all(np.all(np.diff(h[o:o + n].astype(np.int64)) >= 0) for o, n in zip(m["cr_off"], m["n"]))
        heap, radix = sd.reference(c), ob.collect_seed_hits(m, h, qlen)
        assert heap.shape[0] == c["na"] and np.array_equal(heap[:, 0], radix[:, 0]) and (heap != radix).any(), "the heap order differs from the radix sort's"


def test_key_widths():
    cases = sd.set_c_kb()
    assert [c["kb"] for c in cases] == [1, 8, 9, 16, 17, 24, 25, 31, 32, 33, 32, 33]
    assert [c["na"] for c in cases] == [3000] * 10 + [16384] * 2
    for c in cases:
        ref, _ = check_case(c)
        diff = int(np.bitwise_or.reduce(ref[:, 0]) ^ np.bitwise_and.reduce(ref[:, 0]))
        b0, b1 = (diff & 0xffffffff).bit_length(), ((diff >> 32) & 0x7fffffff).bit_length()
        assert diff & 0xffffffff == (1 << b0) - 1 and (diff >> 32) & 0x7fffffff == (1 << b1) - 1, "exactly the wanted bits differ"


def test_key_and_index_widths_add_up_to_64_and_65():
    cases = sd.set_c_sum()
    assert [(c["kb"] + c["idb"], c["idb"]) for c in cases] == [(64, 11), (65, 11), (65, 11), (64, 15), (65, 15), (65, 15), (64, 11), (65, 12)]
    assert [c["na"] for c in cases[-2:]] == [2048, 2049] and all(16384 < c["na"] <= 32768 for c in cases[3:6])
    for c in cases:
        check_case(c)
        longest = max(n for _, n in c["runs"])
        assert longest == 224 if c["name"].endswith("run224") else longest < 224, (c["name"], longest)


def test_bucket_structure():
    cases = {c["name"]: c for c in sd.set_d()}
    assert len(cases) == 10
    for c in cases.values():
        assert 300 <= c["na"] <= 4000, (c["name"], c["na"])
        ref, _ = check_case(c)
        tree = sd.bucket_tree(ref[:, 0])
        assert all(hi - lo > 64 for _, lo, hi, _ in tree)
        shift, digits = sd.first_split(tree)
        assert shift == c["top"][0] and (c["top"][1] is None or digits == c["top"][1]), (c["name"], shift, digits)
        for sh, want in c.get("nodes", []):
            found = [dg for s, _, _, dg in tree if s == sh and set(dg) == set(want) and all(v is None or dg[k] == v for k, v in want.items())]
            assert found, (c["name"], sh, want)
    fill_x = lambda name: sd.fill_anchors(cases[name]["read"])[:, 0]
    for tag in ("two", "three"):
        # misplaced records of the top pass, counted on the fill order: position < the lower side's size and digit of the upper side, and the other way round
        for kind, want in (("single", 1), ("none", 0), ("all", 300)):
            x = fill_x(f"D-{tag}-{kind}")
            n_low = int(((x >> U(56)) == 0).sum())
            assert int(((x[:n_low] >> U(56)) == 0x80).sum()) == want, (tag, kind)
        assert len(sd.first_split(sd.bucket_tree(np.sort(fill_x(f"D-{tag}-all"))))[1]) == (2 if tag == "two" else 3)
    # sub-buckets of 64 and 65: both hold equal keys, only the one of 65 (and the one of 150) gets another pass
    ref = sd.reference(cases["D-sub-64-65"])
    assert sd.runs_of(ref[:64, 0]) and sd.runs_of(ref[64:129, 0])
    assert sorted(hi - lo for s, lo, hi, _ in sd.bucket_tree(ref[:, 0]) if s == 48) == [65, 150]
    # lowest byte only: every digit of the one pass that moves anything is occupied here or there, the keys agree above
    x = sd.reference(cases["D-low-byte"])[:, 0]
    assert int(np.bitwise_or.reduce(x) ^ np.bitwise_and.reduce(x)) < 256 and len(sd.first_split(sd.bucket_tree(x))[1]) > 200
    # D-deep: the only equal keys are the 65 of the lowest level
    c = cases["D-deep"]
    assert c["na"] == 65 + 7 * 40
    main = np.nonzero(sd.reference(c)[:, 0] >> U(8) == U(0x01010101010101))[0]
    assert main.size == 65 and all(main[0] <= s and s + n <= main[-1] + 1 for s, n in c["runs"]) and c["runs"]


def test_encoding_batch():
    """set E cannot be reordered on purpose or not: what is asserted is the encoding (the NumPy restatement of map.c:222-243 against the oracle, in check_case) and that
    the batch holds what it names"""
    cases = sd.set_e()
    for c in cases:
        qlen, m, h = c["read"]
        ref = sd.reference(c)
        fill = sd.fill_anchors(c["read"])
        assert ref.shape[0] == c["na"] and np.array_equal(ob.radix_sort_128x(fill), ref)
    qlen, m, h = cases[0]["read"]
    assert qlen == 2**31 - 1 and set(m["q_span"]) == set(range(1, 256))
    assert {(int(s) >> 1, int(s) & 1) for s in m["seg_tandem"]} == {(s, t) for s in (0, 1, 127, 255) for t in (0, 1)}
    start = (m["q_pos"] >> 1).astype(np.int64) + 1 - m["q_span"]
    for strand in (0, 1):
        assert ((start == 0) & (m["q_pos"] & 1 == strand)).any() and ((m["q_pos"] >> 1 == qlen - 1) & (m["q_pos"] & 1 == strand)).any()
    y = sd.reference(cases[0])[:, 1] & U(0xffffffff)
    assert y.min() == 0 and y.max() == qlen - 1, "forward and reverse-strand query positions reach both ends"
    assert [c["read"][0] for c in cases[1:3]] == [1, 15] and cases[3]["na"] == 1


def test_tandem_tasks_give_the_named_chain_counts():
    from mm2chain import params
    P = params.map_ont()
    for n in sd.TANDEM_CHAINS:
        t = sd.tandem_task(n, 9700 + n)
        u, b = ob.mm_chain_dp(P, 3, 40, t)
        assert u.size == n and b.shape[0] == 4 * n, (n, u.size)
        first = b[np.concatenate(([0], np.cumsum(u & U(0xffffffff))[:-1])).astype(np.int64), 0]
        assert np.unique(first).size < first.size, "chains start at equal x"
    assert sd.TANDEM_CHAINS == (64, 65, 768, 769)
