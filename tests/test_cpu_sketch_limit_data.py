"""tests/sketch_limit_data.py does what it says: asserted from the models alone (sketch_model, index_model), without a GPU.  These are conditions on the inputs of
tests/test_gpu_sketch_limits.py -- a limit input that does not reach its limit tests nothing.  Every case of the data module is checked: none is skipped or filtered.

The boundary numbers below are written out, not derived from the data module's constants; the constants themselves are compared with the kernel source once.  The
models are pinned to the reference at these very inputs by tests/golden/ref_sketch_limits.npz (make_ref_sketch_limit_fixtures.py).  Every deliberate error of the
data module's restatement is caught by the cases named for it."""
import os
import re

import numpy as np
import pytest

import index_model as im
import sketch_limit_data as sd
import sketch_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "minimap2-fpga_amd", "csrc")
FIX = os.path.join(HERE, "golden", "ref_sketch_limits.npz")
SETTINGS = [(15, 10, 0), (16, 10, 0), (28, 255, 0), (19, 5, 1), (5, 3, 1), (15, 1, 0)]
IDS = ["k%d-w%d-hpc%d" % S for S in SETTINGS]


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


def facts(S, name):
    return sd.by_name(S, name)["facts"]


def test_constants_mirror_the_kernel_source():
    sk = open(os.path.join(CSRC, "sketch.hip")).read()
    host = open(os.path.join(CSRC, "mm2chain_sketch.cpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, sk).group(1))
    assert sd.CH == const("CH") == 64 and sd.SC == const("SC") == 256
    assert sd.SPAN_CUT == 256 and "q >= 0 && span < 256" in sk and "if (span < 256)" in sk
    assert sd.ROUND == 64 and "base += 64" in sk and "/ 64;" in sk
    assert "y_bits = 32 + std::max(bits_for((uint64_t)(n_seqs - 1)), 1)" in host
    assert [sd.y_bits(n) for n in (1, 2, 3, 4, 5, 8, 9, 256, 257, 65536, 65537)] == [33, 33, 34, 34, 35, 35, 36, 40, 41, 48, 49]
    assert "(1. - (double)frac) * (double)ix->n" in host and "(int64_t)(uint32_t)v" in host
    assert "if (b.cnt >= k)" in sk and "b.reset ? b.l" in sk and "if (mx >= x)" in sk and "if (s2 > rep_en)" in sk and "t < A.mid_occ" in sk
    assert sd.SETTINGS == SETTINGS


def test_batches_stay_within_their_caps():
    sizes = {S: sum(len(r) for r in sd.batch(S)[0]) for S in SETTINGS}
    print(sizes)
    for S, n in sizes.items():
        assert n <= 400_000, f"{S}: {n} bases"
        reads, where = sd.batch(S)
        assert sorted(where.values()) == sorted((a, b) for a, b in where.values()) and max(b for _, b in where.values()) == len(reads)
        assert len({c["name"] for c in sd.cases(S)}) == len(sd.cases(S))
    assert sizes[(28, 255, 0)] >= 350_000, "the w = 255 sweep is the largest batch"


# ---- every case reaches the limit it names -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SETTINGS, ids=IDS)
def test_registers_across_lanes(S):
    k, w, hpc = S
    names = [c["name"] for c in sd.cases(S) if c["family"] == "registers"]
    if not hpc:
        want = [f"n_run_{run}_at_{off}" for run in (1, 63, 64, 65, 128, 200) for off in (0, 1, 62, 63)]
        assert names[:24] == want
        for name in want:
            c = sd.by_name(S, name)
            r = c["reads"][0]
            at = r.index(b"N")
            run = len(r) - len(r[at:].lstrip(b"N")) - at
            assert (run, at % 64) == (int(name.split("_")[2]), int(name.split("_")[4])) == (c["facts"]["run"], c["facts"]["in_lane"]), name
            assert len(r) - at - run >= w + k, "minimizers behind the run"
        if k == 28:
            perms = [(27, 28, 29), (27, 29, 28), (28, 27, 29), (28, 29, 27), (29, 27, 28), (29, 28, 27)]
            assert names[24:] == ["push_%d_%d_%d" % p for p in perms]
            for p in perms:
                c = sd.by_name(S, "push_%d_%d_%d" % p)
                assert tuple(c["facts"]["pushes"]) == p == tuple(sd.lane_pushes(c["reads"][0], 0)[2:5])
        else:
            assert len(names) == 24
    else:
        assert names == ["hp_run_64", "hp_run_65", "hp_run_128", "hp_run_129"]
        for name, silent in zip(names, (0, 1, 1, 2)):
            c = sd.by_name(S, name)
            r = c["reads"][0]
            assert r.index(b"A" * c["facts"]["run"]) == 128 and r[127:128] != b"A" and r[128 + c["facts"]["run"]:][:1] != b"A"
            assert c["facts"]["silent_lanes"] == silent == sum(1 for n in sd.lane_pushes(r, 1) if n == 0), name


@pytest.mark.parametrize("S", [(16, 10, 0), (28, 255, 0)], ids=["k16-w10", "k28-w255"])
def test_palindromes_across_an_ambiguous_run(S):
    k, w, hpc = S
    for m in (1, 64, 70, 130):
        a, c = sd.by_name(S, f"palindrome_across_{m}"), sd.by_name(S, f"palindrome_control_{m}")
        ra, rc = a["reads"][0], c["reads"][0]
        at = ra.index(b"N")
        assert ra.count(b"N") == m and ra[at:at + m] == b"N" * m and at == 100 + k // 2
        h = ra[at - k // 2:at]
        assert ra[at + m:at + m + k // 2] == sd.revcomp(h), "the two halves of a symmetric k-mer on either side of the run"
        assert sum(x != y for x, y in zip(ra, rc)) == 1 and ra[at - k // 2] != rc[at - k // 2], "the control differs in one base of h"
        tail = ra[at + m:]
        assert sd.tail_differs(ra, tail, S) is True is a["facts"]["tail_differs"], f"m = {m}: the tail's sketch is that of the tail alone"
        assert sd.tail_differs(rc, tail, S) is False is c["facts"]["tail_differs"], f"m = {m}: the control's tail differs too"
    assert not [c for S2 in SETTINGS if S2[0] % 2 for c in sd.cases(S2) if c["family"] == "palindrome"]


@pytest.mark.parametrize("S", SETTINGS, ids=IDS)
def test_l_reaches_its_three_values_on_lane_edges(S):
    k, w, hpc = S
    values = [("k", k), ("wk1", w + k - 1), ("wk", w + k)]
    if w == 1:
        values.pop(1)                                                      # w + k - 1 == k
    names = [c["name"] for c in sd.cases(S) if c["family"] == "l_edges"]
    assert names == [f"l_{n}_at_{e}" for n, _ in values for e in (63, 0)]
    for n, v in values:
        for e in (63, 0):
            c = sd.by_name(S, f"l_{n}_at_{e}")
            r = c["reads"][0]
            at = r.index(b"N")
            _, _, L, P = sd.slots(r, *S)
            first = next(p for l, p in zip(L, P) if p > at and l == v)
            assert first % 64 == e == c["facts"]["in_lane"] and c["facts"]["l"] == v, c["name"]
            assert r.count(b"N") == 1
    # the selection: the slot with l == w + k - 1 at a lane's last, first and second slot
    slots_at = {(28, 255, 0): (511, 512, 513)}.get(S, (255, 256, 257))
    fw = [c for c in sd.cases(S) if c["family"] == "first_window"]
    assert [c["name"] for c in fw] == [f"first_window_at_{s}" for s in slots_at]
    for c, s in zip(fw, slots_at):
        _, _, L, P = sd.slots(c["reads"][0], *S)
        at = c["reads"][0].index(b"N")
        assert c["facts"]["slot"] == s and L[s] == w + k - 1 and L[s - 1] == w + k - 2 and P[s] > at, c["name"]
        assert (c["facts"]["window_ties"] >= 1) == (w > 1), f"{c['name']}: the first window holds its smallest x more than once"


@pytest.mark.parametrize("S", SETTINGS, ids=IDS)
def test_slots_lag_positions(S):
    k, w, hpc = S
    lag = {c["name"]: c for c in sd.cases(S) if c["family"] == "lag"}
    counts = {(15, 10, 0): (255, 256, 257, 512, 65535, 65536, 65537), (19, 5, 1): (255, 256, 257, 512, 65536)}.get(S, (255, 256, 257, 512))
    want = ([] if k % 2 or hpc else ["lag_at_only", "lag_at_flanked"]) + (["lag_two_runs"] if hpc else []) + [f"slots_{n}" for n in counts] + ["all_n_256"]
    assert list(lag) == want
    for n in counts:
        c = lag[f"slots_{n}"]
        r = c["reads"][0]
        assert c["facts"]["n_slots"] == n == len(sd.slots(r, *S)[0]) and b"N" not in r
        assert (len(r) == n) if not hpc else (len(r) > n * 5 // 4), "under HPC the bases outnumber the slots"
    assert lag["all_n_256"]["reads"] == [b"N" * 256] and lag["all_n_256"]["facts"] == {"n_slots": 256, "minimizers": 0}
    if k % 2 == 0:
        # an alternating run has no slot once the registers are full: k - 1 slots, whatever its length
        assert lag["lag_at_only"]["reads"] == [b"AT" * 700] and lag["lag_at_only"]["facts"] == {"n_slots": k - 1, "bases": 1400, "empty_tail_lanes": 5}
        f = lag["lag_at_flanked"]["facts"]
        assert f["n_slots"] == {16: 213, 28: 226}[k] and f["empty_tail_lanes"] == 5 and len(sd.slots(lag["lag_at_flanked"]["reads"][0], *S)[0]) == f["n_slots"]
    if hpc:
        assert lag["lag_two_runs"]["facts"] == {"n_slots": 122, "bases": 1120, "empty_tail_lanes": 4}
        assert len(sd.slots(lag["lag_two_runs"]["reads"][0], *S)[0]) == 122
    for c in lag.values():
        if "empty_tail_lanes" in c["facts"]:
            assert c["facts"]["empty_tail_lanes"] >= 1


TIES = {  # setting -> {period: (reads, reads with an equal-x pair on both sides of a multiple of 256 slots)}
    (15, 10, 0): {7: (31, 31), 2: (31, 12)}, (16, 10, 0): {7: (31, 31)}, (28, 255, 0): {3: (256, 26), 100: (16, 16)},
    (19, 5, 1): {2: (31, 8)}, (5, 3, 1): {2: (31, 31)}, (15, 1, 0): {}}


@pytest.mark.parametrize("S", SETTINGS, ids=IDS)
def test_ties_on_a_selection_lane_boundary(S):
    k, w, hpc = S
    ties = [c for c in sd.cases(S) if c["family"] == "ties"]
    seen = {}
    for c in ties:
        p, o = (int(v[1:]) for v in c["name"].split("_")[1:])
        r = c["reads"][0]
        assert b"N" not in r and c["facts"]["start"] == 230 + o
        unit = r[230 + o:230 + o + p]
        reps = 30 if p == 100 else 40
        assert r[230 + o:230 + o + p * reps] == unit * reps and p < w and len(r) == 230 + o + p * reps + 60, c["name"]
        n, yes = seen.get(p, (0, 0))
        seen[p] = (n + 1, yes + (sd.straddles(sd.sk(S, r), sd.slots(r, *S)[3]) > 0))
        assert (c["facts"]["straddles"] > 0) == (sd.straddles(sd.sk(S, r), sd.slots(r, *S)[3]) > 0)
    assert seen == TIES[S], seen
    for p, (n, _) in seen.items():
        assert n == (len(range(0, 256, 16)) if p == 100 else max(w, 30) + 1), "one read per offset 0 ... max(w, 30) (every 16th for the period of 100)"


@pytest.mark.parametrize("S", [(19, 5, 1), (5, 3, 1)], ids=["k19-w5", "k5-w3"])
def test_hpc_span_at_255_256_257(S):
    k, w, hpc = S
    span = [c for c in sd.cases(S) if c["family"] == "span"]
    assert [c["name"] for c in span] == [f"span_{T}_at_{o}" for T in (255, 256, 257) for o in (0, 1, 63)] + ["span_255_n_before_run", "span_255_n_cuts_walk"]
    for c in span[:9]:
        T, o = c["facts"]["T"], c["facts"]["in_lane"]
        r = c["reads"][0]
        at = r.index(b"A" * (T - k + 1))
        assert at % 64 == o and at >= 128 and r[at - 1:at] != b"A"
        behind = r[at + T - k + 1:at + T]
        assert len(behind) == k - 1 and b"A" != behind[:1] and all(behind[i] != behind[i + 1] for i in range(k - 2)), "k - 1 runs of one base"
        # the k steps whose last k runs hold the long run all have span T: a minimizer among them (k >= w) only when T fits 8 bits
        assert (set(c["facts"]["spans"]) == {255}) if T == 255 else (c["facts"]["spans"] == []), c["name"]
        every = [int(x) & 0xFF for x, _ in sd.sk(S, r)]
        assert (255 in every) == (T == 255) and max(every) <= 255
    assert span[9]["facts"]["spans"] == ([255] if k == 19 else []) and span[9]["reads"][0].count(b"N") == 1
    assert set(span[10]["facts"]["spans"]) == {255} and span[10]["reads"][0].count(b"N") == 1


@pytest.mark.parametrize("S", SETTINGS, ids=IDS)
def test_read_boundaries_and_the_long_read(S):
    k, w, hpc = S
    c = sd.by_name(S, "boundary_reads")
    lens = [len(r) for r in c["reads"]]
    allowed = {0, 1, k - 1, k, w + k - 2, w + k - 1, w + k, 63, 64, 65, 127, 128, 129, 255, 256, 257}
    assert len(lens) == 600 and lens[:3] == [0, 0, 0] == lens[-3:] and lens[255:258] == [300, 300, 300]
    assert set(lens) - {300} == allowed and c["facts"]["lengths"] == len(allowed)
    assert c["facts"]["empty"] == lens.count(0) >= 30
    assert c["facts"]["without_minimizers"] == sum(1 for r in c["reads"] if not sd.sk(S, r)) > c["facts"]["empty"]
    first, last = sd.batch(S)[1]["boundary_reads"]
    assert last - first == 600
    lr = sd.by_name(S, "long_read")
    assert lr["facts"]["bases"] == len(lr["reads"][0]) >= 70_000 and lr["facts"]["n_slots"] >= 65_536 + 4 * 256, lr["facts"]
    assert lr["facts"]["parts"] >= 100, "made of the cases above"


def test_every_case_belongs_to_a_checked_family():
    for S in SETTINGS:
        assert {c["family"] for c in sd.cases(S)} <= {"registers", "palindrome", "l_edges", "first_window", "lag", "ties", "span", "boundary", "long"}
        for c in sd.cases(S):
            assert c["kwh"] == S and c["reads"] and all(isinstance(r, bytes) for r in c["reads"])


# ---- lookups ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_lookup_cases_reach_their_limits():
    names = [c["name"] for c in sd.lookup_cases()]
    assert names == ["tandem_edges", "tandem_unfiltered", "mid_occ_1", "mid_occ_2", "mid_occ_50", "mid_occ_0", "mid_occ_2147483647", "rep_len_rounds"]
    c = sd.lookup_by_name("tandem_edges")
    r = c["reads"]
    assert r[0] == r[1] == r[3] and r[2] == r[0][:len(r[0]) // 2] and r[0][:24] == r[0][-24:]
    keys = [[int(x) >> 8 for x, _ in sm.sketch(s, 10, 15)] for s in r]
    assert keys[0][-1] == keys[1][0] and keys[0][0] != keys[0][1], "the last minimizer of a read and the first of the next share their key"
    res = sd.lookup_model(c)
    assert res[0][0][-1][4] & 1 == 0 and res[1][0][0][4] & 1 == 0 and c["facts"]["edge_pairs"] == 2
    assert c["facts"]["edge_tandems"] == [1, 1], "a read that ends in, and one that begins with, a tandem repeat"
    assert c["facts"]["minimizers_of_short"] == [1, 1] and [len(k_) for k_ in keys[6:]] == [1, 1]
    assert len(r[0]) + len(r[1]) == c["facts"]["group_cut"] == 696
    u = sd.lookup_by_name("tandem_unfiltered")
    assert u["facts"]["kept_neighbours_equal"] == 17 and u["facts"]["their_tandem"] == [0] and u["facts"]["repetitive"] == 18
    for mid_occ in (1, 2, 50):
        f = sd.lookup_by_name(f"mid_occ_{mid_occ}")["facts"]
        assert (f["at_mid_occ"], f["one_below"], f["kept"], f["minimizers"]) == (155, 332, 332, 487) and f["rep_len"] == 1664
    c = sd.lookup_by_name(f"mid_occ_{mid_occ}")
    look = sm.table_lookup(*c["table"][:3])
    ts = [look(int(x) >> 8)[1] for s in c["reads"] for x, _ in sm.sketch(s, 10, 15)]
    assert sorted(set(ts)) == [49, 50] and ts.count(50) == 155
    f = sd.lookup_by_name("mid_occ_0")["facts"]
    assert (f["kept"], f["minimizers"], f["rep_len"]) == (0, 487, 2743), "mid_occ = 0: absent keys are repetitive too"
    f = sd.lookup_by_name("mid_occ_2147483647")["facts"]
    assert (f["kept"], f["minimizers"], f["rep_len"]) == (487, 487, 0)
    for c in sd.lookup_cases():
        assert int(c["table"][2].max()) < 2**31 and c["table"][3].size >= int(c["table"][1][-1]) + int(c["table"][2][-1])
    f = sd.lookup_by_name("rep_len_rounds")["facts"]
    kinds = [(kind, j) for j in (63, 64, 65, 128) for kind in ("touch", "overlap", "apart")] + [("all", n) for n in (63, 64, 65, 129)] + [("none", 0)]
    assert f["design"] == kinds and all(f["as_designed"])
    assert f["gap"] == [0, -14, 1] * 4 + [-14] * 4 + [None], "st - rep_en at the later minimizer: touching, overlapping, one apart"
    assert f["minimizers"][12:] == [63, 64, 65, 129, 136]
    assert f["rep_len"] == [30, 16, 30] * 4 + [77, 78, 79, 143, 0]


# ---- index build --------------------------------------------------------------------------------------------------------------------------------------------------
def test_sequence_lists_reach_their_limits():
    assert sd.N_SEQS == (1, 2, 3, 4, 5, 8, 9, 256, 257, 65536, 65537)
    planted = {1: [0], 2: [0, 1], 3: [0, 1, 2], 4: [0, 1, 2, 3], 5: [0, 3, 4], 8: [0, 3, 4, 7], 9: [0, 7, 8], 256: [0, 127, 128, 255], 257: [0, 255, 256],
               65536: [0, 32767, 32768, 65535], 65537: [0, 65535, 65536]}
    for n in sd.N_SEQS:
        seqs, at = sd.seq_list(n)
        f = sd.list_facts(n)
        assert len(seqs) == n and list(at) == planted[n] == f["planted_in"]
        assert all(sd.plant((15, 10, 0)) in seqs[i] for i in at)
        assert f["spanning_keys"] == f["ascending"] == 6, f"{n}: keys whose hits run from sequence 0 to sequence {n - 1}, ascending in rid"
        assert f["with_minimizers"] == min(n, 40) - (1 if n in (257, 65537) else 0) and sum(1 for s in seqs if len(s) >= 15) == f["with_minimizers"]
        if n > 300:
            assert sum(1 for s in seqs if not s) >= n - 250
    lens = [len(s) for s in sd.seq_list(65537)[0]]
    found = {name: sd.chunks(lens, lim) for name, lim in sd.CHUNKINGS}
    assert [len(found[name]) for name, _ in sd.CHUNKINGS] == [151, 443, 1]
    assert sum(1 for _, _, bases in found["a chunk of empty sequences only"] if bases == 0) == 5
    own = found["every sequence with bases its own chunk"]
    assert len({a for a, _, _ in own}) == 443 >= 200 and max(a for a, _, _ in own) == 65536
    assert all(sum(1 for L in lens[a:b] if L) <= 1 for a, b, _ in own)
    hp = sd.hpc_build_seqs()
    assert len(hp) >= 60 and any(b"A" * 129 in s for s in hp) and any(b"A" * 237 in s for s in hp)


def test_max_occ_tables_sit_on_integer_boundaries():
    assert sd.OCC_KEYS == (1, 2, 3, 4999, 5000, 5001, 9999, 10000, 10001) and sd.OCC_FRACS == (2e-4, 0.25, 0.5, 1.0, 0.0)
    assert [sd.occ_rank(n, 2e-4) for n in sd.OCC_KEYS] == [0, 1, 2, 4998, 4999, 4999, 9997, 9998, 9998]
    assert [sd.occ_rank(n, 0.25) for n in sd.OCC_KEYS] == [0, 1, 2, 3749, 3750, 3750, 7499, 7500, 7500]
    for nk in sd.OCC_KEYS:
        keys, cr, n, hits = sd.occ_table(nk)
        assert np.array_equal(np.sort(n), np.arange(1, nk + 1)) and np.unique(keys).size == nk and hits.size == nk
        for frac in sd.OCC_FRACS:
            rank = sd.occ_rank(nk, frac)
            assert frac == 0.0 or rank < nk, "the reference reads out of bounds where the rank equals n_keys"
            want = 2**31 - 1 if frac == 0.0 else rank + 2              # the counts sorted are 1 ... n_keys
            assert im.cal_max_occ(n, frac) == want == sd.max_occ_v(n, frac), (nk, frac)


# ---- the model is the reference's at these inputs -----------------------------------------------------------------------------------------------------------------
def _input_sha(reads):
    import hashlib
    import struct
    h = hashlib.sha256()
    for r in reads:
        h.update(struct.pack("<q", len(r)) + bytes(r))
    return np.frombuffer(h.digest(), np.uint8)


@pytest.mark.parametrize("S", SETTINGS, ids=IDS)
def test_model_equals_the_reference_on_every_read(fx, S):
    name = "k%d_w%d_h%d" % S
    cs = sd.cases(S)
    assert fx[name + "_input_sha"].shape[0] == len(cs)
    for i, c in enumerate(cs):
        assert np.array_equal(_input_sha(c["reads"]), fx[name + "_input_sha"][i]), f"{c['name']}: the data module no longer makes the input the fixture was made from"
    mini = sd.model(S)
    assert np.array_equal(np.concatenate([[0], np.cumsum([m.shape[0] for m in mini])]), fx[name + "_off"])
    reads, where = sd.batch(S)
    for c in cs:
        for r in range(*where[c["name"]]):
            assert np.array_equal(sm.sha(mini[r]), fx[name + "_sha"][r]), f"{c['name']}: read {r} ({len(reads[r])} bases): the model differs from the reference"


@pytest.mark.parametrize("S", [(15, 10, 0), (19, 5, 1)], ids=["k15-w10", "k19-w5-hpc"])
@pytest.mark.parametrize("n_seqs", [3, 257])
def test_index_model_equals_the_reference(fx, S, n_seqs):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ref_sketch_limit_fixtures", os.path.join(HERE, "golden", "make_ref_sketch_limit_fixtures.py"))
    k, w, hpc = S
    name = "k%d_w%d_h%d_n%d" % (S + (n_seqs,))
    seqs = sd.seq_list(n_seqs, S)[0]
    keys, cr, n, pool = im.build_index(seqs, k, w, hpc)
    assert np.array_equal(_input_sha(seqs), fx[name + "_input_sha"][0])
    assert np.array_equal(sm.sha(np.concatenate([keys.astype("<u8").view(np.uint8), n.astype("<u4").view(np.uint8)])), fx[name + "_table_sha"][0])
    plant = [key for key in sd.planted_keys(S) if key in set(keys.tolist())]
    assert plant == fx[name + "_plant_keys"].tolist() and len(plant) >= 6
    for key, want in zip(plant, fx[name + "_plant_sha"]):
        i = int(np.searchsorted(keys, np.uint64(key)))
        hits = pool[cr[i]:cr[i] + n[i]]
        assert np.array_equal(sm.sha(hits), want), f"key {key:#x}: the hit list differs from the reference's"
        assert int(hits[0] >> np.uint64(32)) == 0 and int(hits[-1] >> np.uint64(32)) == n_seqs - 1
    mid_occ = int(fx[name + "_mid_occ"][0])
    assert im.cal_max_occ(n) == mid_occ
    # collect_matches against that index, the pool offsets left out
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    reads = mod.index_reads(S, n_seqs)
    assert np.array_equal(_input_sha(reads), fx[name + "_input_sha"][1])
    look = sm.table_lookup(keys, cr, n)
    mo = [0]
    for q, r in enumerate(reads):
        m, rep_len, mini_pos = sm.collect_matches(sm.sketch_array(r, w, k, hpc), look, mid_occ)
        m = sm.match_array(m)
        mo.append(mo[-1] + m.size)
        fields = np.ascontiguousarray(m[list(mod.MATCH_FIELDS.names)]).astype(mod.MATCH_FIELDS)
        assert np.array_equal(sm.sha(fields), fx[name + "_match_sha"][q]), f"read {q}: the matches differ from the reference's"
        assert np.array_equal(sm.sha(np.array(mini_pos, np.uint64)), fx[name + "_mini_pos_sha"][q]) and rep_len == int(fx[name + "_rep_len"][q])
    assert mo == fx[name + "_match_off"].tolist()
    # mm_idx_cal_max_occ(2e-4) of so few keys is the largest count plus one: nothing is repetitive here (the lookup cases choose t per key instead)
    assert mo[-1] > 100 and not fx[name + "_rep_len"].any(), "reads that match"


# ---- each family discriminates -------------------------------------------------------------------------------------------------------------------------------------
def _caught(S, families, err):
    """the cases of these families on which the restatement with `err` switched on differs from the model"""
    out = []
    for c in sd.cases(S):
        if c["family"] in families:
            if any(not np.array_equal(sd.lanes_sketch(r, *S, err), np.array(sd.sk(S, r), dtype=np.uint64).reshape(-1, 2)) for r in c["reads"]):
                out.append(c["name"])
    return out


@pytest.mark.parametrize("S", SETTINGS, ids=IDS)
def test_the_restatement_without_an_error_is_the_model(S):
    for c in sd.cases(S):
        for r in c["reads"][:40]:
            if len(r) <= 5000:
                assert np.array_equal(sd.lanes_sketch(r, *S), np.array(sd.sk(S, r), dtype=np.uint64).reshape(-1, 2)), c["name"]


def test_registers_cleared_at_an_ambiguous_base_are_caught_by_the_palindromes():
    for S in ((16, 10, 0), (28, 255, 0)):
        assert _caught(S, ("palindrome", "registers"), "clear_at_n") == [f"palindrome_across_{m}" for m in (1, 64, 70, 130)]


def test_a_span_cut_one_off_is_caught_by_the_span_cases():
    at = [f"span_255_at_{o}" for o in (0, 1, 63)]
    assert _caught((19, 5, 1), ("span",), "span_255") == at + ["span_255_n_before_run", "span_255_n_cuts_walk"]
    assert _caught((5, 3, 1), ("span",), "span_255") == at + ["span_255_n_cuts_walk"]
    for S in ((19, 5, 1), (5, 3, 1)):
        assert _caught(S, ("span",), "span_257") == [f"span_256_at_{o}" for o in (0, 1, 63)]


def test_a_rebuild_that_keeps_the_oldest_minimum_is_caught_by_the_ties():
    counts = {}
    for S in SETTINGS:
        got = _caught(S, ("ties", "first_window"), "rebuild_gt")
        counts[S] = len(got)
        if S[1] > 1:
            assert any(n.startswith("ties_") for n in got), S
    print(counts)
    assert counts[(15, 1, 0)] == 0, "w = 1: one slot, no tie to choose from"
    assert all(counts[S] >= 5 for S in SETTINGS if S[1] > 1), counts
    got = _caught((28, 255, 0), ("ties",), "rebuild_gt")
    assert any(n.startswith("ties_p3_") for n in got) and any(n.startswith("ties_p100_") for n in got)


def test_a_first_window_loop_left_out_at_a_lanes_first_slot_is_caught_there_only():
    for S in SETTINGS:
        want = [] if S[1] == 1 else ["first_window_at_512" if S == (28, 255, 0) else "first_window_at_256"]
        assert _caught(S, ("first_window",), "no_first_window") == want, S


def test_l_not_reset_across_a_lane_edge_is_caught_and_l_not_saturated_cannot_be():
    for S in SETTINGS:
        got = _caught(S, ("registers", "l_edges"), "l_noreset")
        if not S[2]:
            assert {f"n_run_{run}_at_{o}" for run in (1, 63) for o in (62, 63)} <= set(got), (S, got)
        else:
            assert "l_k_at_63" in got, (S, got)
        # sk_slots caps l again at the lane's first step, whatever the scan handed over
        assert _caught(S, ("registers", "l_edges", "first_window"), "l_unsat") == [], S


def _lookup_caught(err):
    out = {}
    for c in sd.lookup_cases():
        k, w, hpc = c["kwh"]
        minis = [sm.sketch_array(r, w, k, hpc) for r in c["reads"]]
        look = sm.table_lookup(*c["table"][:3])
        ref = sd.lookup_model(c)
        assert sd.collect_matches_v(minis, look, c["mid_occ"]) == ref, c["name"]
        bad = [q for q, (a, b) in enumerate(zip(sd.collect_matches_v(minis, look, c["mid_occ"], err), ref)) if a != b]
        if bad:
            out[c["name"]] = bad
    return out


def test_lookup_errors_are_caught_by_their_cases():
    assert _lookup_caught("tandem_across_reads") == {"tandem_edges": [0, 1, 2]}, "r | r and r | r[:len//2]: the flag looked across a read's edge"
    got = _lookup_caught("mid_le")
    assert set(got) == {"tandem_unfiltered", "mid_occ_1", "mid_occ_2", "mid_occ_50", "mid_occ_0", "rep_len_rounds"}
    assert "mid_occ_2147483647" not in got, "no t reaches 2^31 - 1"
    assert _lookup_caught("rep_round_reset")["rep_len_rounds"] == [4, 10, 14, 15], "the overlapping pairs (63, 64) and (127, 128), and 65 / 129 repetitive in a row"
    assert _lookup_caught("rep_ge") == {}, "touching intervals add up to the same length merged or apart: '>=' for '>' is no error"


def test_a_y_sort_one_bit_short_is_caught_by_every_list_of_two_or_more():
    for n in sd.N_SEQS:
        mini = sd.list_minimizers(n)
        ref = im.build_from_minimizers(mini)
        for a, b in zip(sd.build_index_v(mini, n), ref):
            assert np.array_equal(a, b)
        wrong = sd.build_index_v(mini, n, "y_bits_short")
        assert np.array_equal(wrong[3], ref[3]) == (n == 1), f"{n} sequences: the top bit of the largest rid decides an order"


def test_a_max_occ_rank_one_off_is_caught_by_every_table():
    for nk in sd.OCC_KEYS:
        n = sd.occ_table(nk)[2]
        for frac in sd.OCC_FRACS[:-1]:
            rank, ref = sd.occ_rank(nk, frac), im.cal_max_occ(n, frac)
            assert (sd.max_occ_v(n, frac, "occ_rank_up") != ref) == (rank + 1 < nk), (nk, frac)
            assert (sd.max_occ_v(n, frac, "occ_rank_down") != ref) == (rank > 0), (nk, frac)
    assert sd.max_occ_v(sd.occ_table(5001)[2], 2e-4, "occ_rank_up") == 5002 and sd.max_occ_v(sd.occ_table(5001)[2], 2e-4, "occ_rank_down") == 5000
