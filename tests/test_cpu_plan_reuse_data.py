"""The preconditions of tests/test_gpu_plan_reuse.py, asserted from the oracle and the stated rules alone: the data sets of tests/reuse_data.py, run one after the
other on ONE plan, differ from run to run in everything a plan keeps between runs -- so a run that read a word the run before left behind (the packed f / p side array,
st[], the class bytes, the cut arena) differs from the oracle somewhere and the GPU test cannot pass by luck.  Nothing here calls the library."""
import numpy as np
import pytest

import reuse_data as rd
from tile_model import chain_tile_model

PAIRS = sorted({(a, b) for a, b in zip(rd.ORDER[:-1], rd.ORDER[1:])})


def test_offsets_fit_the_packed_ring_and_one_task_is_cut():
    assert max(rd.SIZES) <= rd.PK_MAX_N and max(rd.SIZES) >= 8192 and 0 in rd.SIZES and 1 in rd.SIZES      # (8192: the default plan_cut_min)
    assert len(rd.ORDER) <= 9 and set(rd.ORDER) == set("ABCDEF")
    for name in "ABCDEF":
        for t in rd.get(name):
            assert np.all(t[1:, 0] >= t[:-1, 0]), name                                                 # sorted by x, as mm_chain_dp needs


@pytest.mark.parametrize("a,b", PAIRS)
def test_consecutive_sets_differ_in_f_and_p(a, b):
    (fa, pa), (fb, pb) = rd.reference(a), rd.reference(b)
    worst_f, worst_p = 1.0, 1.0
    for k, n in enumerate(rd.SIZES):
        if n <= 64:
            continue
        s = slice(rd.OFF[k], rd.OFF[k + 1])
        df, dp = float((fa[s] != fb[s]).mean()), float((pa[s] != pb[s]).mean())
        worst_f, worst_p = min(worst_f, df), min(worst_p, dp)
        assert df >= 0.90 and dp >= 0.01, f"{a} -> {b}, task {k}: f differs at {df:.3f} of the anchors, p at {dp:.3f}"
    print(f"{a} -> {b}: smallest share of differing f {worst_f:.3f}, of differing p {worst_p:.3f}")


def test_class_bits_change_around_c():
    bits = {name: rd.expected_class_bits(rd.get(name)) for name in "ABCD"}
    live = np.array(rd.SIZES) > 0
    assert np.array_equal(bits["A"], bits["B"])                                                        # B redraws the spans and keeps every class
    assert ((bits["A"] & 8) != 0)[live].all() and not (bits["A"] & 2).any()
    for other in "BD":
        n = int(((bits["C"] != bits[other]) & live).sum())
        print(f"class bits 1 and 3 of C and {other} differ for {n} tasks")
        assert n >= 3, (bits["C"], bits[other])
    c = rd.get("C")
    assert rd.span_sum(c[0]) > rd.PK_MAX_F and rd.span_sum(c[7]) > rd.PK_MAX_F and not (bits["C"][[0, 7]] & 8).any()
    assert (bits["C"][live] & 2).all()                  # tasks 1, 2 and 6 hold more than wide_share_threshold % of the anchors: every task takes the 32-bit ring
    assert rd.span_sum(rd.get("B")[0]) <= rd.PK_MAX_F


def test_d_and_e_have_other_empty_windows():
    seen = {}
    for name in "DE":
        _, p = rd.reference(name)
        tasks, cuts = rd.get(name), set()
        for k, t in enumerate(tasks):
            e = rd.empty_windows(t)
            assert e.tolist() == [j + 1 for j in rd.JUMPS[name].get(k, ())], (name, k, e)
            assert (p[rd.OFF[k] + e] == -1).all()
            cuts |= {(k, int(i)) for i in e}
        seen[name] = cuts
    assert seen["D"] and seen["E"] and not (seen["D"] & seen["E"]), seen
    assert sum(k == 0 for k, _ in seen["D"]) == 1 and sum(k == 0 for k, _ in seen["E"]) == 2      # task 0, the one at plan_cut_min: two pieces in D, three in E
    for name in "ABCF":
        assert all(rd.empty_windows(t).size == 0 for t in rd.get(name)[:1]), name                       # the task that is cut has nothing to cut at in the other sets


@pytest.mark.parametrize("name", "AB")
def test_scored_tiles_come_from_beyond_the_packed_ring(name):
    """the model of the tile loop's control flow: scored tiles deeper than the four tiles of the packed f / p ring exist (deep_fp), so the side array d_w is read"""
    P = rd.scalars()
    deep = ring = 0
    for k in (1, 8):
        t = rd.get(name)[k]
        avg = float(np.float32(.01 * float(np.float32(rd.span_sum(t))) / t.shape[0]))
        st = {}
        chain_tile_model(P, t, avg, stats=st, NX=16, NF=4, score_exit="off", late_stamps=False)
        deep += st["deep_fp"]; ring += st["ring_pass"]
    print(f"set {name}: deep_fp {deep}, ring_pass {ring}")
    assert deep > 0 and ring > deep


def test_f_of_the_dense_tasks_and_far_windows():
    """F: windows of tasks 2 and 6 reach beyond the ring of 16 tiles (960 anchors before the current tile)"""
    for k in (2, 6):
        t = rd.get("F")[k]
        x = t[:, 0]
        st = np.searchsorted(x, x - np.uint64(5000), side="left")
        assert int((np.arange(x.size) - st).max()) > 64 * 16, k
