"""The seed-hit path at the limits of its size classes, key widths, run lengths and bucket forms: the reads of tests/seed_limit_data.py (tests/test_cpu_seed_limit_data.py
asserts that each reaches its limit and that a stable sort would not pass) through mm2chain.seed_hits_batch, SeedPlan.run and SeedPlan.run_skip, bit for bit against
the oracle's collect_seed_hits."""
import numpy as np
import pytest
import torch

import oracle_binding as ob
import seed_limit_data as sd
from test_gpu_seed_hits import _batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def _compare(cases, got, what):
    for k, c in enumerate(cases):
        ref = sd.reference(c)
        assert got[k].shape == ref.shape, f"{what}: {c['name']}: {got[k].shape[0]} anchors, expected {ref.shape[0]}"
        bad = np.nonzero((got[k] != ref).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {c['name']}: {bad.size} of {ref.shape[0]} anchors differ, first at {i}: "
                                 f"{int(got[k][i, 0]):#x} {int(got[k][i, 1]):#x} instead of {int(ref[i, 0]):#x} {int(ref[i, 1]):#x}")


def _host(cases, what):
    import mm2chain
    mo, m, h, ql = _batch([c["read"] for c in cases])
    ao, a = mm2chain.seed_hits_batch(mo, m, h, ql)
    _compare(cases, [a[ao[k]:ao[k + 1]] for k in range(len(cases))], what + " (seed_hits_batch)")


def _plan(cases, what, flag=0, heap=False):
    """SeedPlan.run (where no flag drops hits), then SeedPlan.run_skip with `flag` on the same plan: anchors, and the packed offsets against the exact counts"""
    import mm2chain
    mo, m, h, ql = _batch([c["read"] for c in cases])
    cap = np.concatenate([[0], np.cumsum([int(c["read"][1]["n"].sum()) for c in cases])]).astype(np.int64)
    sp = mm2chain.SeedPlan(mo, cap)
    if heap:
        sp.set_heap_sort(True)
    d_m = torch.from_numpy(m.view(np.uint8).copy()).cuda(); d_h = torch.from_numpy(h.view(np.int64).copy()).cuda(); d_q = torch.from_numpy(ql).cuda()
    try:
        if flag == 0:
            a = sp.run(d_m, d_h, d_q); sp.check()
            a = a.cpu().numpy().view(np.uint64)
            _compare(cases, [a[cap[k]:cap[k + 1]] for k in range(len(cases))], what + " (SeedPlan.run)")
        a, off = sp.run_skip(d_m, d_h, d_q, flag, None, None, None, None); sp.check()
        a, off = a.cpu().numpy().view(np.uint64), off.cpu().numpy()
        want = np.concatenate([[0], np.cumsum([c["na"] for c in cases])])
        assert np.array_equal(off, want), f"{what}: offsets of the kept anchors {off} instead of {want}"
        _compare(cases, [a[off[k]:off[k + 1]] for k in range(len(cases))], what + " (SeedPlan.run_skip)")
    finally:
        sp.close()


def _all(cases, what):
    _host(cases, what)
    _plan(cases, what)


# ---- A: runs of equal x ---------------------------------------------------------------------------------------------------------------------------------------------
def test_runs_of_222_to_1000_equal_x():
    """runs at both sides of RUN_MAX = 224 in the one-wave class: 223 (the longest the windowed fix-up takes, starting at every residue modulo 64, at position 0, ending
    at position na - 1), 224 and more (the full sort of the arrangement)"""
    _all(sd.set_a_223() + sd.set_a_lengths(), "runs")


def test_runs_of_223_and_224_in_the_multi_wave_classes_and_reads_of_one_x():
    _all(sd.set_a_long() + sd.set_a_one_x(), "long runs")


def test_runs_of_223_and_224_with_the_digits_in_memory(monkeypatch):
    monkeypatch.setenv("MM2C_TIE_GLOBAL_ABOVE", "1000")                          # read when a seed plan is made
    cases = sd.set_a_223()[:2] + [c for c in sd.set_a_lengths() if c["name"] in ("A-L224", "A-L223+224")]
    assert all(c["na"] > 1000 for c in cases)
    for waves in ("1", "8"):
        monkeypatch.setenv("MM2C_TIE_GLOBAL_WAVES", waves)
        _host(cases, f"digits in memory, {waves} wave(s)")


# ---- B: size classes ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_n_and_n_plus_1_anchors_at_every_class_boundary(which):
    _all(sd.set_b_batches()[which], f"boundaries, batch {which}")


def test_sort_boundaries_through_the_global_sort_and_the_one_wave_kernels(monkeypatch):
    cases = [sd.size_case(n) for n in (5120, 16385, 5121, 16384)]
    monkeypatch.setenv("MM2C_LDS_SORT", "0")
    _host(cases, "MM2C_LDS_SORT=0")
    monkeypatch.delenv("MM2C_LDS_SORT")
    monkeypatch.setenv("MM2C_MW_SORT", "0")
    _host([cases[0], cases[1]], "MM2C_MW_SORT=0")


def test_capacity_in_one_class_and_kept_count_in_another():
    """MM_F_FOR_ONLY keeps an exact number of a read's hits: the sorts go by the capacity (16 385 and 131 073: the sixteen-wave kernels), seed_ties by the kept count
    (64: no replay, 65, 2 561, 5 121, 12 289: the first read of four classes); the packed offsets give the counts"""
    cases = [sd.skip_case(cap, kept) for cap, kept in sd.SKIP_CASES]
    order = [2, 4, 0, 3, 1]
    _plan([cases[k] for k in order], "capacity against count", flag=ob.F_FOR_ONLY)


def test_heap_order_with_2047_2048_and_2049_matches():
    """the heap of seed_heap lives in LDS for up to 2 048 matches and in the read's scratch beyond"""
    cases = [sd.heap_case(n) for n in (2049, 2047, 2048)]
    _plan(cases, "heap", heap=True)


# ---- C: key widths --------------------------------------------------------------------------------------------------------------------------------------------------
def test_key_widths_from_1_to_33_bits():
    _all(sd.set_c_kb(), "kb")


def test_key_and_index_bits_of_64_and_65():
    """kb + idb = 64: the last one-word key (about 20 000 anchors: on sixteen waves); 65: the anchors themselves are sorted, by one wave, and again at the end of
    seed_ties -- with every run shorter than 224 and with a run of 224; 2 048 against 2 049 anchors: one more anchor, one more index bit"""
    _all(sd.set_c_sum(), "kb + idb")


# ---- D: bucket structure ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lds", "memory-1-wave", "memory-8-waves"])
def test_bucket_forms_of_the_replay(route, monkeypatch):
    if route != "lds":
        monkeypatch.setenv("MM2C_TIE_GLOBAL_ABOVE", "64")
        monkeypatch.setenv("MM2C_TIE_GLOBAL_WAVES", "1" if route == "memory-1-wave" else "8")
    _all(sd.set_d(), route)


# (the epilogue's other limits -- key width, 1 024 chain ends, 768 with distinct x, CAP / 2, 4 096 tied chains, chunks of 256: tests/test_gpu_epilogue_limits.py)
def test_epilogue_orders_64_65_768_and_769_chains_with_equal_first_x():
    import mm2chain
    from mm2chain import params
    P = params.map_ont()
    tasks = [sd.tandem_task(n, 9700 + n) for n in sd.TANDEM_CHAINS]
    off = np.concatenate([[0], np.cumsum([t.shape[0] for t in tasks])]).astype(np.int64)
    res = mm2chain.mm_chain_dp_batch(P, 3, 40, off, np.concatenate(tasks), epilogue_threads=0)
    for k, t in enumerate(tasks):
        u_ref, b_ref = ob.mm_chain_dp(P, 3, 40, t)
        assert u_ref.size == sd.TANDEM_CHAINS[k]
        assert np.array_equal(res[k][0], u_ref) and np.array_equal(res[k][1], b_ref), f"{sd.TANDEM_CHAINS[k]} chains: the order differs from the reference's"


# ---- E: encoding ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_spans_segments_query_ends_and_query_lengths():
    _all(sd.set_e(), "encoding")
