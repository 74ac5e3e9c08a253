"""tests/limit_data.py does what it says: asserted from the oracle's f / p alone, without a GPU.  These are conditions on the inputs of tests/test_gpu_scalar_limits.py --
a limit input that does not reach its limit tests nothing."""
import time

import numpy as np
import pytest

import limit_data as ld
from helpers import oracle_batch
from reuse_data import batch



def _xq(t):
    return (t[:, 0] & np.uint64(0xffffffff)).astype(np.int64), (t[:, 1] & np.uint64(0xffffffff)).astype(np.int64)


def best_links(tasks, f, p):
    """dr, dq, anchors strictly between p[i] and i, and f[p[i]] of every anchor that has a predecessor"""
    a, off = batch(tasks)
    cols = []
    for k, t in enumerate(tasks):
        pp, ff = p[off[k]:off[k + 1]], f[off[k]:off[k + 1]]
        i = np.nonzero(pp >= 0)[0]
        x, q = _xq(t)
        cols.append((x[i] - x[pp[i]], q[i] - q[pp[i]], i - pp[i] - 1, ff[pp[i]]))
    return [np.concatenate(c) for c in zip(*cols)]


def check_tasks(tasks):
    for t in tasks:
        assert t.dtype == np.uint64 and t.shape[0] > 0 and t.shape[1] == 2
        assert np.all(t[1:, 0] >= t[:-1, 0]), "a task must be sorted by x"


def _oracle(P, tasks):
    a, off = batch(tasks)
    return oracle_batch(P, off, a)


X_CASES = [(65534, 32768), (65535, 32768), (65536, 32768), (65537, 32768), (65535, 32767), (65535, 32769)]


@pytest.mark.parametrize("far", [False, True], ids=["ring", "far"])
@pytest.mark.parametrize("D,dq_max", X_CASES)
def test_x_limit_links_are_taken_at_the_limit_and_never_beyond(D, dq_max, far):
    P, tasks = ld.x_limit_far(D, dq_max) if far else ld.x_limit(D, dq_max)
    check_tasks(tasks)
    assert (P.max_dist_x, P.max_dist_y, P.bw, P.gap_scale) == (D, dq_max, min(D, dq_max) - 1, 1.0) and min(D, dq_max) - 1 >= P.bw
    f, p = _oracle(P, tasks)
    dr, dq, between, f_pred = best_links(tasks, f, p)
    # every kind of link occurs in the input at least four times: the first anchor of a cluster and the last of the cluster before it (in x: the nearest
    # anchor of all that lies at least 30 000 below and is not a stepping anchor, i.e. is followed by another anchor within 20)
    seen = {}
    for t in tasks[:16 if not far else len(tasks)]:
        x, q = _xq(t)
        dense = np.concatenate((np.diff(x) <= 20, [False])) | np.concatenate(([False], np.diff(x) <= 20))
        xc, qc = x[dense], q[dense]
        heads = np.nonzero(np.diff(xc) > 30000)[0]
        for h in heads:
            key = (int(xc[h + 1] - xc[h]), int(qc[h + 1] - qc[h]))
            seen[key] = seen.get(key, 0) + 1
    for kind in ld.limit_kinds(D, dq_max):
        assert seen.get(kind, 0) >= 4, (kind, seen)
    # nothing beyond the limits is ever taken
    assert not (dr > D).any() and not (dq > dq_max).any() and not (np.abs(dr - dq) > P.bw).any()
    assert (dr == D + 1).sum() == 0 and (dq == dq_max + 1).sum() == 0
    # at the limits: dq == dq_max always; dr == D where the band admits it (D - dq_max <= bw), else the band's own edge dq_max + bw
    edge = min(D, dq_max + P.bw)
    at_edge = dr == edge
    assert (dq == dq_max).sum() >= 4 and at_edge.sum() >= 4, ((dq == dq_max).sum(), at_edge.sum())
    if D - dq_max > P.bw:
        assert edge < D and (dr > edge).sum() == 0              # (65536, 65537 with dq_max 32768; 65535 with 32767: no link at dr == D can pass chain.c:205)
    else:
        assert edge == D
    # ... each from a predecessor whose f outweighs the gap cost, with the margin the builder promises
    lim = dr >= edge - 1
    for a_dr, a_dq, a_f in zip(dr[lim], dq[lim], f_pred[lim]):
        assert a_f > ld.required_f(P, int(a_dr), int(a_dq)) + 500, (a_dr, a_dq, a_f)
    if far:
        assert between[lim].min() >= 1100 and P.max_iter >= between[lim].max() + 1
    else:
        assert between[lim].max() < 900 and between[lim].min() >= 20
        # the tasks for the compact ring: q values that span exactly the bound, and a link whose dr needs bit 15
        for t in tasks[16:]:
            assert ld.q_span(t) == 65535 - dq_max
        _, off = batch(tasks)
        dr_c = best_links(tasks[16:], f[off[16]:], p[off[16]:])[0]
        assert (dr_c >= 32768).sum() >= 4 and dr_c.max() <= 65534
        for t in tasks[:16]:
            assert ld.q_span(t) > 65535 - dq_max


@pytest.mark.parametrize("dq_max", [32767, 32768])
def test_q_spans_on_both_sides_of_the_bound_of_the_largest_max_dq(dq_max):
    P, tasks, modes = ld.q_span_at_scalar_limit(dq_max)
    check_tasks(tasks)
    assert min(P.max_dist_x, P.max_dist_y) == dq_max and P.max_dist_x == 65535
    bound = 65535 - dq_max
    for t, mode in zip(tasks, modes):
        s = ld.q_span(t)
        assert (s <= bound) == (mode in (0, 3)), (mode, s)
        if mode in (3, 4):
            assert s == bound + (mode == 4)
    _oracle(P, tasks)


def test_key32_n_reaches_the_largest_score_of_the_guard():
    (P, t0), (P1, t1) = ld.key32_limit("n")
    check_tasks(t0 + t1)
    assert t0[0].shape[0] == 32767 and t1[0].shape[0] == 32768 and P.max_skip == ld.INT32_MAX and P.max_iter == 5000
    f0, p0 = ld.reference(P, t0)
    f1, p1 = ld.reference(P1, t1)
    assert 32767 * 255 >= int(f0.max()) >= 32767 * 255 - 255 * 64
    assert 32768 * 255 >= int(f1.max()) >= 32768 * 255 - 255 * 64
    # 32768 * 255 = 8 355 840 is still below 2^23 = 8 388 608: one anchor past the guard the word is not yet at its end
    assert int(f1.max()) < (1 << 23)
    assert (p0[1:] != np.arange(32766)).sum() >= 48                        # the jitter makes other origins than the neighbour win


def test_key32_span_reaches_the_largest_score_of_the_guard():
    (P255, t), (P256, _) = ld.key32_limit("span")
    check_tasks(t)
    assert (P255.q_span_override, P256.q_span_override) == (255, 256) and t[0].shape[0] == 32767
    f, p = ld.reference(P255, t)
    assert int(f.max()) == 32767 * 255 and np.array_equal(p, np.arange(-1, 32766))
    f, p = ld.reference(P256, t)
    assert np.array_equal(f, 256 * np.arange(1, 32768)) and np.array_equal(p, np.arange(-1, 32766))
    assert (1 << 23) > int(f.max()) == 32767 * 256 == (1 << 23) - 256         # 8 388 352: the last multiple of 256 below 2^23


def test_key32_gap_scale_and_bw_cases():
    cases = ld.key32_limit("gap_scale")
    assert [P.gap_scale for P, _ in cases] == [4.0, 4.5] and all(P.bw <= 511 for P, _ in cases)
    fs = [ld.reference(P, t)[0] for P, t in cases]
    check_tasks(cases[0][1])
    assert (fs[0] != fs[1]).sum() > 1000 and min(int(f.max()) for f in fs) > 7000000
    for P, t in ld.key32_limit("bw"):
        check_tasks(t)
        assert P.bw in (131072, 131073) and P.max_dist_x == P.max_dist_y == 200000 and t[0].shape[0] == 32767
        f, p = ld.reference(P, t)
        dr, dq, between, f_pred = best_links(t, f, p)
        dd = np.abs(dr - dq)
        assert ((dd >= P.bw - 64) & (dd <= P.bw)).sum() >= 4 and (dd == P.bw).sum() >= 1 and not (dd > P.bw).any()
        assert int(f.max()) > (1 << 21)


@pytest.mark.parametrize("bw", ld.TABLE_BW)
def test_table_limit_links_at_the_last_entries(bw):
    cases = {gs: (P, t) for gs, (P, t) in zip(ld.TABLE_GS * 2, ld.table_limit()) if P.bw == bw}
    assert all(np.float32(gs) == np.float32(P.gap_scale) for gs, (P, _) in cases.items()) and len(cases) == 5
    tasks = cases[0.8][1]
    check_tasks(tasks)
    assert len(tasks) == 7 and all(200 <= t.shape[0] <= 3000 for t in tasks)
    fs = {}
    for gs, (P, t) in cases.items():
        f, p = _oracle(P, t)
        fs[gs] = f
        dr, dq, _, _ = best_links(t[-1:], f[-t[-1].shape[0]:], p[-t[-1].shape[0]:])
        dd = np.abs(dr - dq)
        assert ((dd >= 509) & (dd <= 511)).sum() >= 10, (gs, np.bincount(dd)[505:])
        assert (dd == 512).sum() == (3 if bw == 512 else 0)
    assert (fs[-19.5] != fs[19.5]).any() and (fs[-20.0] != fs[20.0]).any() and (fs[19.5] != fs[20.0]).any()


def test_preset_data():
    P, tasks = ld.splice_tasks()
    check_tasks(tasks)
    assert (P.max_dist_x, P.max_dist_y, P.bw, P.is_cdna, P.n_segs) == (200000, 2000, 200000, 1, 1)
    f, p = _oracle(P, tasks)
    _, off = batch(tasks)
    for k, intron in enumerate((1000, 10000, 100000, 200000, 200001)):
        dr = best_links(tasks[k:k + 1], f[off[k]:off[k + 1]], p[off[k]:off[k + 1]])[0]
        assert (dr == intron).sum() == (4 if intron <= P.max_dist_x else 0), (intron, dr.max())      # every intron up to max_dist_x is bridged, one more is not
    P, tasks = ld.sr_tasks()
    check_tasks(tasks)
    assert (P.max_dist_x, P.max_dist_y, P.bw, P.is_cdna, P.n_segs) == (500, 300, 100, 0, 2)
    assert all(10 <= t.shape[0] <= 200 for t in tasks)
    assert all(len(np.unique((t[:, 1] >> np.uint64(48)) & np.uint64(0xff))) == 2 for t in tasks)
    _oracle(P, tasks)


def test_prediction_windows():
    import oracle_binding as ob
    t, probes = ld.predict_window_task()
    check_tasks([t])
    ns, tot, trip = ob.predict(t, 5000)
    assert list(ns[probes]) == [1, 1, 1, 1, 2, 8, 8, 8]
    x = t[:, 0].astype(np.int64)
    win = [int(((x[:i] >= x[i] - 5000)).sum()) for i in probes]
    assert win == [0, 1, 127, 128, 129, 1023, 1024, 1500]


def test_zz_the_module_builds_in_under_twenty_seconds():
    """every builder once more, from nothing, and the oracle over the largest input"""
    t0 = time.perf_counter()
    for D, dq_max in X_CASES:
        ld.x_limit(D, dq_max)
        P, tasks = ld.x_limit_far(D, dq_max)
    _oracle(P, tasks)
    for dq_max in (32767, 32768):
        ld.q_span_at_scalar_limit(dq_max)
    for kind in ("n", "span", "gap_scale", "bw"):
        ld.key32_limit(kind)
    ld.table_limit(); ld.splice_tasks(); ld.sr_tasks(); ld.predict_window_task()
    took = time.perf_counter() - t0
    print(f"limit data: every builder in {took:.1f} s")
    assert took < 20.0, took
