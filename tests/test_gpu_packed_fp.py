"""The packed f / p ring of the tile kernel (csrc/chain_dp_tile.h, Lds<> RING 3): f - 14 and the piece-relative p of a ring anchor in ONE word (18 + 14 bits, both
signed), four tiles of them in the LDS that held two tiles of pairs, and the same word in a side array so that a scored tile deeper than the ring is one load.  The
prepass marks the tasks whose values fit (bit 3 of the class byte: at most 8192 anchors, span sum at most 2^17 - 1); every other task runs the form with pairs.
Every case is compared element for element with the CPU oracle, with the knob on and off, and the class bytes are read back to show who took which form."""
import numpy as np
import pytest

from helpers import assert_same, gpu_batch, knobs, oracle_batch  # noqa: F401 (knobs: a fixture)
from reuse_data import PK_MAX_F, PK_MAX_N, batch, chain_with_noise, span_sum, task_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    import torch
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def run_both(P, tasks, knobs, what, ref_tasks=None):
    """oracle == GPU with packed_fp 1 == GPU with packed_fp 0; returns the class bytes of the run with the knob on"""
    import torch
    import mm2chain
    a, off = batch(tasks)
    # (ref_tasks: the anchors the oracle runs on, where P holds something the oracle's scalars do not -- q_span_override -- and other anchors say the same)
    f_ref, p_ref = oracle_batch(P, off, a if ref_tasks is None else batch(ref_tasks)[0])
    out = {}
    # a plan with a longer task runs without the packed ring altogether, and says so; so does a plan whose gap cost can be a gain (gap_scale < 0: f may pass the span sum)
    plan_packed = max(t.shape[0] for t in tasks) <= PK_MAX_N and P.gap_scale >= 0
    for pk in (1, 0):
        knobs("packed_fp", pk)
        v = []
        f, p = gpu_batch(P, off, a, variant=v)
        assert_same(f, p, f_ref, p_ref, off, f"{what}, packed_fp={pk}: {v[0]}")
        assert "loop=asm" in v[0] and "compact=1" in v[0] and f"packed_fp={pk if plan_packed else 0}" in v[0], v
        out[pk] = (f, p)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    # the class bytes of one more run with the knob off and on, one wave per piece: they differ in bit 3 only (the ring-size class and the ring form are what they were)
    knobs("coop_plans", 0)
    d_a = torch.from_numpy(a.view(np.int64).reshape(-1, 2)).cuda()
    d_f = torch.empty(a.shape[0], dtype=torch.int32, device="cuda"); d_p = torch.empty_like(d_f)
    by_knob = {}
    for pk in (0, 1):
        knobs("packed_fp", pk)
        plan = mm2chain.ChainPlan(P, off)
        plan.run(d_a, d_f, d_p)
        torch.cuda.synchronize()
        by_knob[pk] = np.frombuffer(plan.last_classes(), np.uint8).copy()
        plan.close()
        assert_same(d_f.cpu().numpy(), d_p.cpu().numpy(), f_ref, p_ref, off, f"{what}, class read-back run, packed_fp={pk}")
    cls = by_knob[1]
    assert not (by_knob[0] & 8).any() and np.array_equal(by_knob[0], cls & ~np.uint8(8)), (by_knob[0], cls)
    f_bound = [P.q_span_override * t.shape[0] if P.q_span_override >= 0 else span_sum(t) for t in tasks]   # what the scores add: the anchors' spans, or the override for each
    want = np.array([plan_packed and b <= PK_MAX_F for b in f_bound])
    assert np.array_equal((cls & 8) != 0, want), (cls, want)
    return cls


@pytest.mark.parametrize("gap_scale", [1.0, 0.8])
def test_scored_tiles_at_every_depth_of_the_ring_and_beyond(gap_scale, knobs):
    """Tasks of 64 k + r anchors (k = 3 .. 6, r = 0, 1, 63) whose chain anchors have their scored predecessors 1, 2, 3, 4, 5 and more tiles back (one chain anchor
    every 40 / 64 / 100 anchors, eleven of them inside a window): the ring of pairs (depth <= 2), the packed ring (<= 4) and the deep fetch are each the source.  A
    dense read whose windows are longer than the ring of 16 tiles takes the `far` form.  gap_scale 0.8 with bw 500: the forms with the gap-cost table."""
    from mm2chain import params, synth
    P = params.map_ont() if gap_scale == 1.0 else params.make_params(max_dist_x=5000, max_dist_y=5000, bw=500, gap_scale=gap_scale)
    rng = np.random.default_rng(404)
    tasks = [chain_with_noise(rng, 64 * k + r, every) for k in (3, 4, 5, 6) for r in (0, 1, 63) for every in (40, 64, 100)]
    # the model of the loop's control flow says where the f / p of the scored tiles come from: for these tasks some lie within two tiles (the ring of pairs holds
    # them), some at three or four (only the packed ring does) and some deeper (the fetch from memory either way)
    from tile_model import chain_tile_model
    got = dict(ring=0, deep2=0, deep4=0)
    for t in tasks[-9:]:                                                   # the tasks of 64 * 6 + r anchors
        avg = float(np.float32(.01 * float(np.float32(span_sum(t))) / t.shape[0]))
        for nf in (2, 4):
            st = {}
            chain_tile_model(P, t, avg, stats=st, NX=16, NF=nf, score_exit="off", late_stamps=False)
            got[f"deep{nf}"] += st["deep_fp"]
        got["ring"] += st["ring_pass"]
    assert got["deep4"] > 0 and got["deep2"] > got["deep4"] and got["ring"] > got["deep2"], got
    tasks.append(synth.make_stream("dense", 1, 2500, seed=41, locus=9000)[1].numpy().view(np.uint64))
    tasks.append(synth.make_stream("mixed", 1, 1500, seed=42)[1].numpy().view(np.uint64))
    cls = run_both(P, tasks, knobs, f"ring depth, gap_scale={gap_scale}")
    assert ((cls & 8) != 0).all()
    import mm2chain
    knobs("packed_fp", 1); knobs("coop_plans", 0)
    v = []
    a, off = batch(tasks)
    gpu_batch(P, off, a, variant=v)
    assert f"TAB={int(gap_scale != 1.0)}" in v[0] and "packed_fp=1" in v[0], v


def test_piece_lengths_at_the_limit_of_p(knobs):
    """p lives in 14 signed bits: a piece of up to 8192 anchors fits (p <= 8190).  Colinear chains of 8191, 8192, 8193 and 9000 anchors (their last anchors have the
    largest p a task of that length can have), equal to the oracle on whichever side they fall; the class bytes show that both sides occurred."""
    from mm2chain import params
    P = params.map_ont()
    rng = np.random.default_rng(8192)
    tasks = []
    for n in (PK_MAX_N - 1, PK_MAX_N, PK_MAX_N + 1, 9000):
        k = np.arange(n)
        pos = 1000 + 30 * k
        q = np.where(rng.random(n) < 0.9, 50 + 30 * k, 50 + 30 * k + rng.integers(600, 3000, n))
        tasks.append(task_of(pos, q, np.full(n, 15)))
    for t in tasks[:3]:
        assert span_sum(t) <= PK_MAX_F                                    # (it is the length that decides for 8193; 9000 anchors fail both bounds)
    cls = run_both(P, tasks[:2], knobs, "p limit, at and below")          # one plan of tasks that fit: the packed form
    assert [bool(c & 8) for c in cls] == [True, True]
    cls = run_both(P, tasks[2:], knobs, "p limit, above")                 # one more anchor: the plan takes the form with pairs
    assert [bool(c & 8) for c in cls] == [False, False]
    cls = run_both(P, tasks, knobs, "p limit, both sides in one plan")
    assert not (cls & 8).any()


def test_span_sums_at_the_limit_of_f(knobs):
    """f - 14 lives in 18 signed bits and f is at most the task's span sum: tasks whose span sum is at most 2^17 - 1 fit.  A colinear chain of span 255 in steps of 255
    (every anchor adds 255: f reaches 255 times its length) with a second diagonal of span-1 anchors (f - 14 below zero is stored too), long enough that the span
    sum lands just below (513 * 255 + 200 = 131 015) and just above (514 * 255 + 200 = 131 270) the bound."""
    from mm2chain import params
    P = params.map_ont()
    tasks = []
    for m in (513, 514):
        k = np.arange(m)
        e = np.arange(200)
        pos = np.concatenate((1000 + 255 * k, 1100 + 600 * e))
        q = np.concatenate((100 + 255 * k, 5000 + 600 * e))
        span = np.concatenate((np.full(m, 255), np.full(200, 1)))
        tasks.append(task_of(pos, q, span))
    assert span_sum(tasks[0]) <= PK_MAX_F < span_sum(tasks[1])
    a, off = batch(tasks)
    f_ref, _ = oracle_batch(P, off, a)
    assert f_ref[:off[1]].max() == 513 * 255 and f_ref.min() == 1          # the largest f the word must hold, and the smallest
    cls = run_both(P, tasks, knobs, "f limit")
    assert [bool(c & 8) for c in cls] == [True, False]


def test_no_predecessor_and_predecessors_in_the_first_tile(knobs):
    """p = -1 and p = 0 through the word: anchor 0 of the task, then 200 / 330 noise anchors without any predecessor (p = -1, stored and read back as such), then
    anchors on the diagonal of anchor 0 whose only predecessor inside the band is anchor 0 itself, three to five tiles back."""
    from mm2chain import params
    P = params.map_ont()
    rng = np.random.default_rng(11)
    tasks = []
    for n_noise in (200, 270, 330):
        pos = np.concatenate(([1000], 1001 + np.arange(n_noise) * 9, 4100 + np.arange(20) * 2000))
        q = np.concatenate(([100], 60000 - np.arange(n_noise) * 170, 3200 + np.arange(20) * 2000))        # noise: q falls while x rises, no pair passes (and the q values stay within the compact ring's span)
        tasks.append(task_of(pos, q, np.full(pos.shape[0], 15)))
    a, off = batch(tasks)
    _, p_ref = oracle_batch(P, off, a)
    for k, n_noise in enumerate((200, 270, 330)):
        t = p_ref[off[k]:off[k + 1]]
        assert (t[1:1 + n_noise] == -1).all() and t[1 + n_noise] == 0, t[:n_noise + 3]
    run_both(P, tasks, knobs, "p = -1 and p = 0")


def test_device_cut_pieces_inherit_the_form(knobs):
    """Tasks of at least 8192 anchors with an empty window in the middle are cut into pieces on the device (pbase != 0 for the second piece); the pieces carry their
    task's class.  One task of exactly 8192 anchors (fits the word) and one of 10 000 (does not), with short tasks of both kinds, in one batch."""
    from mm2chain import params, synth
    P = params.map_ont()
    rng = np.random.default_rng(5)
    tasks = []
    for n in (PK_MAX_N, 10000):
        k = np.arange(n)
        pos = 1000 + 20 * k + np.where(k >= n // 2 + 7, 50000, 0)            # x jumps by more than max_dist_x: an empty window
        q = np.where(rng.random(n) < 0.85, 60 + 20 * k, 60 + 20 * k + rng.integers(600, 2500, n))
        tasks.append(task_of(pos, q, np.full(n, 15)))
    tasks.append(synth.make_stream("mixed", 1, 700, seed=6)[1].numpy().view(np.uint64))
    tasks.append(chain_with_noise(rng, 600, 64, span=255))                       # span sum 153 000: a short task that does not fit
    a, off = batch(tasks)
    _, p_ref = oracle_batch(P, off, a)
    assert p_ref[off[0] + PK_MAX_N // 2 + 7] == -1 and p_ref[off[0] + PK_MAX_N - 1] > PK_MAX_N // 2   # second piece: p relative to the task, beyond its first half
    mixed = [tasks[0], tasks[2], tasks[3]]                                   # the cut task that fits, a short one that fits, a short one that does not: one plan, both forms
    cls = run_both(P, mixed, knobs, "device-cut pieces, tasks of both kinds")
    assert [bool(c & 8) for c in cls] == [True, True, False]
    cls = run_both(P, tasks, knobs, "device-cut pieces, with a task too long for the word")
    assert not (cls & 8).any()


def _gaining_colinear_task(rng, n, span):
    """the recipe of helpers.steep_colinear_task (one colinear chain, every anchor's best predecessor its neighbour, x and q of a link apart by a jitter of 200 .. 420,
    within bw = 500) with the jitter always on the side of x: q advances 5 .. 25 per link, so the q values of 2000 anchors span less than the compact ring allows, while
    the gap cost of a link is (int)(dd * avg) + log2(dd) / 2 with dd = 200 .. 420"""
    dq = rng.integers(5, 26, n)
    dd = rng.integers(200, 421, n)
    return task_of((1 << 20) + np.cumsum(dq + dd), 100 + np.cumsum(dq), np.full(n, span))


@pytest.mark.parametrize("coop_plans", [0, 2])
@pytest.mark.parametrize("gap_scale,span", [(-15.0, 15), (-0.5, 60)])
def test_a_gap_cost_that_is_a_gain_takes_f_beyond_the_span_sum(gap_scale, span, coop_plans, knobs):
    """gap_scale < 0 (the table forms admit -20 < gap_scale < 20): every link of a colinear chain with jitter GAINS |gap_scale| * ((int)(dd * avg) + log2(dd) / 2), so
    f passes the sum of the spans -- the bound by which the prepass says a task fits the packed word.  Three tasks of 300, 700 and 2000 anchors with compact q and span
    sums of at most 120 000, so nothing else keeps them from the packed ring.  gap_scale -15, span 15: about 750 a link, every task's f passes 2^17 + 14.  gap_scale
    -0.5: f of the 300-anchor task stays below 2^17 and that of the 2000-anchor task passes it (with span 60: at span 15 and bw 500 a link gains at most
    0.5 * (75 + 4) + 15 = 55, and 2000 links stay below 2^17 whatever the anchors).  Equal to the oracle with the knob on and off, one wave per piece and by the
    library's own route; the plan runs without the packed ring and says so."""
    from mm2chain import params
    from reuse_data import expected_class_bits
    P = params.make_params(gap_scale=gap_scale, bw=500)
    rng = np.random.default_rng(1517)
    tasks = [_gaining_colinear_task(rng, n, span) for n in (300, 700, 2000)]
    assert all(span_sum(t) <= PK_MAX_F for t in tasks) and not (expected_class_bits(tasks) & 2).any()      # tasks of the compact ring, within the stated bound
    a, off = batch(tasks)
    f_ref, p_ref = oracle_batch(P, off, a)
    top = [int(f_ref[off[k]:off[k + 1]].max()) for k in range(3)]
    if gap_scale == -15.0:
        assert min(top) > PK_MAX_F + 14, top
    else:
        assert top[0] < (1 << 17) < top[2], top
    knobs("coop_plans", coop_plans)
    if coop_plans == 0:
        cls = run_both(P, tasks, knobs, f"gap_scale={gap_scale}")
        assert not (cls & 8).any()
        return
    for pk in (1, 0):                    # the library's own route
        knobs("packed_fp", pk)
        v = []
        f, p = gpu_batch(P, off, a, variant=v)
        assert_same(f, p, f_ref, p_ref, off, f"gap_scale={gap_scale}, coop_plans=2, packed_fp={pk}: {v[0]}")
        assert "packed_fp=1" not in v[0], v


def test_q_span_override_at_the_limit_of_f(knobs):
    """with q_span_override every score adds the override, whatever the anchors' own spans: the bound on f is override * n.  255 * 514 = 131 070 fits the word and
    255 * 515 = 131 325 does not; the anchors' own spans (15) would let both in.  The oracle's scalars have no override: it runs on the same anchors with span 255
    written into them, which is the same computation here -- every pair of a strictly colinear chain has dd = 0, so its gap cost is 0 whatever avg_qspan is, the one
    other place a span enters."""
    from mm2chain import params
    from reuse_data import with_spans
    P = params.make_params(q_span_override=255)
    tasks = []
    for n in (514, 515):
        k = np.arange(n)
        tasks.append(task_of(1000 + 255 * k, 100 + 255 * k, np.full(n, 15)))
    as_255 = [with_spans(t, 255) for t in tasks]
    assert 255 * 514 <= PK_MAX_F < 255 * 515 and all(span_sum(t) <= PK_MAX_F for t in tasks)
    a, off = batch(as_255)
    f_ref, _ = oracle_batch(P, off, a)
    assert int(f_ref[:off[1]].max()) == 255 * 514 and int(f_ref[off[1]:].max()) == 255 * 515      # f reaches the bound exactly
    cls = run_both(P, tasks, knobs, "q_span_override at the f bound", ref_tasks=as_255)
    assert [bool(c & 8) for c in cls] == [True, False]
