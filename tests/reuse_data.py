"""Seeded data for running ONE plan on many inputs (tests/test_gpu_plan_reuse.py), and the helpers that build it.  tests/test_cpu_plan_reuse_data.py asserts, from the
oracle alone, that consecutive sets of the run order differ in nearly every f, in p, in the class bits the prepass must find, in where the empty windows are and in
where the f / p of scored tiles come from: a run that read anything the run before left in the plan's workspace cannot then equal the oracle by luck.

One offsets array serves every set (SIZES): no task is longer than PK_MAX_N, so the plan may take the packed f / p ring; task 0 reaches plan_cut_min.
  A  compact q, spans 15, colinear chains with noise (one chain anchor every 40 / 64 / 100 anchors: scored tiles at depths 1 to 6 and beyond)
  B  A's x and q, spans redrawn in 8..40 (skewed to the low end, so that the span sum of task 0 stays below PK_MAX_F: every class bit stays)
  C  tasks 1, 2 and 6 with q values that alias mod 2^16 (respan_q modes 2 and 7: the 32-bit ring -- and they hold more than wide_share_threshold of the anchors, so
     every task takes it); tasks 0 and 7 with span 255 (span sums beyond PK_MAX_F: no packed word)
  D  an x jump beyond max_dist_x after anchor 4103 of task 0 and after anchor 2000 of task 6
  E  jumps after anchors 1500 and 6500 of task 0, none in task 6
  F  tasks 2 and 6 dense (a locus of 9000: windows beyond the ring of 16 tiles)
C to F are drawn with seeds and spans of their own, so that f and p differ from the set run before them whatever it was."""
import numpy as np

from helpers import oracle_batch, respan_q

PK_MAX_N = 8192            # csrc/chain_kernel.h
PK_MAX_F = (1 << 17) - 1   # csrc/chain_dp_tile.h
WIDE_PCT = 40              # csrc/chain_kernel.h, LaunchArgs::wide_pct
RID = np.uint64(1) << np.uint64(32)
SIZES = (8192, 700, 3000, 1, 0, 64, 6000, 4097, 257)
OFF = np.concatenate(([0], np.cumsum(SIZES))).astype(np.int64)
EVERY = (100, 40, 64, 40, 40, 64, 64, 40, 100)      # (the long tasks take the sparse chains: their q values must span less than 65535 - max_dq for the compact ring)
ORDER = "ABCDAEFBC"
JUMPS = {"D": {0: (4103,), 6: (2000,)}, "E": {0: (1500, 6500)}}


def task_of(pos, q, span):
    """uint64 [n, 2] from reference positions, query positions and spans, sorted by x (stable)"""
    x = RID | np.asarray(pos, np.int64).astype(np.uint64)
    y = (np.asarray(span, np.int64).astype(np.uint64) << np.uint64(32)) | (np.asarray(q, np.int64).astype(np.uint64) & np.uint64(0xffffffff))
    o = np.argsort(x, kind="stable")
    return np.ascontiguousarray(np.stack((x[o], y[o]), 1))


def chain_with_noise(rng, n, every, step=450, span=15, q0=100):
    """A colinear chain with one anchor every `every` positions of the array, `step` apart in x and q (about 5000 / step of them inside a window of 5000), and noise
    anchors in between whose q lies 3000-4000 off the diagonal (no pair of a chain anchor and a noise anchor passes bw = 500): the scored predecessors of a chain
    anchor sit every, 2 * every, ... anchors back, i.e. in tiles 1, 2, 3, ... before its own."""
    k = np.arange(n)
    pos = 1000 + (k * step) // every
    on = k % every == 0
    q = np.where(on, q0 + pos - 1000, q0 + pos - 1000 + 3000 + rng.integers(0, 1000, n))
    return task_of(pos, q, np.full(n, span))


def batch(tasks):
    return np.concatenate(tasks), np.concatenate(([0], np.cumsum([t.shape[0] for t in tasks]))).astype(np.int64)


def span_sum(t):
    return int(((t[:, 1] >> np.uint64(32)) & np.uint64(0xff)).sum())


def with_spans(task, span):
    t = task.copy()
    t[:, 1] = (np.broadcast_to(np.asarray(span, np.int64), (t.shape[0],)).astype(np.uint64) << np.uint64(32)) | (t[:, 1] & np.uint64(0xffffffff))
    return t


def with_x_jumps(task, after, by=50000):
    """every anchor behind anchor `after` moved up by `by` in x (more than max_dist_x: anchor after + 1 has an empty window); the order stays"""
    t = task.copy()
    for k in after:
        t[k + 1:, 0] += np.uint64(by)
    return t


def _base(seed, span):
    rng = np.random.default_rng(seed)
    return [chain_with_noise(rng, n, every, span=span) for n, every in zip(SIZES, EVERY)]


def _make(name):
    from mm2chain import synth
    if name == "A":
        return _base(1, 15)
    if name == "B":
        rng = np.random.default_rng(2)
        return [with_spans(t, np.where(rng.random(t.shape[0]) < 0.85, rng.integers(8, 14, t.shape[0]), rng.integers(16, 41, t.shape[0]))) for t in get("A")]
    if name == "C":
        tasks, rng = _base(3, 14), np.random.default_rng(33)
        for k, mode in ((1, 2), (2, 7), (6, 2)):
            tasks[k] = respan_q(rng, tasks[k], 5000, mode)
        for k in (0, 7):
            tasks[k] = with_spans(tasks[k], 255)
        return tasks
    if name in JUMPS:
        tasks = _base(4 if name == "D" else 5, 13 if name == "D" else 12)
        for k, after in JUMPS[name].items():
            tasks[k] = with_x_jumps(tasks[k], after)
        return tasks
    assert name == "F"
    tasks = _base(6, 7)
    for k, seed in ((2, 61), (6, 62)):
        tasks[k] = synth.make_stream("dense", 1, SIZES[k], seed=seed, locus=9000)[1].numpy().view(np.uint64)
    return tasks


_SETS, _REFS = {}, {}


def get(name):
    """the tasks of a set (list of uint64 [n, 2]), built once per process"""
    if name not in _SETS:
        tasks = _make(name)
        assert tuple(t.shape[0] for t in tasks) == SIZES, name
        _SETS[name] = tasks
    return _SETS[name]


def scalars():
    from mm2chain import params as pm
    return pm.map_ont()


def anchors(name):
    return batch(get(name))[0]


def reference(name):
    """(f, p) of the oracle for a set with the map-ont scalars, computed once per process and handed out read-only"""
    if name not in _REFS:
        f, p = oracle_batch(scalars(), OFF, anchors(name))
        f.setflags(write=False); p.setflags(write=False)
        _REFS[name] = (f, p)
    return _REFS[name]


def expected_class_bits(tasks, max_dq=5000, packed=True):
    """bits 1 and 3 of the class byte per task, by the rules of include/mm2chain.h and the prepass's comments (chain_window_start_t, chain_cls_settle): bit 1, the task's q
    values span more than 65535 - max_dq, or such tasks hold more than wide_share_threshold % of the plan's anchors (then every task carries it); bit 3, the task has
    at most PK_MAX_N anchors and a span sum of at most PK_MAX_F, in a plan whose longest task has at most PK_MAX_N anchors"""
    n = np.array([t.shape[0] for t in tasks], np.int64)
    q = [(t[:, 1] & np.uint64(0xffffffff)).astype(np.int64) for t in tasks]
    wide = np.array([t.size > 0 and int(t.max() - t.min()) > 65535 - max_dq for t in q])
    if 100 * int(n[wide].sum()) > WIDE_PCT * int(n.sum()):
        wide[:] = True
    plan_packed = packed and int(n.max()) <= PK_MAX_N
    fits = np.array([plan_packed and 0 < t.shape[0] <= PK_MAX_N and span_sum(t) <= PK_MAX_F for t in tasks])
    return (np.where(wide, 2, 0) | np.where(fits, 8, 0)).astype(np.uint8)


def empty_windows(task, max_dist_x=5000):
    """the anchors i > 0 whose window is empty: x[i] - x[i - 1] > max_dist_x (chain.c:192)"""
    x = task[:, 0]
    return 1 + np.nonzero(x[1:] > x[:-1] + np.uint64(max_dist_x))[0]
