"""Seeded inputs that put the SCALARS of a call at the limits of the DP kernels' compact forms (tests/test_gpu_scalar_limits.py runs them; tests/test_cpu_limit_data.py
asserts, from the oracle alone, that each one reaches the limit it names).  Every builder returns (P, [tasks]) or, where the scalars themselves are what varies, a list
of such pairs.

  form                                   guard                                                            builder
  compact x / q ring (low 16 bits)       0 <= max_dist_x <= 65535, 1 <= max_dq <= 32768                    x_limit, x_limit_far, q_span_at_scalar_limit
  q24 long ring (16 bits of x)           max_dist_x <= 65535                                              x_limit, x_limit_far
  one-word push key score << 7 | origin  n < 2^15, q_span_override <= 255, 0 <= gap_scale <= 4, bw <= 2^17  key32_limit
  gap-cost table (int16, 512 entries)    0 <= bw <= 511, -20 < gap_scale < 20                             table_limit

What the band allows.  A link passes chain.c:203-205 with dq <= max_dq and |dr - dq| <= bw, so dr <= max_dq + bw; the hand-written loop runs with bw <= max_dq - 1, and
x_limit takes bw = max_dq - 1: the widest band that loop serves.  With dq_max = 32768 the longest link that can ever win has dr = 65535, whatever max_dist_x is; for
max_dist_x = 65536 and 65537 that link (BAND_EDGE) is the limit link, and none at dr == max_dist_x exists.  A task that holds a link of dq = dq_max has q values that
span more than 65535 - dq_max, so the prepass gives it the 32-bit ring (or the q24 ring): in the compact ring the q span bounds dr by (65535 - max_dq) + bw <= 65534.
The `compact` tasks of x_limit hold the longest link that fits a compact task (its dr needs bit 15 of the 16-bit difference)."""
import numpy as np

from helpers import respan_q
from reuse_data import task_of, with_spans

INT32_MAX = 2**31 - 1
SPAN = 15
AVG15 = float(np.float32(.01 * float(np.float32(15.0))))        # avg_qspan_scaled of a task whose spans are all 15 (chain.c:48-49)
BAND_EDGE = "band-edge"


def gap_cost(dd, avg):
    """chain.c:209,218 for one link, gap_scale 1: (int)(dd * avg) + (log2(dd) >> 1)"""
    return int(np.float32(dd) * np.float32(avg)) + ((int(dd).bit_length() - 1) >> 1 if dd else 0)


def _cluster(rng, n, x0, q0, lo=5, hi=20):
    """n colinear anchors from (x0, q0): the same steps of lo..hi in x and q (no gap cost inside a cluster; a link gains min(step, span))"""
    s = np.concatenate(([0], np.cumsum(rng.integers(lo, hi + 1, n - 1))))
    return x0 + s, q0 + s


def limit_kinds(D, dq_max):
    """(dr, dq) of the nine limit links and of the band-edge link"""
    kinds = [(dr, dq) for dr in (D - 1, D, D + 1) for dq in (dq_max - 1, dq_max, dq_max + 1)]
    bw = min(D, dq_max) - 1
    return kinds + [(min(D, dq_max + bw), dq_max)]


def _limit_task(rng, links, between, cluster_n=(520, 600)):
    """Clusters joined by the links (dr, dq) between the last anchor of one and the first of the next; `between` = (lo, hi): so many stepping anchors with x
    spread evenly inside the link and q 40 000 or 80 000 BELOW the cluster before it, falling: no pair with a stepping anchor passes chain.c:202-203 except, among
    two groups, pairs that score far below the span -- they hold the window together (no empty window: nothing is cut there) and lie between p[i] and i."""
    xs, qs, ends = [], [], []
    x0, q0 = 1 << 20, 400000
    for g in range(len(links) + 1):
        x, q = _cluster(rng, int(rng.integers(cluster_n[0], cluster_n[1] + 1)), x0, q0)
        xs.append(x); qs.append(q)
        if g == len(links):
            break
        dr, dq = links[g]
        k = int(rng.integers(between[0], between[1] + 1))
        j = np.arange(k)
        xs.append(int(x[-1]) + (j + 1) * dr // (k + 1))
        qs.append(int(q[0]) - 40000 * (1 + g % 2) - j)
        x0, q0 = int(x[-1]) + dr, int(q[-1]) + dq
    x, q = np.concatenate(xs), np.concatenate(qs)
    assert q.min() > 0 and q.max() < (1 << 24) and x.max() < (1 << 31)
    return task_of(x, q, np.full(x.shape[0], SPAN))


def _compact_task(rng, D, dq_max):
    """The longest link a task of the compact ring can hold: two clusters whose q values together span exactly 65535 - dq_max, joined by a link of dd == bw."""
    bw = min(D, dq_max) - 1
    bound = 65535 - dq_max
    xa, qa = _cluster(rng, int(rng.integers(520, 601)), 1 << 20, 1000)
    xb, qb = _cluster(rng, int(rng.integers(300, 401)), 0, 0)
    dq = bound - int(qa[-1] - qa[0]) - int(qb[-1])
    dr = min(dq + bw, D)
    k = int(rng.integers(20, 201))
    j = np.arange(k)
    xs = int(xa[-1]) + (j + 1) * dr // (k + 1)
    qs = int(qa[0]) + (j * 7) % 64                    # stepping anchors at the low end of the q range (no pair with them gains)
    x = np.concatenate((xa, xs, int(xa[-1]) + dr + xb))
    q = np.concatenate((qa, qs, int(qa[-1]) + dq + qb))
    assert int(q.max() - q.min()) == bound
    return task_of(x, q, np.full(x.shape[0], SPAN))


def _x_limit(D, dq_max, between, links_per_task, reps, max_iter, seed):
    from mm2chain import params
    rng = np.random.default_rng(seed)
    P = params.make_params(max_dist_x=D, max_dist_y=dq_max, bw=min(D, dq_max) - 1, gap_scale=1.0, max_iter=max_iter)
    kinds = limit_kinds(D, dq_max)
    tasks = []
    for _ in range(reps):
        order = [kinds[k] for k in rng.permutation(len(kinds))]
        while len(order) % links_per_task:
            order.append(kinds[int(rng.integers(0, len(kinds)))])
        for k in range(0, len(order), links_per_task):
            tasks.append(_limit_task(rng, order[k:k + links_per_task], between))
    return P, tasks, rng


def x_limit(D, dq_max):
    """Limit links with 20 .. 200 anchors inside them: the candidate sits within the ring of 16 tiles.  Four tasks of three links per round, four rounds (every kind
    at least four times), then four tasks for the compact ring."""
    P, tasks, rng = _x_limit(D, dq_max, (20, 200), 3, 4, 5000, 65535 + D % 7)
    if 1 <= dq_max <= 65000:
        tasks += [_compact_task(rng, D, dq_max) for _ in range(4)]
    return P, tasks


def x_limit_far(D, dq_max=32768):
    """The same links with 1 100 .. 3 000 anchors inside them: the candidate is beyond the ring (the far fetch; with far_ring 2 the long ring)."""
    P, tasks, _ = _x_limit(D, dq_max, (1100, 3000), 2, 4, 5000, 70000 + D % 7)
    return P, tasks


def required_f(P, dr, dq):
    """what f of the anchor before a link must exceed for the link to beat the span alone (chain.c:207-220, spans 15, gap_scale 1)"""
    return gap_cost(abs(dr - dq), AVG15) + SPAN - min(dr, dq, SPAN)


def q_span_at_scalar_limit(dq_max):
    """respan_q modes 0 (as drawn: compact), 3 (span exactly 65535 - dq_max), 4 (one more) and 2 (aliases mod 2^16) of three streams whose q values span 25 535; returns
    (P, tasks, modes)"""
    from mm2chain import params, synth
    rng = np.random.default_rng(3000 + dq_max)
    P = params.make_params(max_dist_x=65535, max_dist_y=dq_max, bw=500)
    tasks, modes = [], []
    for k, (prof, n) in enumerate((("mixed", 3000), ("colinear", 2500), ("dense", 1500))):
        base = synth.make_stream(prof, 1, n, seed=3100 + k)[1].numpy().view(np.uint64)
        base = respan_q(rng, base, 40000, 3)                # (q values clamped to a span of 25 535: compact under either max_dq)
        for mode in (0, 3, 4, 2):
            tasks.append(respan_q(rng, base, dq_max, mode)); modes.append(mode)
    return P, tasks, modes


def q_span(t):
    q = (t[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
    return int(q.max() - q.min())


# ---- the one-word push key of the cooperative kernel
KEY_N = 32767


def _colinear255(rng, n, jitter_share=0.0, jitter_hi=4, lo=255, hi=300, noise=0):
    """one chain of span 255 whose links advance 255 .. 300 in x and q (each gains the whole span); a share of the links is off the diagonal by 1 .. jitter_hi;
    `noise` anchors lie 5 000 off it in q (outside any band used here: the chain passes them by, its anchor behind one takes the anchor before it)"""
    step = rng.integers(lo, hi + 1, n)
    jit = np.where(rng.random(n) < jitter_share, rng.integers(1, jitter_hi + 1, n), 0)
    x = (1 << 20) + np.cumsum(step + jit)
    q = 1000 + np.cumsum(step)
    if noise:
        q[rng.choice(np.arange(100, n - 100), noise, replace=False)] += 5000
    return task_of(x, q, np.full(n, 255))


def _bw_task(rng, n, bw):
    """clusters of about 3 000 anchors of span 255 (f of a cluster's end: 765 000) joined by links with dr - dq = bw - 64 .. bw + 1: the gap cost of such a link is
    (int)(2.55 * 131 072) + 8 = 334 241, which the cluster before it outweighs"""
    step = rng.integers(255, 301, n)
    extra = np.zeros(n, np.int64)
    heads = np.arange(3000, n - 500, 3000)
    dd = np.concatenate(([bw, bw - 64, bw - 1, bw + 1], bw - rng.integers(0, 65, max(len(heads) - 4, 0))))[:len(heads)]
    extra[heads] = dd
    x = (1 << 20) + np.cumsum(step + extra)
    q = 1000 + np.cumsum(step)
    return task_of(x, q, np.full(n, 255)), heads, dd


def key32_limit(kind):
    """list of (P, [tasks]).  max_skip = INT32_MAX, max_iter = 5000: no anchor fails the rank test, whole tiles are eligible and take the straight-line pushes."""
    from mm2chain import params
    rng = np.random.default_rng({"n": 1, "span": 2, "gap_scale": 3, "bw": 4}[kind] + 32000)
    kw = dict(max_skip=INT32_MAX, max_iter=5000)
    if kind == "n":
        P = params.make_params(max_dist_x=20000, max_dist_y=20000, bw=500, **kw)
        return [(P, [_colinear255(rng, KEY_N, 0.01, noise=48)]), (P, [_colinear255(rng, KEY_N + 1, 0.01, noise=48)])]
    if kind == "span":
        # (strictly colinear in steps of 256 .. 300: no gap cost, every link gains the override itself; the anchors' own spans say 255)
        t = _colinear255(rng, KEY_N, lo=256)
        return [(params.make_params(max_dist_x=20000, max_dist_y=20000, bw=500, q_span_override=s, **kw), [t]) for s in (255, 256)]
    if kind == "gap_scale":
        t = _colinear255(rng, KEY_N, 0.008, 500, noise=48)
        return [(params.make_params(max_dist_x=20000, max_dist_y=20000, bw=500, gap_scale=g, **kw), [t]) for g in (4.0, 4.5)]
    assert kind == "bw"
    out = []
    for bw in (131072, 131073):
        t, _, _ = _bw_task(rng, KEY_N, bw)
        out.append((params.make_params(max_dist_x=200000, max_dist_y=200000, bw=bw, **kw), [t]))
    return out


def reference(P, tasks):
    """f, p of the oracle over the tasks of one case.  The oracle's scalars have no q_span_override: up to 255 it runs on the same anchors with that span written
    into them; beyond (the 8-bit field of the anchor cannot say it) the literal emulation of the reference's device kernel takes the span as a scalar -- the same
    computation for these tasks (windows below its look-back of 1 024, no max_skip in either)."""
    import oracle_binding as ob
    from helpers import oracle_batch
    from reuse_data import batch
    a, off = batch(tasks)
    if P.q_span_override > 255:
        assert P.max_skip == INT32_MAX and P.gap_scale == 1.0
        fs, ps = zip(*(ob.chain_hw_literal(P.max_dist_x, P.max_dist_y, P.bw, P.q_span_override, .01 * P.q_span_override, t) for t in tasks))
        return np.concatenate(fs), np.concatenate(ps)
    if P.q_span_override >= 0:
        a = with_spans(a, P.q_span_override)
    return oracle_batch(P, off, a)


# ---- the gap-cost table
TABLE_BW = (511, 512)
TABLE_GS = (0.8, 19.5, -19.5, 20.0, -20.0)


def _table_task(rng, n=3000, every=200):
    """clusters of `every` colinear anchors (span 15, steps 15 .. 25: f grows by 15 an anchor, 3 000 per cluster) joined by links with dr - dq = 509 .. 512: at
    gap_scale 20 such a link costs 20 * ((int)(511 * .15) + 4) = 1 600"""
    step = rng.integers(15, 26, n)
    extra = np.zeros(n, np.int64)
    heads = np.arange(every, n, every)
    extra[heads] = 509 + np.arange(len(heads)) % 4
    return task_of((1 << 20) + np.cumsum(step + extra), 1000 + np.cumsum(step), np.full(n, SPAN))


def table_tasks():
    from mm2chain import synth
    rng = np.random.default_rng(511)
    tasks = [synth.make_stream("mixed", 1, n, seed=5110 + k)[1].numpy().view(np.uint64) for k, n in enumerate((200, 3000, 777, 1500, 2048, 449))]
    return tasks + [_table_task(rng)]


def table_limit():
    """list of (P, [tasks]): bw 511 and 512 with each gap_scale, over six mixed tasks and one whose links have |dr - dq| of 509 .. 512"""
    from mm2chain import params
    tasks = table_tasks()
    return [(params.make_params(bw=bw, gap_scale=gs), tasks) for bw in TABLE_BW for gs in TABLE_GS]


# ---- presets
def splice_tasks():
    """one task per intron length: exons of 60 .. 200 colinear anchors joined by a jump in x alone (dq stays a step) of 10^3, 10^4, 10^5, max_dist_x and
    max_dist_x + 1"""
    from mm2chain import params
    P = params.splice()
    rng = np.random.default_rng(200000)
    tasks = []
    for intron in (1000, 10000, 100000, P.max_dist_x, P.max_dist_x + 1):
        xs, qs = [], []
        x0, q0 = 1 << 20, 500
        for _ in range(5):
            x, q = _cluster(rng, int(rng.integers(60, 201)), x0, q0, 5, 35)
            q = q + rng.integers(-2, 3, q.shape[0])
            xs.append(x); qs.append(q)
            x0, q0 = int(x[-1]) + intron, int(q.max()) + int(rng.integers(5, 36))
        tasks.append(task_of(np.concatenate(xs), np.concatenate(qs), np.full(sum(x.shape[0] for x in xs), SPAN)))
    return P, tasks


def sr_tasks(n_tasks=24):
    """two-segment tasks of 10 .. 200 anchors (the shape of tests/test_gpu_parity.py's _multiseg_task: dr == 0 between segments included)"""
    from helpers import mk_anchor, pack
    from mm2chain import params
    rng = np.random.default_rng(2150)
    tasks = []
    for _ in range(n_tasks):
        rows, pos, q = [], 1 << 20, 100
        for _ in range(int(rng.integers(10, 201))):
            pos += int(rng.integers(0, 40)); q += int(rng.integers(-30, 60))
            rows.append(mk_anchor(0, 3, pos, max(q, 1), span=21, seg=int(rng.integers(0, 2))))
        tasks.append(pack(rows))
    return params.sr(), tasks


# ---- the prediction pass
def random_task(rng, n, n_refs, n_segs, dense):
    """adversarial anchors in the shape of tests/test_gpu_parity.py's _random_task: several references and both strands in one task, duplicated x, huge jumps"""
    from helpers import mk_anchor, pack
    rows = []
    for r in range(n_refs):
        strand, rid = int(rng.integers(0, 2)), int(rng.integers(0, 5))
        pos = int(rng.integers(0, 1 << 20)); q = int(rng.integers(0, 5000))
        for _ in range(n // n_refs + (n % n_refs if r == 0 else 0)):
            u = rng.random()
            pos += 0 if u < .08 else int(rng.integers(1, 12 if dense else 400)) if u < .95 else int(rng.integers(3000, 30000))
            q += int(rng.integers(-40, 60 if dense else 300))
            rows.append(mk_anchor(strand, rid, pos, max(q, 0), span=int(rng.integers(1, 40)), seg=int(rng.integers(0, n_segs))))
    return pack(rows)


def predict_window_task(windows=(0, 1, 127, 128, 129, 1023, 1024, 1500), D=5000):
    """One anchor per entry of `windows` whose window (the anchors before it within D in x, chain.c:62-66) holds exactly that many anchors: a block of w anchors with
    one x, then the probe D above it, then a gap of more than D.  Returns the task and the probes' indices."""
    xs, probes = [], []
    x0 = 1 << 20
    for w in windows:
        xs += [x0] * w
        probes.append(len(xs))
        xs.append(x0 + D)
        x0 += 3 * D + 7
    x = np.array(xs, np.int64)
    return task_of(x, 100 + np.arange(x.shape[0]) % 5000, np.full(x.shape[0], SPAN)), np.array(probes)
