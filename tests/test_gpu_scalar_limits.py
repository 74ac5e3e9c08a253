"""The DP kernels at the SCALAR limits of their compact forms: max_dist_x at 65535 / 65536 and max_dq at 32768 / 32769 (the compact x / q ring and the q24 long ring keep 16
bits of x), the one-word push key of the eight-wave cooperative kernel at n = 2^15, spans of 255 / 256, gap_scale 4 / 4.5 and bw 2^17, the gap-cost table at bw 511 / 512
and |gap_scale| 20, the splice and sr presets, and the prediction pass.  The inputs are tests/limit_data.py's; tests/test_cpu_limit_data.py shows from the oracle alone
that each reaches the limit it names.  Everything is compared element for element with the CPU oracle, and the variant text says which form ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import limit_data as ld
import oracle_binding as ob
from helpers import assert_same, gpu_batch, knobs, oracle_batch  # noqa: F401 (knobs: a fixture)
from reuse_data import batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


_CASES = {}


def case(name, *args):
    """(P, tasks, anchors, offsets, f_ref, p_ref) of one builder call: built and run through the oracle once per process, handed out read-only"""
    key = (name,) + args
    if key not in _CASES:
        P, tasks = getattr(ld, name)(*args)[:2]
        a, off = batch(tasks)
        f, p = oracle_batch(P, off, a)
        for arr in (a, off, f, p):
            arr.setflags(write=False)
        _CASES[key] = (P, tasks, a, off, f, p)
    return _CASES[key]


def class_bytes(P, off, a, f_ref, p_ref, what):
    """the class bytes of one more run, one wave per piece (the caller has pinned coop_plans 0)"""
    import mm2chain
    d_a = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 2)).cuda()
    d_f = torch.empty(a.shape[0], dtype=torch.int32, device="cuda"); d_p = torch.empty_like(d_f)
    plan = mm2chain.ChainPlan(P, off)
    plan.run(d_a, d_f, d_p)
    torch.cuda.synchronize()
    cls = np.frombuffer(plan.last_classes(), np.uint8).copy()
    plan.close()
    assert_same(d_f.cpu().numpy(), d_p.cpu().numpy(), f_ref, p_ref, off, f"{what}, class read-back run")
    return cls


# ---- (a) max_dist_x at the last value of the 16-bit forms and beyond
@pytest.mark.parametrize("route", ["packed", "pairs", "long-ring-q24", "long-ring-32-bit", "several-waves"])
@pytest.mark.parametrize("far", [False, True], ids=["ring", "far"])
@pytest.mark.parametrize("D", [65534, 65535, 65536, 65537])
def test_max_dist_x_at_the_limit_of_the_sixteen_bit_rings(D, far, route, knobs):
    """Links of dr = max_dist_x - 1, max_dist_x and one more (and of the band's own edge, dr = 65535, for 65536 and 65537), dq = 32767, 32768, 32769, with the
    candidate inside the ring of 16 tiles or 1 100 .. 3 000 anchors back.  The tasks that hold such a link have wide q values (32-bit ring; with far_ring 2 the long
    ring in its q24 form, which keeps 16 bits of x: there dr = 65535 is a full-range difference); four tasks take the compact ring with the longest link their q span
    allows.  compact=1 and q24=1 up to 65535, neither beyond."""
    P, tasks, a, off, f_ref, p_ref = case("x_limit_far" if far else "x_limit", D, 32768)
    ok16 = D <= 65535
    knobs("wide_share_threshold", 100)                       # the split between compact and 32-bit tasks always stands
    if route == "pairs": knobs("packed_fp", 0)
    if route.startswith("long-ring"): knobs("far_ring", 2); knobs("q24_ring", int(route == "long-ring-q24"))
    if route == "several-waves": knobs("coop_plans", 1)
    v = []
    f, p = gpu_batch(P, off, a, variant=v)
    assert_same(f, p, f_ref, p_ref, off, f"max_dist_x={D}, {route}: {v[0]}")
    if route == "several-waves":
        assert v[0].startswith("chain_dp_coop<W=16,") and "loop=asm" in v[0] and "TAB=0" in v[0], v
        return
    assert v[0].startswith("chain_dp_tile<") and "loop=asm" in v[0] and "GS1=1" in v[0] and "TAB=0" in v[0] and "FAR=1" in v[0], v
    assert f"compact={int(ok16)}" in v[0] and f"packed_fp={int(ok16 and route != 'pairs')}" in v[0], v
    if route.startswith("long-ring"):
        assert "classes=1" in v[0] and f"q24={int(ok16 and route == 'long-ring-q24')}" in v[0], v
    if route == "packed" and not far:
        knobs("coop_plans", 0)
        cls = class_bytes(P, off, a, f_ref, p_ref, f"max_dist_x={D}")
        if ok16:
            assert (cls[:16] & 2).all() and not (cls[16:] & 2).any() and (cls[16:] & 8).all(), cls   # the limit links' tasks: 32-bit ring; the last four: compact, packed


# ---- (b) max_dq at 32768
@pytest.mark.parametrize("dq_max,compact", [(32767, 1), (32768, 1), (32769, 0)])
def test_max_dq_at_the_limit_of_the_compact_ring(dq_max, compact, knobs):
    """max_dist_x = 65535 with max_dist_y = 32767, 32768 (the last max_dq the compact ring takes: its bound on a task's q span is then 32767) and 32769"""
    P, tasks, a, off, f_ref, p_ref = case("x_limit", 65535, dq_max)
    knobs("wide_share_threshold", 100)
    for far_ring in (1, 2):
        knobs("far_ring", far_ring)
        v = []
        f, p = gpu_batch(P, off, a, variant=v)
        assert_same(f, p, f_ref, p_ref, off, f"max_dq={dq_max}, far_ring={far_ring}: {v[0]}")
        assert f"compact={compact}" in v[0] and "loop=asm" in v[0] and "q24=1" in v[0], v
    knobs("far_ring", 1); knobs("coop_plans", 0)
    cls = class_bytes(P, off, a, f_ref, p_ref, f"max_dq={dq_max}")
    if compact:
        assert (cls[:16] & 2).all() and not (cls[16:] & 2).any(), cls


@pytest.mark.parametrize("dq_max", [32767, 32768])
def test_q_spans_at_the_bound_of_the_largest_max_dq(dq_max, knobs):
    """q spans of exactly 65535 - max_dq and one more, and differences that alias mod 2^16, under the largest max_dq the compact ring admits: bit 1 of the class byte
    (the 32-bit ring) clear for the tasks as drawn and at the bound, set one past it and for the aliasing ones"""
    P, tasks, modes = ld.q_span_at_scalar_limit(dq_max)
    a, off = batch(tasks)
    f_ref, p_ref = oracle_batch(P, off, a)
    knobs("wide_share_threshold", 100)
    v = []
    f, p = gpu_batch(P, off, a, variant=v)
    assert_same(f, p, f_ref, p_ref, off, f"q span at max_dq={dq_max}: {v[0]}")
    assert "compact=1" in v[0] and "loop=asm" in v[0], v
    knobs("coop_plans", 0)
    cls = class_bytes(P, off, a, f_ref, p_ref, f"q span at max_dq={dq_max}")
    assert [bool(c & 2) for c in cls] == [m in (4, 2) for m in modes], (cls, modes)


# ---- (c) the one-word push key of the eight-wave cooperative kernel
@pytest.mark.parametrize("width", [8, 16, 1])
@pytest.mark.parametrize("kind", ["n", "span", "gap_scale", "bw"])
def test_one_word_push_key_at_its_guards(kind, width, knobs):
    """Tasks of 32 767 / 32 768 anchors of span 255 (f up to 8 355 585 / 8 355 840), q_span_override 255 / 256 (f up to 8 388 352), gap_scale 4 / 4.5 and bw 131 072 /
    131 073 with links at the band's edge: the eight-wave kernel pushes score << 7 | origin in one word on the near side of each guard and (score, origin) in two on
    the far side; sixteen waves take the two-sweep form, one wave the tile kernel.  max_skip = INT32_MAX: whole tiles are eligible and take the straight-line pushes."""
    knobs("coop_plans", 1 if width > 1 else 0)
    if width == 8: knobs("coop_w8_above", 0)
    for P, tasks in ld.key32_limit(kind):
        a, off = batch(tasks)
        f_ref, p_ref = ld.reference(P, tasks)
        v = []
        f, p = gpu_batch(P, off, a, variant=v)
        what = f"{kind}: n={a.shape[0]}, q_span_override={P.q_span_override}, gap_scale={P.gap_scale}, bw={P.bw}, width {width}: {v[0]}"
        assert_same(f, p, f_ref, p_ref, off, what)
        if width > 1:
            assert v[0].startswith(f"chain_dp_coop<W={width},") and "loop=asm" in v[0] and f"TAB={int(P.gap_scale != 1.0)}" in v[0], v
        else:
            assert v[0].startswith("chain_dp_tile<") and "loop=asm" in v[0], v


# ---- (d) the gap-cost table
@pytest.mark.parametrize("gap_scale", ld.TABLE_GS)
@pytest.mark.parametrize("bw", ld.TABLE_BW)
def test_gap_cost_table_at_its_last_entry_and_largest_scale(bw, gap_scale, knobs):
    """bw 511 (the table's last entry is read: links of |dr - dq| = 511) and 512, gap_scale just inside and at +-20: TAB=1 exactly for bw <= 511 and
    -20 < gap_scale < 20; a negative gap_scale runs without the packed f / p ring and says so"""
    P, tasks = [c for c in ld.table_limit() if c[0].bw == bw and np.float32(c[0].gap_scale) == np.float32(gap_scale)][0]
    a, off = batch(tasks)
    f_ref, p_ref = oracle_batch(P, off, a)
    knobs("packed_fp", 1)
    v = []
    f, p = gpu_batch(P, off, a, variant=v)
    assert_same(f, p, f_ref, p_ref, off, f"bw={bw}, gap_scale={gap_scale}: {v[0]}")
    tab = bw <= 511 and -20 < gap_scale < 20 and gap_scale != 1
    assert f"TAB={int(tab)}" in v[0] and ("loop=asm" in v[0]) == tab, v
    assert f"packed_fp={int(tab and gap_scale >= 0)}" in v[0], v
    if gap_scale < 0:
        assert "packed_fp=0" in v[0], v


# ---- (e) presets
@pytest.fixture(params=[3, 4], ids=["general-in-wave-kernel", "general-in-tile-kernel"])
def general_kernel(request):
    import mm2chain
    with mm2chain.tuned(ring_class=request.param):
        yield request.param


@pytest.mark.parametrize("preset", ["splice", "sr"])
def test_splice_and_sr_presets(preset, general_kernel):
    """-x splice (is_cdna, reference gap and bw of 200 000: introns of 10^3 .. 200 000 are bridged, 200 001 is not) and -x sr (two segments, gaps of 500 / 300)"""
    P, tasks = ld.splice_tasks() if preset == "splice" else ld.sr_tasks()
    a, off = batch(tasks)
    f_ref, p_ref = oracle_batch(P, off, a)
    v = []
    f, p = gpu_batch(P, off, a, variant=v)
    assert_same(f, p, f_ref, p_ref, off, f"{preset}: {v[0]}")
    assert "GEN=1" in v[0] and v[0].startswith("chain_dp_tile<" if general_kernel == 4 else "chain_dp_wave<"), v


# ---- (f) the prediction pass
def _predict(plan, d_a, want):
    """mm2c_plan_predict_device with the outputs named in `want` (a subset of "ns", "ts", "tt") and NULL for the others; returns what was written, and checks that
    nothing else was"""
    bufs = {"ns": torch.full((max(plan.total, 1),), 0xAB, dtype=torch.uint8, device="cuda"),
            "ts": torch.full((max(plan.n_tasks, 1),), -77, dtype=torch.int64, device="cuda"),
            "tt": torch.full((max(plan.n_tasks, 1),), -77, dtype=torch.int64, device="cuda")}
    ptr = lambda k: C.c_void_p(bufs[k].data_ptr()) if k in want else None
    rc = plan.lib.mm2c_plan_predict_device(plan.handle, C.c_void_p(d_a.data_ptr()) if d_a is not None else None, ptr("ns"), ptr("ts"), ptr("tt"),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}


@pytest.mark.parametrize("max_dist_x", [0, 50, 5000, 65535, 100000])
def test_prediction_pass_windows_references_and_optional_outputs(max_dist_x):
    """chain.c:53-78 per task against the oracle's: tasks of 1 .. 3 000 anchors with several references and both strands, one task with windows of exactly 0, 1, 127,
    128, 129, 1 023, 1 024 and 1 500 anchors (1, 1, 1, 1, 2, 8, 8, 8 subparts; trip counts capped at 1 024), every subset of the three outputs"""
    import mm2chain
    from mm2chain import params
    rng = np.random.default_rng(53 + max_dist_x)
    tasks = [ld.random_task(rng, n, 3 if n >= 64 else 1, 1, bool(k % 2)) for k, n in enumerate((1, 2, 64, 65, 1025, 3000))]
    win, probes = ld.predict_window_task(D=max_dist_x)
    tasks.append(win)
    a, off = batch(tasks)
    ref = [ob.predict(t, max_dist_x) for t in tasks]
    assert list(ref[-1][0][probes]) == [1, 1, 1, 1, 2, 8, 8, 8]
    ns_ref = np.concatenate([r[0] for r in ref]); ts_ref = np.array([r[1] for r in ref]); tt_ref = np.array([r[2] for r in ref])
    d_a = torch.from_numpy(a.view(np.int64).reshape(-1, 2)).cuda()
    plan = mm2chain.ChainPlan(params.make_params(max_dist_x=max_dist_x), off)
    for want in ((), ("ns",), ("ts",), ("tt",), ("ns", "ts"), ("ns", "tt"), ("ts", "tt"), ("ns", "ts", "tt")):
        got = _predict(plan, d_a, want)
        for k, r in (("ns", ns_ref), ("ts", ts_ref), ("tt", tt_ref)):
            if k in want:
                assert np.array_equal(got[k], r), (max_dist_x, want, k, np.nonzero(got[k] != r)[0][:5])
            else:
                assert (got[k] == (0xAB if k == "ns" else -77)).all(), (max_dist_x, want, k)
    got = _predict(plan, d_a, ("ns", "tt"))
    k = len(tasks) - 1
    assert list(got["ns"][off[k] + probes]) == [1, 1, 1, 1, 2, 8, 8, 8] and int(got["tt"][k]) == tt_ref[k]
    win_x = win[:, 0].astype(np.int64)
    trips = [min(int((win_x[:i] >= win_x[i] - max_dist_x).sum()), 1024) for i in probes]
    assert trips == [0, 1, 127, 128, 129, 1023, 1024, 1024]
    plan.close()
    empty = mm2chain.ChainPlan(params.make_params(max_dist_x=max_dist_x), np.zeros(1, np.int64))      # a plan without tasks: nothing is launched, nothing written
    got = _predict(empty, None, ("ns", "ts", "tt"))
    assert (got["ns"] == 0xAB).all() and (got["ts"] == -77).all() and (got["tt"] == -77).all()
    empty.close()
