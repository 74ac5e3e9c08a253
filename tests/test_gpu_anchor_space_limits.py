"""mapq_gather (csrc/chain_mapq.hip) and err_walk (csrc/chain_esterr.hip) at the limits of their traversal of the batch's b index space: every batch layout of
tests/anchor_space_limit_data.py through MapqPlan.run with anchors and, on the same stream, its outputs through EstErrPlan.run.  Regions, n_out, n_b_out, a[],
(n_match, n_tot) and avg_k equal the reference record (tests/golden/ref_mapq_limits.npz, ref_esterr_limits.npz) byte for byte, div included once the host's pow is
applied, and every row and anchor the record does not own still holds the fill: each read's tail from n_b_out on, the space in front of b_off[0], the guards.
Each layout runs on plans of exactly its size and through the host entries; then all of them on one pair of plans, in two orders, each behind other data; the
second-turn layout with its first anchor at 8 388 608 - 6 000 on plans of 8 388 608 + 16 384 anchors, filled and checked on the device; and the eight-read layout
on three workgroups behind each of two refusals, where both kernels go read by read."""
import numpy as np
import pytest
import torch

import anchor_space_limit_data as D
import esterr_model as EM
from mapq_data import MAPQ_DEFAULT
from regs_model import REG

pytestmark = pytest.mark.gpu
REG_FILL, B_FILL, N_FILL, ERR_FILL, AVG_FILL, GUARD = 0xee, -3, -9, -7, -5.0, 3
LAYOUTS = {L["name"]: L for L in D.layouts()}
PLAIN = [n for n, L in LAYOUTS.items() if not L["gpu_only"]]


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def ref():
    rs = D.reference()
    for R in rs.values():
        c = R["case"]
        R["cnts"], R["avg_k"] = EM.counts(R["mid"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"])
    return rs


def _opt():
    from mm2chain import params
    return params.mapq_opts(**MAPQ_DEFAULT)


def _pack(rs, b_off, n_reads=None):
    """the reads one after another at the given anchor offsets, each with one filler row behind its hits; padded with empty reads; the reads' reference lengths are
    appended to one array and the rid of their hits is moved accordingly"""
    n_reads = len(rs) if n_reads is None else n_reads
    pad = n_reads - len(rs)
    off = lambda v: np.concatenate([[0], np.cumsum(v + [0] * pad)]).astype(np.int64)
    u_off, m_off = off([R["hits"].size + 1 for R in rs]), off([R["case"]["mini_pos"].size for R in rs])
    r_off = off([R["case"]["ref_len"].size for R in rs])
    b_off = np.concatenate([np.asarray(b_off, np.int64), np.full(pad, b_off[-1], np.int64)])
    regs = np.full((int(u_off[-1]), 80), REG_FILL, np.uint8)
    for k, R in enumerate(rs):
        g = R["hits"].copy()
        g["rid"] += int(r_off[k])
        regs[u_off[k]:u_off[k] + g.size] = g.view(np.uint8).reshape(-1, 80)
    cat = lambda parts, empty: np.concatenate(list(parts) + [empty])
    return {"u_off": u_off, "b_off": b_off, "mini_off": m_off, "r_off": r_off, "regs": regs, "b": cat((R["case"]["a"] for R in rs), np.zeros((0, 2), np.uint64)),
            "mini_pos": cat((R["case"]["mini_pos"] for R in rs), np.zeros(0, np.uint64)), "ref_len": cat((R["case"]["ref_len"] for R in rs), np.zeros(0, np.uint32)),
            "n_in": np.array([R["hits"].size for R in rs] + [0] * pad, np.int32), "qlen": np.array([R["case"]["qlen"] for R in rs] + [1000] * pad, np.int32),
            "rep_len": np.array([R["case"]["rep_len"] for R in rs] + [0] * pad, np.int32)}


def _run(mp, ep, pk, window=0):
    """MapqPlan.run with anchors, then EstErrPlan.run on its outputs, one stream, nothing coming back in between.  The anchors lie at pk["b_off"][0] on; b and b_out
    are made on the device.  -> host copies; of b_out only the rows from `window` on, the rows in front of it are checked on the device"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lo = int(pk["b_off"][0])
    regs = np.full((max(mp.n_u_cap, 1), 80), REG_FILL, np.uint8); regs[:pk["regs"].shape[0]] = pk["regs"]
    d_b = torch.zeros((max(mp.n_b_cap, 1), 2), dtype=torch.int64, device="cuda")
    d_b[lo:lo + pk["b"].shape[0]] = t(pk["b"].view(np.int64))
    out = torch.full((max(mp.n_u_cap, 1) + GUARD, 80), REG_FILL, dtype=torch.uint8, device="cuda")
    n_out = torch.full((mp.n_reads + GUARD,), N_FILL, dtype=torch.int32, device="cuda")
    b_out = torch.full((max(mp.n_b_cap, 1) + GUARD, 2), B_FILL, dtype=torch.int64, device="cuda")
    n_b_out = torch.full((mp.n_reads + GUARD,), N_FILL, dtype=torch.int64, device="cuda")
    err = torch.full((max(ep.n_u_cap, 1) + GUARD, 2), ERR_FILL, dtype=torch.int32, device="cuda")
    avg = torch.full((ep.n_reads + GUARD,), AVG_FILL, dtype=torch.float32, device="cuda")
    mpos = np.zeros(max(ep.n_mini_cap, 1), np.int64); mpos[:pk["mini_pos"].size] = pk["mini_pos"].view(np.int64)
    d_uo, d_bo, d_q = t(pk["u_off"]), t(pk["b_off"]), t(pk["qlen"])
    mp.run(_opt(), d_uo, t(regs), t(pk["n_in"]), d_bo, d_b, d_q, t(pk["rep_len"]), regs_out=out, n_out=n_out, b_out=b_out, n_b_out=n_b_out)
    ep.run(d_uo, out, n_out, d_bo, b_out, t(pk["mini_off"]), t(mpos), d_q, t(pk["ref_len"].view(np.int32)), err=err, avg_k=avg)
    torch.cuda.synchronize()
    assert bool((d_b[:lo] == 0).all()) and bool((d_b[lo + pk["b"].shape[0]:] == 0).all()) and np.array_equal(d_b[lo:lo + pk["b"].shape[0]].cpu().numpy(), pk["b"].view(np.int64)), "d_b was written"
    assert bool((b_out[:window] == B_FILL).all()), "anchors in front of the batch's first were written"
    return {"regs": out.cpu().numpy(), "n_out": n_out.cpu().numpy(), "b_out": b_out[window:].cpu().numpy().view(np.uint64), "n_b_out": n_b_out.cpu().numpy(),
            "err": err.cpu().numpy(), "avg": avg.cpu().numpy(), "window": window}


def _assert_batch(got, pk, rs, what, refused=()):
    """every read against the record; everything the record does not own against the fill"""
    import mm2chain
    n_reads = pk["u_off"].size - 1
    want_b = np.full(got["b_out"].shape, np.uint64(B_FILL & 0xffffffffffffffff), np.uint64)
    used = np.zeros(got["regs"].shape[0], bool)
    for k in range(n_reads):
        lo = int(pk["u_off"][k])
        if k in refused:
            assert got["n_out"][k] == N_FILL and got["n_b_out"][k] == N_FILL and got["avg"][k] == AVG_FILL, f"{what}: the refused read {k} wrote its counts"
            continue
        if k >= len(rs):                                                        # a padding read
            assert got["n_out"][k] == 0 and got["n_b_out"][k] == 0, f"{what}: padding read {k}"
            continue
        R = rs[k]
        mid, fin = R["mid"].copy(), R["out"].copy()
        mid["rid"] += int(pk["r_off"][k]); fin["rid"] += int(pk["r_off"][k])
        n = mid.size
        used[lo:lo + n] = True
        assert got["n_out"][k] == n and got["n_b_out"][k] == R["a"].shape[0], f"{what}: {R['name']} (read {k}): n_out {got['n_out'][k]}, n_b_out {got['n_b_out'][k]}; the record {n}, {R['a'].shape[0]}"
        g = got["regs"][lo:lo + n].reshape(-1).view(REG)
        assert g.tobytes() == mid.tobytes(), f"{what}: {R['name']} (read {k}): the final regions differ from the record"
        e = got["err"][lo:lo + n]
        assert np.array_equal(e, R["cnts"]), f"{what}: {R['name']} (read {k}): (n_match, n_tot) {e.tolist()}, the record {R['cnts'].tolist()}"
        assert np.float32(got["avg"][k]).tobytes() == np.float32(R["avg_k"]).tobytes(), f"{what}: {R['name']} (read {k}): avg_k {got['avg'][k]!r}, the record {R['avg_k']!r}"
        g = g.copy()
        mm2chain.est_err_apply([0], [n], e.copy(), got["avg"][k:k + 1], g)
        assert g.tobytes() == fin.tobytes(), f"{what}: {R['name']} (read {k}): div {g['div'].tolist()}, the record {fin['div'].tolist()} (the fixture's libm: {R['libm']})"
        at = int(pk["b_off"][k]) - got["window"]
        want_b[at:at + R["a"].shape[0]] = R["a"]
    bad = np.nonzero((got["b_out"] != want_b).any(axis=1))[0]
    assert bad.size == 0, f"{what}: b_out differs from the record (or a tail, the front or the guard from the fill) at positions {(bad[:6] + got['window']).tolist()}, reads at {pk['b_off'].tolist()}"
    assert (got["regs"][~used] == REG_FILL).all() and (got["err"][~used] == ERR_FILL).all(), f"{what}: rows no region of the record owns were written"
    assert (got["n_out"][n_reads:] == N_FILL).all() and (got["n_b_out"][n_reads:] == N_FILL).all() and (got["avg"][n_reads:] == AVG_FILL).all(), f"{what}: guard counts were written"


def _plans(n_reads, pk_list, n_b_cap):
    import mm2chain
    n_u = max(int(pk["u_off"][-1]) for pk in pk_list)
    n_m = max(pk["mini_pos"].size for pk in pk_list)
    return mm2chain.MapqPlan(n_reads, n_u, n_b_cap, max_log_arg=1 << 16), mm2chain.EstErrPlan(n_reads, n_u, n_b_cap, n_m)


def _host_entries(pk, rs, what):
    import mm2chain
    h = mm2chain.join_mapq_batch(_opt(), pk["u_off"], pk["regs"], pk["n_in"], pk["b_off"], pk["b"], pk["qlen"], pk["rep_len"])
    regs = np.full_like(pk["regs"], REG_FILL)
    b = np.zeros_like(pk["b"])
    for k, R in enumerate(rs):
        lo, bo = int(pk["u_off"][k]), int(pk["b_off"][k])
        mid = R["mid"].copy()
        mid["rid"] += int(pk["r_off"][k])
        assert h[1][k] == mid.size and h[0][lo:lo + mid.size].tobytes() == mid.tobytes(), f"join_mapq_batch, {what}: {R['name']} (read {k}): regions"
        assert h[3][k] == R["a"].shape[0] and h[2][bo:bo + R["a"].shape[0]].tobytes() == R["a"].tobytes(), f"join_mapq_batch, {what}: {R['name']} (read {k}): a[]"
        regs[lo:lo + mid.size] = mid.view(np.uint8).reshape(-1, 80)
        b[bo:bo + R["a"].shape[0]] = R["a"]
    n_fin = np.array([R["mid"].size for R in rs], np.int32)
    g, err, avg = mm2chain.est_err_batch(pk["u_off"], regs, n_fin, pk["b_off"], b, pk["mini_off"], pk["mini_pos"], pk["qlen"], pk["ref_len"])
    for k, R in enumerate(rs):
        lo, n = int(pk["u_off"][k]), R["mid"].size
        fin = R["out"].copy()
        fin["rid"] += int(pk["r_off"][k])
        assert np.array_equal(err[lo:lo + n].view(np.int32).reshape(-1, 2), R["cnts"]) and avg[k].tobytes() == np.float32(R["avg_k"]).tobytes(), f"est_err_batch, {what}: {R['name']} (read {k})"
        assert g[lo:lo + n].tobytes() == fin.tobytes(), f"est_err_batch, {what}: {R['name']} (read {k}): regions (the fixture's libm: {R['libm']})"


@pytest.mark.parametrize("name", PLAIN)
def test_a_layout_on_plans_of_its_own_size_and_through_the_host_entries(ref, name):
    L = LAYOUTS[name]
    rs = [ref[n] for n in L["reads"]]
    pk = _pack(rs, D.b_off(L))
    mp, ep = _plans(len(rs), [pk], int(pk["b_off"][-1]))
    try:
        got = _run(mp, ep, pk)
        mp.check(); ep.check()
        _assert_batch(got, pk, rs, name)
    finally:
        ep.close(); mp.close()
    _host_entries(pk, rs, name)


def test_every_layout_again_on_one_pair_of_plans_behind_other_data(ref):
    n_reads = max(len(LAYOUTS[n]["reads"]) for n in PLAIN)
    pks = {n: _pack([ref[r] for r in LAYOUTS[n]["reads"]], D.b_off(LAYOUTS[n]), n_reads) for n in PLAIN}
    mp, ep = _plans(n_reads, list(pks.values()), max(int(pk["b_off"][-1]) for pk in pks.values()))
    try:
        for order in (PLAIN, PLAIN[::-1]):
            for n in order:
                got = _run(mp, ep, pks[n])
                mp.check(); ep.check()
                _assert_batch(got, pks[n], [ref[r] for r in LAYOUTS[n]["reads"]], f"{n}, on the shared plans")
    finally:
        ep.close(); mp.close()


def test_the_second_turn_of_the_grid(ref):
    """the batch's first anchor at TURN - 6000 on plans of TURN + 16384 anchors: 2048 workgroups, whose first four take the slices from TURN on in their second turn;
    every position in front of b_off[0] is one of a slice whose search ends at read 0 and whose lanes must skip.  b and b_out are made on the device (134 MB each),
    the 8.4 M positions in front of the batch are compared there and only the window from TURN - 8192 on comes back"""
    L = LAYOUTS["second_turn"]
    rs = [ref[n] for n in L["reads"]]
    pk = _pack(rs, D.b_off(L))
    other = _pack(rs[::-1], np.concatenate([[0], np.cumsum([R["case"]["a"].shape[0] for R in rs[::-1]])]) + D.SECOND_TURN_B_OFF0 + 1000)
    assert int(pk["b_off"][0]) == D.TURN - 6000 and int(other["b_off"][-1]) <= D.SECOND_TURN_CAP and (D.SECOND_TURN_CAP + D.SLICE - 1) // D.SLICE > D.GRID_CAP
    mp, ep = _plans(len(rs), [pk, other], D.SECOND_TURN_CAP)
    window = D.TURN - 2 * D.SLICE
    try:
        for p, reads, what in ((pk, rs, "second_turn"), (other, rs[::-1], "second_turn, reversed and 1000 further"), (pk, rs, "second_turn, again")):
            got = _run(mp, ep, p, window=window)
            mp.check(); ep.check()
            _assert_batch(got, p, reads, what)
        print(f"mapq_join, mapq_gather: {mp.last_kernel_ms()} ms; err_reads, err_walk, err_finish: {ep.last_kernel_ms()} ms")
    finally:
        ep.close(); mp.close()


@pytest.mark.parametrize("kind", list(D.BY_READ_REFUSALS))
def test_read_by_read_behind_a_refusal(ref, kind):
    """eight reads on three workgroups; one read is refused, so mapq_gather and err_walk go read by read: `r += gridDim.x` and `q += 256` take further steps, lanes
    carry their memo from hit300 to drop4_front, and fail_2reg's two regions fail in one wave.  The refused read writes nothing, the seven others are exact"""
    L = LAYOUTS["by_read"]
    rs = [ref[n] for n in L["reads"]]
    sound = _pack(rs, D.b_off(L))
    bad = D.BY_READ_REFUSALS[kind]
    pk = {k: v.copy() for k, v in sound.items()}
    if kind == "offset":
        assert bad == len(rs) - 1
        pk["b_off"][bad + 1] = D.BY_READ_CAP + 9                                # its anchors leave the plan's capacity
    else:
        h = pk["regs"][int(pk["u_off"][bad]):int(pk["u_off"][bad]) + 1].reshape(-1).view(REG)
        h["as"] = 100000                                                        # a hit that leaves the read's anchors
    mp, ep = _plans(len(rs), [sound], D.BY_READ_CAP)
    try:
        got = _run(mp, ep, pk)
        rc, _, _ = mp.counts()
        assert rc == -2 and ep.refused() == (-2, 1), f"{kind}: MapqPlan {rc}, EstErrPlan {ep.refused()}"
        _assert_batch(got, pk, rs, f"by_read, {kind}", refused=(bad,))
        got = _run(mp, ep, sound)                                               # the same plans on the sound batch afterwards: the slice path again
        mp.check(); ep.check()
        _assert_batch(got, sound, rs, f"by_read, sound behind {kind}")
    finally:
        ep.close(); mp.close()
