"""The region plan's promise about broken reads (include/mm2chain.h): a read whose offsets leave the plan's capacities gets unspecified regions, check()
answers MM2C_E_ARG, and "the regions of the other reads are not affected".  The fill pass looks chains up in per-chain scratch (cstart, cend, crank) that only the
sort pass of an accepted read writes, so the promise has to hold on a plan whose scratch still holds another run: every pattern below follows a clean run of the same
four reads in reverse order, and is followed by a clean run in a third order that has to be exact again.  The output has guard rows behind the plan's capacity.

By the code none of the patterns makes a kernel touch memory outside the buffers, which are padded to the capacities: regs_sort tests a read's offsets before any
access; the fill kernels load b only inside an accepted read's extent (below b_off[n_reads] when every read was accepted), write regions only below n_u_cap, and
index their LDS table below its size."""
import os

import numpy as np
import pytest
import torch

import regs_data
import regs_model as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("one_chain", "cnt1_among", "rows", "sort65")
N_U_CAP, N_B_CAP, GUARD = 1400, 2000, 8


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def reads():
    """the four cases in forward order, each with the rows the reference's hit.o made of it"""
    Z = np.load(os.path.join(GOLDEN, "ref_regs.npz"))
    assert int(Z["reg_size"]) == M.REG.itemsize
    idx = {c["name"]: k for k, c in enumerate(regs_data.cases())}
    out = []
    for name in NAMES:
        c = dict(regs_data.cases()[idx[name]])
        c["want"] = Z["regs"][Z["reg_off"][idx[name]]:Z["reg_off"][idx[name] + 1]].copy()
        assert c["want"].shape == (c["u"].size, 80)
        out.append(c)
    return out


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view({8: np.int64, 4: np.int32}[x.dtype.itemsize])).cuda()


def _run(plan, cs, u_off=None, b_off=None, shift=(0, 0)):
    """cs as one batch, every buffer padded to the plan's capacities, under the given offsets (the true ones by default); shift: that many unused chains and anchors
    in front of the batch -> (regions and guard rows uint8 [n_u_cap + GUARD, 80], the true u_off, the true b_off)"""
    uo, u, bo, b, qlen, hash_ = regs_data.batch(cs)
    uo, bo = uo + shift[0], bo + shift[1]
    pad = lambda x, n: np.concatenate([np.zeros((shift[x.ndim - 1],) + x.shape[1:], x.dtype), x, np.zeros((n - x.shape[0] - shift[x.ndim - 1],) + x.shape[1:], x.dtype)])
    full = torch.full((N_U_CAP + GUARD, 80), 0xee, dtype=torch.uint8, device="cuda")
    regs = plan.run(_dev(uo if u_off is None else np.asarray(u_off, np.int64)), _dev(pad(u, N_U_CAP)), _dev(bo if b_off is None else np.asarray(b_off, np.int64)),
                    _dev(pad(b, N_B_CAP)), _dev(qlen), _dev(hash_), regs=full[:N_U_CAP])
    assert regs.data_ptr() == full.data_ptr()
    return full, uo, bo


def _differences(got, cs, uo, which):
    """per read of `which`: the fields in which its regions differ from the fixture"""
    bad = []
    for r in which:
        g, w = got[uo[r]:uo[r + 1]].reshape(-1).view(M.REG), cs[r]["want"].reshape(-1).view(M.REG)
        fields = [f for f in M.REG.names if not np.array_equal(g[f], w[f])]
        if fields or g.tobytes() != w.tobytes():
            rows = sorted({int(i) for f in fields for i in np.nonzero(g[f] != w[f])[0]})
            bad.append(f"read {r} ({cs[r]['name']}): {fields} differ in {len(rows)} of {g.size} regions, first {rows[0] if rows else '?'}: "
                       f"got {[int(g[f][rows[0]]) for f in fields] if rows else '?'} want {[int(w[f][rows[0]]) for f in fields] if rows else '?'}")
    return bad


def _clean(plan, cs, what):
    full, uo, _ = _run(plan, cs)
    plan.check()
    got = full.cpu().numpy()
    bad = _differences(got, cs, uo, range(len(cs)))
    assert not bad, f"{what}:\n" + "\n".join(bad)
    assert (got[N_U_CAP:] == 0xee).all(), f"{what}: the rows behind n_u_cap were written"


def _patterns(uo, bo):
    u, b = [int(x) for x in uo], [int(x) for x in bo]
    return {"last_three_u_beyond": ([u[0], u[1], N_U_CAP + 5, N_U_CAP + 5, N_U_CAP + 9], b),
            "middle_two_u_negative": ([u[0], u[1], -4, u[3], u[4]], b),
            "first_u_negative": ([-3, u[1], u[2], u[3], u[4]], b),
            "last_b_beyond": (u, [b[0], b[1], b[2], b[3], N_B_CAP + 7]),
            "last_b_negative": (u, [b[0], b[1], b[2], b[3], -4]),
            "last_b_below_the_good_reads": (u, [b[0], b[1], b[2], b[3], b[1]])}


PATTERNS = ("last_three_u_beyond", "middle_two_u_negative", "first_u_negative", "last_b_beyond", "last_b_negative", "last_b_below_the_good_reads")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_broken_offsets_beside_good_reads_on_a_plan_that_ran_other_data(pattern, reads):
    import mm2chain
    cs = reads
    plan = mm2chain.RegPlan(4, N_U_CAP, N_B_CAP)
    try:
        _clean(plan, cs[::-1], "step 1, the reads in reverse order")          # leaves scratch that differs from what the next run writes
        uo, _, bo, _, _, _ = regs_data.batch(cs)
        u_off, b_off = _patterns(uo, bo)[pattern]
        good = [r for r in range(4) if 0 <= u_off[r] <= u_off[r + 1] <= N_U_CAP and 0 <= b_off[r] <= b_off[r + 1] <= N_B_CAP]
        assert 1 <= len(good) < 4 and all(u_off[r] == uo[r] and u_off[r + 1] == uo[r + 1] and b_off[r] == bo[r] and b_off[r + 1] == bo[r + 1] for r in good)
        full, _, _ = _run(plan, cs, u_off, b_off)
        with pytest.raises(mm2chain.Mm2cError, match="code -2"):
            plan.check()
        got = full.cpu().numpy()
        bad = _differences(got, cs, uo, good)
        print(f"{pattern}: good reads {good}; " + ("all exact" if not bad else " | ".join(bad)))
        assert not bad, f"{pattern}: reads beside the refused ones differ from the fixture:\n" + "\n".join(bad)
        assert (got[N_U_CAP:] == 0xee).all(), f"{pattern}: the rows behind n_u_cap were written"
        _clean(plan, [cs[2], cs[0], cs[3], cs[1]], "step 3, the clean batch in a third order after the broken run")
    finally:
        plan.close()


def test_a_batch_that_does_not_start_at_chain_0_on_a_plan_that_ran_other_data(reads):
    """u_off[0] = 3 and b_off[0] = 5 are inside the capacities: the chains below u_off[0] keep the scratch of the run before, which the fill pass must not search"""
    import mm2chain
    cs = reads
    plan = mm2chain.RegPlan(4, N_U_CAP, N_B_CAP)
    try:
        _clean(plan, cs[::-1], "the reads in reverse order")
        full, uo, bo = _run(plan, cs, shift=(3, 5))
        assert uo[0] == 3 and bo[0] == 5 and plan.check() == 0
        got = full.cpu().numpy()
        bad = _differences(got, cs, uo, range(4))
        assert not bad, "a batch that starts at chain 3, anchor 5:\n" + "\n".join(bad)
        assert (got[N_U_CAP:] == 0xee).all()
        _clean(plan, [cs[2], cs[0], cs[3], cs[1]], "the clean batch in a third order")
    finally:
        plan.close()
