"""The fold order of the tile kernel's hand-written loop (csrc/chain_dp_tile.h: stamps and marks of a scored chunk behind the fold's decision, MM2C_ST_LEAN /
MM2C_ST_FAR) on the CPU: the model of the loop in that order (tests/tile_model.py, its default) against the oracle, and the inputs of tests/late_stamp_data.py against
what they are named for.  A chunk whose fold B0 takes the score-bound exit leaves before any of its stamps is written; every other fold stamps before it reads a mark.
A. the standard inputs at max_skip 0, 1 and 25: the model equals the oracle, exits without stamps happen in the own tile and are followed, in the same tile, by
anchors whose fold reads own-tile marks, and a fold B0 that stays reaches the `break` at each max_skip (late stamps are still counted); B. windows of 1 .. 6 whole older
tiles with and without a partly covered one: the best candidate is the deepest, on either side of the end of the f / p ring; C. first tile and short last tile;
D. the device-cut task; E. with the exit off nothing leaves without stamps and the counters are those of the model with the stamps before the fold (late_stamps=False)."""
import numpy as np
import pytest

import late_stamp_data as ls
import oracle_binding as ob
import score_exit_data as sx
from tile_loop_harness import run_model, same as _same
from tile_model import chain_tile_model


def _run(P, t, **kw):
    """(oracle f, p), (model f, p), stats, events"""
    ref, got, st, _, ev = run_model(P, t, **kw)
    return ref, got, st, ev


@pytest.mark.parametrize("form", list(ls.FORMS))
def test_a_standard_inputs_equal_the_oracle(form):
    from mm2chain import params
    compact, NX, NF = ls.FORMS[form]
    for max_skip in ls.SKIPS:
        P = params.make_params(max_skip=max_skip)
        S = dict.fromkeys(("exits", "exits_unstamped", "stamped_chunks", "cpp_chunks", "own_pass", "ring_pass", "near_pass", "deep_pass", "break_in_b0", "break_in_fold_a"), 0)
        followed = 0
        for k, t in enumerate(ls.standard_tasks()):
            ref, got, st, ev = _run(P, t, NX=NX, NF=NF, compact=compact)
            assert _same(ref, got), (form, max_skip, k)
            for key in S:
                S[key] += st[key]
            # an exit without stamps in the own-tile chunk, and later in the same tile an anchor whose fold reads a mark of its own tile
            marks = np.array(ev["own_marks"], np.int64)
            followed += sum(1 for i, where in ev["unstamped"] if where == "own" and ((marks > i) & (marks // 64 == i // 64)).any())
        assert 0 < S["exits_unstamped"] <= S["exits"], (form, max_skip, S)
        assert S["stamped_chunks"] + S["cpp_chunks"] == S["own_pass"] + S["ring_pass"] - S["exits_unstamped"], (form, max_skip, S)
        assert S["near_pass"] + S["deep_pass"] == S["ring_pass"] and S["deep_pass"] > 0, (form, max_skip, S)
        assert followed >= 3, (form, max_skip, followed)
        assert S["break_in_b0"] >= 3 and S["break_in_fold_a"] >= 3, (form, max_skip, S)   # a B0 that stays, stamps late and ends the scan by its marks


@pytest.mark.parametrize("m,part", ls.DEPTH_CASES)
def test_b_windows_around_the_end_of_the_fp_ring(m, part):
    P, t, info = ls.depth_case(m, part)
    T, cands = info["T"], info["cands"]
    assert len(cands) == m + (part > 0)
    for form, (compact, NX, NF) in ls.FORMS.items():
        ref, got, st, _ = _run(P, t, NX=NX, NF=NF, compact=compact)
        f, p = ref
        assert _same(ref, got), (m, part, form)
        # what the input is named for, from the oracle alone: lone candidates, the deepest is T's best, and each older tile of the window holds one
        assert all(p[j] == -1 and f[j] == 100 + 22 * d for d, j in cands)
        assert p[T] == cands[-1][1] and f[T] > f[cands[-1][1]]
        assert [(T - 30 - j + 63) // 64 for _, j in cands] == [d for d, _ in cands]
        # ... and from the model: T alone scores ring tiles, one per candidate, on the side of the f / p ring's end that its depth says
        assert st["ring_pass"] == len(cands) and st["near_pass"] == min(len(cands), NF) and st["deep_pass"] == max(len(cands) - NF, 0), (m, part, form, st)
        assert st["part_pass"] == (part > 0) and st["fold_b0"] >= len(cands)


def test_c_first_tile_and_short_last_tile():
    from mm2chain import params
    P = params.map_ont()
    for t in sx.short_tasks():
        for compact, NX, NF in ls.FORMS.values():
            ref, got, st, ev = _run(P, t, NX=NX, NF=NF, compact=compact)
            assert _same(ref, got), t.shape[0]
            assert all(i >= 64 for i, _ in ev["unstamped"])       # no exit during the first tile: every chunk of it stamps


def test_d_the_pieces_of_the_device_cut_task():
    P, t = sx.cut_task()
    avg = ob.avg_qspan(t)
    f, p, _ = ob.chain_fpv(P, t, avg)
    for s, e in sx.cut_pieces(P, t):
        st = {}
        fm, pm = chain_tile_model(P, t[s:e], avg, NX=16, NF=4, compact=True, stats=st)
        assert np.array_equal(fm, f[s:e]) and np.array_equal(np.where(pm >= 0, pm + s, pm), p[s:e]), (s, e)
        assert st["exits_unstamped"] > 0


def test_e_exit_off_and_the_counters_of_the_earlier_model():
    from mm2chain import params
    P = params.make_params(max_skip=3)
    for t in sx.fold_and_stream_tasks():
        avg = ob.avg_qspan(t)
        for mode in ("auto", "off"):
            a, b = {}, {}
            ra = chain_tile_model(P, t, avg, NX=16, NF=4, compact=True, stats=a, score_exit=mode, late_stamps=False)
            rb = chain_tile_model(P, t, avg, NX=16, NF=4, compact=True, stats=b, score_exit=mode)
            assert _same(ra, rb)
            assert all(a[k] == b[k] for k in a if k != "far_stamp"), {k: (a[k], b[k]) for k in a if a[k] != b[k]}   # (far stamps: an exit without stamps writes none)
            assert b["far_stamp"] <= a["far_stamp"]
            if mode == "off":
                assert b["exits_unstamped"] == 0 and b["stamped_chunks"] + b["cpp_chunks"] == b["own_pass"] + b["ring_pass"]
