"""The score-bound exit of the tile kernel's hand-written loop (csrc/chain_dp_tile.h, MM2C_EXIT_TEST) on the CPU: the model of the loop with the exit
(tests/tile_model.py with late_stamps=False: the loop as it was when it got the exit) against the oracle.  An anchor's scan ends once pfx + span_i <= best, pfx being the largest f before the tile in progress: a pair scores
at most f[j] + span_i while the gap cost is not a gain, so f / p cannot change -- the exit only replaces the rest of a scan that would have counted skip events.
A. the standard inputs; B. the equality edge (f[j] + span_i == best leaves, == best + 1 does not); C. first tile and short last tile; D. gap_scale < 0, where the
bound does not hold and the exit stays off; E. the task the GPU test has cut into pieces on the device."""
import numpy as np
import pytest

import oracle_binding as ob
import score_exit_data as sx
from tile_loop_harness import run_model, same as _same
from tile_model import LABEL_KEYS, chain_tile_model


def _run(P, t, **kw):
    """(oracle f, p), (model f, p), stats, anchors that left early"""
    return run_model(P, t, late_stamps=False, **kw)[:4]


@pytest.mark.parametrize("form", list(sx.FORMS))
def test_a_standard_inputs_equal_the_oracle_and_keep_every_label_warm(form):
    from mm2chain import params
    compact, NX = sx.FORMS[form]
    S = dict.fromkeys(LABEL_KEYS + ("exits",), 0)
    for max_skip in sx.SKIPS:
        P = params.make_params(max_skip=max_skip)
        for k, t in enumerate(sx.standard_tasks()):
            ref, got, st, _ = _run(P, t, NX=NX, compact=compact)
            assert _same(ref, got), (form, max_skip, k)
            for key in S:
                S[key] += st[key]
    assert S["exits"] > 0
    cold = [k for k in LABEL_KEYS if S[k] < 3]
    assert not cold, f"{form}: sub-paths of the fold that go cold with the exit in: {cold}"


@pytest.mark.parametrize("kind,far", sx.EDGE_CASES)
def test_b_equality_edge(kind, far):
    P, t, info = sx.edge_case(kind, far)
    T, c, j = info["T"], info["c"], info["j"]
    for form, (compact, NX) in sx.FORMS.items():
        ref, got, st, ex = _run(P, t, NX=NX, compact=compact)
        f, p = ref
        assert _same(ref, got), (kind, far, form)
        # what the input is named for, from the oracle alone: T's tile starts after j, j is lone, and f[j] + span_T is the best through c (fires) or one more (holds)
        assert j < T - T % 64 <= c < T and p[j] == -1 and f[j] == 30 and p[c] == j
        assert (T - j > 960) == far
        older = f[:T - T % 64]
        if kind == "fires":
            assert f[T] == info["best"] == f[j] + sx.SPAN and p[T] == c and older.max() == f[j]
            assert T in ex
        else:
            assert f[T] == info["best"] == f[c] + sx.SPAN - 2 + 1 == f[j] + sx.SPAN and p[T] == j
            assert T not in ex
        # with the exit off the same f / p: the exit changed nothing
        _, off_, st0, ex0 = _run(P, t, NX=NX, compact=compact, score_exit="off")
        assert _same(ref, off_) and st0["exits"] == 0 and not ex0


def test_c_first_tile_and_short_last_tile():
    from mm2chain import params
    P = params.map_ont()
    exits = 0
    for t in sx.short_tasks():
        for compact, NX in sx.FORMS.values():
            ref, got, st, ex = _run(P, t, NX=NX, compact=compact)
            assert _same(ref, got), t.shape[0]
            assert all(i >= 64 for i in ex)                       # no pfx during the first tile
            if t.shape[0] <= 64:
                assert st["exits"] == 0
            exits += st["exits"]
    assert exits > 0


def test_d_negative_gap_scale_has_teeth():
    P, tasks, info = sx.negative_gap_case()
    T, c = info["T"], info["c"]
    for k, t in enumerate(tasks):
        ref, got, st, _ = _run(P, t, NX=16, compact=True)         # "auto": off for gap_scale < 0, as the host decides
        assert _same(ref, got) and st["exits"] == 0
        forced, ex = _run(P, t, NX=16, compact=True, score_exit="force")[1::2]
        if k == 0:
            # the gain of the link to j lifts it over the bound: the oracle takes j, the forced exit has left with c
            assert ref[1][T] == info["j"] and ref[1][c] == -1 and ref[0][T] > ref[0][info["j"]] + sx.SPAN
            assert T in ex and forced[1][T] == c and forced[0][T] < ref[0][T], "with the exit forced on, gap_scale < 0 must change f / p: the host's condition would have no teeth"


def test_e_the_device_cut_task_is_cut_and_its_pieces_exit():
    P, t = sx.cut_task()
    pieces = sx.cut_pieces(P, t)
    assert len(pieces) > 1 and all(e - s >= sx.CUT_SEG_MIN for s, e in pieces) and pieces[0][0] == 0 and pieces[-1][1] == t.shape[0]
    avg = ob.avg_qspan(t)                                         # avg_qspan_scaled is the whole task's (chain.c:48-49): every piece inherits it
    f, p, _ = ob.chain_fpv(P, t, avg)
    exits = []
    for s, e in pieces:
        st, ex = {}, []
        fm, pm = chain_tile_model(P, t[s:e], avg, NX=16, compact=True, stats=st, exit_anchors=ex, late_stamps=False)
        assert np.array_equal(fm, f[s:e]) and np.array_equal(np.where(pm >= 0, pm + s, pm), p[s:e]), (s, e)
        assert all(i >= 64 for i in ex)                           # a piece starts its own pfx: nothing leaves during its first tile
        exits.append(st["exits"])
    assert min(exits) > 0, exits
