"""CPU tests of the batch layouts of tests/anchor_space_limit_data.py and of the lane-level model of mapq_gather / err_walk (tests/anchor_space_model.py): the
fixtures of the module's reads agree with the models of the arithmetic; every layout plants what it says (positions, and memo hits and misses read from the model's
trace); the right model equals the reference record on every layout, on the second-turn layout under the real grid cap and on a short copy under a cap of 2, and
on the read-by-read path; each wrong variant differs from the record on a new layout.

What the OLD batch layouts tell apart (printed by test_each_wrong_variant_is_caught_by_a_new_layout, not asserted): the batches tests/test_gpu_mapq.py builds from
mapq_data (one per option group, and one read per call, the first n_b_out anchors of a read compared) and those tests/test_gpu_esterr.py builds from esterr_data
(all cases in order, reversed, and one read per call):

  variant            new layouts that catch it                                          old mapq_data batches    old esterr_data batches
  memo_no_read       9: across_sq_sq, across_sq_copy, across_copy_sq, across_err_other, ...    yes                      yes
  memo_le            15: memo_join256/257/512/513, memo_adjoin*, ewalk256/257/512/513, ...     no                       no
  stale_flag         16: every layout with a join (edge_absorbed_*, memo_join*, ...)           yes                      -
  ignore_n_b_out     18: every layout with a dropped secondary (edge_dropped_*, edge_last_*)   no (tails not compared)  -
  search_first       0: output-neutral, see below                                              no                       no
  step_once          25: boundary_empty*, every layout with reads shorter than 256             yes                      yes
  stride_minus_1     24, by the visit count only: output-neutral, see below                    no                       no
  stride_plus_1      1: second_turn (and its short copy under a cap of 2)                      no                       no
  front_not_skipped  1: second_turn                                                            no                       no
  read_lags_tab      39: across_err_k0 and every region longer than 256                        -                        yes
  pred_minus_1       11: edge_rev_pred_*, ewalk*, across_err_other, by_read, second_turn       -                        yes

The many small reads of the old batches do carry a stale memo from read to read (a lane meets a new read at every step), so memo_no_read is one they would have
caught; what they cannot reach is the memo-hit branch inside a read (memo_le), the tails, the second turn and the space in front of b_off[0].

search_first cannot change the output of these kernels: every lane steps from the searched read with `while (p >= be) ++r` (chain_mapq.hip, mapq_gather; chain_esterr.hip,
err_walk), which walks over the empty reads of the run.  The test shows on boundary_empty1/2 that the variant's search does land on another read and that the output is
the same; step_once is the variant those layouts catch instead.  stride_minus_1 is output-neutral too: with p0 += (grid - 1) * slice every slice is still taken,
some by two workgroups, and both kernels are idempotent (a copy; an atomicMin) -- only the model's count of visits per position tells it, and on the GPU it would cost
time, not correctness.  stride_plus_1 is its output-visible sibling: a slice of the second turn is never taken."""
import numpy as np
import pytest

import anchor_space_limit_data as D
import anchor_space_model as A
import esterr_data
import esterr_model as EM
import mapq_data
import mapq_model as MM

JOIN = np.uint64(1 << 40)


@pytest.fixture(scope="module")
def ref():
    rs = D.reference()
    for R in rs.values():
        c = R["case"]
        R["cnts"], R["avg_k"] = EM.counts(R["mid"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"])
    return rs


def _batch(ref, L, **kw):
    rs = [ref[n] for n in L["reads"]]
    return rs, A.prepare(rs, D.b_off(L), **kw)


def _check(rs, B, variant=None, **kw):
    """-> None if the model (or its variant) equals the record on this batch, else what differs"""
    out, _ = A.gather(B, variant, **kw)
    want = A.expected_b_out(B, rs)
    if not kw.get("by_read") and any(B["visits"].get(p, 0) != 1 for p in range(max(B["b_off"][0], B["base"]), B["b_off"][-1])):
        return "a position of the batch is not visited exactly once"
    if out.tobytes() != want.tobytes():
        return f"b_out differs at {(np.nonzero((out != want).any(axis=1))[0][:4] + B['base']).tolist()}"
    ff, _ = A.walk(B, want, variant, **kw)
    nm = A.n_match(B, want, ff)
    for k, R in enumerate(rs):
        if nm[k] is not None and nm[k] != R["cnts"][:, 0].tolist():
            return f"n_match of read {k} ({R['name']}): {nm[k]}, the record {R['cnts'][:, 0].tolist()}"
    return None


def test_the_fixtures_of_the_new_reads_agree_with_the_models(ref):
    total = 0
    for n, R in ref.items():
        c = R["case"]
        fin, wa, _ = MM.join_mapq(R["hits"], c["a"], c["qlen"], c["mapq"], c["rep_len"])
        assert fin.tobytes() == R["mapq_out"].tobytes() == R["mid"].tobytes() and wa.tobytes() == R["mapq_a"].tobytes() == R["a"].tobytes(), n
        assert EM.est_err(R["mid"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"]).tobytes() == R["out"].tobytes(), n
        total += c["a"].shape[0]
        if n.startswith("fill"):                                                # one chain, one hit (copy state), every minimizer present
            assert c["u"].size == 1 and R["hits"].size == 1 and R["cnts"][:, 0].tolist() == [c["a"].shape[0]], n
    assert total < 60000
    assert ref["empty"]["case"]["a"].shape[0] == 0 and ref["empty"]["hits"].size == 0


def test_every_layout_plants_what_it_says(ref):
    S = D.SLICE
    Ls = {L["name"]: L for L in D.layouts()}
    moves = lambda n: A.prepare([ref[n]], [0, ref[n]["case"]["a"].shape[0]])["rd"][0]["moves"]
    # ---- the reads of interest ----
    assert ref["absorbed"]["out"].size == 1 and ref["absorbed"]["a"][D.NAMED, 1] & JOIN and not (ref["absorbed"]["a"][:, 1] & JOIN)[np.arange(80) != D.NAMED].any()
    assert moves("absorbed") == [(0, 0, 40, 0), (40, 40, 40, 1)] and moves("dropped") == [(0, 0, 40, 0), (44, 40, 40, 0)]
    assert ref["dropped"]["a"].shape[0] == 80 and ref["dropped"]["case"]["a"].shape[0] == 84 and not (ref["dropped"]["a"][:, 1] & JOIN).any()
    assert ref["failing"]["cnts"][:, 0].tolist() == [D.NAMED] and ref["rev_pred"]["cnts"][:, 0].tolist() == [59]
    assert sorted(zip(ref["k0"]["out"]["as"].tolist(), ref["k0"]["out"]["cnt"].tolist())) == [(0, 40), (40, 60)] and (ref["k0"]["cnts"][:, 0] == ref["k0"]["out"]["cnt"]).all()
    for c in D.MEMO_SIZES:
        assert moves(f"memo_join{c}") == [(0, 0, c, 0), (c, c, c, 1)] and ref[f"memo_join{c}"]["out"]["cnt"].tolist() == [2 * c]
        assert moves(f"memo_adjoin{c}") == [(0, 0, c, 0), (c + 4, c, c, 0)] and sorted(ref[f"memo_adjoin{c}"]["out"]["cnt"].tolist()) == [c, c]
        e = ref[f"ewalk{c}"]["out"]
        assert sorted(zip(e["as"].tolist(), e["cnt"].tolist(), ((e["flags"] >> 10) & 1).tolist())) == [(0, c, 1), (c, c, 0)]
    assert moves("hit300") == [(0, 0, 300, 0), (300, 300, 40, 0)] and moves("drop4_front") == [(4, 0, 300, 0), (304, 300, 40, 0)]
    assert ref["copy_as4"]["hits"]["as"].tolist() == [4] and ref["copy340"]["hits"].size == 1
    er, ef = ref["e_rev_other"], ref["e_fwd"]
    assert er["case"]["qlen"] != ef["case"]["qlen"] and not set(er["case"]["mini_pos"].tolist()) & set(ef["case"]["mini_pos"].tolist())
    assert sorted(((er["out"]["flags"] >> 10) & 1).tolist()) == [0, 1] and not ((ef["out"]["flags"] >> 10) & 1).any()
    assert ref["fail_a"]["cnts"][:, 0].tolist() == [395] and ref["fail_b"]["cnts"][:, 0].tolist() == [3] and sorted(ref["fail_2reg"]["cnts"][:, 0].tolist()) == [5, 140]
    # ---- positions ----
    for at in (S - 1, S, S + 1):
        for rd in ("absorbed", "dropped", "failing", "k0", "rev_pred", "last"):
            L = Ls[f"edge_{rd}_{at}"]
            assert L["at"]["p"] == at and D.b_off(L)[L["at"]["read"]] + L["at"]["q"] == at, L["name"]
        L = Ls[f"edge_last_{at}"]
        assert D.b_off(L)[3] == at + 1 and L["reads"][3] == "dropped"            # the read ends on `at`, a squeezed read begins behind it
    for e in (0, 1, 2):
        L = Ls[f"boundary_empty{e}"]
        bo = D.b_off(L).tolist()
        assert L["at"]["p"] == S and bo.count(S) == e + 1 and bo.count(0) == e + 1 and bo.count(bo[-1]) == e + 1, L["name"]
    assert [int(D.b_off(Ls[f"end_{v}"])[-1]) for v in (S, S + 1, 2 * S)] == [S, S + 1, 2 * S]
    L = Ls["second_turn"]
    bo = D.b_off(L)
    assert L["at"]["p"] == D.TURN and bo[0] == D.TURN - 6000 and bo[L["at"]["read"]] < D.TURN < bo[L["at"]["read"] + 1] and L["reads"][L["at"]["read"]] == "memo_adjoin512"
    assert 18000 <= bo[-1] - bo[0] <= 22000 and 20 <= len(L["reads"]) <= 24
    L = Ls["by_read"]
    bo = D.b_off(L)
    assert len(L["reads"]) == 8 and all(300 <= D.length(n) <= 1500 for n in L["reads"]) and (D.BY_READ_CAP + S - 1) // S == 3
    assert (bo[2] + 395) // 64 == (bo[3] + 3) // 64, "fail_a's and fail_b's failing anchors lie in one wave of the slice path"
    # ---- the memo, from the model's trace ----
    n_plants = 0
    for L in D.layouts():
        if not L["plants"]:
            continue
        rs, B = _batch(ref, L)
        out, tg = A.gather(B)
        _, tw = A.walk(B, A.expected_b_out(B, rs))
        for kernel, k, q, what in L["plants"]:
            got = (tg if kernel == "mapq" else tw)[int(D.b_off(L)[k]) + q]
            assert got == what, f"{L['name']}: {kernel} at q = {q} of read {k}: the lane's memo gives {got!r}, the layout says {what!r}"
            n_plants += 1
    assert n_plants > 40
    rs, B = _batch(ref, Ls["edge_dropped_4095"])
    assert [A.gather(B)[1][int(D.b_off(Ls["edge_dropped_4095"])[2]) + q] for q in (79, 80, 83)] == ["miss", "tail", "tail"]


def test_the_right_model_equals_the_record_on_every_layout(ref):
    for L in D.layouts():
        rs, B = _batch(ref, L, n_b_cap=D.SECOND_TURN_CAP if L["name"] == "second_turn" else None)
        assert _check(rs, B) is None, L["name"]
    short = dict(next(L for L in D.layouts() if L["name"] == "second_turn"), reads=D.SECOND_TURN[:9], b_off0=2 * D.SLICE - 6000)
    rs, B = _batch(ref, short, n_b_cap=2 * D.SLICE + 4 * D.SLICE)
    assert D.b_off(short)[-1] > 2 * D.SLICE + 1000 and _check(rs, B, grid_cap=2) is None, "the short copy under a grid cap of 2"
    assert _check(rs, B, "stride_minus_1", grid_cap=2) is not None and _check(rs, B, "stride_plus_1", grid_cap=2) is not None


def test_the_right_model_equals_the_record_read_by_read(ref):
    L = next(L for L in D.layouts() if L["name"] == "by_read")
    for kind, bad in D.BY_READ_REFUSALS.items():
        rs, B = _batch(ref, L, n_b_cap=D.BY_READ_CAP, refused=(bad,))
        assert A._grid(B, D.SLICE, D.GRID_CAP) == 3
        assert _check(rs, B, by_read=True) is None, kind
        out, tg = A.gather(B, by_read=True)
        lo, hi = (int(v) for v in D.b_off(L)[bad:bad + 2])
        assert (out[lo:hi] == A.FILL).all() and not any(lo <= p < hi for p in tg), "the refused read is not touched"
        _, tw = A.walk(B, out, by_read=True)
        assert tg[int(D.b_off(L)[4]) + 100] == "miss" and tg[int(D.b_off(L)[4]) + 256 + 10] == "hit" and "hit" in tw.values(), "the memo is consulted on this path"
    rs, B = _batch(ref, L, n_b_cap=D.BY_READ_CAP, refused=(5,))
    assert _check(rs, B, "memo_no_read", by_read=True) is not None, "hit300 and drop4_front are one workgroup's neighbours: a stale memo copies from the wrong source"


def _old_batches():
    """the batch layouts of the existing GPU tests, as (kernel, reads, b_off)"""
    Z = np.load(mapq_data.__file__.replace("mapq_data.py", "golden/ref_mapq.npz"))
    cs = mapq_data.cases()
    mq = [{"name": c["name"], "case": c, "hits": Z["hits_in"][Z["in_off"][k]:Z["in_off"][k + 1]].reshape(-1).view(MM.REG), "a": Z["a_out"][Z["a_off"][k]:Z["a_off"][k + 1]]}
          for k, c in enumerate(cs)]
    off = lambda rs: np.concatenate([[0], np.cumsum([R["case"]["a"].shape[0] for R in rs])])
    out = []
    for _, idx in mapq_data.groups():
        rs = [mq[k] for k in idx]
        out.append(("mapq", rs, off(rs)))
    out += [("mapq", [R], off([R])) for R in mq]
    er = esterr_data.reference()
    for R in er:
        c = R["case"]
        R["mid"] = R["in"]
        R["cnts"] = EM.counts(R["in"], R["a"], c["mini_pos"], c["qlen"], c["ref_len"])[0]
    eo = lambda rs: np.concatenate([[0], np.cumsum([R["a"].shape[0] for R in rs])])
    out += [("esterr", er, eo(er)), ("esterr", er[::-1], eo(er[::-1]))] + [("esterr", [R], eo([R])) for R in er]
    return out


def _old_tells(old, variant):
    """whether any old batch tells the variant from the record, by what the old tests compare: the first n_b_out anchors of every read; n_match of every region"""
    tells = {"mapq": False, "esterr": False}
    for kernel, rs, bo in old:
        if tells[kernel]:
            continue
        if kernel == "mapq":
            B = A.prepare(rs, bo, opt=rs[0]["case"]["mapq"])
            out, _ = A.gather(B, variant)
            tells[kernel] = any(out[int(bo[k]):int(bo[k]) + R["a"].shape[0]].tobytes() != R["a"].tobytes() for k, R in enumerate(rs))
        else:
            rs = [{k: v for k, v in R.items() if k != "hits"} for R in rs]
            B = A.prepare(rs, bo)
            ff, _ = A.walk(B, B["b"], variant)
            nm = A.n_match(B, B["b"], ff)
            tells[kernel] = any(nm[k] != R["cnts"][:, 0].tolist() for k, R in enumerate(rs))
    return tells


CAUGHT_BY = {"memo_no_read": ["across_sq_sq", "across_copy_sq", "across_err_other"], "memo_le": ["memo_join256", "memo_adjoin256", "ewalk256", "memo_join512", "memo_adjoin512", "ewalk512"],
             "stale_flag": ["edge_absorbed_4096", "memo_join255"], "ignore_n_b_out": ["edge_dropped_4095", "edge_last_4096", "memo_adjoin513"],
             "step_once": ["boundary_empty1", "boundary_empty2"], "stride_minus_1": ["second_turn"], "stride_plus_1": ["second_turn"], "front_not_skipped": ["second_turn"],
             "read_lags_tab": ["across_err_k0"], "pred_minus_1": ["edge_rev_pred_4095", "ewalk257", "across_err_other"]}


def test_each_wrong_variant_is_caught_by_a_new_layout(ref):
    Ls = D.layouts()
    prepared = {}
    for L in Ls:
        prepared[L["name"]] = _batch(ref, L, n_b_cap=D.SECOND_TURN_CAP if L["name"] == "second_turn" else D.BY_READ_CAP if L["name"] == "by_read" else None)
    old = _old_batches()
    print()
    for v in A.VARIANTS:
        caught = [L["name"] for L in Ls if _check(*prepared[L["name"]], v) is not None]
        t = _old_tells(old, v)
        print(f"{v:18s} caught by {len(caught):2d} new layouts {caught[:6]}; old mapq_data batches: {'yes' if t['mapq'] else 'no'}; old esterr_data batches: {'yes' if t['esterr'] else 'no'}")
        if v == "search_first":
            assert not caught, "search_first changed an output: the lanes' own step no longer hides it -- move it into CAUGHT_BY"
            continue
        missing = [n for n in CAUGHT_BY[v] if n not in caught]
        assert not missing, f"{v}: not caught by {missing}"
    for e in (1, 2):                                                            # search_first lands elsewhere on the run of equal b_off at SLICE, and the lanes step to the same reads
        rs, B = prepared[f"boundary_empty{e}"]
        A.gather(B)
        right = dict(B["searched"])
        A.gather(B, "search_first")
        assert B["searched"][D.SLICE] == right[D.SLICE] - e and B["searched"][0] == right[0] - e == 0
