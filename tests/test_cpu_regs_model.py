"""tests/regs_model.py against the reference's own mm_gen_regs (tests/golden/ref_regs.npz: every byte of every mm_reg1_t, every read hash), and -- from the model alone --
that every family of tests/regs_data.py reaches the boundary it is there for."""
import os

import numpy as np
import pytest

import regs_data as D
import regs_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_regs.npz"))


@pytest.fixture(scope="module")
def model():
    return {c["name"]: M.gen_regs(c["hash"], c["qlen"], c["u"], c["a"]) for c in D.cases()}


def by_name(name):
    return next(c for c in D.cases() if c["name"] == name)


def test_model_reproduces_every_byte_of_the_reference(ref, model):
    cs = D.cases()
    assert [c["name"] for c in cs] == [str(n) for n in ref["names"]] and int(ref["reg_size"]) == M.REG.itemsize
    off = ref["reg_off"]
    for k, c in enumerate(cs):
        want = ref["regs"][off[k]:off[k + 1]].reshape(-1).view(M.REG)
        got = model[c["name"]]
        assert got.size == want.size == c["u"].size
        bad = [i for i in range(got.size) if got[i].tobytes() != want[i].tobytes()]
        assert not bad, f"{c['name']}: region {bad[0]}:\n got {got[bad[0]]}\nwant {want[bad[0]]}"
    assert int(ref["n_tie_reads"]) == M.n_tie_reads(cs)


def test_model_reproduces_every_read_hash(ref):
    assert [M.read_hash(*h) for h in D.HASH_CASES] == [int(h) for h in ref["hashes"]]
    assert len({int(h) for h in ref["hashes"]}) >= len(D.HASH_CASES) - 1 and D.HASH_CASES[0][0] is None and any(n and max(n) > 127 for n, _, _ in D.HASH_CASES)


def test_cases_are_deterministic_and_consistent():
    a = D.cases()
    D._CASES = None
    b = D.cases()
    assert len(a) == len(b) and all(x["name"] == y["name"] and x["hash"] == y["hash"] and np.array_equal(x["u"], y["u"]) and np.array_equal(x["a"], y["a"]) for x, y in zip(a, b))
    for c in a:
        cnt = (c["u"] & np.uint64(0xffffffff)).astype(np.int64)
        assert (cnt >= 1).all() and cnt.sum() == c["a"].shape[0], c["name"]


def test_small_counts_and_real_chains():
    names = [c["name"] for c in D.cases()]
    assert sum(n.startswith("frag") for n in names) >= 8 and sum(n.startswith("testdata") for n in names) >= 3
    assert by_name("no_chains")["u"].size == 0 and by_name("one_chain")["u"].size == 1 and int(by_name("cnt1")["u"][0]) & 0xffffffff == 1


def test_fill_pass_boundaries_are_met():
    """one chain on each side of every boundary, in the batch (where a case starts wherever the cases before it end) and alone (where it starts at anchor 0)"""
    cnts = lambda n: [int(v) & 0xffffffff for v in by_name(n)["u"]]
    assert {2, 63, 64, 65, 128, 129} <= set(cnts("rows"))
    assert {D.FILL_GROUP - 1, D.FILL_GROUP, D.FILL_GROUP + 1} <= set(cnts("row_groups"))
    assert {D.FILL_SLICE - 1, D.FILL_SLICE, D.FILL_SLICE + 1} <= set(cnts("slice_exact")) and cnts("slice_exact")[0] == D.FILL_SLICE   # alone: ends exactly with slice 0
    assert cnts("slice_minus")[:2] == [D.FILL_SLICE - 1, 2]                                   # alone: the second chain crosses from slice 0 into slice 1
    assert {D.FILL_BLOCK - 1, D.FILL_BLOCK, D.FILL_BLOCK + 1} <= set(cnts("block"))
    assert cnts("long_chain")[0] > 19 * D.FILL_SLICE and max(cnts("long_between")) == 20000
    # in the batch: chains that lie inside one slice, chains that cross one boundary, chains that cover whole slices
    u_off, u, b_off, b, _, _ = D.batch(D.cases())
    start = np.concatenate([[0], np.cumsum((u & np.uint64(0xffffffff)).astype(np.int64))])
    first, last = start[:-1] // D.FILL_SLICE, (start[1:] - 1) // D.FILL_SLICE
    assert (first == last).sum() > 1000 and (last == first + 1).sum() > 20 and (last > first + 1).sum() >= 5    # (the three of "block", the two long ones)
    assert (start[:-1] % D.FILL_SLICE == 0).any() and (start[1:] % D.FILL_ROW == 0).any()


def test_sort_sizes_are_met():
    for n in (D.RS_MIN, D.RS_MIN + 1):
        c = by_name(f"sort{n}")
        zx = [e[0] for e in M.keys(c["hash"], c["u"], c["a"])]
        assert len(zx) == n == len(set(zx))
    assert [by_name(f"ties{n}")["u"].size for n in (64, 65, 300, D.TS_MAX, D.TS_MAX + 1)] == [64, 65, 300, D.TS_MAX, D.TS_MAX + 1]


def test_planted_ties_need_the_references_sort(model):
    """every tie read holds pairs, a triple, and for each of the 8 bytes two keys that differ in that byte only; above 64 chains a stable sort gives another array
    than klib's, up to 64 the same one"""
    for n in (64, 65, 300, D.TS_MAX, D.TS_MAX + 1):
        c = by_name(f"ties{n}")
        zx = np.array([e[0] for e in M.keys(c["hash"], c["u"], c["a"])], np.uint64)
        vals, counts = np.unique(zx, return_counts=True)
        assert (counts == 2).sum() >= 3 and (counts >= 3).sum() >= 1
        x = vals[:, None] ^ vals[None, :]
        for byte in range(8):
            only = (x != 0) & ((x & ~(np.uint64(0xff) << np.uint64(8 * byte))) == 0)
            assert only.any(), f"ties{n}: no two keys differ in byte {byte} alone"
        first = c["a"][np.concatenate([[0], np.cumsum((c["u"] & np.uint64(0xffffffff)).astype(np.int64))[:-1]])]
        same_key = [np.nonzero(zx == v)[0] for v in vals[counts >= 2]]
        assert any(not (first[g] == first[g][0]).all() for g in same_key), "no equal keys from different first anchors"
        stable = M.gen_regs(c["hash"], c["qlen"], c["u"], c["a"], sort=M.stable_sort)
        if n <= D.RS_MIN:
            assert stable.tobytes() == model[c["name"]].tobytes()
        elif n != D.RS_MIN + 1:
            assert stable.tobytes() != model[c["name"]].tobytes(), f"ties{n}: a stable sort gives the reference's order -- the planted ties show nothing"
    # 64 chains: the later of two equal chains comes first after the reversal
    c = by_name("ties64")
    zx = [e[0] for e in M.keys(c["hash"], c["u"], c["a"])]
    as_of = np.concatenate([[0], np.cumsum((c["u"] & np.uint64(0xffffffff)).astype(np.int64))[:-1]])
    r = model["ties64"]
    pos = {int(a): i for i, a in enumerate(r["as"])}
    i, j = next((i, j) for i in range(64) for j in range(i + 1, 64) if zx[i] == zx[j])
    assert pos[int(as_of[j])] < pos[int(as_of[i])]


def test_coordinate_and_fuzzy_length_cases_reach_their_branches(model):
    for rev in (0, 1):
        rs = [int(model[f"rs_clamp_rev{rev}_{d}"]["rs"][0]) for d in (-1, 0, 1)]
        assert rs == [0, 0, 1] and int(model[f"rs_clamp_rev{rev}_0"]["flags"][0]) == rev << 10
    r = model["low_word_sign"]
    assert sorted(int(v) for v in r["re"]) == [-(1 << 31) + 0x41, -7]          # (int32_t) of 0x80000040 + 1 and of 0xfffffff8 + 1
    a = by_name("low_word_sign")["a"]
    xl = a[:, 0].astype(np.uint32).view(np.int32).astype(np.int64)
    assert 0x7fffffff in xl and -(1 << 31) in xl and (np.diff(xl[4:]) < 0).any()   # the low word crosses 2^31 inside a chain; a negative tl without overflow
    assert (model["rid_all_ones"]["rid"] == 0x7fffffff).all() and sorted(int(f) for f in model["rid_all_ones"]["flags"]) == [0, 1 << 10]
    a = by_name("fuzzy_branches")["a"]
    tl = np.diff(a[:, 0].astype(np.int64) & 0xffffffff); ql = np.diff(a[:, 1].astype(np.int64) & 0xffffffff)
    span = 15
    assert (tl > ql).any() and (tl == ql).any() and (tl < ql).any()
    for v in (span, span + 1):
        assert ((tl == v) & (ql > span + 1)).any() and ((ql == v) & (tl > span + 1)).any() and ((tl == v) & (ql == v)).any()
    assert {c["hash"] for c in D.cases()} >= {0, 0xffffffff}
    assert any((c["a"][:, 0] >> np.uint64(63)).any() for c in D.cases()) and any(not (c["a"][:, 0] >> np.uint64(63)).all() for c in D.cases())
