"""The shapes of tests/frag_data.py, asserted from the CPU model alone: tests/test_gpu_frag_e2e.py compares the library with the same model results, so it
cannot pass without the library having met a decision over more than 64 chains, ties in every lane layout, a compaction beyond one block, segment boundaries
inside repeats and a second pass of tens of thousands of anchors.  Nothing here calls the library."""
import numpy as np
import pytest

import frag_data as fd
import frag_model as fm
import sketch_model as sm


def _runs(flags):
    best = cur = 0
    for v in flags:
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


def _scores(u):
    return (u >> np.uint64(32)).astype(np.int64)


def _monotone_segments(cpu, res):
    """along every chain the segment number never comes back (frag_data's docstring): changes + 1 is the number of distinct segments, so a chain reading
    0,1,0 cannot be made from sequences; the decision's way of counting shows only in frag_model.n_chained_segs on hand patterns"""
    n = 0
    for r in res:
        for p in (r["first"], r):
            cnt = (p["u"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            off = 0
            for c in cnt:
                d = np.diff(fd.seg_ids(p["b"][off:off + c]))
                assert (d >= 0).all() or (d <= 0).all()
                off += int(c); n += 1
            if p["u"].size:
                assert fm.n_chained_segs(p["u"], p["b"]) == np.unique(fd.seg_ids(fd.best_chain(p["u"], p["b"])[2])).size
    return n


def test_n_chained_segs_counts_changes():
    def chain(segs):
        b = np.zeros((len(segs), 2), np.uint64)
        b[:, 1] = [(s << fm.SEG_SHIFT) | (15 << 32) | (100 + 20 * i) for i, s in enumerate(segs)]
        return np.array([50 << 32 | len(segs)], np.uint64), b
    assert fm.n_chained_segs(*chain([0, 1, 0])) == 3           # changes, not distinct segments
    assert fm.n_chained_segs(*chain([0, 0, 1])) == 2
    assert fm.n_chained_segs(*chain([0, 1, 2])) == 3
    assert fm.n_chained_segs(*chain([1])) == 1
    # the first of equal scores, and the anchors before it skipped
    u0, b0 = chain([0, 0, 0]); u1, b1 = chain([0, 1]); u2, b2 = chain([2, 2])
    u, b = np.concatenate([u2 - np.uint64(1 << 32), u0, u1]), np.concatenate([b2, b0, b1])
    assert fm.n_chained_segs(u, b) == 1 and fm.n_chained_segs(np.concatenate([u2 - np.uint64(1 << 32), u1, u0]), np.concatenate([b2, b1, b0])) == 2


def test_set_a_the_decision_at_wave_width():
    a = fd.get("a")
    res = a.run(True)
    assert sum(len(s) for s in a.refs) < 200_000
    for nm, r in zip(a.names, res):
        assert r["first"]["rep_len"] > 0, f"{nm}: the decision is only made with rep_len > 0"
        assert r["first"]["u"].size >= 65, f"{nm}: {r['first']['u'].size} chains"
    assert _monotone_segments(a, res) > 1000

    def best(name):
        f = a.by_name(name)["first"]
        i, sc, b = fd.best_chain(f["u"], f["b"])
        return i, sc, fd.seg_ids(b), f
    # the second trip of the score loop and a prefix over more than 64 entries of u
    for name, n_segs in (("best_hi", 2), ("three_best_hi", 3)):
        i, sc, seg, f = best(name)
        assert i >= 64 and f["u"].size >= 65 and (np.sort(_scores(f["u"]))[-2] < sc), (name, i)
        assert np.unique(seg).size == n_segs and not a.by_name(name)["rechained"]
    # the second trip of the loop over the segment changes
    i, sc, seg, f = best("change_63_64")
    assert seg.size >= 65 and seg[63] == 0 and seg[64] == 1 and (np.nonzero(np.diff(seg))[0] + 1).tolist() == [64]
    assert not a.by_name("change_63_64")["rechained"]
    i, sc, seg, f = best("change_late")
    assert seg.size >= 65 and (np.nonzero(np.diff(seg))[0] + 1).tolist()[0] > 64 and not a.by_name("change_late")["rechained"]
    i, sc, seg, f = best("three_plain")
    ch = (np.nonzero(np.diff(seg))[0] + 1).tolist()
    assert len(ch) == 2 and ch[0] >= 64 and ch[1] >= 128 and not a.by_name("three_plain")["rechained"]
    # the only change between anchors 0 and 1: the first trip's first lane
    i, sc, seg, f = best("change_0_1")
    assert seg.size >= 65 and (np.nonzero(np.diff(seg))[0] + 1).tolist() == [1] and not a.by_name("change_0_1")["rechained"]
    # ties: two chains of equal, strictly largest score, one over both segments and one inside segment 1; the first decides
    want = {"tie_lanes": lambda i, j: i < j < 64 and i % 64 != j % 64,
            "tie_same_lane": lambda i, j: j == i + 64,
            "tie_low_lane_later": lambda i, j: i < 64 <= j and j % 64 < i}
    first_is_whole = {}
    for name, ok in want.items():
        r = a.by_name(name)
        f = r["first"]
        sc = _scores(f["u"])
        top = np.nonzero(sc == sc.max())[0]
        assert top.size == 2 and ok(int(top[0]), int(top[1])), (name, top)
        spans = [np.unique(fd.seg_ids(fd.chain_of(f["u"], f["b"], int(t)))).size for t in top]
        assert sorted(spans) == [1, 2], (name, spans)
        first_is_whole[name] = spans[0] == 2
        assert r["rechained"] == (spans[0] < 2), name          # the other pick flips the decision
    assert set(first_is_whole.values()) == {True, False}, "both orders of the whole and the partial chain"
    # three segments: a best chain over 0,1 only and one over 0,2 only re-chain
    for name, reads in (("three_reads_0_1", [0, 1]), ("three_reads_0_2", [0, 2])):
        i, sc, seg, f = best(name)
        assert np.unique(seg).tolist() == reads and a.by_name(name)["rechained"], (name, np.unique(seg))
        assert a.by_name(name)["n_anchors"] > f["n_anchors"], "the second pass saw the motif's hits"
    assert [len(ids) for _, ids in a.groups] == [7, 4]
    for h, ids in a.groups:
        fd.chunk_bases_for([a.frags[g] for g in ids])
    # the order among equal x differs between the two sorts, the decision does not
    assert [r["rechained"] for r in a.run(False)] == [r["rechained"] for r in res]


def test_set_b_compaction_beyond_one_block():
    b = fd.get("b")
    res = b.run(True)
    flags = np.array([r["rechained"] for r in res])
    assert len(res) >= 600 and all(len(f) == 2 and all(100 <= len(s) <= 150 for s in f) for f in b.frags)
    assert flags.sum() > 256 and (~flags).sum() > 256, (int(flags.sum()), int((~flags).sum()))
    assert _runs(flags) >= 257 and _runs(~flags) >= 257 and flags[0] and flags[-1]
    assert sum(1 for r in res if r["first"]["rep_len"] > 0 and not r["rechained"]) >= 20, "unflagged fragments that the decision had to look at"
    assert sum(1 for r in res if r["rechained"] and r["first"]["u"].size == 0) >= 1 and sum(1 for r in res if r["rechained"] and r["first"]["u"].size) > 256
    # chunks of two or three fragments: with none, one and all of them flagged; and one of 300
    ch = fd.frag_chunks(b.frags, fd.chunk_bases_for(b.frags))
    per = {int(flags[r0:r1].sum()) == 0 for r0, r1 in ch}, {int(flags[r0:r1].sum()) == r1 - r0 for r0, r1 in ch}
    assert per[0] == {True, False} and per[1] == {True, False} and any(0 < flags[r0:r1].sum() < r1 - r0 for r0, r1 in ch)
    cb = sum(len(s) for f in b.frags[:300] for s in f)
    assert fd.frag_chunks(b.frags, cb)[0] == (0, 300)
    assert _monotone_segments(b, res) > 300


def test_set_c_segment_boundaries():
    c = fd.get("c")
    res = c.run(True)
    only_by_neighbour = touching = 0
    for g, (nm, r) in enumerate(zip(c.names, res)):
        f, segs = r["first"], c.frags[g]
        alone = [sm.collect_matches(fm.collect_minimizers([s], c.w, c.k), c.lookup, c.mid_occ) for s in segs]
        bits_alone = np.array([m[4] & 1 for a in alone for m in a[0]], np.int64)
        bits = (f["matches"]["seg_tandem"] & 1).astype(np.int64)
        assert bits.size == bits_alone.size
        kept_here = (bits == 1) & (bits_alone == 0) & (f["matches"]["n"] > 0)        # kept, with hits, tandem only through the other segment
        only_by_neighbour += int(kept_here.sum())
        if nm == "empty_middle":
            assert kept_here.sum() == 2 and set((f["matches"]["seg_tandem"][kept_here] >> 1).tolist()) == {0, 2}, "across the empty segment"
        # rep_len: never more or less than the segments' own (frag_data's docstring), but intervals of two segments that touch take the merging branch
        assert f["rep_len"] == sum(a[1] for a in alone), nm
        mini = r["mini"]
        rep = np.array([c.lookup(int(x) >> 8)[1] >= c.mid_occ for x in mini[:, 0]])
        assert rep.sum() == mini.shape[0] - f["matches"].size
        en = ((mini[:, 1] & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).astype(np.int64) + 1
        st = en - (mini[:, 0] & np.uint64(0xFF)).astype(np.int64)
        seg = (mini[:, 1] >> np.uint64(32)).astype(np.int64)
        i = np.nonzero(rep)[0]
        touching += int(((seg[i][1:] != seg[i][:-1]) & (st[i][1:] == en[i][:-1])).sum())
        if nm in ("array_and_member", "two_members"):
            assert rep.sum() > 64, (nm, int(rep.sum()))
    assert only_by_neighbour >= 6 and touching >= 2, (only_by_neighbour, touching)
    lens = [[len(s) for s in f] for f in c.frags]
    assert all(len(l) == 3 for l in lens) and any(l[1] == 0 for l in lens) and any(0 < l[1] < c.k for l in lens)
    assert all(2000 <= x <= 8000 for l in lens for x in l if x >= c.k)
    assert any(b"N" in s and b"n" in s for f in c.frags for s in [b"".join(f)]) and any(s[:1].islower() for f in c.frags for s in f if s)
    flags = [r["rechained"] for r in res]
    assert any(flags) and not all(flags)
    fd.chunk_bases_for(c.frags)
    _monotone_segments(c, res)


def test_set_d_nothing_to_seed_in_the_first_pass():
    d = fd.get("d")
    res = d.run(True)
    assert 150_000 <= len(d.refs[0]) <= 350_000 and (d.mid_occ, d.max_occ) == (1000, 5000) and d.groups[0][0] == (500, 300, 100, 25, 5000, 2, 25, 0, 2)
    deep = [r for nm, r in zip(d.names, res) if nm == "deep"]
    plain = [r for nm, r in zip(d.names, res) if nm == "plain"]
    assert len(deep) == 3 and len(plain) >= 4
    for r in deep:
        f = r["first"]
        assert f["n_anchors"] == 0 and f["u"].size == 0 and f["rep_len"] > 0 and r["rechained"] and not (f["matches"]["n"] > 0).any()
        assert 30_000 <= r["n_anchors"] <= 50_000 and r["n_anchors"] > 8192, r["n_anchors"]
        assert r["u"].size > 64
    for r in plain:
        assert not r["rechained"] and r["u"].size >= 1 and r["first"]["rep_len"] == 0


def test_set_e_hpc():
    a, c = fd.get("e_a"), fd.get("e_c")
    assert (a.k, a.w, a.hpc, c.k, c.w, c.hpc) == (19, 10, 1, 19, 10, 1)
    ra, rc = a.run(True), c.run(True)
    assert max(r["first"]["u"].size for r in ra) >= 65 and {r["rechained"] for r in ra} == {True, False} and all(r["first"]["rep_len"] > 0 for r in ra)
    assert max(fd.best_chain(r["first"]["u"], r["first"]["b"])[0] for r in ra) >= 64
    assert {r["rechained"] for r in rc} == {True, False} and all(r["first"]["rep_len"] > 0 for r in rc)
    assert max(r["mini"].shape[0] - r["first"]["matches"].size for r in rc) > 64, "repetitive minimizers"
