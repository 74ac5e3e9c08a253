"""tests/epilogue_limit_data.py does what it says: asserted from the oracle alone (ob.backtrack, ob.chain_fpv), without a GPU.  These are conditions on the inputs of
tests/test_gpu_epilogue_limits.py -- a limit input that does not reach its limit tests nothing.  Every case of the data module is checked: none is skipped or filtered.

The boundary numbers below are written out, not derived from the data module's constants; the constants themselves are compared with the kernel source once."""
import os
import re

import numpy as np

import epilogue_limit_data as ed
import oracle_binding as ob

U = np.uint64


def observed(case):
    """what the oracle's output says of a case: kept chains, their scores (the 32-bit field as int32) and lengths, equal neighbours among their first x"""
    u, b = ed.reference(case)
    score = (u >> U(32)).astype(np.uint32).view(np.int32)
    length = (u & U(0xffffffff)).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(length)[:-1])).astype(np.int64)
    x = b[first, 0]
    assert int(length.sum()) == b.shape[0] and np.all(x[1:] >= x[:-1])
    return dict(nk=int(u.size), score=score, length=length, first_x=x, ties=int((x[1:] == x[:-1]).sum()))


def check(name, **want):
    """the facts of a case against their recomputation and against the oracle, then against the numbers the caller wrote down"""
    c = ed.by_name(name)
    fa = c["facts"]
    f, p = c["f"].astype(np.int64), c["p"].astype(np.int64)
    assert f.size == p.size == c["a"].shape[0] == fa["n"] and np.all(p < np.arange(f.size)) and p.min() >= -1
    assert np.all(c["a"][1:, 0] >= c["a"][:-1, 0]) and np.unique(c["a"][:, 1]).size == f.size, name
    # v[] the slow way, an anchor at a time (chain.c:106-111); chain ends and their peaks as chain.c:349-367 finds them
    v = f.copy()
    for i in range(f.size):
        if p[i] >= 0:
            v[i] = max(v[i], v[p[i]])
    ends = np.setdiff1d(np.nonzero(v >= c["min_sc"])[0], p[p >= 0])
    assert ends.size == fa["nu"] and int(v[ends].max()) == fa["top"] and int(v[ends].min()) == fa["low"], name
    got = observed(c)
    assert got["nk"] == fa["nk"] and got["ties"] == fa["ties"], (name, got["nk"], got["ties"], fa)
    assert np.abs(f).max() <= 1 << 30
    for key, val in want.items():
        assert fa[key] == val, f"{name}: {key} is {fa[key]}, the case needs {val}"
    return c, got


def test_constants_mirror_the_kernel_source():
    src = open(os.path.join(ob.ROOT, "minimap2-fpga_amd", "csrc", "chain_epilogue.hip")).read()
    def const(name):
        return int(re.search(r"\b%s = (\d+)\b" % name, src).group(1))
    assert (ed.FUSE_S, ed.FUSE_L) == (const("FUSE_S"), const("FUSE_L")) == (5120, 7680)
    assert ed.ENDS_MAX == 2 * const("FNT") == 1024 and "nu <= 2 * FNT" in src
    assert ed.RANK_MAX == const("RANK_MAX") == 768 and ed.TS_MAX == const("TS_MAX") == 4096
    assert ed.W == 64 * const("K") == 256 and "W = 64 * K" in src
    assert ed.WIDE == 1 << 19 and "(1 << 19)" in src


def test_every_case_is_in_the_batch_and_in_a_pair():
    cases = ed.forest_cases()
    names = [c["name"] for c in cases]
    assert len(names) == 43 and sorted(n for pair in ed.PAIRS.values() for n in pair) == sorted(names)
    assert {n.split("/")[0] for n in names} == {"score_19", "score_nonpositive", "score_bytes", "ends_1024", "rank_768_by_key", "rank_768_general", "half_cap",
                                                "ties_4096", "chunk_256", "one_path", "third_cap"}
    sizes = [c["facts"]["n"] for c in cases]
    assert sizes != sorted(sizes) and sizes != sorted(sizes, reverse=True)
    off, a, f, p, task = ed.batch(cases, ed.EMPTY_AT)
    assert off.size - 1 == 46 and off[-1] == a.shape[0] == f.size == p.size == sum(sizes) < 200000
    empty = np.nonzero(np.diff(off) == 0)[0]
    assert empty.size == 3 and empty[0] > 0 and empty[-1] < 45 and np.all(np.diff(empty) > 1)
    for c, k in zip(cases, task):
        assert off[k] > 0 or k == 0
        assert np.array_equal(f[off[k]:off[k + 1]], c["f"]) and np.array_equal(a[off[k]:off[k + 1]], c["a"])
    assert ed.groups(cases) == [(1, -5), (1, 40), (2, -5), (2, 40)]


def test_score_19_straddles_the_one_word_key():
    tops = []
    for top, wide in ((524287, False), (524288, True), (524289, True)):
        c, got = check(f"score_19/top-{top}", top=top, nu=303, nk=302)
        assert c["facts"]["n"] < 5120 and c["facts"]["nu"] <= 1024 and c["facts"]["low"] >= 1
        assert (c["facts"]["top"] >= 1 << 19) == wide
        assert int(got["score"].max()) == top and int(got["score"].min()) == 40 == c["min_sc"]        # the kept branch scores exactly min_sc
        # the two branches stop at one anchor of the best chain, near 2^19
        f, p = c["f"], c["p"]
        best = int(np.argmax(f))
        on_best = set()
        j = best
        while j >= 0:
            on_best.add(j); j = int(p[j])
        heads = [i for i in range(f.size) if int(p[i]) in on_best and i not in on_best]
        assert len(heads) == 2 and p[heads[0]] == p[heads[1]] and int(f[p[heads[0]]]) == (1 << 19) - 2000
        ends, sc = ed.chain_ends(f, p, c["min_sc"])
        branch = sorted(int(s) - int(f[p[heads[0]]]) for e, s in zip(ends, sc) if e not in on_best and _root(p, e) == _root(p, best))
        assert branch == [39, 40], branch                                                            # one dropped, one kept
        assert 40 + int(f[p[heads[0]]]) not in got["score"]                                          # the kept chain reports the difference, not f[peak]
        tops.append(c)
    for c in tops[1:]:                                                                               # nothing but the best peak's f differs
        assert np.array_equal(c["p"], tops[0]["p"]) and np.array_equal(c["a"], tops[0]["a"]) and int((c["f"] != tops[0]["f"]).sum()) == 1


def _root(p, i):
    while p[i] >= 0:
        i = int(p[i])
    return int(i)


def test_score_nonpositive_has_a_zero_a_negative_and_a_peak_listed_twice():
    for min_cnt, nk in ((2, 33), (1, 34)):
        c, got = check(f"score_nonpositive/min_cnt-{min_cnt}", nu=34, nk=nk, low=-2)
        assert c["min_sc"] == -5 and c["min_cnt"] == min_cnt
        ends, sc = ed.chain_ends(c["f"], c["p"], -5)
        assert 0 in sc and -2 in sc and (sc > 0).sum() >= 30 and -10 not in sc and -10 in c["f"]
        assert 0 in got["score"] and -2 in got["score"]
        # two chain ends under one peak: both have v = f[peak] = 50 and f below it
        twice = [int(e) for e, s in zip(ends, sc) if c["f"][e] < s]
        assert len(twice) == 2 and c["p"][twice[0]] == c["p"][twice[1]] and int(c["f"][c["p"][twice[0]]]) == 50
        peak = c["a"][c["p"][twice[0]]]
        assert int(((got["length"] == 2) & (got["score"] == 50)).sum()) == 1                         # the first listing: the peak and its root
        # min_cnt = 1: the second listing is a chain of the peak alone, scored f[peak] - f[parent] = 30; min_cnt = 2: only the first listing survives
        alone = (got["length"] == 1) & (got["score"] == 30) & (got["first_x"] == peak[0])
        assert int(alone.sum()) == (1 if min_cnt == 1 else 0)
    assert np.array_equal(ed.by_name("score_nonpositive/min_cnt-2")["f"], ed.by_name("score_nonpositive/min_cnt-1")["f"])


def test_score_bytes_differ_in_every_byte_of_the_score():
    for C, over in ((700, False), (1100, True)):
        c, got = check(f"score_bytes/chains-{C}", nu=C, nk=C, top=1 << 30)
        assert (64 < C <= 768) != over and (C > 1024) == over
        for b in (8, 16, 19, 24, 30):
            assert (1 << b) - 1 in got["score"] and (1 << b) in got["score"], (C, b)
        sc = got["score"].astype(np.int64)
        diff = int(np.bitwise_or.reduce(sc) ^ np.bitwise_and.reduce(sc))
        assert all((diff >> s) & 255 for s in (0, 8, 16, 24)), hex(diff)
        assert 100 in sc and (1 << 30) - 400 not in sc                                               # the branch off the path of 2^30: a difference of two large f


def test_ends_1024_and_1025():
    for C in (1024, 1025):
        c, _ = check(f"ends_1024/all-kept-{C}", nu=C, nk=C)
        assert c["facts"]["top"] < 1 << 19 and c["facts"]["low"] >= 1 and c["facts"]["n"] <= 5120
        c, got = check(f"ends_1024/few-kept-{C}", nu=C, nk=25)
        assert c["facts"]["top"] < 1 << 19 and c["facts"]["low"] >= 1 and c["min_cnt"] == 2 and np.all(got["length"] == 12)


def test_rank_768_and_769_in_both_forms():
    for C in (768, 769):
        c, got = check(f"rank_768_by_key/{C}", nu=C, nk=C, ties=0)
        assert c["facts"]["top"] < 1 << 19 and c["facts"]["low"] >= 1 and np.unique(got["first_x"]).size == C
        c, got = check(f"rank_768_general/{C}", nu=C, nk=C, ties=0)
        assert c["facts"]["top"] >= 1 << 19 and int((got["score"] >= 1 << 19).sum()) == 1 and c["facts"]["n"] <= 5120


def test_half_cap_in_both_classes():
    for nu, n in ((2560, 5120), (2561, 5120), (3840, 7680), (3841, 7680)):
        c, _ = check(f"half_cap/nu-{nu}-n-{n}", nu=nu, nk=nu, n=n)
        assert c["facts"]["top"] < 1 << 19                        # the general form by the number of chain ends alone
    assert 2 * 2560 == 5120 and 2 * 3840 == 7680                  # CAP / 2 of the two classes


def test_third_cap_in_both_classes():
    for nk, n in ((1706, 3412), (1707, 3414), (2560, 5121), (2561, 5122)):
        c, _ = check(f"third_cap/nk-{nk}-n-{n}", nu=nk, nk=nk, n=n)
        assert nk > 1024 and c["facts"]["top"] < 1 << 19          # the general form, by the number of chain ends
    assert 5120 // 3 == 1706 and 7680 // 3 == 2560 and 3414 <= 5120 < 5121


def test_ties_4096_and_4097_are_reordered_by_the_reference():
    for name, nk, n in (("a-fused-4096", 4096, 7680), ("a-fused-4097", 4097, 7680), ("b-chunked-4096", 4096, 8192), ("b-chunked-4097", 4097, 8194),
                        ("c-roots-4097", 4097, 4097)):
        c, got = check(f"ties_4096/{name}", nu=nk, nk=nk, n=n, ties=2048)
        assert c["min_cnt"] == 1 and (n > 7680) == name.startswith("b")
        # a stable sort of the chains in rank order would put the better chain of every pair first: the reference does not (ksort.h:101-151)
        pair = np.nonzero(got["first_x"][1:] == got["first_x"][:-1])[0]
        assert np.all(np.diff(pair) > 1)                          # pairs, no longer runs
        worse_first = int((got["score"][pair] < got["score"][pair + 1]).sum())
        assert 0 < worse_first < pair.size, f"{name}: a stable sort would pass ({worse_first} of {pair.size} pairs)"


def test_chunk_256_sizes_and_links():
    for n in (255, 256, 257, 511, 512, 513):
        c, got = check(f"chunk_256/path-{n}", n=n, nu=1, nk=1)
        assert np.array_equal(c["p"], np.arange(n) - 1) and got["length"][0] == n
    for C in (255, 256, 257):
        c, got = check(f"chunk_256/link-{C}", nu=C, nk=C, n=5 * C)
        p = c["p"]
        assert np.all(p[:C] == -1) and np.array_equal(p[C:], np.arange(C, 5 * C) - C)         # every link is exactly i - C
        assert np.all(got["length"] == 5)


def test_one_path_of_5120_to_7681():
    for n in (5120, 5121, 7680, 7681):
        c, got = check(f"one_path/{n}", n=n, nu=1, nk=1)
        assert np.array_equal(c["p"], np.arange(n) - 1) and got["length"][0] == n and 1 <= c["facts"]["top"] < 1 << 19
    for n in (5120, 7680):
        c, got = check(f"one_path/{n}-wide", n=n, nu=1, nk=1, top=(1 << 19) + n)
        assert np.array_equal(c["p"], np.arange(n) - 1) and got["length"][0] == n


def test_dp_score_19_crosses_2_to_the_19_in_the_real_dp():
    P, tasks = ed.dp_score_19()
    assert [t.shape[0] for t in tasks] == [2056, 2057, 300, 2058]
    for t, want in zip((tasks[0], tasks[1], tasks[3]), (524280, 524535, 524790)):
        f, p, v = ob.chain_fpv(P, t)
        assert int(f.max()) == 255 * t.shape[0] == want
        assert np.array_equal(p, np.arange(t.shape[0]) - 1)
    assert 524280 < 1 << 19 <= 524535
    f, _, _ = ob.chain_fpv(P, tasks[2])
    assert 0 < int(f.max()) < 1 << 19
    u, b = ob.mm_chain_dp(P, 3, 40, tasks[1])
    assert u.size == 1 and int(u[0] >> U(32)) == 524535 and int(u[0] & U(0xffffffff)) == 2057
