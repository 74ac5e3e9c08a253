"""GPU tests of the batched seeds-to-chains path with skip_seed (map.c:122-147): -x ava-ont (NO_DIAG | NO_DUAL) and the strand-restricted modes through the
host-buffer entries (mm2c_seed_hits_batch_host_skip, mm2c_seed_chain_batch_host_skip / _pool_skip), and the sixteen-wave expansion of long reads with skip_seed
(seed_expand_mw<16, true>).  Against the anchor lists of the reference's own map.o (tests/golden/ref_seed_hits_ava.npz) and against the oracle's
collect_seed_hits + mm_chain_dp."""
import os

import numpy as np
import pytest
import torch

import oracle_binding as ob

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AVA = ob.F_NO_DIAG | ob.F_NO_DUAL


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def _batch(reads):
    """reads: list of (qlen, matches with read-local cr_off, hits) -> one CSR batch with a shared hit pool"""
    mo, ms, hs, ql, base = [0], [], [], [], 0
    for qlen, m, hits in reads:
        m = np.array(m, dtype=ob.MATCH_DTYPE, copy=True)
        m["cr_off"] += base
        base += hits.size
        ms.append(m); hs.append(np.asarray(hits, np.uint64)); ql.append(qlen); mo.append(mo[-1] + m.size)
    return (np.array(mo, np.int64), np.concatenate(ms) if ms else np.zeros(0, ob.MATCH_DTYPE),
            np.concatenate(hs) if hs else np.zeros(0, np.uint64), np.array(ql, np.int32))


def _random_read(rng, n_matches, max_n, rid_count, pos_range, qlen=12000, dup_frac=0.0):
    """matches with random hit lists; dup_frac > 0 (the same hit list under two query minimizers) makes anchors with equal x"""
    m = np.zeros(n_matches, ob.MATCH_DTYPE)
    m["n"] = rng.integers(0, max_n + 1, n_matches)
    m["q_pos"] = (np.sort(rng.integers(15, qlen, n_matches)).astype(np.uint32) << 1) | rng.integers(0, 2, n_matches).astype(np.uint32)
    m["q_span"] = 15
    m["seg_tandem"] = rng.integers(0, 2, n_matches)
    lists = []
    for k in range(n_matches):
        n = int(m["n"][k])
        if k > 0 and dup_frac > 0 and rng.random() < dup_frac and lists[-1].size == n:
            lists.append(lists[-1].copy())
            continue
        rid = rng.integers(0, rid_count, n).astype(np.uint64)
        pos = np.sort(rng.integers(0, pos_range, n)).astype(np.uint64)
        lists.append((rid << np.uint64(32)) | (pos << np.uint64(1)) | rng.integers(0, 2, n).astype(np.uint64))
    m["n"] = [x.size for x in lists]
    m["cr_off"] = np.concatenate([[0], np.cumsum(m["n"].astype(np.int64))[:-1]])
    return qlen, m, (np.concatenate(lists) if lists else np.zeros(0, np.uint64))


def _capacity(mo, m):
    return np.concatenate([[0], np.cumsum([int(m["n"][mo[k]:mo[k + 1]].sum()) for k in range(mo.size - 1)])]).astype(np.int64)


def _fixture():
    d = np.load(os.path.join(GOLDEN, "ref_seed_hits_ava.npz"))
    n = int(d["n_reads"])
    reads = [(int(d[f"r{k}_qlen"]), d[f"r{k}_matches"], d[f"r{k}_hits"]) for k in range(n)]
    q_lo = np.array([int(d[f"r{k}_qlo"]) for k in range(n)], np.int32)
    q_eq = np.array([int(d[f"r{k}_qeq"]) for k in range(n)], np.int32)
    h = [int(v) for v in d["chain_scalars"]]
    from mm2chain import params
    P = params.make_params(h[0], h[1], h[2], h[3], h[4], 1.0, h[7], h[8])
    return d, reads, q_lo, q_eq, P, h[5], h[6]


def test_all_vs_all_fixture_through_the_host_entries():
    """the 37 reads of map.o mapped against themselves (-x ava-ont): anchors per read equal the reference's, anchor_off holds the kept counts, chains equal
    mm_chain_dp on the reference's anchors"""
    import mm2chain
    d, reads, q_lo, q_eq, P, min_cnt, min_sc = _fixture()
    mo, m, h, ql = _batch(reads)
    skip = mm2chain.SeedSkip(int(d["flag"]), d["ref_rank"], d["ref_len"], q_lo, q_eq)
    ao, a = mm2chain.seed_hits_batch_skip(mo, m, h, ql, skip)
    kept = [d[f"r{k}_anchors"].shape[0] for k in range(len(reads))]
    assert np.array_equal(np.diff(ao), kept)
    for k in range(len(reads)):
        assert np.array_equal(a[ao[k]:ao[k + 1]], d[f"r{k}_anchors"]), f"read {k}: anchors differ"
    ao2, res = mm2chain.seed_chain_batch_skip(P, min_cnt, min_sc, mo, m, h, ql, skip)
    assert np.array_equal(ao2, ao)
    n_chains = 0
    for k in range(len(reads)):
        u_ref, b_ref = ob.mm_chain_dp(P, min_cnt, min_sc, d[f"r{k}_anchors"])
        assert np.array_equal(res[k][0], u_ref) and np.array_equal(res[k][1], b_ref), f"read {k}: chains differ"
        n_chains += u_ref.size
    assert n_chains >= 20 and int(ao[-1]) < int(_capacity(mo, m)[-1]) // 4


@pytest.mark.parametrize("mode", ["host-pool-ranges", "host-pool-shared", "resident-pool"])
def test_all_vs_all_pipelined_in_chunks(mode):
    """the fixture six times over, in at least ten chunks of whole reads on the two-stream pipeline: hits uploaded per chunk as ranges, once as a whole (reads shuffled
    against the pool) or resident (mm2c_seed_chain_batch_pool_skip); the packed offsets of every chunk placed behind the chunks before.  Twice, both against the oracle."""
    import mm2chain
    d, base, q_lo1, q_eq1, P, min_cnt, min_sc = _fixture()
    ref_anchors = [d[f"r{k}_anchors"] for k in range(len(base))] * 6
    reads = base * 6
    q_lo, q_eq = np.tile(q_lo1, 6), np.tile(q_eq1, 6)
    mo, m, h, ql = _batch(reads)
    if mode == "host-pool-shared":
        order = np.random.default_rng(5).permutation(len(reads))
        cnt = np.diff(mo)
        m = np.concatenate([m[mo[k]:mo[k + 1]] for k in order])
        mo = np.concatenate([[0], np.cumsum(cnt[order])]).astype(np.int64)
        ql, q_lo, q_eq = ql[order], q_lo[order], q_eq[order]
        ref_anchors = [ref_anchors[k] for k in order]
    skip = mm2chain.SeedSkip(int(d["flag"]), d["ref_rank"], d["ref_len"], q_lo, q_eq)
    total = int(_capacity(mo, m)[-1])
    mm2chain.stage_stats(reset=True)
    with mm2chain.tuned(pipeline_chunk_anchors=max(1024, total // 14)):
        if mode == "resident-pool":
            pool = mm2chain.HitPool(h)
            out = [mm2chain.seed_chain_batch_pool_skip(P, min_cnt, min_sc, mo, m, pool, ql, skip) for _ in range(2)]
            pool.close()
        else:
            out = [mm2chain.seed_chain_batch_skip(P, min_cnt, min_sc, mo, m, h, ql, skip) for _ in range(2)]
    st = mm2chain.stage_stats()
    assert st["calls"] == 2 and st["chunks"] >= 20 and st["seed_ns"] > 0 and st["dp_ns"] > 0 and st["epi_ns"] > 0 and st["total_ns"] > 0, st
    kept = np.array([r.shape[0] for r in ref_anchors])
    for call, (ao, res) in enumerate(out):
        assert np.array_equal(np.diff(ao), kept), f"{mode}: call {call}: anchor offsets"
        for k, ra in enumerate(ref_anchors):
            u_ref, b_ref = ob.mm_chain_dp(P, min_cnt, min_sc, ra)
            assert np.array_equal(res[k][0], u_ref) and np.array_equal(res[k][1], b_ref), f"{mode}: call {call}, read {k}: chains differ"


N_REF = 8


def _long_batch():
    """short reads, reads without hits, and four reads beyond 16 384 hits (one beyond 10^5; match counts that are no multiple of 64, a long run of matches without
    hits, one match with thousands of hits); rids over N_REF references, the reads' names placed among them so that the name comparison gives < 0, == 0 and > 0,
    hits on the diagonal of the reads whose name is a reference of their length"""
    rng = np.random.default_rng(2024)
    reads = [_random_read(rng, 300, 5, N_REF, 1 << 20, qlen=12000),
             _random_read(rng, 9001, 6, N_REF, 1 << 24, qlen=120000, dup_frac=0.1),
             _random_read(rng, 0, 0, 1, 10),
             _random_read(rng, 2500, 8, N_REF, 1 << 22, qlen=40000),
             _random_read(rng, 40001, 7, N_REF, 1 << 26, qlen=200000, dup_frac=0.05),
             _random_read(rng, 7003, 8, N_REF, 1 << 23, qlen=90000)]
    qlen, m, h = _random_read(rng, 6000, 9, N_REF, 1 << 25, qlen=100000)
    lists = [h[int(c):int(c) + int(n)] for c, n in zip(m["cr_off"], m["n"])]
    for k in range(1000, 2500):
        lists[k] = lists[k][:0]                                                     # 1 500 matches in a row without a hit
    lists[4000] = (np.uint64(3) << np.uint64(32)) | (np.sort(rng.integers(0, 1 << 25, 7000)).astype(np.uint64) << np.uint64(1))   # one minimizer with 7 000 hits
    m = m.copy(); m["n"] = [x.size for x in lists]; m["cr_off"] = np.concatenate([[0], np.cumsum(m["n"].astype(np.int64))[:-1]])
    reads.insert(4, (qlen, m, np.concatenate(lists)))
    m0 = np.zeros(50, ob.MATCH_DTYPE); m0["q_pos"] = np.arange(50) * 20; m0["q_span"] = 15
    reads.insert(2, (5000, m0, np.zeros(0, np.uint64)))                             # matches, none with a hit
    ref_rank = rng.permutation(N_REF).astype(np.int32)
    ref_len = rng.integers(1000, 300000, N_REF).astype(np.int32)
    n = len(reads)
    q_lo = rng.integers(0, N_REF + 1, n).astype(np.int32); q_eq = np.zeros(n, np.int32)
    rid_of_rank = np.argsort(ref_rank)
    for r, own in ((1, 0), (4, 3), (5, 5), (6, 7), (7, 2)):                        # these reads are named as a reference of their own length
        rid = int(rid_of_rank[own]); q_lo[r] = own; q_eq[r] = 1; ref_len[rid] = reads[r][0]
        qlen, m, h = reads[r]
        h = h.copy()
        sel = np.nonzero(m["n"] > 0)[0][::17]
        qpos = (m["q_pos"][sel] >> 1).astype(np.uint64)
        h[m["cr_off"][sel]] = (np.uint64(rid) << np.uint64(32)) | (qpos << np.uint64(1)) | (m["q_pos"][sel] & 1).astype(np.uint64)   # the diagonal
        sel = np.nonzero(m["n"] > 0)[0][8::17]
        qpos = (m["q_pos"][sel] >> 1).astype(np.uint64) + np.uint64(1000)
        h[m["cr_off"][sel]] = (np.uint64(rid) << np.uint64(32)) | (qpos << np.uint64(1)) | (m["q_pos"][sel] & 1).astype(np.uint64)   # beside it: chains
        reads[r] = (qlen, m, h)
    return reads, ref_rank, ref_len, q_lo, q_eq


def test_long_reads_with_every_skip_flag_on_sixteen_waves_and_on_one(monkeypatch):
    """every flag (ava-ont's pair, each alone, FOR_ONLY, REV_ONLY, none, and no names at all) on a batch with long reads: anchors against the oracle's collect_seed_hits with
    the same flags, chains against mm_chain_dp on them; MM2C_MW_SORT=1 and =0 alike, and with =1 the long reads are expanded on sixteen waves"""
    import mm2chain
    from mm2chain import params
    reads, ref_rank, ref_len, q_lo, q_eq = _long_batch()
    mo, m, h, ql = _batch(reads)
    cap = _capacity(mo, m)
    sizes = np.diff(cap)
    assert (sizes > 16384).sum() >= 3 and sizes.max() > 100000 and (sizes == 0).sum() >= 2, sizes
    cmp = [np.sign(np.where(ref_rank < q_lo[r], 1, np.where((ref_rank == q_lo[r]) & (q_eq[r] == 1), 0, -1))) for r in range(len(reads))]
    assert {-1, 0, 1} <= set(np.concatenate(cmp).tolist())
    P = params.map_ont()
    d_m = torch.from_numpy(m.view(np.uint8).copy()).cuda(); d_h = torch.from_numpy(h.view(np.int64)).cuda(); d_q = torch.from_numpy(ql).cuda()
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()
    configs = [(AVA, True), (ob.F_NO_DIAG, True), (ob.F_NO_DUAL, True), (ob.F_FOR_ONLY, True), (ob.F_REV_ONLY, True), (0, True), (AVA, False)]
    n_dropped = {}
    for flag, names in configs:
        rr, rl, lo, eq = (ref_rank, ref_len, q_lo, q_eq) if names else (None, None, None, None)
        skip = mm2chain.SeedSkip(flag, rr, rl, lo, eq)
        refs = [ob.collect_seed_hits(mr, hr, qlen, flag, rr, rl, int(lo[k]) if names else 0, int(eq[k]) if names else 0) for k, (qlen, mr, hr) in enumerate(reads)]
        chains = [ob.mm_chain_dp(P, 3, 40, a) for a in refs]
        got = {}
        for mw in ("1", "0"):
            monkeypatch.setenv("MM2C_MW_SORT", mw)                                  # read when a seed plan is made
            what = f"flag {flag:#x}{'' if names else ' without names'}, MM2C_MW_SORT={mw}"
            ao, a = mm2chain.seed_hits_batch_skip(mo, m, h, ql, skip)
            ao2, res = mm2chain.seed_chain_batch_skip(P, 3, 40, mo, m, h, ql, skip)
            assert np.array_equal(ao, ao2), what
            for k, ref in enumerate(refs):
                assert np.array_equal(a[ao[k]:ao[k + 1]], ref), f"{what}: read {k}: {ao[k + 1] - ao[k]} anchors, the oracle keeps {ref.shape[0]}"
                assert np.array_equal(res[k][0], chains[k][0]) and np.array_equal(res[k][1], chains[k][1]), f"{what}: read {k}: chains differ"
            sp = mm2chain.SeedPlan(mo, cap)                                         # the device entry: which kernel expanded the long reads
            d_a, d_off = sp.run_skip(d_m, d_h, d_q, flag, dev(rr), dev(rl), dev(lo), dev(eq))
            sp.check()
            assert np.array_equal(d_off.cpu().numpy(), ao), what
            assert np.array_equal(d_a.cpu().numpy().view(np.uint64)[:ao[-1]], a), what
            n_mw = sp.last_expand_mw()
            assert n_mw == (int((sizes > 16384).sum()) if mw == "1" else 0), f"{what}: {n_mw} reads expanded on sixteen waves"
            sp.close()
            got[mw] = (ao, a, res)
        assert np.array_equal(got["1"][0], got["0"][0]) and np.array_equal(got["1"][1], got["0"][1])
        n_dropped[(flag, names)] = int(cap[-1] - got["1"][0][-1])
    assert n_dropped[(0, True)] == 0 and n_dropped[(AVA, False)] == 0
    assert min(n_dropped[(f, True)] for f in (AVA, ob.F_NO_DIAG, ob.F_NO_DUAL, ob.F_FOR_ONLY, ob.F_REV_ONLY)) > 0, n_dropped
    assert n_dropped[(AVA, True)] > n_dropped[(ob.F_NO_DUAL, True)] > n_dropped[(ob.F_NO_DIAG, True)], n_dropped


def test_heap_sort_with_skip_seed_through_the_host_entries():
    """mm2c_tune("heap_sort", 1): the plans of the skip entries leave collect_seed_hits_heap's order (map.c:149-213) among equal x, long reads included"""
    import mm2chain
    from mm2chain import params
    rng = np.random.default_rng(77)
    reads = [_random_read(rng, 400, 6, 3, 5000, qlen=20000, dup_frac=0.3), _random_read(rng, 7001, 6, 3, 1 << 16, qlen=80000, dup_frac=0.2),
             _random_read(rng, 1500, 5, 3, 20000, qlen=30000, dup_frac=0.3)]
    for qlen, mr, hr in reads:                                                  # hit lists ascending, as mm_idx_get hands them out: the heap then pops x in order
        for c, n in zip(mr["cr_off"], mr["n"]):
            hr[int(c):int(c) + int(n)].sort()
    mo, m, h, ql = _batch(reads)
    assert np.diff(_capacity(mo, m)).max() > 16384
    ref_rank = np.array([2, 0, 1], np.int32); ref_len = np.array([20000, 80000, 5], np.int32)
    q_lo = np.array([2, 0, 1], np.int32); q_eq = np.array([1, 1, 0], np.int32)
    skip = mm2chain.SeedSkip(AVA, ref_rank, ref_len, q_lo, q_eq)
    P = params.map_ont()
    with mm2chain.tuned(heap_sort=1):
        ao, a = mm2chain.seed_hits_batch_skip(mo, m, h, ql, skip)
        ao2, res = mm2chain.seed_chain_batch_skip(P, 3, 40, mo, m, h, ql, skip)
    n_ties = 0
    for k, (qlen, mr, hr) in enumerate(reads):
        ref = ob.collect_seed_hits(mr, hr, qlen, AVA, ref_rank, ref_len, int(q_lo[k]), int(q_eq[k]), heap=True)
        assert np.array_equal(a[ao[k]:ao[k + 1]], ref), f"read {k}: anchors differ from collect_seed_hits_heap"
        u_ref, b_ref = ob.mm_chain_dp(P, 3, 40, ref)
        assert np.array_equal(res[k][0], u_ref) and np.array_equal(res[k][1], b_ref), f"read {k}: chains differ"
        n_ties += int((ref[1:, 0] == ref[:-1, 0]).sum())
        fwd = ref[:, 0] >> np.uint64(63) == 0
        assert np.all(np.diff(ref[fwd, 0].astype(np.int64)) >= 0) and np.all(np.diff(ref[~fwd, 0]) >= 0)   # each strand ascending, as mm_chain_dp needs
    assert np.array_equal(ao, ao2) and n_ties > 0


def test_errors_are_reported_not_written():
    """a long read whose capacity disagrees with its hits under skip_seed (device check, nothing written); a hit naming a reference beyond ref_rank and NO_DUAL with ranks but
    without q_lo (host checks, before any kernel runs)"""
    import mm2chain
    from mm2chain import params
    rng = np.random.default_rng(31)
    qlen, m, h = _random_read(rng, 6000, 8, 4, 1 << 24, qlen=90000)
    n = int(m["n"].sum())
    assert n > 16384
    d_m = torch.from_numpy(m.view(np.uint8).copy()).cuda(); d_h = torch.from_numpy(h.view(np.int64)).cuda()
    d_q = torch.tensor([qlen], dtype=torch.int32, device="cuda")
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    for wrong in (n + 5, n - 5):
        plan = mm2chain.SeedPlan(np.array([0, m.size], np.int64), np.array([0, wrong], np.int64))
        anchors = torch.zeros((max(n, wrong) + 64, 2), dtype=torch.int64, device="cuda")
        _, off = plan.run_skip(d_m, d_h, d_q, AVA, i32(0, 1, 2, 3), i32(5, 5, 5, 5), i32(2), i32(1), anchors=anchors)
        with pytest.raises(mm2chain.Mm2cError):
            plan.check()
        assert plan.last_expand_mw() == 1 and int(off[-1]) == 0                 # the read keeps nothing
        assert not bool(anchors.any())                                          # and nothing was written
        plan.close()
    P = params.map_ont()
    mo, ql = np.array([0, m.size], np.int64), np.array([qlen], np.int32)
    short = mm2chain.SeedSkip(AVA, [0, 1, 2], [5, 5, 5], [1], [1])                # rids go up to 3
    with pytest.raises(mm2chain.Mm2cError, match="beyond"):
        mm2chain.seed_hits_batch_skip(mo, m, h, ql, short)
    with pytest.raises(mm2chain.Mm2cError, match="beyond"):
        mm2chain.seed_chain_batch_skip(P, 3, 40, mo, m, h, ql, short)
    pool = mm2chain.HitPool(h)
    try:
        with pytest.raises(mm2chain.Mm2cError, match="beyond"):
            mm2chain.seed_chain_batch_pool_skip(P, 3, 40, mo, m, pool, ql, short)
        ok = mm2chain.SeedSkip(AVA, [0, 1, 2, 3], [5, 5, 5, 5], [1], [1])
        ao, _ = mm2chain.seed_chain_batch_pool_skip(P, 3, 40, mo, m, pool, ql, ok)  # the same pool with enough ranks
        assert 0 < ao[-1] < n
    finally:
        pool.close()
    no_q = mm2chain.SeedSkip(ob.F_NO_DUAL, [0, 1, 2, 3], [5, 5, 5, 5], [1], [1])
    no_q.q_lo = no_q.q_eq = None                                                 # past the Python checks: the library refuses it itself
    with pytest.raises(mm2chain.Mm2cError, match="q_lo"):
        mm2chain.seed_chain_batch_skip(P, 3, 40, mo, m, h, ql, no_q)
    with pytest.raises(mm2chain.Mm2cError, match="q_lo"):
        mm2chain.seed_hits_batch_skip(mo, m, h, ql, no_q)


def test_split_across_two_device_contexts_equals_one():
    """two device contexts on the one card (as tests/test_gpu_multidevice.py): the batch is split into contiguous read ranges by capacity, each range packs its
    own offsets, and anchor_off / u / b are closed up -- equal to one context's results"""
    import mm2chain
    from mm2chain import params
    d, base, q_lo1, q_eq1, P, min_cnt, min_sc = _fixture()
    rng = np.random.default_rng(3)
    extra = [_random_read(rng, 3000, 9, 4, 1 << 22, qlen=60000) for _ in range(3)]
    reads = base * 2 + extra
    q_lo = np.concatenate([np.tile(q_lo1, 2), [0, 2, 4]]).astype(np.int32)
    q_eq = np.concatenate([np.tile(q_eq1, 2), [1, 0, 0]]).astype(np.int32)
    ref_rank = np.concatenate([d["ref_rank"], np.arange(d["ref_rank"].size, d["ref_rank"].size + 4)]).astype(np.int32)
    ref_len = np.concatenate([d["ref_len"], [60000] * 4]).astype(np.int32)
    extra_rid = np.uint64(d["ref_rank"].size)                                   # the random reads' references come after the fixture's
    reads[-3:] = [(q, mr, hr + (extra_rid << np.uint64(32))) for q, mr, hr in extra]
    q_lo[-3:] += d["ref_rank"].size
    mo, m, h, ql = _batch(reads)
    skip = mm2chain.SeedSkip(AVA, ref_rank, ref_len, q_lo, q_eq)
    mm2chain.shutdown()
    mm2chain.init_devices([0, 0])
    try:
        assert mm2chain.device_count() == 2
        with mm2chain.tuned(multi_min_anchors=1000):
            ao2, res2 = mm2chain.seed_chain_batch_skip(P, min_cnt, min_sc, mo, m, h, ql, skip)
    finally:
        mm2chain.shutdown()
        mm2chain.init(0)
    ao1, res1 = mm2chain.seed_chain_batch_skip(P, min_cnt, min_sc, mo, m, h, ql, skip)
    assert np.array_equal(ao1, ao2)
    assert ao1[-1] < _capacity(mo, m)[-1]
    for k in range(len(reads)):
        assert np.array_equal(res1[k][0], res2[k][0]) and np.array_equal(res1[k][1], res2[k][1]), k
    for k in range(len(base)):
        assert np.array_equal(np.diff(ao1)[k], d[f"r{k}_anchors"].shape[0])
        u_ref, b_ref = ob.mm_chain_dp(P, min_cnt, min_sc, d[f"r{k}_anchors"])
        assert np.array_equal(res1[k][0], u_ref) and np.array_equal(res1[k][1], b_ref), k
