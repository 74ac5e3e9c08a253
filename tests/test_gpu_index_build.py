"""mm2c_minidx_build (MinimizerIndex.build): the minimizer index made on the device from the sequences.  Every comparison is exact.
  1. against the reference's own index (tests/golden/ref_sketch.npz), over the fixture's reference set rebuilt as tests/test_cpu_index_model.py rebuilds it;
  2. against the NumPy model (tests/index_model.py) over a sweep of (k, w, hpc) and awkward sequence lists;
  3. chunking: index_chunk_bases below the longest sequence, equal to a short one, and the default give one and the same index;
  4. scale: 2.4 * 10^7 bases, against index_model.build_from_minimizers fed the device's own (pinned) sketch with the rid OR-ed in;
  5. use: lookups, reads in / chains out (all-vs-all with skip flags too) and the matches-in pool entry agree with an index made from the model's table;
  6. replicas: two slots on the one card;
  7. lifetime: build / destroy repeatedly, a created index over a caller's pool afterwards, and the statistics add up."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import index_model as im
import oracle_binding as ob
from helpers import assert_table as _assert_table
from helpers import knobs  # noqa: F401 (knobs: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "ref_sketch.npz")
DATA = os.path.join(HERE, "golden", "ref_testdata")
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.array([3, 2, 1, 0], np.uint8)
MIN_CNT, MIN_SC = 3, 40
AVA = ob.F_NO_DIAG | ob.F_NO_DUAL
INT32_MAX = 2**31 - 1
RESULT_KEYS = ("anchor_off", "u_off", "u", "b_off", "b", "rep_len", "mini_off", "mini_pos")


@pytest.fixture(autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


# ---- data ----------------------------------------------------------------------------------------------------------------------------------------------

def _generator():
    spec = importlib.util.spec_from_file_location("make_ref_sketch_fixtures", os.path.join(HERE, "golden", "make_ref_sketch_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """the reference sequences of the fixture's index, in its order: MT-human, t-inv, the synthetic chromosomes, repeats, repeats2"""
    g = _generator()
    tmp = tmp_path_factory.mktemp("syn")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), str(tmp / "syn"), "--genome-mb", "0.05",
                           "--reads", "6", "--read-len", "4000", "--seed", "5"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(2026)
    g.adversarial(rng)                                         # the draws before the repeat units
    unit = rng.choice(np.frombuffer(b"ACGT", np.uint8), 150).tobytes()
    unit2 = rng.choice(np.frombuffer(b"ACGT", np.uint8), 24).tobytes()
    seqs = []
    for p in (os.path.join(DATA, "MT-human.fa"), os.path.join(DATA, "t-inv.fa"), str(tmp / "syn.ref.fa")):
        seqs += g.read_fasta(p)
    return seqs + [unit * 80, unit2 * 300]


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def model_map_ont(refs):
    """the model's table of the fixture's reference set at map-ont k / w"""
    return im.build_index(refs, 15, 10, 0)


def _txt(codes):
    return ACGT[codes].tobytes()


def _ont(rng, s, err):
    """substitutions, deletions and insertions at a total rate err (2-bit codes in, 2-bit codes out)"""
    u = rng.random(s.size)
    s = s.copy()
    sub = u < err * 0.4
    s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) % 4
    keep = ~((u >= err * 0.4) & (u < err * 0.7))
    ins = np.nonzero(((u >= err * 0.7) & (u < err))[keep])[0]
    s = s[keep]
    return np.insert(s, ins + 1, rng.integers(0, 4, ins.size, dtype=np.uint8))


def _sample(rng, g, L, err):
    c = int(rng.integers(0, len(g)))
    L = min(L, g[c].size)
    p = int(rng.integers(0, g[c].size - L + 1))
    s = g[c][p:p + L]
    if rng.random() < 0.5:
        s = COMP[s[::-1]]
    return _ont(rng, s, err)


def _codes(seq):
    """A C G T bytes (either case) as 2-bit codes; anything else is dropped"""
    a = np.frombuffer(bytes(seq).upper(), np.uint8)
    a = a[np.isin(a, ACGT)]
    return np.searchsorted(ACGT, a).astype(np.uint8)


def _reads_from(refs, n, seed):
    """ONT-like reads from both strands of the reference set, a read that is absent from it, and degenerate ones"""
    rng = np.random.default_rng(seed)
    g = [c for c in (_codes(s) for s in refs) if c.size >= 3000]
    reads = [_txt(_sample(rng, g, int(rng.integers(1500, 9001)), 0.07)) for _ in range(n)]
    reads.insert(3, _txt(rng.integers(0, 4, 3000, dtype=np.uint8)))
    reads[7:7] = [b"", b"ACG", b"N" * 400]
    return reads


def _ava_reads(seed=77):
    """all-vs-all, as tests/test_gpu_read_chain_e2e.py makes them at a smaller size: overlapping reads from one window, a unique read, degenerate reads and a
    chimera of the window"""
    rng = np.random.default_rng(seed)
    win = rng.integers(0, 4, 40_000, dtype=np.uint8)
    reads = [_txt(_sample(rng, [win], int(rng.integers(3000, 9001)), 0.06)) for _ in range(20)]
    reads.insert(11, _txt(rng.integers(0, 4, 3000, dtype=np.uint8)))                  # maps only to itself: every hit on its own diagonal
    reads[15:15] = [b"", b"ACG", b"N" * 500, _txt(rng.integers(0, 4, 15, dtype=np.uint8))]
    reads.append(_txt(_sample(rng, [win], 3000, 0.05)) + _txt(_sample(rng, [win], 3000, 0.05)))
    return reads


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------------

def _model_occ(n, frac):
    """index_model.cal_max_occ, and INT32_MAX for an index without keys (the reference is undefined there; include/mm2chain.h says what the library returns)"""
    return INT32_MAX if n.size == 0 else im.cal_max_occ(n, frac)


def _same_results(got, ref, what):
    for k in RESULT_KEYS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k} differs"


# ---- 1. the reference's own index ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["map_ont", "ava_ont"])
def test_built_index_equals_the_reference_index(refs, fx, name):
    import mm2chain
    k, w, hpc = (int(v) for v in fx[name + "_kwh"])
    idx = mm2chain.MinimizerIndex.build(refs, k, w, hpc)
    keys, cr_off, n, pool = idx.export()
    rk, rn, rcr, rpool = fx[name + "_keys"], fx[name + "_n"], fx[name + "_cr_off"], fx[name + "_pool"]
    assert np.array_equal(keys, rk), f"{name}: {keys.size} keys, the reference {rk.size}"
    assert np.array_equal(n, rn)
    assert idx.n_keys == keys.size and idx.n_hits == pool.size == int(n.sum())
    for i in range(keys.size):                                 # the offsets differ (singletons live in the reference's hash table); the hits do not
        a, b, c = int(cr_off[i]), int(rcr[i]), int(n[i])
        assert np.array_equal(pool[a:a + c], rpool[b:b + c]), f"{name}: key {int(keys[i]):#x} ({c} hits) differs"
    assert (n > 1).sum() > 500 and n.max() >= fx[name + "_mid_occ"][0], "the input has multi-hit keys and keys at or above mid_occ"
    assert idx.mid_occ == int(fx[name + "_mid_occ"][0])
    assert idx.cal_max_occ(2e-4) == idx.mid_occ
    print(f"{name}: {keys.size} keys, {pool.size} hits, mid_occ {idx.mid_occ}")
    idx.close()


# ---- 2. the NumPy model over a sweep ----------------------------------------------------------------------------------------------------------------------

def _awkward(seed):
    """seeded random sequences with N runs, lower case, a zero-length sequence, one shorter than every k of the sweep but 4, and a tandem repeat of a 24-base
    unit 2500 times over: its few keys hold thousands of hits each (the build sorts and groups in global memory: there is no LDS tile to outgrow)"""
    rng = np.random.default_rng(seed)
    a = bytearray(_txt(rng.integers(0, 4, 30_000, dtype=np.uint8)))
    a[4000:4300] = b"N" * 300; a[9000:9001] = b"N"; a[20_000:20_040] = b"n" * 40
    a[12_000:15_000] = bytes(a[12_000:15_000]).lower()
    b = _txt(rng.integers(0, 4, 12_000, dtype=np.uint8))
    unit = _txt(rng.integers(0, 4, 24, dtype=np.uint8))
    homopolymers = b"".join(bytes([c]) * int(rng.integers(1, 9)) for c in _txt(rng.integers(0, 4, 1500, dtype=np.uint8)))
    return [bytes(a), b"", b, b"ACGTA", unit * 2500, b[3000:9000], homopolymers, b"N" * 50, _txt(rng.integers(0, 4, 40, dtype=np.uint8))]


@pytest.mark.parametrize("k,w,hpc", [(15, 10, 0), (19, 10, 0), (19, 19, 1), (28, 1, 0), (4, 3, 0), (11, 255, 1)])
def test_sweep_against_the_numpy_model(k, w, hpc):
    import mm2chain
    seqs = _awkward(1000 + k * 7 + w)
    lists = {"all": seqs, "single": [seqs[0]], "single tandem": [seqs[4]], "empty": [], "only empty sequences": [b"", b""], "nothing to index": [b"NNNN", b"AC"]}
    for what, lst in lists.items():
        ref = im.build_index(lst, k, w, hpc)
        idx = mm2chain.MinimizerIndex.build(lst, k, w, hpc, mid_occ_frac=2e-4)
        got = idx.export()
        _assert_table(got, ref, f"k {k} w {w} hpc {hpc}, {what}")
        assert idx.n_keys == ref[0].size and idx.n_hits == ref[3].size
        assert idx.mid_occ == _model_occ(ref[2], 2e-4)
        for frac in (2e-4, 0.0, 0.5):
            assert idx.cal_max_occ(frac) == _model_occ(ref[2], frac), f"k {k} w {w} hpc {hpc}, {what}: cal_max_occ({frac})"
        if what == "all":
            assert ref[2].max() >= 2000, "the tandem repeat's keys hold thousands of hits"
            if (k, w) == (4, 3):
                assert ref[0].size <= 256 and ref[2].max() > 1000, "few keys, very long hit lists"
        if what in ("empty", "only empty sequences"):
            assert idx.n_keys == 0 and idx.n_hits == 0 and idx.mid_occ == INT32_MAX
            cr, n = idx.lookup(np.arange(5, dtype=np.uint64))
            assert not n.any() and not cr.any()
        idx.close()


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------------------------------

def test_chunking_does_not_change_the_index(refs, knobs):
    import mm2chain
    lens = [len(s) for s in refs]
    short = min(l for l in lens if l > 0)
    out = {}
    for name, cb in (("below the longest sequence", max(lens) // 3), ("one short sequence", short), ("default", None)):
        lim = mm2chain.tune_get("index_chunk_bases")[1] if cb is None else cb
        knobs("index_chunk_bases", lim)
        mm2chain.index_stats(reset=True)
        idx = mm2chain.MinimizerIndex.build(refs, 15, 10)
        out[name] = idx.export() + (idx.mid_occ,)
        st = mm2chain.index_stats()
        # the host's rule: a chunk takes whole sequences while its bases stay within index_chunk_bases, at least one sequence
        off = np.concatenate([[0], np.cumsum(lens)])
        want, r0 = 0, 0
        while r0 < len(lens):
            r1 = r0 + 1
            while r1 < len(lens) and off[r1 + 1] - off[r0] <= lim:
                r1 += 1
            want, r0 = want + 1, r1
        assert st["chunks"] == want, f"{name}: {st['chunks']} chunks, the rule gives {want}"
        assert (st["chunks"] > 1) == (cb is not None), f"{name}: {st['chunks']} chunks"
        print(f"index_chunk_bases {lim}: {st['chunks']} chunks")
        idx.close()
    first = out["default"]
    for name, got in out.items():
        for a, b in zip(got[:4], first[:4]):
            assert np.array_equal(a, b), f"{name}: the export differs from the one-chunk build"
        assert got[4] == first[4]


# ---- 4. scale -------------------------------------------------------------------------------------------------------------------------------------------

def test_scale_2e7_bases(knobs):
    import mm2chain
    rng = np.random.default_rng(4242)
    lens = [9_000_000, 6_500_000, 0, 5_000_000, 3_000_000, 499_999, 1]
    seqs = [ACGT[rng.integers(0, 4, L, dtype=np.uint8)] for L in lens]
    rep = seqs[0][1_000_000:1_200_000]                                                 # planted copies: keys with many hits across sequences
    for s, p in ((seqs[1], 50_000), (seqs[3], 4_000_000), (seqs[4], 2_700_000), (seqs[0], 8_000_000)):
        s[p:p + rep.size] = rep
    assert sum(lens) >= 20_000_000
    k, w = 15, 10
    knobs("index_chunk_bases", 8_000_000)                                     # several chunks, one of them a sequence longer than the chunk
    mm2chain.index_stats(reset=True)
    idx = mm2chain.MinimizerIndex.build(seqs, k, w)
    st = mm2chain.index_stats()
    assert st["chunks"] >= 3 and st["bases"] == sum(lens)
    off, mini = mm2chain.sketch_batch(seqs, k, w)                                      # pinned by tests/test_gpu_sketch.py; rid 0
    rid = np.repeat(np.arange(len(seqs), dtype=np.uint64), np.diff(off))
    mini[:, 1] |= rid << np.uint64(32)
    ref = im.build_from_minimizers(mini)
    assert idx.n_hits == mini.shape[0] == st["minimizers"] and idx.n_keys == ref[0].size == st["keys"]
    got = idx.export()
    for a, b, name in zip(got, ref, ("keys", "cr_off", "n", "pool")):
        assert np.array_equal(a, b), f"{name} differs"
    assert ref[2].max() >= 5
    for frac in (2e-4, 0.5):
        assert idx.cal_max_occ(frac) == im.cal_max_occ(ref[2], frac)
    print(f"scale: {sum(lens)} bases, {idx.n_hits} minimizers, {idx.n_keys} keys, {st['chunks']} chunks; "
          + ", ".join(f"{k_} {st[k_] / 1e6:.1f} ms" for k_ in ("h2d_ns", "sketch_ns", "sort_ns", "group_ns", "occ_ns", "replicate_ns")))
    idx.close()


# ---- 5. use ---------------------------------------------------------------------------------------------------------------------------------------------

def _lookup_agrees(built, made, table, rng):
    keys, cr_off, n, pool = table
    absent = rng.integers(0, 1 << 2 * built.k, 4000, dtype=np.uint64)
    absent = absent[~np.isin(absent, keys)]
    assert absent.size > 3000
    q = np.concatenate([keys, absent, np.array([1 << 2 * built.k, 2**64 - 1], np.uint64)])   # ... and keys that no index of this k can hold
    cr_b, n_b = built.lookup(q)
    cr_m, n_m = made.lookup(q)
    assert np.array_equal(n_b, n_m) and np.array_equal(n_b[:keys.size], n) and not n_b[keys.size:].any()
    pool_b = built.export()[3]
    for i in np.nonzero(n_b)[0]:
        assert np.array_equal(pool_b[cr_b[i]:cr_b[i] + n_b[i]], pool[cr_m[i]:cr_m[i] + n_m[i]]), f"key {int(q[i]):#x}: the hit lists differ"


def test_a_built_index_is_used_like_a_made_one(refs, model_map_ont):
    import mm2chain
    from mm2chain import params
    P = params.map_ont()
    keys, cr_off, n, pool = model_map_ont
    built = mm2chain.MinimizerIndex.build(refs, 15, 10)
    made = mm2chain.MinimizerIndex(15, 10, 0, keys, cr_off, n, hits=pool)
    assert built.mid_occ == im.cal_max_occ(n) == made.cal_max_occ(2e-4), "cal_max_occ also serves an index made by mm2c_minidx_create"
    _lookup_agrees(built, made, model_map_ont, np.random.default_rng(9))
    ek, ecr, en, epool = made.export()                                                 # a made index: its table sorted by key, the caller's pool untouched
    assert np.array_equal(ek, keys) and np.array_equal(ecr, cr_off) and np.array_equal(en, n) and epool.size == 0
    reads = _reads_from(refs, 40, 31)
    for mid in (built.mid_occ, 3, INT32_MAX):
        got = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, built, mid)
        ref = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, made, mid)
        _same_results(got, ref, f"read_chain_batch, mid_occ {mid}")
        if mid == built.mid_occ:
            assert sum(u.size > 0 for u, _ in got["chains"]) >= 15 and got["rep_len"].any(), "reads that map, and reads that meet repetitive keys"
        a = mm2chain.sketch_match_batch(reads, built, mid)
        b = mm2chain.sketch_match_batch(reads, made, mid)
        for k_ in ("match_off", "anchor_off", "rep_len", "mini_off", "mini_pos"):
            assert np.array_equal(a[k_], b[k_]), f"sketch_match_batch, mid_occ {mid}: {k_} differs"
        for f in ("n", "q_pos", "q_span", "seg_tandem"):                                # (cr_off points into each index's own pool)
            assert np.array_equal(a["matches"][f], b["matches"][f]), f"sketch_match_batch, mid_occ {mid}: matches.{f} differs"
        # matches in, chains out through the built index's own pool
        qlen = [len(s) for s in reads]
        chains = mm2chain.seed_chain_batch_pool(P, MIN_CNT, MIN_SC, a["match_off"], a["matches"], built.pool, qlen)
        for r, ((u, bb), (ur, br)) in enumerate(zip(chains, ref["chains"])):
            assert np.array_equal(u, ur) and np.array_equal(bb, br), f"seed_chain_batch_pool over .pool, mid_occ {mid}: read {r} differs"
    built.close(); made.close()


def test_all_vs_all_with_the_reads_as_their_own_index():
    import mm2chain
    from mm2chain import params
    P = params.ava_ont()
    reads = _ava_reads()
    table = im.build_index(reads, 15, 5, 0)
    keys, cr_off, n, pool = table
    built = mm2chain.MinimizerIndex.build(reads, 15, 5)
    made = mm2chain.MinimizerIndex(15, 5, 0, keys, cr_off, n, hits=pool)
    _assert_table(built.export(), table, "ava-ont reads")
    assert built.mid_occ == im.cal_max_occ(n)
    _lookup_agrees(built, made, table, np.random.default_rng(10))
    nr = len(reads)
    rank, ref_len = np.arange(nr, dtype=np.int32), np.array([len(s) for s in reads], np.int32)
    q_lo, q_eq = np.arange(nr, dtype=np.int32), np.ones(nr, np.int32)
    skip = mm2chain.SeedSkip(AVA, rank, ref_len, q_lo, q_eq)
    got = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, built, built.mid_occ, skip=skip)
    ref = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, made, built.mid_occ, skip=skip)
    _same_results(got, ref, "all-vs-all read_chain_batch")
    free = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, built, built.mid_occ)
    assert free["anchor_off"][-1] > got["anchor_off"][-1] > 0, "anchors were skipped, and anchors were kept"
    assert sum(u.size > 0 for u, _ in got["chains"]) >= 10
    m = mm2chain.sketch_match_batch(reads, built, built.mid_occ)
    ao, chains = mm2chain.seed_chain_batch_pool_skip(P, MIN_CNT, MIN_SC, m["match_off"], m["matches"], built.pool, [len(s) for s in reads], skip)
    assert np.array_equal(ao, got["anchor_off"])
    for r, ((u, b), (ur, br)) in enumerate(zip(chains, got["chains"])):
        assert np.array_equal(u, ur) and np.array_equal(b, br), f"seed_chain_batch_pool_skip over .pool: read {r} differs"
    built.close(); made.close()


# ---- 6. replicas ----------------------------------------------------------------------------------------------------------------------------------------

def test_two_slots_on_one_card(refs):
    import mm2chain
    from mm2chain import params
    P = params.map_ont()
    reads = _reads_from(refs, 30, 5)
    one = mm2chain.MinimizerIndex.build(refs, 15, 10)
    ref = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, one, one.mid_occ)
    table, occ = one.export(), one.mid_occ
    one.close()
    mm2chain.shutdown()
    mm2chain.init_devices([0, 0])
    try:
        assert mm2chain.device_count() == 2
        two = mm2chain.MinimizerIndex.build(refs, 15, 10)
        assert two.mid_occ == occ
        for a, b in zip(two.export(), table):
            assert np.array_equal(a, b)
        got = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, two, two.mid_occ)
        _same_results(got, ref, "two slots")
        assert sum(u.size > 0 for u, _ in got["chains"]) >= 10
        two.close()
    finally:
        mm2chain.shutdown()
        mm2chain.init()


# ---- 7. lifetime ----------------------------------------------------------------------------------------------------------------------------------------

def test_build_destroy_build_and_the_statistics(refs, model_map_ont):
    import mm2chain
    from mm2chain import params
    P = params.map_ont()
    keys, cr_off, n, pool = model_map_ont
    mm2chain.index_stats(reset=True)
    assert not any(mm2chain.index_stats().values())
    first = None
    for rnd in range(4):
        idx = mm2chain.MinimizerIndex.build(refs, 15, 10)
        view = idx.pool
        assert view.size == idx.n_hits == pool.size and idx.n_keys == keys.size
        got = idx.export()
        first = first or got
        for a, b in zip(got, first):
            assert np.array_equal(a, b), f"round {rnd}"
        idx.close()
        view.close()                                                                   # a view: closing it after its index frees nothing
        idx.close()                                                                    # ... and closing twice is harmless
    st = mm2chain.index_stats()
    assert st["calls"] == 4 and st["chunks"] == 4
    assert st["bases"] == 4 * sum(len(s) for s in refs) and st["minimizers"] == 4 * pool.size and st["keys"] == 4 * keys.size
    assert st["sketch_ns"] > 0 and st["sort_ns"] > 0 and st["group_ns"] > 0
    # a created index over a caller's pool still works, and destroying it leaves that pool alone
    hp = mm2chain.HitPool(pool)
    made = mm2chain.MinimizerIndex(15, 10, 0, keys, cr_off, n, pool=hp)
    built = mm2chain.MinimizerIndex.build(refs, 15, 10)
    reads = _reads_from(refs, 12, 77)
    ref = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, built, built.mid_occ)
    built.close()
    got = mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, made, built.mid_occ)
    _same_results(got, ref, "a created index after the built ones")
    made.close()
    made2 = mm2chain.MinimizerIndex(15, 10, 0, keys, cr_off, n, pool=hp)              # the caller's pool outlives its index
    _same_results(mm2chain.read_chain_batch(P, MIN_CNT, MIN_SC, reads, made2, built.mid_occ), ref, "the caller's pool after its first index")
    made2.close(); hp.close()
    assert mm2chain.index_stats(reset=True)["calls"] == 5 and mm2chain.index_stats()["calls"] == 0
