"""GPU tests of the device sketch and lookups (csrc/sketch.hip; mm2c_sketch_batch, mm2c_minidx_*, mm2c_sketch_match_batch): bit for bit against the reference's
own mm_sketch / collect_matches output (tests/golden/ref_sketch.npz: counts and SHA-256 per read) and against the Python restatement (tests/sketch_model.py) on seeded random and
adversarial batches, one read of 10^6 bases among them."""
import os

import numpy as np
import pytest
import torch

import sketch_model as sm

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sketch.npz")
CONFIGS = ["map_ont", "ava_ont", "asm20", "sr", "map_pb", "ava_pb", "even_k16", "w1", "w255"]


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


def _reads(fx):
    off, seq = fx["seq_off"], fx["seq"]
    return [seq[off[r]:off[r + 1]].tobytes() for r in range(off.size - 1)]


def _index(fx, name):
    import mm2chain
    k, w, hpc = (int(v) for v in fx[name + "_kwh"])
    pool = mm2chain.HitPool(fx[name + "_pool"])
    return mm2chain.MinimizerIndex(k, w, hpc, fx[name + "_keys"], fx[name + "_cr_off"], fx[name + "_n"], pool=pool)


@pytest.mark.parametrize("name", CONFIGS)
def test_sketch_equals_reference(fx, name):
    import mm2chain
    k, w, hpc = (int(v) for v in fx[name + "_kwh"])
    off, mini = mm2chain.sketch_batch((fx["seq_off"], fx["seq"]), k, w, hpc)
    assert np.array_equal(off, fx[name + "_off"])
    for r in range(off.size - 1):
        assert np.array_equal(sm.sha(mini[off[r]:off[r + 1]]), fx[name + "_sha"][r]), f"{name}: read {r} differs from the reference"


def _rand_reads(rng, lens, n_frac=0.0, hp=False):
    out = []
    for L in lens:
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), L)
        if n_frac:
            s[rng.random(L) < n_frac] = ord("N")
        if hp and L > 50:                                    # long homopolymers and tandem repeats dropped in
            for _ in range(max(1, L // 3000)):
                a = int(rng.integers(0, L - 20)); s[a:a + int(rng.integers(5, 400))] = s[a]
                a = int(rng.integers(0, L - 20)); unit = s[a:a + int(rng.integers(1, 6))].copy(); run = np.tile(unit, 40)[:L - a]; s[a:a + run.size] = run
        out.append(s.tobytes())
    return out


def _check_model(reads, k, w, hpc):
    import mm2chain
    off, mini = mm2chain.sketch_batch(reads, k, w, hpc)
    for r, s in enumerate(reads):
        assert np.array_equal(mini[off[r]:off[r + 1]], sm.sketch_array(s, w, k, hpc)), f"read {r} ({len(s)} bases) differs, k={k} w={w} hpc={hpc}"


@pytest.mark.parametrize("k,w,hpc", [(15, 10, 0), (16, 7, 0), (19, 5, 1), (28, 255, 0), (1, 1, 0), (2, 3, 1), (12, 200, 1)])
def test_sketch_equals_model_mixed(k, w, hpc):
    rng = np.random.default_rng(1000 + 7 * k + w + hpc)
    lens = [0, 1, k - 1, k, w + k - 2, w + k - 1, w + k, 63, 64, 65, 255, 256, 257] + list(rng.integers(1, 5000, 30))
    reads = _rand_reads(rng, lens, n_frac=0.01, hp=True)
    reads += [b"AT" * 700, b"N" * 100 + b"ACGT" * 300 + b"N" * 100, bytes(range(256)) * 4, b"acgtu" * 300, b"A" * 1000 + b"C" * 600]
    _check_model(reads, k, w, hpc)


def test_sketch_mostly_short_reads():
    rng = np.random.default_rng(3)
    k, w = 15, 10
    lens = list(rng.integers(0, w + k - 1, 3000)) + [5000, 20000]
    _check_model(_rand_reads(rng, lens, n_frac=0.02), k, w, 0)


def test_sketch_one_read_of_a_million_bases():
    rng = np.random.default_rng(4)
    reads = _rand_reads(rng, [1_000_000, 3000, 700], n_frac=0.0005, hp=True)
    _check_model(reads, 15, 10, 0)
    _check_model(reads[:1], 19, 10, 1)


@pytest.mark.parametrize("name", ["map_ont", "ava_ont"])
def test_matches_equal_reference(fx, name):
    import mm2chain
    idx = _index(fx, name)
    r = mm2chain.sketch_match_batch((fx["seq_off"], fx["seq"]), idx, int(fx[name + "_mid_occ"][0]))
    mo = fx[name + "_match_off"]
    assert np.array_equal(r["match_off"], mo)
    for q in range(mo.size - 1):
        assert np.array_equal(sm.sha(r["matches"][mo[q]:mo[q + 1]]), fx[name + "_match_sha"][q]), f"{name}: matches of read {q} differ"
        assert np.array_equal(sm.sha(r["mini_pos"][mo[q]:mo[q + 1]]), fx[name + "_mini_pos_sha"][q]), f"{name}: mini_pos of read {q} differ"
    assert np.array_equal(r["rep_len"], fx[name + "_rep_len"]) and (r["rep_len"] > 0).any()
    assert np.array_equal(r["mini_off"], mo)
    n = r["matches"]["n"].astype(np.int64)
    assert np.array_equal(r["anchor_off"], np.concatenate([[0], np.cumsum([n[a:b].sum() for a, b in zip(r["match_off"][:-1], r["match_off"][1:])])]))
    idx.close()


def test_matches_equal_model_other_mid_occ(fx):
    """mid_occ of 1, 3 and larger than any count: repetitive minimizers everywhere, some, none"""
    import mm2chain
    name = "map_ont"
    idx = _index(fx, name)
    look = sm.table_lookup(fx[name + "_keys"], fx[name + "_cr_off"], fx[name + "_n"])
    minis = [sm.sketch_array(s, 10, 15) for s in _reads(fx)]
    for mid_occ in (1, 3, 1 << 30):
        r = mm2chain.sketch_match_batch((fx["seq_off"], fx["seq"]), idx, mid_occ)
        for q in range(len(minis)):
            m, rep_len, mini_pos = sm.collect_matches(minis[q], look, mid_occ)
            got = r["matches"][r["match_off"][q]:r["match_off"][q + 1]]
            assert [tuple(int(v) for v in t) for t in got.tolist()] == m
            assert int(r["rep_len"][q]) == rep_len
            assert r["mini_pos"][r["mini_off"][q]:r["mini_off"][q + 1]].tolist() == mini_pos
    idx.close()


def test_lookup_absent_keys(fx):
    name = "map_ont"
    idx = _index(fx, name)
    keys = fx[name + "_keys"]
    present = keys[::97]
    absent = np.setdiff1d(np.random.default_rng(5).integers(0, 1 << 30, 5000).astype(np.uint64), keys)[:1000]
    q = np.concatenate([present, absent, np.array([(1 << 30), (1 << 63)], np.uint64)])
    cr, n = idx.lookup(q)
    assert np.array_equal(cr[:present.size], fx[name + "_cr_off"][::97]) and np.array_equal(n[:present.size], fx[name + "_n"][::97])
    assert (n[present.size:] == 0).all() and (cr[present.size:] == 0).all()
    idx.close()


def test_errors(fx):
    import mm2chain
    from mm2chain import Mm2cError
    pool = mm2chain.HitPool(fx["map_ont_pool"])
    keys, cr, n = fx["map_ont_keys"], fx["map_ont_cr_off"], fx["map_ont_n"]
    with pytest.raises(Mm2cError):                                   # duplicate key
        mm2chain.MinimizerIndex(15, 10, 0, np.concatenate([keys, keys[:1]]), np.concatenate([cr, cr[:1]]), np.concatenate([n, n[:1]]), pool=pool)
    with pytest.raises(Mm2cError):                                   # key >= 2^(2k)
        mm2chain.MinimizerIndex(15, 10, 0, np.array([1 << 30], np.uint64), [0], [1], pool=pool)
    with pytest.raises(Mm2cError):                                   # k > 28
        mm2chain.MinimizerIndex(29, 10, 0, keys, cr, n, pool=pool)
    for w in (0, 256):
        with pytest.raises(Mm2cError):
            mm2chain.MinimizerIndex(15, w, 0, keys, cr, n, pool=pool)
        with pytest.raises(Mm2cError):
            mm2chain.sketch_batch([b"ACGT" * 10], 15, w)
    with pytest.raises(Mm2cError):
        mm2chain.sketch_batch([b"ACGT" * 10], 29, 10)
    with pytest.raises(Mm2cError):                                   # offset + n beyond the pool
        mm2chain.MinimizerIndex(15, 10, 0, np.array([5], np.uint64), [pool.size - 1], [2], pool=pool)
    with pytest.raises(Mm2cError):
        mm2chain.MinimizerIndex(15, 10, 0, np.array([5], np.uint64), [-1], [1], pool=pool)
    lib = mm2chain.load()
    off = np.array([0, 4], np.int64); seq = np.frombuffer(b"ACGT", np.uint8).copy()
    res = lib.mm2c_read_result_create()
    assert lib.mm2c_sketch_match_batch(None, 10, 1, off.ctypes.data, seq.ctypes.data, res) == -2    # a null index
    P = mm2chain.params.map_ont()
    import ctypes as C
    assert lib.mm2c_read_chain_batch(C.byref(P), 3, 40, None, 10, 1, off.ctypes.data, seq.ctypes.data, None, res) == -2
    lib.mm2c_read_result_free(res)
    pool.close()


@pytest.mark.parametrize("k", [15, 28])
def test_lookup_bounds_of_a_key_table_with_both_end_keys(k):
    """keys 0 and 2^(2k) - 1 present: every key returns exactly its (cr_off, n); its neighbours, 0, 2^(2k) - 1 and 2^64 - 1, when absent, return (0, 0)"""
    import mm2chain
    rng = np.random.default_rng(k)
    top = (1 << 2 * k) - 1
    keys = np.unique(np.concatenate([np.array([0, 1, top - 1, top], np.uint64), rng.integers(2, top - 1, 3000, dtype=np.uint64) & ~np.uint64(1)]))
    n = rng.integers(1, 9, keys.size).astype(np.uint32)
    cr = np.concatenate([[0], np.cumsum(n.astype(np.int64))[:-1]])
    pool = mm2chain.HitPool(np.arange(int(n.sum()), dtype=np.uint64))
    perm = rng.permutation(keys.size)                               # the table is handed over unsorted
    idx = mm2chain.MinimizerIndex(k, 10, 0, keys[perm], cr[perm], n[perm], pool=pool)
    table = {int(a): (int(b), int(c)) for a, b, c in zip(keys, cr, n)}
    q = np.unique(np.concatenate([keys, keys + np.uint64(1), keys[keys > 0] - np.uint64(1), np.array([0, top, top + 1, (1 << 64) - 1], np.uint64)]))
    assert q.dtype == np.uint64 and q.max() == np.uint64((1 << 64) - 1) and top + 1 in q
    got_cr, got_n = idx.lookup(q)
    exp = np.array([table.get(int(x), (0, 0)) for x in q], np.int64).reshape(-1, 2)
    assert (exp[:, 1] == 0).sum() > 1000 and 0 in table and top in table
    assert np.array_equal(got_cr, exp[:, 0]) and np.array_equal(got_n.astype(np.int64), exp[:, 1])
    idx.close()
    for one in (0, top, 12345):                                     # a one-key index
        idx = mm2chain.MinimizerIndex(k, 10, 0, [one], [3], [2], pool=pool)
        q1 = np.array([0, 1, one - 1 if one else 2, one, one + 1, top, (1 << 64) - 1], np.uint64)
        c1, n1 = idx.lookup(q1)
        assert np.array_equal(n1, np.where(q1 == one, 2, 0)) and np.array_equal(c1, np.where(q1 == one, 3, 0)), one
        idx.close()
    pool.close()


def test_a_zero_key_index_matches_nothing():
    """mm2c_minidx_create with n_keys = 0: every lookup returns n = 0; reads in give their minimizers and no matches, no anchors, no chains, rep_len 0"""
    import mm2chain
    from mm2chain import params
    pool = mm2chain.HitPool(np.zeros(1, np.uint64))
    idx = mm2chain.MinimizerIndex(15, 10, 0, np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint32), pool=pool)
    cr, n = idx.lookup(np.array([0, 1, 12345, (1 << 30) - 1, (1 << 64) - 1], np.uint64))
    assert not n.any() and not cr.any()
    reads = _rand_reads(np.random.default_rng(5), [0, 14, 15, 3000, 20000])
    so, mini = mm2chain.sketch_batch(reads, 15, 10)
    assert mini.shape[0] > 1000
    s = mm2chain.sketch_match_batch(reads, idx, 300)
    ref = [sm.collect_matches(mini[so[r]:so[r + 1]], lambda key: (0, 0), 300) for r in range(len(reads))]
    assert np.array_equal(s["match_off"], so) and not s["matches"]["n"].any() and not s["rep_len"].any()
    assert np.array_equal(s["matches"], sm.match_array([x for mt, _, _ in ref for x in mt]))
    got = mm2chain.read_chain_batch(params.map_ont(), 3, 40, reads, idx, 300)
    assert np.array_equal(got["mini_off"], so) and not got["anchor_off"].any() and got["u"].size == 0 and got["b"].size == 0 and not got["rep_len"].any()
    assert np.array_equal(got["mini_pos"], np.array([p for _, _, mp in ref for p in mp], np.uint64))
    idx.close(); pool.close()
