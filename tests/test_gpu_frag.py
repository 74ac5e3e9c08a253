"""GPU tests of the fragment entries (mm2c_sketch_frag_batch, mm2c_sketch_match_frag_batch, mm2c_frag_chain_batch): paired and multi-segment reads and the
max_occ re-chain of map.c:318-340, bit for bit against what the reference's own mm_map_frag did (tests/golden/ref_frag.npz) and, for shapes made by hand,
against the CPU model (tests/frag_model.py, itself pinned to that fixture by tests/test_cpu_frag_model.py)."""
import os

import numpy as np
import pytest
import torch

import frag_model as fm
import sketch_model as sm
from helpers import knobs  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_frag.npz")
FOR_ONLY = 0x100000


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


@pytest.fixture(autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def _index(fx, p=""):
    import mm2chain
    pool = mm2chain.HitPool(fx[p + "pool"])
    return mm2chain.MinimizerIndex(int(fx["k"]), int(fx["w"]), bool(p), fx[p + "keys"], fx[p + "cr_off"], fx[p + "n"], pool=pool)


def _sub(fx, ids):
    """the fragments `ids` as (frag_off, seq_off, seq)"""
    fo, so, seq = fx["frag_off"], fx["seq_off"], fx["seq"]
    segs = [seq[so[s]:so[s + 1]] for g in ids for s in range(fo[g], fo[g + 1])]
    f = np.zeros(len(ids) + 1, np.int64); f[1:] = np.cumsum([fo[g + 1] - fo[g] for g in ids])
    o = np.zeros(len(segs) + 1, np.int64); o[1:] = np.cumsum([s.size for s in segs])
    return f, o, np.concatenate(segs) if segs else np.zeros(0, np.uint8)


def _cat(fx, off, arr, ids):
    parts = [fx[arr][fx[off][g]:fx[off][g + 1]] for g in ids]
    return np.concatenate(parts) if parts else fx[arr][:0]


def _groups(fx):
    """fragments that may share a call: the same mm_chain_dp scalars (under -x sr max_dist_x / max_dist_y go by the total length) -> ids"""
    out = {}
    for g, h in enumerate(fx["par"]):
        out.setdefault(tuple(int(v) for v in h), []).append(g)
    return out


def _params(h, gap_scale=1.0):
    from mm2chain import params
    return params.make_params(max_dist_x=h[0], max_dist_y=h[1], bw=h[2], max_skip=h[3], max_iter=h[4], gap_scale=gap_scale, is_cdna=h[7], n_segs=h[8])


@pytest.mark.parametrize("hpc", [0, 1])
@pytest.mark.parametrize("n_segs", [2, 3])
def test_sketch_and_matches_equal_the_reference(fx, n_segs, hpc):
    import mm2chain
    p = "hpc_" if hpc else ""
    ids = np.nonzero(np.diff(fx["frag_off"]) == n_segs)[0]
    frags = _sub(fx, ids)
    off, mini = mm2chain.sketch_frag_batch(frags, int(fx["k"]), int(fx["w"]), bool(hpc))
    want = [fx[p + "mini"][fx[p + "mini_off"][g]:fx[p + "mini_off"][g + 1]] for g in ids]
    assert np.array_equal(np.diff(off), [m.shape[0] for m in want]) and np.array_equal(mini, np.concatenate(want))
    idx = _index(fx, p)
    got = mm2chain.sketch_match_frag_batch(frags, idx, int(fx["mid_occ"]))
    m = _cat(fx, p + "match_off", p + "matches", ids)
    cnt = np.diff(fx[p + "match_off"])[ids]
    assert np.array_equal(np.diff(got["match_off"]), cnt) and np.array_equal(got["matches"], m)
    assert np.array_equal(got["rep_len"], fx[p + "rep_len1"][ids])
    assert np.array_equal(got["mini_off"], got["match_off"]) and np.array_equal(got["mini_pos"], _cat(fx, p + "match_off", p + "mini_pos1", ids))
    na = np.array([int(fx[p + "matches"]["n"][fx[p + "match_off"][g]:fx[p + "match_off"][g + 1]].sum()) for g in ids])
    assert np.array_equal(np.diff(got["anchor_off"]), na)
    idx.close()


def _check_final(fx, variant, got, ids, first=False):
    v = lambda name: fx[variant + "_" + name]
    t = "1" if first else ""
    assert np.array_equal(np.diff(got["anchor_off"]), v("na" + t)[ids])
    assert np.array_equal(np.diff(got["u_off"]), np.diff(v(f"u{t}_off"))[ids]) and np.array_equal(got["u"], _cat(fx, f"{variant}_u{t}_off", f"{variant}_u{t}", ids))
    assert np.array_equal(np.diff(got["b_off"]), np.diff(v(f"b{t}_off"))[ids]) and np.array_equal(got["b"], _cat(fx, f"{variant}_b{t}_off", f"{variant}_b{t}", ids))
    if first:
        assert np.array_equal(got["rep_len"], fx["rep_len1"][ids]) and np.array_equal(got["mini_pos"], _cat(fx, "match_off", "mini_pos1", ids))
        assert got["n_rechained"] == 0 and not got["rechained"].any()
    else:
        assert np.array_equal(got["rep_len"], v("rep_len")[ids]) and np.array_equal(got["mini_pos"], _cat(fx, variant + "_mp_off", variant + "_mini_pos", ids))
        assert np.array_equal(got["rechained"], v("rechained")[ids]) and got["n_rechained"] == int(v("rechained")[ids].sum())
    assert np.array_equal(np.diff(got["mini_off"]), [fx[variant + "_mp_off"][g + 1] - fx[variant + "_mp_off"][g] if not first else
                                                     fx["match_off"][g + 1] - fx["match_off"][g] for g in ids])


@pytest.mark.parametrize("variant", ["heap", "radix", "heap_for"])
def test_frag_chain_equals_the_reference(fx, variant, knobs):
    import mm2chain
    knobs("heap_sort", 0 if variant == "radix" else 1)
    skip = mm2chain.SeedSkip(FOR_ONLY) if variant == "heap_for" else None
    idx = _index(fx)
    n_re = 0
    for h, ids in _groups(fx).items():
        got = mm2chain.frag_chain_batch(_params(h), h[5], h[6], _sub(fx, ids), idx, int(fx["mid_occ"]), int(fx["max_occ"]), skip=skip)
        _check_final(fx, variant, got, np.array(ids))
        n_re += got["n_rechained"]
    assert n_re >= 12
    idx.close()


def test_max_occ_equal_mid_occ_is_the_first_pass(fx, knobs):
    import mm2chain
    knobs("heap_sort", 1)
    idx = _index(fx)
    for h, ids in _groups(fx).items():
        got = mm2chain.frag_chain_batch(_params(h), h[5], h[6], _sub(fx, ids), idx, int(fx["mid_occ"]), int(fx["mid_occ"]))
        _check_final(fx, "heap", got, np.array(ids), first=True)
    idx.close()


def test_single_segment_fragments_equal_read_chain_batch(fx):
    import mm2chain
    from mm2chain import params
    idx = _index(fx)
    reads = (fx["seq_off"], fx["seq"])
    nr = fx["seq_off"].size - 1
    P = params.make_params(max_dist_x=500, max_dist_y=300, bw=100, n_segs=1)
    a = mm2chain.read_chain_batch(P, 2, 25, reads, idx, int(fx["mid_occ"]))
    b = mm2chain.frag_chain_batch(P, 2, 25, (np.arange(nr + 1),) + reads, idx, int(fx["mid_occ"]), int(fx["mid_occ"]))
    for key in ("anchor_off", "u_off", "u", "b_off", "b", "rep_len", "mini_off", "mini_pos"):
        assert np.array_equal(a[key], b[key]), key
    assert a["u"].size > 0 and b["n_rechained"] == 0
    idx.close()


def _one_segment(fx):
    """every segment of the fixture, the zero-length ones included, as reads and as fragments of one segment each"""
    reads = (fx["seq_off"], fx["seq"])
    nr = fx["seq_off"].size - 1
    assert (np.diff(fx["seq_off"]) == 0).any()
    return nr, reads, (np.arange(nr + 1),) + reads


@pytest.mark.parametrize("hpc", [0, 1])
def test_single_segment_fragments_equal_the_sketch_and_match_entries(fx, hpc):
    """a read is a fragment of one segment: the fragment entries give what the read entries give, array for array"""
    import mm2chain
    nr, reads, frags = _one_segment(fx)
    a = mm2chain.sketch_batch(reads, int(fx["k"]), int(fx["w"]), bool(hpc))
    b = mm2chain.sketch_frag_batch(frags, int(fx["k"]), int(fx["w"]), bool(hpc))
    assert a[0].size == nr + 1 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].shape[0] > 0
    idx = _index(fx, "hpc_" if hpc else "")
    a = mm2chain.sketch_match_batch(reads, idx, int(fx["mid_occ"]))
    b = mm2chain.sketch_match_frag_batch(frags, idx, int(fx["mid_occ"]))
    assert set(a) == set(b) == {"match_off", "matches", "anchor_off", "rep_len", "mini_off", "mini_pos"}
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    assert (np.diff(a["match_off"]) > 0).any() and a["match_off"].size == nr + 1
    idx.close()


def test_chunks_are_cut_between_fragments(fx, knobs):
    import mm2chain
    knobs("heap_sort", 1)
    idx = _index(fx)
    h, ids = max(_groups(fx).items(), key=lambda kv: len(kv[1]))          # the pairs of 2 x 150: every kind but (f) is among them
    frags = _sub(fx, ids)
    one = mm2chain.frag_chain_batch(_params(h), h[5], h[6], frags, idx, int(fx["mid_occ"]), int(fx["max_occ"]))
    before = mm2chain.sketch_stats()
    knobs("read_chunk_bases", 700)                                 # two fragments of 300 bases a chunk
    many = mm2chain.frag_chain_batch(_params(h), h[5], h[6], frags, idx, int(fx["mid_occ"]), int(fx["max_occ"]))
    n_chunks = mm2chain.sketch_stats()["chunks"] - before["chunks"]
    assert n_chunks >= len(ids) // 2
    for key in ("anchor_off", "u_off", "u", "b_off", "b", "rep_len", "mini_off", "mini_pos", "rechained", "n_rechained"):
        assert np.array_equal(one[key], many[key]), key
    re = np.nonzero(one["rechained"])[0]
    assert np.unique(re // 2).size >= 4, "re-chained fragments in several chunks"
    for c in "abcde":
        assert np.intersect1d(fx["kind_" + c], ids).size >= 3
    _check_final(fx, "heap", many, np.array(ids))
    idx.close()


def test_every_fragment_a_chunk_of_its_own(fx, knobs):
    """read_chunk_bases = 1: a chunk boundary on both sides of every fragment of every kind, (f) included -- chunks whose segment range begins or ends with a
    zero-length segment, and one re-chained fragment per chunk.  Every group of fragments that may share a call; equal to the one-chunk run and to the reference"""
    import mm2chain
    knobs("heap_sort", 1)
    idx = _index(fx)
    seen = []
    for h, ids in _groups(fx).items():
        frags = _sub(fx, ids)
        knobs("read_chunk_bases", 1 << 27)
        one = mm2chain.frag_chain_batch(_params(h), h[5], h[6], frags, idx, int(fx["mid_occ"]), int(fx["max_occ"]))
        before = mm2chain.sketch_stats()["chunks"]
        knobs("read_chunk_bases", 1)
        many = mm2chain.frag_chain_batch(_params(h), h[5], h[6], frags, idx, int(fx["mid_occ"]), int(fx["max_occ"]))
        assert mm2chain.sketch_stats()["chunks"] - before == len(ids)
        for key in ("anchor_off", "u_off", "u", "b_off", "b", "rep_len", "mini_off", "mini_pos", "rechained", "n_rechained"):
            assert np.array_equal(one[key], many[key]), (h, key)
        _check_final(fx, "heap", many, np.array(ids))
        off, mini = mm2chain.sketch_frag_batch(frags, int(fx["k"]), int(fx["w"]))
        assert np.array_equal(mini, _cat(fx, "mini_off", "mini", ids))
        seen += ids
    for c in "abcdef":
        for n_segs in (2, 3):
            k = np.intersect1d(fx["kind_" + c], seen)
            assert (np.diff(fx["frag_off"])[k] == n_segs).sum() >= 3, (c, n_segs)
    f = fx["kind_f"]
    lens = [np.diff(fx["seq_off"][fx["frag_off"][g]:fx["frag_off"][g + 1] + 1]) for g in f]
    assert any(l[0] == 0 for l in lens) and any(l[-1] == 0 for l in lens) and any(l[0] and l[-1] and (l == 0).any() for l in lens)
    assert fx["heap_rechained"][f].any()
    idx.close()


def test_three_fragments_as_a_tuple_are_fragments(fx):
    """a tuple of exactly three fragments is not mistaken for (frag_off, seq_off, seq)"""
    import mm2chain
    ids = [int(g) for g in fx["kind_d"][:3]]
    fo, so, seq = _sub(fx, ids)
    as_lists = tuple([seq[so[s]:so[s + 1]].tobytes() for s in range(fo[g], fo[g + 1])] for g in range(3))
    a = mm2chain.sketch_frag_batch(as_lists, int(fx["k"]), int(fx["w"]))
    b = mm2chain.sketch_frag_batch((fo, so, seq), int(fx["k"]), int(fx["w"]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].size == 4


def _model(fx, frags, h, mid_occ, max_occ):
    lookup = sm.table_lookup(fx["keys"], fx["cr_off"], fx["n"])
    return [fm.map_frag(f, int(fx["w"]), int(fx["k"]), lookup, fx["pool"], _params(h), h[5], h[6], mid_occ, max_occ, heap=True) for f in frags]


def _equal_model(got, want):
    for g, r in enumerate(want):
        u, b = got["chains"][g]
        assert np.array_equal(u, r["u"]) and np.array_equal(b, r["b"]), g
        assert got["rep_len"][g] == r["rep_len"] and got["rechained"][g] == r["rechained"] and got["anchor_off"][g + 1] - got["anchor_off"][g] == r["n_anchors"]
        assert np.array_equal(got["mini_pos"][got["mini_off"][g]:got["mini_off"][g + 1]], r["mini_pos"])


@pytest.mark.parametrize("shape", ["all_empty", "empty_first", "empty_last", "alone", "255_one_base"])
def test_edge_shapes(fx, shape, knobs):
    import mm2chain
    knobs("heap_sort", 1)
    idx = _index(fx)
    g = int(fx["kind_b"][0])                                               # a pair that re-chains
    s = [fx["seq"][fx["seq_off"][i]:fx["seq_off"][i + 1]].tobytes() for i in range(fx["frag_off"][g], fx["frag_off"][g + 1])]
    frags = {"all_empty": [[b"", b""], s, [b"", b""]], "empty_first": [[b"", s[1]], s], "empty_last": [s, [s[0], b""]], "alone": [s],
             "255_one_base": [[bytes([c]) for c in (s[0] + s[1])[:255]]]}[shape]
    n_segs = len(frags[0])
    h = (500, 300, 100, 25, 5000, 2, 25, 0, n_segs)
    got = mm2chain.frag_chain_batch(_params(h), h[5], h[6], frags, idx, int(fx["mid_occ"]), int(fx["max_occ"]))
    _equal_model(got, _model(fx, frags, h, int(fx["mid_occ"]), int(fx["max_occ"])))
    off, mini = mm2chain.sketch_frag_batch(frags, int(fx["k"]), int(fx["w"]))
    want = [fm.collect_minimizers(f, int(fx["w"]), int(fx["k"])) for f in frags]
    assert np.array_equal(np.diff(off), [m.shape[0] for m in want]) and np.array_equal(mini, np.concatenate(want))
    if shape == "all_empty":
        assert off[1] == 0 and got["u_off"][1] == 0 and got["rechained"][0] == 0 and got["rechained"][1] == 1
    if shape == "255_one_base":
        assert mini.shape[0] == 0 and got["u"].size == 0
    idx.close()


def test_refusals(fx):
    import mm2chain
    idx = _index(fx)
    P2 = _params((500, 300, 100, 25, 5000, 2, 25, 0, 2))
    seq = np.frombuffer(b"ACGT" * 100, np.uint8)
    for frag_off, seq_off in (([0, 256], np.arange(257)),                   # 256 segments
                              ([0, 2, 2, 4], [0, 50, 100, 150, 200]),       # an empty fragment
                              ([0, 2, 3], [0, 50, 100, 150, 200]),          # frag_off does not end at n_reads
                              ([0, 3, 2, 4], [0, 50, 100, 150, 200])):      # not monotone
        with pytest.raises(mm2chain.Mm2cError, match=r"code -2"):
            mm2chain.frag_chain_batch(P2, 2, 25, (frag_off, seq_off, seq), idx, 8, 40)
        with pytest.raises(mm2chain.Mm2cError, match=r"code -2"):
            mm2chain.sketch_match_frag_batch((frag_off, seq_off, seq), idx, 8)
    with pytest.raises(mm2chain.Mm2cError, match=r"code -2.*n_segs"):       # three segments, par->n_segs = 2
        mm2chain.frag_chain_batch(P2, 2, 25, ([0, 2, 5], [0, 50, 100, 150, 200, 250], seq), idx, 8, 40)
    idx.close()


def test_best_chain_tie_takes_the_first(fx, knobs):
    """two chains of equal score, only the second spanning both segments: the reference's `max < score` scan keeps the first, which misses a segment, so the
    fragment re-chains.  Built by hand: an index over the pair's own minimizers whose hits lie on one diagonal each"""
    import mm2chain
    knobs("heap_sort", 1)
    k, w, mid_occ, max_occ = int(fx["k"]), int(fx["w"]), 8, 40
    rng = np.random.default_rng(5)
    segs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), 300).tobytes() for _ in range(2)]
    mini = fm.collect_minimizers(segs, w, k)
    pos, seg = (mini[:, 1] & np.uint64(0xFFFFFFFF)) >> np.uint64(1), mini[:, 1] >> np.uint64(32)

    def spaced(cands, n, after=-100):
        out = []
        for i in cands:
            if int(pos[i]) >= after + 30 and len(out) < n:
                out.append(int(i)); after = int(pos[i])
        assert len(out) == n
        return out
    s0, s1 = np.nonzero(seg == 0)[0], np.nonzero(seg == 1)[0]
    one_seg = spaced(s0, 4)                                                 # chain of four anchors of segment 0
    both = spaced(s0[s0 > one_seg[-1]], 2) + spaced(s1, 2)                  # two of segment 0, two of segment 1
    rep = int(s1[-1])                                                       # one repetitive minimizer: rep_len > 0
    assert rep not in both and len(set(mini[one_seg + both + [rep], 0] >> np.uint64(8))) == 9

    def build(rid_one, rid_both):
        rows = {}
        for rid, ids in ((rid_one, one_seg), (rid_both, both)):
            for i in ids:
                rows[int(mini[i, 0]) >> 8] = [rid << 32 | (int(pos[i]) + 1000) << 1 | (int(mini[i, 1]) & 1)]
        rows[int(mini[rep, 0]) >> 8] = [2 << 32 | (5000 * j) << 1 for j in range(1, mid_occ + 3)]
        keys = sorted(rows)
        n = np.array([len(rows[key]) for key in keys], np.uint32)
        cr = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
        return np.array(keys, np.uint64), cr, n, np.array([v for key in keys for v in rows[key]], np.uint64)
    h = (500, 600, 100, 25, 5000, 2, 25, 0, 2)
    for rids in ((0, 1), (1, 0)):                                           # whichever layout puts the one-segment chain first among the equals
        keys, cr, n, pool = build(*rids)
        r = fm.map_frag(segs, w, k, sm.table_lookup(keys, cr, n), pool, _params(h), h[5], h[6], mid_occ, max_occ, heap=True)
        u, b = r["first"]["u"], r["first"]["b"]
        n0 = int(u[0]) & 0xFFFFFFFF if u.size else 0
        if u.size == 2 and u[0] >> np.uint64(32) == u[1] >> np.uint64(32) and fm.n_chained_segs(u, b) == 1 and fm.n_chained_segs(u[1:], b[n0:]) == 2:
            break
    else:
        pytest.fail("no layout gives two chains of equal score with the one-segment chain first")
    assert r["rechained"]
    idx = mm2chain.MinimizerIndex(k, w, False, keys, cr, n, hits=pool)
    got = mm2chain.frag_chain_batch(_params(h), h[5], h[6], [segs], idx, mid_occ, max_occ)
    assert got["n_rechained"] == 1 and got["rechained"][0] == 1
    _equal_model(got, [r])
    first = mm2chain.frag_chain_batch(_params(h), h[5], h[6], [segs], idx, mid_occ, mid_occ)
    assert np.array_equal(first["u"], u) and np.array_equal(first["b"], b) and first["n_rechained"] == 0
    idx.close()
