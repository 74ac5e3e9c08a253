"""GPU tests of mm2c_frag_chain_batch_gaps: fragments whose mates have different lengths in ONE call, every fragment chained with the (max_dist_x, max_dist_y)
map.c:305-314 gives for its total length -- against what the reference's own mm_map_frag did (tests/golden/ref_frag_gaps.npz, whose fragments include ones that
chain differently with any one pair for all: tests/test_cpu_frag_gaps_data.py) and, for the variants of the gap options, against the CPU model."""
import os

import numpy as np
import pytest
import torch

import frag_gaps_model as gm
import frag_model as fm
import sketch_model as sm

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_frag_gaps.npz")
KEYS = ("anchor_off", "u_off", "u", "b_off", "b", "rep_len", "mini_off", "mini_pos", "rechained", "n_rechained", "task_dists")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


@pytest.fixture(autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    with mm2chain.tuned(heap_sort=1):
        yield
    mm2chain.shutdown()


def _index(fx):
    import mm2chain
    return mm2chain.MinimizerIndex(int(fx["k"]), int(fx["w"]), False, fx["keys"], fx["cr_off"], fx["n"], pool=mm2chain.HitPool(fx["pool"]))


def _sub(fx, ids):
    fo, so, seq = fx["frag_off"], fx["seq_off"], fx["seq"]
    segs = [seq[so[s]:so[s + 1]] for g in ids for s in range(fo[g], fo[g + 1])]
    f = np.zeros(len(ids) + 1, np.int64); f[1:] = np.cumsum([fo[g + 1] - fo[g] for g in ids])
    o = np.zeros(len(segs) + 1, np.int64); o[1:] = np.cumsum([s.size for s in segs])
    return f, o, np.concatenate(segs) if segs else np.zeros(0, np.uint8)


def _cat(fx, off, arr, ids):
    parts = [fx[arr][fx[off][g]:fx[off][g + 1]] for g in ids]
    return np.concatenate(parts) if parts else fx[arr][:0]


def _params(h, x=None, y=None):
    """the call's scalars from a recorded row; the two distances are whatever the caller likes (the gaps entry ignores them)"""
    from mm2chain import params
    return params.make_params(max_dist_x=h[0] if x is None else x, max_dist_y=h[1] if y is None else y, bw=h[2], max_skip=h[3], max_iter=h[4], gap_scale=1.0,
                              is_cdna=h[7], n_segs=h[8])


def _gaps(fx, **kw):
    import mm2chain
    g = dict(zip(("is_sr", "max_gap", "max_gap_ref", "max_frag_len"), (int(v) for v in fx["gaps"])))
    g.update(kw)
    return mm2chain.frag_gaps(**g)


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


def _ids(fx, n_segs):
    return np.nonzero(np.diff(fx["frag_off"]) == n_segs)[0]


def _call(fx, idx, ids, max_occ=None, gaps=None, x=1, y=1):
    """all the fragments `ids` in one call; par's own distances are set to something no fragment has"""
    import mm2chain
    h = [int(v) for v in fx["par"][ids[0]]]
    return mm2chain.frag_chain_batch_gaps(_params(h, x, y), h[5], h[6], _sub(fx, ids), idx, int(fx["mid_occ"]), int(fx["max_occ"] if max_occ is None else max_occ),
                                          _gaps(fx) if gaps is None else gaps)


@pytest.mark.parametrize("n_segs", [2, 3])
def test_mixed_lengths_in_one_call_equal_the_reference(fx, n_segs):
    idx = _index(fx)
    ids = _ids(fx, n_segs)
    got = _call(fx, idx, ids)
    assert np.array_equal(got["task_dists"], fx["par"][ids, :2])
    assert len({tuple(r) for r in got["task_dists"].tolist()}) >= 12 and got["n_rechained"] >= 3
    _check_final(fx, "heap", got, ids)
    idx.close()


@pytest.mark.parametrize("n_segs", [2, 3])
def test_chunks_of_a_few_fragments(fx, n_segs):
    """read_chunk_bases so small that every few fragments are a chunk: the pairs follow their fragments, re-chained ones included"""
    import mm2chain
    idx = _index(fx)
    ids = _ids(fx, n_segs)
    one = _call(fx, idx, ids)
    before = mm2chain.sketch_stats()["chunks"]
    with mm2chain.tuned(read_chunk_bases=900):
        many = _call(fx, idx, ids)
    assert mm2chain.sketch_stats()["chunks"] - before >= len(ids) // 4
    for key in KEYS:
        assert np.array_equal(one[key], many[key]), key
    assert np.array_equal(many["task_dists"], fx["par"][ids, :2])
    _check_final(fx, "heap", many, ids)
    idx.close()


@pytest.mark.parametrize("n_segs", [2, 3])
def test_max_occ_equal_mid_occ_is_the_first_pass(fx, n_segs):
    idx = _index(fx)
    ids = _ids(fx, n_segs)
    got = _call(fx, idx, ids, max_occ=int(fx["mid_occ"]))
    _check_final(fx, "heap", got, ids, first=True)
    assert np.array_equal(got["task_dists"], fx["par"][ids, :2])
    idx.close()


@pytest.mark.parametrize("variant", ["max_gap_ref", "no_max_frag_len", "not_sr"])
def test_gap_options_against_the_model(fx, variant):
    """max_gap_ref > 0 is honoured, max_frag_len <= 0 gives max_gap, is_sr = 0 gives max_dist_y = max_gap: the model's map_frag per fragment with the model's pair"""
    idx = _index(fx)
    kw = {"max_gap_ref": {"max_gap_ref": 350}, "no_max_frag_len": {"max_frag_len": 0}, "not_sr": {"is_sr": 0}}[variant]
    gaps = _gaps(fx, **kw)
    ids = np.concatenate([_ids(fx, 2)[::3], fx["planted"][fx["planted"] < _ids(fx, 3)[0]]])       # pairs: every third, and the planted ones
    ids = np.unique(ids)
    got = _call(fx, idx, ids, gaps=gaps)
    q = gm.qlen_sums(fx["frag_off"], fx["seq_off"])[ids]
    want = gm.frag_dists(q, gaps.is_sr, gaps.max_gap, gaps.max_gap_ref, gaps.max_frag_len)
    assert np.array_equal(got["task_dists"], want)
    assert not np.array_equal(want, fx["par"][ids, :2])
    lookup = sm.table_lookup(fx["keys"], fx["cr_off"], fx["n"])
    fo, so = fx["frag_off"], fx["seq_off"]
    n_other = 0
    for j, g in enumerate(ids):
        h = [int(v) for v in fx["par"][g]]
        segs = [fx["seq"][so[s]:so[s + 1]].tobytes() for s in range(fo[g], fo[g + 1])]
        r = fm.map_frag(segs, int(fx["w"]), int(fx["k"]), lookup, fx["pool"], _params(h, int(want[j, 0]), int(want[j, 1])), h[5], h[6], int(fx["mid_occ"]),
                        int(fx["max_occ"]), heap=True)
        u, b = got["chains"][j]
        assert np.array_equal(u, r["u"]) and np.array_equal(b, r["b"]), (variant, g)
        assert got["rep_len"][j] == r["rep_len"] and got["rechained"][j] == r["rechained"] and got["anchor_off"][j + 1] - got["anchor_off"][j] == r["n_anchors"]
        n_other += not np.array_equal(u, fx["heap_u"][fx["heap_u_off"][g]:fx["heap_u_off"][g + 1]])
    if variant == "not_sr":
        assert (want[:, 1] == gaps.max_gap).all()
    else:
        assert n_other >= 2, "the option changes some fragment's chains"
    idx.close()


def test_fixed_length_fragments_equal_the_existing_entry(fx):
    """the fragments of the fixture's common pair through both entries: the existing one called with the scalars the formula gives"""
    import mm2chain
    idx = _index(fx)
    common = tuple(int(v) for v in fx["common"])
    for n_segs in (2, 3):
        ids = np.array([g for g in _ids(fx, n_segs) if tuple(int(v) for v in fx["par"][g, :2]) == common])
        assert ids.size >= 8
        h = [int(v) for v in fx["par"][ids[0]]]
        old = mm2chain.frag_chain_batch(_params(h), h[5], h[6], _sub(fx, ids), idx, int(fx["mid_occ"]), int(fx["max_occ"]))
        new = _call(fx, idx, ids)
        for key in KEYS[:-1]:
            assert np.array_equal(old[key], new[key]), key
        assert "task_dists" not in old and (new["task_dists"] == common).all()
    idx.close()


def test_a_fragment_of_total_length_zero_yields_nothing(fx):
    import mm2chain
    idx = _index(fx)
    g = int(fx["planted"][0])
    s = [fx["seq"][fx["seq_off"][i]:fx["seq_off"][i + 1]].tobytes() for i in range(fx["frag_off"][g], fx["frag_off"][g + 1])]
    h = [int(v) for v in fx["par"][g]]
    for frags in ([[b"", b""], s, [b"", b""]], [[b"", b""]]):
        got = mm2chain.frag_chain_batch_gaps(_params(h, 1, 1), h[5], h[6], frags, idx, int(fx["mid_occ"]), int(fx["max_occ"]), _gaps(fx))
        assert got["u_off"][1] == 0 and got["b_off"][1] == 0 and got["anchor_off"][1] == 0 and got["rep_len"][0] == 0
        assert tuple(got["task_dists"][0]) == (800, 100)
        if len(frags) == 3:
            assert tuple(got["task_dists"][1]) == tuple(fx["par"][g, :2]) and got["u_off"][3] == got["u_off"][2]
            assert np.array_equal(got["chains"][1][0], fx["heap_u"][fx["heap_u_off"][g]:fx["heap_u_off"][g + 1]])
            assert np.array_equal(got["chains"][1][1], fx["heap_b"][fx["heap_b_off"][g]:fx["heap_b_off"][g + 1]])
    idx.close()


def test_single_segment_fragments_of_mixed_lengths(fx):
    """n_segs = 1: every segment of the fixture a fragment of its own, against the model fragment by fragment"""
    import mm2chain
    idx = _index(fx)
    so = fx["seq_off"]
    segs = [fx["seq"][so[s]:so[s + 1]].tobytes() for s in range(0, so.size - 1, 2)]
    h = [int(v) for v in fx["par"][0]]; h[8] = 1
    got = mm2chain.frag_chain_batch_gaps(_params(h, 1, 1), h[5], h[6], [[s] for s in segs], idx, int(fx["mid_occ"]), int(fx["max_occ"]), _gaps(fx))
    want = gm.frag_dists([len(s) for s in segs], *[int(v) for v in fx["gaps"]])
    assert np.array_equal(got["task_dists"], want) and len({tuple(r) for r in want.tolist()}) >= 12
    lookup = sm.table_lookup(fx["keys"], fx["cr_off"], fx["n"])
    n_chains = 0
    for j, s in enumerate(segs):
        r = fm.map_frag([s], int(fx["w"]), int(fx["k"]), lookup, fx["pool"], _params(h, int(want[j, 0]), int(want[j, 1])), h[5], h[6], int(fx["mid_occ"]),
                        int(fx["max_occ"]), heap=True)
        u, b = got["chains"][j]
        assert np.array_equal(u, r["u"]) and np.array_equal(b, r["b"]) and got["rechained"][j] == r["rechained"], j
        n_chains += u.size
    assert n_chains >= 20
    idx.close()
