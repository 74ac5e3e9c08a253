"""The device sketch, the minimizer lookups (csrc/sketch.hip) and the index build (csrc/index_build.hip, build_index / cal_max_occ in csrc/mm2chain_sketch.cpp) at the
limits of their lanes: the reads, tables and sequence lists of tests/sketch_limit_data.py (tests/test_cpu_sketch_limit_data.py asserts that each reaches its limit,
that the models equal the reference there, and which deliberate error each family would catch) through sketch_batch, sketch_frag_batch, sketch_match_batch,
read_chain_batch, MinimizerIndex.build and cal_max_occ.  Every comparison is exact.  The models run once per module (sketch_limit_data.model)."""
import numpy as np
import pytest
import torch

import frag_model as fm
import index_model as im
import sketch_limit_data as sd
import sketch_model as sm
from helpers import assert_table, knob_setter, knobs  # noqa: F401 (knobs: a fixture)

pytestmark = pytest.mark.gpu

IDS = {S: "k%d-w%d-hpc%d" % S for S in sd.SETTINGS}
INT32_MAX = 2**31 - 1
# written out, so that collecting the tests builds no case (test_the_lists_below_are_the_data_modules compares)
COMMON = ("boundary", "first_window", "l_edges", "lag", "long", "registers")
FAMILIES = {(15, 10, 0): COMMON + ("ties",), (16, 10, 0): COMMON + ("palindrome", "ties"), (28, 255, 0): COMMON + ("palindrome", "ties"),
            (19, 5, 1): COMMON + ("span", "ties"), (5, 3, 1): COMMON + ("span", "ties"), (15, 1, 0): COMMON}
LOOKUPS = ("tandem_edges", "tandem_unfiltered", "mid_occ_1", "mid_occ_2", "mid_occ_50", "mid_occ_0", "mid_occ_2147483647", "rep_len_rounds")


@pytest.fixture(scope="module", autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


def test_the_lists_below_are_the_data_modules():
    assert {S: tuple(sorted(sd.families(S))) for S in sd.SETTINGS} == {S: tuple(sorted(f)) for S, f in FAMILIES.items()}
    assert tuple(c["name"] for c in sd.lookup_cases()) == LOOKUPS


# ---- the sketch ---------------------------------------------------------------------------------------------------------------------------------------------------
def _explain(S, case, r, read, got, ref):
    """the first differing minimizer of a read: its slot and its position"""
    n = min(got.shape[0], ref.shape[0])
    bad = np.nonzero((got[:n] != ref[:n]).any(axis=1))[0]
    i = int(bad[0]) if bad.size else n
    row = ref[i] if i < ref.shape[0] else got[i]
    pos = int(row[1]) >> 1 & 0x7FFFFFFF
    P = sd.slots(read, *S, light=True)[3]
    slot = P.index(pos) if pos in P else -1
    return (f"{IDS[S]}: {case} (read {r}, {len(read)} bases): {got.shape[0]} minimizers, the model {ref.shape[0]}; the first difference is minimizer {i}, "
            f"position {pos}, slot {slot} (slot {slot % sd.SC} of selection lane {slot // sd.SC}, position {pos % sd.CH} of lane {pos // sd.CH})")


def _check_reads(S, names):
    """sketch_batch over the reads of these cases, in their order, against the model"""
    import mm2chain
    reads, where = sd.batch(S)
    ref = sd.model(S)
    idx = [(n, r) for n in names for r in range(*where[n])]
    off, mini = mm2chain.sketch_batch([reads[r] for _, r in idx], *S)
    assert off.size == len(idx) + 1 and off[0] == 0 and off[-1] == mini.shape[0]
    for i, (name, r) in enumerate(idx):
        got = mini[off[i]:off[i + 1]]
        if not np.array_equal(got, ref[r]):
            raise AssertionError(_explain(S, name, r, reads[r], got, ref[r]))


@pytest.mark.parametrize("S", sd.SETTINGS, ids=list(IDS.values()))
def test_all_limit_reads_in_one_batch(S):
    """every case of a setting with its neighbours around it: a lane that reads past its read's edge shows in the next read"""
    _check_reads(S, [c["name"] for c in sd.cases(S)])


@pytest.mark.parametrize("S,family", [(S, f) for S in sd.SETTINGS for f in FAMILIES[S]], ids=lambda v: IDS.get(v, v) if isinstance(v, tuple) else v)
def test_family_alone(S, family):
    """the cases of one family in a batch of their own: other chunk, lane and tile numbers than in the whole batch"""
    _check_reads(S, [c["name"] for c in sd.cases(S) if c["family"] == family][::-1])


def _frag_expected(S, frag, first):
    """frag_model.collect_minimizers (map.c:64-77) over the model's sketches of the segments (reads first, first + 1, ... of batch(S))"""
    out, total = [], 0
    for i, s in enumerate(frag):
        m = sd.model(S)[first + i].copy()
        m[:, 1] += np.uint64((i << 32) + (total << 1))
        out.append(m)
        total += len(s)
    return np.concatenate(out)


@pytest.mark.parametrize("n_segs", [2, 3])
@pytest.mark.parametrize("S", sd.SETTINGS, ids=list(IDS.values()))
def test_the_batch_as_fragments(S, n_segs):
    """the same reads as segments of two- and three-segment fragments: the same sketch kernels with fr_tag on top; the empty segments of the boundary reads tie in
    owner()"""
    import mm2chain
    frags = sd.fragments(S, n_segs)
    off, mini = mm2chain.sketch_frag_batch(frags, *S)
    assert off.size == len(frags) + 1 and off[-1] == mini.shape[0]
    k, w, hpc = S
    first, where = sd.batch(S)[1]["boundary_reads"][0] // n_segs, sd.batch(S)[1]
    for g in (0, 1, first, first + 1, first + 2, len(frags) - 1):             # the shortcut over the cached sketches is frag_model's own result
        if sum(len(s) for s in frags[g]) < 2000:
            assert np.array_equal(_frag_expected(S, frags[g], g * n_segs), fm.collect_minimizers(frags[g], w, k, hpc)), g
    empty = sum(1 for f in frags for s in f if not s)
    assert empty >= 30, "fragments with empty segments"
    name_at = {r: n for n, (a, b) in where.items() for r in range(a, b)}
    for g, f in enumerate(frags):
        got, ref = mini[off[g]:off[g + 1]], _frag_expected(S, f, g * n_segs)
        assert np.array_equal(got, ref), f"{IDS[S]}: fragment {g} of {n_segs} segments ({[name_at[g * n_segs + i] for i in range(len(f))]}) differs"


# ---- lookups ------------------------------------------------------------------------------------------------------------------------------------------------------
def _index_of(c):
    import mm2chain
    k, w, hpc = c["kwh"]
    keys, cr, n, hits = c["table"]
    return mm2chain.MinimizerIndex(k, w, hpc, keys, cr, n, hits=hits)


def _flat(res):
    """sm.collect_matches' results per read as the arrays the library returns"""
    matches = sm.match_array([m for ms, _, _ in res for m in ms])
    match_off = np.concatenate([[0], np.cumsum([len(ms) for ms, _, _ in res])]).astype(np.int64)
    anchor_off = np.concatenate([[0], np.cumsum([sum(m[1] for m in ms) for ms, _, _ in res])]).astype(np.int64)
    return {"matches": matches, "match_off": match_off, "anchor_off": anchor_off, "mini_off": match_off,
            "rep_len": np.array([rl for _, rl, _ in res], np.int32), "mini_pos": np.array([p for _, _, mp in res for p in mp], np.uint64)}


@pytest.mark.parametrize("name", LOOKUPS)
def test_lookups_equal_the_model(name):
    import mm2chain
    c = sd.lookup_by_name(name)
    idx = _index_of(c)
    try:
        got = mm2chain.sketch_match_batch(c["reads"], idx, c["mid_occ"])
        ref = _flat(sd.lookup_model(c))
        for key in ("match_off", "anchor_off", "mini_off", "rep_len", "mini_pos"):
            if not np.array_equal(got[key], ref[key]):
                q = int(np.nonzero(got[key][:ref[key].size] != ref[key][:got[key].size])[0][0])
                raise AssertionError(f"{name}, mid_occ {c['mid_occ']}: {key} differs first at {q}: {got[key][q]} instead of {ref[key][q]}")
        for f in ("cr_off", "n", "q_pos", "q_span", "seg_tandem"):
            bad = np.nonzero(got["matches"][f] != ref["matches"][f])[0]
            assert bad.size == 0, f"{name}, mid_occ {c['mid_occ']}: matches.{f} differs at match {int(bad[0])} (read {int(np.searchsorted(ref['match_off'], bad[0], 'right')) - 1})"
    finally:
        idx.close()


def test_a_neighbour_in_another_chunk_changes_nothing(knobs):
    """[r, r, r[:len//2], r]: the last minimizer of a read and the first of the next share their key.  read_chain_batch cut between them (read_chunk_bases = one read,
    then two reads) gives the offsets, rep_len, mini_pos and chains of the uncut call, and the model's"""
    import mm2chain
    from mm2chain import params
    c = sd.lookup_by_name("tandem_edges")
    ref = _flat(sd.lookup_model(c))
    idx = _index_of(c)
    one = len(c["reads"][0])
    assert c["facts"]["group_cut"] == 2 * one
    out = {}
    try:
        for lim in (1 << 27, one, 2 * one):
            knobs("read_chunk_bases", lim)
            mm2chain.sketch_stats(reset=True)
            out[lim] = mm2chain.read_chain_batch(params.map_ont(), 3, 40, c["reads"], idx, c["mid_occ"])
            chunks = mm2chain.sketch_stats()["chunks"]
            assert (chunks == 1) if lim == 1 << 27 else (chunks >= 3), f"read_chunk_bases {lim}: {chunks} chunks"
    finally:
        idx.close()
    for lim, got in out.items():
        for key in ("anchor_off", "mini_off", "rep_len", "mini_pos"):
            assert np.array_equal(got[key], ref[key]), f"read_chunk_bases {lim}: {key} differs from the model"
        for key in ("u_off", "u", "b_off", "b"):
            assert np.array_equal(got[key], out[1 << 27][key]), f"read_chunk_bases {lim}: {key} differs from the uncut call"
    assert out[1 << 27]["b"].shape[0] > 0


# ---- index build --------------------------------------------------------------------------------------------------------------------------------------------------
def _check_build(seqs, S, ref, what, n_chunks=None):
    import mm2chain
    mm2chain.index_stats(reset=True)
    idx = mm2chain.MinimizerIndex.build(list(seqs), *S, mid_occ_frac=2e-4)    # an error ("not in (key, y) order") raises with its message: a failure
    try:
        if n_chunks is not None:
            assert mm2chain.index_stats()["chunks"] == n_chunks, f"{what}: {mm2chain.index_stats()['chunks']} chunks, the host's rule gives {n_chunks}"
        got = idx.export()
        assert_table(got, ref, what)
        assert idx.n_keys == ref[0].size and idx.n_hits == ref[3].size
        keys = np.array(sd.planted_keys(S), np.uint64)
        cr, n = idx.lookup(keys)
        rows = {int(a): (int(b), int(c)) for a, b, c in zip(ref[0], ref[1], ref[2])}
        for key, c, m in zip(keys.tolist(), cr.tolist(), n.tolist()):
            rc, rn = rows.get(key, (0, 0))
            assert m == rn and np.array_equal(got[3][c:c + m], ref[3][rc:rc + rn]), f"{what}: the planted key {key:#x} has {m} hits, the model {rn}"
        for frac in (2e-4, 0.25, 0.5, 1.0, 0.0):
            assert idx.cal_max_occ(frac) == im.cal_max_occ(ref[2], frac), f"{what}: cal_max_occ({frac})"
        assert idx.mid_occ == im.cal_max_occ(ref[2], 2e-4)
        return got
    finally:
        idx.close()


@pytest.mark.parametrize("n_seqs", sd.N_SEQS)
def test_build_over_lists_that_cross_a_bit_of_the_rid(n_seqs):
    S = (15, 10, 0)
    ref = im.build_from_minimizers(sd.list_minimizers(n_seqs, S))
    _check_build(sd.seq_list(n_seqs, S)[0], S, ref, f"{n_seqs} sequences")


def test_chunking_of_65537_sequences_does_not_change_the_index():
    import mm2chain
    S = (15, 10, 0)
    seqs = sd.seq_list(65_537, S)[0]
    ref = im.build_from_minimizers(sd.list_minimizers(65_537, S))
    lens = [len(s) for s in seqs]
    out = {}
    with knob_setter() as tune:
        for name, lim in sd.CHUNKINGS:
            tune("index_chunk_bases", lim)
            out[name] = _check_build(seqs, S, ref, f"65 537 sequences, {name}", n_chunks=len(sd.chunks(lens, lim)))
    for name, got in out.items():
        for a, b in zip(got, out["default"]):
            assert np.array_equal(a, b), f"{name}: the export differs from the one-chunk build"


@pytest.mark.parametrize("what", ["lists of 3 and 257", "the sketch cases"])
def test_hpc_builds(what):
    S = (19, 5, 1)
    if what == "the sketch cases":
        seqs = sd.hpc_build_seqs()
        _check_build(seqs, S, im.build_index(seqs, *S), "(19, 5, 1) over the HPC sketch cases")
    else:
        for n_seqs in (3, 257):
            _check_build(sd.seq_list(n_seqs, S)[0], S, im.build_from_minimizers(sd.list_minimizers(n_seqs, S)), f"(19, 5, 1), {n_seqs} sequences")


@pytest.mark.parametrize("n_keys", sd.OCC_KEYS)
def test_cal_max_occ_where_the_rank_sits_on_an_integer(n_keys):
    import mm2chain
    keys, cr, n, hits = sd.occ_table(n_keys)
    idx = mm2chain.MinimizerIndex(15, 10, 0, keys, cr, n, hits=hits)
    try:
        for frac in sd.OCC_FRACS:
            want = im.cal_max_occ(n, frac)
            assert want == (INT32_MAX if frac == 0.0 else sd.occ_rank(n_keys, frac) + 2)
            assert idx.cal_max_occ(frac) == want, f"{n_keys} keys, frac {frac}: rank {sd.occ_rank(n_keys, frac)}"
    finally:
        idx.close()
