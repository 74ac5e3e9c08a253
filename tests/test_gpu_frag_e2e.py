"""Fragments in, chains out (mm2c_frag_chain_batch) against the CPU model, fragment by fragment and bit for bit, at the shapes of tests/frag_data.py: the
re-chain decision over more than 64 chains with ties in every lane layout, the compaction of more than 256 flagged fragments, segment boundaries inside
repeats, a second pass of tens of thousands of anchors per fragment, and the HPC sketch.  tests/test_cpu_frag_shapes.py asserts that the model results used
here have those shapes."""
import numpy as np
import pytest
import torch

import frag_data as fd

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


@pytest.fixture(scope="module")
def sets():
    return {name: fd.get(name) for name in ("a", "b", "c", "d", "e_a", "e_c")}


def _calls(cpu, idx, heap, mid_occ, max_occ, chunk_bases=None):
    """one call per group; returns [(ids, result)] and the chunks the calls made"""
    import mm2chain
    out, n_chunks = [], 0
    for h, ids in cpu.groups:
        frags = [cpu.frags[g] for g in ids]
        cb = chunk_bases(frags) if chunk_bases else 1 << 27
        with mm2chain.tuned(heap_sort=int(heap), read_chunk_bases=int(cb)):
            before = mm2chain.sketch_stats()["chunks"]
            got = mm2chain.frag_chain_batch(fd.params_of(h), h[5], h[6], frags, idx, mid_occ, max_occ)
            made = mm2chain.sketch_stats()["chunks"] - before
        rule = len(fd.frag_chunks(frags, cb))
        assert made == rule, f"read_chunk_bases {cb}: {made} chunks, the host's rule gives {rule}"
        out.append((ids, got))
    return out


@pytest.mark.parametrize("name,heap", [("a", 1), ("a", 0), ("b", 1), ("b", 0), ("c", 1), ("c", 0), ("d", 1), ("e_a", 1), ("e_c", 1)])
def test_sets_against_the_model(sets, name, heap):
    import mm2chain
    cpu = sets[name]
    want = cpu.run(bool(heap))
    pool, idx = cpu.gpu_index()
    before = mm2chain.frag_stats()
    n_re = 0
    for ids, got in _calls(cpu, idx, heap, cpu.mid_occ, cpu.max_occ):
        stats = mm2chain.frag_stats()
        fd.compare(got, want, ids, cpu.names, f"set {name}, heap_sort {heap} (frag_stats {stats})")
        n_re += got["n_rechained"]
    after = mm2chain.frag_stats()
    model_re = sum(int(r["rechained"]) for r in want)
    assert after["fragments"] - before["fragments"] == len(cpu.frags) and after["rechained"] - before["rechained"] == model_re == n_re, (before, after, model_re)
    assert after["calls"] - before["calls"] == len(cpu.groups)
    idx.close(); pool.close()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_max_occ_equal_mid_occ_is_the_first_pass(sets, name):
    cpu = sets[name]
    want = cpu.run(True)
    pool, idx = cpu.gpu_index()
    for ids, got in _calls(cpu, idx, 1, cpu.mid_occ, cpu.mid_occ):
        fd.compare(got, want, ids, cpu.names, f"set {name}, max_occ = mid_occ", first=True)
    idx.close(); pool.close()


@pytest.mark.parametrize("name", ["c", "e_c"])
def test_matches_of_fragments_across_segment_boundaries(sets, name):
    import mm2chain
    cpu = sets[name]
    want = [r["first"] for r in cpu.run(True)]
    pool, idx = cpu.gpu_index()
    got = mm2chain.sketch_match_frag_batch(cpu.frags, idx, cpu.mid_occ)
    for g, r in enumerate(want):
        at = f"set {name}: fragment {g} ({cpu.names[g]})"
        m0, m1 = int(got["match_off"][g]), int(got["match_off"][g + 1])
        assert m1 - m0 == r["matches"].size, f"{at}: {m1 - m0} matches, the model {r['matches'].size}"
        for field in r["matches"].dtype.names:
            assert np.array_equal(got["matches"][field][m0:m1], r["matches"][field]), f"{at}: matches.{field} differs"
        assert int(got["rep_len"][g]) == r["rep_len"], f"{at}: rep_len {int(got['rep_len'][g])}, the model {r['rep_len']}"
        assert np.array_equal(got["mini_pos"][m0:m1], r["mini_pos"]), f"{at}: mini_pos differs"
        cap = int(got["anchor_off"][g + 1] - got["anchor_off"][g])
        assert cap == int(r["matches"]["n"].sum()), f"{at}: capacity {cap}, the model {int(r['matches']['n'].sum())}"
    assert np.array_equal(got["mini_off"], got["match_off"])
    off, mini = mm2chain.sketch_frag_batch(cpu.frags, cpu.k, cpu.w, bool(cpu.hpc))
    for g, r in enumerate(cpu.run(True)):
        assert np.array_equal(mini[off[g]:off[g + 1]], r["mini"]), f"set {name}: fragment {g} ({cpu.names[g]}): minimizers differ"
    idx.close(); pool.close()


@pytest.mark.parametrize("name,how", [("a", "two_or_three"), ("b", "two_or_three"), ("b", "300"), ("c", "two_or_three")])
def test_chunks_of_fragments(sets, name, how):
    """the second pass's compaction per chunk: chunks with none, one and all of their fragments flagged; equal to the one-chunk run and to the model"""
    cpu = sets[name]
    want = cpu.run(True)
    pool, idx = cpu.gpu_index()
    rule = fd.chunk_bases_for if how == "two_or_three" else (lambda frags: sum(len(s) for f in frags[:300] for s in f))
    one = _calls(cpu, idx, 1, cpu.mid_occ, cpu.max_occ)
    many = _calls(cpu, idx, 1, cpu.mid_occ, cpu.max_occ, chunk_bases=rule)
    for (ids, a), (_, b) in zip(one, many):
        fd.compare(b, want, ids, cpu.names, f"set {name}, chunks of {how}")
        for key in fd.KEYS:
            assert np.array_equal(a[key], b[key]), f"set {name}, chunks of {how}: {key} differs from the one-chunk run"
    idx.close(); pool.close()
