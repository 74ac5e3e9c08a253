"""Reads in, chains out (mm2c_read_chain_batch) against a CPU pipeline built from pinned parts, read by read, at realistic shapes: a seeded 2 Mb genome
with planted repeat families and a 1 Mb region of ten diverged copies of one 101 kb unit, ONT-like reads from both strands, chimeras, N runs, lowercase,
degenerate reads, reads absent from the genome and one read of 10^6 bases with more than 10^6 anchors.  The CPU side: the key table of
tests/index_model.py, sketch_model.sketch_array and collect_matches, the oracle's collect_seed_hits (skip_seed included) and mm_chain_dp -- nothing there
calls the library.  Compared: mini_off / mini_pos, rep_len, the kept anchors per read, u and b; and sketch_match_batch's matches.  Every case asserts that
the shape it is there for occurred: chunks without anchors, an all-vs-all chunk whose anchors were all skipped, the long read alone in its chunk, a chunk of
many short reads, mid_occ = 1 and above every count, and batches with nothing to map."""
import numpy as np
import pytest
import torch

import index_model as im
import oracle_binding as ob
import sketch_model as sm
from helpers import knobs  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
MIN_CNT, MIN_SC = 3, 40
AVA = ob.F_NO_DIAG | ob.F_NO_DUAL
LONG = 1_000_000
COMP = np.array([3, 2, 1, 0], np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(autouse=True)
def _init():
    import mm2chain
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    mm2chain.init()
    yield
    mm2chain.shutdown()


# ---- data ----------------------------------------------------------------------------------------------------------------------------------------------

def _diverge(rng, s, d):
    s = s.copy()
    m = rng.random(s.size) < d
    s[m] = (s[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) % 4
    return s


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


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261015)
    bg = [rng.integers(0, 4, 250_000, dtype=np.uint8) for _ in range(4)]
    for L, copies, d in ((1500, 80, 0.02), (600, 250, 0.03), (300, 400, 0.01)):      # repeat families: some keys reach mid_occ
        unit = rng.integers(0, 4, L, dtype=np.uint8)
        for _ in range(copies):
            c, = rng.integers(0, 4, 1)
            p = int(rng.integers(0, bg[c].size - L))
            bg[c][p:p + L] = _diverge(rng, unit, float(rng.uniform(d / 2, d)))
    unit = rng.integers(0, 4, 101_000, dtype=np.uint8)                                # the long read's source: 10 copies at 1-2 %
    rep = np.concatenate([_diverge(rng, unit, float(rng.uniform(0.01, 0.02))) for _ in range(10)])
    genome = bg + [rep]
    txt = lambda s: ACGT[s].tobytes()
    reads = []
    for _ in range(36):                                                                # ONT-like, 2-30 kb, both strands
        reads.append(txt(_sample(rng, genome, int(rng.integers(2000, 30001)), 0.08)))
    for _ in range(3):                                                                 # chimeras across sequences
        reads.append(txt(_sample(rng, bg[:2], 6000, 0.06)) + txt(_sample(rng, bg[2:], 5000, 0.06)))
    s = bytearray(txt(_sample(rng, genome, 9000, 0.05)))
    s[3000:3400] = b"N" * 400; s[6000:6050] = b"N" * 50
    s[:1500] = s[:1500].lower()
    reads.append(bytes(s))                                                             # N runs and lowercase
    reads.append(txt(_sample(rng, genome, 7000, 0.05)).lower())
    degenerate = [b"", txt(rng.integers(0, 4, 7, dtype=np.uint8)), txt(rng.integers(0, 4, 15, dtype=np.uint8)),
                  txt(rng.integers(0, 4, 19, dtype=np.uint8)), b"N" * 3000, b"n" * 40, b""]
    absent = [txt(rng.integers(0, 4, int(L), dtype=np.uint8)) for L in (4000, 12000, 800)]
    p = int(rng.integers(0, rep.size - LONG - 4000))
    long_read = txt(_ont(rng, rep[p:p + LONG + 4000], 0.005)[:LONG])
    # the order places the degenerate reads together (a chunk without anchors), the long read in the middle and short reads around it
    reads = reads[:20] + degenerate + reads[20:30] + [long_read] + absent + reads[30:]
    return {"genome": [txt(s) for s in genome], "reads": reads, "long": reads.index(long_read), "n_degenerate": len(degenerate)}


def _cat(parts, dtype, width=None):
    parts = [np.asarray(p, dtype) for p in parts]
    if not parts or sum(p.shape[0] for p in parts) == 0:
        return np.zeros((0,) if width is None else (0, width), dtype)
    return np.concatenate([p.reshape((-1,) if width is None else (-1, width)) for p in parts])


class Cpu:
    """the CPU pipeline for one preset: the model index and the reads' minimizers, and collect_matches / collect_seed_hits / mm_chain_dp per mid_occ"""

    def __init__(self, refs, reads, k, w, hpc, P):
        self.k, self.w, self.hpc, self.P, self.reads = k, w, hpc, P, reads
        self.keys, self.cr_off, self.n, self.pool = im.build_index(refs, k, w, hpc)
        self.mid_occ = im.cal_max_occ(self.n)
        self.lookup = sm.table_lookup(self.keys, self.cr_off, self.n)
        self.mini = [sm.sketch_array(s, w, k, hpc) for s in reads]
        self.cache = {}

    def run(self, mid_occ, skip_kw=None):
        key = (mid_occ, skip_kw is not None)
        if key in self.cache:
            return self.cache[key]
        mo, ms, mp, rl, cap, ao, chains = [0], [], [], [], [0], [0], []
        for r, s in enumerate(self.reads):
            matches, rep_len, mini_pos = sm.collect_matches(self.mini[r], self.lookup, mid_occ)
            m = sm.match_array(matches)
            kw = skip_kw(r) if skip_kw else {}
            a = ob.collect_seed_hits(m, self.pool, len(s), **kw)
            chains.append(ob.mm_chain_dp(self.P, MIN_CNT, MIN_SC, a))
            ms.append(m); mp.append(mini_pos); rl.append(rep_len)
            mo.append(mo[-1] + m.size); cap.append(cap[-1] + int(m["n"].sum())); ao.append(ao[-1] + a.shape[0])
        ref = {"match_off": np.array(mo, np.int64), "matches": np.concatenate(ms) if ms else np.zeros(0, sm.MATCH_DTYPE),
               "mini_pos": _cat(mp, np.uint64), "rep_len": np.array(rl, np.int32), "cap": np.array(cap, np.int64), "anchor_off": np.array(ao, np.int64),
               "chains": chains}
        self.cache[key] = ref
        return ref

    def gpu_index(self):
        import mm2chain
        pool = mm2chain.HitPool(self.pool)
        return pool, mm2chain.MinimizerIndex(self.k, self.w, self.hpc, self.keys, self.cr_off, self.n, pool=pool)


@pytest.fixture(scope="module")
def presets(data):
    from mm2chain import params
    out = {"map_ont": Cpu(data["genome"], data["reads"], 15, 10, 0, params.map_ont())}
    short = [s for i, s in enumerate(data["reads"]) if i != data["long"]]                # the long read is map-ont's alone
    out["asm20"] = Cpu(data["genome"], short, 19, 10, 0, params.asm20())
    out["hpc"] = Cpu(data["genome"], short, 19, 10, 1, params.map_ont())
    return out


def _ava_reads(data):
    """all-vs-all: 30 overlapping reads from one 120 kb window (about 5x), a unique read, the degenerate reads, a chimera of the window"""
    rng = np.random.default_rng(77)
    win = np.frombuffer(data["genome"][1][50_000:170_000], np.uint8)
    win = np.searchsorted(ACGT, win).astype(np.uint8)
    txt = lambda s: ACGT[s].tobytes()
    reads = [txt(_sample(rng, [win], int(rng.integers(5000, 25001)), 0.06)) for _ in range(30)]
    reads.insert(11, txt(rng.integers(0, 4, 3000, dtype=np.uint8)))                    # maps only to itself: every hit on its own diagonal
    reads[20:20] = [b"", b"ACG", b"N" * 500, txt(rng.integers(0, 4, 15, dtype=np.uint8))]
    reads.append(txt(_sample(rng, [win], 4000, 0.05)) + txt(_sample(rng, [win], 4000, 0.05)))
    return reads, 11


@pytest.fixture(scope="module")
def ava(data):
    from mm2chain import params
    reads, unique = _ava_reads(data)
    cpu = Cpu(reads, reads, 15, 5, 0, params.ava_ont())                                # the index is the reads themselves: rid = read number
    n = len(reads)
    rank, ref_len = np.arange(n, dtype=np.int32), np.array([len(s) for s in reads], np.int32)
    q_lo, q_eq = np.arange(n, dtype=np.int32), np.ones(n, np.int32)                    # names read_000...: rank = name order, every read one of the names
    cpu.skip_arrays = (rank, ref_len, q_lo, q_eq)
    cpu.skip_kw = lambda r: dict(flag=AVA, ref_rank=rank, ref_len=ref_len, q_lo=int(q_lo[r]), q_eq=int(q_eq[r]))
    cpu.unique = unique
    return cpu


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------------------

def _chunks(reads, chunk_bases):
    """the host's rule (mm2chain_sketch.cpp, mm2c_read_chain_batch): a chunk takes reads while its bases stay within read_chunk_bases, at least one read"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in reads])]).astype(np.int64)
    cb, n, out, r0 = max(int(chunk_bases), 1), len(reads), [], 0
    while r0 < n:
        r1 = r0 + 1
        while r1 < n and off[r1 + 1] - off[r0] <= cb:
            r1 += 1
        out.append((r0, r1))
        r0 = r1
    return out


def _compare(got, ref, what):
    n = ref["rep_len"].size
    assert np.array_equal(got["mini_off"], ref["match_off"]), f"{what}: mini_off differs"
    for r in range(n):
        a, b = int(ref["match_off"][r]), int(ref["match_off"][r + 1])
        assert np.array_equal(got["mini_pos"][a:b], ref["mini_pos"][a:b]), f"{what}: read {r}: mini_pos differs"
    assert np.array_equal(got["rep_len"], ref["rep_len"]), f"{what}: rep_len differs at reads {np.nonzero(got['rep_len'] != ref['rep_len'])[0][:8]}"
    assert np.array_equal(got["anchor_off"], ref["anchor_off"]), \
        f"{what}: kept anchors differ at reads {np.nonzero(np.diff(got['anchor_off']) != np.diff(ref['anchor_off']))[0][:8]}"
    for r in range(n):
        u, b = got["chains"][r]
        ur, br = ref["chains"][r]
        assert np.array_equal(u, ur) and np.array_equal(b, br), f"{what}: read {r}: {u.size} chains, the oracle's mm_chain_dp {ur.size}; u or b differ"


def _compare_matches(sm_, ref, what):
    assert np.array_equal(sm_["match_off"], ref["match_off"]), f"{what}: match_off differs"
    assert np.array_equal(sm_["matches"], ref["matches"]), f"{what}: matches differ"
    assert np.array_equal(sm_["rep_len"], ref["rep_len"]), f"{what}: rep_len differs"
    assert np.array_equal(sm_["anchor_off"], ref["cap"]), f"{what}: capacities differ"
    assert np.array_equal(sm_["mini_pos"], ref["mini_pos"]), f"{what}: mini_pos differs"


def _run(cpu, mid_occ, skip=None, chunk_bases=1 << 27, idx=None):
    import mm2chain
    with mm2chain.tuned(read_chunk_bases=int(chunk_bases)):
        before = mm2chain.sketch_stats()["chunks"]
        got = mm2chain.read_chain_batch(cpu.P, MIN_CNT, MIN_SC, cpu.reads, idx, mid_occ, skip=skip)
        n_chunks = mm2chain.sketch_stats()["chunks"] - before
    assert n_chunks == len(_chunks(cpu.reads, chunk_bases)), f"chunk_bases {chunk_bases}: {n_chunks} chunks, the host's rule gives {len(_chunks(cpu.reads, chunk_bases))}"
    return got


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["map_ont", "asm20", "hpc"])
def test_presets_against_the_cpu_pipeline(presets, data, name):
    import mm2chain
    cpu = presets[name]
    ref = cpu.run(cpu.mid_occ)
    caps = np.diff(ref["cap"])
    assert (cpu.n >= cpu.mid_occ).sum() > 0 and (ref["rep_len"] > 0).sum() >= 3, f"{name}: repetitive keys and reads that meet them"
    assert sum(u.size > 0 for u, _ in ref["chains"]) >= 30 and (caps == 0).sum() >= 5
    if name == "map_ont":
        assert caps[data["long"]] >= LONG, f"the long read has {caps[data['long']]} anchors"
    pool, idx = cpu.gpu_index()
    got = _run(cpu, cpu.mid_occ, idx=idx)
    _compare(got, ref, name)
    _compare_matches(mm2chain.sketch_match_batch(cpu.reads, idx, cpu.mid_occ), ref, name)
    lens = [len(s) for s in cpu.reads]
    print(f"{name}: {len(lens)} reads, {sum(lens)} bases, {int(ref['anchor_off'][-1])} anchors, {sum(u.size for u, _ in ref['chains'])} chains, "
          f"mid_occ {cpu.mid_occ}" + (f", long read {int(caps[data['long']])} anchors" if name == "map_ont" else ""))
    idx.close(); pool.close()


def test_chunk_shapes_map_ont(presets, data):
    """read_chunk_bases below the long read, between, and above everything: identical outputs, equal to the CPU pipeline, and every chunk shape occurred"""
    cpu = presets["map_ont"]
    ref = cpu.run(cpu.mid_occ)
    caps = np.diff(ref["cap"])
    pool, idx = cpu.gpu_index()
    shapes = {"no_anchors": 0, "long_alone": 0, "many_short": 0}
    first = None
    for cb in (1 << 27, 200_000, 30_000, 5_000):
        got = _run(cpu, cpu.mid_occ, chunk_bases=cb, idx=idx)
        _compare(got, ref, f"map-ont, read_chunk_bases {cb}")
        if first is None:
            first = got
        for k in ("mini_off", "mini_pos", "rep_len", "anchor_off", "u_off", "u", "b_off", "b"):
            assert np.array_equal(got[k], first[k]), f"read_chunk_bases {cb}: {k} differs from one chunk"
        ch = _chunks(cpu.reads, cb)
        shapes["no_anchors"] += sum(int(caps[r0:r1].sum() == 0) for r0, r1 in ch)
        shapes["long_alone"] += sum((r0, r1) == (data["long"], data["long"] + 1) for r0, r1 in ch)
        shapes["many_short"] += sum(r1 - r0 >= 8 and not r0 <= data["long"] < r1 for r0, r1 in ch)
    print(f"map-ont chunk shapes over 4 sizes: {shapes}")
    assert all(v > 0 for v in shapes.values()), shapes
    idx.close(); pool.close()


def test_all_vs_all_self_mapping(ava):
    """-x ava-ont with the reads as the index: the self diagonals and the dual pairs are skipped, chunk by chunk too"""
    import mm2chain
    cpu = ava
    ref = cpu.run(cpu.mid_occ, cpu.skip_kw)
    caps, kept = np.diff(ref["cap"]), np.diff(ref["anchor_off"])
    assert caps.sum() > kept.sum() > 0
    assert caps[cpu.unique] > 0 and kept[cpu.unique] == 0, "the unique read hits only its own diagonal"
    no_dual = [ob.collect_seed_hits(ref["matches"][ref["match_off"][r]:ref["match_off"][r + 1]], cpu.pool, len(s), flag=ob.F_NO_DIAG,
                                    ref_rank=cpu.skip_arrays[0], ref_len=cpu.skip_arrays[1], q_lo=r, q_eq=1).shape[0] for r, s in enumerate(cpu.reads)]
    assert sum(no_dual) > kept.sum(), "dual pairs were skipped"
    skip = mm2chain.SeedSkip(AVA, *cpu.skip_arrays)
    pool, idx = cpu.gpu_index()
    _compare_matches(mm2chain.sketch_match_batch(cpu.reads, idx, cpu.mid_occ), ref, "ava-ont")
    shapes = {"no_anchors": 0, "all_skipped": 0, "many_short": 0}
    for cb in (1 << 27, 40_000, 1):
        got = _run(cpu, cpu.mid_occ, skip=skip, chunk_bases=cb, idx=idx)
        _compare(got, ref, f"ava-ont, read_chunk_bases {cb}")
        ch = _chunks(cpu.reads, cb)
        shapes["no_anchors"] += sum(int(caps[r0:r1].sum() == 0) for r0, r1 in ch)
        shapes["all_skipped"] += sum(int(caps[r0:r1].sum() > 0 and kept[r0:r1].sum() == 0) for r0, r1 in ch)
        shapes["many_short"] += sum(r1 - r0 >= 8 for r0, r1 in ch)
    lens = [len(s) for s in cpu.reads]
    print(f"ava-ont: {len(lens)} reads, {sum(lens)} bases, {int(caps.sum())} hits, {int(kept.sum())} anchors kept, chunk shapes {shapes}")
    assert all(v > 0 for v in shapes.values()), shapes
    idx.close(); pool.close()


def test_mid_occ_corners(presets):
    """mid_occ = 1: every key in the index is repetitive, only absent keys stay (n = 0): no anchors, no chains, rep_len over the minimizers with hits;
    the model's cal_max_occ; and above every count"""
    import mm2chain
    cpu = presets["asm20"]
    pool, idx = cpu.gpu_index()
    for mid in (1, cpu.mid_occ, int(cpu.n.max()) + 1):
        ref = cpu.run(mid)
        if mid == 1:
            assert ref["cap"][-1] == 0 and ref["match_off"][-1] > 0 and (ref["rep_len"] > 0).sum() >= 30
            assert (ref["matches"]["n"] == 0).all()
        if mid > cpu.n.max():
            assert (ref["rep_len"] == 0).all()
        got = _run(cpu, mid, idx=idx)
        _compare(got, ref, f"asm20, mid_occ {mid}")
        if mid == 1:
            assert got["u_off"][-1] == 0 and got["b_off"][-1] == 0 and got["anchor_off"][-1] == 0
        _compare_matches(mm2chain.sketch_match_batch(cpu.reads, idx, mid), ref, f"asm20, mid_occ {mid}")
    idx.close(); pool.close()


def test_batches_with_nothing_to_map(presets, knobs):
    import mm2chain
    cpu = presets["map_ont"]
    pool, idx = cpu.gpu_index()
    for reads in ([], [b"", b"N" * 5000, b"", b"nnnnNNNN", b""]):
        for cb in (1 << 27, 1):
            knobs("read_chunk_bases", cb)
            got = mm2chain.read_chain_batch(cpu.P, MIN_CNT, MIN_SC, reads, idx, cpu.mid_occ)
            for k in ("anchor_off", "u_off", "b_off", "mini_off"):
                assert got[k].size == len(reads) + 1 and not got[k].any(), (len(reads), k)
            assert got["rep_len"].size == len(reads) and not got["rep_len"].any()
            assert got["u"].size == got["b"].size == got["mini_pos"].size == 0
            sk = mm2chain.read_chain_batch(cpu.P, MIN_CNT, MIN_SC, reads, idx, cpu.mid_occ,
                                           skip=mm2chain.SeedSkip(AVA, np.arange(5), [1] * 5, [0] * len(reads), [1] * len(reads)))
            assert not sk["anchor_off"].any() and sk["u"].size == 0
        s = mm2chain.sketch_match_batch(reads, idx, cpu.mid_occ)
        assert s["match_off"].size == len(reads) + 1 and not s["match_off"].any() and s["matches"].size == 0
    idx.close(); pool.close()
