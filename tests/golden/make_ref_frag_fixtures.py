"""Fragment fixtures: the reference's own mm_map_frag (map.o) with n_segs = 2 and 3 under the -x sr option values, on simulated pairs and triples from
ref_testdata/MT-human.fa and from a small synthetic genome with planted repeats, with mid_occ / max_occ set by hand so low that the repeats cross them.
Compiles tests/golden/frag_dump.c against the reference objects and the oracle that build() leaves in oracle/_ref/.  Output: tests/golden/ref_frag.npz (data only).

Layout.  k, w, mid_occ, max_occ; the index as keys (ascending) / cr_off / n / pool; the fragments as frag_off / seq_off / seq.  Per fragment, from the first pass
(max_occ = mid_occ): mini_off / mini (collect_minimizers), match_off / matches (mm2c_match_t) / mini_pos1 / rep_len1; par = the ten scalars of its mm_chain_dp
calls (max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, is_cdna, n_segs) and gap_scale.  Per variant v in heap (MM_F_HEAP_SORT, what -x sr sets),
radix (without it) and heap_for (with MM_F_FOR_ONLY): v_rechained (mm_chain_dp was called twice), v_rep_len (mm_tbuf_t.rep_len), v_mp_off / v_mini_pos, and for the
LAST call v_na (anchors handed in), v_u_off / v_u, v_b_off / v_b; for the FIRST call v_na1, v_u1_off / v_u1, v_b1_off / v_b1.  heap_a_off / heap_a: the anchor list
of the last call.  hpc_*: the same index, minimizers, matches, mini_pos1 and rep_len1 with MM_I_HPC (homopolymer-compressed k-mers), for the sketch and the lookups alone.
kind_a .. kind_f: the fragments of each kind the tests need (asserted below: at least three of each)."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_OBJ = os.path.join(ROOT, "oracle", "_ref")
DATA = os.path.join(HERE, "ref_testdata")
sys.path.insert(0, HERE)
from make_ref_sketch_fixtures import read_fasta  # noqa: E402

K, W, MID_OCC, MAX_OCC = 21, 11, 8, 40
MATCH = np.dtype([("cr_off", "<i8"), ("n", "<u4"), ("q_pos", "<u4"), ("q_span", "<u4"), ("seg_tandem", "<u4")])
ACGT = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, s, rate=0.01):
    a = np.frombuffer(s, np.uint8).copy()
    m = rng.random(a.size) < rate
    a[m] = rng.choice(ACGT, int(m.sum()))
    return a.tobytes()


def make_fragments(rng, mt, syn, rep, spans):
    """fragments of n_segs = 2 (2 x 150) and 3 (3 x 100); `spans` = where the repeat copies lie in `rep`"""
    frags = []
    for n_segs, L, step in ((2, 150, 230), (3, 100, 130)):
        def cut(ref, p, err=0.01):
            return [mutate(rng, ref[p + i * step:p + i * step + L], err) for i in range(n_segs)]
        for _ in range(6):                                                   # unique sequence: rep_len == 0
            frags.append(cut(mt, int(rng.integers(0, len(mt) - 600))))
        for c in syn:                                                        # the genome's own diverged repeat families: whatever they give
            for _ in range(3):
                frags.append(cut(c, int(rng.integers(0, len(c) - 600))))
        a_copies, b_copies, spacers = spans
        for j in (2, 7, 11, 15):                                             # all of it inside a copy of unit A (mid_occ <= occurrences < max_occ): no chain at first
            frags.append(cut(rep, a_copies[j], 0.0))
        for j in (5, 30):                                                    # inside unit B (occurrences >= max_occ): no chain in either pass
            frags.append(cut(rep, b_copies[j], 0.0))
        for j in (1, 4, 9, 13):                                              # first segment in the unique spacer, the rest in the copy of unit A behind it
            frags.append(cut(rep, spacers[j] + 300 - L - 20, 0.0))
        for j in (3, 6, 10, 14):                                             # unique first segments, the last one running into unit A: rep_len > 0, one chain over all
            frags.append(cut(rep, spacers[j] + 300 - (n_segs - 1) * step - L + 45, 0.0))
        ov = W + K - 1                                                       # a segment that begins with the last window of the one before: that window's minimizer
        for _ in range(4):                                                   # is the last of one list and the first of the next
            p = int(rng.integers(0, len(mt) - 600))
            frags.append([mt[p + i * (L - ov):p + i * (L - ov) + L] for i in range(n_segs)])
        for hole in range(n_segs):                                           # a zero-length segment inside a non-empty fragment
            f = cut(mt, int(rng.integers(0, len(mt) - 600)))
            f[hole] = b""
            frags.append(f)
        f = cut(rep, spacers[8] + 300 - L + 60, 0.0)                         # ... and one that re-chains
        f[n_segs - 1] = b""
        frags.append(f)
    return frags


def parse(path, n_frags):
    raw, pos = open(path, "rb").read(), 0
    n_pool, = struct.unpack_from("<q", raw, pos); pos += 8
    pool = np.frombuffer(raw, np.uint64, n_pool, pos); pos += 8 * n_pool
    n_keys, = struct.unpack_from("<q", raw, pos); pos += 8
    kt = np.frombuffer(raw, np.dtype([("key", "<u8"), ("cr_off", "<i8"), ("n", "<u4")]), n_keys, pos); pos += 20 * n_keys
    F = []
    for _ in range(n_frags):
        d = {}
        d["n_segs"], d["qlen"] = struct.unpack_from("<ii", raw, pos); pos += 8
        n, = struct.unpack_from("<q", raw, pos); pos += 8
        d["mini"] = np.frombuffer(raw, np.uint64, 2 * n, pos).reshape(n, 2); pos += 16 * n
        d["rep_len1"], = struct.unpack_from("<i", raw, pos); pos += 4
        n, = struct.unpack_from("<q", raw, pos); pos += 8
        d["matches"] = np.frombuffer(raw, MATCH, n, pos); pos += 24 * n
        d["mini_pos1"] = np.frombuffer(raw, np.uint64, n, pos); pos += 8 * n
        d["n_calls"], d["rep_len"] = struct.unpack_from("<ii", raw, pos); pos += 8
        n, = struct.unpack_from("<q", raw, pos); pos += 8
        d["mini_pos"] = np.frombuffer(raw, np.uint64, n, pos); pos += 8 * n
        d["calls"] = []
        for _ in range(d["n_calls"]):
            c = {"h": np.frombuffer(raw, np.int32, 9, pos), "gap_scale": struct.unpack_from("<f", raw, pos + 36)[0]}; pos += 40
            n, = struct.unpack_from("<q", raw, pos); pos += 8
            c["a"] = np.frombuffer(raw, np.uint64, 2 * n, pos).reshape(n, 2); pos += 16 * n
            n, = struct.unpack_from("<i", raw, pos); pos += 4
            c["u"] = np.frombuffer(raw, np.uint64, n, pos); pos += 8 * n
            n, = struct.unpack_from("<q", raw, pos); pos += 8
            c["b"] = np.frombuffer(raw, np.uint64, 2 * n, pos).reshape(n, 2); pos += 16 * n
            d["calls"].append(c)
        F.append(d)
    assert pos == len(raw)
    return pool, np.sort(kt, order="key"), F


def csr(parts):
    """offsets of the parts and, for arrays, the parts one after another"""
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return off, np.concatenate(parts) if parts and isinstance(parts[0], np.ndarray) else None


def main():
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "frag_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("kthread", "kalloc", "misc", "bseq", "sketch", "sdust", "index", "align", "hit", "map", "format", "pe", "esterr",
                                                      "splitidx", "ksw2_ll_sse", "ksw2_extz2_sse", "ksw2_extd2_sse", "ksw2_exts2_sse", "chain_oracle")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", "-I" + os.path.join(ROOT, "oracle"), os.path.join(HERE, "frag_dump.c")] + objs +
                          ["-o", dump, "-Wl,--wrap=mm_sketch", "-lz", "-lm", "-lpthread"])   # (the wrapper: frag_dump.c on zero-length segments)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), os.path.join(tmp, "syn"), "--genome-mb", "0.03",
                           "--reads", "1", "--read-len", "1000", "--seed", "3"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(2027)
    rnd = lambda n: rng.choice(ACGT, n).tobytes()
    mt = read_fasta(os.path.join(DATA, "MT-human.fa"))[0]
    syn = read_fasta(os.path.join(tmp, "syn.ref.fa"))
    # the planted repeats: unit A 20 times (mid_occ <= 20 < max_occ), unit B 60 times (>= max_occ), each copy behind 300 unique bases
    unit_a, unit_b = rnd(600), rnd(600)
    rep, a_copies, b_copies, spacers = b"", [], [], []
    for j in range(80):
        spacers.append(len(rep)); rep += rnd(300)
        (a_copies if j < 20 else b_copies).append(len(rep)); rep += unit_a if j < 20 else unit_b
    rep += rnd(300)
    ref = os.path.join(tmp, "ref.fa")
    with open(ref, "wb") as f:
        f.write(b">MT_human\n" + mt + b"\n")
        for i, c in enumerate(syn):
            f.write(b">chr%d\n" % (i + 1) + c + b"\n")
        f.write(b">repeats\n" + rep + b"\n")
    frags = make_fragments(rng, mt, syn, rep, (a_copies, b_copies, spacers))
    segs = [s for f in frags for s in f]
    frag_off, _ = csr(frags)
    seq_off, _ = csr(segs)
    fpath = os.path.join(tmp, "frags.bin")
    with open(fpath, "wb") as f:
        f.write(struct.pack("<qq", len(frags), len(segs)) + frag_off.tobytes() + seq_off.tobytes() + b"".join(segs))
    runs = {}
    for name, flags in (("heap", 1), ("radix", 0), ("heap_for", 3)):
        o = os.path.join(tmp, name + ".bin")
        subprocess.check_call([dump, str(K), str(W), str(MID_OCC), str(MAX_OCC), str(flags), ref, fpath, o])
        runs[name] = parse(o, len(frags))
    pool, kt, F = runs["heap"]
    out = {"k": np.array(K), "w": np.array(W), "mid_occ": np.array(MID_OCC), "max_occ": np.array(MAX_OCC), "pool": pool.copy(),
           "keys": kt["key"].copy(), "cr_off": kt["cr_off"].copy(), "n": kt["n"].copy(),
           "frag_off": frag_off, "seq_off": seq_off, "seq": np.frombuffer(b"".join(segs), np.uint8)}
    out["mini_off"], out["mini"] = csr([d["mini"] for d in F])
    out["match_off"], out["matches"] = csr([d["matches"] for d in F])
    _, out["mini_pos1"] = csr([d["mini_pos1"] for d in F])
    out["rep_len1"] = np.array([d["rep_len1"] for d in F], np.int32)
    assert all(d["n_calls"] >= 1 for d in F)
    out["par"] = np.array([d["calls"][-1]["h"] for d in F], np.int32)
    out["gap_scale"] = np.array([d["calls"][-1]["gap_scale"] for d in F], np.float32)
    for name, (pool_v, kt_v, Fv) in runs.items():
        assert np.array_equal(pool_v, pool) and np.array_equal(kt_v, kt)
        for d, e in zip(F, Fv):                                              # the flags change nothing before the seed hits
            assert np.array_equal(d["mini"], e["mini"]) and np.array_equal(d["matches"], e["matches"]) and d["rep_len1"] == e["rep_len1"]
        out[name + "_rechained"] = np.array([d["n_calls"] == 2 for d in Fv], np.uint8)
        out[name + "_rep_len"] = np.array([d["rep_len"] for d in Fv], np.int32)
        out[name + "_mp_off"], out[name + "_mini_pos"] = csr([d["mini_pos"] for d in Fv])
        for tag, which in (("", -1), ("1", 0)):
            out[name + "_na" + tag] = np.array([d["calls"][which]["a"].shape[0] for d in Fv], np.int64)
            out[name + f"_u{tag}_off"], out[name + "_u" + tag] = csr([d["calls"][which]["u"] for d in Fv])
            out[name + f"_b{tag}_off"], out[name + "_b" + tag] = csr([d["calls"][which]["b"] for d in Fv])
    out["heap_a_off"], out["heap_a"] = csr([d["calls"][-1]["a"] for d in F])
    o = os.path.join(tmp, "hpc.bin")
    subprocess.check_call([dump, str(K), str(W), str(MID_OCC), str(MAX_OCC), "5", ref, fpath, o])
    pool_h, kt_h, Fh = parse(o, len(frags))
    out.update({"hpc_pool": pool_h.copy(), "hpc_keys": kt_h["key"].copy(), "hpc_cr_off": kt_h["cr_off"].copy(), "hpc_n": kt_h["n"].copy()})
    out["hpc_mini_off"], out["hpc_mini"] = csr([d["mini"] for d in Fh])
    out["hpc_match_off"], out["hpc_matches"] = csr([d["matches"] for d in Fh])
    _, out["hpc_mini_pos1"] = csr([d["mini_pos1"] for d in Fh])
    out["hpc_rep_len1"] = np.array([d["rep_len1"] for d in Fh], np.int32)
    assert not np.array_equal(out["hpc_mini"], out["mini"]) and (out["hpc_rep_len1"] > 0).any()
    for key in list(out):
        if out[key].dtype == np.float64:                                     # an empty concatenation
            out[key] = out[key].astype(np.uint64)
    # the kinds
    kinds = {c: [] for c in "abcdef"}
    for g, d in enumerate(F):
        if d["n_calls"] == 2:
            kinds["a" if d["calls"][0]["u"].size == 0 else "b"].append(g)
        elif d["rep_len1"] > 0:
            kinds["c"].append(g)
        else:
            kinds["d"].append(g)
        m = d["mini"]
        if m.shape[0] > 1 and np.any((m[1:, 0] >> np.uint64(8) == m[:-1, 0] >> np.uint64(8)) & (m[1:, 1] >> np.uint64(32) != m[:-1, 1] >> np.uint64(32))):
            kinds["e"].append(g)
        lens = np.diff(seq_off[frag_off[g]:frag_off[g + 1] + 1])
        if (lens == 0).any() and lens.sum() > 0:
            kinds["f"].append(g)
    for c, v in kinds.items():
        for n_segs in (2, 3):
            have = [g for g in v if F[g]["n_segs"] == n_segs]
            print(f"kind {c}, n_segs {n_segs}: {len(have)} fragments")
            assert len(have) >= 3, f"kind {c} with n_segs = {n_segs}: only {len(have)} fragments -- adjust the planted repeats"
        out["kind_" + c] = np.array(v, np.int64)
    # the re-chain must make a difference somewhere, and the sort order too
    assert any(d["calls"][0]["u"].size != d["calls"][-1]["u"].size or not np.array_equal(d["calls"][0]["b"], d["calls"][-1]["b"]) for d in F if d["n_calls"] == 2)
    print("fragments whose chains differ between heap and radix order:",
          sum(not np.array_equal(d["calls"][-1]["b"], e["calls"][-1]["b"]) for d, e in zip(F, runs["radix"][2])))
    path = os.path.join(HERE, "ref_frag.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(frags), "fragments,", int(out["heap_rechained"].sum()), "re-chained")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
