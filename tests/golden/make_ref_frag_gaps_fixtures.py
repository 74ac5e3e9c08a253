"""Fixture for per-fragment chaining distances: the reference's own mm_map_frag (map.o) with n_segs = 2 and 3 under the -x sr option values (max_gap 100,
max_frag_len 800, as tests/golden/frag_dump.c sets them) on fragments whose mates have DIFFERENT lengths, so that max_chain_gap_ref / max_chain_gap_qry
(map.c:305-314) differ from fragment to fragment.  frag_dump.c records the ten scalars of every mm_chain_dp call, so the reference itself states each
fragment's (max_dist_x, max_dist_y).  Same genome recipe and the same hand-set mid_occ / max_occ as make_ref_frag_fixtures.py; needs what build() leaves in
oracle/_ref/.  Output: tests/golden/ref_frag_gaps.npz (data only).

Layout.  k, w, mid_occ, max_occ; the index as keys / cr_off / n / pool; the fragments as frag_off / seq_off / seq; gaps = (is_sr, max_gap, max_gap_ref,
max_frag_len).  Per fragment: par (the nine integer scalars of its mm_chain_dp calls: max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, is_cdna,
n_segs), gap_scale, match_off (kept matches of the first pass), mini_pos1, rep_len1, and for the run with MM_F_HEAP_SORT heap_rechained, heap_rep_len,
heap_mp_off / heap_mini_pos, heap_na / heap_u / heap_b of the LAST call, heap_na1 / heap_u1 / heap_b1 of the FIRST, heap_a_off / heap_a (the anchors handed to
the last call).  common = the fixture's most frequent (max_dist_x, max_dist_y); planted = the fragments made so that chaining them with `common` instead of
their own pair gives other chains (asserted below with the CPU oracle)."""
import os
import struct
import subprocess
import sys
import tempfile
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))
from make_ref_frag_fixtures import ACGT, DATA, K, MAX_OCC, MID_OCC, REF_OBJ, W, csr, mutate, parse  # noqa: E402
from make_ref_sketch_fixtures import read_fasta  # noqa: E402

GAPS = (1, 100, -1, 800)                                                     # is_sr, max_gap, max_gap_ref, max_frag_len: what frag_dump.c runs with


def differs_with(par_h, pair, a):
    """the chains of anchor list `a` with the scalars par_h and with `pair` in the place of its two distances: do u / b differ?"""
    import oracle_binding as ob
    from mm2chain import params
    mk = lambda x, y: params.make_params(max_dist_x=int(x), max_dist_y=int(y), bw=int(par_h[2]), max_skip=int(par_h[3]), max_iter=int(par_h[4]), gap_scale=1.0,
                                         is_cdna=int(par_h[7]), n_segs=int(par_h[8]))
    if a.shape[0] == 0:
        return False
    u0, b0 = ob.mm_chain_dp(mk(par_h[0], par_h[1]), int(par_h[5]), int(par_h[6]), a)
    u1, b1 = ob.mm_chain_dp(mk(*pair), int(par_h[5]), int(par_h[6]), a)
    return not (np.array_equal(u0, u1) and np.array_equal(b0, b1))


def check_fixture(fx):
    """what keeps the fixture from going soft; tests/test_cpu_frag_gaps_data.py runs it again on the committed file"""
    n_segs = np.diff(fx["frag_off"])
    pairs = [tuple(int(v) for v in h[:2]) for h in fx["par"]]
    common = tuple(int(v) for v in fx["common"])
    assert Counter(pairs).most_common(1)[0][0] == common
    for ns in (2, 3):
        ids = np.nonzero(n_segs == ns)[0]
        assert len({pairs[g] for g in ids}) >= 12, (ns, "distinct pairs")
        re = [g for g in ids if fx["heap_rechained"][g]]
        assert len(re) >= 3 and len({pairs[g] for g in re}) >= 2, (ns, "re-chained fragments")
        dif = [g for g in ids if pairs[g] != common and
               differs_with(fx["par"][g], common, fx["heap_a"][fx["heap_a_off"][g]:fx["heap_a_off"][g + 1]])]
        assert len(dif) >= 5, (ns, "fragments whose chains need their own pair", dif)
        qs = np.array([fx["seq_off"][fx["frag_off"][g + 1]] - fx["seq_off"][fx["frag_off"][g]] for g in ids])
        mg, mfl = int(fx["gaps"][1]), int(fx["gaps"][3])
        assert (qs < mg).any() and (qs > mg).any() and (mfl - qs < mg).any() and (mfl - qs > mg).any(), (ns, "both sides of the two maxima")


def make_fragments(rng, mt, rep, spans):
    frags, planted = [], []
    a_copies, b_copies, spacers = spans
    for n_segs, fixed, big in ((2, 150, 380), (3, 100, 250)):
        def cut(ref, p, lens, gap, err=0.01):
            out = []
            for L in lens:
                out.append(mutate(rng, ref[p:p + L], err)); p += L + gap
            return out
        for _ in range(8):                                                   # the fixture's common pair: fixed-length mates
            frags.append(cut(mt, int(rng.integers(0, len(mt) - 1500)), [fixed] * n_segs, 80))
        for _ in range(16):                                                  # mates of random lengths
            frags.append(cut(mt, int(rng.integers(0, len(mt) - 1500)), [int(v) for v in rng.integers(30, 251, n_segs)], int(rng.integers(0, 120))))
        frags.append(cut(mt, 2000, [30] * n_segs, 10))                       # qlen_sum < max_gap
        frags.append(cut(mt, 4000, [big] * n_segs, 20))                      # max_frag_len - qlen_sum < max_gap
        for j, L in ((2, 150), (7, 120), (11, 90), (15, 180)):               # inside a copy of unit A: no chain with mid_occ, re-chained with max_occ
            frags.append(cut(rep, a_copies[j], [L] * n_segs, 20, 0.0))
        # long mates: own max_dist_x = max_frag_len - qlen_sum is SHORTER than the common one, and the mates lie further apart on the reference than that
        long_l, long_gap = (240, 400) if n_segs == 2 else (200, 300)
        for _ in range(4):
            planted.append(len(frags)); frags.append(cut(mt, int(rng.integers(0, len(mt) - 2500)), [long_l] * n_segs, long_gap, 0.0))
        # short mates: own max_dist_x is LONGER than the common one, and the mates lie further apart than the common one allows
        short_l, short_gap = (60, 560) if n_segs == 2 else (50, 540)
        for _ in range(4):
            planted.append(len(frags)); frags.append(cut(mt, int(rng.integers(0, len(mt) - 2500)), [short_l] * n_segs, short_gap, 0.0))
    return frags, planted


def main():
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "frag_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("kthread", "kalloc", "misc", "bseq", "sketch", "sdust", "index", "align", "hit", "map", "format", "pe", "esterr",
                                                      "splitidx", "ksw2_ll_sse", "ksw2_extz2_sse", "ksw2_extd2_sse", "ksw2_exts2_sse", "chain_oracle")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", "-I" + os.path.join(ROOT, "oracle"), os.path.join(HERE, "frag_dump.c")] + objs +
                          ["-o", dump, "-Wl,--wrap=mm_sketch", "-lz", "-lm", "-lpthread"])
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), os.path.join(tmp, "syn"), "--genome-mb", "0.03",
                           "--reads", "1", "--read-len", "1000", "--seed", "3"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(2027)
    rnd = lambda n: rng.choice(ACGT, n).tobytes()
    mt = read_fasta(os.path.join(DATA, "MT-human.fa"))[0]
    syn = read_fasta(os.path.join(tmp, "syn.ref.fa"))
    unit_a, unit_b = rnd(600), rnd(600)                                      # unit A 20 times (mid_occ <= 20 < max_occ), unit B 60 times, each behind 300 unique bases
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
    frags, planted = make_fragments(np.random.default_rng(4051), mt, rep, (a_copies, b_copies, spacers))
    segs = [s for f in frags for s in f]
    frag_off, _ = csr(frags)
    seq_off, _ = csr(segs)
    fpath = os.path.join(tmp, "frags.bin")
    with open(fpath, "wb") as f:
        f.write(struct.pack("<qq", len(frags), len(segs)) + frag_off.tobytes() + seq_off.tobytes() + b"".join(segs))
    o = os.path.join(tmp, "heap.bin")
    subprocess.check_call([dump, str(K), str(W), str(MID_OCC), str(MAX_OCC), "1", ref, fpath, o])
    pool, kt, F = parse(o, len(frags))
    assert all(d["n_calls"] >= 1 for d in F)
    out = {"k": np.array(K), "w": np.array(W), "mid_occ": np.array(MID_OCC), "max_occ": np.array(MAX_OCC), "pool": pool.copy(),
           "keys": kt["key"].copy(), "cr_off": kt["cr_off"].copy(), "n": kt["n"].copy(), "gaps": np.array(GAPS, np.int32),
           "frag_off": frag_off, "seq_off": seq_off, "seq": np.frombuffer(b"".join(segs), np.uint8), "planted": np.array(planted, np.int64)}
    out["match_off"], _ = csr([d["matches"] for d in F])
    _, out["mini_pos1"] = csr([d["mini_pos1"] for d in F])
    out["rep_len1"] = np.array([d["rep_len1"] for d in F], np.int32)
    out["par"] = np.array([d["calls"][-1]["h"] for d in F], np.int32)
    for d in F:                                                              # a re-chained fragment keeps its pair
        assert all(np.array_equal(c["h"], d["calls"][-1]["h"]) for c in d["calls"])
    out["gap_scale"] = np.array([d["calls"][-1]["gap_scale"] for d in F], np.float32)
    out["heap_rechained"] = np.array([d["n_calls"] == 2 for d in F], np.uint8)
    out["heap_rep_len"] = np.array([d["rep_len"] for d in F], np.int32)
    out["heap_mp_off"], out["heap_mini_pos"] = csr([d["mini_pos"] for d in F])
    for tag, which in (("", -1), ("1", 0)):
        out["heap_na" + tag] = np.array([d["calls"][which]["a"].shape[0] for d in F], np.int64)
        out[f"heap_u{tag}_off"], out["heap_u" + tag] = csr([d["calls"][which]["u"] for d in F])
        out[f"heap_b{tag}_off"], out["heap_b" + tag] = csr([d["calls"][which]["b"] for d in F])
    out["heap_a_off"], out["heap_a"] = csr([d["calls"][-1]["a"] for d in F])
    out["common"] = np.array(Counter(tuple(int(v) for v in h[:2]) for h in out["par"]).most_common(1)[0][0], np.int32)
    for key in list(out):
        if out[key].dtype == np.float64:                                     # an empty concatenation
            out[key] = out[key].astype(np.uint64)
    check_fixture(out)
    path = os.path.join(HERE, "ref_frag_gaps.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(frags), "fragments,", int(out["heap_rechained"].sum()), "re-chained,",
          len({tuple(h[:2]) for h in out["par"].tolist()}), "distinct pairs, common", tuple(out["common"]))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
