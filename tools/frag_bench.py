"""Paired reads through the fragment entries: what the tagging pass and the per-fragment lookups cost, and what the max_occ re-chain costs.

  python3 tools/frag_bench.py [--pairs 200000] [--read-len 150] [--genome-mb 50] [--reps 5] [--pkg DIR --single-only]

1. device time of sketch + lookups (mm2c_get_sketch_stats: HIP events around them) per base, for 2 x read-len pairs through mm2c_sketch_match_frag_batch and for
   the same segments as single reads through mm2c_sketch_match_batch (the entry and kernels of the single-segment path, which the fragment entries leave as they
   were), and their ratio.  Median of --reps runs after one warm-up.
2. mm2c_frag_chain_batch on the same pairs with the -x sr chaining scalars: the share of fragments re-chained and the device time of the second pass
   (mm2c_get_frag_stats), beside the wall time of the call with and without the second pass.
--pkg DIR takes the mm2chain package (with its built library) from another checkout, and --single-only stops after the single-read figure of 1., which needs
nothing a build without the fragment entries lacks: together they measure the PARENT commit's mm2c_sketch_match_batch on the same bases (same seeds).
The index is built on the device from the genome (k = 21, w = 11, as -x sr); mid_occ is the index's 2e-4 fraction, max_occ five times that (the ratio of
-x sr's 1000 / 5000, which a genome of this size never reaches).  Prints one JSON object."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = sys.argv[sys.argv.index("--pkg") + 1] if "--pkg" in sys.argv[1:-1] else os.path.join(ROOT, "minimap2-fpga_amd")
sys.path.insert(0, PKG)
import mm2chain  # noqa: E402
from mm2chain import params  # noqa: E402


def read_fasta(path):
    seqs, cur = [], None
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                cur = []
                seqs.append(cur)
            else:
                cur.append(line.rstrip(b"\n"))
    return [b"".join(s) for s in seqs]


def device_s(fn):
    mm2chain.sketch_stats(reset=True)
    t0 = time.perf_counter()
    fn()
    wall = time.perf_counter() - t0
    st = mm2chain.sketch_stats()
    return (st["sketch_ns"] + st["lookup_ns"]) * 1e-9, st, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-mb", type=float, default=50.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pkg", default=None, help="directory that holds the mm2chain package of another build (read before the import above)")
    ap.add_argument("--single-only", action="store_true")
    args = ap.parse_args()
    L, out = args.read_len, {"argv": sys.argv[1:], "library": mm2chain.LIB_PATH}
    with tempfile.TemporaryDirectory(prefix="mm2c_frag_") as w:
        pre = os.path.join(w, "syn")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), pre, "--genome-mb", str(args.genome_mb), "--reads", "1"],
                              stdout=subprocess.DEVNULL)
        genome = read_fasta(pre + ".ref.fa")
    mm2chain.init()
    idx = mm2chain.MinimizerIndex.build(genome, 21, 11)
    mid_occ, max_occ = idx.mid_occ, 5 * idx.mid_occ
    out["index"] = {"keys": idx.n_keys, "hits": idx.n_hits, "mid_occ": mid_occ, "max_occ": max_occ}
    rng = np.random.default_rng(3)
    g = np.frombuffer(b"".join(genome), np.uint8)
    st = rng.integers(0, g.size - 600, args.pairs)
    ins = rng.integers(2 * L, 500, args.pairs)
    starts = np.stack([st, st + ins - L], axis=1).reshape(-1)                 # both mates on the strand mm_map_frag sees them on
    seq = g[(starts[:, None] + np.arange(L)[None, :]).reshape(-1)].copy()
    err = rng.random(seq.size) < 0.01
    seq[err] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(err.sum()))
    seq_off = np.arange(2 * args.pairs + 1, dtype=np.int64) * L
    frag_off = np.arange(args.pairs + 1, dtype=np.int64) * 2
    single = lambda: mm2chain.sketch_match_batch((seq_off, seq), idx, mid_occ)
    frag = lambda: mm2chain.sketch_match_frag_batch((frag_off, seq_off, seq), idx, mid_occ)
    bases = int(seq.size)
    single()                                                                  # warm-up: code objects, device memory cache
    s = [device_s(single) for _ in range(args.reps)]
    if args.single_only:
        ms = statistics.median(x[0] for x in s)
        out["sketch_lookup"] = {"bases": bases, "pairs": args.pairs, "single_device_s": [round(x[0], 5) for x in s], "single_ns_per_base": round(ms / bases * 1e9, 4),
                                "single_split_s": {"sketch": s[-1][1]["sketch_ns"] * 1e-9, "lookup": s[-1][1]["lookup_ns"] * 1e-9}}
        idx.close()
        mm2chain.shutdown()
        print(json.dumps(out, indent=1))
        return
    frag()
    f = [device_s(frag) for _ in range(args.reps)]
    ms, mf = statistics.median(x[0] for x in s), statistics.median(x[0] for x in f)
    out["sketch_lookup"] = {"bases": bases, "pairs": args.pairs, "single_device_s": [round(x[0], 5) for x in s], "frag_device_s": [round(x[0], 5) for x in f],
                            "single_ns_per_base": round(ms / bases * 1e9, 4), "frag_ns_per_base": round(mf / bases * 1e9, 4), "ratio_frag_over_single": round(mf / ms, 4),
                            "single_split_s": {"sketch": s[-1][1]["sketch_ns"] * 1e-9, "lookup": s[-1][1]["lookup_ns"] * 1e-9},
                            "frag_split_s": {"sketch": f[-1][1]["sketch_ns"] * 1e-9, "lookup": f[-1][1]["lookup_ns"] * 1e-9}}
    # the chains: -x sr scalars for a total length of 2 L (map.c:306-314; options.c:123-140)
    P = params.make_params(max_dist_x=max(800 - 2 * L, 100), max_dist_y=max(2 * L, 100), bw=100, max_skip=25, max_iter=5000, n_segs=2)
    mm2chain.tune("heap_sort", 1)
    chain = lambda mo: mm2chain.frag_chain_batch(P, 2, 25, (frag_off, seq_off, seq), idx, mid_occ, mo)
    chain(max_occ)
    rec = []
    for _ in range(max(args.reps // 2, 1)):
        mm2chain.frag_stats(reset=True)
        t0 = time.perf_counter(); r = chain(max_occ); w2 = time.perf_counter() - t0
        fs = mm2chain.frag_stats()
        t0 = time.perf_counter(); chain(mid_occ); w1 = time.perf_counter() - t0
        rec.append({"wall_s_two_pass": round(w2, 4), "wall_s_one_pass": round(w1, 4), "second_pass_device_s": round(fs["rechain_ns"] * 1e-9, 5),
                    "rechained": int(r["n_rechained"]), "share_rechained": round(r["n_rechained"] / args.pairs, 5),
                    "with_rep_len": int((r["rep_len"] > 0).sum()), "chains": int(r["u"].size)})
    out["rechain"] = rec
    idx.close()
    mm2chain.shutdown()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
