"""Paired reads through the fragment entries: what the tagging pass and the per-fragment lookups cost, and what the max_occ re-chain costs.

  python3 tools/frag_bench.py [--pairs 200000] [--read-len 150] [--genome-mb 50] [--reps 5] [--pkg DIR --single-only] [--varlen]

1. device time of sketch + lookups (mm2c_get_sketch_stats: HIP events around them) per base, for 2 x read-len pairs through mm2c_sketch_match_frag_batch and for
   the same segments as single reads through mm2c_sketch_match_batch (the entry and kernels of the single-segment path, which the fragment entries leave as they
   were), and their ratio.  Median of --reps runs after one warm-up.
2. mm2c_frag_chain_batch on the same pairs with the -x sr chaining scalars: the share of fragments re-chained and the device time of the second pass
   (mm2c_get_frag_stats), beside the wall time of the call with and without the second pass.
3. --varlen (instead of 1. and 2.): per-fragment chaining distances.  The same pairs with each mate trimmed to a random length (uniform in 50 .. read-len)
   (a) through ONE mm2c_frag_chain_batch_gaps call and (b) grouped by total length, one mm2c_frag_chain_batch call per group with that length's scalars (the only
   way without per-fragment distances), summed; (c) the untrimmed pairs through mm2c_frag_chain_batch and through mm2c_frag_chain_batch_gaps, and
   their segments as fragments of one segment through both.  Wall time of the
   calls, and device time from the library's counters: sketch + lookups (mm2c_get_sketch_stats), seed hits and window prepass + DP (mm2c_get_stage_stats; dp_ns is
   the sum of the chain plans' own kernel timers).  --reps calls each after one warm-up; (a) and (b) must give the same chains.
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


def chain_timed(fn):
    """one chaining call: wall time and the device times the library's counters hold for it"""
    mm2chain.sketch_stats(reset=True)
    mm2chain.stage_stats(reset=True)
    t0 = time.perf_counter()
    r = fn()
    wall = time.perf_counter() - t0
    sk, ss = mm2chain.sketch_stats(), mm2chain.stage_stats()
    return {"wall_s": wall, "sketch_lookup_s": (sk["sketch_ns"] + sk["lookup_ns"]) * 1e-9, "seed_s": ss["seed_ns"] * 1e-9, "dp_s": ss["dp_ns"] * 1e-9}, r


def add(recs):
    return {k: sum(x[k] for x in recs) for k in recs[0]}


def summary(recs):
    """--reps records of chain_timed -> every value and the median, per figure"""
    out = {k: {"values": [round(x[k], 5) for x in recs], "median": round(statistics.median(x[k] for x in recs), 5)} for k in recs[0]}
    out["device_s"] = {"median": round(statistics.median(x["sketch_lookup_s"] + x["seed_s"] + x["dp_s"] for x in recs), 5)}
    return out


def varlen(args, out, g, st, ins, idx, mid_occ, max_occ, fixed):
    L, n = args.read_len, args.pairs
    rng = np.random.default_rng(5)
    lens = rng.integers(min(50, L), L + 1, 2 * n)
    starts = np.stack([st, st + ins - lens[1::2]], axis=1).reshape(-1)           # mate 1 trimmed at its end, mate 2 at its start: the insert stays
    seq_off = np.zeros(2 * n + 1, np.int64)
    seq_off[1:] = np.cumsum(lens)

    pos = np.repeat(starts - seq_off[:-1], lens) + np.arange(seq_off[-1])
    seq = g[pos].copy()
    err = rng.random(seq.size) < 0.01
    seq[err] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(err.sum()))

    def cut(segs):
        """(frag_off, seq_off, seq) of the pairs whose segments are segs"""
        so = np.zeros(segs.size + 1, np.int64)
        so[1:] = np.cumsum(lens[segs])
        return np.arange(segs.size // 2 + 1, dtype=np.int64) * 2, so, seq[np.repeat(seq_off[segs] - so[:-1], lens[segs]) + np.arange(so[-1])]

    par = lambda t: params.make_params(max_dist_x=max(800 - t, 100), max_dist_y=max(t, 100), bw=100, max_skip=25, max_iter=5000, n_segs=2)
    gaps = mm2chain.frag_gaps(is_sr=1, max_gap=100, max_gap_ref=-1, max_frag_len=800)   # -x sr: what par(t) holds, per fragment
    allp = (np.arange(n + 1, dtype=np.int64) * 2, seq_off, seq)
    tot = lens.reshape(-1, 2).sum(1)
    groups = [(int(t), cut((2 * np.flatnonzero(tot == t)[:, None] + np.arange(2)[None, :]).reshape(-1))) for t in np.unique(tot)]
    one = lambda: mm2chain.frag_chain_batch_gaps(par(2 * L), 2, 25, allp, idx, mid_occ, max_occ, gaps)
    digest = lambda r: (int(r["u"].size), int(r["b"].shape[0]), int(r["u"].sum(dtype=np.uint64)), int(r["n_rechained"]))

    def per_group():
        recs, d = [], (0, 0, 0, 0)
        for t, fr in groups:
            rec, r = chain_timed(lambda: mm2chain.frag_chain_batch(par(t), 2, 25, fr, idx, mid_occ, max_occ))
            recs.append(rec)
            d = tuple((x + y) & (2 ** 64 - 1) for x, y in zip(d, digest(r)))
        return add(recs), d

    def timed(fn):
        rec, r = chain_timed(fn)
        return rec, digest(r)

    dists = one()["task_dists"].copy()                                        # (warm-up)
    per_group()
    a = [timed(one) for _ in range(args.reps)]
    b = [per_group() for _ in range(args.reps)]
    same = all(x[1] == y[1] for x in a for y in b)                            # chains, anchors in chains, sum of u, fragments re-chained
    out["varlen"] = {"pairs": n, "bases": int(seq_off[-1]), "mate_len": [int(lens.min()), int(lens.max())], "groups": len(groups),
                     "distinct_dist_pairs": int(np.unique(dists, axis=0).shape[0]), "chains": a[0][1][0], "same_chains": bool(same),
                     "one_gaps_call": summary([x[0] for x in a]), "one_call_per_length": summary([x[0] for x in b])}
    # (c) the pairs of fixed length: the call-scalar entry against the per-fragment one, turn about
    old = lambda: mm2chain.frag_chain_batch(par(2 * L), 2, 25, fixed, idx, mid_occ, max_occ)
    new = lambda: mm2chain.frag_chain_batch_gaps(par(2 * L), 2, 25, fixed, idx, mid_occ, max_occ, gaps)
    old(); new()
    o, w = [], []
    for _ in range(args.reps):
        o.append(timed(old)); w.append(timed(new))
    out["fixed_len"] = {"pairs": n, "read_len": L, "same_chains": bool(all(x[1] == y[1] for x, y in zip(o, w))),
                        "frag_chain_batch": summary([x[0] for x in o]), "frag_chain_batch_gaps": summary([x[0] for x in w])}
    # the same segments as fragments of ONE segment: the call-scalar entry takes the tile kernel there, the per-fragment one the general one-wave kernel
    p1 = params.make_params(max_dist_x=max(800 - L, 100), max_dist_y=max(L, 100), bw=100, max_skip=25, max_iter=5000, n_segs=1)
    single = (np.arange(2 * n + 1, dtype=np.int64), fixed[1], fixed[2])
    old1 = lambda: mm2chain.frag_chain_batch(p1, 2, 25, single, idx, mid_occ, max_occ)
    new1 = lambda: mm2chain.frag_chain_batch_gaps(p1, 2, 25, single, idx, mid_occ, max_occ, gaps)
    old1(); new1()
    o1, w1 = [], []
    for _ in range(args.reps):
        o1.append(timed(old1)); w1.append(timed(new1))
    out["fixed_len_single_segment"] = {"fragments": 2 * n, "same_chains": bool(all(x[1] == y[1] for x, y in zip(o1, w1))),
                                       "frag_chain_batch": summary([x[0] for x in o1]), "frag_chain_batch_gaps": summary([x[0] for x in w1])}
    same = same and out["fixed_len_single_segment"]["same_chains"]
    if not (same and out["fixed_len"]["same_chains"]):
        raise SystemExit("the entries disagree: " + json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-mb", type=float, default=50.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pkg", default=None, help="directory that holds the mm2chain package of another build (read before the import above)")
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--varlen", action="store_true", help="per-fragment chaining distances: mates of random length in one call against one call per total length")
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
    if args.varlen:
        mm2chain.tune("heap_sort", 1)
        varlen(args, out, g, st, ins, idx, mid_occ, max_occ, (frag_off, seq_off, seq))
        idx.close()
        mm2chain.shutdown()
        print(json.dumps(out, indent=1))
        return
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
