"""Sketch + lookup on the device (mm2c_sketch_match_batch) and the batched host with and without MM2_BATCH_GPU_SKETCH=1.

  python3 tools/sketch_bench.py [--reads 120000] [--genome-mb 50] [--batch-bases 100000000] [--threads 16] [--skip-e2e]

1. device time of the sketch and of the lookups (mm2c_get_sketch_stats: HIP events around them) and G bases/s, on the reads of the e2e workload (synthetic
   genome with planted repeats, 10 kb ONT-like reads, tools/make_synth_genome.py) and on long reads (10^5 and 10^6 bases).  The index is a stand-in built here
   from the genome's own minimizers (every key with its occurrences; mid_occ from the 2e-4 fraction as mm_idx_cal_max_occ): the lookups do the same work as
   against the reference's index.
2. oracle/_ref/mm2_batchhost on the same files twice, default and MM2_BATCH_GPU_SKETCH=1: wall seconds, the host's stage sums, the library's stage and sketch
   lines, and the PAF md5, which must be the same.
Prints one JSON object."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))
import mm2chain  # noqa: E402


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


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return off, np.frombuffer(b"".join(seqs), np.uint8)


def stand_in_index(genome, k=15, w=10):
    off, mini = mm2chain.sketch_batch(pack(genome), k, w, False)
    rid = np.repeat(np.arange(len(genome), dtype=np.uint64), np.diff(off))
    key = mini[:, 0] >> np.uint64(8)
    order = np.argsort(key, kind="stable")
    key = key[order]
    pool = (rid[order] << np.uint64(32)) | (mini[order, 1] & np.uint64(0xFFFFFFFF))
    keys, start, n = np.unique(key, return_index=True, return_counts=True)
    cnt = np.sort(n)[::-1]
    mid_occ = int(cnt[int(len(cnt) * 2e-4)]) + 1 if len(cnt) else 1
    hp = mm2chain.HitPool(pool)
    return mm2chain.MinimizerIndex(k, w, 0, keys, start.astype(np.int64), n.astype(np.uint32), pool=hp), mid_occ


def device_pass(reads, idx, mid_occ, batch_bases):
    mm2chain.sketch_stats(reset=True)
    t0, i, n_matches = time.perf_counter(), 0, 0
    while i < len(reads):
        j, b = i, 0
        while j < len(reads) and (j == i or b + len(reads[j]) <= batch_bases):
            b += len(reads[j]); j += 1
        r = mm2chain.sketch_match_batch(pack(reads[i:j]), idx, mid_occ)
        n_matches += int(r["match_off"][-1])
        i = j
    wall = time.perf_counter() - t0
    st = mm2chain.sketch_stats()
    dev = (st["sketch_ns"] + st["lookup_ns"]) * 1e-9
    return {"reads": len(reads), "bases": st["bases"], "minimizers": st["minimizers"], "matches": st["matches"], "calls": st["calls"],
            "upload_s": round(st["h2d_ns"] * 1e-9, 4), "sketch_s": round(st["sketch_ns"] * 1e-9, 4), "lookup_s": round(st["lookup_ns"] * 1e-9, 4),
            "device_s": round(dev, 4), "gbases_per_s_device": round(st["bases"] / dev / 1e9, 2) if dev else None,
            "wall_s_incl_host_copies": round(wall, 2)}


def run_host(pre, threads, mini_batch, gpu_sketch):
    env = dict(os.environ, MM2_MINI_BATCH=str(mini_batch), MM2C_QUIET="1")
    env.pop("MM2_BATCH_GPU_SKETCH", None)
    if gpu_sketch:
        env["MM2_BATCH_GPU_SKETCH"] = "1"
    paf = pre + (".gpu_sketch.paf" if gpu_sketch else ".default.paf")
    t0 = time.perf_counter()
    with open(paf, "wb") as fo:
        r = subprocess.run(["timeout", "-k", "10", "300", os.path.join(ROOT, "oracle", "_ref", "mm2_batchhost"), "-t", str(threads), pre + ".ref.fa", pre + ".reads.fa"],
                           stdout=fo, stderr=subprocess.PIPE, env=env)
    rec = {"wall_s": round(time.perf_counter() - t0, 3), "rc": r.returncode, "paf_md5": hashlib.md5(open(paf, "rb").read()).hexdigest()}
    err = r.stderr.decode(errors="replace")
    for key, pat in (("host_stage_sums", r"stages \(summed over mini-batches, they overlap\): (.*)"), ("library_stage_stats", r"inside the library \(mm2c_get_stage_stats\): (.*)"),
                     ("sketch_stats", r"sketch and lookups on the device \(mm2c_get_sketch_stats\): (.*)"), ("process", r"(HIP start-up .*)")):
        m = re.search(pat, err)
        if m:
            rec[key] = m.group(1).strip()
    if r.returncode != 0:
        rec["stderr_tail"] = err[-600:]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=120000)
    ap.add_argument("--genome-mb", type=float, default=50.0)
    ap.add_argument("--batch-bases", type=int, default=100_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    out = {"argv": sys.argv[1:]}
    with tempfile.TemporaryDirectory(prefix="mm2c_sketch_") as w:
        pre = os.path.join(w, "syn")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), pre, "--genome-mb", str(args.genome_mb), "--reads", str(args.reads)],
                              stdout=subprocess.DEVNULL)
        mm2chain.init()
        genome = read_fasta(pre + ".ref.fa")
        idx, mid_occ = stand_in_index(genome)
        out["index"] = {"keys": idx.size, "hits": idx.pool.size, "mid_occ": mid_occ}
        reads = read_fasta(pre + ".reads.fa")
        device_pass(reads[:2000], idx, mid_occ, args.batch_bases)                      # warm-up: code objects, device memory cache
        out["ont_10kb"] = device_pass(reads, idx, mid_occ, args.batch_bases)
        g = b"".join(genome)
        rng = np.random.default_rng(1)
        for name, n, L in (("long_1e5", 200, 100_000), ("long_1e6", 20, 1_000_000)):
            st = rng.integers(0, len(g) - L, n)
            out[name] = device_pass([g[s:s + L] for s in st], idx, mid_occ, args.batch_bases)
        idx.close()
        mm2chain.shutdown()
        if not args.skip_e2e:
            out["e2e"] = {"workload": f"{args.reads} reads, {args.genome_mb} Mb genome, -t {args.threads}, -K {args.batch_bases}",
                          "default": run_host(pre, args.threads, args.batch_bases, False), "gpu_sketch": run_host(pre, args.threads, args.batch_bases, True)}
            out["e2e"]["paf_identical"] = out["e2e"]["default"]["paf_md5"] == out["e2e"]["gpu_sketch"]["paf_md5"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
