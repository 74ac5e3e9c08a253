"""The minimizer index built on the device (mm2c_minidx_build) against the host's mm_idx_gen on the same genome.

  python3 tools/index_bench.py [--genome-mb 50] [--rounds 3] [--chunk-bases N] [--threads 16] [--skip-host]

1. MinimizerIndex.build over the synthetic genome (tools/make_synth_genome.py) at map-ont k / w: after one warm-up build (code objects, device memory cache)
   `rounds` timed builds; per build the wall time (host clock around the call, which ends synchronised) and the stage split of mm2c_get_index_stats.
2. oracle/_ref/mm2_batchhost on the same genome with a handful of reads: the `index` stage it prints is the host's mm_idx_gen with -t threads, the thing the
   device build replaces.  Skipped when the binary is absent or with --skip-host.
Prints one JSON object."""
import argparse
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

STAGES = ("h2d_ns", "sketch_ns", "sort_ns", "group_ns", "occ_ns", "replicate_ns")


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


def one_build(packed, k, w):
    mm2chain.index_stats(reset=True)
    t0 = time.perf_counter()
    idx = mm2chain.MinimizerIndex.build(packed, k, w)
    wall = time.perf_counter() - t0
    st = mm2chain.index_stats()
    rec = {"wall_s": round(wall, 4), "chunks": st["chunks"], "bases": st["bases"], "minimizers": st["minimizers"], "keys": st["keys"], "mid_occ": idx.mid_occ}
    rec.update({k_[:-3] + "_s": round(st[k_] * 1e-9, 4) for k_ in STAGES})
    rec["stages_s"] = round(sum(st[k_] for k_ in STAGES) * 1e-9, 4)
    idx.close()
    return rec


def host_index(pre, threads):
    exe = os.path.join(ROOT, "oracle", "_ref", "mm2_batchhost")
    if not os.path.exists(exe):
        return {"skipped": "oracle/_ref/mm2_batchhost is not built"}
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", "300", exe, "-t", str(threads), pre + ".ref.fa", pre + ".reads.fa"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       env=dict(os.environ, MM2C_QUIET="1"))
    err = r.stderr.decode(errors="replace")
    rec = {"rc": r.returncode, "threads": threads, "process_wall_s": round(time.perf_counter() - t0, 3)}
    m = re.search(r"stages \(summed over mini-batches, they overlap\): index ([0-9.]+) s", err)
    if m:
        rec["index_s"] = float(m.group(1))
    else:
        rec["stderr_tail"] = err[-600:]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=50.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk-bases", type=int, default=0, help="mm2c_tune(\"index_chunk_bases\"); 0: the library's default")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    k, w = 15, 10                                                                      # map-ont
    out = {"argv": sys.argv[1:], "k": k, "w": w}
    with tempfile.TemporaryDirectory(prefix="mm2c_index_") as tmp:
        pre = os.path.join(tmp, "syn")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), pre, "--genome-mb", str(args.genome_mb), "--reads", "200"],
                              stdout=subprocess.DEVNULL)
        genome = read_fasta(pre + ".ref.fa")
        packed = pack(genome)
        out["genome"] = {"sequences": len(genome), "bases": int(packed[0][-1])}
        mm2chain.init()
        if args.chunk_bases > 0:
            mm2chain.tune("index_chunk_bases", args.chunk_bases)
        out["warm_up"] = one_build(packed, k, w)
        out["builds"] = [one_build(packed, k, w) for _ in range(args.rounds)]
        mm2chain.shutdown()
        walls = sorted(b["wall_s"] for b in out["builds"])
        out["device_build_wall_s_median"] = walls[len(walls) // 2] if walls else None
        if not args.skip_host:
            out["host_mm_idx_gen"] = host_index(pre, args.threads)
            if out["host_mm_idx_gen"].get("index_s") and walls:
                out["host_over_device"] = round(out["host_mm_idx_gen"]["index_s"] / walls[len(walls) // 2], 2)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
