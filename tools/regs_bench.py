"""Chains to regions on the device: what the regs plan (mm_gen_regs, csrc/chain_regs.hip) costs beside the device epilogue that feeds it.

  python3 tools/regs_bench.py [--reads 65536] [--per-read 5000] [--profile mixed] [--reps 5] [--seed 1]

The stream of bench.py (synth.make_stream) is chained on the device (DP, then the epilogue: mm2c_plan_chains_device), the numbers of chains and of chain anchors are read
back once to size the regs plan, and epilogue and regs plan then run --reps times each on the same data after one warm-up.  Times are the library's own HIP events
(mm2c_plan_last_epilogue_ms, mm2c_regplan_last_ms, mm2c_regplan_last_kernel_ms), medians.  fill_gbps: the 16 bytes of every chain anchor over the fill kernel's
time -- that kernel reads b once and is meant to be bound by it.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))
import mm2chain  # noqa: E402
from mm2chain import params, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--per-read", type=int, default=5000)
    ap.add_argument("--profile", default="mixed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    mm2chain.init()
    P = params.map_ont()
    off, a = synth.make_stream(args.profile, args.reads, args.per_read, seed=args.seed, device="cuda")
    n_reads, total = off.numel() - 1, a.shape[0]
    f = torch.empty(total, dtype=torch.int32, device="cuda")
    p = torch.empty_like(f)
    plan = mm2chain.ChainPlan(P, off.numpy())
    plan.run(a, f, p)
    epi = []
    for _ in range(args.reps + 1):
        u_off, u, b_off, b = plan.chains(a, f, p, 3, 40)
        torch.cuda.synchronize()
        epi.append(plan.last_epilogue_ms())
    n_u, n_b = int(u_off[-1]), int(b_off[-1])
    qlen = torch.full((n_reads,), 4 * args.per_read, dtype=torch.int32, device="cuda")
    hash_ = torch.from_numpy(np.array([mm2chain.read_hash(b"read%d" % r, 4 * args.per_read) for r in range(min(n_reads, 1024))], np.uint32).view(np.int32)).cuda()
    hash_ = hash_.repeat((n_reads + hash_.numel() - 1) // hash_.numel())[:n_reads].contiguous()
    rp = mm2chain.RegPlan(n_reads, n_u, n_b)
    regs = torch.empty((max(n_u, 1), 80), dtype=torch.uint8, device="cuda")
    ms, sort_ms, fill_ms = [], [], []
    for _ in range(args.reps + 1):
        rp.run(u_off, u, b_off, b, qlen, hash_, regs=regs)
        ties = rp.check()
        ms.append(rp.last_ms())
        s, fl = rp.last_kernel_ms()
        sort_ms.append(s); fill_ms.append(fl)
    med = lambda v: statistics.median(v[1:])
    lens = (u[:n_u] & 0xffffffff)
    out = {"profile": args.profile, "reads": n_reads, "anchors": total, "chains": n_u, "n_b": n_b, "longest_chain": int(lens.max()) if n_u else 0, "reads_with_ties": ties,
           "epilogue_ms": round(med(epi), 3), "regs_ms": round(med(ms), 3), "regs_sort_ms": round(med(sort_ms), 3), "regs_fill_ms": round(med(fill_ms), 3),
           "fill_gbps": round(16e-6 * n_b / med(fill_ms), 1) if n_b else 0.0, "regs_over_epilogue": round(med(ms) / med(epi), 4),
           "regs_ms_all": [round(v, 3) for v in ms[1:]], "epilogue_ms_all": [round(v, 3) for v in epi[1:]]}
    rp.close(); plan.close()
    mm2chain.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
