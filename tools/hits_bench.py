"""Regions to hits on the device: what the hit plan (mm_set_parent + mm_select_sub, csrc/chain_hits.hip) costs beside the region plan and the device epilogue that feed it.

  python3 tools/hits_bench.py [--reads 65536] [--per-read 5000] [--profile mixed] [--reps 5] [--seed 1] [--k 15]

The stream of bench.py (synth.make_stream) is chained on the device (DP, then the epilogue: mm2c_plan_chains_device), the numbers of chains and of chain anchors are read
back once to size the plans, and epilogue, region plan and hit plan then run --reps times each on the same data after one warm-up, in the same process.  Times are the
library's own HIP events (mm2c_plan_last_epilogue_ms, mm2c_regplan_last_ms, mm2c_hitplan_last_ms), medians.  hits_gbps: the 80 bytes of every region read twice and of
every hit written once over the hit plan's time.  Prints one JSON line."""
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
from mm2chain._native import MM2C_HIT_LDS_REGIONS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--per-read", type=int, default=5000)
    ap.add_argument("--profile", default="mixed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--k", type=int, default=15)
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
    hp = mm2chain.HitPlan(n_reads, n_u)
    regs = torch.empty((max(n_u, 1), 80), dtype=torch.uint8, device="cuda")
    hits = torch.empty_like(regs)
    n_out = torch.empty(max(n_reads, 1), dtype=torch.int32, device="cuda")
    opt = params.hit_opts(args.k)
    reg_ms, hit_ms = [], []
    for _ in range(args.reps + 1):
        rp.run(u_off, u, b_off, b, qlen, hash_, regs=regs)
        hp.run(opt, u_off, regs, regs_out=hits, n_out=n_out)
        rp.check()
        n_hits = hp.check()
        reg_ms.append(rp.last_ms()); hit_ms.append(hp.last_ms())
    med = lambda v: statistics.median(v[1:])
    per = (u_off[1:] - u_off[:-1])
    h = hits.cpu().numpy().reshape(-1).view(mm2chain.REG_DTYPE)
    uo, no = u_off.cpu().numpy(), n_out.cpu().numpy()[:n_reads]
    keep = np.zeros(max(n_u, 1), bool)
    idx = np.repeat(uo[:-1], no) + (np.arange(int(no.sum())) - np.repeat(np.cumsum(no) - no, no))
    keep[idx] = True
    prim = int((h["id"] == h["parent"])[keep].sum())
    out = {"profile": args.profile, "reads": n_reads, "anchors": total, "regions": n_u, "hits": int(n_hits), "primaries": prim,
           "regions_per_read_mean": round(n_u / max(n_reads, 1), 1), "regions_per_read_max": int(per.max()) if n_reads else 0,
           "reads_beyond_lds_class": int((per > MM2C_HIT_LDS_REGIONS).sum()),
           "epilogue_ms": round(med(epi), 3), "regs_ms": round(med(reg_ms), 3), "hits_ms": round(med(hit_ms), 3),
           "hits_gbps": round((160e-6 * n_u + 80e-6 * n_hits) / med(hit_ms), 1) if n_u else 0.0,
           "hits_over_epilogue": round(med(hit_ms) / med(epi), 4), "hits_over_regs": round(med(hit_ms) / med(reg_ms), 4),
           "hits_ms_all": [round(v, 3) for v in hit_ms[1:]], "regs_ms_all": [round(v, 3) for v in reg_ms[1:]], "epilogue_ms_all": [round(v, 3) for v in epi[1:]]}
    hp.close(); rp.close(); plan.close()
    mm2chain.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
