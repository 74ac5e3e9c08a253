"""Hits to mapping quality on the device: what the mapq plan (mm_join_long + mm_set_mapq, csrc/chain_mapq.hip) costs beside the region plan and the hit plan that feed it,
with and without the anchors out.

  python3 tools/mapq_bench.py [--reads 65536] [--per-read 5000] [--profile mixed] [--reps 5] [--seed 1] [--k 15] [--max-log-arg 4194304]

The stream of bench.py (synth.make_stream) is chained on the device (DP, then the epilogue: mm2c_plan_chains_device), the numbers of chains and of chain anchors are read
back once to size the plans, and region plan, hit plan and mapq plan then run --reps times on one stream after one warm-up, first with d_b_out == NULL, then with it.
Times are the library's own HIP events (mm2c_regplan_last_ms / _last_kernel_ms, mm2c_hitplan_last_ms, mm2c_mapqplan_last_ms / _last_kernel_ms), medians.
gather_gbps: 16 bytes read and 16 written per copied anchor over mapq_gather's time; fill_gbps: the 16 bytes of every chain anchor regs_fill reads over its time, on the
same b in the same run.  Prints one JSON line."""
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
    ap.add_argument("--max-log-arg", type=int, default=1 << 22)
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
    for _ in range(3):
        u_off, u, b_off, b = plan.chains(a, f, p, 3, 40)
        torch.cuda.synchronize()
        epi.append(plan.last_epilogue_ms())
    n_u, n_b = int(u_off[-1]), int(b_off[-1])
    qlen = torch.full((n_reads,), 4 * args.per_read, dtype=torch.int32, device="cuda")
    rep_len = (torch.arange(n_reads, dtype=torch.int32, device="cuda") * 131) % 900
    hash_ = torch.from_numpy(np.array([mm2chain.read_hash(b"read%d" % r, 4 * args.per_read) for r in range(min(n_reads, 1024))], np.uint32).view(np.int32)).cuda()
    hash_ = hash_.repeat((n_reads + hash_.numel() - 1) // hash_.numel())[:n_reads].contiguous()
    rp = mm2chain.RegPlan(n_reads, n_u, n_b)
    hp = mm2chain.HitPlan(n_reads, n_u)
    mp = mm2chain.MapqPlan(n_reads, n_u, n_b, args.max_log_arg)
    regs = torch.empty((max(n_u, 1), 80), dtype=torch.uint8, device="cuda")
    hits, fin = torch.empty_like(regs), torch.empty_like(regs)
    n_hits = torch.empty(max(n_reads, 1), dtype=torch.int32, device="cuda")
    n_out = torch.empty_like(n_hits)
    b_out = torch.empty((max(n_b, 1), 2), dtype=torch.int64, device="cuda")
    n_b_out = torch.empty(max(n_reads, 1), dtype=torch.int64, device="cuda")
    ho, mo = params.hit_opts(args.k), params.mapq_opts()
    T = {k: [] for k in ("regs", "fill", "hits", "mapq_null", "join", "gather", "mapq_b")}
    n_joined = n_beyond = 0
    for with_b in (False, True):
        for _ in range(args.reps + 1):
            rp.run(u_off, u, b_off, b, qlen, hash_, regs=regs)
            hp.run(ho, u_off, regs, regs_out=hits, n_out=n_hits)
            mp.run(mo, u_off, hits, n_hits, b_off, b, qlen, rep_len, regs_out=fin, n_out=n_out, b_out=b_out if with_b else None, n_b_out=n_b_out if with_b else None)
            rp.check(); hp.check()
            rc, n_joined, n_beyond = mp.counts()
            if rc not in (0, -3):
                mp.check()
            if with_b:
                T["regs"].append(rp.last_ms()); T["fill"].append(rp.last_kernel_ms()[1]); T["hits"].append(hp.last_ms())
                j, g = mp.last_kernel_ms()
                T["join"].append(j); T["gather"].append(g); T["mapq_b"].append(mp.last_ms())
            else:
                T["mapq_null"].append(mp.last_ms())
    med = lambda v: statistics.median(v[1:])
    per = (u_off[1:] - u_off[:-1])
    copied = int(n_b_out[:n_reads].sum())
    out = {"profile": args.profile, "reads": n_reads, "anchors": total, "regions": n_u, "chain_anchors": n_b, "hits": int(n_hits[:n_reads].sum()),
           "final_regions": int(n_out[:n_reads].sum()), "joins": int(n_joined), "beyond_table": int(n_beyond), "anchors_out": copied,
           "hits_per_read_max": int(n_hits[:n_reads].max()) if n_reads else 0, "reads_beyond_lds_class": int((n_hits[:n_reads] > MM2C_HIT_LDS_REGIONS).sum()),
           "regions_per_read_max": int(per.max()) if n_reads else 0,
           "epilogue_ms": round(statistics.median(epi[1:]), 3), "regs_ms": round(med(T["regs"]), 3), "regs_fill_ms": round(med(T["fill"]), 3), "hits_ms": round(med(T["hits"]), 3),
           "mapq_ms_no_anchors": round(med(T["mapq_null"]), 3), "mapq_ms_with_anchors": round(med(T["mapq_b"]), 3), "mapq_join_ms": round(med(T["join"]), 3),
           "mapq_gather_ms": round(med(T["gather"]), 3),
           "gather_gbps": round(32e-6 * copied / med(T["gather"]), 1) if copied else 0.0, "fill_gbps": round(16e-6 * n_b / med(T["fill"]), 1) if n_b else 0.0,
           "mapq_ms_no_anchors_all": [round(v, 3) for v in T["mapq_null"][1:]], "mapq_join_ms_all": [round(v, 3) for v in T["join"][1:]],
           "mapq_gather_ms_all": [round(v, 3) for v in T["gather"][1:]], "regs_ms_all": [round(v, 3) for v in T["regs"][1:]], "hits_ms_all": [round(v, 3) for v in T["hits"][1:]]}
    mp.close(); hp.close(); rp.close(); plan.close()
    mm2chain.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
