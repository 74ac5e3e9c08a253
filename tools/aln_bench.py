#!/usr/bin/env python3
"""Device time of the alignment-task plan on ONT-like regions: by default 98 304 regions of about 11.6 kb, the shape profiles/update_extra.md used, one
region a read.  The reads are exact slices of a random 16 Mb contig on the forward strand; the anchors lie 40 bases apart with a shift of 12 to 40 bases on the read
axis at one step in twenty (the long gaps the two seed filters work on), so the anchors' diagonal drifts as an ONT read's does; the plan does not look at whether
the bases under an anchor match.  Times are the plan's HIP events (aln_plan with aln_scan, aln_emit, aln_gather), the median of --reps runs after a warm-up, every
run on a fresh copy of the anchors (their flags are in/out).  gather_gbps: the pool bytes written per second; gather_rw_gbps counts the bytes read as well (a read
base is one byte, a reference base half a byte); copy_gbps: a device-to-device copy of the pool's size in the same process, read plus written.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=98304)
    ap.add_argument("--anchors", type=int, default=289)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--slots", type=int, default=2048)
    args = ap.parse_args()
    import mm2chain
    from mm2chain import params, RefSeq, AlnPlan, REG_DTYPE, ALN_REG_DTYPE
    mm2chain.init()
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(args.seed)
    n, na, k, step = args.regions, args.anchors, 15, 40
    glen, qlen = 1 << 24, 14 + step * na + 420
    G = torch.randint(0, 4, (glen,), device=dev, dtype=torch.uint8, generator=g)
    w = G.view(-1, 8).to(torch.int64)
    S = sum(w[:, j] << (4 * j) for j in range(8)).cpu().numpy().astype(np.uint32)
    ref = RefSeq(np.array([0], np.uint64), np.array([glen], np.uint32), S)
    start = torch.randint(0, glen - qlen - 6000, (n,), device=dev, generator=g) + 5500
    reads = torch.empty((n, qlen), dtype=torch.uint8, device=dev)
    ar = torch.arange(qlen, device=dev)
    for c0 in range(0, n, 2048):
        reads[c0:c0 + 2048] = G[(start[c0:c0 + 2048, None] + ar[None, :])]
    p = 14 + step * torch.arange(na, device=dev)
    hit = torch.rand((n, na), device=dev, generator=g) < 0.05
    shift = torch.randint(12, 41, (n, na), device=dev, generator=g) * (torch.randint(0, 2, (n, na), device=dev, generator=g) * 2 - 1)
    shift = torch.where(hit, shift, torch.zeros_like(shift)); shift[:, 0] = 0
    d = torch.cumsum(shift.clamp(min=-(step - 1)), 1)
    y = (p[None, :] + 200 + d).clamp(min=k - 1)
    y = torch.cummax(y, 1).values.clamp(max=qlen - 1)
    x = start[:, None] + 200 + p[None, :]
    b0 = torch.stack([x, (k << 32) | y], 2).contiguous()                                # [n, na, 2] int64: rid 0, forward
    yh = y.cpu().numpy(); xh = x.cpu().numpy()
    regs = np.zeros(n, REG_DTYPE)
    regs["cnt"], regs["as"], regs["mlen"] = na, 0, na * k
    regs["rs"], regs["re"], regs["qs"], regs["qe"] = xh[:, 0] + 1 - k, xh[:, -1] + 1, yh[:, 0] + 1 - k, yh[:, -1] + 1
    off = lambda per: torch.arange(n + 1, device=dev, dtype=torch.int64) * per
    u_off, b_off, read_off = off(1), off(na), off(qlen)
    d_regs = torch.from_numpy(regs.view(np.uint8).reshape(n, -1)).to(dev)
    o = params.aln_opts("map-ont")
    caps = dict(items=n * (na // 4 + 8), tasks=n * (na // 4 + 8), pool=n * (2 * qlen + 2 * 12000 + 64))
    plan = AlnPlan(n, caps["items"], caps["tasks"], caps["pool"], n * na, n * qlen, n_slots=args.slots)
    outs, T = None, []
    for rep in range(args.reps + 1):
        b = b0.clone()
        kw = dict(zip(("aln_regs", "items", "tasks", "cig_off", "pool"), outs)) if outs else {}
        outs = plan.run(o, ref, n, n, u_off, d_regs, b_off, b.view(-1), read_off, reads.view(-1), **kw)
        tot = plan.check()
        T.append(plan.last_kernel_ms())
    med = lambda j: float(np.median([t[j] for t in T[1:]]))
    areg = outs[0].cpu().numpy().reshape(-1).view(ALN_REG_DTYPE)[:n]
    flags = (b.view(n, na, 2)[:, :, 1] >> 40) & 3
    src = torch.empty(tot[3], dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    torch.cuda.synchronize(); dst.copy_(src); torch.cuda.synchronize()
    t0 = time.perf_counter(); dst.copy_(src); torch.cuda.synchronize(); copy_s = time.perf_counter() - t0
    span_t = int((areg["re0"].astype(np.int64) - areg["rs0"]).sum()); span_q = int((areg["qe0"].astype(np.int64) - areg["qs0"]).sum())
    left_q = int((areg["qs"].astype(np.int64) - areg["qs0"]).sum()); left_t = int((areg["rs"].astype(np.int64) - areg["rs0"]).sum())
    read_bytes = span_q + left_q + (span_t + left_t) // 2
    out = {"regions": n, "anchors_per_region": na, "read_len": qlen, "items": tot[0], "tasks": tot[1], "cigar_words": tot[2], "pool_bytes": tot[3],
           "mean_items": round(tot[0] / n, 2), "mean_cnt1": round(float(areg["cnt1"].mean()), 2), "trimmed_regions": int((areg["cnt1"] != na).sum()),
           "anchors_ignored": int((flags & 2).ne(0).sum()), "long_joins": int((flags & 1).ne(0).sum()), "slots": args.slots,
           "aln_plan_scan_ms": round(med(0), 3), "aln_emit_ms": round(med(1), 3), "aln_gather_ms": round(med(2), 3), "all_ms": [[round(v, 3) for v in t] for t in T],
           "plan_regions_per_s": round(n / med(0) * 1e3), "plan_us_per_region_wave": round(med(0) * 1e3 * min(args.slots, n) / n, 2),
           "gather_gbps": round(tot[3] / med(2) * 1e-6, 1), "gather_rw_gbps": round((tot[3] + read_bytes) / med(2) * 1e-6, 1), "copy_gbps": round(2 * tot[3] / copy_s * 1e-9, 1)}
    print(json.dumps(out))
    plan.close(); ref.close()
    mm2chain.shutdown()


if __name__ == "__main__":
    main()
