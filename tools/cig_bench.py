#!/usr/bin/env python3
"""Device time of the CIGAR-join plan on the ONT-like regions of tools/aln_bench.py: by default 98 304 regions of about 11.6 kb, one region a read.  The
alignment-task plan makes items, tasks and the pool; the ksw results are synthesised so that the DP need not run to time this: an extension gets min(qlen, tlen) M
and does not reach the end, a gap fill gets m/2 M, the length difference as one I or D word, and the rest of the M, so every region passes the length check of
align.c:284, nothing drops and there is no second pass.  Times are the plan's HIP events, the median of --reps runs after a warm-up with the smallest and the
largest beside it.  gather_rw_gbps: the words cig_gather reads plus the words it writes, four bytes each, per second; copy_gbps: a device-to-device copy of the
words it reads, read plus written, between events in the same process.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=98304)
    ap.add_argument("--anchors", type=int, default=289)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import mm2chain
    from mm2chain import params, RefSeq, AlnPlan, CigPlan, REG_DTYPE, KSW_TASK_DTYPE, KSW_RES_DTYPE, ZDROP_RES_DTYPE, CIG_REG_DTYPE
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
    y = torch.cummax((p[None, :] + 200 + d).clamp(min=k - 1), 1).values.clamp(max=qlen - 1)
    x = start[:, None] + 200 + p[None, :]
    b = torch.stack([x, (k << 32) | y], 2).contiguous()
    yh, xh = y.cpu().numpy(), x.cpu().numpy()
    regs = np.zeros(n, REG_DTYPE)
    regs["cnt"], regs["as"], regs["mlen"] = na, 0, na * k
    regs["rs"], regs["re"], regs["qs"], regs["qe"] = xh[:, 0] + 1 - k, xh[:, -1] + 1, yh[:, 0] + 1 - k, yh[:, -1] + 1
    off = lambda per: torch.arange(n + 1, device=dev, dtype=torch.int64) * per
    u_off, b_off, read_off = off(1), off(na), off(qlen)
    d_regs = torch.from_numpy(regs.view(np.uint8).reshape(n, -1)).to(dev)
    o = params.aln_opts("map-ont")
    caps = dict(items=n * (na // 4 + 8), tasks=n * (na // 4 + 8), pool=n * (2 * qlen + 2 * 12000 + 64))
    plan = AlnPlan(n, caps["items"], caps["tasks"], caps["pool"], n * na, n * qlen)
    aregs, items, tasks, cig_off, pool = plan.run(o, ref, n, n, u_off, d_regs, b_off, b.view(-1), read_off, reads.view(-1))
    n_items, n_tasks, n_slots_words, _ = plan.check()
    # the synthetic ksw results, made on the host once
    tk = tasks.cpu().numpy().reshape(-1).view(KSW_TASK_DTYPE)[:n_tasks]
    co = cig_off.cpu().numpy()[:n_tasks + 1]
    ql, tl = tk["qlen"].astype(np.int64), tk["tlen"].astype(np.int64)
    ext = (tk["flag"] & 0x40) != 0
    m = np.minimum(ql, tl)
    m1 = np.where(ext, m, m // 2)
    dlt = np.where(ext, 0, ql - tl)
    m2 = np.where(ext, 0, m - m1)
    W = np.stack([m1 << 4, (np.abs(dlt) << 4) | np.where(dlt > 0, 1, 2), m2 << 4], 1).astype(np.uint32)
    ok = np.stack([m1 > 0, dlt != 0, m2 > 0], 1)
    n_cig = ok.sum(1)
    assert (n_cig <= np.diff(co)).all()
    cigar = np.zeros(max(int(co[-1]), 1), np.uint32)
    cigar[(co[:-1, None] + np.cumsum(ok, 1) - 1)[ok]] = W[ok]
    res = np.zeros(n_tasks, KSW_RES_DTYPE)
    res["max"], res["score"], res["n_cigar"] = m, m, n_cig
    res["max_q"] = res["max_t"] = res["mqe_t"] = m - 1
    d_res = torch.from_numpy(res.view(np.uint8).reshape(n_tasks, -1)).to(dev)
    d_cigar = torch.from_numpy(cigar.view(np.int32)).to(dev)
    d_zres = torch.zeros((max(n_tasks, 1), ZDROP_RES_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    words_in = int(n_cig.sum())
    cp = CigPlan(n, n_items, n_tasks, int(co[-1]), 16, 16, caps["pool"], n * na, words_in, n)
    score = params.ksw_scores("map-ont")
    copt = dict(zdrop=o["zdrop"], zdrop_inv=o["zdrop_inv"], bw_ext=o["bw_ext"], min_cnt=o["min_cnt"], flag=0, cig_shift=0)
    res2 = torch.zeros((16, KSW_RES_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    cigar2 = torch.zeros(16, dtype=torch.int32, device=dev)
    outs2, outs, T = None, None, []
    for rep in range(args.reps + 1):
        kw = dict(zip(("tasks2", "cig_off2", "second_of"), outs2)) if outs2 else {}
        outs2 = cp.second(copt, score, n, aregs, items, tasks, d_zres, pool, **kw)
        n2, _ = cp.second_check()
        kw = dict(zip(("cig_regs", "cig_out", "in_off", "extra_tasks", "extra_reg"), outs)) if outs else {}
        outs = cp.join(copt, n, n, u_off, d_regs, b_off, b.view(-1), read_off, aregs, items, cig_off, d_res, d_cigar, d_zres, outs2[2], outs2[1], res2, cigar2, **kw)
        words_out, n_extra = cp.check()
        T.append(cp.last_kernel_ms())
    assert n2 == 0 and n_extra == n
    cr = outs[0].cpu().numpy().reshape(-1).view(CIG_REG_DTYPE)[:n]
    src = torch.empty(words_in, dtype=torch.int32, device=dev); dst = torch.empty_like(src)
    copies = []
    for rep in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1))
    med = lambda j: float(np.median([t[j] for t in T[1:]]))
    rng = lambda j: [round(min(t[j] for t in T[1:]), 3), round(max(t[j] for t in T[1:]), 3)]
    names = ("cig_second_count_scan", "cig_second_emit", "cig_cut", "cig_scan", "cig_gather")
    out = {"regions": n, "items": n_items, "tasks": n_tasks, "mean_items": round(n_items / n, 2), "words_in": words_in, "words_out": words_out, "merges": words_in - words_out,
           "mean_words_out": round(words_out / n, 2), "reps": args.reps}
    for j, nm in enumerate(names):
        out[nm + "_ms"] = round(med(j), 3); out[nm + "_min_max_ms"] = rng(j)
    out["cut_regions_per_s"] = round(n / med(2) * 1e3)
    out["gather_rw_gbps"] = round(4 * (words_in + words_out) / med(4) * 1e-6, 1)
    out["copy_gbps"] = round(8 * words_in / float(np.median(copies[1:])) * 1e-6, 1)
    out["copy_ms"] = round(float(np.median(copies[1:])), 4)
    out["mean_n_used"] = round(float(cr["n_used"].mean()), 2)
    print(json.dumps(out))
    cp.close(); plan.close(); ref.close()
    mm2chain.shutdown()


if __name__ == "__main__":
    main()
