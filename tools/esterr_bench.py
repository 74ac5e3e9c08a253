"""Chain-anchor divergence on the device: what the est-err plan (the counts of mm_est_err, csrc/chain_esterr.hip) costs beside the region, hit and mapq plans that feed it.

  python3 tools/esterr_bench.py [--reads 65536] [--per-read 5000] [--profile mixed] [--reps 5] [--seed 1] [--k 15] [--extra-every 4]

The stream of bench.py (synth.make_stream) is chained on the device as tools/mapq_bench.py does it; region plan, hit plan, mapq plan WITH anchors out (the step a host
must add today to get div at all) and est-err plan then run --reps times on one stream after one warm-up.  The synthetic stream has no reads, so mini_pos is made
from the chain anchors: per read the forward query position (by the anchor's own strand bit, as get_for_qpos) of every chain anchor, plus one unmatched minimizer
behind every --extra-every-th of them, sorted, repeated positions removed; spans are the anchors' own.  Every anchor of every final region is therefore in mini_pos,
as in a real read, and the walk of a region ends where two of its anchors share or lose their order of positions.
Times are the library's own HIP events, medians.  walk_gbps: the 16 bytes of every anchor a final region covers over err_walk's time (its walk predecessor is the
neighbour another lane loads); gather_gbps: 16 bytes read and 16 written per copied anchor over mapq_gather's time, on the same b in the same run.  Prints one JSON
line."""
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


def make_mini_pos(b_off, b, qlen, extra_every):
    """-> (mini_off int64 [n_reads + 1], mini_pos int64) on the device"""
    n_reads, n_b = b_off.numel() - 1, b.shape[0]
    read = torch.repeat_interleave(torch.arange(n_reads, device=b.device), b_off[1:] - b_off[:-1])
    y, span = b[:, 1] & 0xffffffff, (b[:, 1] >> 32) & 0xff
    pos = torch.where(b[:, 0] < 0, qlen - 1 - (y + 1 - span), y)                 # the strand bit is the sign of x
    ok = (pos >= 0) & (pos < (1 << 31) - 2)
    key = (read << 40) | (pos << 8) | span
    key = key[ok]
    key = torch.cat([key, key[::extra_every] + (1 << 8)])                        # an unmatched minimizer one position behind
    del read, y, pos, ok
    key = torch.sort(key).values
    keep = torch.ones_like(key, dtype=torch.bool)
    keep[1:] = (key[1:] >> 8) != (key[:-1] >> 8)                                 # one minimizer per (read, position): the first span
    key = key[keep]
    mini_off = torch.searchsorted(key >> 40, torch.arange(n_reads + 1, device=b.device)).contiguous()
    return mini_off, (((key & 0xff) << 32) | ((key >> 8) & 0xffffffff)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--per-read", type=int, default=5000)
    ap.add_argument("--profile", default="mixed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--extra-every", type=int, default=4)
    args = ap.parse_args()
    mm2chain.init()
    P = params.map_ont()
    off, a = synth.make_stream(args.profile, args.reads, args.per_read, seed=args.seed, device="cuda")
    n_reads, total = off.numel() - 1, a.shape[0]
    f = torch.empty(total, dtype=torch.int32, device="cuda")
    p = torch.empty_like(f)
    plan = mm2chain.ChainPlan(P, off.numpy())
    plan.run(a, f, p)
    u_off, u, b_off, b = plan.chains(a, f, p, 3, 40)
    torch.cuda.synchronize()
    n_u, n_b = int(u_off[-1]), int(b_off[-1])
    q = max(4 * args.per_read, int((b[:n_b, 1] & 0xffffffff).max()) + 256 if n_b else 0)   # every anchor lies inside the read, on either strand
    qlen = torch.full((n_reads,), q, dtype=torch.int32, device="cuda")
    rep_len = (torch.arange(n_reads, dtype=torch.int32, device="cuda") * 131) % 900
    hash_ = torch.from_numpy(np.array([mm2chain.read_hash(b"read%d" % r, q) for r in range(min(n_reads, 1024))], np.uint32).view(np.int32)).cuda()
    hash_ = hash_.repeat((n_reads + hash_.numel() - 1) // hash_.numel())[:n_reads].contiguous()
    mini_off, mini_pos = make_mini_pos(b_off, b[:n_b], q, args.extra_every)
    n_m = int(mini_off[-1])
    rp = mm2chain.RegPlan(n_reads, n_u, n_b)
    hp = mm2chain.HitPlan(n_reads, n_u)
    mp = mm2chain.MapqPlan(n_reads, n_u, n_b)
    ep = mm2chain.EstErrPlan(n_reads, n_u, n_b, n_m)
    regs = torch.empty((max(n_u, 1), 80), dtype=torch.uint8, device="cuda")
    hits, fin = torch.empty_like(regs), torch.empty_like(regs)
    n_hits = torch.empty(max(n_reads, 1), dtype=torch.int32, device="cuda")
    n_out = torch.empty_like(n_hits)
    b_out = torch.empty((max(n_b, 1), 2), dtype=torch.int64, device="cuda")
    n_b_out = torch.empty(max(n_reads, 1), dtype=torch.int64, device="cuda")
    err = torch.empty((max(n_u, 1), 2), dtype=torch.int32, device="cuda")
    avg_k = torch.empty(max(n_reads, 1), dtype=torch.float32, device="cuda")
    ho, mo = params.hit_opts(args.k), params.mapq_opts()
    # the reference sequences: as many as the regions name, all longer than any position
    rp.run(u_off, u, b_off, b, qlen, hash_, regs=regs)
    torch.cuda.synchronize()
    n_ref = int(regs.view(torch.int32)[:n_u, 2].max()) + 1 if n_u else 1
    ref_len = torch.full((n_ref,), (1 << 31) - 1, dtype=torch.int32, device="cuda")
    T = {k: [] for k in ("regs", "hits", "mapq", "join", "gather", "err", "reads", "walk", "finish")}
    for _ in range(args.reps + 1):
        rp.run(u_off, u, b_off, b, qlen, hash_, regs=regs)
        hp.run(ho, u_off, regs, regs_out=hits, n_out=n_hits)
        mp.run(mo, u_off, hits, n_hits, b_off, b, qlen, rep_len, regs_out=fin, n_out=n_out, b_out=b_out, n_b_out=n_b_out)
        ep.run(u_off, fin, n_out, b_off, b_out, mini_off, mini_pos, qlen, ref_len, err=err, avg_k=avg_k)
        rp.check(); hp.check()
        rc, _, _ = mp.counts()
        if rc not in (0, -3):
            mp.check()
        ep.check()
        T["regs"].append(rp.last_ms()); T["hits"].append(hp.last_ms()); T["mapq"].append(mp.last_ms())
        j, g = mp.last_kernel_ms()
        T["join"].append(j); T["gather"].append(g); T["err"].append(ep.last_ms())
        r_, w_, f_ = ep.last_kernel_ms()
        T["reads"].append(r_); T["walk"].append(w_); T["finish"].append(f_)
    med = lambda v: statistics.median(v[1:])
    # what the plan found, over the valid rows
    row_read = torch.repeat_interleave(torch.arange(n_reads, device="cuda"), u_off[1:] - u_off[:-1])
    valid = (torch.arange(n_u, device="cuda") - u_off[row_read]) < n_out[:n_reads][row_read]
    cnt = fin.view(torch.int32)[:n_u, 1][valid].to(torch.int64)
    e = err[:n_u][valid].to(torch.int64)
    covered, copied = int(cnt.sum()), int(n_b_out[:n_reads].sum())
    out = {"profile": args.profile, "reads": n_reads, "anchors": total, "chain_anchors": n_b, "final_regions": int(valid.sum()), "anchors_in_regions": covered,
           "anchors_out": copied, "mini_pos": n_m, "n_ref": n_ref, "regions_div_minus_one": int((e[:, 0] == 0).sum()), "regions_all_matched": int((e[:, 0] == cnt).sum()),
           "n_match_sum": int(e[:, 0].clamp(min=0).sum()), "n_tot_sum": int(e[:, 1].sum()), "avg_k_mean": round(float(avg_k[:n_reads].mean()), 4),
           "regs_ms": round(med(T["regs"]), 3), "hits_ms": round(med(T["hits"]), 3), "mapq_ms_with_anchors": round(med(T["mapq"]), 3),
           "mapq_join_ms": round(med(T["join"]), 3), "mapq_gather_ms": round(med(T["gather"]), 3), "esterr_ms": round(med(T["err"]), 3),
           "err_reads_ms": round(med(T["reads"]), 3), "err_walk_ms": round(med(T["walk"]), 3), "err_finish_ms": round(med(T["finish"]), 3),
           "walk_gbps": round(16e-6 * covered / med(T["walk"]), 1) if covered else 0.0, "gather_gbps": round(32e-6 * copied / med(T["gather"]), 1) if copied else 0.0,
           "walk_over_gather": round(med(T["walk"]) / med(T["gather"]), 2) if copied else 0.0,
           "download_bytes_plan": 8 * int(valid.sum()) + 4 * n_reads, "download_bytes_host_walk": 16 * copied + 8 * n_m,
           "esterr_ms_all": [round(v, 3) for v in T["err"][1:]], "err_walk_ms_all": [round(v, 3) for v in T["walk"][1:]],
           "err_reads_ms_all": [round(v, 3) for v in T["reads"][1:]], "mapq_gather_ms_all": [round(v, 3) for v in T["gather"][1:]]}
    ep.close(); mp.close(); hp.close(); rp.close(); plan.close()
    mm2chain.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
