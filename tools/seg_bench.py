"""Fragment hits per segment on the device: what the multi hit plan (mm_select_sub_multi, csrc/chain_hits.hip) and the seg plan (mm_seg_gen, csrc/chain_segs.hip) cost
beside the plans that stand around them, on pairs of 2 x 150 bases under the -x sr scalars.

  python3 tools/seg_bench.py [--frags 131072] [--reps 7] [--seed 1] [--k 21]

Synthetic pairs: every fragment gets one to four chains of 6 to 24 anchors -- the first across both mates, the others on one mate or across, at another place of the
reference or near the first -- written directly as the compact (u, b) the device epilogue leaves; no DP is run.  Five stages then run --reps times on one stream
after one warm-up: region plan, multi hit plan (per-fragment gap_ref), seg plan, hit plan (pri_ratio 0) and mapq plan (do_join 0, anchors out) over the segment
reads.  Times are the library's own HIP events (the plans' _last_ms / _last_kernel_ms), medians.  scatter_over_gather: seg_scatter's time over mapq_gather's, which
moves the same segment anchors (16 bytes read and 16 written each); scatter_gbps / gather_gbps: those 32 bytes per anchor over the kernel's time.  Prints one JSON
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
from mm2chain import params  # noqa: E402

QLEN, SPAN = 150, 21


def make_pairs(n_frags, seed):
    """-> u_off, u, b_off, b (uint64 [., 2]) of n_frags pairs"""
    rng = np.random.default_rng(seed)
    n_ch = rng.integers(1, 5, n_frags)
    u_off = np.concatenate([[0], np.cumsum(n_ch)]).astype(np.int64)
    n_u = int(u_off[-1])
    frag = np.repeat(np.arange(n_frags), n_ch)
    first = np.arange(n_u) == u_off[frag]
    cnt = rng.integers(6, 25, n_u)
    kind = np.where(first, 0, rng.integers(0, 3, n_u))                         # 0: across both mates, 1: on the first, 2: on the second
    qs = np.where(kind == 2, rng.integers(150, 170, n_u), rng.integers(0, 20, n_u))
    qe = np.where(kind == 1, rng.integers(120, 150, n_u), rng.integers(270, 300, n_u))
    rev = rng.integers(0, 2, n_u)
    near = rng.integers(0, 2, n_u).astype(bool) & ~first
    x_first = rng.integers(100000, 4000000, n_frags)[frag]
    x0 = np.where(first, x_first, np.where(near, x_first + rng.integers(-300, 300, n_u), rng.integers(100000, 4000000, n_u)))
    rev = np.where(near, rev[u_off[frag]], rev)
    score = np.where(first, rng.integers(150, 300, n_u), rng.integers(30, 200, n_u))
    u = (score.astype(np.uint64) << np.uint64(32)) | cnt.astype(np.uint64)
    b_off_chain = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n_b = int(b_off_chain[-1])
    ch = np.repeat(np.arange(n_u), cnt)
    j = np.arange(n_b) - b_off_chain[ch]
    d = np.maximum(cnt[ch] - 1, 1)
    y0 = np.where(rev == 0, qs + SPAN - 1, 2 * QLEN - qe + SPAN - 1)[ch]
    y1 = np.where(rev == 0, qe - 1, 2 * QLEN - qs - 1)[ch]
    y = y0 + (y1 - y0) * j // d
    x = x0[ch] + (y - y0)
    fwd = np.where(rev[ch] == 0, y + 1 - SPAN, 2 * QLEN - 1 - (y + 1 - SPAN))         # the k-mer's first base on its own strand: no segment coordinate below 0
    sid = (fwd >= QLEN).astype(np.uint64)
    b = np.zeros((n_b, 2), np.uint64)
    b[:, 0] = (rev[ch].astype(np.uint64) << np.uint64(63)) | x.astype(np.uint64)
    b[:, 1] = (sid << np.uint64(48)) | (np.uint64(SPAN) << np.uint64(32)) | y.astype(np.uint64)
    b_off = b_off_chain[u_off]
    return u_off, u, b_off, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--k", type=int, default=21)
    args = ap.parse_args()
    mm2chain.init()
    nf = args.frags
    u_off_h, u_h, b_off_h, b_h = make_pairs(nf, args.seed)
    n_u, n_b = int(u_off_h[-1]), int(b_off_h[-1])
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).cuda()
    u_off, u, b_off, b = cu(u_off_h), cu(u_h), cu(b_off_h), cu(b_h)
    qsum = torch.full((nf,), 2 * QLEN, dtype=torch.int32, device="cuda")
    seg_len = torch.full((2 * nf,), QLEN, dtype=torch.int32, device="cuda")
    gap_ref = (500 - (torch.arange(nf, dtype=torch.int32, device="cuda") % 7)).contiguous()              # per fragment, as under -x sr with mates of several lengths
    rep_len = ((torch.arange(nf, dtype=torch.int32, device="cuda") * 131) % 90).contiguous()
    hash_ = torch.from_numpy(np.array([mm2chain.read_hash(b"pair%d" % r, 2 * QLEN) for r in range(min(nf, 1024))], np.uint32).view(np.int32)).cuda()
    hash_ = hash_.repeat((nf + hash_.numel() - 1) // hash_.numel())[:nf].contiguous()
    rp, hp, sp = mm2chain.RegPlan(nf, n_u, n_b), mm2chain.HitPlan(nf, n_u), mm2chain.SegPlan(nf, 2, n_u, n_b)
    hp2, mp = mm2chain.HitPlan(2 * nf, sp.n_su_cap), mm2chain.MapqPlan(2 * nf, sp.n_su_cap, n_b, 1 << 16)
    ho, mo = params.hit_opts(args.k, pri_ratio=0.5, best_n=20), params.hit_multi_opts(2, 500)
    ho0, qo = params.hit_opts(args.k, pri_ratio=0.0), params.mapq_opts(do_join=0, min_cnt=2, min_chain_score=25)
    regs = torch.empty((max(n_u, 1), 80), dtype=torch.uint8, device="cuda")
    hits = torch.empty_like(regs)
    n_hits = torch.empty(nf, dtype=torch.int32, device="cuda")
    seg_hits = torch.empty((max(sp.n_su_cap, 1), 80), dtype=torch.uint8, device="cuda")
    fin = torch.empty_like(seg_hits)
    n_seg_hits = torch.empty(2 * nf, dtype=torch.int32, device="cuda")
    n_fin = torch.empty_like(n_seg_hits)
    b_out = torch.empty((max(n_b, 1), 2), dtype=torch.int64, device="cuda")
    n_b_out = torch.empty(2 * nf, dtype=torch.int64, device="cuda")
    T = {k: [] for k in ("regs", "hits_multi", "seg", "seg_count", "seg_offsets", "seg_scatter", "seg_regs", "seg_mark", "hits_seg", "mapq", "mapq_join", "mapq_gather")}
    out = None
    n_su = n_sb = 0
    for _ in range(args.reps + 1):
        rp.run(u_off, u, b_off, b, qsum, hash_, regs=regs)
        hp.run_multi(ho, mo, u_off, seg_len, regs, gap_ref, regs_out=hits, n_out=n_hits)
        out = sp.run(u_off, hits, n_hits, b_off, b, seg_len, hash_, rep_len, out=out)
        hp2.run(ho0, out["su_off"], out["seg_regs"], regs_out=seg_hits, n_out=n_seg_hits)
        mp.run(qo, out["su_off"], seg_hits, n_seg_hits, out["sb_off"], out["sb"], seg_len, out["seg_rep_len"], regs_out=fin, n_out=n_fin, b_out=b_out, n_b_out=n_b_out)
        rp.check(); hp.check()
        n_su, n_sb = sp.check()
        hp2.check(); mp.check()
        T["regs"].append(rp.last_ms()); T["hits_multi"].append(hp.last_ms()); T["seg"].append(sp.last_ms())
        for key, v in zip(("seg_count", "seg_offsets", "seg_scatter", "seg_regs", "seg_mark"), sp.last_kernel_ms()):
            T[key].append(v)
        T["hits_seg"].append(hp2.last_ms()); T["mapq"].append(mp.last_ms())
        j, g = mp.last_kernel_ms()
        T["mapq_join"].append(j); T["mapq_gather"].append(g)
    med = lambda v: statistics.median(v[1:])
    copied = int(n_b_out.sum())
    res = {"frags": nf, "regions": n_u, "chain_anchors": n_b, "hits": int(n_hits.sum()), "segment_chains": int(n_su), "segment_anchors": int(n_sb),
           "final_regions": int(n_fin.sum()), "anchors_out": copied}
    res.update({k + "_ms": round(med(v), 4) for k, v in T.items()})
    res["scatter_over_gather"] = round(med(T["seg_scatter"]) / med(T["mapq_gather"]), 2) if med(T["mapq_gather"]) > 0 else None
    res["scatter_gbps"] = round(32e-6 * n_sb / med(T["seg_scatter"]), 1) if n_sb else 0.0
    res["gather_gbps"] = round(32e-6 * copied / med(T["mapq_gather"]), 1) if copied else 0.0
    res["count_gbps"] = round(16e-6 * n_sb / med(T["seg_count"]), 1) if n_sb else 0.0
    res.update({k + "_ms_all": [round(x, 4) for x in v[1:]] for k, v in T.items() if k in ("seg_count", "seg_scatter", "mapq_gather", "hits_multi")})
    for p in (mp, hp2, sp, hp, rp):
        p.close()
    mm2chain.shutdown()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
