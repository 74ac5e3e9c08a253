"""Aligned regions to final hits on the device: what the finish plan's two entries (csrc/align_finish.hip) cost, and for orientation the hit plan and the mapq plan on the
same batch of regions (they ignore p: same reads, same region counts, the chain-level steps).

  python3 tools/fin_bench.py [--reads 65536] [--per-read 8] [--reps 9] [--seed 1]        (the second shape of profiles/finish_regions.md: --reads 256 --per-read 300)

A synthetic batch under map-ont options: every read has --per-read aligned regions with p, in overlapping pairs on the query (one secondary per pair), ten chain anchors
each, one region in eight split behind its fifth anchor.  FinPlan.apply, FinPlan.run, HitPlan.run and MapqPlan.run (do_join = 0: no anchors read) each run --reps times
after one warm-up in the same process; times are the library's own HIP events, medians with the smallest and largest beside them.  Prints one JSON line."""
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
from mm2chain import params, REG_DTYPE, PEXT_DTYPE, CIG_REG_DTYPE, EXTRA_RES_DTYPE  # noqa: E402

ANCHORS = 10


def make(reads, per, seed):
    rng = np.random.default_rng(seed)
    n = reads * per
    j = np.tile(np.arange(per), reads)
    r = np.zeros(n, REG_DTYPE)
    r["id"] = r["parent"] = j
    r["cnt"] = ANCHORS
    r["score"] = r["score0"] = rng.integers(50, 500, n)
    r["qs"] = 1000 * (j // 2); r["qe"] = r["qs"] + 800 + 50 * (j % 2)
    r["rs"] = 100000 * j + r["qs"]; r["re"] = r["rs"] + (r["qe"] - r["qs"])
    r["as"] = ANCHORS * j
    r["mlen"] = 400; r["blen"] = 500
    r["hash"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    r["p"] = np.arange(n) + 1
    px = np.zeros(n, PEXT_DTYPE)
    px["dp_max"] = px["dp_score"] = rng.integers(100, 2000, n)
    i = np.tile(np.arange(ANCHORS, dtype=np.uint64), n)
    b = np.zeros((n * ANCHORS, 2), np.uint64)
    b[:, 0] = np.uint64(1000) + np.uint64(40) * i + np.repeat(np.arange(n, dtype=np.uint64) % np.uint64(7), ANCHORS)
    b[:, 1] = (np.uint64(15) << np.uint64(32)) | (np.uint64(50) + np.uint64(37) * i)
    cig = np.zeros(n, CIG_REG_DTYPE)
    cig["has_p"] = 1; cig["split_n"] = np.where(np.arange(n) % 8 == 3, 5, 0)
    cig["rs1"], cig["re1"], cig["r_qs"], cig["r_qe"], cig["dp_score"] = r["rs"], r["re"], r["qs"], r["qe"], px["dp_score"]
    xe = np.zeros(n, EXTRA_RES_DTYPE)
    xe["n_cigar"], xe["blen"], xe["mlen"], xe["dp_max"] = 7, 500, 400, px["dp_max"]
    off = lambda k: np.arange(reads + 1, dtype=np.int64) * k
    return dict(n=n, regs=r, pext=px, b=b, cig=cig, xe=xe, u_off=off(per), b_off=off(per * ANCHORS), read_off=off(20000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--per-read", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    mm2chain.init()
    D = make(args.reads, args.per_read, args.seed)
    n, reads = D["n"], args.reads
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u_off, regs, b_off, b, read_off = t(D["u_off"]), t(D["regs"].view(np.uint8).reshape(-1, 80)), t(D["b_off"]), t(D["b"].view(np.int64)), t(D["read_off"])
    cig, xr, xe, oo = t(D["cig"].view(np.uint8)), t(np.arange(n, dtype=np.int32)), t(D["xe"].view(np.uint8)), t(np.arange(n + 1, dtype=np.int64) * 8)
    pext0 = t(D["pext"].view(np.uint8).reshape(-1, 32))
    n_in = torch.full((reads,), args.per_read, dtype=torch.int32, device="cuda")
    qlen = torch.full((reads,), 20000, dtype=torch.int32, device="cuda")
    rep = torch.zeros(reads, dtype=torch.int32, device="cuda")
    fp = mm2chain.FinPlan(reads, n, n, max_log_arg=1 << 16)
    hp = mm2chain.HitPlan(reads, n)
    mp = mm2chain.MapqPlan(reads, n, n * ANCHORS, max_log_arg=1 << 16)
    fo, ho, mo = params.fin_opts(), params.hit_opts(15), params.mapq_opts(do_join=0)
    cap = n // 8 + 1
    ms = {"fin_apply": [], "fin_select": [], "hits_select": [], "mapq_join": []}
    out = hits = None
    for _ in range(args.reps + 1):
        A = fp.apply(reads, n, u_off, regs, b_off, b, read_off, cig, n, xr, xe, oo, cap)
        pext = pext0.clone()
        out, n_out = fp.run(fo, u_off, regs, n_in, pext, qlen, rep)
        fp.apply_check(); n_hits = fp.check()
        a_ms, s_ms = fp.last_ms()
        hits, h_out = hp.run(ho, u_off, regs)
        hp.check()
        mp.run(mo, u_off, hits, h_out, b_off, b, qlen, rep)
        mp.check()
        ms["fin_apply"].append(a_ms); ms["fin_select"].append(s_ms); ms["hits_select"].append(hp.last_ms()); ms["mapq_join"].append(mp.last_ms())
    res = {"reads": reads, "regions_per_read": args.per_read, "regions": n, "children": int(A[5].cpu()[0]), "final_hits": int(n_hits),
           "reads_beyond_lds_class": reads if args.per_read > 128 else 0}
    for k, v in ms.items():
        v = v[1:]
        res[k + "_ms"] = round(statistics.median(v), 4); res[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    res["fin_select_us_per_read"] = round(1e3 * res["fin_select_ms"] / reads, 4)
    res["fin_select_gbps"] = round((80e-6 * n + 32e-6 * n + 80e-6 * n_hits) / res["fin_select_ms"], 1)
    for p in (fp, hp, mp):
        p.close()
    mm2chain.shutdown()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
