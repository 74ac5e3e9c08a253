"""The two ends of a fragment paired on the device: what pair_select (csrc/pair_ends.hip) costs, and for orientation fin_select on the same regions (every mate's list
as one read of the finish plan, its output thrown away).

  python3 tools/pair_bench.py [--frags 65536] [--per-mate 4] [--reps 9] [--seed 1]        (the second shape of profiles/pair_ends.md: --frags 256 --per-mate 150)

A synthetic batch under the -x sr options: every mate has --per-mate final regions with p on one reference and strand, region j of mate 1 100 bases behind region j
of mate 0, 1000 bases from one j to the next: --per-mate candidate pairs with different scores, one walk step each before the break; every tenth region of mate 0
starts where the one before it does (equal keys: above 64 regions the sort replays klib's passes).  PairPlan.run works in place, so every repetition gets a fresh
copy of the regions.  Each entry runs --reps times after one warm-up in the same process; times are the library's own HIP events, medians with the smallest and
largest beside them.  Prints one JSON line."""
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
from mm2chain import params, REG_DTYPE, PEXT_DTYPE  # noqa: E402


def make(frags, per, seed):
    rng = np.random.default_rng(seed)
    n = 2 * frags * per
    j = np.tile(np.arange(per), 2 * frags)
    s = np.tile(np.repeat(np.arange(2), per), frags)
    r = np.zeros(n, REG_DTYPE)
    r["id"] = j
    r["cnt"] = 10
    r["qe"] = 150
    jj = np.where((s == 0) & (j % 10 == 9), j - 1, j)
    r["rs"] = 10000 + 1000 * jj + 250 * s
    r["re"] = r["rs"] + 150
    r["mlen"] = 145; r["blen"] = 150
    r["hash"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    r["flags"] = (np.where(j == 0, 30 | 1 << 12, 0) | s << 16).astype(np.uint32)
    r["p"] = np.arange(n) + 1
    px = np.zeros(n, PEXT_DTYPE)
    px["dp_max"] = px["dp_score"] = rng.integers(200, 300, n)
    r["score"] = r["score0"] = px["dp_max"]
    return r, px


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=65536)
    ap.add_argument("--per-mate", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    mm2chain.init()
    F, per = args.frags, args.per_mate
    r, px = make(F, per, args.seed)
    n = r.size
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    f_off = t(np.arange(2 * F + 1, dtype=np.int64) * per)
    regs0, pext = t(r.view(np.uint8).reshape(-1, 80)), t(px.view(np.uint8).reshape(-1, 32))
    cnt = torch.full((2 * F,), per, dtype=torch.int32, device="cuda")
    qlen = torch.full((2 * F,), 150, dtype=torch.int32, device="cuda")
    rep = torch.zeros(2 * F, dtype=torch.int32, device="cuda")
    pp = mm2chain.PairPlan(F, n, n, max_log_arg=1 << 16)
    fp = mm2chain.FinPlan(2 * F, n, n, max_log_arg=1 << 16, match_sc=2)
    po, fo = params.pair_opts("sr"), params.fin_opts("sr", best_n=1 << 20)
    ms = {"pair_select": [], "fin_select": []}
    proper = hits = 0
    for _ in range(args.reps + 1):
        regs = regs0.clone()
        pp.run(po, f_off, regs, cnt, pext, qlen)
        proper = pp.check()
        ms["pair_select"].append(pp.last_ms())
        fp.run(fo, f_off, regs0, cnt, pext.clone(), qlen, rep)
        hits = fp.check()
        ms["fin_select"].append(fp.last_ms()[1])
    res = {"fragments": F, "regions_per_mate": per, "regions": n, "proper_pairs": int(proper), "fin_select_hits": int(hits),
           "fragments_beyond_lds_class": F if 2 * per > 128 else 0}
    for k, v in ms.items():
        v = v[1:]
        res[k + "_ms"] = round(statistics.median(v), 4); res[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    res["pair_select_us_per_fragment"] = round(1e3 * res["pair_select_ms"] / F, 4)
    res["pair_select_gbps"] = round((80e-6 * n + 4e-6 * n + 16e-6 * n) / res["pair_select_ms"], 1)   # 80 bytes a region and 4 of its record in, two words a region out
    pp.close(); fp.close()
    mm2chain.shutdown()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
