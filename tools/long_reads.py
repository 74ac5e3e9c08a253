#!/usr/bin/env python3
"""Long reads (BASELINE config 5's regime, SURVEY 8 a1: n = 1e5 .. 1e6 anchors per task, chain_hardware.h:62-64 admits 5 187 500): the chaining DP and the
seed-hit path on batches that have FEWER tasks than the GPU has wave slots, at the anchor density of the bench's ava-ont stream (20 000 anchors in a
400 kb locus = 50 per kb: locus = 20 x anchors per read; -x ava-ont scalars, options.c:83-86).

usage: python tools/long_reads.py [--sizes 2048x100000,1024x300000,256x1000000] [--routes auto,one-wave,coop16,coop8] [--no-seed] [--skip] [--distinct N] [--profile mixed]
Every route's f / p of the first distinct reads are compared with the CPU oracle; one line per (size, route).  bench.py imports measure() for its `long_reads` leg.
--skip adds the seed-hit path under skip_seed as -x ava-ont runs it (measure_skip): the hits spread over 64 references as long as the reads, read r named as reference
r % 64, flag NO_DIAG | NO_DUAL -- once with the long reads expanded on sixteen waves (MM2C_MW_SORT=1) and once on one (=0), every distinct read against the oracle."""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np   # noqa: E402
import torch         # noqa: E402
import mm2chain      # noqa: E402
from mm2chain import params, synth   # noqa: E402
import oracle_binding as ob          # noqa: E402

ROUTES = {   # tuning knobs of a route (the library's defaults are route 'auto': chosen per run, on the device when long tasks are cut first)
    "auto": {"coop_plans": 2},
    "one-wave": {"coop_plans": 0},
    "coop": {"coop_plans": 1, "coop_max_tasks": 1 << 30},                             # several waves per piece always; sixteen or eight by the number of pieces
    "coop16": {"coop_plans": 1, "coop_max_tasks": 1 << 30, "coop_w8_above": 1 << 30},
    "coop8": {"coop_plans": 1, "coop_max_tasks": 1 << 30, "coop_w8_above": 0},
}
QLEN = 1 << 26


def set_route(name):
    mm2chain.tune("coop_max_tasks", 1024); mm2chain.tune("coop_w8_above", 256)
    for k, v in ROUTES[name].items():
        mm2chain.tune(k, v)


def measure(reads, per, routes=("auto",), dp=True, seed=True, reps=3, check=2, profile="mixed", distinct=0, say=None):
    """one size: `reads` reads of `per` anchors (a few distinct ones, replicated into separate memory).  Returns a dict: per route the DP kernel + prepass ms, anchors/s,
    what ran and whether f / p of the first `check` reads equal the oracle; the seed-hit path's ms, anchors/s and whether its anchors equal the oracle's."""
    say = say or (lambda *a: None)
    P = params.ava_ont()
    distinct = distinct or max(2, min(reads, 3_200_000 // per))
    times = max(1, reads // distinct)
    off1, a1 = synth.make_stream(profile, distinct, per, seed=11, device="cuda", locus=20 * per)
    off, a = synth.replicate(off1, a1, times)
    total = int(off[-1]); n_tasks = off.numel() - 1
    a1_h = a1.cpu().numpy().view(np.uint64); off1_h = off1.numpy()
    n_chk = min(check, distinct)
    end = int(off1_h[n_chk])
    out = {"reads": n_tasks, "anchors_per_read": per, "anchors": total, "distinct_reads": distinct, "verified_reads": n_chk}
    t0 = time.perf_counter()
    f_ref, p_ref, _ = ob.chain_batch(P, off1_h[: n_chk + 1], a1_h[:end], min(8, os.cpu_count() or 1))
    t_cpu = time.perf_counter() - t0
    say(f"== {n_tasks} reads x {per} anchors = {total} anchors ({distinct} distinct); oracle on {n_chk} reads: {end / t_cpu / 1e6:.2f} M anchors/s on {min(8, n_chk)} thread(s)")
    if dp:
        d_f = torch.empty(total, dtype=torch.int32, device="cuda"); d_p = torch.empty_like(d_f)
        out["dp"] = {}
        for route in routes:
            set_route(route)
            plan = mm2chain.ChainPlan(P, off.numpy())
            ms = []
            for _ in range(reps):
                d_f.fill_(-7); d_p.fill_(-7)
                plan.run(a, d_f, d_p)
                torch.cuda.synchronize()
                ms.append((plan.last_kernel_ms(), plan.last_prepass_ms()))
            k_ms, pre_ms = min(ms, key=sum)                                    # the best run as a whole (a cold first run has a slow prepass)
            ok = bool(np.array_equal(d_f[:end].cpu().numpy(), f_ref) and np.array_equal(d_p[:end].cpu().numpy(), p_ref))
            ok = ok and bool(torch.equal(d_f[total - int(off1[-1]):], d_f[: int(off1[-1])])) and bool(torch.equal(d_p[total - int(off1[-1]):], d_p[: int(off1[-1])]))
            pieces, one_wave, coop = plan.last_route()
            out["dp"][route] = {"kernel_ms": round(k_ms, 3), "prepass_ms": round(pre_ms, 3), "value": total / ((k_ms + pre_ms) * 1e-3), "unit": "anchors/s",
                                "pieces": pieces, "pieces_one_wave_each": one_wave, "pieces_several_waves_each": coop, "identical_to_oracle": ok}
            say(f"DP {route:9s}: kernel {k_ms:9.2f} ms + prepass {pre_ms:6.2f} ms = {total / ((k_ms + pre_ms) * 1e-3) / 1e9:6.3f} G anchors/s  "
                f"(all runs {[round(m[0], 2) for m in ms]})  identical to the oracle: {ok}  pieces {pieces}: {one_wave} x 1 wave, {coop} x 16 waves")
            plan.close()
        set_route("auto")
        del d_f, d_p
    if seed:
        ms_, hs_, mo_, ao_, mt_, ht_, mo_t, ao_t = _seed_batch(a1_h, off1_h, distinct, times)
        sp = mm2chain.SeedPlan(mo_t, ao_t)
        d_m = torch.from_numpy(mt_.view(np.uint8)).cuda(); d_h = torch.from_numpy(ht_.view(np.int64)).cuda()
        d_q = torch.full((n_tasks,), QLEN, dtype=torch.int32, device="cuda")
        d_as = sp.run(d_m, d_h, d_q)
        sms = []
        for _ in range(reps):
            d_as = sp.run(d_m, d_h, d_q, d_as)
            torch.cuda.synchronize()
            sms.append(sp.last_ms())
        n_ties = sp.check()
        got = d_as[: int(ao_[n_chk])].cpu().numpy().view(np.uint64)
        ok_s = True
        for k in range(n_chk):
            mk = ms_[k].copy(); mk["cr_off"] -= ao_[k]
            ok_s = ok_s and np.array_equal(got[ao_[k]:ao_[k + 1]], ob.collect_seed_hits(mk, hs_[k], QLEN))
        s_ms = min(sms)
        out["seed_hits"] = {"ms": round(s_ms, 3), "value": int(ao_t[-1]) / (s_ms * 1e-3), "unit": "anchors/s", "reads_with_equal_x": int(n_ties), "identical_to_oracle": bool(ok_s)}
        say(f"seed hits -> sorted anchors: {s_ms:9.2f} ms = {int(ao_t[-1]) / (s_ms * 1e-3) / 1e9:6.3f} G anchors/s  (all runs {[round(m, 2) for m in sms]})  "
            f"reads with equal x: {n_ties} of {n_tasks}; identical to the oracle: {bool(ok_s)}")
        sp.close(); del d_m, d_h, d_as, d_q
    del a, a1
    torch.cuda.empty_cache()
    return out


def _seed_batch(a1_h, off1_h, distinct, times, n_refs=0):
    """matches -> sorted anchors: matches derived from the reads (one match per query position, hits = the anchors at that position), the distinct reads replicated
    `times` times; n_refs > 0: the hits' reference ids spread over that many references.  Returns the per-read matches / hits of the distinct reads with their
    offsets, and the replicated batch (matches, hits, match offsets, hit offsets)"""
    rng = np.random.default_rng(64)
    ms_, hs_, mo_, ao_ = [], [], [0], [0]
    for k in range(distinct):
        m_k, h_k = synth.matches_from_anchors(a1_h[off1_h[k]:off1_h[k + 1]], QLEN)
        if n_refs:
            h_k = (h_k & np.uint64(0xffffffff)) | (rng.integers(0, n_refs, h_k.size).astype(np.uint64) << np.uint64(32))
        m_k["cr_off"] += ao_[-1]
        ms_.append(m_k); hs_.append(h_k); mo_.append(mo_[-1] + m_k.size); ao_.append(ao_[-1] + h_k.size)
    m1_, h1_ = np.concatenate(ms_), np.concatenate(hs_)
    mt_ = np.tile(m1_, times); mt_["cr_off"] += np.repeat(np.arange(times, dtype=np.int64) * h1_.size, m1_.size)
    mo_t = np.concatenate([[0], np.tile(np.diff(mo_), times).cumsum()]).astype(np.int64)
    ao_t = np.concatenate([[0], np.tile(np.diff(ao_), times).cumsum()]).astype(np.int64)
    return ms_, hs_, mo_, ao_, mt_, np.tile(h1_, times), mo_t, ao_t


N_REFS = 64


def measure_skip(reads, per, reps=3, profile="mixed", distinct=0, say=None):
    """the seed-hit path of one size under skip_seed as -x ava-ont runs it (NO_DIAG | NO_DUAL): hits over N_REFS references of the reads' length, read r named as
    reference r % N_REFS (so about half of every read's hits name a reference below it and are dropped, and the diagonal goes).  Long reads on sixteen waves
    (MM2C_MW_SORT=1) and on one (=0): ms, hits/s, how many reads took the sixteen-wave expansion, the share of hits kept and whether every distinct read's anchors
    equal the oracle's collect_seed_hits with the same flags."""
    say = say or (lambda *a: None)
    distinct = distinct or max(2, min(reads, 3_200_000 // per))
    times = max(1, reads // distinct)
    off1, a1 = synth.make_stream(profile, distinct, per, seed=11, device="cuda", locus=20 * per)   # the reads of measure()'s seed leg
    a1_h = a1.cpu().numpy().view(np.uint64); off1_h = off1.numpy()
    del a1
    ms_, hs_, mo_, ao_, mt_, ht_, mo_t, ao_t = _seed_batch(a1_h, off1_h, distinct, times, n_refs=N_REFS)
    n_reads = mo_t.size - 1
    flag = ob.F_NO_DIAG | ob.F_NO_DUAL
    ref_rank = np.arange(N_REFS, dtype=np.int32); ref_len = np.full(N_REFS, QLEN, np.int32)
    q_lo = (np.arange(n_reads) % N_REFS).astype(np.int32); q_eq = np.ones(n_reads, np.int32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_m = torch.from_numpy(mt_.view(np.uint8)).cuda(); d_h = torch.from_numpy(ht_.view(np.int64)).cuda()
    d_q = torch.full((n_reads,), QLEN, dtype=torch.int32, device="cuda")
    d_rr, d_rl, d_lo, d_eq = dev(ref_rank), dev(ref_len), dev(q_lo), dev(q_eq)
    hits = int(ao_t[-1])
    out = {"reads": n_reads, "hits_per_read": per, "hits": hits, "distinct_reads": distinct, "flag": flag, "refs": N_REFS}
    say(f"== skip_seed (NO_DIAG | NO_DUAL): {n_reads} reads x {per} hits = {hits} hits ({distinct} distinct), {N_REFS} references")
    old = os.environ.get("MM2C_MW_SORT")
    try:
        for mw in ("1", "0"):
            os.environ["MM2C_MW_SORT"] = mw                                     # read when a seed plan is made
            sp = mm2chain.SeedPlan(mo_t, ao_t)
            d_as, d_off = sp.run_skip(d_m, d_h, d_q, flag, d_rr, d_rl, d_lo, d_eq)
            sms = []
            for _ in range(reps):
                d_as, d_off = sp.run_skip(d_m, d_h, d_q, flag, d_rr, d_rl, d_lo, d_eq, anchors=d_as)
                torch.cuda.synchronize()
                sms.append(sp.last_ms())
            sp.check()
            n_mw = sp.last_expand_mw()
            off_h = d_off.cpu().numpy()
            got = d_as[: int(off_h[distinct])].cpu().numpy().view(np.uint64)
            ok = True
            for k in range(distinct):
                mk = ms_[k].copy(); mk["cr_off"] -= ao_[k]
                ref = ob.collect_seed_hits(mk, hs_[k], QLEN, flag, ref_rank, ref_len, int(q_lo[k]), int(q_eq[k]))
                ok = ok and np.array_equal(got[off_h[k]:off_h[k + 1]], ref)
            s_ms = min(sms)
            kept = int(off_h[-1])
            out[f"mw_sort={mw}"] = {"ms": round(s_ms, 3), "value": hits / (s_ms * 1e-3), "unit": "hits/s", "reads_expanded_on_16_waves": n_mw,
                                    "kept_share": round(kept / hits, 4), "identical_to_oracle": bool(ok)}
            say(f"seed hits with skip_seed, MM2C_MW_SORT={mw}: {s_ms:9.2f} ms = {hits / (s_ms * 1e-3) / 1e9:6.3f} G hits/s  (all runs {[round(m, 2) for m in sms]})  "
                f"reads on 16 waves {n_mw}; kept {kept} of {hits} hits ({kept / hits:.3f}); identical to the oracle ({distinct} distinct reads): {bool(ok)}")
            sp.close(); del d_as, d_off
    finally:
        if old is None:
            os.environ.pop("MM2C_MW_SORT", None)
        else:
            os.environ["MM2C_MW_SORT"] = old
    del d_m, d_h
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x100000,1024x300000,256x1000000")
    ap.add_argument("--routes", default="auto,one-wave,coop16,coop8")
    ap.add_argument("--profile", default="mixed")
    ap.add_argument("--distinct", type=int, default=0, help="distinct reads generated per size (0: about 3.2e6 anchors' worth, at least 2)")
    ap.add_argument("--no-seed", action="store_true")
    ap.add_argument("--no-dp", action="store_true")
    ap.add_argument("--skip", action="store_true", help="also the seed-hit path under skip_seed (NO_DIAG | NO_DUAL), long reads on sixteen waves and on one")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=2, help="reads per size compared with the oracle")
    args = ap.parse_args()
    mm2chain.init()
    P = params.ava_ont()
    print(f"# long reads: ava-ont scalars (max_dist {P.max_dist_x}, bw {P.bw}, max_iter {P.max_iter}, max_skip {P.max_skip}), profile {args.profile}, locus = 20 x anchors per read")
    for spec in args.sizes.split(","):
        reads, per = (int(v) for v in spec.split("x"))
        measure(reads, per, routes=args.routes.split(","), dp=not args.no_dp, seed=not args.no_seed, reps=args.reps, check=args.check, profile=args.profile,
                distinct=args.distinct, say=lambda *a: print(*a, flush=True))
        if args.skip:
            measure_skip(reads, per, reps=args.reps, profile=args.profile, distinct=args.distinct, say=lambda *a: print(*a, flush=True))
    mm2chain.shutdown()


if __name__ == "__main__":
    main()
