#!/usr/bin/env python3
"""How often an anchor of a synthetic stream takes each path of the hand-written loop of chain_dp_tile (own-tile chunk, older tiles from the
ring, deep f / p, beyond the ring; fold A / B1 / B2; the `break` of chain.c:231), counted by the NumPy model of the kernel's control flow
(tests/tile_model.py, checked against the CPU oracle in tests/test_cpu_oracle.py; by default the loop before the score-bound exit, which the instruction budgets
of profiles/r2_isa_budget.md go by).  Together with tools/isa_budget.py this decomposes the
per-anchor instruction counts of the PMC profiles.   python tools/chunk_stats.py [profile ...] [--reads N] [--anchors M]
--fp-depth: how deep the SCORED ring tiles lie (tiles before the own one): 1-2 = the f / p ring of pairs, 3-4 = what the packed f / p ring adds, > 4 = the deep fetch
either way (profiles/packed_fp.md).  The model counts a scored ring tile beyond NF tiles as deep_fp, so two runs (NF 2 and NF 4) give the three bins.
--score-exit: what the score-bound exit of the loop (chain_dp_tile.h, MM2C_EXIT_TEST) takes away, from the model with the stamps before the fold (late_stamps=False) run with the
exit on and off, NX 16 / NF 4: anchors that leave early, ring tiles no longer visited, how many of those were scored and deep-fetched, and anchors whose f / p differ
between the two runs (must be 0); last, the scored chunks none of whose candidates could beat the best (what a chunk-level score skip would look at), off -> on.
--late-stamps: the fold order in which a chunk stamps only once its fold knows that the scan goes on (chain_dp_tile.h, MM2C_ST_LEAN / MM2C_ST_FAR), from the model
as it stands (its defaults), NX 16 / NF 4: exits of the score-bound test and how many of them leave before any stamp of their chunk (fold B0's),
scored chunks that stamp, scored ring tiles by phase (within the f / p ring, beyond it), anchors that visit a tile beyond the f / p ring, anchors whose ring window
runs out (Lend), folds B0, and anchors whose f / p differ from the model with the stamps before the fold (must be 0)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
from mm2chain import params, synth  # noqa: E402
from tile_model import chain_tile_model  # noqa: E402

BEFORE = dict(score_exit="off", late_stamps=False)    # the loop before the exit and the late stamps: what the default table and --fp-depth have always counted


def avg_qspan(t):
    return float(np.float32(.01 * float(np.float32(int(((t[:, 1] >> np.uint64(32)) & np.uint64(0xff)).sum()))) / t.shape[0]))


if __name__ == "__main__":
    args = sys.argv[1:]
    reads = int(args[args.index("--reads") + 1]) if "--reads" in args else 6
    m = int(args[args.index("--anchors") + 1]) if "--anchors" in args else 5000
    profiles = [a for a in args if not a.startswith("--") and not a.isdigit()] or ["mixed", "dense", "colinear"]
    P = params.map_ont()
    NX = 16 if "--nx16" in args else 8
    span = 19 if "--asm20" in args else 15
    keys = ("no_window", "own_chunks", "own_pass", "ring_chunks", "ring_pass", "deep_fp", "far_chunks", "far_pass", "fold_a", "fold_b0", "fold_b1",
            "fold_b2_closed", "fold_b2_scan", "breaks", "eq_run_anchors")
    if "--tile-skip" in args:
        # round 6: what a per-tile bitmap of diagonal buckets would reject (skip_rejects of skip_tested ring-tile visits; skip_missed: visits without a surviving lane that
        # the bitmap lets through; skip_wrong must be 0)
        keys = ("ring_chunks", "ring_pass", "skip_tested", "skip_rejects", "skip_missed", "skip_wrong")
    if "--score-exit" in args:
        print(f"Per anchor, map-ont parameters, {reads} reads x {m} anchors of each bench.py stream (seed 1, span {span}), NX 16 / NF 4, exit off -> on:\n")
        print("| stream | anchors that exit early | ring tiles no longer visited | ... of them scored | ... of them deep-fetched | wrong exits | futile scored chunks |\n|---|---|---|---|---|---|---|")
        for prof in profiles:
            off, a = synth.make_stream(prof, reads, m, seed=1, q_span=span)
            off = off.numpy(); a = a.numpy().view(np.uint64)
            tot = {mode: dict.fromkeys(("anchors", "exits", "ring_chunks", "ring_pass", "deep_fp", "futile_scores"), 0) for mode in ("off", "auto")}
            wrong = 0
            for k in range(reads):
                t = a[off[k]:off[k + 1]]
                res = {}
                for mode in ("off", "auto"):
                    st = {}
                    res[mode] = chain_tile_model(P, t, avg_qspan(t), stats=st, NX=16, NF=4, compact=True, score_exit=mode, late_stamps=False)
                    for kk in tot[mode]:
                        tot[mode][kk] += st[kk]
                wrong += int(((res["off"][0] != res["auto"][0]) | (res["off"][1] != res["auto"][1])).sum())
            n, o, x = tot["off"]["anchors"], tot["off"], tot["auto"]
            print(f"| {prof} | {x['exits'] / n:.3f} | {(o['ring_chunks'] - x['ring_chunks']) / n:.3f} of {o['ring_chunks'] / n:.3f} | {(o['ring_pass'] - x['ring_pass']) / n:.3f} of {o['ring_pass'] / n:.3f} | "
                  f"{(o['deep_fp'] - x['deep_fp']) / n:.3f} of {o['deep_fp'] / n:.3f} | {wrong} | {o['futile_scores'] / n:.3f} -> {x['futile_scores'] / n:.3f} |")
        sys.exit(0)
    if "--late-stamps" in args:
        print(f"Per anchor, map-ont parameters, {reads} reads x {m} anchors of each bench.py stream (seed 1, span {span}), NX 16 / NF 4:\n")
        print("| stream | exits | ... before any stamp of the chunk | scored chunks (own + ring) | ... that stamp | scored ring tiles within the f / p ring | ... beyond it | "
              "anchors that go beyond it | ring windows that run out | folds B0 | wrong |\n|---|---|---|---|---|---|---|---|---|---|---|")
        for prof in profiles:
            off, a = synth.make_stream(prof, reads, m, seed=1, q_span=span)
            off = off.numpy(); a = a.numpy().view(np.uint64)
            tot = dict.fromkeys(("anchors", "exits", "exits_unstamped", "own_pass", "ring_pass", "stamped_chunks", "cpp_chunks", "near_pass", "deep_pass", "phase_changes", "lend", "fold_b0"), 0)
            wrong = 0
            for k in range(reads):
                t = a[off[k]:off[k + 1]]
                st = {}
                f1, p1 = chain_tile_model(P, t, avg_qspan(t), stats=st, NX=16, NF=4, compact=True)
                f0, p0 = chain_tile_model(P, t, avg_qspan(t), NX=16, NF=4, compact=True, late_stamps=False)
                wrong += int(((f0 != f1) | (p0 != p1)).sum())
                for kk in tot:
                    tot[kk] += st[kk]
            n = tot["anchors"]
            print(f"| {prof} | {tot['exits'] / n:.3f} | {tot['exits_unstamped'] / n:.3f} | {(tot['own_pass'] + tot['ring_pass']) / n:.3f} | {(tot['stamped_chunks'] + tot['cpp_chunks']) / n:.3f} | "
                  f"{tot['near_pass'] / n:.3f} | {tot['deep_pass'] / n:.3f} | {tot['phase_changes'] / n:.3f} | {tot['lend'] / n:.3f} | {tot['fold_b0'] / n:.3f} | {wrong} |")
        sys.exit(0)
    if "--fp-depth" in args:
        print(f"Scored ring tiles per anchor by depth, map-ont parameters, {reads} reads x {m} anchors of each bench.py stream (seed 1, span {span}), NX {NX}:\n")
        print("| stream | scored ring tiles | depth 1-2 | depth 3-4 | depth > 4 |\n|---|---|---|---|---|")
        for prof in profiles:
            off, a = synth.make_stream(prof, reads, m, seed=1, q_span=span)
            off = off.numpy(); a = a.numpy().view(np.uint64)
            n_anchors, ring_pass, deep = 0, 0, {2: 0, 4: 0}
            for k in range(reads):
                t = a[off[k]:off[k + 1]]
                for nf in (2, 4):
                    st = {}
                    chain_tile_model(P, t, avg_qspan(t), stats=st, NX=NX, NF=nf, **BEFORE)
                    deep[nf] += st["deep_fp"]
                n_anchors += st["anchors"]; ring_pass += st["ring_pass"]
            print(f"| {prof} | {ring_pass / n_anchors:.3f} | {(ring_pass - deep[2]) / n_anchors:.3f} | {(deep[2] - deep[4]) / n_anchors:.3f} | {deep[4] / n_anchors:.3f} |")
        sys.exit(0)
    print(f"Per anchor, map-ont parameters, {reads} reads x {m} anchors of each bench.py stream (seed 1, span {span}), NX {NX} / NF 2:\n")
    print("| stream | " + " | ".join(keys) + " |")
    print("|---|" + "---|" * len(keys))
    for prof in profiles:
        off, a = synth.make_stream(prof, reads, m, seed=1, q_span=span)
        off = off.numpy(); a = a.numpy().view(np.uint64)
        tot = dict.fromkeys(("anchors",) + keys, 0)
        for k in range(reads):
            t = a[off[k]:off[k + 1]]
            st = {}
            chain_tile_model(P, t, avg_qspan(t), stats=st, NX=NX, tile_skip="--tile-skip" in args, **BEFORE)
            for kk in tot:
                tot[kk] += st[kk]
        print(f"| {prof} | " + " | ".join(f"{tot[k] / tot['anchors']:.3f}" for k in keys) + " |")
