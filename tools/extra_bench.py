"""An aligned region finished on the device: what the two kernels of the extra plan (csrc/align_extra.hip: extra_update = mm_update_extra, extra_zdrop = mm_test_zdrop)
cost on ONT-like regions under the map-ont scores.

  python3 tools/extra_bench.py [--regs 98304] [--len 10000] [--distinct 64] [--slots 2048] [--reps 3] [--seed 1]

--distinct regions are made by the seeded edit script of tests/extra_data.py (about --len alignment columns, an indel every 8 to 12 bases, most of them at the right
end of a repeat so that left alignment moves them) and laid out --regs / --distinct times in device memory, each copy with sequences, CIGAR and output slot of its
own, so that the kernels read as many bytes as --regs different regions would.  Three legs, each --reps times after one warm-up: extra_update without and with
is_eqx, and extra_zdrop on the same CIGARs laid out as a ksw plan leaves them.  Times are the plan's own HIP events, medians.
Each time is set against the bytes the kernel must read and write (sequences once, CIGAR words in and out, tasks and results) and the rate of a device-to-device copy
measured in the same process: `memory_ms` is the time in which the memory alone would finish, `times_memory` how far the kernel is from it.
The results of the first copies of every distinct region are compared with tests/extra_model.py.  The reference's functions are static in align.c; they can be timed
only where its source lies beside the objects of oracle/_ref/, which this tool does not assume: the CPU side is not timed, and the output says so.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mm2chain  # noqa: E402
from mm2chain import params  # noqa: E402
import extra_data  # noqa: E402
import extra_model  # noqa: E402


def copy_rate():
    """bytes per millisecond a device-to-device copy moves (read plus written)"""
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"); b = torch.empty_like(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(4):
        ev[0].record(); b.copy_(a); ev[1].record(); torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return 2 * a.numel() / statistics.median(ms[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regs", type=int, default=98304); ap.add_argument("--len", type=int, default=10000); ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--slots", type=int, default=2048); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    regs = [extra_data.edit_region(rng, a.len) for _ in range(a.distinct)]
    copies = max(1, a.regs // a.distinct)
    n = copies * a.distinct
    sc = params.ksw_scores("map-ont")
    score = (np.array(sc["mat"], np.int8), sc["q"], sc["e"], sc["q2"], sc["e2"])
    expect = [[extra_model.update_extra(q, t, c, score[0], score[1], score[2], x) for x in (0, 1)] for q, t, c in regs]
    # one block of the distinct regions, then `copies` of it
    seq = np.concatenate([np.concatenate([q, t]) for q, t, _ in regs]).astype(np.uint8)
    cig = np.concatenate([c for _, _, c in regs]).astype(np.uint32)
    qlen = np.array([q.size for q, _, _ in regs]); tlen = np.array([t.size for _, t, _ in regs]); nc = np.array([c.size for _, _, c in regs])
    room = np.array([e[1]["n_cigar"] + 2 for e in expect])                       # a slot for the EQX result
    s_off = np.concatenate([[0], np.cumsum(qlen + tlen)]); c_off = np.concatenate([[0], np.cumsum(nc)]); r_off = np.concatenate([[0], np.cumsum(room)])
    rep = np.arange(copies)[:, None]
    tk = np.zeros(n, mm2chain.EXTRA_TASK_DTYPE)
    tk["q_off"] = (rep * s_off[-1] + s_off[:-1][None, :]).reshape(-1); tk["t_off"] = tk["q_off"] + np.tile(qlen, copies)
    tk["qlen"], tk["tlen"], tk["n_cigar"] = np.tile(qlen, copies), np.tile(tlen, copies), np.tile(nc, copies)
    in_off = (rep * c_off[-1] + c_off[:-1][None, :]).reshape(-1).astype(np.int64)
    out_off = np.concatenate([(rep * r_off[-1] + r_off[:-1][None, :]).reshape(-1), [copies * r_off[-1]]]).astype(np.int64)
    ktk = np.zeros(n, mm2chain.KSW_TASK_DTYPE)
    ktk["q_off"], ktk["t_off"], ktk["qlen"], ktk["tlen"], ktk["w"], ktk["zdrop"], ktk["end_bonus"] = tk["q_off"], tk["t_off"], tk["qlen"], tk["tlen"], 500, 400, -1
    kres = np.zeros(n, mm2chain.KSW_RES_DTYPE); kres["n_cigar"] = tk["n_cigar"]
    kco = np.concatenate([in_off, [copies * c_off[-1]]]).astype(np.int64)

    mm2chain.init()
    rate = copy_rate()
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8) if x.dtype.fields is not None else np.ascontiguousarray(x)).cuda()
    d_seq = d(seq).repeat(copies); d_cig = d(cig.view(np.int32)).repeat(copies)
    slot_words = int(nc.max()) if int(nc.max()) > mm2chain.EXTRA_LDS_WORDS else 0
    plan = mm2chain.ExtraPlan(n, d_seq.numel(), d_cig.numel(), int(out_off[-1]), n_slots=a.slots, slot_words=slot_words)
    d_tk, d_io, d_oo, d_ktk, d_kres, d_kco = d(tk), d(in_off), d(out_off), d(ktk), d(kres), d(kco)
    bases = int((qlen + tlen).sum()) * copies
    out = dict(regs=n, distinct=a.distinct, copies=copies, mean_qlen=float(qlen.mean()), mean_tlen=float(tlen.mean()), mean_n_cigar=float(nc.mean()), bases=bases, slots=a.slots,
               cigars_in_lds=int((nc <= mm2chain.EXTRA_LDS_WORDS).sum()), slot_words=slot_words, copy_gb_per_s=rate / 1e6)
    res = co = zres = None
    for leg, x in (("update", 0), ("update_eqx", 1)):
        ms = []
        for _ in range(a.reps + 1):
            res, co = plan.update(score, x, n, d_tk, d_seq, d_io, d_cig, d_oo, res, co)
            plan.check()
            ms.append(plan.last_kernel_ms()[0])
        m = statistics.median(ms[1:])
        r = res.cpu().numpy().view(mm2chain.EXTRA_RES_DTYPE).reshape(-1)
        words = co.cpu().numpy().view(np.uint32)
        ok = True
        for k in (list(range(a.distinct)) + list(range(n - a.distinct, n))):
            e = expect[k % a.distinct][x]
            ok = ok and all(int(r[f][k]) == e[f] for f in ("n_cigar", "qshift", "tshift", "blen", "mlen", "n_ambi", "dp_max")) and np.array_equal(words[out_off[k]:out_off[k] + e["n_cigar"]], e["cigar"])
        byts = bases + 4 * int(nc.sum()) * copies + 4 * int(r["n_cigar"].sum()) + n * (32 + 32 + 16)
        out[leg] = dict(extra_update_ms=m, all_ms=ms, gbases_per_s=bases / m / 1e6, bytes=byts, memory_ms=byts / rate, times_memory=m * rate / byts, equal_to_model=bool(ok),
                        mean_n_cigar_out=float(r["n_cigar"].mean()))
    ms = []
    for _ in range(a.reps + 1):
        zres = plan.zdrop(score, params.zdrop_opts("map-ont"), n, d_ktk, d_seq, d_kco, d_kres, d_cig, zres)
        plan.check()
        ms.append(plan.last_kernel_ms()[1])
    m = statistics.median(ms[1:])
    z = zres.cpu().numpy().view(mm2chain.ZDROP_RES_DTYPE).reshape(-1)
    ok = True
    for k in range(a.distinct):
        q, t, c = regs[k]
        e = extra_model.test_zdrop(q, t, c, score[0], score[1], score[2], 400, 200, 5000, False)
        ok = ok and all(int(z[f][k]) == e[f] and int(z[f][n - a.distinct + k]) == e[f] for f in e)
    byts = bases + 4 * int(nc.sum()) * copies + n * (40 + 48 + 8 + 32)
    out["zdrop"] = dict(extra_zdrop_ms=m, all_ms=ms, gbases_per_s=bases / m / 1e6, bytes=byts, memory_ms=byts / rate, times_memory=m * rate / byts, equal_to_model=bool(ok),
                        code_1=int(z["code"].sum()), inv_cand=int(z["inv_cand"].sum()))
    out["reference"] = "mm_update_extra and mm_test_zdrop are static in the reference's align.c, whose source this tool does not assume: the CPU side was not timed"
    plan.close()
    mm2chain.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
