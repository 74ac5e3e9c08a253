"""Base alignment on the device: what the ksw plan (ksw_extd2_sse as a batch, csrc/ksw_extd2.hip) costs on synthetic gap-fill tasks under the map-ont scores.

  python3 tools/ksw_bench.py [--tasks 65536] [--min-len 300] [--max-len 2000] [--div 0.1] [--w 500] [--slots 1280] [--reps 3] [--seed 1] [--ref-tasks 2048]

Every task is a target of min-len .. max-len random bases and a query made from it with --div divergence (a third each substitutions, insertions, deletions).
Two legs, each --reps times after one warm-up: the first-pass flag of align.c:733 (KSW_EZ_APPROX_MAX) and the exact maximum (flag 0).  Times are the plan's own HIP
events, medians; cells: the cells of the padded rows the kernel walks (what the reference's 16-byte blocks cover), cells_real: those of the real band.
Where oracle/_ref/ksw2_extd2_sse.o and kalloc.o and a C compiler are present, the reference's own function is linked into a temporary program and timed on the
first --ref-tasks tasks on 1 and 16 host threads (ms scaled to the whole batch by cells); its results are compared with the device's on those tasks.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimap2-fpga_amd"))
import mm2chain  # noqa: E402
from mm2chain import params  # noqa: E402

APPROX_MAX = 0x08

WRAP = r'''
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
typedef struct { uint32_t max:31, zdropped:1; int max_q, max_t, mqe, mqe_t, mte, mte_q, score, m_cigar, n_cigar, reach_end; uint32_t *cigar; } ez_t;
void ksw_extd2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t q, int8_t e, int8_t q2, int8_t e2,
                   int w, int zdrop, int end_bonus, int flag, ez_t *ez);
void *km_init(void); void km_destroy(void *km); void kfree(void *km, void *p);
typedef struct { int64_t q_off, t_off; int32_t qlen, tlen, w, zdrop, end_bonus, flag; } task_t;
typedef struct { int tid, nt; int64_t n; const task_t *t; const uint8_t *seq; const int8_t *sc; int32_t *out; } arg_t;
static void *work(void *p)
{
	arg_t *a = (arg_t*)p; void *km = km_init(); int64_t i;
	for (i = a->tid; i < a->n; i += a->nt) {
		const task_t *t = &a->t[i]; ez_t ez; int32_t *o = a->out + i * 11;
		memset(&ez, 0, sizeof(ez));
		ksw_extd2_sse(km, t->qlen, a->seq + t->q_off, t->tlen, a->seq + t->t_off, 5, a->sc, a->sc[25], a->sc[26], a->sc[27], a->sc[28], t->w, t->zdrop, t->end_bonus, t->flag, &ez);
		o[0] = (int32_t)ez.max; o[1] = ez.zdropped; o[2] = ez.max_q; o[3] = ez.max_t; o[4] = ez.mqe; o[5] = ez.mqe_t; o[6] = ez.mte; o[7] = ez.mte_q; o[8] = ez.score;
		o[9] = ez.n_cigar; o[10] = ez.reach_end;
		kfree(km, ez.cigar);
	}
	km_destroy(km);
	return 0;
}
static int run_ref(int nt, int64_t n, const task_t *t, const uint8_t *seq, const int8_t *sc, int32_t *out)
{
	pthread_t th[64]; arg_t a[64]; int k;
	if (nt < 1 || nt > 64) return -1;
	for (k = 0; k < nt; ++k) { a[k].tid = k; a[k].nt = nt; a[k].n = n; a[k].t = t; a[k].seq = seq; a[k].sc = sc; a[k].out = out; pthread_create(&th[k], 0, work, &a[k]); }
	for (k = 0; k < nt; ++k) pthread_join(th[k], 0);
	return 0;
}
/* in: int64 n, seq_len; int8 sc[29]; task_t t[n]; uint8 seq[seq_len] -- out: int32 [n][11]; prints the milliseconds of the calls alone */
int main(int argc, char **argv)
{
	FILE *f; int64_t h[2]; int8_t sc[29]; task_t *t; uint8_t *seq; int32_t *out; struct timespec t0, t1;
	if (argc != 4 || !(f = fopen(argv[1], "rb"))) return 1;
	if (fread(h, 8, 2, f) != 2 || fread(sc, 1, 29, f) != 29) return 2;
	t = (task_t*)malloc(h[0] * sizeof(task_t)); seq = (uint8_t*)malloc(h[1] + 64); out = (int32_t*)calloc(h[0] * 11, 4);
	if (fread(t, sizeof(task_t), h[0], f) != (size_t)h[0] || fread(seq, 1, h[1], f) != (size_t)h[1]) return 3;
	fclose(f);
	clock_gettime(CLOCK_MONOTONIC, &t0);
	if (run_ref(atoi(argv[3]), h[0], t, seq, sc, out)) return 4;
	clock_gettime(CLOCK_MONOTONIC, &t1);
	if (!(f = fopen(argv[2], "wb"))) return 5;
	fwrite(out, 44, h[0], f); fclose(f);
	printf("%.3f\n", (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) / 1e6);
	return 0;
}
'''


def make_tasks(n, lo, hi, div, w, zdrop, seed):
    rng = np.random.default_rng(seed)
    tlen = rng.integers(lo, hi + 1, n)
    t_off = np.concatenate([[0], np.cumsum(tlen)]).astype(np.int64)
    tot = int(t_off[-1])
    tseq = rng.integers(0, 4, tot).astype(np.uint8)
    r = rng.random(tot)
    cnt = np.where(r < div / 3, 0, np.where(r < 2 * div / 3, 2, 1))               # deleted, followed by an inserted base, kept
    cnt[t_off[:-1]] = np.maximum(cnt[t_off[:-1]], 1)                              # no empty query
    sub = (r >= 2 * div / 3) & (r < div)
    base = np.where(sub, (tseq + 1 + rng.integers(0, 3, tot)) % 4, tseq).astype(np.uint8)
    qseq = np.repeat(base, cnt)
    src = np.repeat(np.arange(tot, dtype=np.int32), cnt)
    second = np.concatenate([[False], src[1:] == src[:-1]])                       # the second copy of a base is the inserted one
    qseq[second] = rng.integers(0, 4, int(second.sum())).astype(np.uint8)
    q_end = np.cumsum(cnt)[t_off[1:] - 1]
    q_off = np.concatenate([[0], q_end]).astype(np.int64)
    qlen = np.diff(q_off)
    tk = np.zeros(n, mm2chain.KSW_TASK_DTYPE)
    tk["q_off"], tk["t_off"], tk["qlen"], tk["tlen"], tk["w"], tk["zdrop"], tk["end_bonus"] = q_off[:-1], t_off[:-1] + qseq.size, qlen, tlen, w, zdrop, -1
    seq = np.concatenate([qseq, tseq])
    cig_off = np.concatenate([[0], np.cumsum((qlen + tlen) // 2 + 8)]).astype(np.int64)
    return tk, seq, cig_off


def cells(tk):
    """(padded, real) cells of all rows of all tasks, as the reference's band of :132-147 gives them"""
    pad = real = 0
    for t in tk:
        ql, tl, w = int(t["qlen"]), int(t["tlen"]), int(t["w"])
        r = np.arange(ql + tl - 1)
        st = np.maximum(np.maximum(0, r - ql + 1), (r - w + 1) >> 1)
        en = np.minimum(np.minimum(tl - 1, r), (r + w) >> 1)
        ok = st <= en
        if not ok.all():
            ok[np.argmin(ok):] = False
        real += int((en - st + 1)[ok].sum())
        pad += int(((en + 16) // 16 * 16 - st // 16 * 16)[ok].sum())
    return pad, real


def load_ref():
    """-> run(nt, tasks, seq, score bytes) -> (ms, int32 [n, 11]), or None.  The reference's objects are not position independent (kalloc.o), so they are linked into
    a temporary program, not a shared object; the program times the calls alone, not its own start or the files it reads."""
    objs = [os.path.join(ROOT, "oracle", "_ref", o) for o in ("ksw2_extd2_sse.o", "kalloc.o")]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not all(os.path.exists(o) for o in objs) or cc is None:
        return None
    tmp = tempfile.mkdtemp()
    src, exe = os.path.join(tmp, "wrap.c"), os.path.join(tmp, "kswref")
    open(src, "w").write(WRAP)
    subprocess.check_call([cc, "-O2", "-no-pie", "-w", src] + objs + ["-o", exe, "-lpthread"])

    def run(nt, tasks, seq, scb):
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([tasks.size, seq.size], np.int64).tobytes()); f.write(scb.tobytes()); f.write(tasks.tobytes()); f.write(seq.tobytes())
        ms = float(subprocess.check_output([exe, fin, fout, str(nt)]).decode().strip())
        return ms, np.fromfile(fout, np.int32).reshape(-1, 11)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=65536); ap.add_argument("--min-len", type=int, default=300); ap.add_argument("--max-len", type=int, default=2000)
    ap.add_argument("--div", type=float, default=0.1); ap.add_argument("--w", type=int, default=500); ap.add_argument("--slots", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--seed", type=int, default=1); ap.add_argument("--ref-tasks", type=int, default=2048)
    a = ap.parse_args()
    sc = params.ksw_scores("map-ont")
    tk, seq, co = make_tasks(a.tasks, a.min_len, a.max_len, a.div, a.w, sc["zdrop"], a.seed)
    pad, real = cells(tk)
    mm2chain.init()
    plan = mm2chain.KswPlan(a.tasks, seq.size, int(co[-1]), a.slots * (4 << 20))
    d_seq, d_co = torch.from_numpy(seq).cuda(), torch.from_numpy(co).cuda()
    out = dict(tasks=a.tasks, min_len=a.min_len, max_len=a.max_len, div=a.div, w=a.w, slots=plan.n_slots, slot_bytes=plan.slot_bytes, cells=pad, cells_real=real,
               mean_qlen=float(tk["qlen"].mean()), mean_tlen=float(tk["tlen"].mean()))
    dev = {}
    for leg, flag in (("approx", APPROX_MAX), ("exact", 0)):
        tk["flag"] = flag
        d_tk = torch.from_numpy(tk.view(np.uint8)).cuda()
        res = cig = None
        ms = []
        for rep in range(a.reps + 1):
            res, cig = plan.run(sc, a.tasks, d_tk, d_seq, d_co, res, cig)
            plan.check()
            ms.append(plan.last_kernel_ms()[0])
        m = statistics.median(ms[1:])
        r = res.cpu().numpy().view(mm2chain.KSW_RES_DTYPE).reshape(-1)
        dev[leg] = r
        out[leg] = dict(ksw_rows_ms=m, all_ms=ms, gcells_per_s=pad / m / 1e6, gcells_real_per_s=real / m / 1e6, zdropped=int(r["zdropped"].sum()),
                        mean_n_cigar=float(r["n_cigar"].mean()))
    plan.close()
    ref = load_ref()
    if ref is None:
        out["reference"] = "oracle/_ref/ksw2_extd2_sse.o, kalloc.o or a C compiler is absent: the reference's function was not timed"
    else:
        n = min(a.ref_tasks, a.tasks)
        sub_pad = cells(tk[:n])[0]
        scb = mm2chain.batch._ksw_score_bytes(sc)
        out["reference"] = dict(tasks=n, cells=sub_pad)
        for leg, flag in (("approx", APPROX_MAX), ("exact", 0)):
            tk["flag"] = flag
            sub = np.ascontiguousarray(tk[:n])
            for nt in (1, 16):
                dt, o = ref(nt, sub, seq, scb)
                out["reference"]["%s_%dt" % (leg, nt)] = dict(ms=dt, ms_whole_batch=dt * pad / sub_pad, gcells_per_s=sub_pad / dt / 1e6)
            names = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "n_cigar", "reach_end")
            got = np.stack([dev[leg][f][:n].astype(np.int64) for f in names], 1)
            out["reference"]["%s_equal" % leg] = bool(np.array_equal(got, o.astype(np.int64)))
    mm2chain.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
