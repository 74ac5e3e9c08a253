"""Fixtures of the CIGAR-join plan: the reference's own mm_align1 (static in align.c) on every region of tests/cig_data.ref_batches() (the regions of tests/aln_data.py
and the ones planted on top so that the reference drops, splits and meets every kind of KINDS), with every ksw call recorded WITH its
CIGAR words, the region's CIGAR and dp_score in front of mm_update_extra, and what mm_align1 leaves in r, r->p and r2.  Compiles tests/golden/cig_dump.c the way
make_ref_aln_fixtures.py compiles aln_dump.c (the reference's align.c is included from the reference's directory, nothing of it is copied), a second time with
-fsanitize=address,undefined, and runs every case through both.
Output: tests/golden/ref_cig.npz (outputs only; the inputs are made again by aln_data).  Per option set NAME of aln_data.OPTS:
  NAME_hd int32 [n_regs, 24]: n_calls, r.rs, r.re, r.qs, r.qe, has_p, p.dp_score, p.dp_max, p.blen, p.mlen, p.n_ambi, p.n_cigar, r2.cnt, r2.as, r2.split_inv, r2.rs, r2.re,
  r2.qs, r2.qe, whether :787 was reached, dp_score and n_cigar there, r.split, 0; NAME_call_off int64 [n_regs + 1]; NAME_calls int32 [n, 19] as ref_aln.npz has them, both
  passes; NAME_cw_off int64 [n + 1] and NAME_cw uint32: the calls' CIGAR words; NAME_pre_off / NAME_pre and NAME_fin_off / NAME_fin: each region's CIGAR in front of and
  behind mm_update_extra.  A region the reference split off is run through mm_align1 again, two levels deep: NAME_c1_* and NAME_c2_* hold the same arrays for the
  children and grandchildren, with NAME_c1_parent / NAME_c2_parent the index of the region one level up, and hd[23:30] = level, r2.score, r2.mlen, r2.blen, r2.parent, as1, cnt1.
  kinds_reached: the region kinds of KINDS the reference alone produced.  The generator REFUSES to write unless every kind is reached and at most half of the
  regions dropped."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_aln_fixtures as A  # noqa: E402
import aln_data  # noqa: E402
import cig_data  # noqa: E402

KINDS = ("undropped_both_ext", "no_left", "no_right", "left_reach_end_1", "left_reach_end_0", "right_reach_end_1", "right_reach_end_0", "ext_n_cigar_0", "dropped_split",
         "dropped_no_split", "j_clamp", "drop_first", "drop_last", "code1", "code2_split_inv", "second_differs", "over_left", "over_gap", "over_right", "merge", "no_merge",
         "run65", "sr_test_0", "sr_test_1", "rev_undropped", "rev_dropped", "child")
EXTZ, RIGHT, APPROX_MAX = 0x40, 0x02, 0x08
HD = 30


def build_dump(tmp, sanitize):
    stub = os.path.join(tmp, "stub.c")
    with open(stub, "w") as f:
        f.write("void mm_idxopt_init(void *o) { (void)o; }\n")
    dump = os.path.join(tmp, "cig_dump_san" if sanitize else "cig_dump")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["gcc", "-w", "-DHAVE_KALLOC", "-msse4.1", "-I" + A.REF] + flags + [os.path.join(HERE, "cig_dump.c"), stub] +
                          [os.path.join(A.REF_OBJ, o + ".o") for o in A.OBJS] + ["-o", dump, "-lz", "-lm", "-lpthread"])
    return dump


def run_ref(B):
    tmp = tempfile.mkdtemp()
    fin = os.path.join(tmp, "in.bin")
    A.write_cases(fin, B)
    raws = []
    for sanitize in (False, True):
        fout = os.path.join(tmp, "out%d.bin" % sanitize)
        subprocess.check_call([build_dump(tmp, sanitize), fin, fout], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        raws.append(open(fout, "rb").read())
    assert raws[0] == raws[1], "the sanitized build gives other bytes"
    return raws[0]


def is_second(c, p, sr):
    """c repeats p's lengths and hashes with only APPROX_MAX cleared (:737); under sr the second pass of the ungapped fill is the call with flag 0"""
    if sr:
        return c[5] == 0 and c[4] == -1
    return p is not None and (c[:2] == p[:2]).all() and (c[6:8] == p[6:8]).all() and p[5] & APPROX_MAX and c[5] == p[5] & ~APPROX_MAX


def kinds_of(o, hd, mine, words, a, as_, cnt, qlen, tlen):
    """the kinds one record shows, from the record and the region's anchors alone"""
    sr, sw = bool(o["flag"] & 1), o["max_sw_mat"] > 0
    K = set()
    if cnt <= 0:
        return K
    lo = lambda v: int(v) & 0x7fffffff
    x = [lo(v) for v in a[as_:as_ + cnt, 0]]
    y0, sp = lo(a[as_, 1]), int(a[as_, 1]) >> 32 & 0xff
    rev = int(a[as_, 0]) >> 63
    left_exp = y0 + 1 - sp > 0 and x[0] + 1 - sp > 0
    right_exp = lo(a[as_ + cnt - 1, 1]) + 1 < qlen and x[-1] + 1 < tlen
    second = [k > 0 and bool(is_second(c, mine[k - 1] if not sr else None, sr)) for k, c in enumerate(mine)] if not sr else [bool(is_second(c, None, sr)) for c in mine]
    left = [c for c in mine if c[5] & EXTZ and c[5] & RIGHT]
    right = [c for c in mine if c[5] & EXTZ and not c[5] & RIGHT]
    gfirst = [k for k, c in enumerate(mine) if not c[5] & EXTZ and not second[k]]
    gall = [k for k, c in enumerate(mine) if not c[5] & EXTZ]
    covered = sum(int(mine[k][1]) for k in gfirst)
    reaches = hd[29] > 0 and covered == x[int(hd[28]) + int(hd[29]) - 1 - as_] - x[int(hd[28]) - as_]
    zdrop_drop = bool(gall) and bool(mine[gall[-1]][9])
    over_gap = sw and not sr and not zdrop_drop and not reaches and cnt > 1
    dropped = zdrop_drop or over_gap
    if not mine and not over_gap and not sr:
        return K
    K.add(("rev_dropped" if dropped else "rev_undropped") if rev else "")
    if not dropped and left and right:
        K.add("undropped_both_ext")
    if left:
        K.add("left_reach_end_%d" % int(left[0][18]))
    elif sw and left_exp:
        K.add("over_left")
    else:
        K.add("no_left")
    if not dropped:
        if right:
            K.add("right_reach_end_%d" % int(right[0][18]))
        elif sw and right_exp:
            K.add("over_right")
        else:
            K.add("no_right")
    if any(c[17] == 0 for c in left + right):
        K.add("ext_n_cigar_0")
    if over_gap:
        K.add("over_gap")
    if dropped:
        K.add("dropped_split" if hd[12] > 0 else "dropped_no_split")
        if len(gfirst) == (0 if over_gap else 1):
            K.add("drop_first")
        if zdrop_drop and reaches:
            K.add("drop_last")
        if over_gap and not gfirst and hd[12] > 0 and hd[13] == int(hd[28]) + 1:
            K.add("j_clamp")                                   # max_t = -1: no anchor at or below rs - 1, j is clamped to 0 and r2 begins at the second anchor
    for k in gall:
        if second[k]:
            if sr:
                K.add("sr_test_1")
            else:
                prev = mine[k - 1]
                K.add("code2_split_inv" if mine[k][3] == o["zdrop_inv"] else "code1")
                if (mine[k][8:] != prev[8:]).any() or words[k].tobytes() != words[k - 1].tobytes():
                    K.add("second_differs")
    if sr and not any(second):
        K.add("sr_test_0")
    used = [words[k] for k, c in enumerate(mine) if c[17] > 0 and not (k + 1 < len(mine) and second[k + 1])]
    for p, q in zip(used, used[1:]):
        K.add("merge" if (p[-1] & 0xf) == (q[0] & 0xf) else "no_merge")
    if len(gfirst) >= 65 and all(mine[k][17] == 1 for k in gfirst) and hd[21] <= 3:
        K.add("run65")
    if hd[23] > 0:
        K.add("child")
    K.discard("")
    return K


def main(out_name="ref_cig.npz"):
    B = cig_data.ref_batches()
    _, ref_len, _ = aln_data.reference()
    raw, at = run_ref(B), 0
    out, kinds, n_regs, n_dropped = {}, set(), 0, 0
    for name, (o, reads) in B.items():
        L = [dict(hd=[], calls=[], call_off=[0], cw=[], cw_off=[0], pre=[], pre_off=[0], fin=[], fin_off=[0], parent=[]) for _ in range(3)]
        for r in reads:
            for g in range(r["regs"].size):
                as_, cnt = int(r["regs"][g]["as"]), int(r["regs"][g]["cnt"])
                level = 0
                while True:
                    hd = np.frombuffer(raw, "<i4", HD, at); at += 4 * HD
                    assert hd[23] == level
                    mine, words = [], []
                    for _ in range(int(hd[0])):
                        c = np.frombuffer(raw, "<i4", 19, at); at += 76
                        w = np.frombuffer(raw, "<u4", int(c[17]), at); at += 4 * int(c[17])
                        mine.append(c); words.append(w)
                    p = np.frombuffer(raw, "<u4", int(hd[21]), at); at += 4 * int(hd[21])
                    f = np.frombuffer(raw, "<u4", int(hd[11]), at); at += 4 * int(hd[11])
                    T = L[level]
                    T["parent"].append(len(L[level - 1]["hd"]) - 1 if level else -1)
                    T["hd"].append(hd); T["calls"].extend(mine); T["call_off"].append(T["call_off"][-1] + len(mine))
                    for w in words:
                        T["cw"].append(w); T["cw_off"].append(T["cw_off"][-1] + w.size)
                    T["pre"].append(p); T["pre_off"].append(T["pre_off"][-1] + p.size); T["fin"].append(f); T["fin_off"].append(T["fin_off"][-1] + f.size)
                    rid = int(r["a"][as_, 0]) >> 32 & 0x7fffffff if cnt > 0 else 0
                    K = kinds_of(o, hd, mine, words, r["a"], as_, cnt, r["fwd"].size, int(ref_len[rid]))
                    kinds |= K
                    n_regs += 1; n_dropped += bool(K & {"dropped_split", "dropped_no_split"})
                    if hd[12] <= 0 or level == 2:
                        break
                    as_, cnt, level = int(hd[13]), int(hd[12]), level + 1
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        for level, T in enumerate(L):
            pf = name + ("_c%d" % level if level else "") + "_"
            out[pf + "hd"] = np.array(T["hd"], np.int32).reshape(-1, HD)
            out[pf + "calls"] = np.array(T["calls"], np.int32).reshape(-1, 19); out[pf + "call_off"] = np.array(T["call_off"], np.int64)
            out[pf + "cw"] = cat(T["cw"], np.uint32); out[pf + "cw_off"] = np.array(T["cw_off"], np.int64)
            out[pf + "pre"] = cat(T["pre"], np.uint32); out[pf + "pre_off"] = np.array(T["pre_off"], np.int64)
            out[pf + "fin"] = cat(T["fin"], np.uint32); out[pf + "fin_off"] = np.array(T["fin_off"], np.int64)
            if level:
                out[pf + "parent"] = np.array(T["parent"], np.int32)
    assert at == len(raw)
    missing = sorted(set(KINDS) - kinds)
    print(n_regs, "regions,", n_dropped, "dropped; kinds reached:", sorted(kinds), "; not reached:", missing)
    assert not missing, "the reference did not reach the kind(s) %s: nothing is written" % missing
    assert 2 * n_dropped <= n_regs, "more than half of the regions dropped"
    out["kinds_reached"] = np.array(sorted(kinds))
    out["counts"] = np.array([n_regs, n_dropped], np.int64)
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(*sys.argv[1:2])
