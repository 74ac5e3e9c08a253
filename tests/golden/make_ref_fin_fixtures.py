"""Finish-plan fixtures: the reference's own mm_filter_regs -> mm_hit_sort -> mm_set_parent -> mm_select_sub -> mm_set_sam_pri -> mm_set_mapq (hit.o: hit.c:125-293,
463-506, with klib's sorts from misc.o and the host's own logf) on every case of tests/fin_data.py that the plan does not refuse, each under its own options, and its
mm_split_reg on fin_data.split_cases().  Compiles tests/golden/fin_dump.c against the reference objects build() leaves in oracle/_ref/.
Output: tests/golden/ref_fin.npz (data only): reg_size, names, libm (the C library's version string the fixture was made with: the mapq values are its logf's),
flt_off / flt_idx (input indices behind mm_filter_regs), srt_off / srt_idx (behind mm_hit_sort), out_off / hits_out (the arrays behind mm_set_mapq, as and p as they
came in), out_idx (the input index of every survivor), out_dp_max2, kinds (what each case reached, read off the reference's output), split_names / split_r / split_r2;
and real_names / real_out_off / real_hits_out / real_out_idx / real_out_dp_max2 / real_kinds: the same outputs for fin_data.real_cases(), the reads of ont, asm20 and sr as
mm_align_skeleton holds them behind its loop, rebuilt from the reference's own record of mm_align1 (ref_cig.npz), with the kinds of REQUIRED_REAL.
The inputs are not stored: fin_data.cases() makes them again.  Nothing is written unless the reference alone reached every kind in REQUIRED."""
import os
import platform
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_OBJ = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fin_data as D  # noqa: E402
import fin_model as M  # noqa: E402

REQUIRED = ("empty", "one", "all_filtered", "filter_some", "seg_split_exempt", "one_end_clipped", "clip_float_keeps", "sort_reorders", "tie_le64_later_first", "n64", "n65",
            "gt64_no_ties", "ties_gt64_not_stable", "lds_128", "scratch_129", "n300", "no_p_kept", "dp_max2_set", "dp_max2_of_three", "identical_no_dp_max2",
            "later_sees_update", "sub_diff_counts", "sub_diff_plus1_does_not", "select_dropped", "p_follows_survivors", "best_n_0", "pri_ratio_0", "all_chains", "sam_pri_rewritten_without_drop",
            "mapq_p_dp2", "mapq_p_no_dp2", "mapq_no_p", "alt_lower", "alt_higher", "floor_504", "cap_60", "n_sub_penalty", "beyond_table_input")
OPT_FMT = "<iiiffiiifiiiii"


def key_of(c, i):
    r, px = c["regs"], c["pext"]
    sc = int(px["dp_max"][int(r["p"][i]) - 1]) if r["p"][i] else int(r["score"][i])
    return ((sc & 0xffffffff) << 32) | int(r["hash"][i])


def kinds_of(c, flt, srt, out, idx, dp2, by_name):
    """what the case reached, from the reference's output alone"""
    K = set()
    r, o, n = c["regs"], c["opt"], c["regs"].size
    mapq = (out["flags"] & 0xff).astype(int)
    pri = out["parent"] == out["id"]
    if n == 0:
        K.add("empty")
    if n == 1 and out.size == 1:
        K.add("one")
    if n > 0 and len(flt) == 0:
        K.add("all_filtered")
    if 0 < len(flt) < n:
        K.add("filter_some")
    if any((int(r["flags"][i]) >> M.SEG_SPLIT_BIT & 1) and r["cnt"][i] < o["min_cnt"] for i in flt):
        K.add("seg_split_exempt")
    q = c["qlen"]
    lim = float(M.F(o["max_clip_ratio"])) * q
    if any(r["p"][i] and (r["qs"][i] > lim) != (q - r["qe"][i] > lim) for i in flt):
        K.add("one_end_clipped")
    if c["name"] == "clip_float" and 0 in flt:
        qs, qe = int(r["qs"][0]), int(r["qe"][0])
        in_float = bool(M.F(qs) > M.F(q) * M.F(o["max_clip_ratio"])) and bool(M.F(q - qe) > M.F(q) * M.F(o["max_clip_ratio"]))
        in_double = qs > lim and q - qe > lim
        assert in_double and not in_float, "the clip case does not tell float from double"
        K.add("clip_float_keeps")
    if len(srt) > 1 and list(srt) != [i for i in flt if i in set(srt)]:
        K.add("sort_reorders")
    keys = [key_of(c, i) for i in srt]
    ties = len(set(keys)) != len(keys)
    stable = [i for _, _, i in sorted(((key_of(c, i), t, i) for t, i in enumerate(i for i in flt if r["cnt"][i] > 0)), key=lambda e: (e[0], e[1]))][::-1]
    if 1 < len(srt) <= 64 and ties:
        assert list(srt) == stable
        t = [p for p, i in enumerate(srt) if keys.count(keys[p]) > 1]
        if srt[t[0]] > srt[t[1]]:
            K.add("tie_le64_later_first")
    if len(srt) == 64:
        K.add("n64")
    if len(srt) == 65:
        K.add("n65")
    if len(srt) > 64 and not ties:
        assert list(srt) == stable
        K.add("gt64_no_ties")
    if len(srt) > 64 and ties and list(srt) != stable:
        K.add("ties_gt64_not_stable")
    if n == D.LDS_CLASS:
        K.add("lds_128")
    if n == D.LDS_CLASS + 1:
        K.add("scratch_129")
    if n == 300:
        K.add("n300")
    if out.size and not r["p"][idx].any():
        K.add("no_p_kept")
    dp2_in = np.array([int(c["pext"]["dp_max2"][int(r["p"][i]) - 1]) if r["p"][i] else 0 for i in idx], int)
    if (dp2 > dp2_in).any():
        K.add("dp_max2_set")
    if c["name"] == "dp_max2_of_three" and dp2[0] == 250 and out["n_sub"][0] == 0:
        K.add("dp_max2_of_three")
    if c["name"] == "identical_after_dp" and dp2[0] == 0 and out["n_sub"][0] == 0 and by_name["identical_but_rs"] == (296, 1):
        K.add("identical_no_dp_max2")
    if c["name"] == "later_sees_update" and (int(out["n_sub"][0]), int(out["subsc"][0]), int(dp2[0])) == (2, 90, 250):
        K.add("later_sees_update")
    if c["name"] == "sub_diff_eq" and out["n_sub"][0] == 1:
        K.add("sub_diff_counts")
    if c["name"] == "sub_diff_plus1" and out["n_sub"][0] == 0 and dp2[0] == 291:
        K.add("sub_diff_plus1_does_not")
    if not o["all_chains"] and out.size < len(srt):
        K.add("select_dropped")
        if any(r["p"][i] and t < len(srt) and srt[t] != i for t, i in enumerate(idx)):
            K.add("p_follows_survivors")
    if o["best_n"] == 0 and out.size < len(srt):
        K.add("best_n_0")
    if o["pri_ratio"] <= 0 and out.size == len(srt) and (~pri).any():
        K.add("pri_ratio_0")
    if o["all_chains"] and out.size and (out["id"] == r["id"][idx]).all() and (out["id"] != np.arange(out.size)).any():
        K.add("all_chains")
    sp_in, sp_out = (r["flags"][idx] >> 12 & 1).astype(int), (out["flags"] >> 12 & 1).astype(int)
    if not o["all_chains"] and out.size == len(srt) > 1 and list(sp_in) != list(sp_out) and list(sp_out) == [1] + [0] * (out.size - 1):
        K.add("sam_pri_rewritten_without_drop")
    for t in np.nonzero(pri)[0]:
        K.add("mapq_no_p" if not r["p"][idx[t]] else "mapq_p_dp2" if dp2[t] > 0 else "mapq_p_no_dp2")
    if c["name"] == "floor_504" and mapq[0] == 1:
        K.add("floor_504")
    if c["name"] == "cap_60" and mapq[0] == 60:
        K.add("cap_60")
    if c["name"] == "n_sub_penalty" and mapq[0] == by_name["n_sub_none"][1] - 6 > 0:
        K.add("n_sub_penalty")
    if c["name"] == "alt_below_sr0" and mapq[0] < by_name.get("alt_below_sr1", (0, 0))[1]:
        K.add("alt_lower")
    if c["name"] == "alt_above_sr0" and mapq[0] == by_name.get("alt_above_sr1", (0, -1))[1] and mapq[0] > 0:
        K.add("alt_higher")
    if c["name"] == "beyond_table" and out.size and max(int(c["pext"]["dp_max"][int(r["p"][i]) - 1]) for i in idx) == D.MAX_LOG_ARG + 1:
        K.add("beyond_table_input")
    return K


def ref_dir():
    """where the reference's headers are: $REF, else the REF of oracle/ref_host/Makefile, which built the objects"""
    if os.environ.get("REF"):
        return os.environ["REF"]
    for line in open(os.path.join(ROOT, "oracle", "ref_host", "Makefile")):
        if line.startswith("REF ?="):
            return line.split("=", 1)[1].strip()
    raise SystemExit("set REF to the reference's source directory")


def run_dump(dump, cs, fin, fout):
    """fin_dump over the cases -> per case (flt, srt, out, idx, dp_max2)"""
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            o = c["opt"]
            f.write(struct.pack("<ii", c["qlen"], c["rep_len"]))
            f.write(struct.pack(OPT_FMT, *[o[k] for k in M.OPT_FIELDS]))
            f.write(struct.pack("<i", c["regs"].size)); f.write(c["regs"].tobytes())
            f.write(struct.pack("<i", c["pext"].size)); f.write(c["pext"].tobytes())
    subprocess.check_call([dump, "regs", fin, fout])
    raw = open(fout, "rb").read()
    size, = struct.unpack_from("<i", raw, 0)
    assert size == 80
    at = 4

    def ints():
        nonlocal at
        n, = struct.unpack_from("<i", raw, at)
        v = np.frombuffer(raw, np.int32, n, at + 4).copy()
        at += 4 + 4 * n
        return v

    res = []
    for c in cs:
        flt, srt = ints(), ints()
        n, = struct.unpack_from("<i", raw, at)
        out = np.frombuffer(raw, M.REG, n, at + 4).copy()
        at += 4 + 80 * n
        idx = ints()
        dp2 = np.frombuffer(raw, np.int32, n, at).copy()
        at += 4 * n
        out["as"] = c["regs"]["as"][idx]; out["p"] = c["regs"]["p"][idx]
        res.append((flt, srt, out, idx, dp2))
    assert at == len(raw)
    return res


# (the reference finds no secondary in any read of that record, so that branch of mm_set_parent -- dp_max2, a drop by mm_select_sub -- is reached by the planted
# cases only; the three kinds below that name it are recorded where met and not required)
REQUIRED_REAL = ("real_child_kept", "real_grandchild_kept", "real_filtered", "real_sort_reorders", "real_all_gone")


def real_kinds_of(c, flt, srt, out, idx, dp2):
    """what a read rebuilt from the alignment record reached, from the reference's output alone"""
    K = set()
    lv = [c["where"][i][0] for i in idx]
    if 1 in lv:
        K.add("real_child_kept")
    if 2 in lv:
        K.add("real_grandchild_kept")
    if len(flt) < c["regs"].size:
        K.add("real_filtered")
    if out.size < len(srt):
        K.add("real_select_dropped")
    if len(srt) > 1 and list(srt) != sorted(srt):
        K.add("real_sort_reorders")
    if (dp2 > 0).any():
        K.add("real_dp_max2_set")
    if c["regs"].size and out.size == 0:
        K.add("real_all_gone")
    if (out["parent"] != out["id"]).any():
        K.add("real_secondary_kept")
    return K


def main():
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "fin_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("hit", "misc", "kalloc")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I" + ref_dir(), os.path.join(HERE, "fin_dump.c")] + objs + ["-o", dump, "-lm", "-lpthread"])
    cs = [c for c in D.cases() if not c["refuse"]]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    res = run_dump(dump, cs, fin, fout)
    size = 80
    by_name = {c["name"]: (int(r[4][0]) if r[4].size else 0, int(r[2]["flags"][0] & 0xff) if r[2].size else 0) for c, r in zip(cs, res)}   # (dp_max2, mapq) of the first hit
    by_name["identical_but_rs"] = (by_name["identical_but_rs"][0], int(res[[c["name"] for c in cs].index("identical_but_rs")][2]["n_sub"][0]))
    kinds = [kinds_of(c, *r, by_name) for c, r in zip(cs, res)]
    reached = set().union(*kinds)
    missing = [k for k in REQUIRED if k not in reached]
    assert not missing, f"the reference did not reach: {missing}"
    # the reads rebuilt from the reference's record of mm_align1 (ref_cig.npz), ont / asm20 / sr
    rc = D.real_cases()
    rres = run_dump(dump, rc, fin, fout)
    rkinds = [real_kinds_of(c, *r) for c, r in zip(rc, rres)]
    rreached = set().union(*rkinds)
    missing = [k for k in REQUIRED_REAL if k not in rreached]
    assert not missing, f"the reference did not reach on the rebuilt reads: {missing}"
    # mm_split_reg
    ss = D.split_cases()
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(ss)))
        for s in ss:
            f.write(s["reg"].tobytes()); f.write(struct.pack("<iii", s["n"], s["qlen"], s["a"].shape[0])); f.write(s["a"].tobytes())
    subprocess.check_call([dump, "split", fin, fout])
    sp = np.frombuffer(open(fout, "rb").read(), M.REG).reshape(len(ss), 2)
    fd = [s for s in ss if s["name"] == "float_double"][0]
    assert M.split_score(int(fd["reg"]["score"]), int(fd["reg"]["cnt"]) - fd["n"], int(fd["reg"]["cnt"])) != M.split_score(int(fd["reg"]["score"]), int(fd["reg"]["cnt"]) - fd["n"], int(fd["reg"]["cnt"]), "float")
    off = lambda v: np.concatenate([[0], np.cumsum([len(x) for x in v])]).astype(np.int64)
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
    path = os.path.join(HERE, "ref_fin.npz")
    np.savez_compressed(path, reg_size=np.array(size), names=np.array([c["name"] for c in cs]), libm=np.array(" ".join(platform.libc_ver())),
                        flt_off=off([r[0] for r in res]), flt_idx=cat([r[0] for r in res], np.int32), srt_off=off([r[1] for r in res]), srt_idx=cat([r[1] for r in res], np.int32),
                        out_off=off([r[2] for r in res]), hits_out=np.concatenate([r[2] for r in res]).view(np.uint8).reshape(-1, 80), out_idx=cat([r[3] for r in res], np.int32),
                        out_dp_max2=cat([r[4] for r in res], np.int32), kinds=np.array([",".join(sorted(k)) for k in kinds]),
                        real_names=np.array([c["name"] for c in rc]), real_out_off=off([r[2] for r in rres]),
                        real_hits_out=np.concatenate([r[2] for r in rres]).view(np.uint8).reshape(-1, 80), real_out_idx=cat([r[3] for r in rres], np.int32),
                        real_out_dp_max2=cat([r[4] for r in rres], np.int32), real_kinds=np.array([",".join(sorted(k)) for k in rkinds]),
                        split_names=np.array([s["name"] for s in ss]), split_r=sp[:, 0].copy().view(np.uint8).reshape(-1, 80), split_r2=sp[:, 1].copy().view(np.uint8).reshape(-1, 80))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "cases,", sum(len(r[2]) for r in res), "hits out,", len(ss), "splits; kinds:", len(reached), ";", len(rc), "rebuilt reads,", sum(len(r[2]) for r in rres), "hits, kinds:", sorted(rreached))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
