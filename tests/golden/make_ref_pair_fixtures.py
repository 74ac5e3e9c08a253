"""Pair-plan fixtures: the reference's own mm_pair with mm_set_pe_thru (pe.o: pe.c:45-63, 76-177, with klib's sorts from misc.o and the host's own logf) on every
case of tests/pair_data.py that the plan does not refuse, and its whole mm_map_frag (map.o) with n_segs = 2 under the -x sr values with MM_F_CIGAR on simulated
2 x 150 pairs from ref_testdata/MT-human.fa and from the small synthetic genome with planted repeats, recorded in front of mm_filter_regs (the input of fin_select) and
in front of and behind mm_pair.  Compiles tests/golden/pair_dump.c against the reference objects and the oracle that build() leaves in oracle/_ref/.
Output: tests/golden/ref_pair.npz (data only): reg_size, names, libm (the C library's version string the fixture was made with: the mapq values are its logf's),
out_off / regs_out (both mates of every planted case behind mm_pair, mate 0 then mate 1, as and p as they came in), kinds (what each case reached, read off the
reference's output); and for the simulated pairs real_qlens, real_rep_len, real_gap (max_gap_ref as mm_pair got it) and the three lists per segment read 2f + s:
real_pre_* (as mm_align_skeleton holds it in front of mm_filter_regs), real_in_* (in front of mm_pair), real_out_* (behind it), each as _off / _regs / _poff / _pext
(p of a region: 0 or 1 + the index among its own list's records), and real_kinds.  The planted inputs are not stored: pair_data.cases() makes them again.
Nothing is written unless the reference alone reached every kind in REQUIRED and REQUIRED_REAL."""
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
DATA = os.path.join(HERE, "ref_testdata")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import pair_data as D  # noqa: E402
import pair_model as M  # noqa: E402
from make_ref_fin_fixtures import ref_dir  # noqa: E402
from make_ref_sketch_fixtures import read_fasta  # noqa: E402

REQUIRED = ("one_end_only", "no_pair_pe_thru", "single_floor2", "floor1", "equal_hi_no_floor", "lift_mate0", "lift_mate1", "old_primary_mapq_zeroed", "sam_pri_moved",
            "under_dp_thres", "pe_bonus_above_sum", "gap_eq_accepted", "gap_plus1_rejected", "break_on_rid", "far_last_hides", "equal_scores_first_wins", "hash_wraps",
            "sub_diff_counted", "sub_diff_not_counted", "alt_lowers", "negative_alt", "blend_raises", "contraction", "pe_thru_off_by_3", "two_primaries", "n64", "n65",
            "ties_gt64_not_stable", "lds_128", "scratch_129", "n300", "n_sub_beyond_table")
REQUIRED_REAL = ("real_one_candidate", "real_several_candidates", "real_one_end_only", "real_both_no_pair")
K, W = 21, 11
ACGT = np.frombuffer(b"ACGT", np.uint8)
bit = lambda r, b: (r["flags"] >> b & 1).astype(int)
mapq = lambda r: (r["flags"] & 0xff).astype(int)


def kinds_of(c, out, by_name):
    """what the case reached, from the reference's output alone; out: [mate 0, mate 1] behind mm_pair"""
    Kd = set()
    rin, n = c["regs"], [o.size for o in out]                                  # (the counts are the reference's: it wrote these arrays)
    name = c["name"]
    changed = any(o.tobytes() != i.tobytes() for o, i in zip(out, rin))
    proper = [np.nonzero(bit(o, M.PROPER_FRAG_BIT))[0] for o in out]
    found = all(p.size == 1 for p in proper)
    assert found or not any(p.size for p in proper)
    thru = [bit(o, M.PE_THRU_BIT).sum() for o in out]
    w = [int(p[0]) for p in proper] if found else None
    if (n[0] == 0) != (n[1] == 0) and not changed:
        Kd.add("one_end_only")
    if min(n) > 0 and not found and thru == [1, 1]:
        Kd.add("no_pair_pe_thru")
    if name == "pe_thru_off_by_3" and thru == [0, 0] and by_name["no_pair_pe_thru"]["thru"] == [1, 1]:
        Kd.add("pe_thru_off_by_3")
    if name == "two_primaries" and thru == [0, 0]:
        Kd.add("two_primaries")
    if found:
        q = [int(mapq(out[s])[w[s]]) for s in range(2)]
        qi = [int(mapq(rin[s])[w[s]]) for s in range(2)]
        if name == "single_floor2" and q == [2, 2] and qi == [0, 0]:
            Kd.add("single_floor2")
        if name == "floor1" and q == [1, 1] and qi == [0, 0]:
            Kd.add("floor1")
        if name == "equal_hi_no_floor" and q == [0, 0]:
            Kd.add("equal_hi_no_floor")
        for s in range(2):
            if rin[s]["parent"][w[s]] != w[s] and (out[s]["parent"] == w[s]).sum() > 1:
                Kd.add(f"lift_mate{s}")
                p = int(rin[s]["parent"][w[s]])
                if mapq(rin[s])[p] > 0 and mapq(out[s])[p] == 0:
                    Kd.add("old_primary_mapq_zeroed")
            if not bit(rin[s], M.SAM_PRI_BIT)[w[s]] and list(np.nonzero(bit(out[s], M.SAM_PRI_BIT))[0]) == [w[s]]:
                Kd.add("sam_pri_moved")
        if name == "under_dp_thres" and q == [2, 2]:
            Kd.add("under_dp_thres")                                           # one candidate: the floor 2 ...
        if name == "pe_bonus_above_sum" and q == [1, 1]:
            Kd.add("pe_bonus_above_sum")                                       # ... and with dp_thres 0 the same regions make two: the floor 1
        if name == "gap_eq" and by_name["gap_plus1"]["found"] is False:        # the same two regions one base further apart are not paired
            Kd.add("gap_eq_accepted")
        if name == "break_on_rid" and w == [1, 0] and q == [2, 2]:
            Kd.add("break_on_rid")
        if name == "equal_scores_j" and w == [1, 0]:
            Kd.add("equal_scores_first_wins")
        if name == "hash_wraps" and w == [1, 0]:
            Kd.add("hash_wraps")
        if name == "sub_diff_eq" and q == [60, 26]:
            Kd.add("sub_diff_counted"); Kd.add("alt_lowers")
        if name == "sub_diff_plus1" and q == [60, 31]:
            Kd.add("sub_diff_not_counted")
        if name == "negative_alt" and q == [1, 1]:
            Kd.add("negative_alt")
        if name == "blend_raises" and q == [60, 48]:
            Kd.add("blend_raises")
        if name == "contraction":
            fused = M.pair_case(c, fp="fused")
            if q == [200, 64] and int(mapq(fused[1])[w[1]]) == 63:
                Kd.add("contraction")
        if name.startswith("alternate_") and w[1] == 0 and w[0] % 2 == 0:      # the winner is of the first group, whose regions have the even indices
            tot = n[0] + n[1]
            stable = max(i for i in range(n[0]) if i % 2 == 0)
            if tot == 64 and w[0] == stable:
                Kd.add("n64")
            if tot > 64 and w[0] != stable:
                Kd.add("ties_gt64_not_stable")
                if tot == 65:
                    Kd.add("n65")
                if tot == D.LDS_CLASS:
                    Kd.add("lds_128")
                if tot == D.LDS_CLASS + 1:
                    Kd.add("scratch_129")
                if tot == 300:
                    Kd.add("n300")
        if name == "n_sub_beyond_table" and q != qi:
            Kd.add("n_sub_beyond_table")                                       # the reference has no table: it goes on where the plan stops
    else:
        if name == "gap_plus1" and min(n) > 0 and by_name["gap_eq"]["found"]:
            Kd.add("gap_plus1_rejected")
        if name == "far_last_hides" and by_name["far_last_alone"]["found"]:     # without the far region the same two regions are paired
            Kd.add("far_last_hides")
    return Kd


def run_planted(dump, cs, fin, fout):
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            o = c["opt"]
            gap = o["max_gap_ref"] if c["gap"] is None else c["gap"]
            f.write(struct.pack("<6i", c["qlens"][0], c["qlens"][1], gap, o["pe_bonus"], o["sub_diff"], o["match_sc"]))
            f.write(struct.pack("<ii", c["regs"][0].size, c["regs"][1].size))
            f.write(c["regs"][0].tobytes()); f.write(c["regs"][1].tobytes())
            f.write(struct.pack("<i", c["pext"].size)); f.write(c["pext"].tobytes())
    subprocess.check_call([dump, "planted", fin, fout])
    raw = open(fout, "rb").read()
    assert struct.unpack_from("<i", raw, 0)[0] == 80
    at, res = 4, []
    for c in cs:
        mates = []
        for s in range(2):
            n, = struct.unpack_from("<i", raw, at)
            assert n == c["regs"][s].size
            out = np.frombuffer(raw, M.REG, n, at + 4).copy()
            idx = np.frombuffer(raw, np.int32, n, at + 4 + 80 * n)
            at += 4 + 84 * n
            assert list(idx) == list(range(n))                                 # mm_pair moves no region
            out["as"] = c["regs"][s]["as"]; out["p"] = c["regs"][s]["p"]
            mates.append(out)
        res.append(mates)
    assert at == len(raw)
    return res


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def mutate(rng, s, rate=0.01):
    a = np.frombuffer(s, np.uint8).copy()
    m = rng.random(a.size) < rate
    a[m] = rng.choice(ACGT, int(m.sum()))
    return a.tobytes()


def make_pairs(rng, mt, syn, rep, a_copies, spacers):
    """2 x 150 pairs, FR: mate 0 forward at p, mate 1 the reverse complement of the insert's end"""
    L = 150
    P = []

    def pair(ref, p, ins, err=0.01):
        return [mutate(rng, ref[p:p + L], err), mutate(rng, revcomp(ref[p + ins - L:p + ins]), err)]
    for _ in range(60):                                                      # unique sequence, inserts of 200 .. 700
        P.append(pair(mt, int(rng.integers(0, len(mt) - 900)), int(rng.integers(200, 700))))
    for _ in range(12):                                                      # the insert beyond max_frag_len: both ends map, no pair
        P.append(pair(mt, int(rng.integers(0, len(mt) - 3000)), int(rng.integers(1200, 2500))))
    for _ in range(8):                                                       # mate 1 on the same strand as mate 0: both ends map, no pair
        f = pair(mt, int(rng.integers(0, len(mt) - 900)), 400)
        P.append([f[0], revcomp(f[1])])
    for _ in range(8):                                                       # the pair turned round (RF)
        f = pair(mt, int(rng.integers(0, len(mt) - 900)), 400)
        P.append([revcomp(f[0]), revcomp(f[1])])
    for _ in range(10):                                                      # one end only: the other is random bases
        f = pair(mt, int(rng.integers(0, len(mt) - 900)), 400)
        k = int(rng.integers(0, 2))
        f[k] = rng.choice(ACGT, L).tobytes()
        P.append(f)
    for c in syn:                                                            # the synthetic genome's own diverged repeat families
        for _ in range(14):
            P.append(pair(c, int(rng.integers(0, len(c) - 900)), int(rng.integers(250, 600))))
    for j in range(20):                                                      # all of it inside a copy of the planted 600-base unit: twenty candidate pairs
        P.append(pair(rep, a_copies[j] + int(rng.integers(0, 150)), int(rng.integers(330, 440)), 0.0 if j % 2 else 0.01))
    for j in range(0, 20, 2):                                                # mate 0 in the unique spacer, mate 1 in the copy behind it: one mate with secondaries
        P.append(pair(rep, spacers[j] + 100, 500, 0.0))
    for j in range(1, 20, 2):                                                # mate 0 in one copy, mate 1 in the next but one: the ends' best hits do not pair
        P.append([rep[a_copies[j] + 20:a_copies[j] + 170], revcomp(rep[a_copies[(j + 2) % 20] + 300:a_copies[(j + 2) % 20] + 450])])
    return P


def parse_real(path, n_frags):
    raw = open(path, "rb").read()
    assert struct.unpack_from("<i", raw, 0)[0] == 80
    at, F = 4, []

    def lst():
        nonlocal at
        n, = struct.unpack_from("<i", raw, at)
        r = np.frombuffer(raw, M.REG, n, at + 4).copy(); at += 4 + 80 * n
        k, = struct.unpack_from("<i", raw, at)
        px = np.frombuffer(raw, M.PEXT, k, at + 4).copy(); at += 4 + 32 * k
        r["as"] = 0                                                            # an offset into the anchors, which the fixture does not hold
        return r, px
    for _ in range(n_frags):
        h = struct.unpack_from("<5i", raw, at); at += 20
        d = dict(qlens=h[:2], rep_len=h[2], gap=h[3])
        d["pre"] = [lst(), lst()]; d["in"] = [lst(), lst()]; d["out"] = [lst(), lst()]
        F.append(d)
    assert at == len(raw)
    return F


def real_kinds_of(d):
    Kd = set()
    (r0, px0), (r1, px1) = d["in"]
    o0, o1 = d["out"][0][0], d["out"][1][0]
    n = [r0.size, r1.size]
    found = bit(o0, M.PROPER_FRAG_BIT).sum() == 1 and bit(o1, M.PROPER_FRAG_BIT).sum() == 1
    # the model on the recorded lists must be the reference, byte for byte: its count of candidates then tells one from several
    px = np.concatenate([px0, px1])
    r1m = r1.copy(); r1m["p"][r1m["p"] != 0] += np.uint64(px0.size)
    opt = dict(D.DEFAULT, max_gap_ref=d["gap"])
    m0, m1, info = M.pair(r0, r1m, px, d["qlens"], opt)
    m1["p"] = r1["p"]
    assert m0.tobytes() == o0.tobytes() and m1.tobytes() == o1.tobytes(), "the model differs from the reference on a simulated pair"
    assert info["found"] == found
    if (n[0] == 0) != (n[1] == 0):
        Kd.add("real_one_end_only")
    if min(n) > 0 and not found:
        Kd.add("real_both_no_pair")
    if found:
        Kd.add("real_one_candidate" if info["n_sc"] == 1 else "real_several_candidates")
        if any(info["lifted"]):
            Kd.add("real_lift")
    if bit(o0, M.PE_THRU_BIT).any():
        Kd.add("real_pe_thru")
    if max(n) > 1:
        Kd.add("real_secondaries")
    return Kd


def main():
    tmp = tempfile.mkdtemp()
    ref = ref_dir()
    dump = os.path.join(tmp, "pair_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("pe", "hit", "misc", "kalloc")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I" + ref, os.path.join(HERE, "pair_dump.c")] + objs + ["-o", dump, "-lm", "-lpthread"])
    cs = [c for c in D.cases() if not c["refuse"]]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    res = run_planted(dump, cs, fin, fout)
    by_name = {c["name"]: dict(thru=[int(bit(o, M.PE_THRU_BIT).sum()) for o in r], found=bool(bit(r[0], M.PROPER_FRAG_BIT).any() and bit(r[1], M.PROPER_FRAG_BIT).any()))
               for c, r in zip(cs, res)}
    kinds = [kinds_of(c, r, by_name) for c, r in zip(cs, res)]
    reached = set().union(*kinds)
    missing = [k for k in REQUIRED if k not in reached]
    assert not missing, f"the reference did not reach: {missing}"

    # the simulated pairs through the reference's whole mm_map_frag
    dump2 = os.path.join(tmp, "pair_dump_real")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("kthread", "kalloc", "misc", "bseq", "sketch", "sdust", "index", "align", "hit", "map", "format", "pe", "esterr",
                                                      "splitidx", "ksw2_ll_sse", "ksw2_extz2_sse", "ksw2_extd2_sse", "ksw2_exts2_sse", "chain_oracle")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-DPAIR_DUMP_REAL", "-I" + ref, "-I" + os.path.join(ROOT, "oracle"), os.path.join(HERE, "pair_dump.c")] + objs +
                          ["-o", dump2, "-Wl,--wrap=mm_pair,--wrap=mm_filter_regs", "-lz", "-lm", "-lpthread"])
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), os.path.join(tmp, "syn"), "--genome-mb", "0.03",
                           "--reads", "1", "--read-len", "1000", "--seed", "3"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(2028)
    rnd = lambda n: rng.choice(ACGT, n).tobytes()
    mt = read_fasta(os.path.join(DATA, "MT-human.fa"))[0]
    syn = read_fasta(os.path.join(tmp, "syn.ref.fa"))
    unit_a = rnd(600)                                                          # the planted repeat: one 600-base unit 20 times, each copy behind 300 unique bases
    rep, a_copies, spacers = b"", [], []
    for j in range(20):
        spacers.append(len(rep)); rep += rnd(300)
        a_copies.append(len(rep)); rep += unit_a
    rep += rnd(300)
    fa = os.path.join(tmp, "ref.fa")
    with open(fa, "wb") as f:
        f.write(b">MT_human\n" + mt + b"\n")
        for i, c in enumerate(syn):
            f.write(b">chr%d\n" % (i + 1) + c + b"\n")
        f.write(b">repeats\n" + rep + b"\n")
    pairs = make_pairs(rng, mt, syn, rep, a_copies, spacers)
    segs = [s for p in pairs for s in p]
    frag_off = np.arange(0, 2 * len(pairs) + 1, 2, dtype=np.int64)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    fpath = os.path.join(tmp, "frags.bin")
    with open(fpath, "wb") as f:
        f.write(struct.pack("<qq", len(pairs), len(segs)) + frag_off.tobytes() + seq_off.tobytes() + b"".join(segs))
    o = os.path.join(tmp, "real.bin")
    subprocess.check_call([dump2, "real", str(K), str(W), fa, fpath, o])
    R = parse_real(o, len(pairs))
    INV, ALT = 1 << 11, 1 << 25
    keep = [d for d in R if not any((l[0]["flags"] & (INV | ALT)).any() for l in d["pre"])]   # fin_select refuses inv / is_alt
    print(f"{len(R)} simulated pairs, {len(R) - len(keep)} left out for an inv region")
    rkinds = [real_kinds_of(d) for d in keep]
    rreached = set().union(*rkinds)
    missing = [k for k in REQUIRED_REAL if k not in rreached]
    assert not missing, f"the reference did not reach on the simulated pairs: {missing}"

    off = lambda v: np.concatenate([[0], np.cumsum([len(x) for x in v])]).astype(np.int64)
    out = dict(reg_size=np.array(80), names=np.array([c["name"] for c in cs]), libm=np.array(" ".join(platform.libc_ver())),
               out_off=off([m for r in res for m in r]), regs_out=np.concatenate([m for r in res for m in r]).view(np.uint8).reshape(-1, 80),
               kinds=np.array([",".join(sorted(k)) for k in kinds]),
               real_qlens=np.array([d["qlens"] for d in keep], np.int32), real_rep_len=np.array([d["rep_len"] for d in keep], np.int32),
               real_gap=np.array([d["gap"] for d in keep], np.int32), real_kinds=np.array([",".join(sorted(k)) for k in rkinds]))
    for tag in ("pre", "in", "out"):
        lists = [l for d in keep for l in d[tag]]
        out[f"real_{tag}_off"] = off([l[0] for l in lists])
        out[f"real_{tag}_regs"] = np.concatenate([l[0] for l in lists]).view(np.uint8).reshape(-1, 80)
        out[f"real_{tag}_poff"] = off([l[1] for l in lists])
        out[f"real_{tag}_pext"] = np.concatenate([l[1] for l in lists]).view(np.uint8).reshape(-1, 32)
    path = os.path.join(HERE, "ref_pair.npz")
    np.savez_compressed(path, **out)
    cnt = {k: sum(k in s for s in rkinds) for k in sorted(rreached)}
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "planted cases, kinds:", len(reached), ";", len(keep), "simulated pairs:", cnt)
    assert os.path.getsize(path) < (1 << 19)


if __name__ == "__main__":
    main()
