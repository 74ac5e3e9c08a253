"""Fixtures of the alignment-task plan: the reference's own mm_align1 (static in align.c) on every region of tests/aln_data.py, with every ksw call it makes recorded.
Compiles tests/golden/aln_dump.c, which includes the reference's align.c from the reference's directory (REF, default: `reference` beside the repository; nothing of
it is copied), against the reference objects build() leaves in oracle/_ref/ -- without align.o -- and a one-line stub for mm_idxopt_init.  The dump is built a second
time with -fsanitize=address,undefined and every case runs through both: a case that trips the sanitizer is an input the reference is not defined on, belongs to
the plan's refusals and is an error of this generator if it stays in.
Output: tests/golden/ref_aln.npz (outputs only; the inputs are made again by aln_data).  Per option set NAME of aln_data.OPTS:
  NAME_names; NAME_ends int32 [n_regs, 3]: as1, cnt1 of mm_fix_bad_ends / mm_max_stretch called directly and the region's dp_score (-2^31 where a second pass replaced the ungapped fill's score); NAME_call_off int64 [n_regs + 1]; NAME_calls int32 [n, 19]: per recorded
  call qlen, tlen, w, zdrop, end_bonus, flag, FNV-1a of the query and of the target bytes, and the eleven ez fields -- second passes of :737 (a call that repeats
  its predecessor's lengths and hashes with only APPROX_MAX cleared) are dropped here; NAME_dropped uint8 [n_regs]: the region's last gap call came back zdropped;
  NAME_flags uint8 [n_anchors]: y >> 40 of every anchor afterwards.
  counts int64 [3]: regions, dropped regions, second passes dropped."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_OBJ = os.path.join(ROOT, "oracle", "_ref")
REF = os.environ.get("REF", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aln_data  # noqa: E402

OBJS = ("kalloc", "misc", "index", "hit", "esterr", "pe", "sketch", "sdust", "bseq", "kthread", "ksw2_extz2_sse", "ksw2_extd2_sse", "ksw2_exts2_sse", "ksw2_ll_sse")
APPROX_MAX = 0x08
PLANTED_KINDS = ("sr_", "hp_", "cnt", "gaps", "fbs", "alt", "lj_", "tandem", "self", "rs_zero", "ctg_", "gap", "near_", "two_regions", "res", "sw_at", "lg")


def build_dump(tmp, sanitize):
    stub = os.path.join(tmp, "stub.c")
    with open(stub, "w") as f:
        f.write("void mm_idxopt_init(void *o) { (void)o; }\n")
    dump = os.path.join(tmp, "aln_dump_san" if sanitize else "aln_dump")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["gcc", "-w", "-DHAVE_KALLOC", "-msse4.1", "-I" + REF] + flags + [os.path.join(HERE, "aln_dump.c"), stub] +
                          [os.path.join(REF_OBJ, o + ".o") for o in OBJS] + ["-o", dump, "-lz", "-lm", "-lpthread"])
    return dump


def write_cases(path, B):
    off, ln, S = aln_data.reference()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", ln.size)); f.write(off.astype("<u8").tobytes()); f.write(ln.astype("<u4").tobytes())
        f.write(struct.pack("<i", S.size)); f.write(S.astype("<u4").tobytes())
        f.write(struct.pack("<i", len(B)))
        for name, (o, reads) in B.items():
            f.write(struct.pack("<20i", o["a"], o["b"], o["q"], o["e"], o["q2"], o["e2"], o["bw"], o["min_chain_score"], o["max_gap"], o["min_cnt"], o["min_ksw_len"], o["end_bonus"],
                                o["zdrop"], o["zdrop_inv"], o["max_sw_mat"], (0x10000000 if o["flag"] & 2 else 0) | (0x1000 if o["flag"] & 1 else 0), o["idx_flag"], o["k"], o["sc_ambi"], 0))
            f.write(struct.pack("<i", len(reads)))
            for r in reads:
                f.write(struct.pack("<3i", r["fwd"].size, r["a"].shape[0], r["regs"].size))
                f.write(r["fwd"].tobytes()); f.write(r["a"].astype("<u8").tobytes()); f.write(r["regs"].tobytes())


def run_ref(B):
    tmp = tempfile.mkdtemp()
    fin = os.path.join(tmp, "in.bin")
    write_cases(fin, B)
    raws = []
    for sanitize in (False, True):
        fout = os.path.join(tmp, "out%d.bin" % sanitize)
        subprocess.check_call([build_dump(tmp, sanitize), fin, fout], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        raws.append(open(fout, "rb").read())
    assert raws[0] == raws[1], "the sanitized build gives other bytes"
    return raws[0]


def main(out_name="ref_aln.npz"):
    B = aln_data.batches()
    raw, at = run_ref(B), 0
    out, n_regs, n_dropped, n_second, dropped_names, whole_kinds = {}, 0, 0, 0, [], set()
    for name, (o, reads) in B.items():
        ends, calls, call_off, dropped, flags, names = [], [], [0], [], [], []
        for r in reads:
            for g in range(r["regs"].size):
                hd = np.frombuffer(raw, "<i4", 4, at); at += 16
                c = np.frombuffer(raw, "<i4", 19 * int(hd[2]), at).reshape(-1, 19); at += 76 * int(hd[2])
                keep, dp = [], int(hd[3])
                for j in range(c.shape[0]):
                    if o["flag"] & 1 and c[j, 5] == 0 and c[j, 4] == -1:
                        n_second += 1                      # sr: the second pass of :737 behind an ungapped fill that tested as dropped; the fill itself makes no call, and
                        last_zdropped = int(c[j, 9])       # the region's dp_score then holds this call's score, not the ungapped one: marked unusable
                        dp = -(1 << 31)
                        continue
                    if keep and (c[j, :2] == c[keep[-1], :2]).all() and (c[j, 6:8] == c[keep[-1], 6:8]).all() and c[j, 5] == c[keep[-1], 5] & ~APPROX_MAX and c[keep[-1], 5] & APPROX_MAX:
                        n_second += 1                      # the second pass of :737; what it returned replaces the first pass's ez in the reference, but the plan only issues the first
                        last_zdropped = int(c[j, 9])
                        continue
                    keep.append(j)
                    last_zdropped = int(c[j, 9])
                gap_last = c.shape[0] > 0 and not (c[-1, 5] & 0x40)
                d = int(bool(gap_last and last_zdropped))
                ends.append([hd[0], hd[1], dp]); calls.append(c[keep]); call_off.append(call_off[-1] + len(keep)); dropped.append(d); names.append(r["names"][g])
                if d:
                    dropped_names.append(name + ":" + r["names"][g])
                else:
                    whole_kinds.update(k for k in PLANTED_KINDS if r["names"][g].startswith(k))
            flags.append(np.frombuffer(raw, "u1", r["a"].shape[0], at)); at += r["a"].shape[0]
        n_regs += len(names); n_dropped += sum(dropped)
        out[name + "_names"] = np.array(names); out[name + "_ends"] = np.array(ends, np.int32).reshape(-1, 3)
        out[name + "_calls"] = np.concatenate(calls).astype(np.int32) if calls else np.zeros((0, 19), np.int32)
        out[name + "_call_off"] = np.array(call_off, np.int64); out[name + "_dropped"] = np.array(dropped, np.uint8)
        out[name + "_flags"] = np.concatenate(flags) if flags else np.zeros(0, np.uint8)
    assert at == len(raw)
    print(n_regs, "regions,", n_dropped, "dropped:", dropped_names, ";", n_second, "second passes dropped")
    # the cap, as a condition: at least three quarters of all regions and one region of every planted kind run to their right-extension decision
    assert 4 * (n_regs - n_dropped) >= 3 * n_regs, "more than a quarter of the regions dropped"
    missing = set(PLANTED_KINDS) - whole_kinds
    assert not missing, "no undropped region of the planted kind(s) %s" % sorted(missing)
    out["counts"] = np.array([n_regs, n_dropped, n_second], np.int64)
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(*sys.argv[1:2])
