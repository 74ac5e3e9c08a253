"""Fixtures of the extra plan: the reference's own mm_update_extra and mm_test_zdrop (static in align.c) on every case of tests/extra_data.py.
Compiles tests/golden/extra_dump.c, which includes the reference's align.c from the reference's directory (REF, default: `reference` beside the repository; nothing of
it is copied), against the reference objects build() leaves in oracle/_ref/ -- without align.o and ksw2_ll_sse.o, whose two functions the dump defines itself -- and
a one-line stub for mm_idxopt_init.  The dump is built a second time with -fsanitize=address,undefined and every case runs through both: a case that trips the
sanitizer is an input the reference is not defined on, belongs to the plan's refusals and is an error of this generator if it stays in.
Output: tests/golden/ref_extra.npz (data only; the inputs are made again by extra_data):
  u_names; u_res int32 [n, 2, 8]: per case and is_eqx 0 / 1: n_cigar, qshift, tshift, blen, mlen, n_ambi, dp_max, 0; u_cig_off int64 [2 n + 1], u_cigar uint32: the
  CIGAR of case k under is_eqx x is u_cigar[u_cig_off[2 k + x] .. u_cig_off[2 k + x + 1]);
  z_names; z_res int32 [n, 9]: max_zdrop, t0 (pos[0][0]), t_len, q_len, FNV-1a of the reverse-complemented query bytes the inversion test received, and the
  return value and whether the inversion test was entered under each threshold set of extra_data.ZD_THR."""
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
import extra_data  # noqa: E402

OBJS = ("kalloc", "misc", "index", "hit", "esterr", "pe", "sketch", "sdust", "bseq", "kthread", "ksw2_extz2_sse", "ksw2_extd2_sse", "ksw2_exts2_sse")


def build_dump(tmp, sanitize):
    stub = os.path.join(tmp, "stub.c")
    with open(stub, "w") as f:
        f.write("void mm_idxopt_init(void *o) { (void)o; }\n")
    dump = os.path.join(tmp, "extra_dump_san" if sanitize else "extra_dump")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["gcc", "-w", "-DHAVE_KALLOC", "-msse4.1", "-I" + REF] + flags + [os.path.join(HERE, "extra_dump.c"), stub] +
                          [os.path.join(REF_OBJ, o + ".o") for o in OBJS] + ["-o", dump, "-lz", "-lm", "-lpthread"])
    return dump


def write_cases(path, us, zs):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", 2 * len(us)))
        for c in us:
            mat, q, e = extra_data.score_set(c["sc"])[:3]
            ln, op = c["cigar"] >> 4, c["cigar"] & 0xf
            assert int(ln[op <= 1].sum()) == c["q"].size and int(ln[(op == 0) | (op >= 2)].sum()) == c["t"].size and (op <= 3).all(), "case %s is not a CIGAR of its sequences" % c["name"]
            for x in (0, 1):
                f.write(struct.pack("<5i", c["q"].size, c["t"].size, c["cigar"].size, c["rev"], x))
                f.write(mat.tobytes()); f.write(struct.pack("<2b", q, e))
                f.write(c["cigar"].astype("<u4").tobytes()); f.write(c["q"].tobytes()); f.write(c["t"].tobytes())
        f.write(struct.pack("<i", len(zs)))
        for c in zs:
            mat, q, e = extra_data.score_set(c["sc"])[:3]
            f.write(struct.pack("<11i", c["q"].size, c["t"].size, c["cigar"].size, *extra_data.ZD_THR[0], *extra_data.ZD_THR[1]))
            f.write(mat.tobytes()); f.write(struct.pack("<2b", q, e))
            f.write(c["cigar"].astype("<u4").tobytes()); f.write(c["q"].tobytes()); f.write(c["t"].tobytes())


def run_ref(us, zs):
    tmp = tempfile.mkdtemp()
    fin = os.path.join(tmp, "in.bin")
    write_cases(fin, us, zs)
    raws = []
    for sanitize in (False, True):
        fout = os.path.join(tmp, "out%d.bin" % sanitize)
        subprocess.check_call([build_dump(tmp, sanitize), fin, fout], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        raws.append(open(fout, "rb").read())
    assert raws[0] == raws[1], "the sanitized build gives other bytes"
    raw, at = raws[0], 0
    u_res, u_cig = [], []
    for c in us:
        pair = []
        for x in (0, 1):
            o = np.frombuffer(raw, "<i4", 9, at); at += 36
            g = np.frombuffer(raw, "<u4", int(o[0]), at); at += 4 * int(o[0])
            assert o[4] == 0 and (o[1] == 0 or o[2] == 0) and (o[2] == 0) == (c["rev"] == 0 or o[1] + o[2] == 0), c["name"]      # re stays; qs moves if !rev, qe if rev
            pair.append([o[0], o[1] + o[2], o[3], o[5], o[6], o[7], o[8], 0]); u_cig.append(g)
        u_res.append(pair)
    z_res = np.frombuffer(raw, "<i4", 9 * len(zs), at).reshape(-1, 9); at += 36 * len(zs)
    assert at == len(raw)
    return np.array(u_res, np.int32).reshape(-1, 2, 8), u_cig, z_res


def main(out_name="ref_extra.npz"):
    us, zs = extra_data.update_cases(), extra_data.zdrop_cases()
    u_res, u_cig, z_res = run_ref(us, zs)
    off = np.concatenate([[0], np.cumsum([g.size for g in u_cig])]).astype(np.int64)
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, u_names=np.array([c["name"] for c in us]), u_res=u_res, u_cig_off=off, u_cigar=np.concatenate(u_cig).astype(np.uint32),
                        z_names=np.array([c["name"] for c in zs]), z_res=z_res.astype(np.int32))
    print("wrote", path, os.path.getsize(path), "bytes;", len(us), "update cases,", int(off[-1]), "CIGAR words,", int((u_res[:, 0, 1:3] != 0).any(1).sum()), "with a leading indel stripped;",
          len(zs), "z-drop cases,", [int((z_res[:, 5 + 2 * k] == 1).sum()) for k in (0, 1)], "with code 1,", [int(z_res[:, 6 + 2 * k].sum()) for k in (0, 1)], "inversion tests")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(*sys.argv[1:2])
