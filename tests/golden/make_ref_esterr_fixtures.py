"""Chain-anchor divergence fixtures: the reference's own mm_gen_regs -> mm_set_parent -> mm_select_sub -> (mm_join_long) -> mm_est_err -> mm_set_mapq (hit.o and
esterr.o, with klib's sorts from misc.o and the host's own pow and logf) on every case of tests/esterr_data.py.  Compiles tests/golden/esterr_dump.c against the
reference objects build() leaves in oracle/_ref/.
Output: tests/golden/ref_esterr.npz (data only): reg_size, names, libm (the C library's version string the fixture was made with), n_out / out_off / regs_out (the raw
mm_reg1_t arrays behind mm_set_mapq, div included), n_b_out / a_off / a_out (the final a[] of every case: uint64 [., 2]).  The chains, anchors, mini_pos and ref_len
are not stored: esterr_data.cases() makes them again.
With arguments `<data module> <file name>` the cases() of another module under tests/ go into another file: `anchor_space_limit_data ref_esterr_limits.npz`."""
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
import importlib  # noqa: E402


def main(module="esterr_data", out_name="ref_esterr.npz"):
    """module: the data module under tests/ whose cases() to run (by default esterr_data, into ref_esterr.npz)"""
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "esterr_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("hit", "esterr", "misc", "kalloc")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", os.path.join(HERE, "esterr_dump.c")] + objs + ["-o", dump, "-lm", "-lpthread"])
    cs = importlib.import_module(module).cases()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            h, m = c["hit"], c["mapq"]
            f.write(struct.pack("<Iiiqii", c["hash"], c["qlen"], c["u"].size, c["a"].shape[0], c["mini_pos"].size, c["ref_len"].size))
            f.write(c["u"].tobytes()); f.write(c["a"].tobytes()); f.write(c["mini_pos"].tobytes()); f.write(c["ref_len"].tobytes())
            f.write(struct.pack("<fiifii", h["mask_level"], h["mask_len"], h["hard_mask_level"], h["pri_ratio"], h["min_diff"], h["best_n"]))
            f.write(struct.pack("<iiiifii", m["do_join"], m["max_join_long"], m["max_join_short"], m["min_join_flank_sc"], m["min_join_flank_ratio"], m["min_cnt"],
                                m["min_chain_score"]))
            f.write(struct.pack("<i", c["rep_len"]))
    subprocess.check_call([dump, fin, fout])
    raw = open(fout, "rb").read()
    size, = struct.unpack_from("<i", raw, 0)
    assert size == 80
    at, n_out, n_b, p_out, p_a = 4, [], [], [], []
    for c in cs:
        n, = struct.unpack_from("<i", raw, at)
        at += 4
        p_out.append(np.frombuffer(raw, np.uint8, n * size, at).reshape(-1, size))
        at += n * size
        n_out.append(n)
        nb, = struct.unpack_from("<q", raw, at)
        at += 8
        p_a.append(np.frombuffer(raw, np.uint64, nb * 2, at).reshape(-1, 2))
        at += nb * 16
        n_b.append(nb)
    assert at == len(raw)
    off = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, reg_size=np.array(size), names=np.array([c["name"] for c in cs]), libm=np.array(" ".join(platform.libc_ver())),
                        n_out=np.array(n_out, np.int64), out_off=off(n_out), regs_out=np.concatenate(p_out),
                        n_b_out=np.array(n_b, np.int64), a_off=off(n_b), a_out=np.concatenate(p_a))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "cases,", sum(n_out), "regions,", sum(n_b), "anchors")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(*sys.argv[1:3])
