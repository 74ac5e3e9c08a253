"""Fragment-segment fixtures: the reference's own mm_gen_regs -> mm_set_parent -> mm_select_sub_multi -> mm_seg_gen -> per segment mm_set_parent -> mm_set_mapq
(hit.o: hit.c:52-88, 125-186, 220-253, 373-427, 463-508; pe.o: pe.c:6-43; klib's sorts from misc.o and the host's own logf) on every case of tests/seg_data.py, each
under its own options.  Compiles tests/golden/seg_dump.c against the reference objects build() leaves in oracle/_ref/.
Output: tests/golden/ref_seg.npz (data only): reg_size, names, libm (the C library's version string the fixture was made with); sel_off / sel (the raw mm_reg1_t
arrays behind mm_select_sub_multi, per case); per segment read (case-major, case k owns seg reads sr_off[k] .. sr_off[k+1]): su_off / su, sb_off / sb (uint64 [., 2]),
seg_regs (out of mm_seg_gen) and seg_final (behind mm_set_mapq), both indexed like su.  The chains and anchors are not stored: seg_data.cases() makes them again."""
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
import regs_model  # noqa: E402
import seg_data  # noqa: E402


def main(out_name="ref_seg.npz"):
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "seg_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("hit", "pe", "misc", "kalloc")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", os.path.join(HERE, "seg_dump.c")] + objs + ["-o", dump, "-lm", "-lpthread"])
    cs = seg_data.cases()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            h, m = c["hit"], c["multi"]
            f.write(struct.pack("<Ii", c["hash"], c["n_segs"])); f.write(c["qlens"].astype("<i4").tobytes())
            f.write(struct.pack("<iq", c["u"].size, c["a"].shape[0]))
            f.write(c["u"].tobytes()); f.write(c["a"].tobytes())
            f.write(struct.pack("<fiifii", h["mask_level"], h["mask_len"], h["hard_mask_level"], h["pri_ratio"], h["min_diff"], h["best_n"]))
            f.write(struct.pack("<ffiii", m["pri1"], m["pri2"], c["gap_ref"], c["mapq"]["min_chain_score"], c["rep_len"]))
    subprocess.check_call([dump, fin, fout])
    raw = open(fout, "rb").read()
    size, = struct.unpack_from("<i", raw, 0)
    assert size == 80
    at = 4
    n_sel, p_sel, n_su, p_su, n_sb, p_sb, p_regs, p_fin, n_sr = [], [], [], [], [], [], [], [], []

    def take(n, dtype, width):
        nonlocal at
        v = np.frombuffer(raw, dtype, n * width, at).reshape(-1, width)
        at += v.nbytes
        return v

    n_tied = 0
    for c in cs:
        n, = struct.unpack_from("<i", raw, at); at += 4
        n_sel.append(n); p_sel.append(take(n, np.uint8, size))
        for s in range(c["n_segs"]):
            nu, = struct.unpack_from("<i", raw, at); at += 4
            u = take(nu, np.uint64, 1)
            na, = struct.unpack_from("<i", raw, at); at += 4
            a = take(na, np.uint64, 2)
            n_su.append(nu); p_su.append(u.reshape(-1)); n_sb.append(na); p_sb.append(a)
            p_regs.append(take(nu, np.uint8, size)); p_fin.append(take(nu, np.uint8, size))
            zx = [z[0] for z in regs_model.keys(c["hash"], u.reshape(-1), a)] if nu else []
            n_tied += (len(set(zx)) != len(zx)) and nu > 64
        n_sr.append(c["n_segs"])
    assert at == len(raw)
    assert n_tied >= 1, "no segment read of more than 64 chains holds equal sort keys"
    off = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, reg_size=np.array(size), names=np.array([c["name"] for c in cs]), libm=np.array(" ".join(platform.libc_ver())),
                        sel_off=off(n_sel), sel=np.concatenate(p_sel), sr_off=off(n_sr), su_off=off(n_su), su=np.concatenate(p_su),
                        sb_off=off(n_sb), sb=np.concatenate(p_sb), seg_regs=np.concatenate(p_regs), seg_final=np.concatenate(p_fin))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "cases,", sum(n_sel), "hits,", sum(n_su), "segment chains,", sum(n_sb), "segment anchors,", n_tied,
          "segment reads of more than 64 chains with tied keys")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(*sys.argv[1:2])
