"""Region fixtures: the reference's own mm_gen_regs (hit.o: hit.c:52-88 with mm_reg_set_coor, mm_cal_fuzzy_len and klib's radix_sort_128x from misc.o) on every case
of tests/regs_data.py, and the read hash of map.c:290-292 computed with the reference's khash.h inlines.  Compiles tests/golden/regs_dump.c against the reference
objects build() leaves in oracle/_ref/.  Output: tests/golden/ref_regs.npz (data only): reg_size (sizeof(mm_reg1_t)), names, reg_off (regions per case), regs (the raw
mm_reg1_t arrays, one after another, uint8), n_tie_reads (cases in which two chains have the same sort key), hashes (one per entry of regs_data.HASH_CASES).  The inputs
are not stored: regs_data.cases() makes them again."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_OBJ = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regs_data  # noqa: E402
import regs_model  # noqa: E402


def main():
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "regs_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("hit", "misc", "kalloc")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", os.path.join(HERE, "regs_dump.c")] + objs + ["-o", dump, "-lm", "-lpthread"])
    cs = regs_data.cases()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            f.write(struct.pack("<IiiQ", c["hash"], c["qlen"], c["u"].size, c["a"].shape[0]) + c["u"].tobytes() + c["a"].tobytes())
        f.write(struct.pack("<i", len(regs_data.HASH_CASES)))
        for name, qlen_sum, seed in regs_data.HASH_CASES:
            nm = name or b""
            f.write(struct.pack("<ii", name is not None, len(nm)) + nm + struct.pack("<ii", qlen_sum, seed))
    subprocess.check_call([dump, fin, fout])
    raw = open(fout, "rb").read()
    size, = struct.unpack_from("<i", raw, 0)
    n_u = np.array([c["u"].size for c in cs], np.int64)
    reg_off = np.zeros(len(cs) + 1, np.int64)
    reg_off[1:] = np.cumsum(n_u)
    regs = np.frombuffer(raw, np.uint8, int(reg_off[-1]) * size, 4).reshape(-1, size)
    hashes = np.frombuffer(raw, np.uint32, len(regs_data.HASH_CASES), 4 + regs.size)
    assert 4 + regs.size + 4 * hashes.size == len(raw)
    path = os.path.join(HERE, "ref_regs.npz")
    np.savez_compressed(path, reg_size=np.array(size), names=np.array([c["name"] for c in cs]), reg_off=reg_off, regs=regs.copy(),
                        n_tie_reads=np.array(regs_model.n_tie_reads(cs)), hashes=hashes.copy())
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "cases,", int(reg_off[-1]), "regions of", size, "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
