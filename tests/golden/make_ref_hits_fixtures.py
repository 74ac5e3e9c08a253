"""Hit fixtures: the reference's own mm_set_parent and mm_select_sub (hit.o: hit.c:125-186, 220-272, with klib's radix_sort_64 from misc.o) on every case of
a data module under tests/, each under its own options.  Usage: make_ref_hits_fixtures.py [data module [output name]] -- hits_data and ref_hits.npz by default,
hits_limit_data ref_hits_limits.npz for the cases at the kernel's own limits.  Compiles tests/golden/hits_dump.c against the reference objects build() leaves in oracle/_ref/.
Output: tests/golden/<output name> (data only): reg_size (sizeof(mm_reg1_t)), names, opts (one row of mask_level, mask_len, hard_mask_level, pri_ratio, min_diff, best_n
per case, as doubles), n_in, n_out, hit_off, hits (the raw mm_reg1_t arrays after the two calls, n_out[k] regions per case one after another, uint8).  The inputs are
not stored: the module's cases() makes them again."""
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
import hits_data  # noqa: E402


def main(module="hits_data", out_name="ref_hits.npz"):
    data = __import__(module)
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "hits_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("hit", "misc", "kalloc")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", os.path.join(HERE, "hits_dump.c")] + objs + ["-o", dump, "-lm", "-lpthread"])
    cs = data.cases()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            o = c["opt"]
            f.write(struct.pack("<fiifiii", o["mask_level"], o["mask_len"], o["hard_mask_level"], o["pri_ratio"], o["min_diff"], o["best_n"], c["regs"].size))
            f.write(c["regs"].tobytes())
    subprocess.check_call([dump, fin, fout])
    raw = open(fout, "rb").read()
    size, = struct.unpack_from("<i", raw, 0)
    assert size == cs[0]["regs"].dtype.itemsize
    at, n_out, parts = 4, [], []
    for c in cs:
        n, = struct.unpack_from("<i", raw, at)
        at += 4
        parts.append(np.frombuffer(raw, np.uint8, n * size, at).reshape(-1, size))
        at += n * size
        n_out.append(n)
    assert at == len(raw)
    hit_off = np.zeros(len(cs) + 1, np.int64)
    hit_off[1:] = np.cumsum(n_out)
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, reg_size=np.array(size), names=np.array([c["name"] for c in cs]), opts=np.array([hits_data.opt_key(c["opt"]) for c in cs], np.float64),
                        n_in=np.array([c["regs"].size for c in cs], np.int64), n_out=np.array(n_out, np.int64), hit_off=hit_off, hits=np.concatenate(parts))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "cases,", int(hit_off[-1]), "hits of", size, "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(*sys.argv[1:3])
