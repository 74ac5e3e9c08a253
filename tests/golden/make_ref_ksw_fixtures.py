"""Base-alignment fixtures: the reference's own ksw_extd2_sse (ksw2_extd2_sse.c, built with SSE4.1 as the rest of oracle/_ref/) on every case of tests/ksw_data.py.
Compiles tests/golden/ksw_dump.c against the reference objects build() leaves in oracle/_ref/ (ksw2_extd2_sse.o, kalloc.o).
Output: tests/golden/ref_ksw.npz (data only): names; ez (int32 [n, 11]: max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end);
cig_off (int64 [n + 1]) and cigar (uint32): case k owns cigar[cig_off[k] .. cig_off[k + 1]).  Inputs are not stored: ksw_data.cases() makes them again.
Every case runs twice, through a kalloc pool filled with 0x00 and with 0xA5 before each call; the two outputs must be equal (the function reads a few bytes behind
its allocation).  A case that differs is an error of this generator, not a case to leave out."""
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
import ksw_data  # noqa: E402


def write_tasks(path, cs):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            mat, q, e, q2, e2 = ksw_data.score_set(c["sc"])
            f.write(struct.pack("<6i", c["q"].size, c["t"].size, c["w"], c["zdrop"], c["end_bonus"], c["flag"]))
            f.write(mat.tobytes()); f.write(struct.pack("<4b", q, e, q2, e2))
            f.write(c["q"].tobytes()); f.write(c["t"].tobytes())


def build_dump(tmp):
    dump = os.path.join(tmp, "ksw_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("ksw2_extd2_sse", "kalloc")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", os.path.join(HERE, "ksw_dump.c")] + objs + ["-o", dump])
    return dump


def run_ref(cs, fills=(0x00, 0xA5)):
    tmp = tempfile.mkdtemp()
    dump = build_dump(tmp)
    fin = os.path.join(tmp, "in.bin")
    write_tasks(fin, cs)

    def parse(raw):
        ez, cig, at = [], [], 0
        for c in cs:
            e = np.frombuffer(raw, "<i4", 11, at); at += 44
            g = np.frombuffer(raw, "<u4", int(e[9]), at); at += 4 * int(e[9])
            ez.append(e); cig.append(g)
        assert at == len(raw)
        return ez, cig

    outs = []
    for fill in fills:
        fout = os.path.join(tmp, "out%d.bin" % fill)
        subprocess.check_call([dump, fin, fout, str(fill)])
        outs.append(parse(open(fout, "rb").read()))
    ez, cig = outs[0]
    for ez2, cig2 in outs[1:]:                                                   # each file parsed on its own, then case by case
        for c, e, g, e2, g2 in zip(cs, ez, cig, ez2, cig2):
            assert np.array_equal(e, e2) and np.array_equal(g, g2), "case %s depends on the pool's fill" % c["name"]
    return np.array(ez, np.int32).reshape(-1, 11), cig


def main(out_name="ref_ksw.npz"):
    cs = ksw_data.cases()
    ez, cig = run_ref(cs)
    off = np.concatenate([[0], np.cumsum([g.size for g in cig])]).astype(np.int64)
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, names=np.array([c["name"] for c in cs]), ez=ez, cig_off=off, cigar=np.concatenate(cig).astype(np.uint32))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "cases,", int(off[-1]), "CIGAR words,", int(ez[:, 1].sum()), "z-dropped,",
          int(ez[:, 10].sum()), "reach_end")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(*sys.argv[1:2])
