"""Sketch / lookup fixtures: the reference's own mm_sketch (sketch.o) on real, synthetic and hand-made adversarial reads under nine (k, w, HPC) settings,
and, for map-ont and ava-ont, the index's key table and pool with collect_matches (map.c:90-123, restated in sketch_dump.c over mm_idx_get) for every read.
Compiles tests/golden/sketch_dump.c against the reference objects that build() leaves in oracle/_ref/.  Output: tests/golden/ref_sketch.npz (data only).
Layout: seq_off / seq = the reads (raw bytes).  Per configuration: <name>_kwh = (k, w, is_hpc), <name>_off = the minimizer offsets per read and
<name>_sha = the SHA-256 of every read's minimizer array (x, y as little-endian uint64 pairs): the outputs themselves would make the file several MB, the
digests pin them bit for bit.  Per index: <name>_keys (ascending) / _cr_off / _n / _pool / _mid_occ, kept whole (the tests build the index from them), and per read
<name>_match_off, <name>_rep_len, and the SHA-256 of the read's matches (cr_off int64, n, q_pos, q_span, seg_tandem uint32: mm2c_match_t) and of its mini_pos."""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_OBJ = os.path.join(ROOT, "oracle", "_ref")
DATA = os.path.join(HERE, "ref_testdata")

CONFIGS = [("map_ont", 15, 10, 0), ("ava_ont", 15, 5, 0), ("asm20", 19, 10, 0), ("sr", 21, 11, 0), ("map_pb", 19, 10, 1), ("ava_pb", 19, 5, 1),
           ("even_k16", 16, 10, 0), ("w1", 15, 1, 0), ("w255", 15, 255, 0)]
INDEXES = [("map_ont", 15, 10), ("ava_ont", 15, 5)]


def read_fasta(path):
    seqs, cur = [], None
    for line in open(path, "rb"):
        line = line.rstrip(b"\r\n")
        if line.startswith(b">"):
            cur = []
            seqs.append(cur)
        elif cur is not None:
            cur.append(line)
    return [b"".join(s) for s in seqs]


def adversarial(rng):
    A = b"ACGT"
    rnd = lambda n: rng.choice(np.frombuffer(A, np.uint8), n).tobytes()
    reads = [
        b"N" * 40 + rnd(300) + b"N" * 7 + rnd(200) + b"NNNN",                # N runs at the start, inside and at the end
        rnd(150).lower() + rnd(150) + b"RYKMSWBDHVN" * 3 + rnd(100),          # lowercase and IUPAC bytes
        rnd(50) + b"A" * 300 + rnd(60) + b"c" * 256 + b"G" * 255 + rnd(80),   # homopolymers of >= 256 bases (the HPC span cut)
        b"ACACACACAC" * 60 + rnd(100) + b"AATT" * 80,                          # short tandem repeats: identical minimizers in a window
        b"AT" * 300 + rnd(50) + b"GC" * 200 + b"ACGT" * 100,                   # symmetric k-mers for even k
        bytes(range(256)) * 3 + rnd(100),                                      # every byte value (0-3 are nucleotides)
        b"", rnd(3), rnd(14), rnd(15),                                          # shorter than k, exactly k
        rnd(10 + 15 - 1), rnd(10 + 15), rnd(5 + 15 - 1), rnd(5 + 15),           # w+k-1 and w+k for map-ont and ava-ont
        rnd(19 + 10 - 1), rnd(255 + 15 - 1), rnd(255 + 15),
        (rnd(40) + b"N") * 30,
        rnd(100_000),                                                            # 1e5 bases
    ]
    return reads


def digests(arrays):
    """SHA-256 of each array's bytes, one row per read"""
    return np.array([np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8) for a in arrays], np.uint8).reshape(-1, 32)


def write_reads(path, reads):
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(reads)))
        f.write(off.tobytes())
        f.write(b"".join(reads))
    return off


def main():
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "sketch_dump")
    objs = [os.path.join(REF_OBJ, o + ".o") for o in ("sketch", "index", "bseq", "kalloc", "kthread", "misc", "sdust")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", os.path.join(HERE, "sketch_dump.c")] + objs + ["-o", dump, "-lz", "-lm", "-lpthread"])
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_genome.py"), os.path.join(tmp, "syn"), "--genome-mb", "0.05",
                           "--reads", "6", "--read-len", "4000", "--seed", "5"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(2026)
    reads = []
    for name in ("MT-orang.fa", "q-inv.fa", "q2.fa"):
        reads += read_fasta(os.path.join(DATA, name))
    reads += read_fasta(os.path.join(tmp, "syn.reads.fa"))
    reads += adversarial(rng)
    # two repeat families in the reference (below): a 150-base unit 80 times sets mid_occ (its ~27 keys are the 2e-4 most frequent), a 24-base unit
    # 300 times lies above it -- the read that carries both has repetitive minimizers (rep_len > 0) and matches with many hits
    unit = rng.choice(np.frombuffer(b"ACGT", np.uint8), 150).tobytes()
    unit2 = rng.choice(np.frombuffer(b"ACGT", np.uint8), 24).tobytes()
    flank = lambda: rng.choice(np.frombuffer(b"ACGT", np.uint8), 300).tobytes()
    reads.append(flank() + unit * 3 + flank() + unit2 * 8 + flank() + unit2 * 4 + flank())
    rpath = os.path.join(tmp, "reads.bin")
    off = write_reads(rpath, reads)
    out = {"seq_off": off, "seq": np.frombuffer(b"".join(reads), np.uint8)}
    for name, k, w, hpc in CONFIGS:
        o = os.path.join(tmp, name + ".bin")
        subprocess.check_call([dump, "sketch", str(k), str(w), str(hpc), rpath, o])
        raw, pos, cnt, mini = open(o, "rb").read(), 0, [0], []
        for _ in range(len(reads)):
            n, = struct.unpack_from("<q", raw, pos); pos += 8
            mini.append(np.frombuffer(raw, np.uint64, 2 * n, pos).reshape(n, 2)); pos += 16 * n
            cnt.append(cnt[-1] + n)
        out[name + "_off"] = np.array(cnt, np.int64)
        out[name + "_sha"] = digests(mini)
        out[name + "_kwh"] = np.array([k, w, hpc], np.int32)
    # the index: MT-human with the synthetic genome behind it would be two parts; one reference file per index keeps it to one part
    refs = os.path.join(tmp, "ref.fa")
    with open(refs, "wb") as f:
        for p in (os.path.join(DATA, "MT-human.fa"), os.path.join(DATA, "t-inv.fa"), os.path.join(tmp, "syn.ref.fa")):
            f.write(open(p, "rb").read().rstrip(b"\n") + b"\n")
        f.write(b">repeats\n" + unit * 80 + b"\n>repeats2\n" + unit2 * 300 + b"\n")
    for name, k, w in INDEXES:
        o = os.path.join(tmp, name + "_idx.bin")
        subprocess.check_call([dump, "index", str(k), str(w), refs, rpath, o])
        raw = open(o, "rb").read()
        mid_occ, = struct.unpack_from("<i", raw, 0); pos = 4
        n_pool, = struct.unpack_from("<q", raw, pos); pos += 8
        pool = np.frombuffer(raw, np.uint64, n_pool, pos); pos += 8 * n_pool
        n_keys, = struct.unpack_from("<q", raw, pos); pos += 8
        kt = np.frombuffer(raw, np.dtype([("key", "<u8"), ("cr_off", "<i8"), ("n", "<u4")]), n_keys, pos); pos += 20 * n_keys
        mo, rl, mats, mps = [0], [], [], []
        for _ in range(len(reads)):
            n_mini, = struct.unpack_from("<q", raw, pos); pos += 8 + 16 * n_mini
            r, = struct.unpack_from("<i", raw, pos); pos += 4
            n_m, = struct.unpack_from("<q", raw, pos); pos += 8
            mats.append(np.frombuffer(raw, np.dtype([("cr_off", "<i8"), ("n", "<u4"), ("q_pos", "<u4"), ("q_span", "<u4"), ("seg_tandem", "<u4")]), n_m, pos))
            pos += 24 * n_m
            mps.append(np.frombuffer(raw, np.uint64, n_m, pos)); pos += 8 * n_m
            mo.append(mo[-1] + n_m); rl.append(r)
        out[name + "_mid_occ"] = np.array([mid_occ], np.int32)
        out[name + "_pool"] = pool.copy()
        kt = np.sort(kt, order="key")
        out[name + "_keys"], out[name + "_cr_off"], out[name + "_n"] = kt["key"].copy(), kt["cr_off"].copy(), kt["n"].copy()
        out[name + "_match_off"] = np.array(mo, np.int64)
        out[name + "_match_sha"] = digests(mats)
        out[name + "_rep_len"] = np.array(rl, np.int32)
        out[name + "_mini_pos_sha"] = digests(mps)
    np.savez_compressed(os.path.join(HERE, "ref_sketch.npz"), **out)


if __name__ == "__main__":
    main()
