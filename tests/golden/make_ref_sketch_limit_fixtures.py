"""Sketch / index fixtures at the limits of the device's lanes: the reference's own mm_sketch (sketch.o) on every read of tests/sketch_limit_data.py under its six
(k, w, HPC) settings, and, for (15, 10, 0) and (19, 5, 1), the reference's index (mm_idx_reader_read) of the lists of 3 and 257 sequences with collect_matches
(map.c:90-123, restated in sketch_dump.c over mm_idx_get) for the lookup reads against it.  Compiles tests/golden/sketch_dump.c against the reference objects that
build() leaves in oracle/_ref/, as make_ref_sketch_fixtures.py does.  Output: tests/golden/ref_sketch_limits.npz (data only).
Layout, per setting k<k>_w<w>_h<hpc>: _off = the minimizer offsets per read of batch(setting), _sha = the SHA-256 of every read's minimizer array (x, y as
little-endian uint64 pairs), _input_sha = the SHA-256 of every case's input (its reads, each behind its length as int64) in the order of cases(setting): a data
module that drifts is noticed.  Per index k<k>_w<w>_h<hpc>_n<n_seqs>: _input_sha of the sequence list and of the reads, _table_sha (keys ascending as uint64, then
their n as uint32), _plant_keys / _plant_sha (every key of the planted string that the index holds, and the SHA-256 of its hit list), _mid_occ
(mm_idx_cal_max_occ(mi, 2e-4)), and per read _match_off, _rep_len and the SHA-256 of its matches without their pool offsets (n, q_pos, q_span, seg_tandem as
uint32: the reference keeps a singleton's hit in its hash table, so offsets differ) and of its mini_pos."""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import make_ref_sketch_fixtures as g          # noqa: E402
import sketch_limit_data as sd                # noqa: E402

INDEX_SETTINGS = ((15, 10, 0), (19, 5, 1))
INDEX_LISTS = (3, 257)
MATCH_FIELDS = np.dtype([("n", "<u4"), ("q_pos", "<u4"), ("q_span", "<u4"), ("seg_tandem", "<u4")])


def name_of(S):
    return "k%d_w%d_h%d" % S


def input_sha(reads):
    h = hashlib.sha256()
    for r in reads:
        h.update(struct.pack("<q", len(r)) + bytes(r))
    return np.frombuffer(h.digest(), np.uint8)


def index_reads(S, n_seqs):
    """the reads looked up in the reference's index of seq_list(n_seqs, S): the reads of two lookup cases, the sequences that carry the planted
    string (they match), and reads without a match"""
    seqs, planted = sd.seq_list(n_seqs, S)
    reads = [r for c in sd.lookup_cases() if c["name"] in ("tandem_edges", "mid_occ_2") for r in c["reads"]]
    return reads + [seqs[i] for i in planted] + [seqs[planted[0]] + b"N" * 70 + seqs[planted[-1]]]


def main():
    tmp = tempfile.mkdtemp()
    dump = os.path.join(tmp, "sketch_dump")
    objs = [os.path.join(g.REF_OBJ, o + ".o") for o in ("sketch", "index", "bseq", "kalloc", "kthread", "misc", "sdust")]
    subprocess.check_call(["gcc", "-O2", "-w", "-DHAVE_KALLOC", "-I/root/reference", os.path.join(HERE, "sketch_dump.c")] + objs + ["-o", dump, "-lz", "-lm", "-lpthread"])
    out = {}
    for S in sd.SETTINGS:
        k, w, hpc = S
        name = name_of(S)
        reads = sd.batch(S)[0]
        rpath, o = os.path.join(tmp, name + ".reads"), os.path.join(tmp, name + ".bin")
        g.write_reads(rpath, reads)
        subprocess.check_call([dump, "sketch", str(k), str(w), str(hpc), rpath, o])
        raw, pos, cnt, mini = open(o, "rb").read(), 0, [0], []
        for _ in range(len(reads)):
            n, = struct.unpack_from("<q", raw, pos); pos += 8
            mini.append(np.frombuffer(raw, np.uint64, 2 * n, pos).reshape(n, 2)); pos += 16 * n
            cnt.append(cnt[-1] + n)
        out[name + "_off"] = np.array(cnt, np.int64)
        out[name + "_sha"] = g.digests(mini)
        out[name + "_input_sha"] = np.array([input_sha(c["reads"]) for c in sd.cases(S)], np.uint8)
    for S in INDEX_SETTINGS:
        k, w, hpc = S
        for n_seqs in INDEX_LISTS:
            name = name_of(S) + "_n%d" % n_seqs
            seqs = sd.seq_list(n_seqs, S)[0]
            reads = index_reads(S, n_seqs)
            fa, rpath, o = os.path.join(tmp, name + ".fa"), os.path.join(tmp, name + ".reads"), os.path.join(tmp, name + ".bin")
            with open(fa, "wb") as f:
                for i, s in enumerate(seqs):                      # a record without bases keeps its number (index.c:330)
                    f.write(b">s%d\n" % i + (s + b"\n" if s else b""))
            g.write_reads(rpath, reads)
            subprocess.check_call([dump, "index", str(k), str(w), fa, rpath, o, str(hpc)])
            raw = open(o, "rb").read()
            mid_occ, = struct.unpack_from("<i", raw, 0); pos = 4
            n_pool, = struct.unpack_from("<q", raw, pos); pos += 8
            pool = np.frombuffer(raw, np.uint64, n_pool, pos); pos += 8 * n_pool
            n_keys, = struct.unpack_from("<q", raw, pos); pos += 8
            kt = np.sort(np.frombuffer(raw, np.dtype([("key", "<u8"), ("cr_off", "<i8"), ("n", "<u4")]), n_keys, pos), order="key"); pos += 20 * n_keys
            mo, rl, mats, mps = [0], [], [], []
            for _ in range(len(reads)):
                n_mini, = struct.unpack_from("<q", raw, pos); pos += 8 + 16 * n_mini
                r, = struct.unpack_from("<i", raw, pos); pos += 4
                n_m, = struct.unpack_from("<q", raw, pos); pos += 8
                m = np.frombuffer(raw, np.dtype([("cr_off", "<i8"), ("n", "<u4"), ("q_pos", "<u4"), ("q_span", "<u4"), ("seg_tandem", "<u4")]), n_m, pos)
                mats.append(np.ascontiguousarray(m[list(MATCH_FIELDS.names)]).astype(MATCH_FIELDS)); pos += 24 * n_m
                mps.append(np.frombuffer(raw, np.uint64, n_m, pos)); pos += 8 * n_m
                mo.append(mo[-1] + n_m); rl.append(r)
            plant = [key for key in sd.planted_keys(S) if key in set(kt["key"].tolist())]
            rows = {int(a): (int(b), int(c)) for a, b, c in zip(kt["key"], kt["cr_off"], kt["n"])}
            out[name + "_input_sha"] = np.array([input_sha(seqs), input_sha(reads)], np.uint8)
            out[name + "_table_sha"] = g.digests([np.concatenate([kt["key"].astype("<u8").view(np.uint8), kt["n"].astype("<u4").view(np.uint8)])])
            out[name + "_plant_keys"] = np.array(plant, np.uint64)
            out[name + "_plant_sha"] = g.digests([pool[rows[key][0]:rows[key][0] + rows[key][1]] for key in plant])
            out[name + "_mid_occ"] = np.array([mid_occ], np.int32)
            out[name + "_match_off"] = np.array(mo, np.int64)
            out[name + "_rep_len"] = np.array(rl, np.int32)
            out[name + "_match_sha"] = g.digests(mats)
            out[name + "_mini_pos_sha"] = g.digests(mps)
    np.savez_compressed(os.path.join(HERE, "ref_sketch_limits.npz"), **out)


if __name__ == "__main__":
    main()
