"""A NumPy restatement of the reference's minimizer index key table, for the tests of reads in, chains out: the minimizers of every reference sequence
(sketch_model.sketch_array, rid = the sequence's number in y's high 32 bits) grouped by key (x >> 8), each key's hits the y values in ascending order
(worker_post, index.c:191-233: radix_sort_64 of p[] per key), and mm_idx_cal_max_occ (index.c:164-185).  Laid out as mm2chain.MinimizerIndex takes it:
keys ascending, cr_off / n into one pool.  Unlike the reference, which keeps a singleton's hit in its hash table, a singleton gets one pool slot."""
import numpy as np

import sketch_model as sm


def sketch_refs(seqs, k, w, is_hpc=False):
    """the minimizers of each reference sequence with its number as rid: uint64 [m, 2] (x, y), in sequence order"""
    parts = []
    for rid, s in enumerate(seqs):
        a = sm.sketch_array(s, w, k, is_hpc)
        if a.shape[0]:
            a[:, 1] |= np.uint64(rid) << np.uint64(32)
        parts.append(a)
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.uint64)


def build_from_minimizers(mini):
    """(keys uint64 ascending, cr_off int64, n uint32, pool uint64) from minimizers uint64 [m, 2]"""
    key = mini[:, 0] >> np.uint64(8)
    order = np.lexsort((mini[:, 1], key))                     # by key, then y ascending within a key
    key, y = key[order], mini[order, 1]
    keys, first, n = np.unique(key, return_index=True, return_counts=True)
    return keys.astype(np.uint64), first.astype(np.int64), n.astype(np.uint32), np.ascontiguousarray(y, dtype=np.uint64)


def build_index(seqs, k, w, is_hpc=False):
    """the key table of mm_idx_build over `seqs` (bytes each): (keys, cr_off, n, pool)"""
    return build_from_minimizers(sketch_refs(seqs, k, w, is_hpc))


def cal_max_occ(n, f=2e-4):
    """mm_idx_cal_max_occ: the ((1 - f) * n_keys)-th smallest hit count (from 0, ks_ksmall), plus 1.  f is a float there, widened to double"""
    n = np.asarray(n)
    if f <= 0:
        return 2**31 - 1
    i = int((1.0 - float(np.float32(f))) * n.size)
    return int(np.partition(n.astype(np.int64), i)[i]) + 1
