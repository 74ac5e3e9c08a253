"""The chaining distances mm_map_frag gives a fragment (map.c:305-314) in a few lines of NumPy, in the reference's int arithmetic: from the fragment's total
length qlen_sum and the four option scalars to (max_dist_x, max_dist_y) = (max_chain_gap_ref, max_chain_gap_qry).  Pinned to what the reference recorded by
tests/test_cpu_frag_gaps_data.py."""
import numpy as np


def frag_dists(qlen_sum, is_sr, max_gap, max_gap_ref, max_frag_len):
    """qlen_sum: int array [n] -> int32 [n, 2] of (max_dist_x, max_dist_y)"""
    q = np.asarray(qlen_sum, np.int64)
    y = np.maximum(q, max_gap) if is_sr else np.full_like(q, max_gap)
    if max_gap_ref > 0:
        x = np.full_like(q, max_gap_ref)
    elif max_frag_len > 0:
        x = np.maximum(max_frag_len - q, max_gap)
    else:
        x = np.full_like(q, max_gap)
    return np.stack([x, y], axis=1).astype(np.int32)


def qlen_sums(frag_off, seq_off):
    fo, so = np.asarray(frag_off, np.int64), np.asarray(seq_off, np.int64)
    return so[fo[1:]] - so[fo[:-1]]
