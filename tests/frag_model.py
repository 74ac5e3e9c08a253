"""A NumPy / Python restatement of mm_map_frag's way from segments to chains for a fragment of several segments (map.c:272-340): collect_minimizers
(map.c:64-77) over sketch_model.sketch, collect_matches over the fragment's joined list (sketch_model.collect_matches), and the re-chain decision of
map.c:318-331.  The seed hits and mm_chain_dp are the CPU oracle's (oracle_binding).  Pinned against the reference by tests/test_cpu_frag_model.py."""
import numpy as np

import sketch_model as sm

SEG_SHIFT = 48
SEG_MASK = 0xFF << SEG_SHIFT                                  # MM_SEED_SEG_MASK (mmpriv.h:22-23)
MM_MAX_SEG = 255


def collect_minimizers(segs, w, k, is_hpc=False):
    """map.c:64-77 (sdust_thres = 0): every segment sketched with rid = its number, its positions shifted by the lengths of the segments before it.
    A segment of length 0 contributes nothing but keeps its number.  Returns uint64 [n, 2]"""
    out, total = [], 0
    for i, s in enumerate(segs):
        for x, y in (sm.sketch(s, w, k, is_hpc) if len(s) else []):
            out.append((x, (y + (i << 32) + (total << 1)) & 0xFFFFFFFFFFFFFFFF))
        total += len(s)
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


def n_chained_segs(u, b):
    """map.c:321-328: the segments of the best chain -- the FIRST one with the strictly largest score above 0"""
    best, best_i, best_off, off = 0, -1, -1, 0
    for i, v in enumerate(u):
        if best < int(v) >> 32:
            best, best_i, best_off = int(v) >> 32, i, off
        off += int(v) & 0xFFFFFFFF
    assert best_i >= 0, "no chain scores above 0: the reference reads u[-1] here"
    cnt = int(u[best_i]) & 0xFFFFFFFF
    seg = (b[best_off:best_off + cnt, 1].astype(np.uint64) & np.uint64(SEG_MASK))
    return 1 + int((seg[1:] != seg[:-1]).sum())


def rechain(mid_occ, max_occ, rep_len, n_segs, u, b):
    """map.c:318-331"""
    if not (max_occ > mid_occ and rep_len > 0):
        return False
    return len(u) == 0 or n_chained_segs(u, b) < n_segs


def map_frag(segs, w, k, lookup, hits, par, min_cnt, min_sc, mid_occ, max_occ, is_hpc=False, heap=True, flag=0):
    """one fragment from its segments to its chains.  lookup(key) -> (cr_off, n) into `hits`; par: the mm_chain_dp scalars (n_segs = len(segs)).
    Returns a dict: mini, first (matches, rep_len, mini_pos, u, b of the pass with mid_occ), rechained, and the final n_anchors, rep_len, mini_pos, u, b"""
    import oracle_binding as ob
    mini = collect_minimizers(segs, w, k, is_hpc)
    qlen = sum(len(s) for s in segs)

    def one_pass(occ):
        m, rep_len, mini_pos = sm.collect_matches(mini, lookup, occ)
        m = sm.match_array(m)
        a = ob.collect_seed_hits(m, hits, qlen, flag=flag, heap=heap)
        if a.shape[0]:
            u, b = ob.mm_chain_dp(par, min_cnt, min_sc, a)
        else:
            u, b = np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64)
        return {"matches": m, "rep_len": rep_len, "mini_pos": np.array(mini_pos, np.uint64), "n_anchors": a.shape[0], "anchors": a, "u": u, "b": b}

    if qlen == 0:                                             # map.c:287
        e = {"matches": sm.match_array([]), "rep_len": 0, "mini_pos": np.zeros(0, np.uint64), "n_anchors": 0, "anchors": np.zeros((0, 2), np.uint64),
             "u": np.zeros(0, np.uint64), "b": np.zeros((0, 2), np.uint64)}
        return dict(e, mini=mini, first=e, rechained=False)
    first = one_pass(mid_occ)
    again = rechain(mid_occ, max_occ, first["rep_len"], len(segs), first["u"], first["b"])
    last = one_pass(max_occ) if again else first
    return dict(last, mini=mini, first=first, rechained=again)
