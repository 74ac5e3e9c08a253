"""A literal Python restatement of mm_sketch (sketch.c:77-143) and collect_matches (map.c:90-123), written from the reference's description, for the tests of
the device sketch (csrc/sketch.hip).  Slow and plain on purpose: one loop, the reference's state, the reference's order."""
import numpy as np

ALL1 = (1 << 64) - 1


def nt4(b):
    """seq_nt4_table (sketch.c:9-26): bytes 0-3 and A C G T U in either case are nucleotides, everything else is ambiguous"""
    if b < 4:
        return b
    return {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("U"): 3}.get(b & 0xDF, 4)


def hash64(key, mask):
    key = (~key + (key << 21)) & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & mask
    key = key ^ key >> 28
    key = (key + (key << 31)) & mask
    return key


def sketch(seq, w, k, is_hpc=False):
    """mm_sketch of one read (bytes) with rid 0: a list of (x, y)"""
    assert 0 < w < 256 and 0 < k <= 28
    s = bytes(seq)
    n = len(s)
    out = []
    if n == 0:
        return out
    shift1, mask = 2 * (k - 1), (1 << 2 * k) - 1
    kmer = [0, 0]
    buf = [(ALL1, ALL1)] * w
    tq = []                                   # tiny_queue_t: run lengths, at most k kept (tq_shift when it holds more)
    l = buf_pos = min_pos = kmer_span = 0
    mn = (ALL1, ALL1)
    i = 0
    while i < n:
        c = nt4(s[i])
        info = (ALL1, ALL1)
        skip_step = False
        if c < 4:
            if is_hpc:
                skip_len = 1
                if i + 1 < n and nt4(s[i + 1]) == c:
                    skip_len = 2
                    while i + skip_len < n and nt4(s[i + skip_len]) == c:
                        skip_len += 1
                    i += skip_len - 1
                tq.append(skip_len)
                kmer_span += skip_len
                if len(tq) > k:
                    kmer_span -= tq.pop(0)
            else:
                kmer_span = l + 1 if l + 1 < k else k
            kmer[0] = (kmer[0] << 2 | c) & mask
            kmer[1] = (kmer[1] >> 2) | (3 ^ c) << shift1
            if kmer[0] == kmer[1]:
                skip_step = True                  # symmetric k-mer: `continue`
            else:
                z = 0 if kmer[0] < kmer[1] else 1
                l += 1
                if l >= k and kmer_span < 256:
                    info = (hash64(kmer[z], mask) << 8 | kmer_span, (i & 0xFFFFFFFF) << 1 & 0xFFFFFFFF | z)
        else:
            l, tq, kmer_span = 0, [], 0
        if not skip_step:
            buf[buf_pos] = info
            if l == w + k - 1 and mn[0] != ALL1:
                for j in list(range(buf_pos + 1, w)) + list(range(0, buf_pos)):
                    if mn[0] == buf[j][0] and buf[j][1] != mn[1]:
                        out.append(buf[j])
            if info[0] <= mn[0]:
                if l >= w + k and mn[0] != ALL1:
                    out.append(mn)
                mn, min_pos = info, buf_pos
            elif buf_pos == min_pos:
                if l >= w + k - 1 and mn[0] != ALL1:
                    out.append(mn)
                mn = (ALL1, mn[1])
                for j in list(range(buf_pos + 1, w)) + list(range(0, buf_pos + 1)):
                    if mn[0] >= buf[j][0]:
                        mn, min_pos = buf[j], j
                if l >= w + k - 1 and mn[0] != ALL1:
                    for j in list(range(buf_pos + 1, w)) + list(range(0, buf_pos + 1)):
                        if mn[0] == buf[j][0] and mn[1] != buf[j][1]:
                            out.append(buf[j])
            buf_pos += 1
            if buf_pos == w:
                buf_pos = 0
        i += 1
    if mn[0] != ALL1:
        out.append(mn)
    return out


def sketch_array(seq, w, k, is_hpc=False):
    m = sketch(seq, w, k, is_hpc)
    return np.array(m, dtype=np.uint64).reshape(-1, 2)


def collect_matches(mini, lookup, max_occ):
    """collect_matches for one read's minimizers (uint64 [n, 2]); lookup(key) -> (cr_off, n) with n = 0 for an absent key.
    Returns (matches as tuples (cr_off, n, q_pos, q_span, seg_tandem), rep_len, mini_pos list)"""
    rep_st = rep_en = rep_len = 0
    matches, mini_pos = [], []
    n = len(mini)
    for i in range(n):
        x, y = int(mini[i][0]), int(mini[i][1])
        q_pos, q_span = y & 0xFFFFFFFF, x & 0xFF
        cr, t = lookup(x >> 8)
        if t >= max_occ:
            en = (q_pos >> 1) + 1
            st = en - q_span
            if st > rep_en:
                rep_len += rep_en - rep_st
                rep_st, rep_en = st, en
            else:
                rep_en = en
        else:
            tandem = 0
            if i > 0 and x >> 8 == int(mini[i - 1][0]) >> 8:
                tandem = 1
            if i < n - 1 and x >> 8 == int(mini[i + 1][0]) >> 8:
                tandem = 1
            matches.append((cr if t else 0, t, q_pos, q_span, (y >> 32) << 1 | tandem))
            mini_pos.append(q_span << 32 | q_pos >> 1)
    rep_len += rep_en - rep_st
    return matches, rep_len, mini_pos


def table_lookup(keys, cr_off, n):
    """a lookup function over a key table (what mm_idx_get returns)"""
    d = {int(a): (int(b), int(c)) for a, b, c in zip(keys, cr_off, n)}
    return lambda key: d.get(int(key), (0, 0))


def sha(a):
    """SHA-256 of an array's bytes as uint8 [32]: the form the fixture (tests/golden/ref_sketch.npz) pins the reference's outputs in"""
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


MATCH_DTYPE = np.dtype([("cr_off", "<i8"), ("n", "<u4"), ("q_pos", "<u4"), ("q_span", "<u4"), ("seg_tandem", "<u4")])   # mm2c_match_t


def match_array(matches):
    """collect_matches' tuples as mm2c_match_t records"""
    return np.array(matches, dtype=MATCH_DTYPE) if matches else np.zeros(0, MATCH_DTYPE)
