"""NumPy / Python restatement of mm_gen_regs (hit.c:52-88) with mm_reg_set_coor (hit.c:23-38), mm_cal_fuzzy_len (hit.c:8-21), hash64 (hit.c:40-50), the literal
radix_sort_128x of ksort.h:101-151 (rs_sort's cycle-leader loop via tests/replay_model.literal, rs_insertsort) and the read hash of map.c:290-292.
`int` arithmetic wraps (two's complement), as the reference's object code does.  Test infrastructure: the fixtures come from the reference's own hit.o
(tests/golden/make_ref_regs_fixtures.py); this file is checked against them (tests/test_cpu_regs_model.py)."""
import numpy as np

import replay_model

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
REG = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0")] +
               [("flags", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("p", "<u8")])          # mm_reg1_t, minimap.h:85-100
assert REG.itemsize == 80
RS_MIN_SIZE = 64


def s32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def hash64(key):
    key = (~key + (key << 21)) & M64
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & M64
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & M64
    key ^= key >> 28
    key = (key + (key << 31)) & M64
    return key


def wang(key):
    key = (key + (~(key << 15) & M32)) & M32
    key ^= key >> 10
    key = (key + (key << 3)) & M32
    key ^= key >> 6
    key = (key + (~(key << 11) & M32)) & M32
    key ^= key >> 16
    return key


def read_hash(name, qlen_sum, seed=11):
    """map.c:290-292; name: bytes or None (`char` is signed in the reference's build)"""
    h = 0
    if name is not None and len(name) > 0:
        c = [x - 256 if x > 127 else x for x in name]
        h = c[0] & M32
        if h:
            for x in c[1:]:
                h = ((h << 5) - h + x) & M32
    h ^= (wang(qlen_sum & M32) + wang(seed & M32)) & M32
    return wang(h)


def insertsort(z, beg, end):
    for i in range(beg + 1, end):
        if z[i][0] < z[i - 1][0]:
            tmp, j = z[i], i
            while j > beg and tmp[0] < z[j - 1][0]:
                z[j] = z[j - 1]
                j -= 1
            z[j] = tmp


def rs_sort(z, beg, end, s):
    dig = [(z[i][0] >> s) & 255 for i in range(beg, end)]
    ids = replay_model.literal(dig, 256)                                     # ksort.h:126-138
    part = [z[beg + i] for i in ids]
    z[beg:end] = part
    if s:
        cnt = [0] * 256
        for d in dig:
            cnt[d] += 1
        s = s - 8 if s > 8 else 0
        at = beg
        for d in range(256):
            if cnt[d] > RS_MIN_SIZE:
                rs_sort(z, at, at + cnt[d], s)
            elif cnt[d] > 1:
                insertsort(z, at, at + cnt[d])
            at += cnt[d]


def radix_sort_128x(z):
    if len(z) <= RS_MIN_SIZE:
        insertsort(z, 0, len(z))
    else:
        rs_sort(z, 0, len(z), 56)


def keys(hash_, u, a):
    """z[] before the sort (hit.c:62-68): [(z.x, z.y)]"""
    z, k = [], 0
    for ui in (int(v) for v in u):
        h = hash64((hash64(int(a[k, 0])) + hash64(int(a[k, 1])) & M64) ^ hash_) & M32
        z.append((ui ^ h, (k << 32 | (s32(ui) & M32)) & M64))
        k += s32(ui)
    return z


def fuzzy_len(a, as_, cnt):
    """(mlen, blen) of hit.c:8-21 for the chain a[as_ : as_ + cnt]"""
    c = a[as_:as_ + cnt]
    span = ((c[:, 1] >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    xl = c[:, 0].astype(np.uint32).view(np.int32).astype(np.int64)
    yl = c[:, 1].astype(np.uint32).view(np.int32).astype(np.int64)
    wrap = lambda v: ((v + (1 << 31)) % (1 << 32)) - (1 << 31)
    tl, ql, sp = wrap(xl[1:] - xl[:-1]), wrap(yl[1:] - yl[:-1]), span[1:]
    bl = np.where(tl > ql, tl, ql)
    ml = np.where((tl > sp) & (ql > sp), sp, np.where(tl < ql, tl, ql))
    return s32(int(span[0]) + int(ml.sum())), s32(int(span[0]) + int(bl.sum()))


def gen_regs(hash_, qlen, u, a, sort=None):
    """mm_gen_regs(km, hash, qlen, n_u, u, a) -> REG[n_u].  sort: radix_sort_128x (default) or a replacement (the tests swap in a stable sort)"""
    u = np.asarray(u, np.uint64)
    a = np.asarray(a, np.uint64).reshape(-1, 2)
    r = np.zeros(u.size, REG)
    if u.size == 0:
        return r
    z = keys(int(hash_), u, a)
    (sort or radix_sort_128x)(z)
    z.reverse()                                                              # hit.c:70-71
    for i, (zx, zy) in enumerate(z):
        ri = r[i]
        cnt, k = s32(zy), zy >> 32
        ri["id"], ri["parent"] = i, -1
        ri["score"] = ri["score0"] = s32(zx >> 32)
        ri["hash"], ri["cnt"], ri["as"], ri["div"] = zx & M32, cnt, s32(k), -1.0
        x0, y0, x1, y1 = int(a[k, 0]), int(a[k, 1]), int(a[k + cnt - 1, 0]), int(a[k + cnt - 1, 1])
        q_span = y0 >> 32 & 0xff
        rev = x0 >> 63
        ri["flags"] = rev << 10
        ri["rid"] = s32((x0 << 1 & M64) >> 33)
        ri["rs"] = s32(x0 + 1 - q_span) if s32(x0 + 1) > q_span else 0
        ri["re"] = s32(x1 + 1)
        if not rev:
            ri["qs"], ri["qe"] = s32(y0 + 1 - q_span), s32(y1 + 1)
        else:
            ri["qs"], ri["qe"] = s32(qlen - s32(y1 + 1)), s32(qlen - s32(y0 + 1 - q_span))
        ri["mlen"], ri["blen"] = fuzzy_len(a, k, cnt)
    return r


def stable_sort(z):
    z.sort(key=lambda e: e[0])


def n_tie_reads(cases):
    """reads in which two chains have the same key z.x"""
    n = 0
    for c in cases:
        zx = [e[0] for e in keys(int(c["hash"]), c["u"], np.asarray(c["a"], np.uint64).reshape(-1, 2))] if len(c["u"]) else []
        n += len(set(zx)) != len(zx)
    return n
