"""The cases of the chains-to-regions tests (mm_gen_regs, hit.c:52-88): seeded, deterministic, made again wherever they are needed; tests/golden/ref_regs.npz holds what
the reference's own hit.o makes of them (tests/golden/make_ref_regs_fixtures.py).  cases() -> [{"name", "hash", "qlen", "u": uint64[n_u], "a": uint64[n_b, 2]}];
batch(cases) -> the CSR arrays the device entries take.

The boundaries of the implementation (csrc/chain_regs.h, chain_regs.hip) the cases stand on both sides of:
  FILL_ROW   = 64    chain anchors of one row (the segmented scan inside the wave),
  FILL_GROUP = 256   chain anchors a wave has in flight at a time (four rows),
  FILL_SLICE = 1024  chain anchors of one wave (a chain inside a slice is stored, one that crosses slices is added atomically; the slice's chains -- at most one per
                     anchor -- are looked up in an LDS table, and only counts that break the preconditions can make them more: tests/test_gpu_regs.py plants those),
  FILL_BLOCK = 4096  chain anchors of one workgroup,
  RS_MIN     = 64    chains: up to here klib's sort is the stable insertion sort, above it the cycle-leader distribution (the replay),
  TS_MAX     = 4096  chains: up to here the replay keeps its arrangement in LDS, above it in memory (the largest class)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FILL_ROW, FILL_GROUP, FILL_SLICE, FILL_BLOCK, RS_MIN, TS_MAX = 64, 256, 1024, 4096, 64, 4096
TIE_HASH = 0x5bd1e995                                                        # the read hash the planted equal keys are searched under
M64 = (1 << 64) - 1


def hash64_np(key):
    key = key.astype(np.uint64)
    with np.errstate(over="ignore"):
        key = ~key + (key << np.uint64(21))
        key = key ^ key >> np.uint64(24)
        key = key + (key << np.uint64(3)) + (key << np.uint64(8))
        key = key ^ key >> np.uint64(14)
        key = key + (key << np.uint64(2)) + (key << np.uint64(4))
        key = key ^ key >> np.uint64(28)
        key = key + (key << np.uint64(31))
    return key


def h_of(x, y, hash_):
    with np.errstate(over="ignore"):
        return (hash64_np((hash64_np(x) + hash64_np(y)) ^ np.uint64(hash_)) & np.uint64(0xffffffff)).astype(np.uint32)


def anchor(rid, pos, qpos, rev=0, span=15):
    return ((rev << 63 | rid << 32 | (pos & 0xffffffff)) & M64, (span << 32 | (qpos & 0xffffffff)) & M64)


def chain(rng, cnt, rid=0, rev=0, pos=1000, qpos=100, span=15, first=None):
    """cnt anchors, x and q ascending by steps that take every branch of hit.c:15-19 now and then; first: the (x, y) of the first anchor"""
    dx = rng.integers(1, 40, cnt); dy = rng.integers(1, 40, cnt)
    same = rng.random(cnt) < 0.5
    dy[same] = dx[same]
    xs = pos + np.cumsum(dx); ys = qpos + np.cumsum(dy)
    a = np.zeros((cnt, 2), np.uint64)
    a[:, 0] = (np.uint64(rev) << np.uint64(63)) | (np.uint64(rid) << np.uint64(32)) | xs.astype(np.uint64)
    a[:, 1] = (np.uint64(span) << np.uint64(32)) | ys.astype(np.uint64)
    if first is not None:
        a[0] = first
    return a


def read(rng, name, cnts, scores=None, hash_=None, qlen=None, firsts=None, **kw):
    cnts = [int(c) for c in cnts]
    if scores is None:
        scores = [int(s) for s in rng.integers(40, 60000, len(cnts))]
    parts = [chain(rng, c, rid=int(rng.integers(0, 5)), rev=int(rng.integers(0, 2)), pos=int(rng.integers(100, 1 << 20)), qpos=int(rng.integers(20, 5000)),
                   first=None if firsts is None else firsts[i], **kw) for i, c in enumerate(cnts)]
    u = np.array([(s & 0xffffffff) << 32 | c for s, c in zip(scores, cnts)], np.uint64)
    a = np.concatenate(parts) if parts else np.zeros((0, 2), np.uint64)
    return {"name": name, "hash": int(rng.integers(0, 1 << 32)) if hash_ is None else hash_, "qlen": int(rng.integers(6000, 50000)) if qlen is None else qlen, "u": u, "a": a}


def equal_h_pairs(n_cand=1 << 18, seed=77):
    """a birthday search over n_cand candidate first anchors: (pairs with equal h, and per byte j of the low word pairs whose h differ in byte j only), under TIE_HASH"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 4, n_cand).astype(np.uint64) << np.uint64(32)) | rng.integers(1000, 1 << 30, n_cand).astype(np.uint64)
    y = (np.uint64(15) << np.uint64(32)) | rng.integers(100, 1 << 20, n_cand).astype(np.uint64)
    h = h_of(x, y, TIE_HASH)

    def collide(key):
        order = np.argsort(key, kind="stable")
        ks = key[order]
        at = np.nonzero(ks[1:] == ks[:-1])[0]
        return [(int(order[i]), int(order[i + 1])) for i in at]
    full = [(i, j) for i, j in collide(h) if (x[i], y[i]) != (x[j], y[j])]
    near = []
    for byte in range(4):
        m = np.uint32(~(0xff << 8 * byte) & 0xffffffff)
        near.append([(i, j) for i, j in collide(h & m) if h[i] != h[j]])
    pt = lambda i: (int(x[i]), int(y[i]))
    return [(pt(i), pt(j)) for i, j in full], [[(pt(i), pt(j)) for i, j in n] for n in near]


def tie_read(rng, name, n_chains, pairs, near, n_pairs=3):
    """a read of n_chains short chains with planted equal keys: pairs (two first anchors of equal h, same u), triples (a pair and a chain that repeats one of its first
    anchors) and, for each of the 8 bytes of the key, two keys that differ in that byte only; the low scores keep the top bytes of all keys equal"""
    cnts = [int(c) for c in rng.integers(1, 4, n_chains)]
    scores = [int(s) for s in rng.integers(40, 3000, n_chains)]
    firsts = [None] * n_chains
    slots = [int(s) for s in rng.permutation(n_chains)]
    take = lambda k: [slots.pop() for _ in range(k)]
    for k in range(n_pairs):                                                 # pairs
        p, q = pairs[k % len(pairs)]
        i, j = take(2)
        firsts[i], firsts[j] = p, q
        cnts[j], scores[j] = cnts[i], scores[i] = 2, 100 + k
    p, q = pairs[n_pairs % len(pairs)]                                       # a triple
    i, j, l = take(3)
    firsts[i], firsts[j], firsts[l] = p, q, p
    cnts[i] = cnts[j] = cnts[l] = 3
    scores[i] = scores[j] = scores[l] = 777
    for byte in range(8):                                                    # equal but for one byte
        i, j = take(2)
        cnts[i] = cnts[j] = 2
        if byte < 4:
            firsts[i], firsts[j] = near[byte][0]
            scores[i] = scores[j] = 900 + byte
        else:
            firsts[i] = firsts[j] = pairs[(n_pairs + 1) % len(pairs)][0]
            scores[i], scores[j] = 1000 + byte, (1000 + byte) ^ (0x5a << 8 * (byte - 4))
    return read(rng, name, cnts, scores, hash_=TIE_HASH, firsts=firsts)


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(20261019)
    out = []
    # real chains: the reference's own mm_map_frag (ref_frag.npz) and the oracle's mm_chain_dp on the reference host's anchor lists (ref_testdata_anchors.npz)
    F = np.load(os.path.join(GOLDEN, "ref_frag.npz"))
    uo, bo, fo, so = F["heap_u_off"], F["heap_b_off"], F["frag_off"], F["seq_off"]
    picked = [g for g in range(uo.size - 1) if uo[g + 1] > uo[g]]
    for g in sorted(picked, key=lambda g: uo[g] - uo[g + 1])[:6] + picked[:4]:
        out.append({"name": f"frag{g}", "hash": int(rng.integers(0, 1 << 32)), "qlen": int(so[fo[g + 1]] - so[fo[g]]), "u": F["heap_u"][uo[g]:uo[g + 1]].copy(),
                    "a": F["heap_b"][bo[g]:bo[g + 1]].copy()})
    T = np.load(os.path.join(GOLDEN, "ref_testdata_anchors.npz"))
    for k in range(int(T["n_calls"])):
        out.append({"name": f"testdata{k}", "hash": int(rng.integers(0, 1 << 32)), "qlen": 20000, "u": T[f"c{k}_u"].copy(), "a": T[f"c{k}_b"].copy()})
    # small counts
    out.append(read(rng, "no_chains", []))
    out.append(read(rng, "one_chain", [17]))
    out.append(read(rng, "cnt1", [1]))
    out.append(read(rng, "cnt1_among", [5, 1, 1, 7, 1]))
    # slice and reduction boundaries of the fill pass
    out.append(read(rng, "rows", [2, FILL_ROW - 1, FILL_ROW, FILL_ROW + 1, 2 * FILL_ROW, 2 * FILL_ROW + 1]))
    out.append(read(rng, "row_groups", [FILL_GROUP, FILL_GROUP + 1, FILL_GROUP - 1, 1, FILL_GROUP - 1, 2]))
    out.append(read(rng, "slice_exact", [FILL_SLICE, FILL_SLICE + 1, FILL_SLICE - 1, 3]))
    out.append(read(rng, "slice_minus", [FILL_SLICE - 1, 2, FILL_SLICE - 1, 1, 1, FILL_SLICE]))
    out.append(read(rng, "block", [FILL_BLOCK, FILL_BLOCK + 1, FILL_BLOCK - 1, 1]))
    out.append(read(rng, "long_chain", [20011]))
    out.append(read(rng, "long_between", [3, 20000, 5]))
    # sort sizes without equal keys
    out.append(read(rng, "sort64", rng.integers(1, 5, RS_MIN)))
    out.append(read(rng, "sort65", rng.integers(1, 5, RS_MIN + 1)))
    # planted equal keys: the stable path, the replay (LDS), and each side of the replay's LDS capacity
    pairs, near = equal_h_pairs()
    assert len(pairs) >= 2 and all(len(n) >= 1 for n in near)
    for n in (RS_MIN, RS_MIN + 1, 300, TS_MAX, TS_MAX + 1):
        out.append(tie_read(rng, f"ties{n}", n, pairs, near))
    # coordinates
    span = 15
    for rev in (0, 1):
        for d in (-1, 0, 1):                                                 # (int32_t)x + 1 below, at and above q_span: rs clamps at 0
            a = chain(rng, 6, rid=2, rev=rev, pos=500, qpos=300, span=span)
            a[0] = anchor(2, span - 1 + d, 30, rev, span)
            out.append({"name": f"rs_clamp_rev{rev}_{d}", "hash": int(rng.integers(0, 1 << 32)), "qlen": 4000, "u": np.array([70 << 32 | 6], np.uint64), "a": a})
    a = np.array([anchor(1, 0x7ffffff0, 100), anchor(1, 0x7fffffff, 110), anchor(1, 0x80000000, 125), anchor(1, 0x80000040, 140),     # the low word crosses 2^31 inside a chain
                  anchor(3, 0x10, 50), anchor(3, 0xfffffff0, 70), anchor(3, 0xfffffff8, 90)], np.uint64)                             # tl = -32: negative without overflow
    out.append({"name": "low_word_sign", "hash": 12345, "qlen": 9000, "u": np.array([90 << 32 | 4, 80 << 32 | 3], np.uint64), "a": a})
    a = chain(rng, 5, rid=0x7fffffff, rev=1, pos=100, qpos=100)
    b = chain(rng, 5, rid=0x7fffffff, rev=0, pos=100, qpos=100)
    out.append({"name": "rid_all_ones", "hash": 99, "qlen": 3000, "u": np.array([55 << 32 | 5, 54 << 32 | 5], np.uint64), "a": np.concatenate([a, b])})
    # fuzzy-length branches: tl above / equal to / below ql, each of tl and ql at span and span + 1
    steps = [(20, 10), (10, 10), (10, 20), (span, span), (span + 1, span + 1), (span, span + 1), (span + 1, span), (span + 1, 40), (40, span + 1), (span, 40), (40, span), (1, 1)]
    xs, ys = np.cumsum([1000] + [s[0] for s in steps]), np.cumsum([200] + [s[1] for s in steps])
    a = np.array([anchor(0, int(x), int(y), 0, span) for x, y in zip(xs, ys)], np.uint64)
    out.append({"name": "fuzzy_branches", "hash": 4242, "qlen": 2000, "u": np.array([300 << 32 | len(xs)], np.uint64), "a": a})
    # the read hash at its ends
    for hv in (0, 0xffffffff):
        out.append(read(rng, f"hash_{hv:x}", [4, 9, 2, 30], hash_=hv))
    for c in out:
        c["u"] = np.ascontiguousarray(c["u"], np.uint64)
        c["a"] = np.ascontiguousarray(c["a"], np.uint64).reshape(-1, 2)
        assert int((c["u"] & np.uint64(0xffffffff)).sum()) == c["a"].shape[0], c["name"]
    _CASES = out
    return out


HASH_CASES = [(None, 0, 11), (b"", 1, 11), (b"read1", 1000, 11), (b"read1", 1000, 0), (b"r", 150, 11), (b"m64011_190830_220126/1/ccs", 15000, 11), (b"\xff\x80high", 300, 11),
              (b"pair/1", 300, 42), (b"a" * 200, 2147483647, -1), (None, 250, 11)]


def batch(cs):
    """(u_off, u, b_off, b, qlen, hash) of the cases as one batch"""
    u_off = np.zeros(len(cs) + 1, np.int64); b_off = np.zeros(len(cs) + 1, np.int64)
    u_off[1:] = np.cumsum([c["u"].size for c in cs]); b_off[1:] = np.cumsum([c["a"].shape[0] for c in cs])
    u = np.concatenate([c["u"] for c in cs] + [np.zeros(0, np.uint64)])
    b = np.concatenate([c["a"] for c in cs] + [np.zeros((0, 2), np.uint64)])
    return u_off, u, b_off, b, np.array([c["qlen"] for c in cs], np.int32), np.array([c["hash"] for c in cs], np.uint32)
