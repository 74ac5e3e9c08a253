"""Seeded tasks for the base-alignment plan (ksw_extd2_sse, ksw2_extd2_sse.c): the inputs behind tests/golden/ref_ksw.npz.  The fixture stores outputs only;
cases() makes the same inputs again, for the generator, the model's test and the GPU tests.  A case is one call of the function: query and target as codes 0..4,
a score set, w, zdrop, end_bonus and flag."""
import numpy as np

SCORE_ONLY, RIGHT, GENERIC_SC, APPROX_MAX, APPROX_DROP, EXTZ_ONLY, REV_CIGAR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x40, 0x80
SUPPORTED = SCORE_ONLY | RIGHT | APPROX_MAX | APPROX_DROP | EXTZ_ONLY | REV_CIGAR
FLAG_BITS = (SCORE_ONLY, RIGHT, APPROX_MAX, APPROX_DROP, EXTZ_ONLY, REV_CIGAR)
ALL_FLAGS = tuple(sum(b for k, b in enumerate(FLAG_BITS) if m >> k & 1) for m in range(64))

# (a, b, q, e, q2, e2, sc_ambi)
SCORES = {
    "ont": (2, 4, 4, 2, 24, 1, 1),
    "asm5": (1, 19, 39, 3, 81, 1, 1),
    "asm10": (1, 9, 16, 2, 41, 1, 1),
    "asm20": (1, 4, 6, 2, 26, 1, 1),
    "sr": (2, 8, 12, 2, 24, 1, 1),
    "swap": (2, 4, 24, 1, 4, 2, 1),       # q2 + e2 < q + e: the function swaps the pieces
    "eeq": (2, 4, 4, 2, 8, 2, 1),         # e == e2: long_thres 0
    "amb0": (2, 4, 4, 2, 24, 1, 0),       # mat[24] == 0: N scores -e2
    "mis12": (2, 12, 4, 2, 24, 1, 1),     # a mismatch at the limit of :100 (12 = 2 (q + e)): an edge cell can prefer a gap that comes out of a padded cell
    "ret": (2, 20, 4, 2, 24, 1, 1),       # -min_sc > 2 (q + e): the early return
}


def gen_mat(a, b, sc_ambi):
    """ksw_gen_simple_mat (align.c:9-22) for m = 5."""
    a, b, sc_ambi = abs(a), -abs(b), -abs(sc_ambi)
    m = np.full((5, 5), b, np.int8)
    m[np.arange(4), np.arange(4)] = a
    m[:, 4] = sc_ambi
    m[4, :] = sc_ambi
    return m.reshape(-1)


def score_set(name):
    a, b, q, e, q2, e2, amb = SCORES[name]
    return gen_mat(a, b, amb), q, e, q2, e2


def _mutate(rng, s, div):
    out = []
    for c in s:
        r = rng.random()
        if r < div / 3:
            continue
        if r < 2 * div / 3:
            out.append(int(rng.integers(0, 4)))
        if r < div:
            out.append(int((c + 1 + rng.integers(0, 3)) % 4))
        else:
            out.append(int(c))
    return np.array(out if out else [0], np.uint8)


def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _pair(rng, ql, tl, div=0.1):
    """A query of ql and a target of tl bases that share a diverged common part."""
    base = _rand(rng, max(ql, tl))
    q = _mutate(rng, base, div)
    q = np.concatenate([q, _rand(rng, ql)])[:ql]
    t = np.concatenate([base, _rand(rng, tl)])[:tl]
    return q.astype(np.uint8), t.astype(np.uint8)


def planted():
    rng = np.random.default_rng(20261020)
    cs = []

    def add(name, q, t, sc="ont", w=50, zdrop=400, end_bonus=-1, flags=ALL_FLAGS):
        q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
        for f in flags:
            cs.append(dict(name="%s/f%02x" % (name, f), q=q, t=t, sc=sc, w=w, zdrop=zdrop, end_bonus=end_bonus, flag=f))

    # lengths on either side of the 16-byte blocks, equal, mixed, and lopsided
    edges = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
    for n in edges:
        q, t = _pair(rng, n, n)
        add("len_%d_%d" % (n, n), q, t)
    for ql, tl in ((1, 17), (17, 1), (15, 33), (33, 15), (16, 64), (64, 16), (31, 65), (65, 32), (1, 1), (2, 1), (1, 2)):
        q, t = _pair(rng, ql, tl)
        add("full_%d_%d" % (ql, tl), q, t, w=-1)
    for n in (127, 128, 129, 255, 256, 257):
        q, t = _pair(rng, n, n + (n % 3) - 1)
        add("len_%d" % n, q, t, w=40)
    for ql, tl in ((128, 17), (16, 129), (257, 33), (31, 256)):
        q, t = _pair(rng, ql, tl)
        add("len_%d_%d" % (ql, tl), q, t, w=-1)
    # bands
    for w in (-1, 0, 1, 2, 3, 15, 16, 17, 32, 100):
        q, t = _pair(rng, 48, 50, 0.15)
        add("w_%d" % w, q, t, w=w)
    for w in (0, 1, 2, 3):
        q, t = _pair(rng, 40, 40, 0.2)
        add("w_%d_sq" % w, q, t, w=w, zdrop=10)
    for ql, tl, w in ((20, 60, 5), (60, 20, 5), (30, 64, 16), (64, 30, 17), (10, 48, 2), (33, 80, 15)):
        q, t = _pair(rng, ql, tl)
        add("band_closes_%d_%d_w%d" % (ql, tl, w), q, t, w=w)
    for tl, ql, w in ((32, 40, 3), (48, 64, 2), (64, 70, 5), (16, 30, 1), (32, 33, 0)):     # tlen a multiple of 16, the last rows have st0 > tlen - 16
        q, t = _pair(rng, ql, tl)
        add("tlen16_%d_%d_w%d" % (ql, tl, w), q, t, w=w)
    for ql, tl, w in ((40, 31, 30), (40, 32, 31), (47, 48, 32), (50, 33, 29)):               # en0 at 15 / 16 (mod 16), st0 across a block
        q, t = _pair(rng, ql, tl)
        add("en0_%d_%d_w%d" % (ql, tl, w), q, t, w=w)
    # scores and bases
    for sc in ("ont", "asm5", "asm10", "asm20", "sr", "swap", "eeq", "amb0", "ret"):
        q, t = _pair(rng, 60, 62, 0.12)
        add("sc_%s" % sc, q, t, sc=sc, w=30, zdrop=200)
        q, t = _pair(rng, 50, 50, 0.1)
        q[7] = 4; t[30] = 4; t[31] = 4; q[31] = 4
        add("sc_%s_N" % sc, q, t, sc=sc, w=20, zdrop=100)
    for n in (18, 19, 20, 21, 22):                                  # rows below, at and above long_thres of map-ont (19)
        q, t = _pair(rng, n, n, 0.05)
        add("long_thres_%d" % n, q, t, w=-1)
    # gaps
    base = _rand(rng, 70)
    ins = _rand(rng, 60)
    add("ins60", np.concatenate([base[:35], ins, base[35:]]), base, w=80)
    add("del60", base, np.concatenate([base[:35], ins, base[35:]]), w=80)
    add("ins60_asm20", np.concatenate([base[:35], ins, base[35:]]), base, sc="asm20", w=80)
    add("del60_swap", base, np.concatenate([base[:35], ins, base[35:]]), sc="swap", w=80)
    add("lead_ins", np.concatenate([_rand(rng, 9), base[:40]]), base[:40], w=20)
    add("lead_del", base[:40], np.concatenate([_rand(rng, 9), base[:40]]), w=20)
    add("trail_ins", np.concatenate([base[:40], _rand(rng, 9)]), base[:40], w=20)
    # equal H in different lanes: homopolymers and tandem repeats, with an indel inside
    add("homo", np.zeros(40, np.uint8), np.zeros(37, np.uint8), w=10, zdrop=20)
    add("homo_w2", np.zeros(33, np.uint8), np.zeros(35, np.uint8), w=2, zdrop=5)
    add("tandem2", np.tile([0, 1], 24), np.tile([0, 1], 21), w=12, zdrop=30)
    add("tandem3", np.tile([0, 1, 2], 15), np.tile([0, 1, 2], 17), w=8, zdrop=10)
    add("tandem_mis", np.tile([0, 1], 20), np.tile([1, 0], 20), w=6, zdrop=8)
    add("all_mis", np.zeros(30, np.uint8), np.ones(30, np.uint8), w=10, zdrop=15)
    add("all_mis_noz", np.zeros(24, np.uint8), np.ones(20, np.uint8), w=-1, zdrop=-1)
    # z-drop
    for z in (-1, 0, 5, 20, 60):
        q, t = _pair(rng, 60, 60, 0.05)
        q[30:] = (q[30:] + 1 + (np.arange(30) % 3)) % 4          # the second half does not match
        add("zdrop_%d_diag" % z, q, t, w=30, zdrop=z)
        q, t = _pair(rng, 64, 50, 0.05)
        q = np.concatenate([q[:25], _rand(rng, 14), q[25:50]])
        add("zdrop_%d_off" % z, q, t, w=30, zdrop=z)
    # EXTZ_ONLY: identical sequences end with mqe == max
    q = _rand(rng, 30)
    for eb in (-1, 0, 1, 5):
        add("extz_equal_eb%d" % eb, q, q, w=10, end_bonus=eb)
        add("extz_tail_eb%d" % eb, q, np.concatenate([q, _rand(rng, 12)]), w=20, end_bonus=eb)
    q, t = _pair(rng, 50, 58, 0.1)
    q[42:] = (q[42:] + 2) % 4
    for eb in (0, 3, 10, 20):
        add("extz_clip_eb%d" % eb, q, t, w=20, end_bonus=eb, zdrop=100)
    # an indel longer than the band is wide: the path runs along the band's edge (it stays inside the padded blocks)
    base = _rand(rng, 60)
    add("band_edge_ins", np.concatenate([base[:20], _rand(rng, 12), base[20:]]), base, w=3)
    add("band_edge_del", base, np.concatenate([base[:20], _rand(rng, 12), base[20:]]), w=3)
    add("band_edge_ins_w1", np.concatenate([base[:30], _rand(rng, 5), base[30:40]]), base[:40], w=1)
    add("band_edge_del_w1", base[:40], np.concatenate([base[:30], _rand(rng, 5), base[30:40]]), w=1)
    add("band_edge_w0", base[:33], base[1:34], w=0)
    # backtracks that leave the padded row: on its right (i > off_end[r]: force_state 1) under map-ont scores, on its left (i < off[r]: force_state 2; seed 156
    # takes both) under a mismatch of 12, where a real cell at the band's left edge prefers the deletion out of the padded cell beside it and the walk goes on
    # through padded cells to the block's first byte.  Found by running seeds of narrow-band tasks through tests/ksw_model.py; test_cpu_ksw_model.py asserts the states
    for seed in (16, 17):
        r2 = np.random.default_rng(seed)
        ql = int(r2.integers(36, 90)); tl = max(20, ql + int(r2.integers(-6, 7))); w = int(r2.integers(1, 5)); div = float(r2.choice([0.1, 0.25, 0.4]))
        q, t = _pair(r2, ql, tl, div)
        add("leave_band_right_%d" % seed, q, t, w=w, end_bonus=5)
    for seed in (156, 575, 1054):
        r2 = np.random.default_rng(seed)
        ql = int(r2.integers(40, 100)); tl = ql - int(r2.integers(0, 12)); w = int(r2.integers(1, 6)); div = float(r2.choice([0.1, 0.25, 0.4]))
        q, t = _pair(r2, ql, tl, div)
        add("leave_band_left_%d" % seed, q, t, sc="mis12", w=w, end_bonus=5)
    # rows whose maximum H is reached at two t that lie in different lanes of the four-lane scan of :333-352, with a z-drop small enough to decide on which of them
    # the maximum was taken: found among the random tasks below (the only inputs on which the lowest-t tie rule showed), kept here under their own names
    rnd = randoms()
    for k in (141, 725, 1419, 1947):
        c = rnd[k]
        add("tie_lanes_%d" % k, c["q"], c["t"], sc=c["sc"], w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flags=tuple(dict.fromkeys((c["flag"], c["flag"] & ~RIGHT, 0, EXTZ_ONLY))))
    return cs


def limits():
    """One task of about 2 000 x 2 100 at w = 500, and one at each edge of the kernel's size classes: the array image fits LDS up to KSW_LDS_T16 = 2 304 padded target
    bases with a query of at most KSW_LDS_Q = 2 304 (csrc/ksw_extd2.h), beyond either it lies in the plan's scratch; a row is walked in chunks of 64 lanes."""
    rng = np.random.default_rng(77)
    cs = []

    def add(name, ql, tl, w, flag, div=0.1, zdrop=400):
        q, t = _pair(rng, ql, tl, div)
        cs.append(dict(name=name, q=q, t=t, sc="ont", w=w, zdrop=zdrop, end_bonus=-1, flag=flag))

    add("big_2000_2100_w500", 2000, 2100, 500, 0)
    add("big_2000_2100_w500_approx", 2000, 2100, 500, APPROX_MAX)
    add("lds_last_t2304", 300, 2304, 40, 0)                      # the last target length with the image in LDS
    add("scratch_first_t2305", 300, 2305, 40, 0)                  # the first with the image in scratch
    add("lds_last_q2304", 2304, 200, 30, EXTZ_ONLY | RIGHT | REV_CIGAR)
    add("scratch_first_q2305", 2305, 200, 30, EXTZ_ONLY | RIGHT | REV_CIGAR)
    add("lds_last_both_2304", 2304, 2304, 30, 0)                  # both LDS limits at once: the image fills the kernel's 30 000 bytes to the last one
    for k, f in enumerate((0, APPROX_MAX, EXTZ_ONLY | RIGHT | REV_CIGAR)):   # p of 4.56 MB each: beyond the plan's default slots of 4 MiB (-x ava-*: bw = 2 000)
        add("p_over_4mib_%d" % k, 1500, 1500 - 7 * k, 2000, f)
    add("row_64_lanes", 70, 70, 125, 0)                           # padded rows of up to 64 and 80 cells: exactly one chunk of 64 lanes, and one block more
    add("row_65_lanes", 90, 90, 127, REV_CIGAR)                   # ... 64, 80 and 96 cells: the second chunk a quarter and half full
    add("row_129_lanes", 140, 140, 257, APPROX_MAX | APPROX_DROP, zdrop=50)   # 128 and 144 cells: two chunks, and a third of one block
    return cs


def randoms(n=2000):
    rng = np.random.default_rng(4242)
    names = [k for k in SCORES if k not in ("ret", "mis12")]
    cs = []
    for i in range(n):
        ql, tl = int(rng.integers(1, 201)), int(rng.integers(1, 201))
        if rng.random() < 0.6:
            tl = max(1, min(200, ql + int(rng.integers(-8, 9))))
        q, t = _pair(rng, ql, tl, float(rng.choice([0.02, 0.1, 0.25])))
        if rng.random() < 0.1:
            q[rng.integers(0, ql)] = 4
        cs.append(dict(name="rnd%04d" % i, q=q, t=t, sc=str(rng.choice(names)), w=int(rng.choice([-1, 0, 1, 2, 3, 5, 10, 17, 50, 300])),
                       zdrop=int(rng.choice([-1, 0, 5, 20, 50, 400])), end_bonus=int(rng.choice([-1, 0, 1, 5, 10])), flag=int(ALL_FLAGS[rng.integers(0, 64)])))
    return cs


_CACHE = {}


def cases():
    if "c" not in _CACHE:
        _CACHE["c"] = planted() + limits() + randoms()
    return _CACHE["c"]
