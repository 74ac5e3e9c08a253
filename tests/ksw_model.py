"""A NumPy restatement of ksw_extd2_sse (ksw2_extd2_sse.c, the SSE4.1 build) that reproduces tests/golden/ref_ksw.npz byte for byte.

The function is not a textbook banded DP: its results depend on its 16-byte blocks.  What the restatement keeps:
  1. rows are computed over whole blocks: the real band [st0, en0] is padded to st = st0 / 16 * 16 .. en = (en0 + 16) / 16 * 16 - 1; u, v, x, y, x2, y2, s are persistent
     arrays by absolute t; padded cells are computed from whatever the arrays hold and real cells read them in later rows; off / off_end, mte_q, the boundary test and
     `en >= r` use the padded st / en;
  2. s[] is refreshed in chunks of 16 from the unaligned st0 (beyond en0, possibly beyond en), with sf zero behind tlen and qr zero behind qlen;
  3. wrapping int8 arithmetic in the order of __dp_code_block1/2, z clamped to mat[0], strict tests in the left form and `z > a ? 0 : 1`, `a >= 0` in the right form;
  4. the exact maximum: H[en0] first, four lanes over t < en1 each with its first strict maximum, combined in lane order with a strict <, then the scalar tail;
  4b. H of row 0 is v[0] - qe with the `qe` made in front of the swap of :78 (the unswapped q + e);
  5. the approximate maximum's three-way walk, ksw_apply_zdrop and ksw_backtrack as in ksw2.h, reach_end only with mqe + end_bonus > max.

`variant` names one deliberate mistake (VARIANTS); tests/test_cpu_ksw_model.py shows that each differs from the fixture on a planted case."""
import numpy as np

NEG_INF = -0x40000000
SCORE_ONLY, RIGHT, APPROX_MAX, APPROX_DROP, EXTZ_ONLY, REV_CIGAR = 0x01, 0x02, 0x08, 0x10, 0x40, 0x80
VARIANTS = ("real_only", "s_exact", "tie_low_t", "mte_q_en0", "off_unpadded", "right_as_left", "reach_ge", "no_clamp")


def _i8(v):
    return np.array(v).astype(np.int8)[()]


def _reset():
    return dict(max=0, zdropped=0, max_q=-1, max_t=-1, mqe=NEG_INF, mqe_t=-1, mte=NEG_INF, mte_q=-1, score=NEG_INF, n_cigar=0, reach_end=0)


def _apply_zdrop(ez, H, r, t, zdrop, e):
    if H > ez["max"]:
        ez["max"], ez["max_t"], ez["max_q"] = H, t, r - t
    elif t >= ez["max_t"] and r - t >= ez["max_q"]:
        tl, ql = t - ez["max_t"], (r - t) - ez["max_q"]
        l = abs(tl - ql)
        if zdrop >= 0 and ez["max"] - H > zdrop + l * e:
            ez["zdropped"] = 1
            return True
    return False


def _backtrack(rows, off, off_end, i, j, rev, stats=None):
    cig = []

    def push(op, n):
        if cig and cig[-1][0] == op:
            cig[-1][1] += n
        else:
            cig.append([op, n])

    state = 0
    while i >= 0 and j >= 0:
        r = i + j
        force = -1
        if i < off[r]:
            force = 2
        if i > off_end[r]:
            force = 1
        tmp = int(rows[r][1][i - rows[r][0]]) if force < 0 else 0
        if state == 0:
            state = tmp & 7
        elif not (tmp >> (state + 2) & 1):
            state = 0
        if state == 0:
            state = tmp & 7
        if force >= 0:
            state = force
            if stats is not None:
                stats.setdefault("force", set()).add(force)
        if state == 0:
            push(0, 1); i -= 1; j -= 1
        elif state == 1 or state == 3:
            push(2, 1); i -= 1
        else:
            push(1, 1); j -= 1
    if i >= 0:
        push(2, i + 1)
    if j >= 0:
        push(1, j + 1)
    if not rev:
        cig.reverse()
    return np.array([n << 4 | op for op, n in cig], np.uint32)


def extd2(query, target, mat, q, e, q2, e2, w, zdrop, end_bonus, flag, variant=None, stats=None):
    """Returns (ez as a dict of the eleven fields, cigar as uint32).  stats (a dict): gets "force", the force_state values the backtrack took, and "widths", the
    padded row widths."""
    assert variant is None or variant in VARIANTS
    qlen, tlen = len(query), len(target)
    ez = _reset()
    none = np.zeros(0, np.uint32)
    if qlen <= 0 or tlen <= 0:
        return ez, none
    mat = np.asarray(mat, np.int8)
    qe0 = q + e                                                     # `qe` of :68 is made in front of the swap of :78; H of row 0 takes it
    if q2 + e2 < q + e:
        q, q2, e, e2 = q2, q, e2, e
    with_cigar, approx, right = not flag & SCORE_ONLY, bool(flag & APPROX_MAX), bool(flag & RIGHT)
    if variant == "right_as_left":
        right = False
    if w < 0:
        w = max(tlen, qlen)
    T16 = (tlen + 15) // 16 * 16
    if -int(mat.min()) > 2 * (q + e):
        return ez, none
    long_thres = 0
    if e != e2:                                                     # C's division truncates towards zero
        n_, d_ = q2 - q, e - e2
        long_thres = (abs(n_) // abs(d_)) * (1 if (n_ < 0) == (d_ < 0) else -1) - 1
    if q2 + e2 + long_thres * e2 > q + e + long_thres * e:
        long_thres += 1
    long_diff = long_thres * (e - e2) - (q2 - q) - e2
    nqe, nqe2 = _i8(-q - e), _i8(-q2 - e2)
    q_, q2_, qe_, qe2_ = _i8(q), _i8(q2), _i8(q + e), _i8(q2 + e2)
    mch, mis = mat[0], mat[1]
    sc_n = _i8(-e2) if mat[24] == 0 else mat[24]
    zero = np.int8(0)
    u = np.full(T16, nqe, np.int8); v = u.copy(); x = u.copy(); y = u.copy()
    x2 = np.full(T16, nqe2, np.int8); y2 = x2.copy()
    s = np.zeros(T16 + 32, np.int8)
    sf = np.zeros(T16 + 32, np.uint8); sf[:tlen] = target
    qr = np.zeros(qlen + 32, np.uint8); qr[:qlen] = np.asarray(query, np.uint8)[::-1]
    H = np.full(T16, NEG_INF, np.int64) if not approx else None
    H0, last_H0_t = 0, 0
    rows, off, off_end = {}, {}, {}
    last_st = last_en = -1

    def edge(r):
        return nqe if r == 0 else _i8(-e) if r < long_thres else _i8(long_diff) if r == long_thres else _i8(-e2)

    for r in range(qlen + tlen - 1):
        st, en = max(0, r - qlen + 1, (r - w + 1) >> 1), min(tlen - 1, r, (r + w) >> 1)
        if st > en:
            ez["zdropped"] = 1
            break
        st0, en0 = st, en
        if variant != "real_only":
            st, en = st // 16 * 16, (en + 16) // 16 * 16 - 1
        if st > 0:
            if last_st <= st - 1 <= last_en:
                x1, x21, v1 = x[st - 1], x2[st - 1], v[st - 1]
            else:
                x1, x21, v1 = nqe, nqe2, nqe
        else:
            x1, x21, v1 = nqe, nqe2, edge(r)
        if en >= r:
            y[r], y2[r], u[r] = nqe, nqe2, edge(r)
        hi = en0 + 1 if variant == "s_exact" else st0 + (en0 - st0) // 16 * 16 + 16
        a_ = sf[st0:hi]; b_ = qr[qlen - 1 - r + st0:qlen - 1 - r + hi]
        sv = np.where(a_ == b_, mch, mis)
        s[st0:hi] = np.where((a_ == 4) | (b_ == 4), sc_n, sv)
        n = en + 1 - st
        if stats is not None:
            stats.setdefault("widths", set()).add(n)
        z = s[st:en + 1].copy()
        xl = np.empty(n, np.int8); xl[0] = x1; xl[1:] = x[st:en]
        vl = np.empty(n, np.int8); vl[0] = v1; vl[1:] = v[st:en]
        x2l = np.empty(n, np.int8); x2l[0] = x21; x2l[1:] = x2[st:en]
        ut = u[st:en + 1].copy()
        a = xl + vl; b = y[st:en + 1] + ut; a2 = x2l + vl; b2 = y2[st:en + 1] + ut
        if with_cigar:
            if not right:
                d = (a > z).astype(np.uint8); z = np.maximum(z, a)
                d[b > z] = 2; z = np.maximum(z, b)
                d[a2 > z] = 3; z = np.maximum(z, a2)
                d[b2 > z] = 4; z = np.maximum(z, b2)
            else:
                d = (~(z > a)).astype(np.uint8); z = np.maximum(z, a)
                d[~(z > b)] = 2; z = np.maximum(z, b)
                d[~(z > a2)] = 3; z = np.maximum(z, a2)
                d[~(z > b2)] = 4; z = np.maximum(z, b2)
        else:
            z = np.maximum(np.maximum(z, a), np.maximum(np.maximum(b, a2), b2))
        if variant != "no_clamp":
            z = np.minimum(z, mch)
        u[st:en + 1] = z - vl
        v[st:en + 1] = z - ut
        tmp = z - q_; a = a - tmp; b = b - tmp
        tmp = z - q2_; a2 = a2 - tmp; b2 = b2 - tmp
        x[st:en + 1] = np.maximum(a, zero) - qe_
        y[st:en + 1] = np.maximum(b, zero) - qe_
        x2[st:en + 1] = np.maximum(a2, zero) - qe2_
        y2[st:en + 1] = np.maximum(b2, zero) - qe2_
        if with_cigar:
            if not right:
                d |= (a > 0).astype(np.uint8) << 3 | (b > 0).astype(np.uint8) << 4 | (a2 > 0).astype(np.uint8) << 5 | (b2 > 0).astype(np.uint8) << 6
            else:
                d |= (a >= 0).astype(np.uint8) << 3 | (b >= 0).astype(np.uint8) << 4 | (a2 >= 0).astype(np.uint8) << 5 | (b2 >= 0).astype(np.uint8) << 6
            rows[r] = (st, d)
            off[r], off_end[r] = (st0, en0) if variant == "off_unpadded" else (st, en)
        if not approx:
            if r > 0:
                hen0 = H[en0 - 1] + u[en0] if en0 > 0 else H[en0] + v[en0]
                H[st0:en0] += v[st0:en0]
                H[en0] = hen0
                max_H, max_t = int(hen0), en0
                if en0 > st0:
                    seg = H[st0:en0]
                    m = int(seg.max())
                    if m > max_H:
                        idx = np.flatnonzero(seg == m)
                        if variant == "tie_low_t":
                            k = idx[0]
                        else:
                            n4 = (en0 - st0) // 4 * 4
                            sse = idx[idx < n4]
                            k = sse[np.lexsort((sse, sse & 3))[0]] if sse.size else idx[0]
                        max_H, max_t = m, st0 + int(k)
            else:
                H[0] = int(v[0]) - qe0
                max_H, max_t = int(H[0]), 0
            if en0 == tlen - 1 and H[en0] > ez["mte"]:
                ez["mte"], ez["mte_q"] = int(H[en0]), r - (en0 if variant == "mte_q_en0" else en)
            if r - st0 == qlen - 1 and H[st0] > ez["mqe"]:
                ez["mqe"], ez["mqe_t"] = int(H[st0]), st0
            if _apply_zdrop(ez, max_H, r, max_t, zdrop, e2):
                break
            if r == qlen + tlen - 2 and en0 == tlen - 1:
                ez["score"] = int(H[tlen - 1])
        else:
            if r > 0:
                if st0 <= last_H0_t <= en0 and st0 <= last_H0_t + 1 <= en0:
                    d0, d1 = int(v[last_H0_t]), int(u[last_H0_t + 1])
                    if d0 > d1:
                        H0 += d0
                    else:
                        H0 += d1; last_H0_t += 1
                elif st0 <= last_H0_t <= en0:
                    H0 += int(v[last_H0_t])
                else:
                    last_H0_t += 1; H0 += int(u[last_H0_t])
            else:
                H0, last_H0_t = int(v[0]) - qe0, 0
            if flag & APPROX_DROP and _apply_zdrop(ez, H0, r, last_H0_t, zdrop, e2):
                break
            if r == qlen + tlen - 2 and en0 == tlen - 1:
                ez["score"] = H0
        last_st, last_en = st, en
    cig = none
    if with_cigar:
        rev = bool(flag & REV_CIGAR)
        if not ez["zdropped"] and not flag & EXTZ_ONLY:
            cig = _backtrack(rows, off, off_end, tlen - 1, qlen - 1, rev, stats)
        elif not ez["zdropped"] and flag & EXTZ_ONLY and (ez["mqe"] + end_bonus >= ez["max"] if variant == "reach_ge" else ez["mqe"] + end_bonus > ez["max"]):
            ez["reach_end"] = 1
            cig = _backtrack(rows, off, off_end, ez["mqe_t"], qlen - 1, rev, stats)
        elif ez["max_t"] >= 0 and ez["max_q"] >= 0:
            cig = _backtrack(rows, off, off_end, ez["max_t"], ez["max_q"], rev, stats)
        ez["n_cigar"] = int(cig.size)
    return ez, cig


FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "n_cigar", "reach_end")


def run_case(c, score_set, variant=None, stats=None):
    mat, q, e, q2, e2 = score_set(c["sc"])
    ez, cig = extd2(c["q"], c["t"], mat, q, e, q2, e2, c["w"], c["zdrop"], c["end_bonus"], c["flag"], variant, stats)
    return np.array([ez[k] for k in FIELDS], np.int64).astype(np.int32), cig
