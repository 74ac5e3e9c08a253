"""Python restatement of mm_est_err (map.c:357, esterr.c) on REG arrays: est_err() is the literal loop of esterr.c:30-64, with pow through ctypes -- the host's own
libm, the function the reference's esterr.o calls on this machine.  If it stops reproducing tests/golden/ref_esterr.npz on the "libm_*" cases only, the machine's
libm is not the fixture's (its version string is in the fixture).

counts() gives what csrc/chain_esterr.hip leaves on the device -- (n_match, n_tot) per region and avg_k per read, n_match 0 for div = -1 and -1 for a read without
mini_pos -- either by the literal loop (walk="loop") or by the parallel identity the kernels use (walk="parallel"): for a strictly increasing mini_pos, walk anchor
k >= 1 is matched iff every 1 <= k' <= k has pos_k' in mini_pos and pos_k' > pos_(k'-1).  div() is esterr.c:62 on those.

The keyword variants restate a step the "natural" way; the tests use them to show that the planted cases tell the difference:
  flank="qe"           the second flank test reads qlen - r->qe
  strand="region"      get_for_qpos turns by r->rev instead of the anchor's own strand bit
  avg="double"         avg_k = (double)sum_k / n, compared and passed to pow as a double
  avg="int"            avg_k = sum_k / n in integers
  cmp="ge"             the four flank compares with >=
  prefix="skip"        a missing anchor is skipped and the anchors behind it still count
  en="last"            en is the index of the last anchor of the walk that is in mini_pos, wherever the prefix stopped"""
import ctypes
import ctypes.util

import numpy as np

from regs_model import REG, s32

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]


def for_qpos(qlen, ax, ay, rev=None):
    x, span = s32(ay), (ay >> 32) & 0xff
    if (ax >> 63) if rev is None else rev:
        x = s32(qlen - 1 - s32(x + 1 - span))
    return x


def mini_idx(mpos, x):
    """get_mini_idx: the binary search as written (on whatever order mini_pos has)"""
    L, R = 0, len(mpos) - 1
    while L <= R:
        m = (L + R) >> 1
        y = mpos[m]
        if y < x:
            L = m + 1
        elif y > x:
            R = m - 1
        else:
            return m
    return -1


def avg_k_of(mini_pos, avg="float"):
    spans = [(int(v) >> 32) & 0xff for v in mini_pos]
    n = len(spans)
    if avg == "double":
        return sum(spans) / n
    if avg == "int":
        return F(sum(spans) // n)
    return F(sum(spans)) / F(n)


def div(n_match, n_tot, avg_k):
    """esterr.c:62"""
    if n_match <= 0:
        return F(-1)
    if n_match >= n_tot:
        return F(0)
    return F(1.0 - _libm.pow(n_match / n_tot, 1.0 / float(avg_k)))


def counts(regs, a, mini_pos, qlen, ref_len, walk="loop", flank="qs", strand="anchor", avg="float", cmp="gt", prefix="stop", en="prefix"):
    """-> (int32 [n, 2] of (n_match, n_tot), avg_k)"""
    r = np.asarray(regs, REG)
    a = np.asarray(a, np.uint64).reshape(-1, 2)
    out = np.zeros((r.size, 2), np.int32)
    n = len(mini_pos)
    if n == 0:
        out[:, 0] = -1
        return out, F(0)
    avg_k = avg_k_of(mini_pos, avg)
    mpos = [s32(int(v)) for v in mini_pos]
    gt = (lambda u, v: u >= v) if cmp == "ge" else (lambda u, v: u > v)
    num = (lambda v: v) if avg == "double" else F
    for i in range(r.size):
        cnt, as_, rev = int(r["cnt"][i]), int(r["as"][i]), (int(r["flags"][i]) >> 10) & 1
        if cnt == 0:
            continue

        def pos(k):
            ax, ay = (int(v) for v in (a[as_ + cnt - 1 - k] if rev else a[as_ + k]))
            return for_qpos(qlen, ax, ay, rev if strand == "region" else None)
        st = last = mini_idx(mpos, pos(0))
        if st < 0:
            continue
        n_match = 1
        if walk == "loop":
            k, j = 1, st + 1
            while j < n and k < cnt:
                if pos(k) == mpos[j]:
                    k, last, n_match = k + 1, j, n_match + 1
                elif prefix == "skip" and mini_idx(mpos, pos(k)) < 0:
                    k += 1
                    continue
                j += 1
        else:
            prev = pos(0)
            for k in range(1, cnt):
                x = pos(k)
                j = mini_idx(mpos, x)
                if j < 0 or not x > prev:
                    break
                n_match, last, prev = n_match + 1, j, x
        if en == "last":
            for k in range(cnt - 1, -1, -1):
                j = mini_idx(mpos, pos(k))
                if j >= 0:
                    last = j
                    break
        l_ref = s32(int(ref_len[int(r["rid"][i])]))
        n_tot = last - st + 1
        if gt(num(int(r["qs"][i])), avg_k) and gt(num(int(r["rs"][i])), avg_k):
            n_tot += 1
        q2 = s32(qlen - int(r["qe" if flank == "qe" else "qs"][i]))
        if gt(num(q2), avg_k) and gt(num(s32(l_ref - int(r["re"][i]))), avg_k):
            n_tot += 1
        out[i] = (n_match, n_tot)
    return out, avg_k


def apply(regs, cnts, avg_k):
    """the regions with div written from the counts (what mm2c_est_err_apply_host does)"""
    r = np.asarray(regs, REG).copy()
    for i in range(r.size):
        if cnts[i, 0] != -1:
            r["div"][i] = div(int(cnts[i, 0]), int(cnts[i, 1]), avg_k)
    return r


def est_err(regs, a, mini_pos, qlen, ref_len, **variant):
    """mm_est_err -> the regions with div"""
    c, avg_k = counts(regs, a, mini_pos, qlen, ref_len, **variant)
    return apply(regs, c, avg_k)
