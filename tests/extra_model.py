"""A Python restatement of mm_update_extra (align.c:240-286, with mm_fix_cigar :91-167 and mm_update_cigar_eqx :169-238) and of mm_test_zdrop (:47-89) up to its
return value, written from the rules of DESIGN 3.18.  It reproduces every byte of tests/golden/ref_extra.npz (tests/test_cpu_extra_model.py).

`wrong` names one deliberately wrong variant; test_cpu_extra_model.py shows on which planted case each differs from the fixture:
  cap_no_shift        the left-alignment cap is the M word's length at entry, without what an earlier shift added
  skip_twice          after a run the I/D repair goes on two words behind the run's end instead of one
  strip_before_return the leading I/D is stripped in front of the `n_cigar <= 1` return
  mismatch_X          EQX in place writes an M word of nothing but mismatches as X
  tie_earliest        z-drop: the earliest point keeps a tie of the maximum
  drop_latest         z-drop: the latest of two equal drops wins
Three variants one might expect cannot differ from the reference on any input it is defined on, and the test says so instead of planting a case:
  no_skip             the repair tests the word at the run's end again (`k = l` without the loop's `++k`): that word is an M or an N of non-zero length, on which the
                      test either fails or finds an empty run
  nm_ignored          the test of :127 not firing on N followed by M: the run it finds is empty (a zero-length N, on which it would not be, is refused)
  merge_prev          equal neighbours merged into the previous word instead of the next: the words that come out are the same"""
import numpy as np

INT32_MIN = -(1 << 31)


class Undefined(Exception):
    """an input the reference is not defined on (the plan refuses it)"""


def fix_cigar(cig, q, t, wrong=None):
    """mm_fix_cigar.  cig: list of words, changed in place -> (cig, qshift, tshift)"""
    qshift = tshift = 0
    n = len(cig)
    lead = lambda: len(cig) > 0 and (cig[0] & 0xf) in (1, 2)
    if n <= 1:
        if wrong == "strip_before_return" and lead():
            if cig[0] & 0xf == 1:
                qshift = cig[0] >> 4
            else:
                tshift = cig[0] >> 4
            del cig[0]
        return cig, qshift, tshift
    orig = list(cig)
    toff = qoff = 0
    to_shrink = False
    for k in range(n):
        op, ln = cig[k] & 0xf, cig[k] >> 4
        if ln == 0:
            to_shrink = True
        if op == 0:
            toff += ln; qoff += ln
        elif op in (1, 2):
            if 0 < k < n - 1 and cig[k - 1] & 0xf == 0 and cig[k + 1] & 0xf == 0:
                prev_len = (orig[k - 1] if wrong == "cap_no_shift" else cig[k - 1]) >> 4
                s, off = (q, qoff) if op == 1 else (t, toff)
                l = 0
                while l < prev_len and s[off - 1 - l] == s[off + ln - 1 - l]:
                    l += 1
                if l > 0:
                    cig[k - 1] -= l << 4; cig[k + 1] += l << 4; qoff -= l; toff -= l
                if l == prev_len:
                    to_shrink = True
            if op == 1:
                qoff += ln
            else:
                toff += ln
        elif op == 3:
            toff += ln
        else:
            raise Undefined("op %d" % op)
    if qoff != len(q) or toff != len(t):
        raise Undefined("the CIGAR does not add up to the sequences")
    k = 0
    while k < n - 2:
        a, b = cig[k] & 0xf, cig[k + 1] & 0xf
        if a > 0 and a + b == 3 and not (wrong == "nm_ignored" and a == 3):
            s = [0, 0, 0]
            l = k
            while l < n:
                op = cig[l] & 0xf
                if op in (1, 2) or cig[l] >> 4 == 0:
                    if op > 2:
                        raise Undefined("a zero-length N inside a run")
                    s[op] += cig[l] >> 4
                else:
                    break
                l += 1
            if s[1] > 0 and s[2] > 0 and l - k > 2:
                cig[k] = s[1] << 4 | 1; cig[k + 1] = s[2] << 4 | 2
                for x in range(k + 2, l):
                    cig[x] &= 0xf
                to_shrink = True
            k = l - 1 if wrong == "no_skip" and l > k else l + 1 if wrong == "skip_twice" else l
        k += 1
    if to_shrink:
        sq = [w for w in cig if w >> 4 != 0]
        out = []
        if wrong == "merge_prev":
            for w in sq:
                if out and out[-1] & 0xf == w & 0xf:
                    out[-1] += w >> 4 << 4
                else:
                    out.append(w)
        else:
            for k in range(len(sq)):
                if k == len(sq) - 1 or sq[k] & 0xf != sq[k + 1] & 0xf:
                    out.append(sq[k])
                else:
                    sq[k + 1] += sq[k] >> 4 << 4
        cig[:] = out
        if not cig:
            raise Undefined("every word is empty")
    if lead():
        if cig[0] & 0xf == 1:
            qshift = cig[0] >> 4
        else:
            tshift = cig[0] >> 4
        del cig[0]
    return cig, qshift, tshift


def eqx(cig, q, t, wrong=None):
    """mm_update_cigar_eqx on the shifted sequences"""
    runs, n_M = [], 0
    qoff = toff = 0
    for w in cig:
        op, ln = w & 0xf, w >> 4
        if op == 0:
            mine = []
            l = 0
            while l < ln:
                same = q[qoff + l] == t[toff + l]
                x = l
                while x < ln and (q[qoff + x] == t[toff + x]) == same:
                    x += 1
                mine.append((x - l) << 4 | (7 if same else 8))
                l = x
            runs.append(mine); n_M += 1
            qoff += ln; toff += ln
        else:
            runs.append(None)
            if op == 1:
                qoff += ln
            else:
                toff += ln
    n_EQX = sum(len(r) for r in runs if r is not None)
    if n_EQX == n_M:
        if wrong == "mismatch_X":
            return [r[0] if r is not None else w for w, r in zip(cig, runs)]
        return [(w >> 4) << 4 | 7 if w & 0xf == 0 else w for w in cig]
    out = []
    for w, r in zip(cig, runs):
        out.extend(r if r is not None else [w])
    return out


def update_extra(q, t, cigar, mat, gq, ge, is_eqx, wrong=None):
    """-> dict(n_cigar, qshift, tshift, blen, mlen, n_ambi, dp_max, cigar uint32)"""
    q, t = [int(x) for x in q], [int(x) for x in t]
    cig = [int(w) for w in cigar]
    for w in cig:
        if w & 0xf > 3 or (w & 0xf == 3 and w >> 4 == 0):
            raise Undefined("op above 3 or an empty N")
    if gq < 0 or ge < 0:
        raise Undefined("negative gap cost")
    cig, qshift, tshift = fix_cigar(cig, q, t, wrong)
    q, t = q[qshift:], t[tshift:]
    s = mx = blen = mlen = n_ambi = 0
    qoff = toff = 0
    for w in cig:
        op, ln = w & 0xf, w >> 4
        if op == 0:
            na = nd = 0
            for l in range(ln):
                cq, ct = q[qoff + l], t[toff + l]
                if ct > 3 or cq > 3:
                    na += 1
                elif ct != cq:
                    nd += 1
                s += int(mat[ct * 5 + cq])
                if s < 0:
                    s = 0
                else:
                    mx = max(mx, s)
            blen += ln - na; mlen += ln - (na + nd); n_ambi += na
            toff += ln; qoff += ln
        elif op in (1, 2):
            seq, off = (q, qoff) if op == 1 else (t, toff)
            na = sum(1 for l in range(ln) if seq[off + l] > 3)
            blen += ln - na; n_ambi += na
            s -= gq + ge * ln
            if s < 0:
                s = 0
            if op == 1:
                qoff += ln
            else:
                toff += ln
        else:
            toff += ln
    if qoff != len(q) or toff != len(t):
        raise Undefined("the CIGAR does not add up to the sequences")
    if is_eqx:
        cig = eqx(cig, q, t, wrong)
    return dict(n_cigar=len(cig), qshift=qshift, tshift=tshift, blen=blen, mlen=mlen, n_ambi=n_ambi, dp_max=mx, cigar=np.array(cig, np.uint32))


def test_zdrop(q, t, cigar, mat, gq, ge, zdrop, zdrop_inv, max_gap, no_inv, wrong=None):
    """-> dict(max_zdrop, t0, t1, q0, q1, code, inv_cand)"""
    score, mx, max_i, max_j, i, j, max_zdrop = 0, INT32_MIN, -1, -1, 0, 0, 0
    pos = [-1, -1, -1, -1]

    def point(pi, pj):
        nonlocal mx, max_i, max_j, max_zdrop, pos
        if score < mx or (wrong == "tie_earliest" and score == mx):
            z = mx - score - abs((pi - max_i) - (pj - max_j)) * ge
            if z > max_zdrop or (wrong == "drop_latest" and z == max_zdrop and z > 0):
                max_zdrop = z
                pos = [max_i, pi, max_j, pj]
        else:
            mx, max_i, max_j = score, pi, pj
    for w in cigar:
        op, ln = int(w) & 0xf, int(w) >> 4
        if op == 0:
            for l in range(ln):
                score += int(mat[int(t[i + l]) * 5 + int(q[j + l])])
                point(i + l, j + l)
            i += ln; j += ln
        elif op in (1, 2, 3):
            score -= gq + ge * ln
            if op == 1:
                j += ln
            else:
                i += ln
            point(i, j)
    inv = int(not no_inv and max_zdrop > zdrop_inv and pos[3] - pos[2] < max_gap and pos[1] - pos[0] < max_gap)
    return dict(max_zdrop=max_zdrop, t0=pos[0], t1=pos[1], q0=pos[2], q1=pos[3], code=int(max_zdrop > zdrop), inv_cand=inv)


test_zdrop.__test__ = False


def fnv1a(b):
    h = 2166136261
    for x in b:
        h = ((h ^ int(x)) * 16777619) & 0xffffffff
    return h


def revcomp_hash(q, q0, q1):
    """the checksum the fixture holds of the bytes ksw_ll_qinit received (align.c:77-80)"""
    return fnv1a([4 if int(c) >= 4 else 3 - int(c) for c in q[q0:q1][::-1]]) if q1 > q0 else fnv1a([])
