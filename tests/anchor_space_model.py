"""Lane-level emulation of the TRAVERSAL of mapq_gather (csrc/chain_mapq.hip) and err_walk (csrc/chain_esterr.hip): the grid of min(ceil(n_b_cap / slice), grid_cap)
workgroups, a workgroup's slices (p0 += grid * slice: the turns), the uniform search in b_off for a slice's first read, every lane's own `while (p >= be) ++r`, the
lanes' positions `lanes` apart with the memo of the hit / table entry found last, and the read-by-read path behind a refusal.  What a read IS comes from the models
of the arithmetic -- mapq_model for the moves and the join flag, esterr_model for positions and the finish -- so this file holds no second copy of those.

prepare(layout reads, b_off, ...) -> a batch; gather(batch) -> (b_out, trace); walk(batch, b) -> (first_fail per read, trace); n_match(batch, b, first_fail) is
err_finish's use of first_fail.  A trace maps a batch position to what the lane did there: "hit" / "miss" of the memo, "copy" (mapq: not a squeezed read), "k0"
(esterr: the first walk anchor), "none" (esterr: no region covers it), "tail" (mapq: behind n_b_out), "front" (in front of the batch's first anchor).

Wrong variants, for the tests only -- no kernel is ever built from them:
  memo_no_read      the memo's hit test without `memo.r == r` / `memo.tr == r`
  memo_le           `q - dst <= cnt` in place of `<`
  stale_flag        mapq: the join flag is taken from the memo as it stood before this position's search
  ignore_n_b_out    mapq: every position of [b_off[r], b_off[r + 1]) is gathered
  search_first      the search lands on the first read of a run of equal b_off (output-neutral: the lanes' own step walks over empty reads; the trace shows it)
  step_once         `if (p >= be)` in place of `while`
  stride_minus_1    p0 += (grid - 1) * slice: every slice is still taken, some twice -- both kernels are idempotent, so only the visit count B["visits"] shows it
  stride_plus_1     p0 += (grid + 1) * slice: a slice of every later turn is never taken
  front_not_skipped positions in front of b_off[0] are not skipped
  read_lags_tab     esterr: mini_pos and qlen are refreshed only at a position that searched the table and got past `k == 0`
  pred_minus_1      esterr: the walk predecessor is a[q - 1] in a reverse region too"""
import numpy as np

import esterr_model as EM
import mapq_model as MM

COPY, SQUEEZED, BAD = 0, 1, -1
FILL = np.uint64(0xfffffffffffffffd)                                           # int64 -3: what the GPU tests fill b_out with
JOIN_BIT = 1 << 40
VARIANTS = ("memo_no_read", "memo_le", "stale_flag", "ignore_n_b_out", "search_first", "step_once", "stride_minus_1", "stride_plus_1", "front_not_skipped", "read_lags_tab", "pred_minus_1")


def prepare(rs, b_off, n_b_cap=None, refused=(), opt=None):
    """rs: per read {"case", "hits" (in front of mm_join_long)}, or for err_walk alone {"case", "mid" (final regions), "a" (final a[])}; refused: read numbers whose state is BAD.
    -> the batch: everything the two kernels read, per read, from the models"""
    b_off = [int(v) for v in b_off]
    n_b_cap = b_off[-1] if n_b_cap is None else int(n_b_cap)
    base = b_off[0] // 4096 * 4096 if b_off[0] >= 8192 else 0                 # the window of b / b_out that is held: nothing of the batch lies in front of it
    B = {"b_off": b_off, "n_b_cap": n_b_cap, "base": base, "rd": [], "b": np.zeros((max(b_off[-1], n_b_cap) - base + 8, 2), np.uint64)}
    for k, R in enumerate(rs):
        c = R["case"]
        o = c["mapq"] if opt is None else opt
        a = c["a"]
        if "hits" in R:
            assert b_off[k + 1] - b_off[k] == a.shape[0] or k in refused
            B["b"][b_off[k] - base:b_off[k] - base + a.shape[0]] = a
            hits = R["hits"]
            fin, wa, _ = MM.join_mapq(hits, a, c["qlen"], o, c["rep_len"])
            order = sorted(range(hits.size), key=lambda i: (int(hits["as"][i]), i))
            squeezed = bool(o["do_join"]) and hits.size >= 2
            moves, dst = [], 0
            for i in order:
                src, cnt = int(hits["as"][i]), int(hits["cnt"][i])
                jn = int(squeezed and cnt > 0 and int(wa[dst, 1]) & JOIN_BIT != 0 and int(a[src, 1]) & JOIN_BIT == 0)
                moves.append((src, dst, cnt, jn))
                dst += cnt
        else:                                                                  # err_walk only: the final regions and the final a[] are given
            fin, wa, squeezed, moves = R["mid"], R["a"], False, []
            B["b"][b_off[k] - base:b_off[k] - base + wa.shape[0]] = wa
        tab = sorted((int(fin["as"][i]), int(fin["cnt"][i]), i, (int(fin["flags"][i]) >> 10) & 1) for i in range(fin.size) if fin["cnt"][i] > 0)
        mp = [EM.s32(int(v)) for v in c.get("mini_pos", ())]
        B["rd"].append({"state": BAD if k in refused else SQUEEZED if squeezed else COPY, "moves": moves, "n_b_out": wa.shape[0] if squeezed else a.shape[0], "a_out": wa,
                        "fin": fin, "tab": tab, "nt": BAD if k in refused else len(tab) if mp else -2, "mini": set(mp), "qlen": int(c["qlen"]), "cnt": [int(v) for v in fin["cnt"]]})
    return B


def _grid(B, slice_, grid_cap):
    return max(min((B["n_b_cap"] + slice_ - 1) // slice_, grid_cap), 1)


def _slices(B, slice_, grid, variant):
    """-> [(workgroup, p0)] in the order a workgroup takes them; slices that end in front of the held window are left out (every position of them has p < b_off[0])"""
    end = B["b_off"][-1]
    stride = (grid - 1 if variant == "stride_minus_1" and grid > 1 else grid + 1 if variant == "stride_plus_1" else grid) * slice_
    out = []
    for wg in range(grid):
        p0 = wg * slice_
        if p0 + slice_ <= B["base"]:
            p0 += (B["base"] - slice_ - p0 + stride) // stride * stride           # the first turn of this workgroup that reaches the window
        while p0 < end:
            if p0 + slice_ > B["base"]:
                out.append((wg, p0))
            p0 += stride
    return out


def _first_read(b_off, p0, variant):
    lo, hi = 0, len(b_off) - 2
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if b_off[mid] <= p0:
            lo = mid
        else:
            hi = mid - 1
    if variant == "search_first":
        while lo > 0 and b_off[lo - 1] == b_off[lo]:
            lo -= 1
    return lo


def _positions(B, slice_, lanes, grid_cap, variant, by_read):
    """the traversal shared by the two kernels: yields (workgroup, lane, read, b_off[read], q) in the order each lane meets its positions, lane by lane (lanes share
    nothing but the memo-free uniform search).  A lane's memo lives as long as its workgroup does, so the caller keys it by (workgroup, lane)."""
    b_off, grid = B["b_off"], _grid(B, slice_, grid_cap)
    n = len(b_off) - 1
    if by_read:
        for wg in range(grid):
            for r in range(wg, n, grid):
                yield ("read", wg, None, r, b_off[r], None)
        return
    end = b_off[-1]
    searched, visits = B.setdefault("searched", {}), B.setdefault("visits", {})
    searched.clear(); visits.clear()
    for wg, p0 in _slices(B, slice_, grid, variant):
        r0 = searched[p0] = _first_read(b_off, p0, variant)
        for tid in range(lanes):
            r, bo, be = r0, b_off[r0], b_off[r0 + 1]
            for k in range(slice_ // lanes):
                p = p0 + k * lanes + tid
                if p >= end:
                    break
                if variant == "step_once":
                    if p >= be:
                        r += 1; bo = be; be = b_off[r + 1]
                else:
                    while p >= be:
                        r += 1; bo = be; be = b_off[r + 1]
                visits[p] = visits.get(p, 0) + 1
                yield ("pos", wg, tid, r, bo, p - bo)


def _row(arr, base, p, sentinel):
    i = p - base
    return arr[i] if 0 <= i < arr.shape[0] else sentinel


def gather(B, variant=None, slice_=4096, lanes=256, grid_cap=2048, by_read=False):
    """mapq_gather -> (b_out of the held window, from B["base"] on, FILL where nothing was written; trace)"""
    base, rd, b = B["base"], B["rd"], B["b"]
    out = np.full_like(b, FILL)
    trace, memo = {}, {}
    wild = np.array([0xbad, 0xbad], np.uint64)

    def one(key, r, bo, q):
        D = rd[r]
        src, jn, what = q, False, "copy"
        if D["state"] == SQUEEZED:
            mr, m = memo.get(key, (-1, (0, 0, 0, 0)))
            stale = m
            in_hit = m[1] <= q and (q - m[1] <= m[2] if variant == "memo_le" else q - m[1] < m[2])
            what = "hit"
            if not ((mr == r or variant == "memo_no_read") and in_hit):
                mv = D["moves"]
                lo, hi = 0, len(mv) - 1
                while lo < hi:
                    mid = (lo + hi + 1) >> 1
                    if mv[mid][1] <= q:
                        lo = mid
                    else:
                        hi = mid - 1
                m, what = mv[lo], "miss"
                memo[key] = (r, m)
            src = m[0] + (q - m[1])
            f = stale if variant == "stale_flag" else m
            jn = f[3] != 0 and q == f[1]
        v = np.array(_row(b, base, bo + src, wild))
        if jn:
            v[1] |= np.uint64(JOIN_BIT)
        if 0 <= bo + q - base < out.shape[0]:
            out[bo + q - base] = v
        trace[bo + q] = what

    for kind, wg, tid, r, bo, q in _positions(B, slice_, lanes, grid_cap, variant, by_read):
        D = rd[r]
        if kind == "read":
            if D["state"] == BAD:
                continue
            for tid in range(lanes):
                for q in range(tid, D["n_b_out"], lanes):
                    one((wg, tid), r, bo, q)
        elif q < 0 and variant != "front_not_skipped":
            trace[bo + q] = "front"
        elif q >= D["n_b_out"] and variant != "ignore_n_b_out":
            trace[bo + q] = "tail"
        else:
            one((wg, tid), r, bo, q)
    return out, trace


def walk(B, b, variant=None, slice_=4096, lanes=256, grid_cap=2048, by_read=False):
    """err_walk on the anchors b (mapq_gather's output for the held window) -> ([first_fail per region] per read, None for a refused read; trace)"""
    base, rd = B["base"], B["rd"]
    ff = [None if D["nt"] == BAD else list(D["cnt"]) for D in rd]
    trace, memo = {}, {}
    wild = np.array([0, 0], np.uint64)

    def one(key, r, bo, q):
        D = rd[r]
        M = memo.setdefault(key, {"tr": -1, "r": -1, "m": (0, 0, 0, 0), "mini": set(), "qlen": 0})
        m = M["m"]
        in_ent = m[0] <= q and (q - m[0] <= m[1] if variant == "memo_le" else q - m[0] < m[1])
        what, searched = "hit", False
        if not ((M["tr"] == r or variant == "memo_no_read") and in_ent):
            what, searched = "miss", True
            if D["nt"] <= 0:
                trace[bo + q] = "none"
                return
            tb = D["tab"]
            lo, hi = 0, len(tb) - 1
            while lo < hi:
                mid = (lo + hi + 1) >> 1
                if tb[mid][0] <= q:
                    lo = mid
                else:
                    hi = mid - 1
            M["tr"], M["m"] = r, tb[lo]
            m = tb[lo]
            if not (m[0] <= q and q - m[0] < m[1]):
                trace[bo + q] = "none"
                return
        as_, cnt, z, rev = m
        j = q - as_
        k = cnt - 1 - j if rev else j
        if k == 0:
            trace[bo + q] = "k0"
            return
        trace[bo + q] = what
        if M["r"] != r and (searched or variant != "read_lags_tab"):
            M["r"], M["mini"], M["qlen"] = r, D["mini"], D["qlen"]
        cur = _row(b, base, bo + q, wild)
        prv = _row(b, base, bo + (q + 1 if rev and variant != "pred_minus_1" else q - 1), wild)
        x, xp = (EM.for_qpos(M["qlen"], int(v[0]), int(v[1])) for v in (cur, prv))
        if x > xp and x in M["mini"]:
            return
        if ff[r] is not None and 0 <= z < len(ff[r]):
            ff[r][z] = min(ff[r][z], k)

    for kind, wg, tid, r, bo, q in _positions(B, slice_, lanes, grid_cap, variant, by_read):
        D = rd[r]
        if kind == "read":
            if D["nt"] <= 0:
                continue
            for tid in range(lanes):
                for q in range(tid, B["b_off"][r + 1] - bo, lanes):
                    one((wg, tid), r, bo, q)
        elif q < 0 and variant != "front_not_skipped":
            trace[bo + q] = "front"
        else:
            one((wg, tid), r, bo, q)
    return ff, trace


def n_match(B, b, ff):
    """err_finish's first column: -1 without mini_pos, 0 where the first walk anchor is no minimizer, first_fail otherwise; None for a refused read"""
    out = []
    for k, D in enumerate(B["rd"]):
        if D["nt"] == BAD:
            out.append(None)
            continue
        if D["nt"] == -2:
            out.append([-1] * len(D["cnt"]))
            continue
        bo, nm = B["b_off"][k], [0] * len(D["cnt"])
        for as_, cnt, z, rev in D["tab"]:
            v = b[bo + as_ + (cnt - 1 if rev else 0) - B["base"]]
            if EM.for_qpos(D["qlen"], int(v[0]), int(v[1])) in D["mini"]:
                nm[z] = ff[k][z]
        out.append(nm)
    return out


def expected_b_out(B, rs):
    """the record: every read's final a[] at its offset, FILL everywhere else (tails behind n_b_out, the space in front of b_off[0], the guard); a refused read owns nothing"""
    out = np.full_like(B["b"], FILL)
    for k, R in enumerate(rs):
        if B["rd"][k]["state"] != BAD:
            lo = B["b_off"][k] - B["base"]
            out[lo:lo + R["a"].shape[0]] = R["a"]
    return out
