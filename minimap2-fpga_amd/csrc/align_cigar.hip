// align_cigar.hip -- ksw results to aligned regions: the rest of mm_align1 (align.c:698-705, 736-764, 772-783).
//   cig_second_count / cig_second_emit   one wave per region, persistent grid, 64 items a step: the list of second passes (:736-737); under sr the ungapped
//                                        item's z-drop test as a prefix sum and a prefix maximum over the wave, 64 bases a step with a carry
//   cig_second_scan                      one workgroup: second-pass tasks and their CIGAR slots of every region -> offsets
//   cig_cut     one wave per region: the first dropped gap item (a ballot), dp_score, the extensions' scalars, j (a ballot scan backwards over the anchors), the
//               number of output words (sum of n_cigar less the merging boundaries) and the length check of :284
//   cig_scan    one workgroup: output words -> offsets, what leaves a capacity, the dense list of mm2c_extra_task_t
//   cig_gather  streaming over the words of the used items, a region taken by one workgroup of 256 lanes in pieces: mm_append_cigar with its merge (:303-306)
// Placement comes from the scans; every store is a plain vector store; the only atomics are the adds of the refusal counters; no floating point.
#include "align_cigar.h"
#include "wave_ops.h"
#include <limits.h>

namespace mm2c {
namespace {

constexpr int KSW_EZ_APPROX_MAX = 0x08;

__device__ inline int64_t slot_of(int64_t s, int shift) { const int64_t c = (s >> shift) + 16; return s < c ? s : c; }   // a task's CIGAR slot, the rule of the first list

// the same over a workgroup of 256 lanes; sw: 4 words of LDS
__device__ inline int b_incl_sum(int v, int lane, int wv, int *sw)
{
	v = wave_incl_sum(v, lane);
	if (lane == 63) sw[wv] = v;
	__syncthreads();
	int add = 0;
	for (int i = 0; i < wv; ++i) add += sw[i];
	__syncthreads();
	return v + add;
}
__device__ inline int b_incl_last(int v, int lane, int wv, int *sw)
{
	v = wave_incl_last(v, lane);
	if (lane == 63) sw[wv] = v;
	__syncthreads();
	if (v < 0) for (int i = wv - 1; i >= 0; --i) if (sw[i] >= 0) { v = sw[i]; break; }
	__syncthreads();
	return v;
}

struct Ctx { int64_t na; const ulonglong2 *a; int32_t qlen; };

// the read of region g, its anchors and its length; false when an offset leaves a capacity
__device__ bool locate(const CigArgs &A, int64_t g, Ctx &C)
{
	RegionRead Q;
	if (!read_of_region(A, g, Q)) return false;
	C.na = Q.na; C.a = A.b + Q.b0; C.qlen = Q.qlen;
	return true;
}

// the effective ez of an item: the second list's where second_of names one, else the first pass's; the reset ez with zdropped = 1 of an item over max_sw_mat
// (:323-325); score and one M word of an sr ungapped item whose test gave 0.  bad: CIG_REFUSED / CIG_INCOMPLETE if the item is consumed.
struct Eff {
	int32_t kind, rs, re, qs, qe, anchor, n, zdropped, max, max_q, max_t, mqe_t, score, reach_end, code, bad;
	const uint32_t *p;                     // its CIGAR words; nullptr: the one word `synth`
	uint32_t synth;
};

__device__ Eff load_eff(const CigArgs &A, int64_t k)
{
	Eff E = {};
	const AlnItem it = A.items[k];
	E.kind = it.kind; E.rs = it.rs; E.re = it.re; E.qs = it.qs; E.qe = it.qe; E.anchor = it.anchor;
	const int base = it.kind & 15;
	if (it.kind & ALN_OVER) { E.zdropped = 1; E.max_q = E.max_t = E.mqe_t = -1; return E; }
	const int32_t s = A.second_of[k];
	const int32_t t = it.task;
	if (base == ALN_UNGAPPED) {
		if (s == CIG_NO_ROOM) { E.bad = CIG_INCOMPLETE; return E; }
		if (s == CIG_LOST) { E.bad = CIG_REFUSED; return E; }                          // its bases leave the pool: the second-pass entry could not test it
		if (s < 0) { E.n = 1; E.synth = (uint32_t)(it.qe - it.qs) << 4; E.score = it.score; return E; }
		E.code = 1;
	} else {
		if (t < 0 || t >= A.tasks_cap) { E.bad = CIG_REFUSED; return E; }
		if (base == ALN_GAP) {
			const ZdropRes z = A.zres[t];
			if (z.status != 0 || (uint32_t)z.code > 2u || (z.code == 0 && s >= 0)) { E.bad = CIG_REFUSED; return E; }
			if (z.code != 0 && s < 0) { E.bad = CIG_INCOMPLETE; return E; }                // its second pass has not been made
			E.code = z.code;
		} else if (s >= 0 || (base != ALN_LEFT && base != ALN_RIGHT)) { E.bad = CIG_REFUSED; return E; }
	}
	const KswRes *R;
	const uint32_t *buf;
	int64_t c0, c1, cap;
	if (s >= 0) {
		if (s >= A.tasks2_cap) { E.bad = CIG_REFUSED; return E; }
		R = A.res2 + s; c0 = A.cig_off2[s]; c1 = A.cig_off2[s + 1]; buf = A.cigar2; cap = A.cig2_cap;
	} else { R = A.res + t; c0 = A.cig_off[t]; c1 = A.cig_off[t + 1]; buf = A.cigar; cap = A.cig_cap; }
	if (c0 < 0 || c1 < c0 || c1 > cap) { E.bad = CIG_REFUSED; return E; }
	const KswRes r = *R;
	if (r.status != 0 || r.n_cigar < 0 || r.n_cigar > c1 - c0) { E.bad = CIG_INCOMPLETE; return E; }
	E.n = r.n_cigar; E.zdropped = r.zdropped; E.max = (int32_t)r.max; E.max_q = r.max_q; E.max_t = r.max_t; E.mqe_t = r.mqe_t; E.score = r.score; E.reach_end = r.reach_end;
	E.p = buf + c0;
	return E;
}

// mm_test_zdrop (:47-89) on one M word of `len` bases, by the wave: every point lies on one diagonal, so z = max - score; the answer is max_zdrop > zdrop
__device__ int sr_test(const CigArgs &A, int64_t qo, int64_t to, int32_t len, int lane)
{
	int carry_s = 0, mv = INT32_MIN, best = 0;
	for (int32_t b0 = 0; b0 < len; b0 += 64) {
		const int32_t j = b0 + lane;
		const bool on = j < len;
		int d = 0;
		if (on) { const int ct = A.seq[to + j], cq = A.seq[qo + j]; d = A.mat[(ct > 4 ? 4 : ct) * 5 + (cq > 4 ? 4 : cq)]; }
		const int S = carry_s + wave_incl_sum(d, lane);
		int v = wave_incl_max(on ? S : INT32_MIN, lane);
		if (mv > v) v = mv;
		best = max(best, wave_max(on ? v - S : 0));
		carry_s = __shfl(S, 63); mv = __shfl(v, 63);
	}
	return best > A.opt.zdrop ? 1 : 0;
}

template <bool EMIT>
__device__ void second_walk(const CigArgs &A, int lane)
{
	for (int64_t g = blockIdx.x; g < A.n_regs; g += gridDim.x) {
		const AlnReg R = A.aregs[g];
		if (R.status != 0 || R.n_items < 0 || R.item0 < 0 || R.item0 > A.items_cap - R.n_items) {
			if (!EMIT && lane == 0) { A.sec[g] = CigSec{0, 0}; if (R.status == 0) atomicAdd(A.flags + 0, 1); }
			continue;
		}
		int64_t tk = 0, cg = 0;
		bool room = true;
		if (EMIT) { const CigSec s = A.sec[g]; tk = s.tk0; cg = s.cg0; room = tk >= 0; }
		for (int32_t i0 = 0; i0 < R.n_items; i0 += 64) {
			const int32_t k = i0 + lane;
			const bool on = k < R.n_items;
			AlnItem it = {};
			if (on) it = A.items[R.item0 + k];
			bool want = false, lost = false;
			KswTask T = {};
			if (on && it.kind == ALN_GAP && it.task >= 0 && it.task < A.tasks_cap) {
				const ZdropRes z = A.zres[it.task];
				if (z.status == 0 && (z.code == 1 || z.code == 2)) {
					want = true;
					T = A.tasks[it.task];
					T.flag &= ~KSW_EZ_APPROX_MAX;
					T.zdrop = z.code == 2 ? A.opt.zdrop_inv : A.opt.zdrop;
				}
			}
			uint64_t um = __ballot(on && it.kind == ALN_UNGAPPED && (A.opt.flag & ALN_F_SR));
			while (um) {                                                               // the ungapped item has no first-pass task: its test is made here
				const int f = __ffsll((unsigned long long)um) - 1;
				um &= um - 1;
				const int32_t uqs = __shfl(it.qs, f), uqe = __shfl(it.qe, f), urs = __shfl(it.rs, f), ure = __shfl(it.re, f);
				const int64_t qo = R.q_off + (uqs - R.qs0), to = R.t_off + (urs - R.rs0);
				const int32_t len = uqe - uqs;
				if (len < 0 || ure - urs < 0 || qo < 0 || to < 0 || qo > A.pool_cap - len || to > A.pool_cap - (ure - urs) || len > ure - urs) {
					if (!EMIT && lane == 0) atomicAdd(A.flags + 0, 1);
					if (lane == f) lost = true;                                            // marked in the map, so that the join refuses the region
					continue;
				}
				if (sr_test(A, qo, to, len, lane) && lane == f) {
					want = true;
					T = KswTask{qo, to, len, ure - urs, A.opt.bw_ext, A.opt.zdrop, -1, 0};
				}
			}
			const int64_t words = want ? slot_of((int64_t)T.qlen + T.tlen, A.opt.cig_shift) : 0;
			const uint64_t m = __ballot(want);
			// slots of up to 2^21 words, 64 of them: below 2^31
			const int inc = wave_incl_sum((int)words, lane);
			if (EMIT && on) {
				const int64_t idx = tk + __popcll(m & ((1ull << lane) - 1));
				A.second_of[R.item0 + k] = lost ? CIG_LOST : !want ? -1 : room ? (int32_t)idx : CIG_NO_ROOM;
				if (want && room) { A.tasks2[idx] = T; A.cig_off2[idx] = cg + inc - words; }
			}
			tk += __popcll(m); cg += __shfl(inc, 63);
		}
		if (!EMIT && lane == 0) A.sec[g] = CigSec{tk, cg};
	}
}

__global__ __launch_bounds__(64) void cig_second_count(const CigArgs A) { second_walk<false>(A, (int)threadIdx.x); }
__global__ __launch_bounds__(64) void cig_second_emit(const CigArgs A) { second_walk<true>(A, (int)threadIdx.x); }

__global__ __launch_bounds__(1024) void cig_second_scan(const CigArgs A)
{
	__shared__ int64_t sh[2][1024];
	const int tid = threadIdx.x;
	int64_t carry[2] = {0, 0};
	for (int64_t base = 0; base < A.n_regs; base += 1024) {
		const int64_t g = base + tid;
		int64_t v[2] = {0, 0}, in[2], tot[2];
		if (g < A.n_regs) { const CigSec s = A.sec[g]; v[0] = s.tk0; v[1] = s.cg0; }
		block_incl_sum_1024(sh, tid, v, in, tot);
		if (g < A.n_regs) {
			CigSec s = {carry[0] + in[0] - v[0], carry[1] + in[1] - v[1]};
			if (v[0] > 0 && (s.tk0 + v[0] > A.tasks2_cap || s.cg0 + v[1] > A.cig2_cap)) { s.tk0 = -1; atomicAdd(A.flags + 2, 1); }
			A.sec[g] = s;
		}
		for (int c = 0; c < 2; ++c) carry[c] += tot[c];
	}
	if (tid == 0) {
		A.totals[0] = carry[0]; A.totals[1] = carry[1];
		if (carry[0] <= A.tasks2_cap) A.cig_off2[carry[0]] = carry[1];
	}
}

__global__ __launch_bounds__(64) void cig_cut(const CigArgs A)
{
	__shared__ int32_t sP[65];
	__shared__ const uint32_t *sp[64];
	__shared__ uint32_t ssyn[64];
	const int lane = threadIdx.x;
	for (int64_t g = blockIdx.x; g < A.n_regs; g += gridDim.x) {
		__syncthreads();
		int status = CIG_REFUSED;
		CigReg O = {};
		do {
			const AlnReg R = A.aregs[g];
			if (R.status != 0) break;
			Ctx C;
			if (!locate(A, g, C)) break;
			const Reg r = A.regs[g];
			if (R.cnt1 == 0 && R.n_items == 0) {                                           // :578: the region stays as it is
				O.rs1 = r.rs; O.re1 = r.re; O.r_qs = r.qs; O.r_qe = r.qe;
				status = 0;
				break;
			}
			if (R.n_items < 0 || R.item0 < 0 || R.item0 > A.items_cap - R.n_items || R.as1 < 0 || R.cnt1 < 1 || (int64_t)R.as1 + R.cnt1 > C.na) break;
			int32_t dp = 0, merges = 0, carry_op = -1, drop = -1, n_used = 0;
			int64_t words = 0, qsum = 0, tsum = 0;
			uint64_t ref = 0, inc = 0;
			for (int32_t i0 = 0; i0 < R.n_items && drop < 0; i0 += 64) {
				const int32_t k = i0 + lane;
				const bool on = k < R.n_items;
				Eff E = {};
				if (on) E = load_eff(A, R.item0 + k);
				const int base = E.kind & 15;
				const bool gap = base == ALN_GAP || base == ALN_UNGAPPED;
				const uint64_t dm = __ballot(on && gap && !E.bad && E.zdropped);
				const int f = dm ? __ffsll((unsigned long long)dm) - 1 : 64;
				if (dm) drop = i0 + f;
				const bool used = on && lane <= f;                                         // the right extension is the last item: behind a drop it is not used
				ref |= __ballot(used && E.bad == CIG_REFUSED); inc |= __ballot(used && E.bad == CIG_INCOMPLETE);
				const int32_t n = used && !E.bad ? E.n : 0;
				if (used && !E.bad) dp += gap ? (E.zdropped ? E.max : E.score) : (n > 0 ? E.max : 0);
				// a boundary merges when the item's first op is the last op of the item with words in front of it (:303)
				uint32_t fw = 0, lw = 0;
				if (n > 0) { fw = E.p ? E.p[0] : E.synth; lw = E.p ? E.p[n - 1] : E.synth; }
				const int il = wave_incl_last(n > 0 ? (int)(lw & 0xf) : -1, lane);
				int prev = __shfl_up(il, 1);
				if (lane == 0 || prev < 0) prev = carry_op;
				merges += __popcll(__ballot(n > 0 && prev == (int)(fw & 0xf)));
				const int last = __shfl(il, 63);
				if (last >= 0) carry_op = last;
				// the lengths of :284, over the words of the step's items
				const int pin = wave_incl_sum(n, lane), tot = __shfl(pin, 63);
				if (lane == 0) sP[0] = 0;
				sP[lane + 1] = pin; sp[lane] = E.p; ssyn[lane] = E.synth;
				__syncthreads();
				for (int32_t w = lane; w < tot; w += 64) {
					int lo = 0, hi = 64;
					while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sP[mid] <= w) lo = mid; else hi = mid; }
					const uint32_t word = sp[lo] ? sp[lo][w - sP[lo]] : ssyn[lo], op = word & 0xf, len = word >> 4;
					if (op <= 1) qsum += len;
					if (op == 0 || op == 2 || op == 3) tsum += len;
				}
				__syncthreads();
				words += tot; n_used += __popcll(__ballot(used));
			}
			if (ref) break;
			if (inc) { status = CIG_INCOMPLETE; break; }
			qsum = wave_sum(qsum); tsum = wave_sum(tsum);
			dp = wave_sum(dp);
			// every lane takes the same scalars
			int32_t rs1 = R.rs, qs1 = R.qs;
			Eff first = {}, lastE = {};
			if (R.n_items > 0) { first = load_eff(A, R.item0); lastE = load_eff(A, R.item0 + R.n_items - 1); }
			const int has_left = R.n_items > 0 && (first.kind & 15) == ALN_LEFT, has_right = R.n_items > 0 && (lastE.kind & 15) == ALN_RIGHT;
			if (has_left) {                                                                // :702-703
				rs1 = first.re - (first.reach_end ? first.mqe_t + 1 : first.max_t + 1);
				qs1 = first.qe - (first.reach_end ? first.qe - first.qs : first.max_q + 1);
			}
			int32_t re1 = R.rs, qe1 = R.qs;                                                // :706
			if (drop >= 0) {
				const Eff D = load_eff(A, R.item0 + drop);
				re1 = D.rs + (D.max_t + 1); qe1 = D.qs + (D.max_q + 1);                    // :755-756
				const int32_t i = D.anchor - R.as1, thr = D.rs + D.max_t;
				if (i < 0 || i >= R.cnt1) break;
				int32_t j = -1;
				for (int32_t j0 = i - 1; j0 >= 0 && j < 0; j0 -= 64) {                     // :749-751, 64 anchors a step, IGNORE / TANDEM ones too
					const int32_t jj = j0 - lane;
					const uint64_t m = __ballot(jj >= 0 && lo32(C.a[R.as1 + jj].x) <= thr);
					if (m) j = j0 - (__ffsll((unsigned long long)m) - 1);
				}
				if (j < 0) j = 0;
				O.dropped = 1; O.drop_item = drop; O.zdrop_code = D.code;
				if (R.cnt1 - (j + 1) >= A.opt.min_cnt) { O.split_n = R.as1 + j + 1 - r.as; O.split_inv = D.code == 2; }
			} else {
				O.drop_item = -1;
				const int32_t lg = R.n_items - 1 - has_right;
				if (lg >= has_left) { const Eff G = load_eff(A, R.item0 + lg); re1 = G.re; qe1 = G.qe; }
				if (has_right) {                                                           // :776-777
					re1 = lastE.rs + (lastE.reach_end ? lastE.mqe_t + 1 : lastE.max_t + 1);
					qe1 = lastE.qs + (lastE.reach_end ? lastE.qe - lastE.qs : lastE.max_q + 1);
				}
			}
			O.has_p = words > 0 || drop >= 0;
			if (words - merges > INT32_MAX) break;
			if (O.has_p && (qsum != (int64_t)qe1 - qs1 || tsum != (int64_t)re1 - rs1)) break;       // :284
			if (qs1 < 0 || rs1 < 0 || qe1 > C.qlen || (int64_t)re1 - rs1 > (int64_t)R.re0 - R.rs0) break;   // :707, 779, 785
			O.n_used = n_used; O.n_cigar = (int32_t)(words - merges); O.dp_score = dp;
			O.rs1 = rs1; O.re1 = re1; O.qs1 = qs1; O.qe1 = qe1;
			O.r_qs = R.rev ? C.qlen - qe1 : qs1; O.r_qe = R.rev ? C.qlen - qs1 : qe1;       // :782-783
			status = 0;
		} while (0);
		if (lane == 0) {
			if (status == 0) A.cregs[g] = O;
			else { A.cregs[g].status = status; atomicAdd(A.flags + (status == CIG_REFUSED ? 0 : 1), 1); }
		}
	}
}

__global__ __launch_bounds__(1024) void cig_scan(const CigArgs A)
{
	__shared__ int64_t sh[2][1024];
	const int tid = threadIdx.x;
	int64_t carry[2] = {0, 0};
	for (int64_t base = 0; base < A.n_regs; base += 1024) {
		const int64_t g = base + tid;
		int64_t v[2] = {0, 0};
		CigReg C = {};
		C.status = -1;
		if (g < A.n_regs) {
			C.status = A.cregs[g].status;
			if (C.status == 0) { C = A.cregs[g]; v[0] = C.n_cigar; v[1] = C.n_cigar > 0; }
		}
		for (int c = 0; c < 2; ++c) sh[c][tid] = v[c];
		__syncthreads();
		for (int d = 1; d < 1024; d <<= 1) {
			int64_t t[2];
			for (int c = 0; c < 2; ++c) t[c] = tid >= d ? sh[c][tid - d] : 0;
			__syncthreads();
			for (int c = 0; c < 2; ++c) sh[c][tid] += t[c];
			__syncthreads();
		}
		if (C.status == 0) {
			const int64_t c0 = carry[0] + sh[0][tid] - v[0], k = carry[1] + sh[1][tid] - v[1];
			if (v[0] > 0 && (c0 + v[0] > A.words_cap || k >= A.extra_cap)) { A.cregs[g].status = CIG_OVER_CAP; atomicAdd(A.flags + 2, 1); }
			else {
				A.cregs[g].cig0 = c0;
				if (v[0] > 0) {
					const AlnReg R = A.aregs[g];
					A.in_off[k] = c0; A.extra_reg[k] = (int32_t)g;
					A.extra[k] = ExtraTask{R.q_off + (C.qs1 - R.qs0), R.t_off + (C.rs1 - R.rs0), C.qe1 - C.qs1, C.re1 - C.rs1, C.n_cigar, R.rev};
				}
			}
		}
		for (int c = 0; c < 2; ++c) carry[c] += sh[c][1023];
		__syncthreads();
	}
	if (tid == 0) {
		A.totals[0] = carry[0]; A.totals[1] = carry[1];
		if (carry[1] <= A.extra_cap) A.in_off[carry[1]] = carry[0];
	}
}

// A region's used items are taken CIG_PIECE at a time (their word prefix, their merge prefix and their sources in LDS), their words CIG_PIECE at a time.  A lane
// finds its word's item by bisection.  A word is a head unless it is the first of its item and the item's boundary merges; its output index is its stream position
// less the merges up to its item.  The merged length is a segmented sum over the heads, carried across lanes, waves, pieces and item pieces: the head that ends a
// segment stores it, the region's last segment is stored at the end.
__global__ __launch_bounds__(CIG_PIECE) void cig_gather(const CigArgs A)
{
	__shared__ int32_t sP[CIG_PIECE + 1], sM[CIG_PIECE], sI[CIG_PIECE], sO[CIG_PIECE], sw[4], sf[4], s_last;
	__shared__ uint32_t ssyn[CIG_PIECE], sS[CIG_PIECE];
	__shared__ const uint32_t *sp[CIG_PIECE];
	__shared__ CigReg sC;
	__shared__ int64_t s_item0;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	for (int64_t g = blockIdx.x; g < A.n_regs; g += gridDim.x) {
		__syncthreads();
		if (tid == 0) { sC = A.cregs[g]; s_item0 = A.aregs[g].item0; }                     // the per-region lookups, once a workgroup
		__syncthreads();
		const CigReg C = sC;
		if (C.status != 0 || C.n_cigar <= 0) continue;
		const int64_t item0 = s_item0;
		uint32_t *const out = A.cig_out + C.cig0;
		int64_t pos = 0;                                                                   // stream words in front of the item piece
		int32_t merges = 0, carry_op = -1;
		uint32_t seg_sum = 0, seg_op = 0;                                                  // the open segment
		int32_t seg_idx = -1;
		for (int32_t c0 = 0; c0 < C.n_used; c0 += CIG_PIECE) {
			const int32_t k = c0 + tid;
			Eff E = {};
			if (k < C.n_used) E = load_eff(A, item0 + k);
			const int32_t n = k < C.n_used && !E.bad ? E.n : 0;
			uint32_t fw = 0, lw = 0;
			if (n > 0) { fw = E.p ? E.p[0] : E.synth; lw = E.p ? E.p[n - 1] : E.synth; }
			const int il = b_incl_last(n > 0 ? (int)(lw & 0xf) : -1, lane, wv, sw);
			sI[tid] = il;
			if (tid == CIG_PIECE - 1) s_last = il;
			__syncthreads();
			int prev = tid > 0 ? sI[tid - 1] : -1;
			if (prev < 0) prev = carry_op;
			__syncthreads();
			const int mg = n > 0 && prev == (int)(fw & 0xf);
			const int mi = b_incl_sum(mg, lane, wv, sw), pi = b_incl_sum(n, lane, wv, sw);
			if (tid == 0) sP[0] = 0;
			sP[tid + 1] = pi; sM[tid] = mi; sp[tid] = E.p; ssyn[tid] = E.synth;
			__syncthreads();
			const int32_t tot = sP[CIG_PIECE];
			for (int32_t w0 = 0; w0 < tot; w0 += CIG_PIECE) {
				const int32_t w = w0 + tid;
				const bool on = w < tot;
				uint32_t len = 0, op = 0;
				int head = 0;
				int32_t oidx = 0;
				if (on) {
					int lo = 0, hi = CIG_PIECE;
					while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sP[mid] <= w) lo = mid; else hi = mid; }
					const uint32_t word = sp[lo] ? sp[lo][w - sP[lo]] : ssyn[lo];
					op = word & 0xf; len = word >> 4;
					const int merged = sM[lo] - (lo > 0 ? sM[lo - 1] : 0);
					head = !(w == sP[lo] && merged);
					oidx = (int32_t)(pos + w - (merges + sM[lo]));
				}
				// the segmented sum: inside the wave, then over the waves in front, then the open segment
				uint32_t S = len;
				int f = head;
				for (int d = 1; d < 64; d <<= 1) {
					const uint32_t us = __shfl_up(S, d);
					const int uf = __shfl_up(f, d);
					if (lane >= d && !f) { S += us; f = uf; }
				}
				if (lane == 63) { sw[wv] = (int32_t)S; sf[wv] = f; }
				__syncthreads();
				if (!f) for (int i = wv - 1; i >= 0; --i) { S += (uint32_t)sw[i]; if (sf[i]) { f = 1; break; } }
				if (!f) S += seg_sum;
				sS[tid] = S; sI[tid] = oidx; sO[tid] = (int32_t)op;
				__syncthreads();
				if (on && head) {                                                          // this head ends the segment in front of it
					const uint32_t pS = tid > 0 ? sS[tid - 1] : seg_sum, pO = tid > 0 ? (uint32_t)sO[tid - 1] : seg_op;
					const int32_t pI = tid > 0 ? sI[tid - 1] : seg_idx;
					if (pI >= 0 && pI < C.n_cigar) out[pI] = pS << 4 | pO;
				}
				const int lastv = (tot - w0 < CIG_PIECE ? tot - w0 : CIG_PIECE) - 1;
				const uint32_t nS = sS[lastv], nO = (uint32_t)sO[lastv];
				const int32_t nI = sI[lastv];
				__syncthreads();
				seg_sum = nS; seg_op = nO; seg_idx = nI;
			}
			pos += tot; merges += sM[CIG_PIECE - 1];
			if (s_last >= 0) carry_op = s_last;
			__syncthreads();
		}
		if (tid == 0 && seg_idx >= 0 && seg_idx < C.n_cigar) out[seg_idx] = seg_sum << 4 | seg_op;
	}
}

unsigned wave_grid(const CigArgs &A) { return (unsigned)(A.n_regs < 8192 ? A.n_regs : 8192); }

} // namespace

hipError_t launch_cig_second_count(const CigArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(cig_second_count, dim3(wave_grid(A)), dim3(64), 0, st, A);
	hipLaunchKernelGGL(cig_second_scan, dim3(1), dim3(1024), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_cig_second_emit(const CigArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(cig_second_emit, dim3(wave_grid(A)), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_cig_cut(const CigArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(cig_cut, dim3(wave_grid(A)), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_cig_scan(const CigArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(cig_scan, dim3(1), dim3(1024), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_cig_gather(const CigArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	const int64_t grid = A.n_regs < 16384 ? A.n_regs : 16384;
	hipLaunchKernelGGL(cig_gather, dim3((unsigned)grid), dim3(CIG_PIECE), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
