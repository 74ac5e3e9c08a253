// align_extra.hip -- the two CIGAR walks that stand around the base alignment in mm_align1 (align.c), each as a batch of independent items, byte for byte:
//   extra_update: mm_update_extra (:240-286) = mm_fix_cigar (:91-167), the counts and dp_max of :249-283, mm_update_cigar_eqx (:169-238), one wave per region;
//   extra_zdrop:  mm_test_zdrop (:47-89) up to its return value and the condition of :72, one wave per ksw task.
// Both are persistent grids: block b takes items b, b + gridDim.x, ... and owns scratch slot b.  A CIGAR is copied into four working arrays of n words (the words,
// two prefix arrays, one more), in LDS up to EXTRA_LDS_WORDS words and in the slot beyond; the sequences are read from global memory where they lie.
// Every serial loop of the source is a scan here:
//   left alignment   -- an indel's match run depends on nothing but the sequences; only its cap, the current length of the M word in front, depends on the indel two
//                       words back: l_k = min(run_k, len_{k-1} + l_{k-2}), a scan over maps x -> min(a, b + x);
//   the I/D repair   -- runs of words that are I, D or empty are disjoint; the lane at the first word of a run walks it;
//   squeeze, merge   -- ballot compaction and a segmented sum;
//   counts, dp_max, EQX and the z-drop walk -- over alignment columns, 64 per step, the column's word by bisection over the column prefix; dp_max by composing
//                       (T, C, P, M) with s' = max(s + T, C), max' = max(max, s + P, M); the z-drop by a prefix sum and a prefix maximum where the later point wins.
// Stores are plain vector stores; the only atomics are the adds of the three counters; every loop's bound is known at its entry or falls with every step.
#include "align_extra.h"
#include "wave_ops.h"

namespace mm2c {

constexpr int XNEG = -0x40000000;
constexpr int XINF = 0x20000000;

// inclusive scan of the maps x -> min(a, b + x) in lane order, applied to `carry`: what comes out of each lane's map
__device__ static inline int x_map_scan(int a, int b, int carry, int lane)
{
	for (int d = 1; d < 64; d <<= 1) {
		const int ao = __shfl_up(a, d), bo = __shfl_up(b, d);
		if (lane >= d) { const int t = b + ao; a = a < t ? a : t; if (a > XINF) a = XINF; b += bo; if (b > XINF) b = XINF; }
	}
	const int c = b + carry;
	return a < c ? a : c;
}

struct XWork { uint32_t *W; int32_t *A, *B, *C; };

// the four arrays of an item of n words, or W == nullptr if they fit neither LDS nor the slot
__device__ static inline XWork x_work(uint32_t *lds, const ExtraArgs &A, int n)
{
	XWork w;
	uint32_t *base = nullptr;
	int64_t pitch = 0;
	if (n <= EXTRA_LDS_WORDS) { base = lds; pitch = EXTRA_LDS_WORDS; }
	else if (n <= A.slot_words) { base = A.scratch + (int64_t)blockIdx.x * 4 * A.slot_words; pitch = A.slot_words; }
	w.W = base; w.A = (int32_t *)(base + pitch); w.B = (int32_t *)(base + 2 * pitch); w.C = (int32_t *)(base + 3 * pitch);
	return w;
}

// the largest w in [0, m) with cp[w] <= c (cp[0] == 0 <= c)
__device__ static inline int x_word_of(const int32_t *cp, int m, int c)
{
	int lo = 0, hi = m - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (cp[mid] <= c) lo = mid; else hi = mid - 1;
	}
	return lo;
}

__global__ __launch_bounds__(64) void extra_update(const ExtraArgs A)
{
	__shared__ uint32_t lds[4 * EXTRA_LDS_WORDS];
	__shared__ int32_t mat[25];
	const int lane = (int)threadIdx.x;
	if (lane < 25) mat[lane] = A.mat[lane];

	for (int64_t i = blockIdx.x; i < A.n; i += gridDim.x) {
		__syncthreads();                                                     // the region before this one has read its last word
		const ExtraTask T = A.tasks[i];
		const int n = T.n_cigar;
		const int64_t i0 = A.in_off[i], o0 = A.out_off[i], o1 = A.out_off[i + 1];
		const bool bad = n < 0 || T.qlen < 0 || T.tlen < 0 || T.qlen > KSW_MAX_LEN || T.tlen > KSW_MAX_LEN || i0 < 0 || i0 > A.in_cap - n || o0 < 0 || o1 < o0 || o1 > A.out_cap ||
		                 T.q_off < 0 || T.t_off < 0 || T.q_off > A.seq_cap - T.qlen || T.t_off > A.seq_cap - T.tlen;
		if (bad) {
			if (lane == 0) { A.res[i].status = EXTRA_REFUSED; atomicAdd(&A.flags[0], 1); }
			continue;
		}
		const XWork X = x_work(lds, A, n);
		if (n > 0 && X.W == nullptr) {
			if (lane == 0) { A.res[i].status = EXTRA_TOO_BIG; atomicAdd(&A.flags[1], 1); }
			continue;
		}
		uint32_t *const W = X.W;
		int32_t *const QP = X.A, *const TP = X.B, *const LR = X.C;
		const uint8_t *qs = A.seq + T.q_off, *ts = A.seq + T.t_off;
		const uint32_t *const in = A.cig_in + i0;
		const int64_t room = o1 - o0;
		uint32_t *const out = A.cig_out + o0;

		// the copy, what the reference is not defined on, and the prefixes of :102,119-122
		{
			int64_t sq = 0, stt = 0;
			int anyzero = 0, anynz = 0, badop = 0;
			uint32_t cq = 0, ct = 0;
			for (int base = 0; base < n; base += 64) {
				const int k = base + lane;
				const bool on = k < n;
				const uint32_t w = on ? in[k] : 0u, op = w & 0xf, len = w >> 4;
				if (on) { W[k] = w; badop |= op > 3 || (op == 3 && len == 0); anyzero |= len == 0; anynz |= len != 0; }
				const uint32_t dq = on && op <= 1 ? len : 0u, dt = on && (op == 0 || op == 2 || op == 3) ? len : 0u;
				sq += dq; stt += dt;
				const uint32_t iq = (uint32_t)wave_incl_sum((int)dq, lane), it = (uint32_t)wave_incl_sum((int)dt, lane);
				if (on) { QP[k] = (int32_t)(cq + iq - dq); TP[k] = (int32_t)(ct + it - dt); }
				cq += (uint32_t)__shfl((int)iq, 63); ct += (uint32_t)__shfl((int)it, 63);
			}
			sq = wave_sum(sq); stt = wave_sum(stt);
			anyzero = __any(anyzero); anynz = __any(anynz); badop = __any(badop);
			if (badop || sq != T.qlen || stt != T.tlen || (n >= 2 && !anynz)) {
				if (lane == 0) { A.res[i].status = EXTRA_REFUSED; atomicAdd(&A.flags[0], 1); }
				continue;
			}
			__syncthreads();
			int m = n, w0 = 0, qshift = 0, tshift = 0;
			if (n >= 2) {                                                    // mm_fix_cigar behind its return of :97
				int shrink = anyzero;
				// :98-124.  c_k: the shift that has lengthened word k when the next word looks at it (l_{k-1} on the M word behind an eligible indel, l_k on the indel)
				int carry_c = 0, carry_elig = 0, carry_lim = 0;
				for (int base = 0; base < n; base += 64) {
					const int k = base + lane;
					const bool on = k < n;
					const uint32_t w = on ? W[k] : 0u, op = w & 0xf;
					const int len = (int)(w >> 4);
					const bool elig = on && k > 0 && k < n - 1 && (op == 1 || op == 2) && (W[k - 1] & 0xf) == 0 && (W[k + 1] & 0xf) == 0;
					const int prev_len = elig ? (int)(W[k - 1] >> 4) : 0;
					const uint8_t *const s = op == 1 ? qs : ts;
					const int pos = elig ? (op == 1 ? QP[k] : TP[k]) : 0;    // prev_len <= pos: the M word in front lies in front on both sequences
					int prev_elig = __shfl_up((int)elig, 1);
					if (lane == 0) prev_elig = carry_elig;
					const bool pass = on && op == 0 && prev_elig;            // the M word behind an eligible indel hands its shift on
					// no run is walked beyond what the cap can be at most: the M word in front plus the most the indel two words back can have moved
					const int lim = x_map_scan(elig || pass ? XINF : 0, prev_len, carry_lim, lane);     // <= pos
					carry_lim = __shfl(lim, 63);
					int raw = 0;
					if (elig) while (raw < lim && raw < EXTRA_RUN_LANE && s[pos - 1 - raw] == s[pos + len - 1 - raw]) ++raw;
					uint64_t more = __ballot(elig && raw == EXTRA_RUN_LANE && raw < lim);
					while (more) {                                           // a long run: 64 bases per step, all lanes on one indel
						const int src = __ffsll((long long)more) - 1;
						more &= more - 1;
						const int p1 = __shfl(pos, src), l1 = __shfl(len, src), o1_ = __shfl((int)op, src), lim1 = __shfl(lim, src);
						const uint8_t *const s1 = o1_ == 1 ? qs : ts;
						int l0 = EXTRA_RUN_LANE, total = 0;
						for (;;) {                                           // l0 grows by 64; at l >= lim1 a lane misses, so it ends
							const int l = l0 + lane;
							const bool hit = l < lim1 && s1[p1 - 1 - l] == s1[p1 + l1 - 1 - l];
							const uint64_t miss = ~__ballot(hit);
							if (miss) { total = l0 + __ffsll((long long)miss) - 1; break; }
							l0 += 64;
						}
						if (lane == src) raw = total;
					}
					// the word's map x -> min(a, b + x) on the shift carried into it
					const int c = x_map_scan(elig ? raw : pass ? XINF : 0, prev_len, carry_c, lane);
					int c_prev = __shfl_up(c, 1);
					if (lane == 0) c_prev = carry_c;
					if (elig && c == prev_len + c_prev) shrink = 1;          // l == prev_len (:117)
					if (on) LR[k] = elig ? c : 0;
					carry_c = __shfl(c, 63); carry_elig = __shfl((int)elig, 63);
				}
				__syncthreads();
				for (int k = lane; k < n; k += 64) {                         // :116 on the M words
					const uint32_t w = W[k];
					if ((w & 0xf) == 0) W[k] = (uint32_t)((int)(w >> 4) + (k > 0 ? LR[k - 1] : 0) - (k < n - 1 ? LR[k + 1] : 0)) << 4;
				}
				__syncthreads();
				// :126-144.  A run is a stretch of words that are I, D or empty; the test fires at the first I,D or D,I pair in it and then skips the stretch
				for (int base = 0; base < n; base += 64) {
					const int k = base + lane;
					bool start = false;
					if (k < n) {
						const uint32_t w = W[k], wp = k > 0 ? W[k - 1] : 0x10u;
						const bool in_run = (w & 0xf) == 1 || (w & 0xf) == 2 || (w >> 4) == 0, prev_in = k > 0 && ((wp & 0xf) == 1 || (wp & 0xf) == 2 || (wp >> 4) == 0);
						start = in_run && !prev_in;
					}
					__syncthreads();
					if (start) {
						int e = k;
						while (e < n) { const uint32_t w = W[e]; if ((w & 0xf) == 1 || (w & 0xf) == 2 || (w >> 4) == 0) ++e; else break; }
						int f = -1;
						for (int x = k; x < e && x + 2 < n; ++x) {
							const uint32_t a = W[x] & 0xf, b = W[x + 1] & 0xf;
							if (a > 0 && a + b == 3) { f = x; break; }
						}
						if (f >= 0) {
							uint32_t s1 = 0, s2 = 0;
							for (int x = f; x < e; ++x) { const uint32_t w = W[x]; if ((w & 0xf) == 1) s1 += w >> 4; else if ((w & 0xf) == 2) s2 += w >> 4; }
							if (s1 > 0 && s2 > 0 && e - f > 2) {
								W[f] = s1 << 4 | 1; W[f + 1] = s2 << 4 | 2;
								for (int x = f + 2; x < e; ++x) W[x] &= 0xf;
								shrink = 1;
							}
						}
					}
				}
				shrink = __any(shrink);
				__syncthreads();
				if (shrink) {                                                // :145-156
					int cnt = 0;
					for (int base = 0; base < n; base += 64) {               // a word moves to an index at or below its own; the wave has read the step's words by then
						const int k = base + lane;
						const uint32_t w = k < n ? W[k] : 0u;
						const bool keep = (w >> 4) != 0;
						const uint64_t mask = __ballot(keep);
						if (keep) W[cnt + lanes_below(mask)] = w;
						cnt += __popcll(mask);
					}
					m = cnt;
					__syncthreads();
					int outn = 0, carry_p = 0, prev_end = 0;
					for (int base = 0; base < m; base += 64) {
						const int j = base + lane;
						const bool on = j < m;
						const uint32_t w = on ? W[j] : 0u, op = w & 0xf;
						const uint32_t nop = j + 1 < m ? W[j + 1] & 0xf : 16u;
						const bool end = on && op != nop;
						const int P = carry_p + wave_incl_sum(on ? (int)(w >> 4) : 0, lane);
						const int ei = wave_incl_max(end ? P : 0, lane);
						int ex = __shfl_up(ei, 1);
						if (lane == 0) ex = 0;
						if (ex < prev_end) ex = prev_end;
						const uint64_t mask = __ballot(end);
						if (end) W[outn + lanes_below(mask)] = (uint32_t)(P - ex) << 4 | op;
						outn += __popcll(mask);
						carry_p = __shfl(P, 63);
						const int el = __shfl(ei, 63);
						if (el > prev_end) prev_end = el;
					}
					m = outn;
					__syncthreads();
				}
				const uint32_t first = W[0];                                 // :157-166 (m >= 1: some length was not zero)
				if ((first & 0xf) == 1) { qshift = (int)(first >> 4); w0 = 1; --m; }
				else if ((first & 0xf) == 2) { tshift = (int)(first >> 4); w0 = 1; --m; }
			}
			qs += qshift; ts += tshift;                                      // :247
			const uint32_t *const F = W + w0;                                // the final CIGAR, m words
			int32_t *const CP = LR;
			// prefixes of the final words on both sequences and in columns: one per base of M, I and D, one for an N word and for an empty I or D
			int n_cols, n_M, sum_M, sum_ID;
			{
				int cq2 = 0, ct2 = 0, cc = 0, nm = 0, sm = 0, sid = 0;
				for (int base = 0; base < m; base += 64) {
					const int k = base + lane;
					const bool on = k < m;
					const uint32_t w = on ? F[k] : 0u, op = w & 0xf;
					const int len = (int)(w >> 4);
					const int dq = on && op <= 1 ? len : 0, dt = on && op != 1 ? len : 0;
					const int dc = !on ? 0 : op == 0 ? len : op == 3 ? 1 : (len > 0 ? len : 1);
					const int iq = wave_incl_sum(dq, lane), it = wave_incl_sum(dt, lane), ic = wave_incl_sum(dc, lane);
					__syncthreads();                                         // QP, TP of the words in front of w0 + k are not read any more
					if (on) { QP[k] = cq2 + iq - dq; TP[k] = ct2 + it - dt; CP[k] = cc + ic - dc; }
					cq2 += __shfl(iq, 63); ct2 += __shfl(it, 63); cc += __shfl(ic, 63);
					nm += on && op == 0; sm += on && op == 0 ? len : 0; sid += on && (op == 1 || op == 2) ? len : 0;
					if (!A.is_eqx && on && k < room) out[k] = w;
				}
				n_cols = cc; n_M = wave_sum(nm); sum_M = wave_sum(sm); sum_ID = wave_sum(sid);
			}
			__syncthreads();
			// :249-282 and :175-193,210-234 over the columns
			int n_amb = 0, n_nm = 0, n_eqx = 0;
			int cT = 0, cC = XNEG, cP = XNEG, cM = XNEG;
			int carry_eq = 0, carry_ev = 0, carry_ls = -1;
			for (int base = 0; base < n_cols; base += 64) {
				const int c = base + lane;
				const bool on = c < n_cols;
				int tT = 0, tC = XNEG, tP = XNEG, tM = XNEG;
				int eq = 0, op = 4, j = 0, len = 0;
				uint32_t word = 0;
				if (on) {
					const int w = x_word_of(CP, m, c);
					word = F[w]; op = (int)(word & 0xf); len = (int)(word >> 4); j = c - CP[w];
					if (op == 0) {
						const int cq = qs[QP[w] + j], ct = ts[TP[w] + j];
						const bool amb = cq > 3 || ct > 3;
						n_amb += amb; n_nm += amb || cq != ct;
						eq = cq == ct;
						const int d = mat[(ct > 4 ? 4 : ct) * 5 + (cq > 4 ? 4 : cq)];
						tT = d; tC = 0; tP = d;
					} else if (op == 1 || op == 2) {
						if (j < len) n_amb += (op == 1 ? qs[QP[w] + j] : ts[TP[w] + j]) > 3;
						if (j == (len > 0 ? len : 1) - 1) { tT = -(A.q + A.e * len); tC = 0; }   // :268-269: the gap clamps, max stays
					}
				}
				for (int d = 1; d < 64; d <<= 1) {                           // the step's columns in order: lane l holds l .. l + 2 d - 1
					const int oT = __shfl_down(tT, d), oC = __shfl_down(tC, d), oP = __shfl_down(tP, d), oM = __shfl_down(tM, d);
					if (lane + d < 64) {
						const int nP = tT + oP, nM = tC + oP, nC = tC + oT;
						tP = tP > nP ? tP : nP; if (tP < XNEG) tP = XNEG;
						tM = tM > nM ? tM : nM; tM = tM > oM ? tM : oM; if (tM < XNEG) tM = XNEG;
						tC = nC > oC ? nC : oC; if (tC < XNEG) tC = XNEG;
						tT += oT;
					}
				}
				{
					const int oT = __shfl(tT, 0), oC = __shfl(tC, 0), oP = __shfl(tP, 0), oM = __shfl(tM, 0);
					const int nP = cT + oP, nM = cC + oP, nC = cC + oT;
					cP = cP > nP ? cP : nP; if (cP < XNEG) cP = XNEG;
					cM = cM > nM ? cM : nM; cM = cM > oM ? cM : oM; if (cM < XNEG) cM = XNEG;
					cC = nC > oC ? nC : oC; if (cC < XNEG) cC = XNEG;
					cT += oT;
				}
				if (A.is_eqx) {
					int eq_prev = __shfl_up(eq, 1);
					if (lane == 0) eq_prev = carry_eq;
					const bool sev = on && (op != 0 ? j == 0 : (j == 0 || eq != eq_prev));   // the column at which an output word begins
					const bool rs = sev && op == 0;
					n_eqx += rs;
					const int ev = carry_ev + wave_incl_sum((int)sev, lane);
					int ls = wave_incl_max(rs ? c : -1, lane);
					if (ls < carry_ls) ls = carry_ls;
					int ls_ex = __shfl_up(ls, 1);
					if (lane == 0) ls_ex = carry_ls;
					if (on && op != 0 && j == 0 && ev - 1 < room) out[ev - 1] = word;
					if (rs && j > 0 && ev - 2 < room) out[ev - 2] = (uint32_t)(c - ls_ex) << 4 | (eq ? 8u : 7u);      // the run in front of this one ends here
					if (on && op == 0 && j == len - 1 && ev - 1 < room) out[ev - 1] = (uint32_t)(c - ls + 1) << 4 | (eq ? 7u : 8u);
					carry_eq = __shfl(eq, 63); carry_ev = __shfl(ev, 63); carry_ls = __shfl(ls, 63);
				}
			}
			n_amb = wave_sum(n_amb); n_nm = wave_sum(n_nm); n_eqx = wave_sum(n_eqx);
			int dp_max = 0;
			if (cP > dp_max) dp_max = cP;
			if (cM > dp_max) dp_max = cM;
			const int n_out = A.is_eqx ? carry_ev : m;
			if (A.is_eqx && n_eqx == n_M) {                                  // :195-201: in place, every M word becomes `=`
				__syncthreads();
				const int lim = n_out < room ? n_out : (int)room;
				for (int k = lane; k < lim; k += 64) { const uint32_t w = out[k]; if ((w & 0xf) == 8) out[k] = (w & ~0xfu) | 7u; }
			}
			const int status = n_out > room ? EXTRA_CIGAR_CUT : 0;
			if (lane == 0) {
				if (status) atomicAdd(&A.flags[2], 1);
				A.res[i] = ExtraRes{n_out, qshift, tshift, sum_M + sum_ID - n_amb, sum_M - n_nm, n_amb, dp_max, status};
			}
		}
	}
}

__global__ __launch_bounds__(64) void extra_zdrop(const ExtraArgs A)
{
	__shared__ uint32_t lds[4 * EXTRA_LDS_WORDS];
	__shared__ int32_t mat[25];
	const int lane = (int)threadIdx.x;
	if (lane < 25) mat[lane] = A.mat[lane];

	for (int64_t i = blockIdx.x; i < A.n; i += gridDim.x) {
		__syncthreads();
		const KswRes R = A.kres[i];
		const KswTask T = A.ktasks[i];
		const int n = R.n_cigar;
		const int64_t c0 = A.cig_off[i], c1 = A.cig_off[i + 1];
		bool bad = R.status != 0 || n < 0 || c0 < 0 || c1 < c0 || c1 > A.in_cap || n > c1 - c0 || T.qlen > KSW_MAX_LEN || T.tlen > KSW_MAX_LEN;
		if (!bad && n > 0) bad = T.qlen < 0 || T.tlen < 0 || T.q_off < 0 || T.t_off < 0 || T.q_off > A.seq_cap - T.qlen || T.t_off > A.seq_cap - T.tlen;
		if (bad) {                                                           // also a task the ksw plan refused, did not run or cut
			if (lane == 0) { A.zres[i].status = EXTRA_REFUSED; atomicAdd(&A.flags[0], 1); }
			continue;
		}
		const XWork X = x_work(lds, A, n);
		if (n > 0 && X.W == nullptr) {
			if (lane == 0) { A.zres[i].status = EXTRA_TOO_BIG; atomicAdd(&A.flags[1], 1); }
			continue;
		}
		uint32_t *const W = X.W;
		int32_t *const IP = X.A, *const JP = X.B, *const CP = X.C;
		const uint8_t *const qs = A.seq + T.q_off, *const ts = A.seq + T.t_off;
		const uint32_t *const in = A.kcigar + c0;
		int n_cols;
		{
			int64_t si = 0, sj = 0;
			uint32_t ci = 0, cj = 0;
			int cc = 0;
			for (int base = 0; base < n; base += 64) {
				const int k = base + lane;
				const bool on = k < n;
				const uint32_t w = on ? in[k] : 0u, op = w & 0xf, len = w >> 4;
				if (on) W[k] = w;
				const uint32_t di = on && (op == 0 || op == 2 || op == 3) ? len : 0u, dj = on && op <= 1 ? len : 0u;
				const int dc = !on ? 0 : op == 0 ? (int)len : op <= 3 ? 1 : 0;     // a point per base of M and per gap word; other ops are passed over as at :56,62
				si += di; sj += dj;
				const uint32_t ii = (uint32_t)wave_incl_sum((int)di, lane), ij = (uint32_t)wave_incl_sum((int)dj, lane);
				const int ic = wave_incl_sum(dc, lane);
				if (on) { IP[k] = (int32_t)(ci + ii - di); JP[k] = (int32_t)(cj + ij - dj); CP[k] = cc + ic - dc; }
				ci += (uint32_t)__shfl((int)ii, 63); cj += (uint32_t)__shfl((int)ij, 63); cc += __shfl(ic, 63);
			}
			si = wave_sum(si); sj = wave_sum(sj);
			if (si > T.tlen || sj > T.qlen) {                                // the walk would leave the sequences
				if (lane == 0) { A.zres[i].status = EXTRA_REFUSED; atomicAdd(&A.flags[0], 1); }
				continue;
			}
			n_cols = cc;
		}
		__syncthreads();
		int carry_s = 0, mv = INT32_MIN, mi = -1, mj = -1;                   // :50
		int best = 0, b_t0 = -1, b_t1 = -1, b_q0 = -1, b_q1 = -1;
		for (int base = 0; base < n_cols; base += 64) {
			const int c = base + lane;
			const bool on = c < n_cols;
			int d = 0, pi = -1, pj = -1;
			if (on) {
				const int w = x_word_of(CP, n, c);
				const uint32_t word = W[w], op = word & 0xf;
				const int len = (int)(word >> 4), j = c - CP[w];
				if (op == 0) {
					pi = IP[w] + j; pj = JP[w] + j;
					const int ct = ts[pi], cq = qs[pj];
					d = mat[(ct > 4 ? 4 : ct) * 5 + (cq > 4 ? 4 : cq)];
				} else {
					d = -(A.q + A.e * len);
					pi = IP[w] + (op == 1 ? 0 : len); pj = JP[w] + (op == 1 ? len : 0);
				}
			}
			const int S = carry_s + wave_incl_sum(d, lane);
			int v = on ? S : INT32_MIN, vi = pi, vj = pj;                    // the inclusive maximum, the later point winning a tie (:34,44)
			for (int dd = 1; dd < 64; dd <<= 1) {
				const int ov = __shfl_up(v, dd), oi = __shfl_up(vi, dd), oj = __shfl_up(vj, dd);
				if (lane >= dd && ov > v) { v = ov; vi = oi; vj = oj; }
			}
			if (mv > v) { v = mv; vi = mi; vj = mj; }                        // what came in front of this step loses a tie against it
			int xv = __shfl_up(v, 1), xi = __shfl_up(vi, 1), xj = __shfl_up(vj, 1);
			if (lane == 0) { xv = mv; xi = mi; xj = mj; }
			int z = -1;
			if (on && S < xv) {
				const int li = pi - xi, lj = pj - xj, diff = li > lj ? li - lj : lj - li;
				z = xv - S - diff * A.e;
			}
			int bz = z, bl = lane;                                           // the largest z of the step, the earliest lane among equals
			for (int m2 = 32; m2 > 0; m2 >>= 1) {
				const int oz = __shfl_xor(bz, m2), ol = __shfl_xor(bl, m2);
				if (oz > bz || (oz == bz && ol < bl)) { bz = oz; bl = ol; }
			}
			if (bz > best) {                                                 // strict: the earlier step keeps an equal drop
				best = bz; b_t0 = __shfl(xi, bl); b_t1 = __shfl(pi, bl); b_q0 = __shfl(xj, bl); b_q1 = __shfl(pj, bl);
			}
			carry_s = __shfl(S, 63); mv = __shfl(v, 63); mi = __shfl(vi, 63); mj = __shfl(vj, 63);
		}
		if (lane == 0) {
			const int inv = !A.zo.no_inv && best > A.zo.zdrop_inv && b_q1 - b_q0 < A.zo.max_gap && b_t1 - b_t0 < A.zo.max_gap;
			A.zres[i] = ZdropRes{best, b_t0, b_t1, b_q0, b_q1, best > A.zo.zdrop ? 1 : 0, inv, 0};
		}
	}
}

static unsigned extra_grid(const ExtraArgs &A) { return (unsigned)(A.n < A.n_slots ? A.n : A.n_slots); }

hipError_t launch_extra_update(const ExtraArgs &A, hipStream_t st)
{
	if (A.n <= 0) return hipSuccess;
	hipLaunchKernelGGL(extra_update, dim3(extra_grid(A)), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_extra_zdrop(const ExtraArgs &A, hipStream_t st)
{
	if (A.n <= 0) return hipSuccess;
	hipLaunchKernelGGL(extra_zdrop, dim3(extra_grid(A)), dim3(64), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
