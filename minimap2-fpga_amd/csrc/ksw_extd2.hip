// ksw_extd2.hip -- ksw_extd2_sse (ksw2_extd2_sse.c: the dual-affine banded DP behind mm_align_pair, align.c:313-339) for a batch of independent tasks, byte for
// byte the reference's SSE4.1 build.  The function's results depend on its 16-byte blocks, so the kernel keeps the reference's array image -- u, v, x, y, x2, y2, s
// as bytes by absolute t, sf, qr, and H as 32-bit words -- and walks the same padded ranges (DESIGN 3.17 has the rules and where each shows).
//
// ksw_rows: one wave per task slot, a persistent grid over the slots: block b runs tasks b, b + gridDim.x, ... one after the other in slot b of the plan's scratch.
// A row (anti-diagonal r) is walked in chunks of 64 lanes over t of the padded range; the left neighbour of x, v, x2 comes from the lane below, and across chunks
// from the last lane's old value (the `x1_`, `v1_`, `x21_` carries of the reference).  One p byte per cell goes to the slot, row pitch n_col_ * 16 as :94.
// The same wave then backtracks on lane 0, run-length encodes into the slot, and all lanes copy the CIGAR into the task's words, reversed unless REV_CIGAR.
// Stores are plain vector stores; the only atomics are the adds of the three refusal counters; every loop's bound is known at its entry.
#include "ksw_extd2.h"

namespace mm2c {

constexpr int KSW_NEG_INF = -0x40000000;

struct KswSizes {
	int64_t off_at, cig_at, img_at, need;  // p lies at 0
	int64_t cig_words;
	int32_t pitch, T16;
	bool lds;
};

__host__ __device__ static inline KswSizes ksw_sizes(int32_t qlen, int32_t tlen, int32_t w, int32_t flag)
{
	KswSizes z;
	const int64_t rows = (int64_t)qlen + tlen - 1;
	const int64_t wide = qlen > tlen ? qlen : tlen, narrow = qlen < tlen ? qlen : tlen;
	const int64_t w1 = (w < 0 ? wide : (int64_t)w) + 1;
	z.T16 = (tlen + 15) / 16 * 16;
	z.pitch = (int32_t)(((narrow < w1 ? narrow : w1) + 15) / 16 + 1) * 16;
	const bool with_cigar = !(flag & 0x01);
	z.off_at = with_cigar ? rows * z.pitch : 0;
	z.cig_at = z.off_at + (with_cigar ? rows * 8 : 0);
	z.cig_words = with_cigar ? rows + 4 : 0;
	z.img_at = (z.cig_at + z.cig_words * 4 + 15) & ~(int64_t)15;
	z.lds = z.T16 <= KSW_LDS_T16 && qlen <= KSW_LDS_Q;
	z.need = z.img_at + (z.lds ? 0 : (int64_t)12 * z.T16 + 32 + ((qlen + 16 + 15) & ~15));
	return z;
}

int64_t ksw_slot_need(int32_t qlen, int32_t tlen, int32_t w, int32_t flag)
{
	if (qlen <= 0 || tlen <= 0) return 0;
	return ksw_sizes(qlen, tlen, w, flag).need;
}

__device__ static inline int w8(int v) { return (int)(int8_t)v; }           // the wrap of an epi8 operation
__device__ static inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ static inline int ksw_edge(const KswScore &S, int r)            // :158,162
{
	return r == 0 ? w8(-S.q - S.e) : r < S.long_thres ? w8(-S.e) : r == S.long_thres ? w8(S.long_diff) : w8(-S.e2);
}

struct KswEz { int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end; };

__device__ static inline bool ksw_zdrop(KswEz &ez, int32_t H, int r, int t, int zdrop, int e)     // ksw_apply_zdrop, ksw2.h:160-176, is_rot
{
	if (H > ez.max) { ez.max = H; ez.max_t = t; ez.max_q = r - t; }
	else if (t >= ez.max_t && r - t >= ez.max_q) {
		const int tl = t - ez.max_t, ql = (r - t) - ez.max_q, l = tl > ql ? tl - ql : ql - tl;
		if (zdrop >= 0 && ez.max - H > zdrop + l * e) { ez.zdropped = 1; return true; }
	}
	return false;
}

__global__ __launch_bounds__(64) void ksw_rows(const KswArgs A)
{
	__shared__ __attribute__((aligned(16))) char lds_img[12 * KSW_LDS_T16 + 32 + KSW_LDS_Q + 16];
	const int lane = (int)threadIdx.x;
	const KswScore S = A.sc;
	char *const slot = A.scratch + (int64_t)blockIdx.x * A.slot_bytes;
	const int nqe = w8(-S.q - S.e), nqe2 = w8(-S.q2 - S.e2), q_ = w8(S.q), q2_ = w8(S.q2), qe_ = w8(S.q + S.e), qe2_ = w8(S.q2 + S.e2);

	for (int64_t i = blockIdx.x; i < A.n_tasks; i += gridDim.x) {
		__syncthreads();                                                     // the task before this one has read its last byte of the image
		const KswTask T = A.tasks[i];
		const int qlen = T.qlen, tlen = T.tlen, flag = T.flag;
		const int64_t c0 = A.cig_off[i], c1 = A.cig_off[i + 1];
		bool bad = (flag & ~KSW_FLAGS) != 0 || qlen > KSW_MAX_LEN || tlen > KSW_MAX_LEN || c0 < 0 || c1 < c0 || c1 > A.cigar_cap;
		const bool empty = qlen <= 0 || tlen <= 0;
		if (!empty) bad = bad || T.q_off < 0 || T.t_off < 0 || T.q_off > A.seq_cap - qlen || T.t_off > A.seq_cap - tlen;
		if (bad) {                                                           // refused: its status and nothing else
			if (lane == 0) { A.res[i].status = KSW_REFUSED; atomicAdd(&A.flags[0], 1); }
			continue;
		}
		KswEz ez = {0, 0, -1, -1, KSW_NEG_INF, -1, KSW_NEG_INF, -1, KSW_NEG_INF, 0, 0};     // ksw_reset_extz
		int status = 0;
		if (empty || S.early) {                                              // the returns of :76 and :100
			if (lane == 0) A.res[i] = KswRes{0u, 0, -1, -1, KSW_NEG_INF, -1, KSW_NEG_INF, -1, KSW_NEG_INF, 0, 0, 0};
			continue;
		}
		const KswSizes Z = ksw_sizes(qlen, tlen, T.w, flag);
		if (Z.need > A.slot_bytes) {
			if (lane == 0) { A.res[i].status = KSW_TOO_BIG; atomicAdd(&A.flags[1], 1); }
			continue;
		}
		const int T16 = Z.T16, pitch = Z.pitch;
		const bool with_cigar = !(flag & 0x01), right = (flag & 0x02) != 0, approx = (flag & 0x08) != 0;
		const int w = T.w < 0 ? (tlen > qlen ? tlen : qlen) : T.w;
		char *const img = Z.lds ? lds_img : slot + Z.img_at;
		int32_t *const H = (int32_t *)img;                                   // [H | u v x y x2 y2 | s (+16) | sf (+16) | qr (+16)]
		int8_t *const u = (int8_t *)img + (size_t)4 * T16, *const v = u + T16, *const x = v + T16, *const y = x + T16, *const x2 = y + T16, *const y2 = x2 + T16;
		int8_t *const s = y2 + T16;
		uint8_t *const sf = (uint8_t *)s + T16 + 16, *const qr = sf + T16 + 16;
		uint8_t *const p = (uint8_t *)slot;
		int2 *const offs = (int2 *)(slot + Z.off_at);
		uint32_t *const ctmp = (uint32_t *)(slot + Z.cig_at);
		const uint8_t *const qs = A.seq + T.q_off, *const ts = A.seq + T.t_off;

		for (int t = lane; t < T16; t += 64) {                               // :111-120
			u[t] = v[t] = x[t] = y[t] = (int8_t)nqe; x2[t] = y2[t] = (int8_t)nqe2; H[t] = KSW_NEG_INF;
		}
		for (int t = lane; t < T16 + 16; t += 64) { s[t] = 0; sf[t] = t < tlen ? ts[t] : (uint8_t)0; }
		for (int t = lane; t < qlen + 16; t += 64) qr[t] = t < qlen ? qs[qlen - 1 - t] : (uint8_t)0;
		__syncthreads();

		int32_t H0 = 0, last_H0_t = 0;
		int last_st = -1, last_en = -1;
		const int rows = qlen + tlen - 1;
		for (int r = 0; r < rows; ++r) {
			int st = 0, en = tlen - 1;
			if (st < r - qlen + 1) st = r - qlen + 1;
			if (en > r) en = r;
			if (st < (r - w + 1) >> 1) st = (r - w + 1) >> 1;
			if (en > (r + w) >> 1) en = (r + w) >> 1;
			if (st > en) { ez.zdropped = 1; break; }
			const int st0 = st, en0 = en;
			st = st / 16 * 16; en = (en + 16) / 16 * 16 - 1;                 // en < T16
			int x1, x21, v1;
			if (st > 0) {
				if (st - 1 >= last_st && st - 1 <= last_en) { x1 = uni(x[st - 1]); x21 = uni(x2[st - 1]); v1 = uni(v[st - 1]); }
				else { x1 = nqe; x21 = nqe2; v1 = nqe; }
			} else { x1 = nqe; x21 = nqe2; v1 = ksw_edge(S, r); }
			if (en >= r && lane == 0) { y[r] = (int8_t)nqe; y2[r] = (int8_t)nqe2; u[r] = (int8_t)ksw_edge(S, r); }     // r <= en < T16
			{	// s[] in chunks of 16 from the unaligned st0 (:166-180): up to st0 + 16 k + 15 <= tlen + 14 < T16 + 16
				const int hi = st0 + (en0 - st0) / 16 * 16 + 16, qo = qlen - 1 - r;    // qo + t >= 0 from st0 on, <= qlen + 14
				for (int t = st0 + lane; t < hi; t += 64) {
					const int a = sf[t], b = qr[qo + t];
					s[t] = (int8_t)((a == 4 || b == 4) ? S.sc_n : a == b ? S.mch : S.mis);
				}
			}
			__syncthreads();
			if (with_cigar && lane == 0) offs[r] = make_int2(st, en);
			uint8_t *const prow = p + (int64_t)r * pitch;
			for (int base = st; base <= en; base += 64) {
				const int t = base + lane;
				const bool on = t <= en;
				int z = 0, xo = 0, vo = 0, x2o = 0, ut = 0, yo = 0, y2o = 0;
				if (on) { z = s[t]; xo = x[t]; vo = v[t]; x2o = x2[t]; ut = u[t]; yo = y[t]; y2o = y2[t]; }
				int xl = __shfl_up(xo, 1), vl = __shfl_up(vo, 1), x2l = __shfl_up(x2o, 1);
				if (lane == 0) { xl = x1; vl = v1; x2l = x21; }
				x1 = __shfl(xo, 63); v1 = __shfl(vo, 63); x21 = __shfl(x2o, 63);
				int a = w8(xl + vl), b = w8(yo + ut), a2 = w8(x2l + vl), b2 = w8(y2o + ut), d;
				if (!right) {
					d = a > z ? 1 : 0; z = z > a ? z : a;
					d = b > z ? 2 : d; z = z > b ? z : b;
					d = a2 > z ? 3 : d; z = z > a2 ? z : a2;
					d = b2 > z ? 4 : d; z = z > b2 ? z : b2;
				} else {
					d = z > a ? 0 : 1; z = z > a ? z : a;
					d = z > b ? d : 2; z = z > b ? z : b;
					d = z > a2 ? d : 3; z = z > a2 ? z : a2;
					d = z > b2 ? d : 4; z = z > b2 ? z : b2;
				}
				z = z < S.mch ? z : S.mch;
				const int un = w8(z - vl), vn = w8(z - ut);
				int tmp = w8(z - q_);
				a = w8(a - tmp); b = w8(b - tmp);
				tmp = w8(z - q2_);
				a2 = w8(a2 - tmp); b2 = w8(b2 - tmp);
				if (!right) d |= (a > 0 ? 0x08 : 0) | (b > 0 ? 0x10 : 0) | (a2 > 0 ? 0x20 : 0) | (b2 > 0 ? 0x40 : 0);
				else d |= (a >= 0 ? 0x08 : 0) | (b >= 0 ? 0x10 : 0) | (a2 >= 0 ? 0x20 : 0) | (b2 >= 0 ? 0x40 : 0);
				if (on) {
					u[t] = (int8_t)un; v[t] = (int8_t)vn;
					x[t] = (int8_t)((a > 0 ? a : 0) - qe_); y[t] = (int8_t)((b > 0 ? b : 0) - qe_);
					x2[t] = (int8_t)((a2 > 0 ? a2 : 0) - qe2_); y2[t] = (int8_t)((b2 > 0 ? b2 : 0) - qe2_);
					if (with_cigar && t - st < pitch) prow[t - st] = (uint8_t)d;
				}
			}
			__syncthreads();
			if (!approx) {                                                   // the exact maximum, :326-366
				int32_t max_H, max_t, hen0, hst0;
				if (r > 0) {
					hen0 = uni(en0 > 0 ? H[en0 - 1] + u[en0] : H[0] + v[0]);    // from the old H[en0 - 1]
					__syncthreads();
					hst0 = hen0;
					const int en1 = st0 + (en0 - st0) / 4 * 4;
					int32_t bh = hen0, bk = -1;                              // H[en0] wins every tie; then the four lanes in lane order, then the tail
					for (int base = st0; base < en0; base += 64) {
						const int t = base + lane;
						int32_t h = 0;
						if (t < en0) {
							h = H[t] + v[t]; H[t] = h;
							const int32_t key = (t < en1 ? ((t - st0) & 3) << 28 : 4 << 28) | t;
							if (h > bh || (h == bh && key < bk)) { bh = h; bk = key; }
						}
						if (base == st0) hst0 = __shfl(h, 0);
					}
					if (lane == 0) H[en0] = hen0;
					for (int m = 32; m > 0; m >>= 1) {
						const int32_t oh = __shfl_xor(bh, m), ok = __shfl_xor(bk, m);
						if (oh > bh || (oh == bh && ok < bk)) { bh = oh; bk = ok; }
					}
					max_H = uni(bh); bk = uni(bk);
					max_t = bk < 0 ? en0 : bk & 0x0fffffff;
				} else {
					hen0 = hst0 = max_H = uni((int)v[0]) - S.qe0; max_t = 0;
					if (lane == 0) H[0] = max_H;
				}
				if (en0 == tlen - 1 && hen0 > ez.mte) { ez.mte = hen0; ez.mte_q = r - en; }
				if (r - st0 == qlen - 1 && hst0 > ez.mqe) { ez.mqe = hst0; ez.mqe_t = st0; }
				if (ksw_zdrop(ez, max_H, r, max_t, T.zdrop, S.e2)) break;
				if (r == rows - 1 && en0 == tlen - 1) ez.score = hen0;
			} else {                                                         // the approximate maximum, :368-382
				if (r > 0) {
					const bool in0 = last_H0_t >= st0 && last_H0_t <= en0, in1 = last_H0_t + 1 >= st0 && last_H0_t + 1 <= en0;
					if (in0 && in1) {
						const int d0 = uni(v[last_H0_t]), d1 = uni(u[last_H0_t + 1]);
						if (d0 > d1) H0 += d0;
						else { H0 += d1; ++last_H0_t; }
					} else if (in0) H0 += uni(v[last_H0_t]);
					else { ++last_H0_t; H0 += uni(u[last_H0_t < T16 ? last_H0_t : T16 - 1]); }
				} else { H0 = uni((int)v[0]) - S.qe0; last_H0_t = 0; }
				if ((flag & 0x10) && ksw_zdrop(ez, H0, r, last_H0_t, T.zdrop, S.e2)) break;
				if (r == rows - 1 && en0 == tlen - 1) ez.score = H0;
			}
			last_st = st; last_en = en;
			__syncthreads();
		}

		if (with_cigar) {                                                    // :389-399 and ksw_backtrack, ksw2.h:119-151, is_rot
			int bi = -1, bj = -1;
			if (!ez.zdropped && !(flag & 0x40)) { bi = tlen - 1; bj = qlen - 1; }
			else if (!ez.zdropped && (flag & 0x40) && ez.mqe + T.end_bonus > ez.max) { ez.reach_end = 1; bi = ez.mqe_t; bj = qlen - 1; }
			else if (ez.max_t >= 0 && ez.max_q >= 0) { bi = ez.max_t; bj = ez.max_q; }
			__syncthreads();                                                 // every p byte and off pair is written
			int n = 0;
			if (lane == 0 && bi >= 0 && bj >= 0) {
				int ii = bi, jj = bj, state = 0, cur_op = -1, cur_len = 0;
				const int64_t cap = Z.cig_words;
				for (int step = qlen + tlen; step > 0 && ii >= 0 && jj >= 0; --step) {   // every step takes one off ii or jj
					const int r = ii + jj;                                   // <= the last row made
					const int2 o = offs[r];
					int force = -1;
					if (ii < o.x) force = 2;
					if (ii > o.y) force = 1;
					const int tmp = force < 0 ? p[(int64_t)r * pitch + (ii - o.x)] : 0;   // ii - o.x <= en - st < pitch
					if (state == 0) state = tmp & 7;
					else if (!(tmp >> (state + 2) & 1)) state = 0;
					if (state == 0) state = tmp & 7;
					if (force >= 0) state = force;
					int op;
					if (state == 0) { op = 0; --ii; --jj; }
					else if (state == 1 || state == 3) { op = 2; --ii; }
					else { op = 1; --jj; }
					if (op == cur_op) ++cur_len;
					else { if (cur_op >= 0) { if (n < cap) ctmp[n] = (uint32_t)cur_len << 4 | cur_op; ++n; } cur_op = op; cur_len = 1; }
				}
				for (int k = 0; k < 2; ++k) {                                // the first deletion, then the first insertion
					const int len = k == 0 ? ii + 1 : jj + 1, op = k == 0 ? 2 : 1;
					if (len <= 0) continue;
					if (op == cur_op) cur_len += len;
					else { if (cur_op >= 0) { if (n < cap) ctmp[n] = (uint32_t)cur_len << 4 | cur_op; ++n; } cur_op = op; cur_len = len; }
				}
				if (cur_op >= 0) { if (n < cap) ctmp[n] = (uint32_t)cur_len << 4 | cur_op; ++n; }
			}
			n = __shfl(n, 0);
			__syncthreads();
			ez.n_cigar = n;
			const int64_t room = c1 - c0;
			const int nw = n < room ? n : (int)room;
			const bool rev = (flag & 0x80) != 0;
			for (int k = lane; k < nw; k += 64) A.cigar[c0 + k] = ctmp[rev ? k : n - 1 - k];
			if (n > room) { status = KSW_CIGAR_CUT; if (lane == 0) atomicAdd(&A.flags[2], 1); }
		}
		if (lane == 0)
			A.res[i] = KswRes{(uint32_t)ez.max, ez.zdropped, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score, ez.n_cigar, ez.reach_end, status};
	}
}

hipError_t launch_ksw_rows(const KswArgs &A, hipStream_t st)
{
	if (A.n_tasks <= 0) return hipSuccess;
	const unsigned grid = (unsigned)(A.n_tasks < A.n_slots ? A.n_tasks : A.n_slots);
	hipLaunchKernelGGL(ksw_rows, dim3(grid), dim3(64), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
