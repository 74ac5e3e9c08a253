// chain_esterr.hip -- mm_est_err (map.c:357, esterr.c) on the GPU, up to the one call of pow: per final region the two integers n_match and n_tot of
// esterr.c:53-61, per read the float avg_k of esterr.c:37-39.  r->div = n_match >= n_tot ? 0 : 1 - pow(n_match / n_tot, 1 / avg_k) stays where the libm is
// (mm2c_est_err_div, mm2chain_esterr.cpp).  Regions and anchors are read-only input: the final regions and the squeezed a[] of the mapq plan (chain_mapq.hip).
//
// Everything is as written in esterr.c: int32_t arithmetic wraps; positions compare as (int32_t)mini_pos[j]; get_for_qpos turns by the strand bit of the anchor
// itself; r->rev chooses the walk direction (walk anchor k is a[as + k], or a[as + cnt - 1 - k]); the second flank test reads qlen - r->qs; the int-against-float
// compares convert the int.  Built with -ffp-contract=off.
//
// The walk of esterr.c:53-58 is not run as a loop.  mini_pos of a one-segment read increases strictly (mm_sketch emits at most one minimizer per position), and
// then, with pos_k the forward query position of walk anchor k: anchor k >= 1 is matched iff every 1 <= k' <= k has pos_k' in mini_pos and pos_k' > pos_(k'-1);
// n_match is 1 + the length of that prefix, en the index of its last anchor in mini_pos.  tests/esterr_model.py holds both forms and the test that they agree.
// So every anchor is tested on its own, and a region keeps the smallest k that fails.
//
// err_reads, one workgroup of four waves per read: checks the offsets; all four waves sum the spans and test the strict increase of mini_pos in one pass (a long
//   read has 10^5 minimizers and only a few hundred such reads fill a batch: one wave would wait for its own loads); the first wave then checks every region's
//   [as, as + cnt) and rid, and only then writes: avg_k, the read's table of (as, cnt, region, rev) over the regions with cnt > 0 in ascending as, and first_fail = cnt per
//   region.  The table is ranked by counting, lane-parallel over the regions: a read has few regions behind mm_select_sub (mapq_join ranks the same way).
//   A read without mini_pos (esterr.c:36) gets n_match = -1 in all its regions and nothing else.
// err_walk, anchor-parallel over slices of ERR_SLICE positions of the b index space, as mapq_gather is and for its reason: one uniform search in b_off finds the
//   slice's first read; a lane finds its region in the read's table (none while its next position lies in the region it found last) and from it its k; it loads
//   its anchor and its walk predecessor, neighbours in memory, 16 bytes each, and searches the read's mini_pos once.  A failing k goes to first_fail by an integer
//   atomicMin: one per wave when the failing lanes of the wave share a region (the common case, a wave covers 64 neighbours), one per failing lane otherwise.
//   Anchors that no region covers are skipped.  The search in b_off needs sound offsets; when err_reads refused a read the workgroups go read by read.
// err_finish, one wave per read, a lane per region: st is the search for pos_0 (absent: n_match = 0, div -1), n_match = first_fail, en the search for
//   pos_(n_match-1), then the two flank tests and the store.
// Ordering between the kernels is the stream's.  Plain vector stores; the only atomics are the atomicMin above and the integer add of the refusal counter.
// Every loop has a bound known at entry.
//
// Precondition (the mapq plan guarantees it): the regions of a read do not overlap in a[].  Where they do, an anchor counts for one of them only and the
// counts of the others are unspecified; nothing is read outside the read's anchors and mini_pos either way.

#include <hip/hip_runtime.h>
#include <climits>
#include "chain_esterr.h"
#include "chain_regs.h"
#include "wave_ops.h"

namespace mm2c {

namespace {

// get_for_qpos (esterr.c:7-14) on an anchor as four 32-bit words: x = .y << 32 | .x, y = .w << 32 | .z
__device__ __forceinline__ int32_t for_qpos(const int32_t qlen, const uint4 a)
{
	const uint32_t x = a.z, q_span = a.w & 0xffu;
	return a.y >> 31 ? (int32_t)((uint32_t)qlen - 1u - (x + 1u - q_span)) : (int32_t)x;
}

// get_mini_idx (esterr.c:16-28): at most 32 rounds
__device__ __forceinline__ int32_t mini_idx(const uint64_t *mp, const int32_t n, const int32_t x)
{
	int32_t L = 0, R = n - 1;
	while (L <= R) {
		const int32_t m = (int32_t)(((uint32_t)L + (uint32_t)R) >> 1);
		const int32_t y = (int32_t)mp[m];
		if (y < x) L = m + 1;
		else if (y > x) R = m - 1;
		else return m;
	}
	return -1;
}

__device__ __forceinline__ void refuse(const ErrArgs &A, const int r, const int lane)
{
	if (lane == 0) { atomicAdd(&A.flags[0], 1); A.state[r] = ERR_READ_BAD; }
}

__global__ __launch_bounds__(ERR_READS_LANES) void err_reads(ErrArgs A)
{
	__shared__ unsigned long long s_sum[ERR_READS_LANES / 64];
	__shared__ int s_bad[ERR_READS_LANES / 64];
	const int r = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
	const int64_t base = A.u_off[r], u1 = A.u_off[r + 1], bo = A.b_off[r], b1 = A.b_off[r + 1], mo = A.mini_off[r], m1 = A.mini_off[r + 1];
	const int64_t n64 = A.n_in[r];
	if (base < 0 || u1 < base || u1 > A.n_u_cap || u1 - base > INT_MAX || n64 < 0 || n64 > u1 - base || bo < 0 || b1 < bo || b1 > A.n_b_cap ||
	    mo < 0 || m1 < mo || m1 > A.n_mini_cap || m1 - mo > INT_MAX) {
		refuse(A, r, tid);                                                       // offsets that leave the capacities or each other: nothing of this read is touched
		return;
	}
	const int n = (int)n64;
	const int64_t bl = b1 - bo, ml = m1 - mo;
	const uint64_t *regs = A.regs + base * REG_WORDS;
	if (ml == 0) {                                                               // esterr.c:36: returns before it touches anything
		for (int i = tid; i < n; i += ERR_READS_LANES) A.err[base + i] = make_int2(-1, 0);
		if (tid == 0) { A.state[r] = ERR_READ_NO_MINI; A.avg_k[r] = 0.0f; }
		return;
	}
	// ---- esterr.c:37-38, and the strict increase the other kernels rely on: all the waves, four independent loads per lane and round; a lane's predecessor
	// is its neighbour's element (lane 0 loads it) ----
	const uint64_t *mp = A.mini_pos + mo;
	unsigned long long sum_k = 0;
	bool bad = false;
	for (int64_t i0 = 0; i0 < ml; i0 += 4 * ERR_READS_LANES) {
		uint64_t v[4], p0[4];
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const int64_t i = i0 + j * ERR_READS_LANES + tid;
			v[j] = i < ml ? mp[i] : 0;
			p0[j] = lane == 0 && i > 0 && i < ml ? mp[i - 1] : 0;
		}
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const int64_t i = i0 + j * ERR_READS_LANES + tid;
			const uint64_t up = __shfl_up((unsigned long long)v[j], 1), prev = lane == 0 ? p0[j] : up;
			if (i < ml) {
				sum_k += v[j] >> 32 & 0xff;
				if (i > 0) bad |= (int32_t)v[j] <= (int32_t)prev;
			}
		}
	}
	sum_k = wave_sum(sum_k);
	const bool wbad = __ballot(bad) != 0;
	if (lane == 0) { s_sum[tid >> 6] = sum_k; s_bad[tid >> 6] = wbad; }
	__syncthreads();
	sum_k = 0;
	bad = false;
	for (int w = 0; w < ERR_READS_LANES / 64; ++w) { sum_k += s_sum[w]; bad |= s_bad[w] != 0; }
	if (tid >= 64) return;                                                       // the regions are the first wave's: a read has few
	// ---- every region's anchors and reference sequence, before anything is read through them ----
	for (int i = lane; i < n; i += 64) {
		const uint64_t *g = regs + (int64_t)i * REG_WORDS;
		const int32_t cnt = reg_get<REG_CNT>(g), rid = reg_get<REG_RID>(g), as = reg_get<REG_AS>(g);
		bad |= cnt < 0 || as < 0 || (int64_t)as + cnt > bl || rid < 0 || rid >= A.n_ref;
	}
	if (__ballot(bad)) { refuse(A, r, lane); return; }
	// ---- the table in ascending as ----
	int nt = 0;
	for (int i0 = 0; i0 < n; i0 += 64) {
		const int i = i0 + lane;
		int32_t cnt = 0, as = 0, rev = 0;
		if (i < n) {
			const uint64_t *g = regs + (int64_t)i * REG_WORDS;
			cnt = reg_get<REG_CNT>(g); as = reg_get<REG_AS>(g); rev = reg_rev(g);
			A.first_fail[base + i] = cnt;
		}
		if (cnt > 0) {
			int rank = 0;
			for (int j = 0; j < n; ++j) {
				const uint64_t *h = regs + (int64_t)j * REG_WORDS;
				const int32_t cj = reg_get<REG_CNT>(h), aj = reg_get<REG_AS>(h);
				rank += cj > 0 && (aj < as || (aj == as && j < i));
			}
			A.tab[base + rank] = make_int4(as, cnt, i, rev);
		}
		nt += __popcll(__ballot(cnt > 0));
	}
	if (lane == 0) {
		A.state[r] = nt;
		A.avg_k[r] = (float)sum_k / (float)(int32_t)ml;                          // esterr.c:39: (float)sum_k / n
	}
}

// what a lane remembers between its positions, 256 apart: the read's mini_pos and qlen, and the table entry it found last
struct WalkMemo { int64_t r, tr; const uint64_t *mp; int32_t ml, qlen; int4 m; };

// one position q of read r (nt table entries): -> the region it fails in and its k, or k = INT_MAX
__device__ __forceinline__ void walk_one(const ErrArgs &A, const int64_t r, const int64_t bo, const int64_t q, const int nt, WalkMemo &memo, int64_t &reg, int &kf)
{
	if (!(memo.tr == r && memo.m.x <= q && q - memo.m.x < memo.m.y)) {
		if (nt <= 0) return;
		const int4 *tb = A.tab + A.u_off[r];
		int lo = 0, hi = nt - 1;                                                 // the last entry with as <= q
		while (lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if (tb[mid].x <= q) lo = mid; else hi = mid - 1;
		}
		memo.tr = r; memo.m = tb[lo];
		if (!(memo.m.x <= q && q - memo.m.x < memo.m.y)) return;                 // no region covers q
	}
	const int as = memo.m.x, cnt = memo.m.y, rev = memo.m.w, j = (int)(q - as);
	const int k = rev ? cnt - 1 - j : j;
	if (k == 0) return;                                                         // the first anchor is err_finish's
	if (memo.r != r) {
		const int64_t mo = A.mini_off[r];
		memo.r = r; memo.mp = A.mini_pos + mo; memo.ml = (int32_t)(A.mini_off[r + 1] - mo); memo.qlen = A.qlen[r];
	}
	const uint4 cur = A.b[bo + q], prv = A.b[bo + (rev ? q + 1 : q - 1)];         // k >= 1: the predecessor lies inside the region
	const int32_t x = for_qpos(memo.qlen, cur), xp = for_qpos(memo.qlen, prv);
	if (x > xp && mini_idx(memo.mp, memo.ml, x) >= 0) return;
	reg = A.u_off[r] + memo.m.z; kf = k;
}

// every lane of the wave arrives here; reg, kf: what walk_one left
__device__ __forceinline__ void post_fail(const ErrArgs &A, const int64_t reg, const int kf)
{
	const bool fail = kf != INT_MAX;
	const unsigned long long m = __ballot(fail);
	if (!m) return;
	const int64_t reg0 = __shfl(reg, __ffsll(m) - 1);
	if (__all(!fail || reg == reg0)) {
		const int mn = wave_min(kf);
		if ((threadIdx.x & 63) == 0) atomicMin(&A.first_fail[reg0], mn);
	} else if (fail) atomicMin(&A.first_fail[reg], kf);
}

__global__ __launch_bounds__(256) void err_walk(ErrArgs A)
{
	const int tid = (int)threadIdx.x;
	WalkMemo memo;
	memo.r = memo.tr = -1; memo.mp = nullptr; memo.ml = 0; memo.qlen = 0; memo.m = make_int4(0, 0, 0, 0);
	if (A.flags[0] != 0) {                                                       // some read was refused: b_off is not to be searched; read by read
		for (int64_t r = blockIdx.x; r < A.n_reads; r += gridDim.x) {
			const int nt = A.state[r];
			if (nt <= 0) continue;
			const int64_t bo = A.b_off[r], bl = A.b_off[r + 1] - bo;
			for (int64_t q0 = 0; q0 < bl; q0 += 256) {
				int64_t reg = -1;
				int kf = INT_MAX;
				if (q0 + tid < bl) walk_one(A, r, bo, q0 + tid, nt, memo, reg, kf);
				post_fail(A, reg, kf);
			}
		}
		return;
	}
	const int64_t end = A.b_off[A.n_reads];
	for (int64_t p0 = (int64_t)blockIdx.x * ERR_SLICE; p0 < end; p0 += (int64_t)gridDim.x * ERR_SLICE) {
		int64_t lo = 0, hi = A.n_reads - 1;                                      // the last read with b_off <= p0: the same in every lane
		while (lo < hi) {
			const int64_t mid = (lo + hi + 1) >> 1;
			if (A.b_off[mid] <= p0) lo = mid; else hi = mid - 1;
		}
		int64_t r = lo, bo = A.b_off[r], be = A.b_off[r + 1];
		for (int k = 0; k < ERR_SLICE / 256; ++k) {
			const int64_t p = p0 + k * 256 + tid;
			int64_t reg = -1;
			int kf = INT_MAX;
			if (p < end) {
				while (p >= be) { ++r; bo = be; be = A.b_off[r + 1]; }               // p < end = b_off[n_reads]: ends at a read that holds p
				if (p >= bo) walk_one(A, r, bo, p - bo, A.state[r], memo, reg, kf);   // (p < bo: in front of the batch's first anchor)
			}
			post_fail(A, reg, kf);
		}
	}
}

__global__ __launch_bounds__(64) void err_finish(ErrArgs A)
{
	const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
	if (A.state[r] < 0) return;                                                  // refused, or without mini_pos: err_reads has said what there is to say
	const int64_t base = A.u_off[r], bo = A.b_off[r], mo = A.mini_off[r];
	const int n = A.n_in[r];
	const int32_t ml = (int32_t)(A.mini_off[r + 1] - mo), qlen = A.qlen[r];
	const uint64_t *mp = A.mini_pos + mo;
	const float avg_k = A.avg_k[r];
	for (int i = lane; i < n; i += 64) {
		const uint64_t *g = A.regs + (base + i) * REG_WORDS;
		const int32_t cnt = reg_get<REG_CNT>(g), rid = reg_get<REG_RID>(g), qs = reg_get<REG_QS>(g), rs = reg_get<REG_RS>(g), re = reg_get<REG_RE>(g), as = reg_get<REG_AS>(g);
		const int rev = reg_rev(g);
		int2 e = make_int2(0, 0);                                                // esterr.c:44-51: div = -1
		if (cnt > 0) {
			const int32_t st = mini_idx(mp, ml, for_qpos(qlen, A.b[bo + as + (rev ? cnt - 1 : 0)]));
			if (st >= 0) {
				const int32_t n_match = A.first_fail[base + i];                      // 1 <= n_match <= cnt
				int32_t en = st;
				if (n_match > 1 && n_match <= cnt) en = mini_idx(mp, ml, for_qpos(qlen, A.b[bo + as + (rev ? cnt - n_match : n_match - 1)]));
				const int32_t l_ref = (int32_t)A.ref_len[rid];
				int32_t n_tot = (int32_t)((uint32_t)en - (uint32_t)st + 1u);
				if ((float)qs > avg_k && (float)rs > avg_k) ++n_tot;                 // esterr.c:60
				if ((float)(int32_t)((uint32_t)qlen - (uint32_t)qs) > avg_k && (float)(int32_t)((uint32_t)l_ref - (uint32_t)re) > avg_k) ++n_tot;   // esterr.c:61: qs
				e = make_int2(n_match, n_tot);
			}
		}
		A.err[base + i] = e;
	}
}

} // namespace

hipError_t launch_err_reads(const ErrArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(err_reads, dim3((unsigned)A.n_reads), dim3(ERR_READS_LANES), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_err_walk(const ErrArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0 || A.n_b_cap <= 0) return hipSuccess;
	const int64_t slices = (A.n_b_cap + ERR_SLICE - 1) / ERR_SLICE;
	hipLaunchKernelGGL(err_walk, dim3((unsigned)(slices < 2048 ? slices : 2048)), dim3(256), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_err_finish(const ErrArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(err_finish, dim3((unsigned)A.n_reads), dim3(64), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
