// chain_segs.hip -- mm_seg_gen (hit.c:373-427) on the GPU: the hits of a fragment of several segments (the hit plan's second mode, chain_hits.hip) and the
// fragment's chain anchors become, per segment, the chains u and anchors a that the reference hands to mm_gen_regs, in the CSR shape of the device epilogue.  The
// regions themselves are chain_regs.hip's, launched over that CSR by the plan (mm2chain_segs.cpp); seg_mark then sets seg_split and seg_id.
//
// A "segment read" is f * n_segs + s.  The reference walks the regions of a fragment in order and appends every anchor to the array of its segment
// (sid = bits 48-55 of y): the anchors of segment s are in (region, j) order, and chain i of the fragment leaves one chain of score[i] in every segment that holds
// one of its anchors (hit.c:399-401 squeezes the others out), in region order.
//
//   seg_walk<false> ("seg_count"), one wave per fragment: checks the offsets, then walks the regions in order, a row of 64 anchors at a time.  A row is counted by
//             one ballot per distinct sid among its lanes (a chain holds its segments in few runs, so the loop over the distinct ids is short; at most 64 rounds).
//             The running counts per segment are in LDS.  It refuses the fragment -- nothing of it is written, its segment reads are empty -- when an offset or
//             n_in leaves the capacities or each other, a region leaves the fragment's anchors, or an anchor has sid >= n_segs (the reference would write out of
//             bounds there).  Otherwise it leaves the chains and anchors per segment read, and the fragment's hash (and rep_len) once per segment.
//   offsets : two exclusive scans (rocPRIM) over the segment reads make su_off and sb_off; a refused fragment counts 0, so the CSR is sound for the plans behind.
//   seg_walk<true> ("seg_scatter"), the same walk again: an anchor's place is sb_off[f, s] + the segment's anchors in earlier regions and rows (the running count)
//             + its rank among the lanes of the same sid in its row (the ballot below its lane).  y is turned by hit.c:414 as the 64-bit subtraction it is, by the
//             anchor's own strand bit.  Behind a region's rows lane s writes the region's chain of segment s, if it holds one.
//   seg_mark, one wave per segment read: ORs seg_split (bit 15) and seg_id (bits 16-23) into the bit-field word of its regions.
//
// The walk is per fragment, not anchor-parallel over slices of b as mapq_gather and err_walk are: fragments of several segments are short-read fragments
// (n_segs > 1 only comes with -x sr), their chains hold tens of anchors, and a batch has as many waves as fragments; the running counts then give every place
// without a search.  Ordering between the kernels is the stream's.  Plain vector stores; the only atomics are integer adds of the refusal counters.  Every loop
// has a bound known at entry.

#include <hip/hip_runtime.h>
#include <climits>
#include <rocprim/device/device_scan.hpp>
#include "chain_segs.h"
#include "chain_regs.h"

namespace mm2c {

namespace {

template <bool WRITE>
__global__ __launch_bounds__(64) void seg_walk(SegArgs A)
{
	__shared__ int32_t s_row[SEG_MAX], s_na[SEG_MAX], s_nu[SEG_MAX];             // per segment: anchors of the region at hand / anchors / chains so far
	__shared__ int32_t s_fwd[SEG_MAX], s_rev[SEG_MAX];                           // hit.c:414: what y loses on either strand
	__shared__ int64_t s_uo[SEG_MAX], s_bo[SEG_MAX];                             // su_off, sb_off of the fragment's segment reads
	const int64_t f = blockIdx.x;
	const int lane = (int)threadIdx.x, n_segs = A.n_segs;
	const int64_t sr0 = f * n_segs;
	const int64_t base = A.u_off[f], u1 = A.u_off[f + 1], bo = A.b_off[f], b1 = A.b_off[f + 1], n64 = A.n_in[f];
	bool bad = false;
	if (WRITE) { if (A.state[f] < 0) return; }
	else bad = base < 0 || u1 < base || u1 > A.n_u_cap || u1 - base > INT_MAX || n64 < 0 || n64 > u1 - base || bo < 0 || b1 < bo || b1 > A.n_b_cap || b1 - bo > INT_MAX;
	const int n = bad ? 0 : (int)n64;
	const int64_t bl = b1 - bo;
	for (int s = lane; s < n_segs; s += 64) {
		s_row[s] = 0; s_na[s] = 0; s_nu[s] = 0;
		if (WRITE) { s_uo[s] = A.su_off[sr0 + s]; s_bo[s] = A.sb_off[sr0 + s]; }
	}
	if (WRITE && lane == 0) {                                                    // hit.c:379-381, in wrapping int
		const int32_t *ql = A.seg_len + sr0;
		uint32_t acc = 0, sum = 0;
		for (int s = 0; s < n_segs; ++s) sum += (uint32_t)ql[s];
		for (int s = 0; s < n_segs; ++s) {
			s_fwd[s] = (int32_t)acc;
			s_rev[s] = (int32_t)(sum - ((uint32_t)ql[s] + acc));
			acc += (uint32_t)ql[s];
		}
	}
	__syncthreads();
	const uint64_t lt = (1ull << lane) - 1;
	int64_t sum_cnt = 0;
	for (int i = 0; i < n && !bad; ++i) {
		const uint64_t *g = A.regs + (base + i) * REG_WORDS;
		const int32_t cnt = reg_get<REG_CNT>(g), score = reg_get<REG_SCORE>(g), as = reg_get<REG_AS>(g);
		if (!WRITE) {
			sum_cnt += cnt > 0 ? cnt : 0;
			if (cnt < 0 || as < 0 || (int64_t)as + cnt > bl || sum_cnt > bl) { bad = true; break; }   // a region that leaves the fragment's anchors, or more than it has
		}
		for (int j0 = 0; j0 < cnt; j0 += 64) {
			const int j = j0 + lane;
			const bool valid = j < cnt;
			uint4 a = make_uint4(0, 0, 0, 0);
			if (valid) a = A.b[bo + as + j];
			const int sid = (int)(a.w >> 16 & 0xff);                                // (y & MM_SEED_SEG_MASK) >> MM_SEED_SEG_SHIFT
			if (!WRITE && __ballot(valid && sid >= n_segs)) { bad = true; break; }
			uint64_t todo = __ballot(valid);
			for (int it = 0; it < 64 && todo; ++it) {                               // one round per distinct sid of the row
				const int s0 = __shfl(sid, __ffsll((unsigned long long)todo) - 1);
				const bool mine = valid && sid == s0;
				const uint64_t m = __ballot(mine);
				const int before = s_na[s0], c = __popcll(m);
				if (WRITE && mine) {
					const int64_t dst = s_bo[s0] + before + __popcll(m & lt);
					const int32_t d = a.y >> 31 ? s_rev[s0] : s_fwd[s0];
					const uint64_t y = ((uint64_t)a.w << 32 | a.z) - (uint64_t)(int64_t)d;
					if (dst >= 0 && dst < A.n_b_cap) A.sb[dst] = make_uint4(a.x, a.y, (uint32_t)y, (uint32_t)(y >> 32));
					else atomicAdd(&A.flags[1], 1);
				}
				__syncthreads();
				if (lane == 0) { s_na[s0] = before + c; s_row[s0] += c; }
				__syncthreads();
				todo &= ~m;
			}
		}
		if (bad) break;
		for (int s = lane; s < n_segs; s += 64) {                                   // hit.c:387, 393, 399-401: this region's chain in segment s, if it has one
			const int c = s_row[s];
			if (c != 0) {
				if (WRITE) {
					const int64_t dst = s_uo[s] + s_nu[s];
					if (dst >= 0 && dst < A.n_su_cap) A.su[dst] = (uint64_t)(uint32_t)score << 32 | (uint32_t)c;
					else atomicAdd(&A.flags[1], 1);
				}
				s_nu[s] += 1; s_row[s] = 0;
			}
		}
		__syncthreads();
	}
	if (WRITE) return;
	if (bad) {                                                                   // nothing of this fragment is touched; its segment reads are empty
		for (int s = lane; s < n_segs; s += 64) { A.cnt_u[sr0 + s] = 0; A.cnt_a[sr0 + s] = 0; }
		if (lane == 0) { atomicAdd(&A.flags[0], 1); A.state[f] = -1; }
		return;
	}
	for (int s = lane; s < n_segs; s += 64) {
		A.cnt_u[sr0 + s] = s_nu[s]; A.cnt_a[sr0 + s] = s_na[s];
		A.seg_hash[sr0 + s] = A.hash[f];
		if (A.rep_len) A.seg_rep_len[sr0 + s] = A.rep_len[f];
	}
	if (lane == 0) A.state[f] = 0;
}

__global__ __launch_bounds__(256) void seg_mark(SegArgs A, uint64_t *seg_regs)
{
	const int64_t sr = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
	const int lane = (int)threadIdx.x & 63;
	if (sr >= A.n_frags * A.n_segs) return;
	const int64_t lo = A.su_off[sr], hi = A.su_off[sr + 1];
	if (lo < 0 || hi > A.n_su_cap) return;                                       // (the scans of counted chains: inside the capacity when seg_walk stored them all)
	const uint64_t bits = reg_put<REG_FLAGS>(REG_SEG_SPLIT | (uint32_t)(sr % A.n_segs) << REG_SEG_ID_SHIFT);   // seg_id < n_segs <= SEG_MAX: eight bits
	for (int64_t i = lo + lane; i < hi; i += 64) seg_regs[i * REG_WORDS + reg_word(REG_FLAGS)] |= bits;
}

} // namespace

size_t seg_scan_bytes(int64_t n_seg_reads)
{
	size_t b = 0;
	(void)rocprim::exclusive_scan(nullptr, b, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n_seg_reads + 1, rocprim::plus<int64_t>());
	return b;
}

hipError_t launch_seg_count(const SegArgs &A, hipStream_t st)
{
	if (A.n_frags <= 0) return hipSuccess;
	hipLaunchKernelGGL(seg_walk<false>, dim3((unsigned)A.n_frags), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_seg_offsets(const SegArgs &A, void *tmp, size_t tmp_bytes, hipStream_t st)
{
	if (A.n_frags <= 0) return hipSuccess;
	const size_t n1 = (size_t)(A.n_frags * A.n_segs) + 1;
	size_t b = tmp_bytes;
	hipError_t e = rocprim::exclusive_scan(tmp, b, A.cnt_u, A.su_off, (int64_t)0, n1, rocprim::plus<int64_t>(), st);
	if (e != hipSuccess) return e;
	b = tmp_bytes;
	if ((e = rocprim::exclusive_scan(tmp, b, A.cnt_a, A.sb_off, (int64_t)0, n1, rocprim::plus<int64_t>(), st)) != hipSuccess) return e;
	// the batch's totals, for the check: no fragment adds to a counter of the whole batch (one atomic per fragment on one address is what a kernel of 10^5 small
	// fragments then waits for)
	if ((e = hipMemcpyAsync(A.flags + 2, A.su_off + (n1 - 1), 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
	return hipMemcpyAsync(A.flags + 4, A.sb_off + (n1 - 1), 8, hipMemcpyDeviceToDevice, st);
}

hipError_t launch_seg_scatter(const SegArgs &A, hipStream_t st)
{
	if (A.n_frags <= 0) return hipSuccess;
	hipLaunchKernelGGL(seg_walk<true>, dim3((unsigned)A.n_frags), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_seg_mark(const SegArgs &A, uint64_t *seg_regs, hipStream_t st)
{
	const int64_t n_sr = A.n_frags * A.n_segs;
	if (n_sr <= 0 || A.n_su_cap <= 0) return hipSuccess;
	hipLaunchKernelGGL(seg_mark, dim3((unsigned)((n_sr + 3) / 4)), dim3(256), 0, st, A, seg_regs);
	return hipGetLastError();
}

} // namespace mm2c
