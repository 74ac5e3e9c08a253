// wave_sort.h -- stable LSD radix sort of one task's records by one wave, shared by the device epilogue (chain_epilogue.hip) and the
// chains-to-regions step (chain_regs.hip).  The wave primitives it uses (lanes_below, wave_incl_sum, wave_or) are those of wave_ops.h.
#ifndef MM2C_WAVE_SORT_H
#define MM2C_WAVE_SORT_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_ops.h"

namespace mm2c {

namespace {

// ---- stable LSD radix sort of one task's records by one wave (8-bit digits, ping-pong between two global buffers) ----
// Bytes in which all keys agree are skipped, so (score << 32 | index) keys cost about four passes.  Per 64 records: the lanes with
// the same digit find each other with eight ballots; rank among them = position in lane order (stable).  `vals` may be NULL.
// The result ends in (k1, v1).  No host involvement -- rocPRIM's segmented sort synchronises the stream on the host.
// SOLO: the wave runs alone inside a bigger block (the other waves wait at the next __syncthreads): its own LDS and memory operations are
// ordered by a workgroup fence, without the barrier.
template <bool SOLO>
__device__ __forceinline__ void sort_sync()
{
	if (SOLO) { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); }
	else __syncthreads();
}
#define __syncthreads_sort() sort_sync<SOLO>()
template <bool DESC, bool SOLO = false>
__device__ void wave_sort64(uint64_t *k0, uint64_t *k1, int32_t *v0, int32_t *v1, int m, int lane, int *s_cnt /* 256 ints of LDS */)
{
	if (m <= 0) return;
	uint64_t diff = 0;
	const uint64_t first = k0[0];
	for (int i = lane; i < m; i += 64) diff |= k0[i] ^ first;
	diff = wave_or(diff);
	uint64_t *src = k0, *dst = k1;
	int32_t *vsrc = v0, *vdst = v1;
	for (int shift = 0; shift < 64; shift += 8) {
		if (((diff >> shift) & 255) == 0) continue;
		for (int d = lane; d < 256; d += 64) s_cnt[d] = 0;
		__syncthreads_sort();
		for (int i = lane; i < m; i += 64) {
			const int d = (int)(src[i] >> shift) & 255;
			atomicAdd(&s_cnt[DESC ? 255 - d : d], 1);
		}
		__syncthreads_sort();
		{
			int h[4], sum = 0;
#pragma unroll
			for (int k = 0; k < 4; ++k) { h[k] = s_cnt[4 * lane + k]; sum += h[k]; }
			int at = wave_incl_sum(sum, lane) - sum;
			__syncthreads_sort();
#pragma unroll
			for (int k = 0; k < 4; ++k) { s_cnt[4 * lane + k] = at; at += h[k]; }
		}
		__syncthreads_sort();
		for (int i0 = 0; i0 < m; i0 += 64) {
			const int i = i0 + lane;
			const bool valid = i < m;
			const uint64_t key = valid ? src[i] : 0;
			const int32_t val = (valid && vsrc) ? vsrc[i] : 0;
			int d = (int)(key >> shift) & 255;
			if (DESC) d = 255 - d;
			uint64_t peers = __ballot(valid);
#pragma unroll
			for (int b = 0; b < 8; ++b) {
				const uint64_t bal = __ballot((d >> b) & 1);
				peers &= ((d >> b) & 1) ? bal : ~bal;
			}
			if (valid) {
				const int rank = lanes_below(peers);
				const int pos = s_cnt[d] + rank;
				dst[pos] = key;
				if (vdst) vdst[pos] = val;
			}
			__syncthreads_sort();
			if (valid && lanes_below(peers) == 0) s_cnt[d] += __popcll(peers);
			__syncthreads_sort();
		}
		{ uint64_t *t = src; src = dst; dst = t; }
		{ int32_t *t = vsrc; vsrc = vdst; vdst = t; }
	}
	if (src != k1) {                                                             // even number of passes: the result is in (k0, v0)
		for (int i = lane; i < m; i += 64) { k1[i] = src[i]; if (v1) v1[i] = vsrc[i]; }
	}
	__syncthreads_sort();
}

#undef __syncthreads_sort

} // namespace

} // namespace mm2c
#endif
