// wave_ops.h -- the wave64 primitives every kernel file shares: lanes below a lane, reductions over the 64 lanes, inclusive scans in lane order, and the
// block scan of the 1024-lane offset kernels.  Integers only: the order of a reduction's steps is free for them (sum, or, min, max), which it is not for
// floating point.  A reduction that carries an index beside its value is its caller's own.  The DP's DPP primitives are in chain_wave.h.
#ifndef MM2C_WAVE_OPS_H
#define MM2C_WAVE_OPS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace mm2c {

__device__ __forceinline__ int32_t lo32(uint64_t v) { return (int32_t)(uint32_t)v; }
__device__ __forceinline__ int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }
__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

// number of set bits of m in the lanes below the caller's
__device__ __forceinline__ int lanes_below(uint64_t m)
{
	return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the templates below take int or wider only (a bool or a short would be summed in its own width): for anything else there is no such function
template <typename T> using wave_int = std::enable_if_t<std::is_integral<T>::value && sizeof(T) >= 4, T>;

// ---- over all 64 lanes; every lane gets the result
template <typename T> __device__ __forceinline__ wave_int<T> wave_sum(T v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
template <typename T> __device__ __forceinline__ wave_int<T> wave_or(T v) { for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o); return v; }
template <typename T> __device__ __forceinline__ wave_int<T> wave_min(T v) { for (int o = 32; o > 0; o >>= 1) { const T y = __shfl_xor(v, o); v = y < v ? y : v; } return v; }
template <typename T> __device__ __forceinline__ wave_int<T> wave_max(T v) { for (int o = 32; o > 0; o >>= 1) { const T y = __shfl_xor(v, o); v = y > v ? y : v; } return v; }

// ---- inclusive over the lanes at or below the caller's.  lane: the caller's lane in its wave (threadIdx.x & 63 inside a larger block)
template <typename T> __device__ __forceinline__ wave_int<T> wave_incl_sum(T v, int lane) { for (int o = 1; o < 64; o <<= 1) { const T y = __shfl_up(v, o); if (lane >= o) v += y; } return v; }
template <typename T> __device__ __forceinline__ wave_int<T> wave_incl_max(T v, int lane) { for (int o = 1; o < 64; o <<= 1) { const T y = __shfl_up(v, o); if (lane >= o && y > v) v = y; } return v; }
// the latest value >= 0 at or in front of the lane, -1 if there is none
__device__ __forceinline__ int wave_incl_last(int v, int lane) { for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(v, o); if (lane >= o && v < 0) v = y; } return v; }

// ---- inclusive sums of N columns over a workgroup of 1024 lanes, one chunk of 1024 rows (Hillis-Steele on the caller's LDS).  Every lane of the workgroup
// calls it, on every chunk.  v: the lane's row; incl: its inclusive sums; total: the chunk's sums, the same in every lane.  The barrier that lets sh be written
// again is the first one of the next call, so what the caller does with the sums is not held up by it.
template <int N>
__device__ __forceinline__ void block_incl_sum_1024(int64_t (*sh)[1024], const int tid, const int64_t (&v)[N], int64_t (&incl)[N], int64_t (&total)[N])
{
	__syncthreads();                                                             // every lane has read the sums of the chunk before
	for (int c = 0; c < N; ++c) sh[c][tid] = v[c];
	__syncthreads();
	for (int d = 1; d < 1024; d <<= 1) {
		int64_t t[N];
		for (int c = 0; c < N; ++c) t[c] = tid >= d ? sh[c][tid - d] : 0;
		__syncthreads();
		for (int c = 0; c < N; ++c) sh[c][tid] += t[c];
		__syncthreads();
	}
	for (int c = 0; c < N; ++c) { incl[c] = sh[c][tid]; total[c] = sh[c][1023]; }
}

} // namespace mm2c
#endif
