// chain_regs.hip -- mm_gen_regs (hit.c:52-88, with mm_reg_set_coor hit.c:23-38 and mm_cal_fuzzy_len hit.c:8-21) on the GPU: the chains of the
// device epilogue (u, b) become the reference's mm_reg1_t array, byte for byte.
//
// The reference walks the chains of one read on one thread.  The two kernels below restate it data-parallel with the same result:
//
//   regs_sort (one wave per read)
//     keys      : as = exclusive prefix sum of (int32_t)u[i]; z.x = u[i] ^ (uint32_t)hash64((hash64(a[as].x) + hash64(a[as].y)) ^ hash)   (hit.c:62-68)
//     order     : radix_sort_128x ascending, then reversed (hit.c:69-71).  Distinct keys have one sorted order; among equal keys klib's sort is an
//                 insertion sort up to 64 records (stable) and the cycle-leader distribution above (radix_replay.h).  So: stable wave_sort64, the
//                 replay only for reads of more than 64 chains that hold equal keys, the stable sort of the replayed arrangement, and the reversal
//                 as rank = n_u - 1 - position -- what epi_tiesort does for chain.c:411.
//     fields    : every byte of the region except mlen / blen, which are written as 0 (hit.c:75-85; calloc's zeros included)
//   regs_fill (anchor-parallel, one wave per slice of 1 024 chain anchors of the whole batch; regs_fill_reads: the same slices read by read)
//     mlen, blen: sums of one term per chain anchor -- the span for the first, the pair term of hit.c:15-19 for every other.  `int` adds wrap, so
//                 the sums are associative: 16-byte loads a row of 64 anchors at a time, a segmented scan inside the wave, the open segment carried
//                 from row to row; a chain that lies inside the slice is stored, one that crosses slices is added with integer atomics.
//
// Preconditions (the host-buffer entry checks them; here they are clamped and counted in flags[0]): every chain has cnt >= 1 and the counts of a
// read add up to its extent of b.  Whatever u holds, an anchor is read only inside [b_off[r], b_off[r+1]) of its read and contributes only to
// a chain of that read.  A read whose offsets leave the plan's capacities is refused (counted in flags[0] and flags[2]); regs_fill_reads then takes the
// place of regs_fill and fills the other reads one by one, because the scratch of the refused read's chains was not written by this run.

#include <hip/hip_runtime.h>
#include <climits>
#include "chain_regs.h"
#include "radix_replay.h"
#include "wave_sort.h"

namespace mm2c {

namespace {

__device__ __forceinline__ uint64_t hash64(uint64_t key)                         // hit.c:40-50
{
	key = (~key + (key << 21));
	key = key ^ key >> 24;
	key = ((key + (key << 3)) + (key << 8));
	key = key ^ key >> 14;
	key = ((key + (key << 2)) + (key << 4));
	key = key ^ key >> 28;
	key = (key + (key << 31));
	return key;
}

// the extents of read r; false when its offsets are not ordered inside the plan's capacities.  Both kernels ask: a read regs_sort refuses writes none of its
// per-chain scratch, so regs_fill must not look there either
__device__ __forceinline__ bool read_extents(const RegArgs &A, int64_t r, int64_t &base, int64_t &nu, int64_t &bbase, int64_t &nb)
{
	base = A.u_off[r]; bbase = A.b_off[r];
	nu = A.u_off[r + 1] - base; nb = A.b_off[r + 1] - bbase;
	return !(base < 0 || bbase < 0 || nu < 0 || nb < 0 || nu > INT_MAX || nb > INT_MAX || base + nu > A.n_u_cap || bbase + nb > A.n_b_cap);
}

// ---- kernel S: keys, order, every field but the fuzzy lengths --------------------------------------------------------------------------
__global__ __launch_bounds__(64) void regs_sort(RegArgs A)
{
	__shared__ uint16_t s_id[REGS_TS_MAX];
	__shared__ uint8_t s_dg[REGS_TS_MAX + 8];                                    // (the walk of radix_replay.h looks one byte beyond the digit it takes)
	__shared__ __attribute__((aligned(8))) int s_cur[576];
	__shared__ int s_lo[257], s_sp;
	const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
	int64_t base, nu64, bbase, nb;
	if (!read_extents(A, r, base, nu64, bbase, nb)) {
		if (lane == 0) { atomicAdd(&A.flags[0], 1); atomicAdd(&A.flags[2], 1); }  // offsets that leave the plan's capacities: nothing of this read is touched
		return;
	}
	const int nu = (int)nu64;
	if (nu == 0) { if (nb != 0 && lane == 0) atomicAdd(&A.flags[0], 1); return; }
	const uint64_t *u = A.u + base;
	const ulonglong2 *b = A.b + bbase;
	const uint32_t hash = A.hash[r];
	const int32_t qlen = A.qlen[r];
	uint64_t *zkey = A.zkey + base, *key0 = A.key0 + base, *key1 = A.key1 + base;
	int64_t *cstart = A.cstart + base, *cend = A.cend + base;
	int32_t *val0 = A.val0 + base, *val1 = A.val1 + base, *tiecnt = A.tiecnt + base, *stack = A.stack + base, *moved = A.moved + base;

	int64_t run = 0;
	int bad = 0;
	for (int i0 = 0; i0 < nu; i0 += 64) {                                        // hit.c:62-68
		const int i = i0 + lane;
		const bool valid = i < nu;
		const uint64_t uu = valid ? u[i] : 0;
		const int32_t cnt = (int32_t)uu;
		bad |= valid && cnt <= 0;
		const int64_t c = cnt > 0 ? cnt : 0;
		const int64_t incl = wave_incl_sum(c, lane);
		const int64_t pre = run + incl - c;                                      // = as
		if (valid) {
			cstart[i] = bbase + (pre < nb ? pre : nb);
			cend[i] = bbase + (pre + c < nb ? pre + c : nb);
			ulonglong2 a0 = make_ulonglong2(0, 0);
			if (nb > 0) a0 = b[pre < nb ? pre : nb - 1];
			const uint64_t z = uu ^ (uint64_t)(uint32_t)hash64((hash64(a0.x) + hash64(a0.y)) ^ (uint64_t)hash);
			zkey[i] = z; key0[i] = z; val0[i] = i;
		}
		run += __shfl(incl, 63);
	}
	bad |= run != nb;
	if (__any(bad) && lane == 0) atomicAdd(&A.flags[0], 1);
	__syncthreads();
	wave_sort64<false>(key0, key1, val0, val1, nu, lane, s_cur);                  // ascending, stable: (key1, val1)

	// tiecnt[i] = equal neighbours before position i of the sorted keys
	int ties = 0;
	for (int i0 = 0; i0 < nu; i0 += 64) {
		const int i = i0 + lane;
		const int flag = (i + 1 < nu && key1[i] == key1[i + 1]) ? 1 : 0;
		const int incl = wave_incl_sum(flag, lane);
		if (i < nu) tiecnt[i] = ties + incl - flag;
		ties += __shfl(incl, 63);
	}
	if (ties > 0 && lane == 0) atomicAdd(&A.flags[1], 1);
	if (ties > 0 && nu > 64) {                                                   // ksort.h:141-143: up to 64 records an insertion sort, stable
		__syncthreads();
		if (nu <= REGS_TS_MAX) {
			replay_passes<uint16_t, false, true>(zkey, 1, key1, 1, tiecnt, nu, s_id, s_dg, stack, moved, nullptr, nullptr, lane, s_cur, s_lo, &s_sp);
			for (int i = lane; i < nu; i += 64) val0[i] = (int32_t)s_id[i];
		} else {                                                                 // does not fit the LDS: the same replay through global memory
			uint8_t *g_dg = (uint8_t *)(stack + 2 * (nu / 64 + 2));
			replay_passes<uint32_t, false, false>(zkey, 1, key1, 1, tiecnt, nu, (uint32_t *)val0, g_dg, stack, moved, nullptr, nullptr, lane, s_cur, s_lo, &s_sp);
		}
		__syncthreads();
		for (int i = lane; i < nu; i += 64) key1[i] = zkey[val0[i]];             // keys of the replayed arrangement
		__syncthreads();
		wave_sort64<false>(key1, key0, val0, val1, nu, lane, s_cur);             // stable: = the insertion sorts of ksort.h:144, sorted order elsewhere
	}
	__syncthreads();

	// hit.c:70-85: position i of the ascending array is region n_u - 1 - i
	for (int i = lane; i < nu; i += 64) {
		const int c = val1[i], j = nu - 1 - i;
		const uint64_t z = zkey[c];
		const int32_t cnt = (int32_t)u[c];
		const int64_t as = cstart[c] - bbase;
		ulonglong2 a0 = make_ulonglong2(0, 0), a1 = a0;
		if (nb > 0) {
			int64_t l = as + cnt - 1;
			l = l < 0 ? 0 : l < nb ? l : nb - 1;
			a0 = b[as < nb ? as : nb - 1]; a1 = b[l];
		}
		const int32_t q_span = (int32_t)(a0.y >> 32 & 0xff);
		const uint32_t rev = (uint32_t)(a0.x >> 63);
		const uint32_t rid = (uint32_t)(a0.x << 1 >> 33);
		const uint32_t x0 = (uint32_t)a0.x + 1u, x1 = (uint32_t)a1.x + 1u, y0 = (uint32_t)a0.y + 1u - (uint32_t)q_span, y1 = (uint32_t)a1.y + 1u;
		const uint32_t rs = (int32_t)x0 > q_span ? x0 - (uint32_t)q_span : 0u, re = x1;
		const uint32_t qs = rev ? (uint32_t)qlen - y1 : y0, qe = rev ? (uint32_t)qlen - y0 : y1;
		const uint32_t score = (uint32_t)(z >> 32);
		uint64_t *o = A.regs + (base + j) * REG_WORDS;
		o[reg_word(REG_ID)] = reg_put<REG_ID>((uint32_t)j) | reg_put<REG_CNT>((uint32_t)cnt);
		o[reg_word(REG_RID)] = reg_put<REG_RID>(rid) | reg_put<REG_SCORE>(score);
		o[reg_word(REG_QS)] = reg_put<REG_QS>(qs) | reg_put<REG_QE>(qe);
		o[reg_word(REG_RS)] = reg_put<REG_RS>(rs) | reg_put<REG_RE>(re);
		o[reg_word(REG_PARENT)] = reg_put<REG_PARENT>(0xffffffffu);                 // parent = MM_PARENT_UNSET, subsc = 0
		o[reg_word(REG_AS)] = reg_put<REG_AS>((uint32_t)as);                        // mlen: regs_fill
		o[reg_word(REG_BLEN)] = 0;                                                  // blen: regs_fill; n_sub
		o[reg_word(REG_SCORE0)] = reg_put<REG_SCORE0>(score) | reg_put<REG_FLAGS>(rev << REG_REV_BIT);
		o[reg_word(REG_HASH)] = reg_put<REG_HASH>((uint32_t)z) | reg_put<REG_DIV>(0xbf800000u);   // div = -1.0f
		o[REG_WORDS - 1] = 0;                                                       // p
		A.crank[base + c] = (int32_t)(base + j);
	}
}

// ---- kernel F: mlen and blen (mm_cal_fuzzy_len) -------------------------------------------------------------------------------------------
// Which chain an anchor belongs to: cstart[] ascends over the whole batch (every chain holds at least one anchor), so the chain of anchor g is the last one
// that starts at or before g -- if g lies before its end.  A wave finds the chains of its slice's first and last anchor by a 64-way search (four rounds for
// millions of chains), copies the starts and ends of the chains between them -- at most one per anchor of the slice, REGS_FILL_CAP -- into LDS relative to the
// slice, and every lane then searches there.  More chains than that between the two only come from counts that break the preconditions (chains without
// anchors): such a slice searches in memory instead (LDS = false), same code.
constexpr int REGS_FILL_CAP = 64 * REGS_FILL_ROWS + 1;
constexpr int REL_FAR = 4096;                                                  // "outside the slice", on either side (the table holds 16-bit values)
constexpr int REGS_FILL_AHEAD = 4;
static_assert(64 * REGS_FILL_ROWS < REL_FAR && REGS_FILL_ROWS % REGS_FILL_AHEAD == 0, "slice shape");

// the last chain of [lo, hi] that starts at or before g (lo when none does); all 64 lanes together
__device__ __forceinline__ int wave_find_chain(const int64_t *cstart, int lo, int hi, int64_t g, int lane)
{
	for (;;) {
		const int w = hi - lo + 1;
		if (w <= 1) return lo;
		const int stride = (w + 63) / 64;
		const int64_t at = (int64_t)lo + (int64_t)lane * stride;
		const uint64_t m = __ballot(at <= hi && cstart[at] <= g);
		if (m == 0) return lo;
		lo += (63 - __clzll(m)) * stride;
		if (stride == 1) return lo;
		if (hi - lo > stride - 1) hi = lo + stride - 1;
	}
}

struct SliceTab {
	const int64_t *cstart, *cend;
	const int16_t *s_cs, *s_ce;                                               // starts and ends of chains c_lo .. relative to g0, in LDS
	int64_t g0;
	int c_lo;
	template <bool LDS> __device__ __forceinline__ int64_t start(int c) const { return LDS ? (int64_t)s_cs[c - c_lo] : cstart[c] - g0; }
	template <bool LDS> __device__ __forceinline__ int64_t end(int c) const { return LDS ? (int64_t)s_ce[c - c_lo] : cend[c] - g0; }
	// the last chain of [lo, hi] that starts at or before position g of the slice (lo when none does); one lane
	template <bool LDS> __device__ __forceinline__ int find(int lo, int hi, int64_t g) const
	{
		while (lo < hi) {
			const int mid = lo + (hi - lo + 1) / 2;
			if (start<LDS>(mid) <= g) lo = mid; else hi = mid - 1;
		}
		return lo;
	}
};

template <bool LDS>
__device__ __forceinline__ void fill_flush(const RegArgs &A, const SliceTab &T, int c, int vb, int vm, int64_t len)
{
	const int rk = A.crank[c];
	if ((uint32_t)rk >= (uint32_t)A.n_u_cap) return;                             // (every chain looked up here had its rank written by this run: the bound of the write all the same)
	int32_t *p = (int32_t *)A.regs + (int64_t)rk * (2 * REG_WORDS) + REG_MLEN;    // mlen, blen
	if (T.start<LDS>(c) >= 0 && T.end<LDS>(c) <= len) { p[0] = vm; p[1] = vb; }  // the whole chain lies in this wave's slice
	else { atomicAdd(p, vm); atomicAdd(p + 1, vb); }
}

// the rows of one slice [g0, g1); the chains of its anchors are c_lo .. c_hi
template <bool LDS>
__device__ __forceinline__ void fill_slice(const RegArgs &A, const SliceTab &T, int64_t g0, int64_t g1, int c_lo, int c_hi, int lane)
{
	const int64_t len = g1 - g0;
	uint32_t pxl = 0, pyl = 0;                                                   // low words of the anchor before the row
	if (g0 > 0) { const ulonglong2 a = A.b[g0 - 1]; pxl = (uint32_t)a.x; pyl = (uint32_t)a.y; }
	int ccid = -1, cb = 0, cm = 0;                                               // the open segment of the rows so far (uniform)
	int row_lo = c_lo;
	auto row = [&](int64_t g, const ulonglong2 a) {
		const int64_t gi = g + lane;
		const bool in = gi < g1;
		const uint32_t xl = (uint32_t)a.x, yl = (uint32_t)a.y;
		const int span = (int)(a.y >> 32 & 0xff);
		uint32_t qx = __shfl_up(xl, 1), qy = __shfl_up(yl, 1);
		if (lane == 0) { qx = pxl; qy = pyl; }
		pxl = __shfl(xl, 63); pyl = __shfl(yl, 63);
		const int64_t rel = (in ? gi : g1 - 1) - g0;
		const int cid = T.find<LDS>(row_lo, c_hi, rel);
		int key = -1, tb = 0, tm = 0;
		if (in) {
			const int64_t cs = T.start<LDS>(cid);
			if (rel >= cs && rel < T.end<LDS>(cid)) {
				key = cid;
				if (rel == cs) tb = tm = span;                                       // hit.c:13
				else {                                                           // hit.c:15-19
					const int tl = (int32_t)(xl - qx), ql = (int32_t)(yl - qy);
					tb = tl > ql ? tl : ql;
					tm = tl > span && ql > span ? span : tl < ql ? tl : ql;
				}
			}
		}
		if (ccid >= 0) {                                                         // the segment the row before left open goes on in lane 0, or is done
			const int k0 = __shfl(key, 0);
			if (lane == 0) { if (k0 == ccid) { tb += cb; tm += cm; } else fill_flush<LDS>(A, T, ccid, cb, cm, len); }
		}
		for (int o = 1; o < 64; o <<= 1) {                                       // segmented inclusive scan: the lanes of a chain are neighbours
			const int yb = __shfl_up(tb, o), ym = __shfl_up(tm, o), yk = __shfl_up(key, o);
			if (lane >= o && yk == key) { tb += yb; tm += ym; }
		}
		const int nk = __shfl_down(key, 1);
		if (key >= 0 && lane != 63 && nk != key) fill_flush<LDS>(A, T, key, tb, tm, len);
		ccid = __shfl(key, 63); cb = __shfl(tb, 63); cm = __shfl(tm, 63);
		row_lo = __shfl(cid, 63);                                                // ascending: no later anchor belongs to an earlier chain
	};
	for (int64_t g = g0; g < g1; g += 64 * REGS_FILL_AHEAD) {                    // the loads of REGS_FILL_AHEAD rows in flight together
		ulonglong2 a[REGS_FILL_AHEAD];
#pragma unroll
		for (int k = 0; k < REGS_FILL_AHEAD; ++k) {
			const int64_t gi = g + 64 * k + lane;
			a[k] = make_ulonglong2(0, 0);
			if (gi < g1) a[k] = A.b[gi];
		}
#pragma unroll
		for (int k = 0; k < REGS_FILL_AHEAD; ++k)
			if (g + 64 * k < g1) row(g + 64 * k, a[k]);
	}
	if (ccid >= 0 && lane == 0) fill_flush<LDS>(A, T, ccid, cb, cm, len);
}

// one slice [g0, g1) of b; its anchors belong to chains among u_lo .. u_hi, whose cstart / cend this run wrote and which ascend
__device__ __forceinline__ void fill_wave_slice(const RegArgs &A, int16_t (*s_tab)[REGS_FILL_CAP + 1], int u_lo, int u_hi, int64_t g0, int64_t g1, int lane)
{
	const int c_lo = wave_find_chain(A.cstart, u_lo, u_hi, g0, lane), c_hi = wave_find_chain(A.cstart, c_lo, u_hi, g1 - 1, lane);
	SliceTab T;
	T.cstart = A.cstart; T.cend = A.cend; T.s_cs = s_tab[0]; T.s_ce = s_tab[1]; T.g0 = g0; T.c_lo = c_lo;
	if (c_hi - c_lo < REGS_FILL_CAP) {
		for (int k = lane; k <= c_hi - c_lo; k += 64) {
			const int64_t cs = A.cstart[c_lo + k] - g0, ce = A.cend[c_lo + k] - g0;
			s_tab[0][k] = (int16_t)(cs < -REL_FAR ? -REL_FAR : cs > REL_FAR ? REL_FAR : cs);
			s_tab[1][k] = (int16_t)(ce < -REL_FAR ? -REL_FAR : ce > REL_FAR ? REL_FAR : ce);
		}
		rp_wave_sync();
		fill_slice<true>(A, T, g0, g1, c_lo, c_hi, lane);
	} else fill_slice<false>(A, T, g0, g1, c_lo, c_hi, lane);
}

// Two routes.  regs_sort accepted every read (flags[2] == 0): the offsets ascend from u_off[0] to u_off[n_reads] inside the capacities, every chain between them has
// its cstart / cend / crank from this run, and a wave takes one slice of b of the whole batch.  It refused a read: the scratch of that read's chains holds whatever an
// earlier run left, so nothing may be searched across reads and nothing derived from u_off[n_reads] / b_off[n_reads].  The waves then stride over the reads, skip those
// that fail regs_sort's test, and take an accepted read's slices one after another, looking only at its own chains and anchors.  Slower, and exact beside a broken read.
// Two kernels, of which one works: they are launched one after the other and each leaves at once when the route is the other's (a kernel of both routes needs a
// third more registers than regs_fill alone, on every run).
__global__ __launch_bounds__(64 * REGS_FILL_WAVES) void regs_fill(RegArgs A)
{
	__shared__ int16_t s_tab[REGS_FILL_WAVES][2][REGS_FILL_CAP + 1];                // per wave: starts, ends (private to the wave: wave-local synchronisation only)
	const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
	if (A.flags[2] != 0) return;
	const int64_t u_lo = A.u_off[0], u_hi = A.u_off[A.n_reads], n_b = A.b_off[A.n_reads];
	const int64_t g0 = ((int64_t)blockIdx.x * REGS_FILL_WAVES + wave) * (64 * REGS_FILL_ROWS);
	if (g0 >= n_b || u_hi <= u_lo) return;
	const int64_t g1 = g0 + 64 * REGS_FILL_ROWS < n_b ? g0 + 64 * REGS_FILL_ROWS : n_b;
	fill_wave_slice(A, s_tab[wave], (int)u_lo, (int)u_hi - 1, g0, g1, lane);
}

__global__ __launch_bounds__(64 * REGS_FILL_WAVES) void regs_fill_reads(RegArgs A)
{
	__shared__ int16_t s_tab[REGS_FILL_WAVES][2][REGS_FILL_CAP + 1];
	const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
	if (A.flags[2] == 0) return;
	const int64_t n_waves = (int64_t)gridDim.x * REGS_FILL_WAVES;
	for (int64_t r = (int64_t)blockIdx.x * REGS_FILL_WAVES + wave; r < A.n_reads; r += n_waves) {
		int64_t base, nu, bbase, nb;
		if (!read_extents(A, r, base, nu, bbase, nb) || nu == 0) continue;
		for (int64_t g0 = bbase; g0 < bbase + nb; g0 += 64 * REGS_FILL_ROWS) {
			const int64_t g1 = g0 + 64 * REGS_FILL_ROWS < bbase + nb ? g0 + 64 * REGS_FILL_ROWS : bbase + nb;
			fill_wave_slice(A, s_tab[wave], (int)base, (int)(base + nu) - 1, g0, g1, lane);
			rp_wave_sync();                                                      // the table is written again for the next slice
		}
	}
}

} // namespace

hipError_t launch_chain_regs(const RegArgs &A, hipStream_t st, hipEvent_t ev_mid, int *n_launches)
{
	hipError_t e;
	if (A.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(regs_sort, dim3((unsigned)A.n_reads), dim3(64), 0, st, A);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev_mid && (e = hipEventRecord(ev_mid, st)) != hipSuccess) return e;
	int nl = 1;
	if (A.n_b_cap > 0) {
		const int64_t per = 64 * REGS_FILL_ROWS * REGS_FILL_WAVES;
		hipLaunchKernelGGL(regs_fill, dim3((unsigned)((A.n_b_cap + per - 1) / per)), dim3(64 * REGS_FILL_WAVES), 0, st, A);
		if ((e = hipGetLastError()) != hipSuccess) return e;
		const int64_t blocks = (A.n_reads + REGS_FILL_WAVES - 1) / REGS_FILL_WAVES;  // a wave per read, the reads beyond 16 384 in turns
		hipLaunchKernelGGL(regs_fill_reads, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(64 * REGS_FILL_WAVES), 0, st, A);
		nl += 2;
	}
	if (n_launches) *n_launches += nl;
	return hipGetLastError();
}

} // namespace mm2c
