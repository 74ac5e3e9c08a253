// chain_hits.hip -- mm_set_parent (hit.c:125-186) and mm_select_sub (hit.c:255-272, with mm_sync_regs / mm_set_sam_pri hit.c:220-253) on the GPU: the
// regions of the region plan (chain_regs.hip) become the reference's hits, byte for byte.  The fields p, is_alt and inv are always 0 here, so the branches on
// them (hit.c:168, 171-176, 261, 266-267) are not built.
//
// One kernel, hits_select, one wave per read.  The reference is sequential in the regions of a read; what is parallel is the walk over the primaries:
//
//   tables    : qs qe score cnt subsc n_sub parent rid rs re per region, and (qs, qe) of the primaries in the order they were made (w, hit.c:132).  In LDS for
//               reads of up to HITS_LDS_MAX regions, in the plan's scratch beyond -- the same code, instantiated on the two kinds of pointer.
//   set_parent: for region i the lanes take the primaries 64 at a time.  Pass 1 packs the clipped overlaps (hit.c:138-145) with a ballot; uncov_len is the
//               measure of [qs_i, qe_i) outside their union.  The reference sorts the intervals and sweeps; the measure does not depend on how it is found, so
//               here every lane takes one candidate gap start g (qs_i or the end of an interval): it opens a gap if no interval holds g, g < qe_i and no earlier
//               interval ends at g too, and the gap reaches to the nearest interval start beyond g (or qe_i).  Integers only; O(n_cov^2 / 64).  Pass 2
//               evaluates hit.c:160-165 per lane -- int -> float, two IEEE divisions, one subtraction, one comparison, as written -- and the first passing
//               primary in w order is the lowest set bit of the first non-empty ballot.  Lane 0 then updates that primary's subsc / n_sub or appends the region
//               to the primaries, before the next region looks.
//   select_sub: hit.c:259-268 compacts in place while it reads r[p]: at step i position p holds the kept region of rank p if k > p, else the original r[p].
//               Lane 0 walks that chain over the tables and leaves the source index of every kept position; no record moves yet.
//   move      : the 80-byte records go from the input to the output through that map, lane-parallel as 8-byte words, patched on the way: id, parent, subsc,
//               n_sub, and -- only when something was dropped (hit.c:269) -- the new ids, the parents through them, and sam_pri (bit 12) on the first hit.
//
// A read whose offsets leave the plan's capacities touches nothing and is counted in flags[0].
//
// hits_select_multi is the same kernel with mm_select_sub_multi (pe.c:6-43) in the place of mm_select_sub, for fragments of several segments (map.c:254): the
// tables gain one row, rev (bit 10 of the bit-field word), and only lane 0's decision walk differs -- the child is judged by min_diff first (integer), then by one
// of three ratios: pri1 when child and parent lie close on the same strand of the same reference sequence (two strict integer compares against
// max_dist = qlens[0] + qlens[1] + max_gap_ref, wrapping, 0 unless n_segs == 2), else pri_ratio or pri2 by which of the two spans both segments.  No identical-hit
// test; n_2nd counts every secondary that passed, kept or not.  hits_select itself is the instantiation without any of it.

#include <hip/hip_runtime.h>
#include <climits>
#include "chain_hits.h"
#include "chain_regs.h"
#include "wave_ops.h"

namespace mm2c {

namespace {

struct HitTab {
	int32_t *qs, *qe, *score, *cnt, *subsc, *nsub, *parent, *rid, *rs, *re, *w, *rev;   // rev: hits_select_multi only
	int2 *pq, *cov;
};

// what mm_select_sub_multi knows of the fragment: qlens[0] and max_dist (pe.c:10)
struct MultiFrag { int32_t q0, max_dist; bool two; };

template <bool MULTI>
__device__ __forceinline__ void hits_read(const HitArgs &A, const HitTab T, const uint64_t *in, uint64_t *out, int32_t *n_out, const int n, const int lane,
                                          const MultiFrag F)
{
	for (int i = lane; i < n; i += 64) {
		uint64_t w[8];                                                           // the 64-bit loads first (those of words nobody asks for are dropped)
		for (int k = 0; k < 8; ++k) w[k] = in[(int64_t)i * REG_WORDS + k];
		T.cnt[i] = reg_get<REG_CNT>(w); T.rid[i] = reg_get<REG_RID>(w); T.score[i] = reg_get<REG_SCORE>(w);
		T.qs[i] = reg_get<REG_QS>(w); T.qe[i] = reg_get<REG_QE>(w); T.rs[i] = reg_get<REG_RS>(w); T.re[i] = reg_get<REG_RE>(w);
		T.parent[i] = reg_get<REG_PARENT>(w); T.subsc[i] = reg_get<REG_SUBSC>(w); T.nsub[i] = reg_get<REG_N_SUB>(w);
		if constexpr (MULTI) T.rev[i] = reg_rev(w);
	}
	__syncthreads();

	// ---- mm_set_parent (hit.c:133-183) ----
	if (lane == 0) { T.w[0] = 0; T.parent[0] = 0; T.pq[0] = make_int2(T.qs[0], T.qe[0]); }
	__syncthreads();
	int k = 1;
	const uint64_t lt = (1ull << lane) - 1;
	for (int i = 1; i < n; ++i) {
		const int si = __builtin_amdgcn_readfirstlane(T.qs[i]), ei = __builtin_amdgcn_readfirstlane(T.qe[i]);
		int uncov_len = 0;
		if (!A.hard_mask_level) {
			int n_cov = 0, len1 = 0;
			for (int j0 = 0; j0 < k; j0 += 64) {                                 // hit.c:138-145
				const int j = j0 + lane;
				int2 q = make_int2(0, 0);
				if (j < k) q = T.pq[j];
				const bool ov = j < k && !(q.y <= si || q.x >= ei);
				const uint64_t m = __ballot(ov);
				const int cs = q.x < si ? si : q.x, ce = q.y > ei ? ei : q.y;
				if (ov) T.cov[n_cov + __popcll(m & lt)] = make_int2(cs, ce);
				if (m) len1 = __shfl(ce - cs, __ffsll((unsigned long long)m) - 1);
				n_cov += __popcll(m);
			}
			if (n_cov == 1) uncov_len = (ei - si) - len1;                        // one interval, clipped to the region: what it leaves
			else if (n_cov > 1) {                                                // hit.c:148-156 as a measure
				__syncthreads();
				int len = 0;
				for (int t0 = 0; t0 <= n_cov; t0 += 64) {
					const int t = t0 + lane;
					const int g = t < n_cov ? T.cov[t].y : si;
					bool open = t <= n_cov && g < ei;
					int end = ei;
					for (int q = 0; q < n_cov; ++q) {
						const int2 c = T.cov[q];
						if (c.x <= g && g < c.y) open = false;
						if (c.x > g && c.x < end) end = c.x;
						if (q < t && t < n_cov && c.y == g) open = false;
					}
					if (open) len += end - g;
				}
				uncov_len = wave_sum(len);
				__syncthreads();
			}
		}
		int found = -1;
		for (int j0 = 0; j0 < k && found < 0; j0 += 64) {                        // hit.c:158-165
			const int j = j0 + lane;
			int2 q = make_int2(0, 0);
			if (j < k) q = T.pq[j];
			const int sj = q.x, ej = q.y;
			const bool ov = j < k && !(ej <= si || sj >= ei);
			const int mn = ej - sj < ei - si ? ej - sj : ei - si;
			const int mx = ej - sj > ei - si ? ej - sj : ei - si;
			const int ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
			const float lhs = (float)ol / (float)mn - (float)uncov_len / (float)mx;
			const uint64_t m = __ballot(ov && lhs > A.mask_level && uncov_len <= A.mask_len);
			if (m) found = j0 + __ffsll((unsigned long long)m) - 1;
		}
		if (lane == 0) {
			if (found >= 0) {                                                    // hit.c:166-178
				const int pi = T.w[found], sci = T.score[i];
				T.parent[i] = pi;                                                // rp->parent: a primary is its own parent
				if (T.subsc[pi] < sci) T.subsc[pi] = sci;
				if (T.cnt[i] >= T.cnt[pi]) ++T.nsub[pi];
			} else {                                                             // hit.c:182
				T.w[k] = i; T.pq[k] = make_int2(si, ei); T.parent[i] = i; T.nsub[i] = 0;
			}
		}
		if (found < 0) ++k;
		__syncthreads();
	}

	// ---- mm_select_sub (hit.c:257-270): which regions stay, and which region a kept position comes from ----
	int32_t *src = T.w, *newidx = T.cnt;                                        // (w and cnt have served)
	int kept = n;
	if (A.pri_ratio > 0.0f) {
		if (lane == 0) {
			int kk = 0, n_2nd = 0;
			for (int i = 0; i < n; ++i) {
				const int p = T.parent[i];
				bool keep = p == i;
				if constexpr (MULTI) {                                           // pe.c:13-36
					if (!keep) {
						const int pp = kk > p ? src[p] : p;                      // what lies at position p by now
						const int sc = T.score[i], scp = T.score[pp];
						if ((int32_t)((uint32_t)sc + (uint32_t)A.min_diff) >= scp) keep = true;
						else {
							float ratio;
							if (T.rev[pp] == T.rev[i] && T.rid[pp] == T.rid[i] && (int32_t)((uint32_t)T.re[i] - (uint32_t)T.rs[pp]) < F.max_dist &&
							    (int32_t)((uint32_t)T.re[pp] - (uint32_t)T.rs[i]) < F.max_dist) ratio = A.pri1;
							else {
								const bool par_both = F.two && T.qs[pp] < F.q0 && T.qe[pp] > F.q0, chi_both = F.two && T.qs[i] < F.q0 && T.qe[i] > F.q0;
								ratio = chi_both || chi_both == par_both ? A.pri_ratio : A.pri2;
							}
							keep = (float)sc >= (float)scp * ratio;
						}
						if (keep && n_2nd++ >= A.best_n) keep = false;           // pe.c:35: every secondary that passed counts
					}
				} else
				if (!keep) {
					const int pp = kk > p ? src[p] : p;                          // what lies at position p by now
					const int sc = T.score[i], scp = T.score[pp];
					if (((float)sc >= (float)scp * A.pri_ratio || (int32_t)((uint32_t)sc + (uint32_t)A.min_diff) >= scp) && n_2nd < A.best_n) {
						if (!(T.qs[i] == T.qs[pp] && T.qe[i] == T.qe[pp] && T.rid[i] == T.rid[pp] && T.rs[i] == T.rs[pp] && T.re[i] == T.re[pp])) keep = true, ++n_2nd;
					}
				}
				if (keep) src[kk++] = i;
			}
			src[n] = kk;
		}
		__syncthreads();
		kept = src[n];
	} else {
		for (int i = lane; i < n; i += 64) src[i] = i;
		__syncthreads();
	}
	const bool sync = kept != n;                                                // hit.c:269
	if (sync) {
		for (int t = lane; t < kept; t += 64) newidx[src[t]] = t;
		__syncthreads();
	}

	// ---- the records ----
	for (int e = lane; e < kept * REG_WORDS; e += 64) {
		const int t = e / REG_WORDS, wd = e - t * REG_WORDS, s = src[t];
		uint64_t v = in[(int64_t)s * REG_WORDS + wd];
		if (wd == reg_word(REG_ID)) v = reg_with<REG_ID>(v, (uint32_t)(sync ? t : s));
		else if (wd == reg_word(REG_PARENT)) v = reg_put<REG_PARENT>((uint32_t)(sync ? newidx[T.parent[s]] : T.parent[s])) | reg_put<REG_SUBSC>((uint32_t)T.subsc[s]);
		else if (wd == reg_word(REG_N_SUB)) v = reg_with<REG_N_SUB>(v, (uint32_t)T.nsub[s]);
		else if (wd == reg_word(REG_FLAGS) && sync) v = (v & ~reg_put<REG_FLAGS>(REG_SAM_PRI)) | reg_put<REG_FLAGS>(t == 0 ? REG_SAM_PRI : 0u);   // hit.c:220-229: region 0 is the first primary
		out[(int64_t)t * REG_WORDS + wd] = v;
	}
	if (lane == 0) { *n_out = kept; atomicAdd(A.total, (unsigned long long)kept); }
}

template <bool MULTI>
__device__ __forceinline__ void hits_block(const HitArgs &A)
{
	__shared__ int32_t s_tab[HITS_TAB_ROWS + (MULTI ? 1 : 0)][HITS_LDS_MAX + 1];
	__shared__ int2 s_pq[HITS_LDS_MAX], s_cov[HITS_LDS_MAX];
	const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
	const int64_t base = A.u_off[r], n64 = A.u_off[r + 1] - base;
	if (base < 0 || n64 < 0 || n64 > INT_MAX || base + n64 > A.n_u_cap) {
		if (lane == 0) atomicAdd(&A.flags[0], 1);                                // offsets that leave the plan's capacities: nothing of this read is touched
		return;
	}
	const int n = (int)n64;
	if (n == 0) { if (lane == 0) A.n_out[r] = 0; return; }
	MultiFrag F;
	F.q0 = 0; F.max_dist = 0; F.two = false;
	if constexpr (MULTI) {
		if (A.n_segs == 2) {                                                     // pe.c:10, in wrapping int
			const int32_t *ql = A.seg_len + (int64_t)r * 2;
			F.two = true; F.q0 = ql[0];
			F.max_dist = (int32_t)((uint32_t)ql[0] + (uint32_t)ql[1] + (uint32_t)(A.gap_ref ? A.gap_ref[r] : A.max_gap_ref));
		}
	}
	const uint64_t *in = A.in + base * REG_WORDS;
	uint64_t *out = A.out + base * REG_WORDS;
	HitTab T;
	if (n <= HITS_LDS_MAX) {
		T.qs = s_tab[0]; T.qe = s_tab[1]; T.score = s_tab[2]; T.cnt = s_tab[3]; T.subsc = s_tab[4]; T.nsub = s_tab[5]; T.parent = s_tab[6];
		T.rid = s_tab[7]; T.rs = s_tab[8]; T.re = s_tab[9]; T.w = s_tab[10]; T.rev = MULTI ? s_tab[HITS_TAB_ROWS + (MULTI ? 1 : 0) - 1] : nullptr;
		T.pq = s_pq; T.cov = s_cov;
		hits_read<MULTI>(A, T, in, out, A.n_out + r, n, lane, F);
	} else {                                                                     // rows of n_u_cap + n_reads entries: a read's rows hold one entry more than it has regions
		const int64_t row = A.n_u_cap + A.n_reads;
		int32_t *g = A.tab + base + r;
		T.qs = g; T.qe = g + row; T.score = g + 2 * row; T.cnt = g + 3 * row; T.subsc = g + 4 * row; T.nsub = g + 5 * row; T.parent = g + 6 * row;
		T.rid = g + 7 * row; T.rs = g + 8 * row; T.re = g + 9 * row; T.w = g + 10 * row; T.rev = MULTI ? g + 11 * row : nullptr;
		T.pq = A.pq + base; T.cov = A.cov + base;
		hits_read<MULTI>(A, T, in, out, A.n_out + r, n, lane, F);
	}
}

__global__ __launch_bounds__(64) void hits_select(HitArgs A) { hits_block<false>(A); }
__global__ __launch_bounds__(64) void hits_select_multi(HitArgs A) { hits_block<true>(A); }

} // namespace

hipError_t launch_chain_hits(const HitArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(hits_select, dim3((unsigned)A.n_reads), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_chain_hits_multi(const HitArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(hits_select_multi, dim3((unsigned)A.n_reads), dim3(64), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
