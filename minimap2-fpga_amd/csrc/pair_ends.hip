// pair_ends.hip -- the two ends of a fragment paired on the GPU, byte for byte the reference's: mm_pair with mm_set_pe_thru (pe.c:45-63, 76-177; map.c:373-374) and
// the flip of the mate that was reverse-complemented before mapping (map.c:455-466), in place on the final regions fin_select wrote.
//
// pair_select (one wave per fragment, PAIR_WAVES fragments per workgroup; the waves of a workgroup never meet, every synchronisation is wave-local).  Entry a of a
// fragment is region a of mate 0 for a < n0, else region a - n0 of mate 1.
//   check   : lanes over the entries; a fragment with one bad entry is refused before anything is written.  The same pass keeps parent and flags of every entry in
//             two rows (all updates are made there and stored at the end) and finds max(0, max dp_max) per mate.
//   early   : pe.c:97-100: one mate without regions -> only the flip.
//   sort    : key = rid << 32 | rs << 1 | (s ^ rev), ascending by klib's radix_sort_pair.  Ties are real (two regions of one mate at one rs).  Up to 64 records
//             klib sorts by insertion = stable: every lane ranks its key against the others.  Above 64: stable wave_sort64, the replay of radix_replay.h when keys
//             are equal, the stable sort of the replayed arrangement -- as regs_sort and fin_select do.
//   rows    : per entry in sorted order: mate / rev / key parity, rid, rs, re, dp_max, hash, and last = the latest even-key entry of the same rev in front (a wave
//             prefix per rev, carried over the chunks of 64).
//   walk    : pe.c:109-130, one lane per odd-key entry: the first test against the entry at `last`, then down from it.  Every lane keeps its best score with the
//             entry pair, its two largest scores as unsigned words (sc is a uint64_t array) and its count; the wave reduces them, the best by (score, first i).
//             A second walk counts the scores whose high word + sub_diff reaches the maximum's: sc is never sorted, radix_sort_64 has no counterpart.
//   found   : proper_frag, the lift per mate, sam_pri, the mapq of pe.c:153-170 in IEEE single precision as written (-ffp-contract=off) with logf((float)n_sub)
//             from the table the host filled with its own logf.
//   pe_thru : pe.c:45-63 on the rows behind the lifts.      flip: map.c:455-466, last, also with one mate empty.
//   store   : word 4 (parent) and word 7 (flags) of every entry when both mates have regions, word 2 (qs, qe) of a flipped mate.
// Refused (status 1, counted, nothing of the fragment written): offsets or counts that leave the capacities or each other; a region with p == 0 or a p that names no
// record; rid < 0; rs < 0 or rs >= 2^30; id that is not the region's position; parent outside the mate.
// Plain vector stores only; the only atomics are the integer adds of the counters.

#include <hip/hip_runtime.h>
#include <climits>
#include "pair_ends.h"
#include "chain_regs.h"
#include "radix_replay.h"
#include "wave_sort.h"

namespace mm2c {

namespace {

constexpr uint32_t PAIR_REV = 1u << REG_REV_BIT, PAIR_PROPER = 1u << 13, PAIR_THRU = 1u << 14;
constexpr int PAIR_ROW = PAIR_LDS_MAX + 2;                                     // even, so every wave's rows are 8-byte aligned
static_assert((PAIR_TAB_ROWS - PAIR_SORT_ROW) * PAIR_ROW >= 576 + 257 + 1 && (PAIR_TAB_ROWS * PAIR_ROW) % 2 == 0 && (PAIR_SORT_ROW * PAIR_ROW) % 2 == 0, "LDS rows");

struct PairTab {
	int32_t *ord, *tmp;                                                        // sorted position -> entry
	int32_t *par, *fl;                                                         // by entry: parent and flags as they will be stored
	int32_t *info, *rid, *rs, *re, *dpmax, *hash, *last;                       // by sorted position; info: mate | rev << 1 | key parity << 2
};

__device__ __forceinline__ void psync() { rp_wave_sync(); }

// pe.c:116-126 for the odd-key entry at sorted position i: fn(j, score) for every candidate that reaches kv_push
template <class Fn>
__device__ __forceinline__ void pair_walk(const PairTab &T, const int i, const int gap, const int dp_thres, Fn fn)
{
	const int L = T.last[i];
	if (L < 0) return;                                                         // pe.c:112
	const int inf = T.info[i], rid = T.rid[i], rs = T.rs[i], dm = T.dpmax[i];
	const uint32_t hs = (uint32_t)T.hash[i];
	if (rid != T.rid[L] || (int32_t)((uint32_t)rs - (uint32_t)T.re[L]) > gap) return;   // pe.c:115: against a[last] whatever its mate
	for (int j = L; j >= 0; --j) {
		const int ij = T.info[j];
		if (((ij ^ inf) & 2) || !((ij ^ inf) & 1)) continue;                   // another rev, or the same mate
		if (rid != T.rid[j] || (int32_t)((uint32_t)rs - (uint32_t)T.re[j]) > gap) break;
		const int32_t sum = (int32_t)((uint32_t)dm + (uint32_t)T.dpmax[j]);
		if (sum < dp_thres) continue;
		fn(j, (int64_t)((uint64_t)(int64_t)sum << 32 | (uint64_t)(hs + (uint32_t)T.hash[j])));
	}
}

__device__ __forceinline__ void pair_frag(const PairArgs &A, PairTab T, const int64_t base, const int64_t b0, const int64_t b1, const int n0, const int n1, int *s_sort,
                                          const int64_t f, const int lane)
{
	const int n = n0 + n1;
	uint64_t *const regs = A.regs;
	auto rec = [&](int a) -> uint64_t * { return regs + (a < n0 ? b0 + a : b1 + (a - n0)) * REG_WORDS; };

	// ---- what is refused; parent and flags of every entry; max dp_max per mate (pe.c:84-96) ----
	bool bad = false;
	int mx0 = 0, mx1 = 0;
	uint64_t key_reg = 0;                                                      // the key of entry `lane` when n <= 64
	for (int a0 = 0; a0 < n; a0 += 64) {
		const int a = a0 + lane;
		if (a < n) {
			const uint64_t *g = rec(a);
			const uint64_t w0 = g[0], w1 = g[1], w3 = g[3], w4 = g[4], w7 = g[7], p = g[REG_WORDS - 1];
			const int s = a >= n0, i = s ? a - n0 : a, ns = s ? n1 : n0;
			const int32_t id = reg_of<REG_ID>(w0), rid = reg_of<REG_RID>(w1), rs = reg_of<REG_RS>(w3), parent = reg_of<REG_PARENT>(w4);
			const uint32_t fl = (uint32_t)reg_of<REG_FLAGS>(w7);
			bool ok = p != 0 && p - 1 < (uint64_t)A.n_pext_cap && rid >= 0 && rs >= 0 && rs < (1 << 30) && id == i && parent >= 0 && parent < ns;
			if (ok) {
				const int32_t dm = A.pext[p - 1].dp_max;
				if (s) mx1 = imax(mx1, dm); else mx0 = imax(mx0, dm);
				const uint64_t key = (uint64_t)(uint32_t)rid << 32 | (uint32_t)(rs << 1 | (s ^ (int)(fl >> REG_REV_BIT & 1u)));
				key_reg = key;
				if (n > 64) A.zkey[base + a] = key;
				T.par[a] = parent; T.fl[a] = (int32_t)fl;
			} else bad = true;
		}
	}
	if (__any(bad)) { if (lane == 0) { A.status[f] = 1; atomicAdd(&A.flags[0], 1); } return; }
	if (lane == 0) A.status[f] = 0;
	psync();

	const bool both = n0 > 0 && n1 > 0;                                        // pe.c:97-100
	if (both) {
		int dp_thres = (int32_t)((uint32_t)wave_max(mx0) + (uint32_t)wave_max(mx1) - (uint32_t)A.pe_bonus);
		if (dp_thres < 0) dp_thres = 0;
		const int gap = A.gap_ref ? A.gap_ref[f] : A.max_gap_ref;

		// ---- radix_sort_pair (pe.c:103) ----
		if (n <= 64) {
			int rank = 0;
			for (int j = 0; j < n; ++j) {
				const uint64_t kj = __shfl(key_reg, j);
				rank += kj < key_reg || (kj == key_reg && j < lane);
			}
			if (lane < n) T.ord[rank] = lane;
		} else {
			int *s_cur = s_sort, *s_lo = s_sort + 576, *s_sp = s_sort + 576 + 257;
			uint64_t *zkey = A.zkey + base, *key0 = A.key0 + base, *key1 = A.key1 + base;
			int32_t *val0 = A.val0 + base, *val1 = A.val1 + base, *tiecnt = A.tiecnt + base, *stack = A.stack + base, *moved = A.moved + base;
			for (int a = lane; a < n; a += 64) { key0[a] = zkey[a]; val0[a] = a; }
			psync();
			wave_sort64<false, true>(key0, key1, val0, val1, n, lane, s_cur);     // ascending, stable: (key1, val1)
			int ties = 0;
			for (int i0 = 0; i0 < n; i0 += 64) {                                 // tiecnt[i] = equal neighbours before position i of the sorted keys
				const int i = i0 + lane;
				const int flag = (i + 1 < n && key1[i] == key1[i + 1]) ? 1 : 0;
				const int incl = wave_incl_sum(flag, lane);
				if (i < n) tiecnt[i] = ties + incl - flag;
				ties += __shfl(incl, 63);
			}
			if (ties > 0) {                                                      // the replay through global memory, as fin_select
				psync();
				uint8_t *g_dg = (uint8_t *)(stack + 2 * (n / 64 + 2));
				replay_passes<uint32_t, false, false>(zkey, 1, key1, 1, tiecnt, n, (uint32_t *)val0, g_dg, stack, moved, nullptr, nullptr, lane, s_cur, s_lo, s_sp);
				psync();
				for (int i = lane; i < n; i += 64) key1[i] = zkey[val0[i]];      // keys of the replayed arrangement
				psync();
				wave_sort64<false, true>(key1, key0, val0, val1, n, lane, s_cur);
			}
			psync();
			for (int i = lane; i < n; i += 64) T.ord[i] = val1[i];
		}
		psync();

		// ---- the rows, in sorted order; last[] (pe.c:112, 128) ----
		int carry0 = -1, carry1 = -1;
		for (int t0 = 0; t0 < n; t0 += 64) {
			const int t = t0 + lane;
			int rev = 0, odd = 1;
			if (t < n) {
				const int a = T.ord[t];
				const uint64_t *g = rec(a);
				const uint64_t w1 = g[1], w3 = g[3], w8 = g[8], p = g[REG_WORDS - 1];
				const int s = a >= n0;
				rev = (int)((uint32_t)T.fl[a] >> REG_REV_BIT & 1u);
				odd = s ^ rev;
				T.info[t] = s | rev << 1 | odd << 2;
				T.rid[t] = reg_of<REG_RID>(w1); T.rs[t] = reg_of<REG_RS>(w3); T.re[t] = reg_of<REG_RE>(w3); T.hash[t] = reg_of<REG_HASH>(w8);
				T.dpmax[t] = A.pext[p - 1].dp_max;
			}
			const int l0 = wave_incl_last(!odd && rev == 0 ? t : -1, lane), l1 = wave_incl_last(!odd && rev == 1 ? t : -1, lane);
			const int m0 = l0 >= 0 ? l0 : carry0, m1 = l1 >= 0 ? l1 : carry1;
			if (t < n) T.last[t] = rev ? m1 : m0;
			carry0 = __shfl(m0, 63); carry1 = __shfl(m1, 63);
		}
		psync();

		// ---- the scan (pe.c:109-130) ----
		int64_t best = -1;
		int bi = INT_MAX, bj = -1, cnt = 0;
		uint64_t u1 = 0, u2 = 0;                                                 // the two largest of sc as unsigned words (0: none yet; only read when sc.n > 1)
		for (int i = lane; i < n; i += 64) {
			if (!(T.info[i] & 4)) continue;
			pair_walk(T, i, gap, dp_thres, [&](int j, int64_t score) {
				if (score > best) { best = score; bi = i; bj = j; }
				const uint64_t u = (uint64_t)score;
				if (u >= u1) { u2 = u1; u1 = u; } else if (u > u2) u2 = u;
				++cnt;
			});
		}
		for (int o = 32; o > 0; o >>= 1) {
			const int64_t ob = __shfl_xor(best, o);
			const int oi = __shfl_xor(bi, o), oj = __shfl_xor(bj, o);
			if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; bj = oj; }   // the first in scan order among equal scores
			const uint64_t o1 = __shfl_xor(u1, o), o2 = __shfl_xor(u2, o);
			const uint64_t second = u1 >= o1 ? (u2 > o1 ? u2 : o1) : (u1 > o2 ? u1 : o2);
			u1 = u1 >= o1 ? u1 : o1; u2 = second;
		}
		const int n_sc = wave_sum(cnt);

		if (n_sc > 0 && best > 0) {                                              // pe.c:134: found at least one pair
			const uint64_t maxhi = (uint64_t)best >> 32;
			int sub = 0;
			for (int i = lane; i < n; i += 64) {                                 // pe.c:154-156
				if (!(T.info[i] & 4)) continue;
				pair_walk(T, i, gap, dp_thres, [&](int, int64_t score) { sub += ((uint64_t)score >> 32) + (uint64_t)(int64_t)A.sub_diff >= maxhi; });
			}
			const int n_sub = wave_sum(sub);
			const int ai = T.ord[bi], aj = T.ord[bj];
			const int w0 = ai < n0 ? ai : aj, w1 = ai < n0 ? aj : ai;             // the winner of either mate, as an entry
			psync();
			for (int s = 0; s < 2; ++s) {
				const int lo = s ? n0 : 0, ns = s ? n1 : n0, win = s ? w1 : w0;
				const int wpar = T.par[win], wfl = T.fl[win];
				psync();
				const bool lift = wpar != win - lo;                              // pe.c:140: ids are positions
				const bool pri = !((uint32_t)wfl & REG_SAM_PRI);
				for (int i = lane; i < ns; i += 64) {
					int par = T.par[lo + i];
					uint32_t fl = (uint32_t)T.fl[lo + i];
					if (lift) {
						if (par == wpar) par = win - lo;                         // pe.c:143-144
						if (i == wpar) fl &= ~0xffu;                             // pe.c:145
					}
					if (pri) fl = (fl & ~REG_SAM_PRI) | (lo + i == win ? REG_SAM_PRI : 0u);
					if (lo + i == win) fl |= PAIR_PROPER;
					T.par[lo + i] = par; T.fl[lo + i] = (int32_t)fl;
				}
				psync();
			}
			// pe.c:153-170
			const uint32_t f0 = (uint32_t)T.fl[w0], f1 = (uint32_t)T.fl[w1];
			int q0 = (int)(f0 & 0xffu), q1 = (int)(f1 & 0xffu);
			int mapq_pe = q0 > q1 ? q0 : q1;
			const uint64_t sechi = u2 >> 32;
			bool beyond = false;
			if (n_sc > 1) {
				if (n_sub > A.max_log_arg) beyond = true;
				else {
					const int mapq_pe_alt = (int)(6.02f * (float)(maxhi - sechi) / (float)A.match_sc - 4.343f * A.logtab[n_sub]);
					mapq_pe = mapq_pe < mapq_pe_alt ? mapq_pe : mapq_pe_alt;
				}
			}
			if (!beyond) {
				if (q0 < mapq_pe) q0 = (int)(.2f * (float)q0 + .8f * (float)mapq_pe + .499f);
				if (q1 < mapq_pe) q1 = (int)(.2f * (float)q1 + .8f * (float)mapq_pe + .499f);
				if (n_sc == 1) { q0 = q0 < 2 ? 2 : q0; q1 = q1 < 2 ? 2 : q1; }
				else if (maxhi > sechi) { q0 = q0 < 1 ? 1 : q0; q1 = q1 < 1 ? 1 : q1; }
			}
			psync();
			if (lane == 0) {
				T.fl[w0] = (int32_t)((f0 & ~0xffu) | ((uint32_t)q0 & 0xffu));
				T.fl[w1] = (int32_t)((f1 & ~0xffu) | ((uint32_t)q1 & 0xffu));
				if (beyond) atomicAdd(&A.counts[0], 1ull);
				atomicAdd(&A.counts[1 + (blockIdx.x & (PAIR_PROPER_SLOTS - 1))], 1ull);   // one address for every fragment would be the kernel's bound (12 ns an add)
			}
			psync();
		}

		// ---- mm_set_pe_thru (pe.c:45-63), behind the lifts ----
		int np0 = 0, np1 = 0, p0 = -1, p1 = -1;
		for (int a = lane; a < n; a += 64) {
			const int s = a >= n0;
			if (T.par[a] == (s ? a - n0 : a)) { if (s) { ++np1; p1 = a; } else { ++np0; p0 = a; } }
		}
		np0 = wave_sum(np0); np1 = wave_sum(np1);
		if (np0 == 1 && np1 == 1) {
			p0 = wave_max(p0); p1 = wave_max(p1);
			const uint64_t *gp = rec(p0), *gq = rec(p1);
			const int32_t prid = reg_of<REG_RID>(gp[1]), qrid = reg_of<REG_RID>(gq[1]);
			const int32_t pqs = reg_of<REG_QS>(gp[2]), pqe = reg_of<REG_QE>(gp[2]), qqs = reg_of<REG_QS>(gq[2]), qqe = reg_of<REG_QE>(gq[2]);
			const int32_t prs = reg_of<REG_RS>(gp[3]), pre = reg_of<REG_RE>(gp[3]), qrs = reg_of<REG_RS>(gq[3]), qre = reg_of<REG_RE>(gq[3]);
			const uint32_t pf = (uint32_t)T.fl[p0], qf = (uint32_t)T.fl[p1];
			const int32_t ds = (int32_t)((uint32_t)prs - (uint32_t)qrs), de = (int32_t)((uint32_t)pre - (uint32_t)qre);
			const int32_t ql0 = A.seg_len[2 * f], ql1 = A.seg_len[2 * f + 1];
			const bool thru = prid == qrid && !((pf ^ qf) & PAIR_REV) && (ds < 0 ? -ds : ds) < 3 && (de < 0 ? -de : de) < 3 &&
			                  ((pqs == 0 && (int32_t)((uint32_t)ql1 - (uint32_t)qqe) == 0) || (qqs == 0 && (int32_t)((uint32_t)ql0 - (uint32_t)pqe) == 0));
			psync();
			if (thru && lane == 0) { T.fl[p0] = (int32_t)(pf | PAIR_THRU); T.fl[p1] = (int32_t)(qf | PAIR_THRU); }
			psync();
		}
	}

	// ---- the flip (map.c:455-466) and the stores ----
	for (int a = lane; a < n; a += 64) {
		const int s = a >= n0;
		uint64_t *g = rec(a);
		const bool flipped = A.flip && (s ? (A.pe_ori & 1) : (A.pe_ori >> 1 & 1));
		uint32_t fl = (uint32_t)T.fl[a];
		if (flipped) {
			const uint64_t w2 = g[2];
			const uint32_t qlen = (uint32_t)A.seg_len[2 * f + s], qs = (uint32_t)reg_of<REG_QS>(w2), qe = (uint32_t)reg_of<REG_QE>(w2);
			g[2] = reg_put<REG_QS>(qlen - qe) | reg_put<REG_QE>(qlen - qs);
			fl ^= PAIR_REV;
		}
		if (both || flipped) g[7] = reg_with<REG_FLAGS>(g[7], fl);
		if (both) g[4] = reg_with<REG_PARENT>(g[4], (uint32_t)T.par[a]);
	}
}

__global__ __launch_bounds__(64 * PAIR_WAVES) void pair_select(PairArgs A)
{
	__shared__ __attribute__((aligned(8))) int32_t s_tab[PAIR_WAVES][PAIR_TAB_ROWS][PAIR_ROW];
	const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
	const int64_t f = (int64_t)blockIdx.x * PAIR_WAVES + wave;
	if (f >= A.n_frags) return;
	const int64_t b0 = A.f_off[2 * f], b1 = A.f_off[2 * f + 1], b2 = A.f_off[2 * f + 2], n0 = A.n[2 * f], n1 = A.n[2 * f + 1];
	if (b0 < 0 || b1 < b0 || b2 < b1 || b2 > A.n_u_cap || b2 - b0 > INT_MAX || n0 < 0 || n0 > b1 - b0 || n1 < 0 || n1 > b2 - b1) {
		if (lane == 0) { A.status[f] = 1; atomicAdd(&A.flags[0], 1); }             // offsets or counts that leave the capacities or each other: nothing of this fragment is touched
		return;
	}
	const int n = (int)(n0 + n1);
	if (n == 0) { if (lane == 0) A.status[f] = 0; return; }
	int32_t *rows[PAIR_TAB_ROWS];
	if (n <= PAIR_LDS_MAX) for (int k = 0; k < PAIR_TAB_ROWS; ++k) rows[k] = s_tab[wave][k];
	else for (int k = 0; k < PAIR_TAB_ROWS; ++k) rows[k] = A.tab + b0 + k * A.n_u_cap;   // n <= b2 - b0 entries of every row are this fragment's
	PairTab T;
	T.ord = rows[0]; T.tmp = rows[1]; T.par = rows[2]; T.fl = rows[3]; T.info = rows[4]; T.rid = rows[5]; T.rs = rows[6]; T.re = rows[7]; T.dpmax = rows[8];
	T.hash = rows[9]; T.last = rows[10];
	pair_frag(A, T, b0, b0, b1, (int)n0, (int)n1, s_tab[wave][PAIR_SORT_ROW], f, lane);
}

} // namespace

hipError_t launch_pair_select(const PairArgs &A, hipStream_t st)
{
	if (A.n_frags <= 0) return hipSuccess;
	hipLaunchKernelGGL(pair_select, dim3((unsigned)((A.n_frags + PAIR_WAVES - 1) / PAIR_WAVES)), dim3(64 * PAIR_WAVES), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
