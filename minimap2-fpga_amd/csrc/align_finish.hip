// align_finish.hip -- the hit-level steps of a read mapped with base alignment (-c / -a), on the GPU, byte for byte the reference's.
//
// fin_apply (one lane per region): what mm_align1 leaves in r (align.c:781-783 and what mm_update_extra put into r->p), with mm_split_reg (hit.c:108-123) where the
//   reference runs it -- in the middle of mm_align1 (align.c:757-760), on the region as the chain left it.  The child r2 is *r of that moment with its own cnt,
//   score, as, parent, coordinates and fuzzy lengths (mm_reg_set_coor, hit.c:23-38, walks the child's anchors); the score is one float division, one product in
//   float, then a DOUBLE add of .499 and a truncation.  The children go to a dense list in region order: a block scan of "splits" gives every region its slot.
//
// fin_select (one wave per read, FIN_WAVES reads per workgroup; the waves of a workgroup never meet, every synchronisation is wave-local): six reference calls.
//   filter    : mm_filter_regs (hit.c:274-293), lanes; the survivors keep their order (ballots).  The clip test is an int -> float product in float and an
//               int-against-float compare in float, as written.
//   sort      : mm_hit_sort (hit.c:188-218), only for more than one survivor: regions with cnt <= 0 go, the key is (uint64_t)score << 32 | hash with score = dp_max
//               under p; ascending by klib's radix_sort_128x, then reversed.  Ties are real (a split child carries its parent's hash).  Up to 64 records klib
//               sorts by insertion = stable: every lane ranks its key against the others.  Above 64: stable wave_sort64, the replay of radix_replay.h when keys
//               are equal, the stable sort of the replayed arrangement -- as regs_sort does for hit.c:65.  A read that mixes kept regions with and without p is
//               refused: the reference asserts there (hit.c:210).
//   tables    : per region in sorted order, in LDS up to FIN_LDS_MAX regions and in the plan's scratch beyond, the same code on the two kinds of pointer.
//   set_parent: hits_select's walk (chain_hits.hip) with hit.c:171-176: dp_max2 of the primary, and cnt_sub from sub_diff, unless the pair is identical after DP.
//   select_sub: hits_select's; a dropped region's p is dropped with it.
//   sam_pri   : hit.c:220-229, always (map.c:267): bit 12 on the first region with id == parent.
//   mapq      : hit.c:463-506, all three branches, in IEEE single precision as written (-ffp-contract=off); the logarithms are looked up in two tables the host
//               filled with its own logf: L[i] = logf((float)i) and L2[i] = logf((float)i / match_sc).
//   move      : the 80-byte records go from the input to the output through sort order and source map, patched on the way; dp_max2 goes to the p records.
//   With all_chains (MM_F_ALL_CHAINS) set_parent, select_sub and sam_pri are skipped (map.c:264): id and parent stay what the input holds.
// Refused, nothing of the read written: offsets that leave the capacities, a region with inv or is_alt, a p that names no record, mixed p.
// Plain vector stores only; the only atomics are the integer adds of the counters.

#include <hip/hip_runtime.h>
#include <climits>
#include "align_finish.h"
#include "chain_regs.h"
#include "radix_replay.h"
#include "wave_sort.h"

namespace mm2c {

namespace {

constexpr uint32_t FLAG_INV = 1u << 11, FLAG_IS_ALT = 1u << 25;                // minimap.h:96: mapq:8, split:2, rev:1, inv:1, ... split_inv:1, is_alt:1
constexpr int FIN_ROW = FIN_LDS_MAX + 2;                                       // a read's rows hold one entry more than it has regions; even, so every wave's rows are 8-byte aligned
static_assert((FIN_TAB_ROWS - FIN_SORT_ROW) * FIN_ROW >= 576 + 257 + 1 && (FIN_TAB_ROWS * FIN_ROW) % 2 == 0 && (FIN_SORT_ROW * FIN_ROW) % 2 == 0, "LDS rows");

struct FinTab {
	int32_t *ord, *tmp;                                                        // sorted position -> region of the input; a second row for the sort, then the new indices
	int32_t *qs, *qe, *score, *cnt, *subsc, *nsub, *parent, *rid, *rs, *re, *w, *dpmax, *dpmax2, *pidx, *idv;
	int2 *pq, *cov;
};

__device__ __forceinline__ void wsync() { rp_wave_sync(); }

// the sort key of hit.c:203 for region i of the input
__device__ __forceinline__ uint64_t fin_key(const FinArgs &A, const uint64_t *in, int i)
{
	const uint64_t *g = in + (int64_t)i * REG_WORDS;
	const uint64_t p = g[REG_WORDS - 1];
	const int32_t score = p ? A.pext[p - 1].dp_max : reg_of<REG_SCORE>(g[reg_word(REG_SCORE)]);
	return (uint64_t)(uint32_t)score << 32 | (uint32_t)reg_of<REG_HASH>(g[reg_word(REG_HASH)]);
}

__device__ __forceinline__ void fin_read(const FinArgs &A, FinTab T, const uint64_t *in, uint64_t *out, const int64_t base, int *s_sort, const int64_t r, const int n_in,
                                         const int lane)
{
	const uint64_t lt = (1ull << lane) - 1;
	const int32_t qlen = A.qlen[r];
	const float clip = (float)qlen * A.max_clip_ratio;                           // hit.c:284: int * float

	// ---- what is refused; mm_filter_regs (hit.c:274-293) ----
	int n1 = 0;
	bool bad_flag = false, bad_p = false;
	for (int i0 = 0; i0 < n_in; i0 += 64) {
		const int i = i0 + lane;
		bool keep = false;
		if (i < n_in) {
			const uint64_t *g = in + (int64_t)i * REG_WORDS;
			const uint64_t w0 = g[0], w2 = g[2], w5 = g[5], w7 = g[7], p = g[REG_WORDS - 1];
			const uint32_t fl = (uint32_t)reg_of<REG_FLAGS>(w7);
			const int32_t cnt = reg_of<REG_CNT>(w0), qs = reg_of<REG_QS>(w2), qe = reg_of<REG_QE>(w2), mlen = reg_of<REG_MLEN>(w5);
			bad_flag |= (fl & (FLAG_INV | FLAG_IS_ALT)) != 0;
			bool flt = !(fl & REG_SEG_SPLIT) && cnt < A.min_cnt;
			if (p != 0) {
				if (p - 1 >= (uint64_t)A.n_pext_cap) bad_p = true;
				else if (mlen < A.min_chain_score) flt = true;
				else if (A.pext[p - 1].dp_max < A.min_dp_max) flt = true;
				else if ((float)qs > clip && (float)(int32_t)((uint32_t)qlen - (uint32_t)qe) > clip) flt = true;
			}
			keep = !flt;
		}
		const uint64_t m = __ballot(keep);
		if (keep) T.ord[n1 + __popcll(m & lt)] = i;
		n1 += __popcll(m);
	}
	if (__any(bad_flag)) { if (lane == 0) atomicAdd(&A.flags[1], 1); return; }
	if (__any(bad_p)) { if (lane == 0) atomicAdd(&A.flags[2], 1); return; }
	wsync();

	// ---- mm_hit_sort (hit.c:188-218) ----
	int n2 = n1;
	if (n1 > 1) {
		int k = 0;
		bool has = false, no = false;
		for (int t0 = 0; t0 < n1; t0 += 64) {                                    // hit.c:198: cnt > 0 (inv is refused), packed in place
			const int t = t0 + lane;
			int i = 0;
			bool live = false;
			if (t < n1) {
				i = T.ord[t];
				const uint64_t *g = in + (int64_t)i * REG_WORDS;
				live = reg_of<REG_CNT>(g[0]) > 0;
				if (live) { if (g[REG_WORDS - 1]) has = true; else no = true; }
			}
			const uint64_t m = __ballot(live);
			wsync();
			if (live) T.ord[k + __popcll(m & lt)] = i;
			k += __popcll(m);
			wsync();
		}
		if ((__any(has) ? 1 : 0) + (__any(no) ? 1 : 0) != 1) { if (lane == 0) atomicAdd(&A.flags[3], 1); return; }   // hit.c:210
		n2 = k;
		if (n2 <= 64) {                                                          // ksort.h: an insertion sort, stable; then the reversal
			uint64_t key = 0;
			int i = 0;
			if (lane < n2) { i = T.ord[lane]; key = fin_key(A, in, i); }
			int rank = 0;
			for (int j = 0; j < n2; ++j) {
				const uint64_t kj = __shfl(key, j);
				rank += kj < key || (kj == key && j < lane);
			}
			wsync();
			if (lane < n2) T.ord[n2 - 1 - rank] = i;
		} else {
			int *s_cur = s_sort, *s_lo = s_sort + 576, *s_sp = s_sort + 576 + 257;
			uint64_t *zkey = A.zkey + base, *key0 = A.key0 + base, *key1 = A.key1 + base;
			int32_t *val0 = A.val0 + base, *val1 = A.val1 + base, *tiecnt = A.tiecnt + base, *stack = A.stack + base, *moved = A.moved + base;
			for (int a = lane; a < n2; a += 64) {
				const uint64_t z = fin_key(A, in, T.ord[a]);
				zkey[a] = z; key0[a] = z; val0[a] = a;
			}
			wsync();
			wave_sort64<false, true>(key0, key1, val0, val1, n2, lane, s_cur);    // ascending, stable: (key1, val1)
			int ties = 0;
			for (int i0 = 0; i0 < n2; i0 += 64) {                                // tiecnt[i] = equal neighbours before position i of the sorted keys
				const int i = i0 + lane;
				const int flag = (i + 1 < n2 && key1[i] == key1[i + 1]) ? 1 : 0;
				const int incl = wave_incl_sum(flag, lane);
				if (i < n2) tiecnt[i] = ties + incl - flag;
				ties += __shfl(incl, 63);
			}
			if (ties > 0) {                                                      // the replay through global memory, as regs_sort beyond its LDS
				wsync();
				uint8_t *g_dg = (uint8_t *)(stack + 2 * (n2 / 64 + 2));
				replay_passes<uint32_t, false, false>(zkey, 1, key1, 1, tiecnt, n2, (uint32_t *)val0, g_dg, stack, moved, nullptr, nullptr, lane, s_cur, s_lo, s_sp);
				wsync();
				for (int i = lane; i < n2; i += 64) key1[i] = zkey[val0[i]];     // keys of the replayed arrangement
				wsync();
				wave_sort64<false, true>(key1, key0, val0, val1, n2, lane, s_cur);
			}
			wsync();
			for (int i = lane; i < n2; i += 64) T.tmp[n2 - 1 - i] = T.ord[val1[i]];   // hit.c:212-213
			int32_t *t = T.ord; T.ord = T.tmp; T.tmp = t;
		}
		wsync();
	}
	if (n2 == 0) { if (lane == 0) A.n_out[r] = 0; return; }

	// ---- the tables, in sorted order ----
	for (int t = lane; t < n2; t += 64) {
		const uint64_t *g = in + (int64_t)T.ord[t] * REG_WORDS;
		const uint64_t w0 = g[0], w1 = g[1], w2 = g[2], w3 = g[3], w4 = g[4], w6 = g[6], p = g[REG_WORDS - 1];
		T.cnt[t] = reg_of<REG_CNT>(w0); T.rid[t] = reg_of<REG_RID>(w1); T.score[t] = reg_of<REG_SCORE>(w1);
		T.qs[t] = reg_of<REG_QS>(w2); T.qe[t] = reg_of<REG_QE>(w2); T.rs[t] = reg_of<REG_RS>(w3); T.re[t] = reg_of<REG_RE>(w3);
		T.parent[t] = reg_of<REG_PARENT>(w4); T.subsc[t] = reg_of<REG_SUBSC>(w4); T.nsub[t] = reg_of<REG_N_SUB>(w6);
		T.idv[t] = A.all_chains ? reg_of<REG_ID>(w0) : t;                       // hit.c:130
		int32_t dm = 0, dm2 = 0;
		if (p) { const Pext e = A.pext[p - 1]; dm = e.dp_max; dm2 = e.dp_max2; }
		T.pidx[t] = p ? (int32_t)(p - 1) : -1; T.dpmax[t] = dm; T.dpmax2[t] = dm2;
	}
	wsync();

	int32_t *src = T.w, *newidx = T.tmp;
	int kept = n2;
	bool sync = false;
	if (!A.all_chains) {
		// ---- mm_set_parent (hit.c:133-183) ----
		if (lane == 0) { T.w[0] = 0; T.parent[0] = 0; T.pq[0] = make_int2(T.qs[0], T.qe[0]); }
		wsync();
		int k = 1;
		for (int i = 1; i < n2; ++i) {
			const int si = __builtin_amdgcn_readfirstlane(T.qs[i]), ei = __builtin_amdgcn_readfirstlane(T.qe[i]);
			int uncov_len = 0;
			if (!A.hard_mask_level) {
				int n_cov = 0, len1 = 0;
				for (int j0 = 0; j0 < k; j0 += 64) {                             // hit.c:138-145
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
				if (n_cov == 1) uncov_len = (ei - si) - len1;
				else if (n_cov > 1) {                                            // hit.c:148-156 as a measure (chain_hits.hip)
					wsync();
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
					wsync();
				}
			}
			int found = -1;
			for (int j0 = 0; j0 < k && found < 0; j0 += 64) {                    // hit.c:158-165
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
				if (found >= 0) {                                                // hit.c:166-178
					const int pi = T.w[found], sci = T.score[i];
					T.parent[i] = pi;
					if (T.subsc[pi] < sci) T.subsc[pi] = sci;
					bool cnt_sub = T.cnt[i] >= T.cnt[pi];
					if (T.pidx[pi] >= 0 && T.pidx[i] >= 0) {                     // hit.c:171-176
						const int sj = T.qs[pi], ej = T.qe[pi];
						const int mn = ej - sj < ei - si ? ej - sj : ei - si;
						const int ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
						if (T.rid[pi] != T.rid[i] || T.rs[pi] != T.rs[i] || T.re[pi] != T.re[i] || ol != mn) {   // not identical after DP
							const int di = T.dpmax[i];
							if (T.dpmax2[pi] < di) T.dpmax2[pi] = di;
							if ((int32_t)((uint32_t)T.dpmax[pi] - (uint32_t)di) <= A.sub_diff) cnt_sub = true;
						}
					}
					if (cnt_sub) ++T.nsub[pi];
				} else {                                                         // hit.c:182
					T.w[k] = i; T.pq[k] = make_int2(si, ei); T.parent[i] = i; T.nsub[i] = 0;
				}
			}
			if (found < 0) ++k;
			wsync();
		}

		// ---- mm_select_sub (hit.c:257-270): which regions stay, and which region a kept position comes from (w has served) ----
		if (A.pri_ratio > 0.0f) {
			if (lane == 0) {
				int kk = 0, n_2nd = 0;
				for (int i = 0; i < n2; ++i) {
					const int p = T.parent[i];
					bool keep = p == i;
					if (!keep) {
						const int pp = kk > p ? src[p] : p;                      // what lies at position p by now
						const int sc = T.score[i], scp = T.score[pp];
						if (((float)sc >= (float)scp * A.pri_ratio || (int32_t)((uint32_t)sc + (uint32_t)A.min_diff) >= scp) && n_2nd < A.best_n) {
							if (!(T.qs[i] == T.qs[pp] && T.qe[i] == T.qe[pp] && T.rid[i] == T.rid[pp] && T.rs[i] == T.rs[pp] && T.re[i] == T.re[pp])) keep = true, ++n_2nd;
						}
					}
					if (keep) src[kk++] = i;
				}
				src[n2] = kk;
			}
			wsync();
			kept = src[n2];
		} else {
			for (int i = lane; i < n2; i += 64) src[i] = i;
			wsync();
		}
		sync = kept != n2;                                                       // hit.c:269
		if (sync) {
			for (int t = lane; t < kept; t += 64) newidx[src[t]] = t;
			wsync();
		}
	} else {
		for (int i = lane; i < n2; i += 64) src[i] = i;
		wsync();
	}

	// ---- the final ids and parents; mm_set_sam_pri (hit.c:220-229); mm_set_mapq (hit.c:463-506) ----
	long long sum_sc = 0;
	int first_pri = INT_MAX;
	int32_t *fpar = T.rs, *fmapq = T.re;                                         // (rs and re have served once the parents are read below)
	for (int t0 = 0; t0 < kept; t0 += 64) {
		const int t = t0 + lane;
		int fp = 0;
		if (t < kept) {
			const int s = src[t];
			fp = sync ? newidx[T.parent[s]] : T.parent[s];
			if (fp == (sync ? t : T.idv[s])) { sum_sc += T.score[s]; first_pri = first_pri < t ? first_pri : t; }
		}
		wsync();
		if (t < kept) fpar[t] = fp;                                              // t <= src[t]: rows rs / re are not read by index any more
	}
	sum_sc = wave_sum(sum_sc);
	first_pri = wave_min(first_pri);
	wsync();
	const float uniq_ratio = (float)sum_sc / (float)(sum_sc + A.rep_len[r]);     // hit.c:473
	for (int t = lane; t < kept; t += 64) {
		const int s = src[t], pi = T.pidx[s];
		int mapq = 0;
		if (fpar[t] == (sync ? t : T.idv[s])) {
			const uint64_t *g = in + (int64_t)T.ord[s] * REG_WORDS;
			const int32_t mlen = reg_of<REG_MLEN>(g[reg_word(REG_MLEN)]), blen = reg_of<REG_BLEN>(g[reg_word(REG_BLEN)]), score0 = reg_of<REG_SCORE0>(g[reg_word(REG_SCORE0)]);
			const int score = T.score[s], cnt = T.cnt[s], n_sub1 = (int32_t)((uint32_t)T.nsub[s] + 1u), dm = T.dpmax[s], dm2 = T.dpmax2[s];
			const int larg = pi >= 0 ? dm : score;                               // the argument of the first logarithm
			if (larg < 0 || larg > A.max_log_arg || n_sub1 < 0 || n_sub1 > A.max_log_arg) atomicAdd(&A.counts[1], 1ull);   // beyond the tables: 0, counted
			else {
				const float pen_s1 = (score > 100 ? 1.0f : 0.01f * (float)score) * uniq_ratio;
				float pen_cm = cnt > 10 ? 1.0f : 0.1f * (float)cnt;
				pen_cm = pen_s1 < pen_cm ? pen_s1 : pen_cm;
				const int subsc = T.subsc[s] > A.min_chain_score ? T.subsc[s] : A.min_chain_score;
				if (pi >= 0 && dm2 > 0 && dm > 0) {                              // hit.c:484-491
					const float identity = (float)mlen / (float)blen;
					const float x = (float)dm2 * (float)subsc / (float)dm / (float)score0;
					mapq = (int)(identity * pen_cm * 40.0f * (1.0f - x * x) * A.logtab2[dm]);
					if (!A.is_sr) {
						const int mapq_alt = (int)(6.02f * identity * identity * (float)(int32_t)((uint32_t)dm - (uint32_t)dm2) / (float)A.match_sc + .499f);
						mapq = mapq < mapq_alt ? mapq : mapq_alt;
					}
				} else {
					const float x = (float)subsc / (float)score0;
					if (pi >= 0) {                                               // hit.c:494-496
						const float identity = (float)mlen / (float)blen;
						mapq = (int)(identity * pen_cm * 40.0f * (1.0f - x) * A.logtab2[dm]);
					} else mapq = (int)(pen_cm * 40.0f * (1.0f - x) * A.logtab[score]);
				}
				mapq -= (int)(4.343f * A.logtab[n_sub1] + .499f);
				mapq = mapq > 0 ? mapq : 0;
				mapq = mapq < 60 ? mapq : 60;
				if (pi >= 0 && dm > dm2 && mapq == 0) mapq = 1;                  // hit.c:504
			}
		}
		fmapq[t] = mapq;
		if (pi >= 0 && !A.all_chains) A.pext[pi].dp_max2 = T.dpmax2[s];         // hit.c:174, on the record the region still names
	}
	wsync();

	// ---- the records ----
	for (int e = lane; e < kept * REG_WORDS; e += 64) {
		const int t = e / REG_WORDS, wd = e - t * REG_WORDS, s = src[t];
		uint64_t v = in[(int64_t)T.ord[s] * REG_WORDS + wd];
		if (wd == reg_word(REG_ID)) v = reg_with<REG_ID>(v, (uint32_t)(sync ? t : T.idv[s]));
		else if (wd == reg_word(REG_PARENT)) v = reg_put<REG_PARENT>((uint32_t)fpar[t]) | reg_put<REG_SUBSC>((uint32_t)T.subsc[s]);
		else if (wd == reg_word(REG_N_SUB)) v = reg_with<REG_N_SUB>(v, (uint32_t)T.nsub[s]);
		else if (wd == reg_word(REG_FLAGS)) {
			uint32_t fl = ((uint32_t)reg_of<REG_FLAGS>(v) & ~0xffu) | (uint32_t)fmapq[t];
			if (!A.all_chains) fl = (fl & ~REG_SAM_PRI) | (t == first_pri ? REG_SAM_PRI : 0u);
			v = reg_with<REG_FLAGS>(v, fl);
		}
		out[(int64_t)t * REG_WORDS + wd] = v;
	}
	if (lane == 0) { A.n_out[r] = kept; atomicAdd(&A.counts[0], (unsigned long long)kept); }
}

__global__ __launch_bounds__(64 * FIN_WAVES) void fin_select(FinArgs A)
{
	__shared__ __attribute__((aligned(8))) int32_t s_tab[FIN_WAVES][FIN_TAB_ROWS][FIN_ROW];
	__shared__ int2 s_pq[FIN_WAVES][FIN_LDS_MAX], s_cov[FIN_WAVES][FIN_LDS_MAX];
	const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
	const int64_t r = (int64_t)blockIdx.x * FIN_WAVES + wave;
	if (r >= A.n_reads) return;
	const int64_t base = A.f_off[r], cap = A.f_off[r + 1] - base, n64 = A.n_in[r];
	if (base < 0 || cap < 0 || cap > INT_MAX || base + cap > A.n_u_cap || n64 < 0 || n64 > cap) {
		if (lane == 0) atomicAdd(&A.flags[0], 1);                                // offsets that leave the capacities or each other: nothing of this read is touched
		return;
	}
	const int n = (int)n64;
	if (n == 0) { if (lane == 0) A.n_out[r] = 0; return; }
	FinTab T;
	int32_t *rows[FIN_TAB_ROWS];
	if (n <= FIN_LDS_MAX) {
		for (int k = 0; k < FIN_TAB_ROWS; ++k) rows[k] = s_tab[wave][k];
		T.pq = s_pq[wave]; T.cov = s_cov[wave];
	} else {                                                                     // rows of n_u_cap + n_reads + 1 entries: a read's rows hold one entry more than it has regions
		const int64_t row = A.n_u_cap + A.n_reads + 1;
		for (int k = 0; k < FIN_TAB_ROWS; ++k) rows[k] = A.tab + base + r + k * row;
		T.pq = A.pq + base; T.cov = A.cov + base;
	}
	T.ord = rows[0]; T.tmp = rows[1]; T.qs = rows[2]; T.qe = rows[3]; T.score = rows[4]; T.cnt = rows[5]; T.subsc = rows[6]; T.nsub = rows[7]; T.parent = rows[8];
	T.rid = rows[9]; T.rs = rows[10]; T.re = rows[11]; T.w = rows[12]; T.dpmax = rows[13]; T.dpmax2 = rows[14]; T.pidx = rows[15]; T.idv = rows[16];
	fin_read(A, T, A.in + base * REG_WORDS, A.out + base * REG_WORDS, base, s_tab[wave][FIN_SORT_ROW], r, n, lane);
}

// ---- fin_apply ----------------------------------------------------------------------------------------------------------------------------
// the last index k of off[0 .. n] with off[k] <= g (0 when none)
__device__ __forceinline__ int64_t fin_last_le(const int64_t *off, int64_t n, int64_t g)
{
	int64_t lo = 0, hi = n;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo + 1) / 2;
		if (off[mid] <= g) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// the entry of the extra plan's list that names region g, -1 when none does (the list ascends)
__device__ __forceinline__ int64_t fin_find_extra(const FinApplyArgs &A, int64_t g)
{
	int64_t lo = 0, hi = A.n_extra - 1;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (A.extra_reg[mid] < g) lo = mid + 1; else hi = mid;
	}
	return A.n_extra > 0 && A.extra_reg[lo] == g ? lo : -1;
}

// hit.c:115: one float division, one int -> float product in float, a double add, a truncation
__device__ __forceinline__ int32_t fin_split_score(int32_t score, int32_t cnt2, int32_t cnt)
{
	const float part = (float)score * ((float)cnt2 / (float)cnt);
	return (int32_t)((double)part + .499);
}

// what fin_apply and fin_children agree on for region g: its read, whether it is split, the child's extent.  -> the region's status
struct FinSplit { int64_t rd, bbase; int32_t n, cnt2, as2, qlen; bool split; };
__device__ __forceinline__ int fin_region(const FinApplyArgs &A, int64_t g, const Reg &R, const FinCigReg &C, FinSplit &S)
{
	S.split = false;
	if (C.status != 0) return C.status == 1 ? FIN_APPLY_REFUSED : FIN_APPLY_INCOMPLETE;
	S.rd = fin_last_le(A.u_off, A.n_reads, g);
	if (S.rd >= A.n_reads || A.u_off[S.rd] > g || A.u_off[S.rd + 1] <= g) return FIN_APPLY_REFUSED;
	S.bbase = A.b_off[S.rd];
	const int64_t nb = A.b_off[S.rd + 1] - S.bbase, ql = A.read_off[S.rd + 1] - A.read_off[S.rd];
	if (S.bbase < 0 || nb < 0 || S.bbase + nb > A.n_b_cap || ql < 0 || ql > INT_MAX) return FIN_APPLY_REFUSED;
	S.qlen = (int32_t)ql;
	S.n = C.split_n;
	if (S.n > 0 && S.n < R.cnt) {                                                // hit.c:108
		S.split = true;
		S.cnt2 = R.cnt - S.n;
		const int64_t as2 = (int64_t)R.as + S.n;
		if (as2 < 0 || as2 + S.cnt2 > nb) return FIN_APPLY_REFUSED;              // the child's anchors leave the read's
		S.as2 = (int32_t)as2;
	}
	return 0;
}

__global__ __launch_bounds__(256) void fin_apply(FinApplyArgs A)
{
	const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (g >= A.n_regs) return;
	const Reg R = ((const Reg *)A.regs)[g];
	const FinCigReg C = A.cig_regs[g];
	FinSplit S;
	int st = fin_region(A, g, R, C, S);
	int64_t k = -1;
	FinExtraRes E = {};
	if (st == 0 && C.has_p) {
		k = fin_find_extra(A, g);
		if (k < 0) st = FIN_APPLY_REFUSED;
		else { E = A.extra_res[k]; if (E.status != 0) st = E.status == 1 ? FIN_APPLY_REFUSED : FIN_APPLY_INCOMPLETE; }
	}
	A.status[g] = st;
	A.slot[g] = st == 0 && S.split ? 1 : 0;
	if (st != 0) { atomicAdd(&A.flags[st == FIN_APPLY_REFUSED ? 0 : 1], 1); return; }   // only the status word
	Reg O = R;
	const bool rev = (R.flags >> REG_REV_BIT & 1u) != 0;
	if (S.split) {                                                               // hit.c:119-122 on the parent
		const int32_t sc2 = fin_split_score(R.score, S.cnt2, R.cnt);
		O.cnt = R.cnt - S.cnt2;
		O.score = (int32_t)((uint32_t)R.score - (uint32_t)sc2);
		O.flags |= 1u << 8;
	}
	O.rs = C.rs1; O.re = C.re1; O.qs = C.r_qs; O.qe = C.r_qe;                    // align.c:781-783
	Pext P = {};
	if (C.has_p) {                                                               // mm_update_extra (align.c:240-286)
		O.rs = (int32_t)((uint32_t)O.rs + (uint32_t)E.tshift);
		if (rev) O.qe = (int32_t)((uint32_t)O.qe - (uint32_t)E.qshift); else O.qs = (int32_t)((uint32_t)O.qs + (uint32_t)E.qshift);
		O.blen = E.blen; O.mlen = E.mlen;
		O.p = (uint64_t)g + 1;
		P.dp_score = C.dp_score; P.dp_max = E.dp_max; P.dp_max2 = 0; P.ambi_strand = (uint32_t)E.n_ambi & 0x3fffffffu; P.n_cigar = E.n_cigar; P.cig0 = A.out_off[k];
	} else O.p = 0;
	((Reg *)A.regs_out)[g] = O;
	A.pext[g] = P;
}

// slot[0 .. n_regs): 0 / 1 -> the exclusive sums; slot[n_regs] and *n_child: the total.  One workgroup: every lane sums a run of consecutive entries, one block scan
__global__ __launch_bounds__(1024) void fin_slots(FinApplyArgs A)
{
	__shared__ int64_t sh[1][1024];
	const int tid = (int)threadIdx.x;
	const int64_t per = (A.n_regs + 1023) / 1024, lo = per * tid, hi = lo + per < A.n_regs ? lo + per : A.n_regs;
	int64_t v[1] = {0}, incl[1], total[1];
	for (int64_t g = lo; g < hi; ++g) v[0] += A.slot[g];
	block_incl_sum_1024<1>(sh, tid, v, incl, total);
	int64_t at = incl[0] - v[0];
	for (int64_t g = lo; g < hi; ++g) { const int32_t f = A.slot[g]; A.slot[g] = (int32_t)at; at += f; }
	if (tid == 0) {
		A.slot[A.n_regs] = (int32_t)total[0];
		*A.n_child = total[0];
		if (total[0] > A.n_child_cap) A.flags[2] = (int32_t)(total[0] - A.n_child_cap);
	}
}

// the child r2 of every split region (hit.c:110-118, 122; align.c:759)
__global__ __launch_bounds__(256) void fin_children(FinApplyArgs A)
{
	const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (g >= A.n_regs || A.status[g] != 0) return;
	const int32_t slot = A.slot[g];
	if (A.slot[g + 1] == slot) return;
	if (slot >= A.n_child_cap) { A.status[g] = FIN_APPLY_OVER_CAP; return; }    // nothing behind the capacity
	const Reg R = ((const Reg *)A.regs)[g];
	const FinCigReg C = A.cig_regs[g];
	FinSplit S;
	(void)fin_region(A, g, R, C, S);
	Reg O = R;
	O.id = -1; O.p = 0;
	O.cnt = S.cnt2;
	O.score = fin_split_score(R.score, S.cnt2, R.cnt);
	O.as = S.as2;
	if (R.parent == R.id) O.parent = -2;                                         // MM_PARENT_TMP_PRI
	const ulonglong2 *a = A.b + S.bbase + S.as2;                                 // mm_reg_set_coor (hit.c:23-38) over the child's anchors
	const ulonglong2 a0 = a[0], a1 = a[S.cnt2 - 1];
	const int32_t q_span = (int32_t)(a0.y >> 32 & 0xff);
	const uint32_t rv = (uint32_t)(a0.x >> 63);
	const uint32_t x0 = (uint32_t)a0.x + 1u, x1 = (uint32_t)a1.x + 1u, y0 = (uint32_t)a0.y + 1u - (uint32_t)q_span, y1 = (uint32_t)a1.y + 1u;
	O.rid = (int32_t)(a0.x << 1 >> 33);
	O.rs = (int32_t)x0 > q_span ? (int32_t)(x0 - (uint32_t)q_span) : 0; O.re = (int32_t)x1;
	O.qs = (int32_t)(rv ? (uint32_t)S.qlen - y1 : y0); O.qe = (int32_t)(rv ? (uint32_t)S.qlen - y0 : y1);
	uint32_t ml = (uint32_t)q_span, bl = (uint32_t)q_span;                       // mm_cal_fuzzy_len (hit.c:8-21), in wrapping int
	uint32_t px = (uint32_t)a0.x, py = (uint32_t)a0.y;
	for (int32_t i = 1; i < S.cnt2; ++i) {
		const ulonglong2 e = a[i];
		const int32_t span = (int32_t)(e.y >> 32 & 0xff), tl = (int32_t)((uint32_t)e.x - px), ql = (int32_t)((uint32_t)e.y - py);
		bl += (uint32_t)(tl > ql ? tl : ql);
		ml += (uint32_t)(tl > span && ql > span ? span : tl < ql ? tl : ql);
		px = (uint32_t)e.x; py = (uint32_t)e.y;
	}
	O.mlen = (int32_t)ml; O.blen = (int32_t)bl;
	O.flags = (R.flags & ~(REG_SAM_PRI | 1u << REG_SPLIT_INV_BIT | 1u << REG_REV_BIT)) | rv << REG_REV_BIT | (C.split_inv ? 1u << REG_SPLIT_INV_BIT : 0u) | 2u << 8;
	((Reg *)A.child)[slot] = O;
	A.child_of[slot] = (int32_t)g;
}

} // namespace

hipError_t launch_fin_apply(const FinApplyArgs &A, hipStream_t st)
{
	hipError_t e;
	const unsigned blocks = (unsigned)((A.n_regs + 255) / 256);
	if (A.n_regs > 0) {
		hipLaunchKernelGGL(fin_apply, dim3(blocks), dim3(256), 0, st, A);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	hipLaunchKernelGGL(fin_slots, dim3(1), dim3(1024), 0, st, A);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (A.n_regs > 0) hipLaunchKernelGGL(fin_children, dim3(blocks), dim3(256), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_fin_select(const FinArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(fin_select, dim3((unsigned)((A.n_reads + FIN_WAVES - 1) / FIN_WAVES)), dim3(64 * FIN_WAVES), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
