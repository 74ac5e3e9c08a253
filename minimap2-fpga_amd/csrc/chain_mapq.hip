// chain_mapq.hip -- mm_join_long (hit.c:315-371, with mm_squeeze_a hit.c:295-313, mm_filter_regs hit.c:274-293, mm_sync_regs / mm_set_sam_pri hit.c:220-253) and
// mm_set_mapq (hit.c:463-508) on the GPU: the hits of the hit plan (chain_hits.hip) become the reference's final regions, byte for byte except `div`, which is
// mm_est_err's and passes through.  p, inv and is_alt are always 0 here, so hit.c:484-491, 494-496, 504 and mm_set_inv_mapq are not built.
//
// mapq_join, one wave per read.  Per-hit tables in LDS up to MAPQ_LDS_MAX hits and in the plan's scratch beyond, the same code on the two kinds of pointer.
//   squeeze   : only with do_join and n >= 2 (hit.c:320).  Lanes rank the hits by (as, index) -- radix_sort_64 on as << 32 | i -- and a wave scan of cnt in that
//               order gives the new as.  No anchor moves here.
//   candidates: the hits with parent == i or parent < 0, in ascending as (hit.c:324-327), packed by ballots.  For every pair of neighbours that is adjacent in
//               squeezed coordinates one lane loads the two anchors of the junction, 16 bytes each, from d_b at the OLD positions: the last anchor of r0, which no
//               join has touched when the pair is tested (the walk runs from the back), and the first anchor of r1, which no join ever changes.
//   walk      : lane 0, from the back (hit.c:329-357), on the tables: r1 has already grown when it meets its predecessor.  The tests as written, in the
//               reference's types.  A join needs no walk over anchors: cnt and score add; rs stays and re is r1's; by strand qs / qe come from r0 / r1 or
//               r1 / r0; blen = blen0 + blen1 - span + max(tl, ql) and mlen = mlen0 + mlen1 - span + (tl > span && ql > span ? span : min(tl, ql)) over the one
//               junction pair, in wrapping int (tests/mapq_model.py shows these identities against the reference's bytes).
//   hierarchy : lane 0, in index order, one level per region, reading regs[parent].parent as it stands at that moment (hit.c:360-367).
//   filter    : only when something was joined (hit.c:368-369): cnt < min_cnt goes, ids become indices, parents go through the old ids, sam_pri is recomputed.
//   mapq      : lanes; the score sum over parent == id as int64, uniq_ratio, pen_s1, pen_cm, x = subsc / score0 and the left-to-right product in IEEE single
//               precision as written (the file is built with -ffp-contract=off); the two logarithms are LOOKED UP in the table the host filled with its own
//               logf.  A primary whose score or n_sub + 1 lies beyond the table gets 0 and is counted.
//   move      : the 80-byte records go from the input to the output through the source map, lane-parallel as 8-byte words, patched on the way.
//   For mapq_gather the kernel leaves per hit, in ascending as, (src, dst, cnt, join) and per read whether it was squeezed.
// Plain vector stores only; the only atomics are the integer adds of the counters.
//
// mapq_gather, anchor-parallel, launched only when d_b_out is given.  The output has the input's index space (read r from b_off[r] on), so a workgroup takes
// slices of MAPQ_SLICE consecutive positions of that space, finds the slice's first read by one uniform binary search in b_off and lets every lane step on from
// there; inside a squeezed read a lane finds its hit by a binary search over dst in the per-hit scratch -- reads have few hits behind mm_select_sub, so that is
// zero to three probes of one cache line, and none while the lane's next position lies in the hit it found last -- and copies one anchor with a 16-byte load and a 16-byte store, OR-ing MM_SEED_LONG_JOIN into the first anchor of an
// absorbed chain.  The search in b_off needs every read's offsets to be sound; when mapq_join refused a read (flags[0] != 0) the workgroups go read by read
// instead, which is slower and touches nothing of a refused read.
//
// Preconditions (the hit plan guarantees them): id == index in every read, cnt >= 1, the chains of a read do not overlap in a[].  A hit whose [as, as + cnt)
// leaves the read's segment of d_b makes the read a refused one.

#include <hip/hip_runtime.h>
#include <climits>
#include "chain_mapq.h"
#include "chain_regs.h"

namespace mm2c {

namespace {

constexpr uint32_t SAM_PRI = 1u << 12;                                         // minimap.h:96: mapq:8, split:2, rev:1, inv:1, sam_pri:1
constexpr int REV_BIT = 10;

struct MapqTab {
	int32_t *as, *cnt, *score, *rid, *rev, *qs, *qe, *rs, *re, *parent, *mlen, *blen, *subsc, *nsub, *score0;   // of the input
	int32_t *newas, *ord, *cand, *adj, *src, *newidx, *cnt0, *jn, *fin;        // fin: final parent, then the final mapq
	uint64_t *jx0, *jy0, *jx1, *jy1;                                           // per candidate position: last anchor of its predecessor, its own first anchor
};

__device__ __forceinline__ long long wave_sum64(long long v)
{
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}

__device__ __forceinline__ void refuse(const MapqArgs &A, const int r, const int lane)
{
	if (lane == 0) { atomicAdd(&A.flags[0], 1); A.state[r] = MAPQ_READ_BAD; }
}

__device__ __forceinline__ void mapq_read(const MapqArgs &A, const MapqTab T, const uint64_t *in, uint64_t *out, int4 *moves, const uint4 *b, const int64_t bl,
                                          const int r, const int n, const int lane)
{
	for (int i = lane; i < n; i += 64) {
		const uint64_t *g = in + (int64_t)i * REG_WORDS;
		const uint64_t w0 = g[0], w1 = g[1], w2 = g[2], w3 = g[3], w4 = g[4], w5 = g[5], w6 = g[6], w7 = g[7];
		T.cnt[i] = T.cnt0[i] = (int32_t)(w0 >> 32); T.rid[i] = (int32_t)w1; T.score[i] = (int32_t)(w1 >> 32);
		T.qs[i] = (int32_t)w2; T.qe[i] = (int32_t)(w2 >> 32); T.rs[i] = (int32_t)w3; T.re[i] = (int32_t)(w3 >> 32);
		T.parent[i] = (int32_t)w4; T.subsc[i] = (int32_t)(w4 >> 32); T.as[i] = T.newas[i] = (int32_t)w5; T.mlen[i] = (int32_t)(w5 >> 32);
		T.blen[i] = (int32_t)w6; T.nsub[i] = (int32_t)(w6 >> 32); T.score0[i] = (int32_t)w7; T.rev[i] = (int32_t)(w7 >> (32 + REV_BIT)) & 1;
		T.jn[i] = 0;
	}
	__syncthreads();

	const bool squeezed = A.do_join && n >= 2;                                  // hit.c:320
	const uint64_t lt = (1ull << lane) - 1;
	int n_drop = 0;
	long long n_b = bl;
	if (squeezed) {
		// ---- the extents of the chains inside the read's segment of b, before anything is read through them ----
		long long tot = 0;
		bool bad = false;
		for (int i = lane; i < n; i += 64) {
			const int as = T.as[i], c = T.cnt[i];
			bad |= as < 0 || c < 0 || (long long)as + c > bl;
			tot += c;
		}
		tot = wave_sum64(tot);
		if (__ballot(bad) || tot > bl) { refuse(A, r, lane); return; }
		n_b = tot;
		// ---- mm_squeeze_a (hit.c:295-313): the order by (as, index), the new as ----
		for (int i = lane; i < n; i += 64) {
			const int as = T.as[i];
			int rank = 0;
			for (int j = 0; j < n; ++j) { const int aj = T.as[j]; rank += aj < as || (aj == as && j < i); }
			T.ord[rank] = i;
		}
		__syncthreads();
		int carry = 0;
		for (int t0 = 0; t0 < n; t0 += 64) {
			const int t = t0 + lane, h = t < n ? T.ord[t] : 0, c = t < n ? T.cnt[h] : 0;
			int incl = c;
			for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
			if (t < n) T.newas[h] = carry + incl - c;
			carry += __shfl(incl, 63);
		}
		__syncthreads();
		// ---- the candidates in ascending as (hit.c:324-327), and the junction anchors of the adjacent pairs ----
		int nc = 0;
		for (int t0 = 0; t0 < n; t0 += 64) {
			const int t = t0 + lane, h = t < n ? T.ord[t] : 0;
			const bool is = t < n && (T.parent[h] == h || T.parent[h] < 0);
			const uint64_t m = __ballot(is);
			if (is) T.cand[nc + __popcll(m & lt)] = h;
			nc += __popcll(m);
		}
		__syncthreads();
		for (int k = 1 + lane; k < nc; k += 64) {
			const int c0 = T.cand[k - 1], c1 = T.cand[k];
			const bool adj = T.cnt[c0] > 0 && T.cnt[c1] > 0 && T.newas[c0] + T.cnt[c0] == T.newas[c1];   // hit.c:335, in squeezed coordinates
			T.adj[k] = adj;
			if (adj) {
				const uint4 e = b[(int64_t)T.as[c0] + T.cnt[c0] - 1], s = b[T.as[c1]];
				T.jx0[k] = (uint64_t)e.y << 32 | e.x; T.jy0[k] = (uint64_t)e.w << 32 | e.z;
				T.jx1[k] = (uint64_t)s.y << 32 | s.x; T.jy1[k] = (uint64_t)s.w << 32 | s.z;
			}
		}
		__syncthreads();
		// ---- the walk from the back (hit.c:329-357) and the hierarchy fix (hit.c:360-367) ----
		if (lane == 0) {
			for (int i = nc - 1; i >= 1; --i) {
				if (!T.adj[i]) continue;
				const int i0 = T.cand[i - 1], i1 = T.cand[i];
				if (T.rid[i0] != T.rid[i1] || T.rev[i0] != T.rev[i1]) continue;
				const uint64_t x0 = T.jx0[i], y0 = T.jy0[i], x1 = T.jx1[i], y1 = T.jy1[i];
				if (x1 <= x0 || (int32_t)y1 <= (int32_t)y0) continue;
				const int d = (int32_t)((uint32_t)y1 - (uint32_t)y0);
				const int max_gap = x0 + (uint64_t)(int64_t)d > x1 ? d : (int)(x1 - x0);   // hit.c:341-342: uint64_t + int, compared unsigned
				const int min_gap = x0 + (uint64_t)(int64_t)d < x1 ? d : (int)(x1 - x0);
				if (max_gap > A.max_join_long || min_gap > A.max_join_short) continue;
				const float pr = (float)A.min_join_flank_sc / (float)A.max_join_long * (float)max_gap;   // float quotient, float product ...
				const int sc_thres = (int)((double)pr + .499);                                          // ... and a double add
				if (T.score[i0] < sc_thres || T.score[i1] < sc_thres) continue;
				const int min_flank_len = (int)((float)max_gap * A.min_join_flank_ratio);
				if (T.re[i0] - T.rs[i0] < min_flank_len || T.qe[i0] - T.qs[i0] < min_flank_len) continue;
				if (T.re[i1] - T.rs[i1] < min_flank_len || T.qe[i1] - T.qs[i1] < min_flank_len) continue;
				const int span = (int)(y1 >> 32 & 0xff);
				const int tl = (int32_t)((uint32_t)x1 - (uint32_t)x0), ql = d;
				T.jn[i1] = 1;                                                    // hit.c:351: MM_SEED_LONG_JOIN on a[r1->as], for mapq_gather
				T.cnt[i0] = (int32_t)((uint32_t)T.cnt[i0] + (uint32_t)T.cnt[i1]);
				T.score[i0] = (int32_t)((uint32_t)T.score[i0] + (uint32_t)T.score[i1]);
				T.re[i0] = T.re[i1];                                             // mm_reg_set_coor (hit.c:23-38) on the joined chain
				if (T.rev[i0]) T.qs[i0] = T.qs[i1]; else T.qe[i0] = T.qe[i1];
				T.blen[i0] = (int32_t)((uint32_t)T.blen[i0] + (uint32_t)T.blen[i1] - (uint32_t)span + (uint32_t)(tl > ql ? tl : ql));
				T.mlen[i0] = (int32_t)((uint32_t)T.mlen[i0] + (uint32_t)T.mlen[i1] - (uint32_t)span + (uint32_t)(tl > span && ql > span ? span : tl < ql ? tl : ql));
				T.cnt[i1] = 0;
				T.parent[i1] = i0;
				++n_drop;
			}
			if (n_drop > 0)
				for (int i = 0; i < n; ++i) {
					const int p = T.parent[i];
					if (p >= 0 && p < n && i != p) {
						const int pp = T.parent[p];
						if (pp >= 0 && pp != p) T.parent[i] = pp;
					}
				}
			if (n_drop > 0) atomicAdd(&A.counts[0], (unsigned long long)n_drop);
		}
		n_drop = __shfl(n_drop, 0);
		__syncthreads();
	}

	// ---- mm_filter_regs + mm_sync_regs, only behind a join (hit.c:368-369): which hits stay, and their new indices ----
	const bool sync = n_drop > 0;
	int kept = n;
	if (sync) {
		kept = 0;
		for (int i0 = 0; i0 < n; i0 += 64) {
			const int i = i0 + lane;
			const bool keep = i < n && !(T.cnt[i] < A.min_cnt);
			const uint64_t m = __ballot(keep);
			if (i < n) T.newidx[i] = keep ? kept + __popcll(m & lt) : -1;
			if (keep) T.src[kept + __popcll(m & lt)] = i;
			kept += __popcll(m);
		}
	} else
		for (int i = lane; i < n; i += 64) T.src[i] = i;
	__syncthreads();

	// ---- the final parents; mm_set_mapq (hit.c:463-508) ----
	long long sum_sc = 0;
	int first_pri = INT_MAX;
	for (int t = lane; t < kept; t += 64) {
		const int s = T.src[t], p = T.parent[s];
		const int fp = !sync ? p : p == -2 ? t : (p >= 0 && p < n && T.newidx[p] >= 0) ? T.newidx[p] : -1;   // hit.c:245-249
		T.fin[t] = fp;
		if (fp == (sync ? t : s)) { sum_sc += T.score[s]; first_pri = first_pri < t ? first_pri : t; }
	}
	sum_sc = wave_sum64(sum_sc);
	for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(first_pri, o); first_pri = v < first_pri ? v : first_pri; }
	__syncthreads();
	const float uniq_ratio = (float)sum_sc / (float)(sum_sc + A.rep_len[r]);
	for (int t = lane; t < kept; t += 64) {
		const int s = T.src[t];
		int mapq = 0;
		if (T.fin[t] == (sync ? t : s)) {
			const int score = T.score[s], cnt = T.cnt[s], n_sub1 = (int32_t)((uint32_t)T.nsub[s] + 1u);
			if (score < 0 || score > A.max_log_arg || n_sub1 < 0 || n_sub1 > A.max_log_arg) atomicAdd(&A.counts[1], 1ull);   // beyond the table: 0, counted
			else {
				const float pen_s1 = (score > 100 ? 1.0f : 0.01f * (float)score) * uniq_ratio;
				float pen_cm = cnt > 10 ? 1.0f : 0.1f * (float)cnt;
				pen_cm = pen_s1 < pen_cm ? pen_s1 : pen_cm;
				const int subsc = T.subsc[s] > A.min_chain_score ? T.subsc[s] : A.min_chain_score;
				const float x = (float)subsc / (float)T.score0[s];
				mapq = (int)(pen_cm * 40.0f * (1.0f - x) * A.logtab[score]);     // hit.c:498
				mapq -= (int)(4.343f * A.logtab[n_sub1] + .499f);
				mapq = mapq > 0 ? mapq : 0;
				mapq = mapq < 60 ? mapq : 60;
			}
		}
		T.jx0[t] = (uint64_t)(uint32_t)T.fin[t] | (uint64_t)(uint32_t)mapq << 32;  // (the junction rows have served)
	}
	__syncthreads();

	// ---- the records ----
	for (int e = lane; e < kept * REG_WORDS; e += 64) {
		const int t = e / REG_WORDS, wd = e - t * REG_WORDS, s = T.src[t];
		uint64_t v = in[(int64_t)s * REG_WORDS + wd];
		const uint64_t fm = T.jx0[t];
		if (wd == 0) v = (uint64_t)(uint32_t)(sync ? t : s) | (uint64_t)(uint32_t)T.cnt[s] << 32;
		else if (wd == 1) v = (v & 0xffffffffull) | (uint64_t)(uint32_t)T.score[s] << 32;
		else if (wd == 2) v = (uint64_t)(uint32_t)T.qs[s] | (uint64_t)(uint32_t)T.qe[s] << 32;
		else if (wd == 3) v = (v & 0xffffffffull) | (uint64_t)(uint32_t)T.re[s] << 32;
		else if (wd == 4) v = (v & 0xffffffff00000000ull) | (fm & 0xffffffffull);
		else if (wd == 5) v = (uint64_t)(uint32_t)T.newas[s] | (uint64_t)(uint32_t)T.mlen[s] << 32;
		else if (wd == 6) v = (v & 0xffffffff00000000ull) | (uint32_t)T.blen[s];
		else if (wd == 7) {
			uint32_t fl = ((uint32_t)(v >> 32) & ~0xffu) | (uint32_t)(fm >> 32);
			if (sync) fl = (fl & ~SAM_PRI) | (t == first_pri ? SAM_PRI : 0u);    // hit.c:220-229
			v = (v & 0xffffffffull) | (uint64_t)fl << 32;
		}
		out[(int64_t)t * REG_WORDS + wd] = v;
	}
	// ---- for mapq_gather ----
	if (squeezed && A.b_out)
		for (int t = lane; t < n; t += 64) { const int h = T.ord[t]; moves[t] = make_int4(T.as[h], T.newas[h], T.cnt0[h], T.jn[h]); }
	if (lane == 0) {
		A.n_out[r] = kept;
		A.state[r] = squeezed ? MAPQ_READ_SQUEEZED : MAPQ_READ_COPY;
		if (A.n_b_out) A.n_b_out[r] = n_b;
	}
}

__global__ __launch_bounds__(64) void mapq_join(MapqArgs A)
{
	__shared__ int32_t s_tab[MAPQ_TAB_ROWS][MAPQ_LDS_MAX + 1];
	__shared__ uint64_t s_junc[MAPQ_JUNC_ROWS][MAPQ_LDS_MAX];
	const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
	const int64_t base = A.u_off[r], cap = A.u_off[r + 1] - base, bo = A.b_off[r], bl = A.b_off[r + 1] - bo;
	const int64_t n64 = A.n_in[r];
	if (base < 0 || cap < 0 || cap > INT_MAX || base + cap > A.n_u_cap || n64 < 0 || n64 > cap || bo < 0 || bl < 0 || bo + bl > A.n_b_cap) {
		refuse(A, r, lane);                                                      // offsets that leave the capacities or each other: nothing of this read is touched
		return;
	}
	const int n = (int)n64;
	MapqTab T;
	int32_t *rows[MAPQ_TAB_ROWS];
	if (n <= MAPQ_LDS_MAX) {
		for (int k = 0; k < MAPQ_TAB_ROWS; ++k) rows[k] = s_tab[k];
		T.jx0 = s_junc[0]; T.jy0 = s_junc[1]; T.jx1 = s_junc[2]; T.jy1 = s_junc[3];
	} else {                                                                     // rows of n_u_cap + n_reads entries: a read's rows hold one entry more than it has hits
		const int64_t row = A.n_u_cap + A.n_reads;
		for (int k = 0; k < MAPQ_TAB_ROWS; ++k) rows[k] = A.tab + base + r + k * row;
		T.jx0 = A.junc + base; T.jy0 = T.jx0 + A.n_u_cap; T.jx1 = T.jy0 + A.n_u_cap; T.jy1 = T.jx1 + A.n_u_cap;
	}
	T.as = rows[0]; T.cnt = rows[1]; T.score = rows[2]; T.rid = rows[3]; T.rev = rows[4]; T.qs = rows[5]; T.qe = rows[6]; T.rs = rows[7]; T.re = rows[8];
	T.parent = rows[9]; T.mlen = rows[10]; T.blen = rows[11]; T.subsc = rows[12]; T.nsub = rows[13]; T.score0 = rows[14]; T.newas = rows[15]; T.ord = rows[16];
	T.cand = rows[17]; T.adj = rows[18]; T.src = rows[19]; T.newidx = rows[20]; T.cnt0 = rows[21]; T.jn = rows[22]; T.fin = rows[23];
	mapq_read(A, T, A.in + base * REG_WORDS, A.out + base * REG_WORDS, A.moves + base, A.b + bo, bl, r, n, lane);
}

// one anchor of read r: position q of its output, which lies at the same position of its input unless the read was squeezed.  memo: the hit this lane found last;
// a lane's positions are 256 apart and a chain is long, so most of the time it still holds q and no probe is made
struct GatherMemo { int64_t r; int4 m; };

__device__ __forceinline__ void gather_one(const MapqArgs &A, const int64_t r, const int64_t bo, const int64_t q, const int st, GatherMemo &memo)
{
	int64_t src = q;
	bool jn = false;
	if (st == MAPQ_READ_SQUEEZED) {
		if (!(memo.r == r && memo.m.y <= q && q - memo.m.y < memo.m.z)) {
			const int4 *mv = A.moves + A.u_off[r];
			int lo = 0, hi = A.n_in[r] - 1;                                      // the last hit with dst <= q
			while (lo < hi) {
				const int mid = (lo + hi + 1) >> 1;
				if (mv[mid].y <= q) lo = mid; else hi = mid - 1;
			}
			memo.r = r; memo.m = mv[lo];
		}
		src = (int64_t)memo.m.x + (q - memo.m.y);
		jn = memo.m.w != 0 && q == memo.m.y;
	}
	uint4 v = A.b[bo + src];
	if (jn) v.w |= 1u << 8;                                                      // MM_SEED_LONG_JOIN, bit 40 of y (mmpriv.h:17)
	A.b_out[bo + q] = v;
}

__global__ __launch_bounds__(256) void mapq_gather(MapqArgs A)
{
	const int tid = (int)threadIdx.x;
	GatherMemo memo;
	memo.r = -1; memo.m = make_int4(0, 0, 0, 0);
	if (A.flags[0] != 0) {                                                       // some read was refused: b_off is not to be searched; read by read
		for (int64_t r = blockIdx.x; r < A.n_reads; r += gridDim.x) {
			const int st = A.state[r];
			if (st == MAPQ_READ_BAD) continue;
			const int64_t bo = A.b_off[r], nb = A.n_b_out[r];
			for (int64_t q = tid; q < nb; q += 256) gather_one(A, r, bo, q, st, memo);
		}
		return;
	}
	const int64_t end = A.b_off[A.n_reads];
	for (int64_t p0 = (int64_t)blockIdx.x * MAPQ_SLICE; p0 < end; p0 += (int64_t)gridDim.x * MAPQ_SLICE) {
		int64_t lo = 0, hi = A.n_reads - 1;                                      // the last read with b_off <= p0: the same in every lane
		while (lo < hi) {
			const int64_t mid = (lo + hi + 1) >> 1;
			if (A.b_off[mid] <= p0) lo = mid; else hi = mid - 1;
		}
		int64_t r = lo, bo = A.b_off[r], be = A.b_off[r + 1];
		for (int k = 0; k < MAPQ_SLICE / 256; ++k) {
			const int64_t p = p0 + k * 256 + tid;
			if (p >= end) break;
			while (p >= be) { ++r; bo = be; be = A.b_off[r + 1]; }               // p < end = b_off[n_reads]: ends at a read that holds p
			if (p >= bo && p - bo < A.n_b_out[r]) gather_one(A, r, bo, p - bo, A.state[r], memo);   // (p < bo: in front of the batch's first anchor)
		}
	}
}

} // namespace

hipError_t launch_mapq_join(const MapqArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(mapq_join, dim3((unsigned)A.n_reads), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_mapq_gather(const MapqArgs &A, hipStream_t st)
{
	if (A.n_reads <= 0 || A.n_b_cap <= 0 || !A.b_out) return hipSuccess;
	const int64_t slices = (A.n_b_cap + MAPQ_SLICE - 1) / MAPQ_SLICE;
	hipLaunchKernelGGL(mapq_gather, dim3((unsigned)(slices < 2048 ? slices : 2048)), dim3(256), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
