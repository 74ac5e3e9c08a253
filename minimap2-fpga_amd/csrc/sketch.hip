// Sketching reads and looking up their minimizers on the device: mm_sketch (sketch.c:77-143) and collect_matches (map.c:90-123) for a batch of
// single-segment reads, bit for bit, in the reference's order.  DESIGN.md section 3.9 gives the exactness argument; in short:
//
//   1. push register.  The k-mer registers of mm_sketch are a function of the last k nucleotides pushed into them (one per base, or one per homopolymer
//      run under HPC; ambiguous bases push nothing and do NOT clear them) and of how many were pushed, up to k.  Every chunk of CH positions summarises its
//      pushes; a segmented scan over the chunks gives every chunk the registers it starts with.
//   2. slots.  A step that is not skipped as a symmetric k-mer writes one buffer entry ("slot": an ambiguous base, or a base / run end whose k-mer is not
//      symmetric).  Per chunk: slots written and the step counter l (reset by an ambiguous base, saturated at w + k: the loop only compares it with k,
//      w + k - 1 and w + k).  A second segmented scan gives each chunk its first slot index and its l; the chunk then writes x, y and l of its slots to
//      slot arrays laid out like the bases (a read never has more slots than bases).  The HPC span is the sum of the last min(runs since the last
//      ambiguous base, k) run lengths, read back from the bases and cut at 256.
//   3. selection.  Between steps the state of the loop is buf (the last w slots) and min / min_pos, and min is always the newest slot holding the
//      window's smallest x ('<=' on arrival, '>=' in the rescan).  A lane takes SC slots, rebuilds that state from the w slots before them and runs the
//      literal loop of sketch.c:109-137 over its slots; its pushes are exactly the pushes of those steps.  A count pass, a scan and a write pass
//      place them.
//   4. lookups.  A minimizer index is a sorted key array with the (pool offset, n) of every key (mm_idx_get, index.c:81-98: n = 0 when absent); matches,
//      is_tandem against the unfiltered neighbours, rep_len (map.c:104-110,120, one wave per read folding the repetitive minimizers in order) and mini_pos.
//   5. fragments.  Reads of several segments (collect_minimizers with n_segs > 1, map.c:64-77) are the segments' sketches tagged with seg << 32 | sum << 1 and
//      joined; the lookups then run per fragment.  The max_occ re-chain (map.c:318-340) is decided per fragment from the chains on the device, and the flagged
//      fragments' minimizers are compacted for a second pass.  DESIGN.md section 3.11.
#include "api_internal.h"
#include "wave_ops.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int CH = 64;        // positions per lane in the push / slot passes
constexpr int SC = 256;       // slots per lane in the selection passes
constexpr int TPB = 256;
constexpr uint64_t ALL1 = ~(uint64_t)0;
constexpr uint64_t SEG_MASK = 0xffULL << 48;   // MM_SEED_SEG_MASK (mmpriv.h:22-23)

__device__ __forceinline__ int nt4(uint8_t b)                  // seq_nt4_table (sketch.c:9-26): bytes 0-3 and A C G T U in either case
{
	if (b < 4) return b;
	const uint8_t u = b & 0xdf;
	return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : (u == 'T' || u == 'U') ? 3 : 4;
}

__device__ __forceinline__ uint64_t hash64(uint64_t key, uint64_t mask)
{
	key = (~key + (key << 21)) & mask;
	key = key ^ key >> 24;
	key = ((key + (key << 3)) + (key << 8)) & mask;
	key = key ^ key >> 14;
	key = ((key + (key << 2)) + (key << 4)) & mask;
	key = key ^ key >> 28;
	key = (key + (key << 31)) & mask;
	return key;
}

// the largest r with off[r] <= g (reads without chunks share their offset with the next read: the last of them is the one that owns g)
__device__ __forceinline__ int64_t owner(const int64_t *off, int64_t n, int64_t g)
{
	int64_t lo = 0, hi = n;
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
	return lo;
}

struct PushSum { uint64_t bits; uint32_t cnt, head; };
struct PushOp {
	uint32_t k; uint64_t mask;
	__host__ __device__ PushSum operator()(const PushSum &a, const PushSum &b) const
	{
		if (b.head) return b;
		PushSum r;
		r.head = a.head;
		if (b.cnt >= k) { r.bits = b.bits; r.cnt = b.cnt; }
		else { r.bits = ((a.bits << (2 * b.cnt)) | b.bits) & mask; r.cnt = a.cnt + b.cnt < k ? a.cnt + b.cnt : k; }
		return r;
	}
};

struct LSum { int64_t slots; uint32_t l; uint16_t reset, head; };
struct LOp {
	uint32_t cap;
	__host__ __device__ LSum operator()(const LSum &a, const LSum &b) const
	{
		LSum r;
		r.slots = b.head ? b.slots : a.slots + b.slots;
		r.l = b.reset ? b.l : (a.l + b.l < cap ? a.l + b.l : cap);
		r.reset = a.reset | b.reset; r.head = a.head | b.head;
		return r;
	}
};

struct SkArgs {
	const uint8_t *seq; const int64_t *seq_off, *chunk_off, *sc_off;
	int64_t n_reads, n_chunks, n_sc;
	int k, w, hpc;
	uint64_t mask;
	PushSum *push, *push_s; LSum *lsum, *lsum_s;           // raw per-chunk summaries and their inclusive scans
	uint64_t *sx, *sy; uint16_t *sl; int64_t *n_slots;
	int64_t *cnt; mm2c_anchor_t *out;
};

// is position i of s[0..L) a step of the loop, and its nucleotide (4 = ambiguous)
__device__ __forceinline__ bool step_at(const uint8_t *s, int64_t L, int64_t i, int hpc, int *c_out)
{
	const int c = nt4(s[i]);
	*c_out = c;
	return c >= 4 || !hpc || i + 1 == L || nt4(s[i + 1]) != c;
}

__global__ void __launch_bounds__(TPB) sk_push(SkArgs A)
{
	const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (g >= A.n_chunks) return;
	const int64_t r = owner(A.chunk_off, A.n_reads, g), j = g - A.chunk_off[r];
	const int64_t b0 = A.seq_off[r], L = A.seq_off[r + 1] - b0, p0 = j * CH, p1 = min(p0 + CH, L);
	const uint8_t *s = A.seq + b0;
	PushSum ps = { 0, 0, j == 0 };
	for (int64_t i = p0; i < p1; ++i) {
		int c;
		if (step_at(s, L, i, A.hpc, &c) && c < 4) { ps.bits = (ps.bits << 2 | (uint64_t)c) & A.mask; ps.cnt += ps.cnt < (uint32_t)A.k; }
	}
	A.push[g] = ps;
}

// WRITE = 0: the chunk's slot / l summary.  WRITE = 1: x, y, l of every slot at its index.
template <int WRITE>
__global__ void __launch_bounds__(TPB) sk_slots(SkArgs A)
{
	const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (g >= A.n_chunks) return;
	const int64_t r = owner(A.chunk_off, A.n_reads, g), j = g - A.chunk_off[r];
	const int64_t b0 = A.seq_off[r], L = A.seq_off[r + 1] - b0, p0 = j * CH, p1 = min(p0 + CH, L);
	const uint8_t *s = A.seq + b0;
	const int k = A.k, w = A.w;
	const uint64_t mask = A.mask, shift1 = 2 * (k - 1);
	const uint32_t cap = (uint32_t)(w + k);
	uint64_t km0 = 0, km1 = 0;
	if (j > 0) {                                               // the registers as the chunks before left them
		const PushSum ps = A.push_s[g - 1];
		for (uint32_t t = 0; t < ps.cnt; ++t) {
			const uint64_t c = ps.bits >> (2 * (ps.cnt - 1 - t)) & 3;
			km0 = (km0 << 2 | c) & mask; km1 = (km1 >> 2) | (3ULL ^ c) << shift1;
		}
	}
	int64_t slot = 0;
	uint32_t l = 0;
	uint16_t reset = j == 0;
	if (WRITE && j > 0) { const LSum pre = A.lsum_s[g - 1]; slot = pre.slots; l = pre.l; }
	uint64_t *sx = A.sx + b0, *sy = A.sy + b0;
	uint16_t *sl = A.sl + b0;
	for (int64_t i = p0; i < p1; ++i) {
		int c;
		if (!step_at(s, L, i, A.hpc, &c)) continue;
		uint64_t x = ALL1, y = ALL1;
		if (c < 4) {
			km0 = (km0 << 2 | (uint64_t)c) & mask; km1 = (km1 >> 2) | (3ULL ^ (uint64_t)c) << shift1;
			if (km0 == km1) continue;                          // symmetric k-mer: no slot, l unchanged
			l = l + 1 < cap ? l + 1 : cap;
			if (WRITE && l >= (uint32_t)k) {
				int span = k;
				if (A.hpc) {                                   // the last min(runs since the last ambiguous base, k) runs, cut at 256
					int runs = 1, cc = c;
					span = 0;
					for (int64_t q = i; q >= 0 && span < 256; --q) {
						const int cq = nt4(s[q]);
						if (cq >= 4) break;
						if (cq != cc) { if (++runs > k) break; cc = cq; }
						++span;
					}
				}
				if (span < 256) {
					const int z = km0 < km1 ? 0 : 1;
					x = hash64(z ? km1 : km0, mask) << 8 | (uint64_t)span;
					y = (uint64_t)((uint32_t)i << 1 | (uint32_t)z);
				}
			}
		} else { l = 0; reset = 1; }
		if (WRITE) { sx[slot] = x; sy[slot] = y; sl[slot] = (uint16_t)l; }
		++slot;
	}
	if (WRITE) { if (p1 == L) A.n_slots[r] = slot; }
	else A.lsum[g] = LSum{ slot, l, reset, (uint16_t)(j == 0) };
}

// WRITE = 0: pushes of the lane's slots counted.  WRITE = 1: written at cnt[g] (the exclusive scan of the counts).
template <int WRITE>
__global__ void __launch_bounds__(TPB) sk_select(SkArgs A)
{
	const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (g >= A.n_sc) return;
	const int64_t r = owner(A.sc_off, A.n_reads, g), j = g - A.sc_off[r];
	const int64_t ns = A.n_slots[r], a = j * SC, b = min(a + SC, ns);
	if (a >= b) { if (!WRITE) A.cnt[g] = 0; return; }
	const int64_t b0 = A.seq_off[r];
	const uint64_t *X = A.sx + b0, *Y = A.sy + b0;
	const uint16_t *Lv = A.sl + b0;
	const int w = A.w, k = A.k;
	const uint32_t wk = (uint32_t)(w + k);
	int64_t n = 0;
	mm2c_anchor_t *out = WRITE ? A.out + A.cnt[g] : nullptr;
	auto push = [&](uint64_t x, uint64_t y) { if (WRITE) out[n] = mm2c_anchor_t{ x, y }; ++n; };
	uint64_t mx = ALL1, my = ALL1;
	int mpos = 0;
	if (a > 0)                                                 // newest slot with the smallest x among the w before the lane's first (older ones count as all-ones)
		for (int64_t t = a - w; t < a; ++t) {
			const uint64_t x = t < 0 ? ALL1 : X[t];
			if (mx >= x) { mx = x; my = t < 0 ? ALL1 : Y[t]; mpos = (int)(((t % w) + w) % w); }
		}
	for (int64_t t = a; t < b; ++t) {
		const int bp = (int)(t % w);
		const uint64_t ix = X[t], iy = Y[t];
		const uint32_t l = Lv[t];
		// buf[jj] holds the newest slot t' <= t with t' % w == jj
		auto slot_of = [&](int jj) { return t - (int64_t)((bp - jj + w) % w); };
		auto bx = [&](int jj) { const int64_t q = slot_of(jj); return q < 0 ? ALL1 : X[q]; };
		auto by = [&](int jj) { const int64_t q = slot_of(jj); return q < 0 ? ALL1 : Y[q]; };
		if (l == wk - 1 && mx != ALL1) {
			for (int jj = bp + 1; jj < w; ++jj) if (mx == bx(jj) && by(jj) != my) push(bx(jj), by(jj));
			for (int jj = 0; jj < bp; ++jj) if (mx == bx(jj) && by(jj) != my) push(bx(jj), by(jj));
		}
		if (ix <= mx) {
			if (l >= wk && mx != ALL1) push(mx, my);
			mx = ix; my = iy; mpos = bp;
		} else if (bp == mpos) {
			if (l >= wk - 1 && mx != ALL1) push(mx, my);
			mx = ALL1;
			for (int jj = bp + 1; jj < w; ++jj) if (mx >= bx(jj)) { mx = bx(jj); my = by(jj); mpos = jj; }
			for (int jj = 0; jj <= bp; ++jj) if (mx >= bx(jj)) { mx = bx(jj); my = by(jj); mpos = jj; }
			if (l >= wk - 1 && mx != ALL1) {
				for (int jj = bp + 1; jj < w; ++jj) if (mx == bx(jj) && my != by(jj)) push(bx(jj), by(jj));
				for (int jj = 0; jj <= bp; ++jj) if (mx == bx(jj) && my != by(jj)) push(bx(jj), by(jj));
			}
		}
	}
	if (b == ns && mx != ALL1) push(mx, my);                   // the final push (sketch.c:141-142)
	if (!WRITE) A.cnt[g] = n;
}

// minimizer offset per read: the scanned count at the read's first selection lane
__global__ void sk_read_off(const int64_t *sc_off, const int64_t *cnt_scan, int64_t n_reads, int64_t *mini_off)
{
	const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r <= n_reads) mini_off[r] = cnt_scan[sc_off[r]];
}

struct LkArgs {
	const mm2c_anchor_t *mini; const int64_t *mini_off; int64_t n_reads, n_mini;
	const uint64_t *keys; const int64_t *key_cr; const uint32_t *key_n; int64_t n_keys;
	int mid_occ;
	int32_t *t; int64_t *cr, *keep, *acnt;                     // per minimizer; keep / acnt: n_mini + 1 flags / counts, then their n_mini + 1 exclusive scans
	mm2c_match_t *matches; uint64_t *mini_pos;
	int64_t *match_off, *anchor_off; int32_t *rep_len;
};

__global__ void __launch_bounds__(TPB) lk_lookup(LkArgs A)
{
	const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (m > A.n_mini) return;
	if (m == A.n_mini) { A.keep[m] = 0; A.acnt[m] = 0; return; }
	const uint64_t key = A.mini[m].x >> 8;
	int64_t lo = 0, hi = A.n_keys;                              // lower bound
	while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (A.keys[mid] < key) lo = mid + 1; else hi = mid; }
	const bool hit = lo < A.n_keys && A.keys[lo] == key;
	const int32_t t = hit ? (int32_t)A.key_n[lo] : 0;
	A.t[m] = t; A.cr[m] = hit ? A.key_cr[lo] : 0;
	const bool keep = t < A.mid_occ;
	A.keep[m] = keep; A.acnt[m] = keep ? (int64_t)(uint32_t)t : 0;
}

__global__ void __launch_bounds__(TPB) lk_emit(LkArgs A)
{
	const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (m >= A.n_mini || !(A.t[m] < A.mid_occ)) return;
	const int64_t r = owner(A.mini_off, A.n_reads, m), q = A.keep[A.n_mini + 1 + m];
	const mm2c_anchor_t p = A.mini[m];
	const uint32_t q_pos = (uint32_t)p.y, q_span = (uint32_t)(p.x & 0xff);
	uint32_t tandem = 0;
	if (m > A.mini_off[r] && p.x >> 8 == A.mini[m - 1].x >> 8) tandem = 1;
	if (m < A.mini_off[r + 1] - 1 && p.x >> 8 == A.mini[m + 1].x >> 8) tandem = 1;
	A.matches[q] = mm2c_match_t{ A.cr[m], (uint32_t)A.t[m], q_pos, q_span, (uint32_t)(p.y >> 32) << 1 | tandem };
	A.mini_pos[q] = (uint64_t)q_span << 32 | q_pos >> 1;
}

// one wave per read: offsets, and rep_len folded over the repetitive minimizers in order (map.c:104-110,120)
__global__ void __launch_bounds__(TPB) lk_reads(LkArgs A)
{
	const int64_t r = ((int64_t)blockIdx.x * TPB + threadIdx.x) / 64;
	const int lane = threadIdx.x & 63;
	if (r > A.n_reads) return;
	const int64_t m0 = A.mini_off[r];
	if (lane == 0) { A.match_off[r] = A.keep[A.n_mini + 1 + m0]; A.anchor_off[r] = A.acnt[A.n_mini + 1 + m0]; }
	if (r == A.n_reads) return;
	const int64_t m1 = A.mini_off[r + 1];
	int rep_st = 0, rep_en = 0, acc = 0;
	for (int64_t base = m0; base < m1; base += 64) {
		const int64_t m = base + lane;
		int st = 0, en = 0;
		const bool rep = m < m1 && A.t[m] >= A.mid_occ;
		if (rep) { const mm2c_anchor_t p = A.mini[m]; en = (int)((uint32_t)p.y >> 1) + 1; st = en - (int)(p.x & 0xff); }
		uint64_t bits = __ballot(rep);
		while (bits) {
			const int src = __ffsll((unsigned long long)bits) - 1;
			bits &= bits - 1;
			const int s2 = __shfl(st, src), e2 = __shfl(en, src);
			if (s2 > rep_en) { acc += rep_en - rep_st; rep_st = s2; rep_en = e2; }
			else rep_en = e2;
		}
	}
	if (lane == 0) A.rep_len[r] = acc + (rep_en - rep_st);
}

// ---- fragments of several segments (collect_minimizers with n_segs > 1, map.c:64-77) and the max_occ re-chain (map.c:318-340); DESIGN.md section 3.11

// y += seg << 32 | sum << 1 for every minimizer of a segment (seg_tag[s], made by the host from the segment lengths)
__global__ void __launch_bounds__(TPB) fr_tag(mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_segs, int64_t n_mini, const uint64_t *seg_tag)
{
	const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (m >= n_mini) return;
	mini[m].y += seg_tag[owner(mini_off, n_segs, m)];
}

// a fragment's list is its segments' lists one after another: its offset is that of its first segment
__global__ void fr_mini_off(const int64_t *mini_off, const int64_t *frag_off, int64_t n_frags, int64_t *frag_mini_off)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g <= n_frags) frag_mini_off[g] = mini_off[frag_off[g]];
}

// The chaining distances of every fragment (map.c:305-314, in the reference's int arithmetic): dists[2 g] = max_chain_gap_ref (mm_chain_dp's max_dist_x),
// dists[2 g + 1] = max_chain_gap_qry (max_dist_y), from the fragment's total length and the call's four scalars.
__global__ void fr_gaps(const int32_t *qlen, int64_t n_frags, mm2c_frag_gaps_t G, int32_t *dists)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= n_frags) return;
	const int qlen_sum = qlen[g];
	const int gap_qry = G.is_sr ? (qlen_sum > G.max_gap ? qlen_sum : G.max_gap) : G.max_gap;
	int gap_ref = G.max_gap;
	if (G.max_gap_ref > 0) gap_ref = G.max_gap_ref;
	else if (G.max_frag_len > 0) { gap_ref = G.max_frag_len - qlen_sum; if (gap_ref < G.max_gap) gap_ref = G.max_gap; }
	dists[2 * g] = gap_ref; dists[2 * g + 1] = gap_qry;
}

struct RcArgs {
	const int64_t *u_off, *b_off; const uint64_t *u; const mm2c_anchor_t *b;   // what the epilogue left: chains per fragment, anchors in chain order
	const int32_t *rep_len; const int64_t *mini_off;
	int64_t n_frags; int n_segs;
	uint8_t *flag; int64_t *sel_cnt, *mini_cnt;                // per fragment (n_frags + 1, the last 0): 1 / its minimizers when flagged, then their exclusive scans
};

// one wave per fragment: rechain = rep_len > 0 && (no chain || the best chain misses a segment), map.c:318-331 (the caller has tested max_occ > mid_occ)
__global__ void __launch_bounds__(TPB) rc_decide(RcArgs A)
{
	const int64_t g = ((int64_t)blockIdx.x * TPB + threadIdx.x) / 64;
	const int lane = threadIdx.x & 63;
	if (g > A.n_frags) return;
	if (g == A.n_frags) { if (lane == 0) { A.sel_cnt[g] = 0; A.mini_cnt[g] = 0; } return; }
	bool rechain = false;
	if (A.rep_len[g] > 0) {
		const int64_t u0 = A.u_off[g], n_u = A.u_off[g + 1] - u0;
		if (n_u == 0) rechain = true;
		else {
			// the FIRST chain with the strictly largest score above 0 (`max < (int)(u[i] >> 32)` from max = 0)
			int best = 0; int64_t best_i = -1;
			for (int64_t i = lane; i < n_u; i += 64) { const int sc = (int)(A.u[u0 + i] >> 32); if (sc > best) { best = sc; best_i = i; } }
			for (int d = 32; d > 0; d >>= 1) {
				const int sc = __shfl_xor(best, d); const int64_t oi = __shfl_xor(best_i, d);
				if (sc > best || (sc == best && oi >= 0 && (best_i < 0 || oi < best_i))) { best = sc; best_i = oi; }
			}
			int n_chained_segs = 1;                              // no chain scores above 0: the reference reads u[-1] there; here the chain counts as one segment
			if (best_i >= 0) {
				int64_t off = 0;
				for (int64_t i = lane; i < best_i; i += 64) off += (int64_t)(uint32_t)A.u[u0 + i];
				off = A.b_off[g] + mm2c::wave_sum(off);
				const int64_t cnt = (int64_t)(int32_t)A.u[u0 + best_i];
				int diff = 0;
				for (int64_t i = 1 + lane; i < cnt; i += 64) diff += (A.b[off + i].y & SEG_MASK) != (A.b[off + i - 1].y & SEG_MASK);
				n_chained_segs += mm2c::wave_sum(diff);
			}
			rechain = n_chained_segs < A.n_segs;
		}
	}
	if (lane == 0) { A.flag[g] = rechain; A.sel_cnt[g] = rechain; A.mini_cnt[g] = rechain ? A.mini_off[g + 1] - A.mini_off[g] : 0; }
}

// the flagged fragments, in order: which they are and where their minimizers go
__global__ void rc_select(const uint8_t *flag, const int64_t *sel_scan, const int64_t *mini_scan, int64_t n_frags, int64_t *sel, int64_t *mini_off2)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g > n_frags) return;
	if (g == n_frags) mini_off2[sel_scan[g]] = mini_scan[g];
	else if (flag[g]) { sel[sel_scan[g]] = g; mini_off2[sel_scan[g]] = mini_scan[g]; }
}

__global__ void __launch_bounds__(TPB) rc_gather(const mm2c_anchor_t *mini, const int64_t *mini_off, const int64_t *sel, const int64_t *mini_off2, int64_t n_sel, int64_t n_mini2,
                                                 mm2c_anchor_t *mini2)
{
	const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (m >= n_mini2) return;
	const int64_t j = owner(mini_off2, n_sel, m);
	mini2[m] = mini[mini_off[sel[j]] + (m - mini_off2[j])];
}

inline unsigned blocks(int64_t n, int per = TPB) { return (unsigned)((n + per - 1) / per); }

} // namespace

namespace mm2c_api {

// ---- device-side pieces used by the entries in mm2chain_sketch.cpp

size_t sketch_scan_bytes(int64_t n_chunks, int64_t n_sc)
{
	size_t b1 = 0, b2 = 0, b3 = 0;
	(void)rocprim::inclusive_scan(nullptr, b1, (PushSum *)nullptr, (PushSum *)nullptr, (size_t)std::max<int64_t>(n_chunks, 1), PushOp{ 15, 0 });
	(void)rocprim::inclusive_scan(nullptr, b2, (LSum *)nullptr, (LSum *)nullptr, (size_t)std::max<int64_t>(n_chunks, 1), LOp{ 1 });
	(void)rocprim::exclusive_scan(nullptr, b3, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)std::max<int64_t>(n_sc, 1) + 1, rocprim::plus<int64_t>());
	return std::max(b1, std::max(b2, b3));
}

size_t lookup_scan_bytes(int64_t n_mini)
{
	size_t b = 0;
	(void)rocprim::exclusive_scan(nullptr, b, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n_mini + 1, rocprim::plus<int64_t>());
	return b;
}

// sizes of the per-chunk arrays
size_t sketch_push_bytes() { return sizeof(PushSum); }
size_t sketch_lsum_bytes() { return sizeof(LSum); }

// The sketch of a batch: reads r at seq[seq_off[r] .. seq_off[r+1]), chunk_off / sc_off = prefix sums of ceil(len / 64) and ceil(len / 256) (n_reads + 1,
// device).  Work arrays: push / lsum (2 n_chunks: summaries, then their scans), sx / sy / sl (total bases), n_slots (n_reads), cnt (2 (n_sc + 1): counts,
// then their exclusive scan).  After the call mini_off holds the minimizers' read offsets (mini_off[n_reads] = their number); `out` needs room for that
// many -- the caller reads it back between sketch_count and sketch_write.
int sketch_count(const uint8_t *seq, const int64_t *seq_off, const int64_t *chunk_off, const int64_t *sc_off, int64_t n_reads, int64_t n_chunks, int64_t n_sc,
                 int k, int w, int hpc, void *push, void *lsum, uint64_t *sx, uint64_t *sy, uint16_t *sl, int64_t *n_slots, int64_t *cnt, int64_t *mini_off,
                 void *scan_tmp, size_t scan_bytes, hipStream_t st)
{
	SkArgs A{};
	A.seq = seq; A.seq_off = seq_off; A.chunk_off = chunk_off; A.sc_off = sc_off;
	A.n_reads = n_reads; A.n_chunks = n_chunks; A.n_sc = n_sc;
	A.k = k; A.w = w; A.hpc = hpc; A.mask = (1ULL << 2 * k) - 1;
	A.push = (PushSum *)push; A.push_s = A.push + n_chunks; A.lsum = (LSum *)lsum; A.lsum_s = A.lsum + n_chunks;
	A.sx = sx; A.sy = sy; A.sl = sl; A.n_slots = n_slots; A.cnt = cnt;
	int64_t *cnt_s = cnt + n_sc + 1;
	HIP_TRY(hipMemsetAsync(n_slots, 0, (size_t)std::max<int64_t>(n_reads, 1) * 8, st));
	if (n_chunks > 0) {
		sk_push<<<blocks(n_chunks), TPB, 0, st>>>(A);
		HIP_TRY(hipGetLastError());
		size_t b = scan_bytes;
		HIP_TRY(rocprim::inclusive_scan(scan_tmp, b, A.push, A.push_s, (size_t)n_chunks, PushOp{ (uint32_t)k, A.mask }, st));
		sk_slots<0><<<blocks(n_chunks), TPB, 0, st>>>(A);
		HIP_TRY(hipGetLastError());
		b = scan_bytes;
		HIP_TRY(rocprim::inclusive_scan(scan_tmp, b, A.lsum, A.lsum_s, (size_t)n_chunks, LOp{ (uint32_t)(w + k) }, st));
		sk_slots<1><<<blocks(n_chunks), TPB, 0, st>>>(A);
		HIP_TRY(hipGetLastError());
	}
	if (n_sc > 0) {
		sk_select<0><<<blocks(n_sc), TPB, 0, st>>>(A);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemsetAsync(cnt + n_sc, 0, 8, st));
	size_t b = scan_bytes;
	HIP_TRY(rocprim::exclusive_scan(scan_tmp, b, cnt, cnt_s, (int64_t)0, (size_t)n_sc + 1, rocprim::plus<int64_t>(), st));
	sk_read_off<<<blocks(n_reads + 1), TPB, 0, st>>>(sc_off, cnt_s, n_reads, mini_off);
	HIP_TRY(hipGetLastError());
	return 0;
}

int sketch_write(const uint8_t *seq, const int64_t *seq_off, const int64_t *sc_off, int64_t n_reads, int64_t n_sc, int k, int w,
                 const uint64_t *sx, const uint64_t *sy, const uint16_t *sl, const int64_t *n_slots, const int64_t *cnt, mm2c_anchor_t *out, hipStream_t st)
{
	if (n_sc == 0) return 0;
	SkArgs A{};
	A.seq = seq; A.seq_off = seq_off; A.sc_off = sc_off; A.n_reads = n_reads; A.n_sc = n_sc; A.k = k; A.w = w;
	A.sx = (uint64_t *)sx; A.sy = (uint64_t *)sy; A.sl = (uint16_t *)sl; A.n_slots = (int64_t *)n_slots; A.cnt = (int64_t *)cnt + n_sc + 1; A.out = out;
	sk_select<1><<<blocks(n_sc), TPB, 0, st>>>(A);
	HIP_TRY(hipGetLastError());
	return 0;
}

// collect_matches for every read: work arrays t (n_mini), cr (n_mini + 1), keep / acnt (2 (n_mini + 1)); outputs matches / mini_pos (room for n_mini), match_off /
// anchor_off (n_reads + 1), rep_len (n_reads)
int lookup_run(const mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_reads, int64_t n_mini, const uint64_t *keys, const int64_t *key_cr,
               const uint32_t *key_n, int64_t n_keys, int mid_occ, int32_t *t, int64_t *cr, int64_t *keep, int64_t *acnt, mm2c_match_t *matches,
               uint64_t *mini_pos, int64_t *match_off, int64_t *anchor_off, int32_t *rep_len, void *scan_tmp, size_t scan_bytes, hipStream_t st)
{
	LkArgs A{};
	A.mini = mini; A.mini_off = mini_off; A.n_reads = n_reads; A.n_mini = n_mini;
	A.keys = keys; A.key_cr = key_cr; A.key_n = key_n; A.n_keys = n_keys; A.mid_occ = mid_occ;
	A.t = t; A.cr = cr; A.keep = keep; A.acnt = acnt; A.matches = matches; A.mini_pos = mini_pos;
	A.match_off = match_off; A.anchor_off = anchor_off; A.rep_len = rep_len;
	lk_lookup<<<blocks(n_mini + 1), TPB, 0, st>>>(A);
	HIP_TRY(hipGetLastError());
	size_t b = scan_bytes;
	HIP_TRY(rocprim::exclusive_scan(scan_tmp, b, keep, keep + n_mini + 1, (int64_t)0, (size_t)n_mini + 1, rocprim::plus<int64_t>(), st));
	b = scan_bytes;
	HIP_TRY(rocprim::exclusive_scan(scan_tmp, b, acnt, acnt + n_mini + 1, (int64_t)0, (size_t)n_mini + 1, rocprim::plus<int64_t>(), st));
	if (n_mini > 0) {
		lk_emit<<<blocks(n_mini), TPB, 0, st>>>(A);
		HIP_TRY(hipGetLastError());
	}
	lk_reads<<<blocks((n_reads + 1) * 64), TPB, 0, st>>>(A);
	HIP_TRY(hipGetLastError());
	return 0;
}

// Fragments: tags the minimizers of every segment with seg_tag (n_segs entries, device) and writes the fragments' offsets into the joined list
// (frag_mini_off, n_frags + 1).  mini_off: the segments' offsets as sketch_count left them; frag_off: n_frags + 1 segment numbers (device).
int frag_tag(mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_segs, int64_t n_mini, const uint64_t *seg_tag, const int64_t *frag_off, int64_t n_frags,
             int64_t *frag_mini_off, hipStream_t st)
{
	if (n_mini > 0) {
		fr_tag<<<blocks(n_mini), TPB, 0, st>>>(mini, mini_off, n_segs, n_mini, seg_tag);
		HIP_TRY(hipGetLastError());
	}
	fr_mini_off<<<blocks(n_frags + 1), TPB, 0, st>>>(mini_off, frag_off, n_frags, frag_mini_off);
	HIP_TRY(hipGetLastError());
	return 0;
}

// the fragments' (max_dist_x, max_dist_y) from their total lengths (qlen, n_frags entries, device) -> dists (2 n_frags, device)
int frag_gaps(const int32_t *qlen, int64_t n_frags, const mm2c_frag_gaps_t *gaps, int32_t *dists, hipStream_t st)
{
	if (n_frags <= 0) return 0;
	fr_gaps<<<blocks(n_frags), TPB, 0, st>>>(qlen, n_frags, *gaps, dists);
	HIP_TRY(hipGetLastError());
	return 0;
}

size_t rechain_scan_bytes(int64_t n_frags) { return lookup_scan_bytes(n_frags); }

// The re-chain decision of map.c:318-331 for every fragment of a chunk and the compaction of the flagged ones.  u_off / u / b_off / b: the epilogue's output on the
// device; mini_off: the fragments' offsets into the minimizers.  flag: n_frags bytes; cnt: 4 (n_frags + 1) (flags and minimizer counts, then their scans);
// sel: n_frags; mini_off2: n_frags + 1.  h_n: the number of flagged fragments and of their minimizers, downloaded (the call waits for the stream).
int rechain_decide(const int64_t *u_off, const uint64_t *u, const int64_t *b_off, const mm2c_anchor_t *b, const int32_t *rep_len, const int64_t *mini_off,
                   int64_t n_frags, int n_segs, uint8_t *flag, int64_t *cnt, int64_t *sel, int64_t *mini_off2, void *scan_tmp, size_t scan_bytes, int64_t h_n[2],
                   hipStream_t st)
{
	RcArgs A{};
	const size_t n1 = (size_t)n_frags + 1;
	A.u_off = u_off; A.u = u; A.b_off = b_off; A.b = b; A.rep_len = rep_len; A.mini_off = mini_off; A.n_frags = n_frags; A.n_segs = n_segs;
	A.flag = flag; A.sel_cnt = cnt; A.mini_cnt = cnt + n1;
	int64_t *sel_scan = cnt + 2 * n1, *mini_scan = cnt + 3 * n1;
	rc_decide<<<blocks((n_frags + 1) * 64), TPB, 0, st>>>(A);
	HIP_TRY(hipGetLastError());
	size_t bytes = scan_bytes;
	HIP_TRY(rocprim::exclusive_scan(scan_tmp, bytes, A.sel_cnt, sel_scan, (int64_t)0, n1, rocprim::plus<int64_t>(), st));
	bytes = scan_bytes;
	HIP_TRY(rocprim::exclusive_scan(scan_tmp, bytes, A.mini_cnt, mini_scan, (int64_t)0, n1, rocprim::plus<int64_t>(), st));
	rc_select<<<blocks(n_frags + 1), TPB, 0, st>>>(flag, sel_scan, mini_scan, n_frags, sel, mini_off2);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(&h_n[0], sel_scan + n_frags, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&h_n[1], mini_scan + n_frags, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

// the minimizers of the flagged fragments, one after another (the sketch is not redone: the reference keeps mv)
int rechain_gather(const mm2c_anchor_t *mini, const int64_t *mini_off, const int64_t *sel, const int64_t *mini_off2, int64_t n_sel, int64_t n_mini2, mm2c_anchor_t *mini2,
                   hipStream_t st)
{
	if (n_mini2 == 0) return 0;
	rc_gather<<<blocks(n_mini2), TPB, 0, st>>>(mini, mini_off, sel, mini_off2, n_sel, n_mini2, mini2);
	HIP_TRY(hipGetLastError());
	return 0;
}

} // namespace mm2c_api

// ---- the minimizer index's device image [keys ascending | cr_off | n]: the host's rows sorted on the device (radix sort of (key, row)), then gathered
namespace {
__global__ void mx_iota(uint32_t *idx, int64_t n)
{
	const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (i < n) idx[i] = (uint32_t)i;
}

__global__ void mx_gather(const uint32_t *idx, const int64_t *cr_in, const uint32_t *n_in, const uint64_t *keys_s, int64_t n, int64_t *cr_out, uint32_t *n_out, int *dup)
{
	const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (i >= n) return;
	const uint32_t j = idx[i];
	cr_out[i] = cr_in[j]; n_out[i] = n_in[j];
	if (i > 0 && keys_s[i] == keys_s[i - 1]) *dup = 1;
}
}

namespace mm2c_api {
int minidx_image(const uint64_t *h_keys, const int64_t *h_cr, const uint32_t *h_n, int64_t n, int key_bits, char *d_img, int *h_dup, hipStream_t st)
{
	*h_dup = 0;
	if (n == 0) return 0;
	uint64_t *d_keys_s = (uint64_t *)d_img;
	int64_t *d_cr_s = (int64_t *)(d_img + (size_t)n * 8);
	uint32_t *d_n_s = (uint32_t *)(d_img + (size_t)n * 16);
	size_t sort_bytes = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0, key_bits));
	size_t at = 0;
	auto lay = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 255) & ~(size_t)255; return o; };
	const size_t o_k = lay((size_t)n * 8), o_cr = lay((size_t)n * 8), o_n = lay((size_t)n * 4), o_i = lay((size_t)n * 4), o_is = lay((size_t)n * 4), o_dup = lay(4),
	             o_tmp = lay(sort_bytes);
	char *d = nullptr;
	HIP_TRY(dev_alloc((void **)&d, at));
	auto body = [&]() -> int {
		HIP_TRY(hipMemcpyAsync(d + o_k, h_keys, (size_t)n * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d + o_cr, h_cr, (size_t)n * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d + o_n, h_n, (size_t)n * 4, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(d + o_dup, 0, 4, st));
		mx_iota<<<blocks(n), TPB, 0, st>>>((uint32_t *)(d + o_i), n);
		HIP_TRY(hipGetLastError());
		size_t b = sort_bytes;
		HIP_TRY(rocprim::radix_sort_pairs(d + o_tmp, b, (uint64_t *)(d + o_k), d_keys_s, (uint32_t *)(d + o_i), (uint32_t *)(d + o_is), (size_t)n, 0, key_bits, st));
		mx_gather<<<blocks(n), TPB, 0, st>>>((const uint32_t *)(d + o_is), (const int64_t *)(d + o_cr), (const uint32_t *)(d + o_n), d_keys_s, n, d_cr_s, d_n_s,
		                                     (int *)(d + o_dup));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(h_dup, d + o_dup, 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		return 0;
	};
	const int rc = body();
	dev_free(d);
	return rc;
}
} // namespace mm2c_api
