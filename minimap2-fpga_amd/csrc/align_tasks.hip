// align_tasks.hip -- regions to alignment tasks (mm_align1, align.c:565-733, 767-771, up to its mm_align_pair calls).
//   aln_plan   one wave per region, persistent grid: validates, mm_fix_bad_ends, rs0 .. qe0, the two seed filters (anchor flags in/out), counts the region's items
//   aln_scan   one workgroup: items, tasks, CIGAR words and pool bytes of every region -> offsets; marks what leaves a capacity
//   aln_emit   one wave per region: walks the gap loop again and writes items, ksw tasks and cig_off at the scanned offsets
//   aln_gather streaming over bases, a region dealt in pieces of 16-base units: the spans from the reads and the packed reference, the reversed left copies
// Placement comes from the scan; every store is a plain vector store; the only atomics are the adds of the refusal counters.
#include "align_tasks.h"
#include "wave_ops.h"

namespace mm2c {
namespace {

constexpr uint64_t SEED_LONG_JOIN = 1ull << 40, SEED_IGNORE = 1ull << 41, SEED_TANDEM = 1ull << 42, SEED_SELF = 1ull << 43;
constexpr int KSW_EZ_RIGHT = 0x02, KSW_EZ_APPROX_MAX = 0x08, KSW_EZ_EXTZ_ONLY = 0x40, KSW_EZ_REV_CIGAR = 0x80;

// a flag word another lane of the wave may just have written (see `Ordering` in aln_plan)
__device__ inline uint64_t ld_y(const ulonglong2 *p) { return __hip_atomic_load(&p->y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int32_t span_of(uint64_t y) { return (int32_t)(y >> 32 & 0xff); }
__device__ inline int64_t r16(int64_t n) { return (n + 15) & ~(int64_t)15; }   // every pool segment starts at a multiple of 16
// y_i - y_{i-1} - (x_i - x_{i-1}) as the reference's int: modulo 2^32 whichever of its three spellings (:372, :402, :430)
__device__ inline int32_t gap_at(const ulonglong2 *a, int32_t i)
{
	const ulonglong2 c = a[i], p = a[i - 1];
	return (int32_t)(((uint32_t)c.y - (uint32_t)p.y) - ((uint32_t)c.x - (uint32_t)p.x));
}

struct RegCtx { int64_t read, na; ulonglong2 *a; int32_t qlen; const uint8_t *fwd; };

// the read of region g and its arrays; false when an offset leaves a capacity
__device__ bool locate(const AlnArgs &A, int64_t g, RegCtx &C)
{
	RegionRead Q;
	if (!read_of_region(A, g, Q) || Q.r0 + Q.qlen > A.reads_cap) return false;
	C.read = Q.read; C.na = Q.na; C.a = A.b + Q.b0; C.qlen = Q.qlen; C.fwd = A.reads + Q.r0;
	return true;
}

__device__ inline uint32_t qbase(const RegCtx &C, bool rev, int32_t i)                  // the read on the anchors' strand (:876)
{
	const uint32_t c = rev ? C.fwd[C.qlen - 1 - i] : C.fwd[i];
	return rev ? (c < 4 ? 3 - c : 4) : c;
}
__device__ inline uint32_t sget(const uint32_t *S, int64_t i) { return S[i >> 3] >> ((i & 7) << 2) & 0xf; }   // mm_seq4_get

// mm_adjust_minier (:350-365).  The HPC form walks the query homopolymer down to i > 0, not >= 0, as written, and the target one (mm_get_hplen_back) down to the
// contig's first base; both are a few bases long, so the lane that owns the anchor walks them
__device__ inline void adjust_minier(const AlnArgs &A, const RegCtx &C, bool rev, int64_t t0, const ulonglong2 v, int32_t *r, int32_t *q)
{
	if (A.opt.idx_flag & ALN_I_HPC) {
		int32_t i = lo32(v.y) - 1;
		const uint32_t c = qbase(C, rev, lo32(v.y));
		for (; i > 0; --i) if (qbase(C, rev, i) != c) break;
		*q = i + 1;
		const int64_t off = t0 + lo32(v.x);
		const uint32_t ct = sget(A.S, off);
		int64_t j = off - 1;
		for (; j >= t0; --j) if (sget(A.S, j) != ct) break;
		*r = lo32(v.x) + 1 - (int32_t)(off - j);
	} else {
		*r = lo32(v.x) - (A.opt.k >> 1); *q = lo32(v.y) - (A.opt.k >> 1);
	}
}

// collect_long_gaps (:367-384) 64 anchors a step: a ballot compaction.  K == nullptr only counts.
__device__ int32_t long_gaps(const ulonglong2 *a, int32_t cnt1, int32_t min_gap, int32_t *K, int lane)
{
	int32_t n = 0;
	for (int32_t i0 = 1; i0 < cnt1; i0 += 64) {
		const int32_t i = i0 + lane;
		bool is = false;
		if (i < cnt1) { const int32_t gap = gap_at(a, i); is = gap < -min_gap || gap > min_gap; }
		const uint64_t m = __ballot(is);
		if (K && is) K[n + __popcll(m & ((1ull << lane) - 1))] = i;
		n += __popcll(m);
	}
	return n;
}

__device__ inline void or_range(ulonglong2 *a, int32_t from, int32_t to, uint64_t bit, int lane)
{
	for (int32_t j = from + lane; j < to; j += 64) a[j].y = ld_y(a + j) | bit;
	__threadfence();
}

// mm_filter_bad_seeds (:386-421) over the long gaps only, as written: every lane walks the same states, the flag ranges are written by the wave
__device__ void filter_bad_seeds(ulonglong2 *a, const int32_t *K, int32_t n, int32_t diff_thres, int32_t max_ext_len, int32_t max_ext_cnt, int lane)
{
	int32_t max = 0, max_st = -1, max_en = -1;
	for (int32_t k = 0;; ++k) {
		int32_t n_ins = 0, n_del = 0, max_diff = 0, max_diff_l = -1;
		if (k == n || k >= max_en) {
			if (max_en > 0) or_range(a, K[max_st], K[max_en], SEED_IGNORE, lane);
			max = 0; max_st = max_en = -1;
			if (k == n) break;
		}
		const int32_t i = K[k];
		int32_t gap = gap_at(a, i);
		if (gap > 0) n_ins += gap; else n_del += -gap;
		const int32_t qs = lo32(a[i - 1].y), rs = lo32(a[i - 1].x);
		for (int32_t l = k + 1; l < n && l <= k + max_ext_cnt; ++l) {
			const int32_t j = K[l];
			if (lo32(a[j].y) - qs > max_ext_len || lo32(a[j].x) - rs > max_ext_len) break;
			gap = gap_at(a, j);
			if (gap > 0) n_ins += gap; else n_del += -gap;
			const int32_t d = n_ins - n_del, diff = n_ins + n_del - (d < 0 ? -d : d);
			if (max_diff < diff) { max_diff = diff; max_diff_l = l; }
		}
		if (max_diff > diff_thres && max_diff > max) { max = max_diff; max_st = k; max_en = max_diff_l; }
	}
}

// mm_filter_bad_seeds_alt (:423-457)
__device__ void filter_bad_seeds_alt(ulonglong2 *a, const int32_t *K, int32_t n, int32_t max_ext, int lane)
{
	for (int32_t k = 0; k < n;) {
		const int32_t i = K[k];
		int32_t l, gap1 = gap_at(a, i), re1 = lo32(a[i].x), qe1 = lo32(a[i].y);
		gap1 = gap1 > 0 ? gap1 : -gap1;
		for (l = k + 1; l < n; ++l) {
			const int32_t j = K[l];
			if (lo32(a[j].y) - qe1 > max_ext || lo32(a[j].x) - re1 > max_ext) break;
			int32_t gap2 = gap_at(a, j);
			const int32_t q_span_pre = span_of(a[j - 1].y), rs2 = lo32(a[j - 1].x) + q_span_pre, qs2 = lo32(a[j - 1].y) + q_span_pre;
			const int32_t m = rs2 - re1 < qs2 - qe1 ? rs2 - re1 : qs2 - qe1;
			gap2 = gap2 > 0 ? gap2 : -gap2;
			if (m > gap1 + gap2) break;
			re1 = lo32(a[j].x); qe1 = lo32(a[j].y); gap1 = gap2;
		}
		if (l > k + 1) {
			const int32_t end = K[l - 1];
			or_range(a, K[k], end, SEED_IGNORE, lane);
			if (lane == 0) a[end].y = ld_y(a + end) | SEED_LONG_JOIN;
		}
		k = l;
	}
}

// the `nearby seeds` loops (:628-639, :655-665), 64 anchors a step from `first` in direction `dir` while x >> 32 stays `key`: the (min_cnt + 1)-th anchor
// beyond (x0, y0) on both axes, if there is one
__device__ bool nearby(const ulonglong2 *a, int64_t first, int64_t end, int dir, uint64_t key, int32_t x0, int32_t y0, int32_t min_cnt, int lane, int32_t *ox, int32_t *oy)
{
	int32_t l = 0;
	for (int64_t i0 = first;; i0 += 64 * dir) {
		const int64_t j = i0 + (int64_t)lane * dir;
		const bool valid = dir < 0 ? j >= 0 : j < end;
		bool same = false, qual = false;
		int32_t x = 0, y = 0;
		if (valid) {
			const ulonglong2 v = a[j];
			same = v.x >> 32 == key;
			if (dir < 0) { x = lo32(v.x) + 1 - span_of(v.y); y = lo32(v.y) + 1 - span_of(v.y); qual = same && x < x0 && y < y0; }
			else { x = lo32(v.x) + 1; y = lo32(v.y) + 1; qual = same && x > x0 && y > y0; }
		}
		const uint64_t stop = __ballot(!same);
		uint64_t qm = __ballot(qual);
		if (stop) qm &= (1ull << (__ffsll((unsigned long long)stop) - 1)) - 1;
		const int32_t c = __popcll(qm);
		if (c > 0 && l + c > min_cnt) {
			int32_t need = min_cnt + 1 - l;
			for (; need > 1; --need) qm &= qm - 1;
			const int f = __ffsll((unsigned long long)qm) - 1;
			*ox = __shfl(x, f); *oy = __shfl(y, f);
			return true;
		}
		l += c;
		if (stop) return false;
	}
}

// mm_max_stretch (:495-521), 64 anchors a step: a segmented sum (score) and count (len) whose segments begin where lq != lr, carried from step to step; a segment
// ends where the next one begins; of the ends' scores the first strict maximum wins (`score > max_score`): inside a step the smaller index breaks a tie, across
// steps only a larger score replaces the best
__device__ void max_stretch(const ulonglong2 *a, int32_t as, int32_t cnt, int lane, int32_t *as1, int32_t *cnt1)
{
	*as1 = as; *cnt1 = cnt;
	if (cnt < 2) return;
	int32_t best = -1, best_i = -1, best_len = 0, carry_s = 0, carry_n = 0;
	for (int32_t i0 = 0; i0 < cnt; i0 += 64) {
		const int32_t i = i0 + lane;
		const bool in = i < cnt;
		int32_t v = 0, n = 0;
		bool head = false, ends = false;
		if (in) {
			const ulonglong2 c = a[as + i];
			const int32_t q_span = span_of(c.y);
			if (i == 0) { head = true; v = q_span; }
			else {
				const ulonglong2 p = a[as + i - 1];
				const int32_t lr = lo32(c.x) - lo32(p.x), lq = lo32(c.y) - lo32(p.y);
				head = lq != lr;
				v = head ? q_span : imin(lq, q_span);
			}
			n = 1;
			ends = i == cnt - 1;
			if (!ends) { const ulonglong2 nx = a[as + i + 1]; ends = lo32(nx.y) - lo32(c.y) != lo32(nx.x) - lo32(c.x); }
		}
		int f = head;
		for (int d = 1; d < 64; d <<= 1) {
			const int32_t uv = __shfl_up(v, d), un = __shfl_up(n, d);
			const int uf = __shfl_up(f, d);
			if (lane >= d && !f) { v += uv; n += un; f = uf; }
		}
		if (!f) { v += carry_s; n += carry_n; }                                            // no segment begins at or before this lane in the step: the carried one goes on
		int64_t key = ends ? ((int64_t)v << 32 | (uint32_t)(0x7fffffff - i)) : -1;
		for (int d = 32; d >= 1; d >>= 1) { const int64_t o = __shfl_xor(key, d); key = o > key ? o : key; }
		if (key >= 0) {
			const int32_t sc = (int32_t)(key >> 32), idx = 0x7fffffff - (int32_t)(uint32_t)key, len = __shfl(n, idx - i0);
			if (sc > best) { best = sc; best_len = len; best_i = as + idx + 1 - len; }
		}
		carry_s = __shfl(v, 63); carry_n = __shfl(n, 63);
	}
	*as1 = best_i; *cnt1 = best_len;
}

struct Cursor { int64_t it, tk, cig; };

template <bool EMIT>
__device__ inline void put_item(const AlnArgs &A, Cursor &c, int64_t g, int32_t kind, int32_t anchor, int32_t rs, int32_t re, int32_t qs, int32_t qe, int64_t q_off, int64_t t_off,
                                int32_t w, int32_t zdrop, int32_t end_bonus, int32_t flag, int lane)
{
	const int32_t ql = qe - qs, tl = re - rs;
	const bool over = A.opt.max_sw_mat > 0 && (int64_t)tl * ql > A.opt.max_sw_mat;      // :323
	if (EMIT && lane == 0) A.items[c.it] = AlnItem{(int32_t)g, kind | (over ? ALN_OVER : 0), anchor, rs, re, qs, qe, over ? -1 : (int32_t)c.tk, 0, 0};
	++c.it;
	if (over) return;
	if (EMIT && lane == 0) { A.tasks[c.tk] = KswTask{q_off, t_off, ql, tl, w, zdrop, end_bonus, flag}; A.cig_off[c.tk] = c.cig; }
	++c.tk;
	const int64_t s = (int64_t)ql + tl;
	c.cig += s < (s >> A.cig_shift) + 16 ? s : (s >> A.cig_shift) + 16;
}

// the calls mm_align1 makes when no task drops (:690-697, :709-733, :767-771), in call order.  The next anchor the gap loop emits at is the first of the
// following ones that is not skipped and is the last, a LONG_JOIN or min_ksw_len on from the last emit on both axes: a ballot over 64 anchors a step, so the
// loop is walked over emits only.
template <bool EMIT>
__device__ void walk(const AlnArgs &A, const RegCtx &C, int64_t t0, const ulonglong2 *a, const AlnReg &R, bool split_inv, int64_t g, Cursor &c, int lane)
{
	const AlnOpt &o = A.opt;
	int32_t rs = R.rs, qs = R.qs;
	if (qs > 0 && rs > 0)
		put_item<EMIT>(A, c, g, ALN_LEFT, R.as1, R.rs0, rs, R.qs0, qs, R.left_off, R.left_off + r16(qs - R.qs0), o.bw_ext, split_inv ? o.zdrop_inv : o.zdrop, o.end_bonus,
		               KSW_EZ_EXTZ_ONLY | KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR, lane);
	if (o.flag & ALN_F_SR) {                                                               // :724-731: the stretch filled without gaps, no ksw task; its score by the wave
		int32_t sc = 0;
		if (EMIT) {
			for (int32_t j = lane; j < R.qe - qs; j += 64) {
				const uint32_t qb = qbase(C, R.rev != 0, qs + j), tb = sget(A.S, t0 + rs + j);
				sc += qb >= 4 || tb >= 4 ? o.e2 : qb == tb ? o.a : -o.b;
			}
			sc = wave_sum(sc);
			if (lane == 0) A.items[c.it] = AlnItem{(int32_t)g, ALN_UNGAPPED, R.as1 + R.cnt1 - 1, rs, R.re, qs, R.qe, -1, sc, 0};
		}
		++c.it;
	}
	for (int32_t i = o.flag & ALN_F_SR ? R.cnt1 : 1; i < R.cnt1;) {
		const int32_t j = i + lane;
		bool cand = false, lj = false;
		int32_t re_j = 0, qe_j = 0;
		if (j < R.cnt1) {
			const ulonglong2 *p = a + R.as1 + j;
			const uint64_t y = ld_y(p);
			adjust_minier(A, C, R.rev != 0, t0, ulonglong2{p->x, y}, &re_j, &qe_j);
			lj = (y & SEED_LONG_JOIN) != 0;
			const bool skip = (y & (SEED_IGNORE | SEED_TANDEM)) && j != R.cnt1 - 1;
			cand = !skip && (j == R.cnt1 - 1 || lj || (qe_j - qs >= o.min_ksw_len && re_j - rs >= o.min_ksw_len));
		}
		const uint64_t m = __ballot(cand);
		if (!m) { i += 64; continue; }
		const int f = __ffsll((unsigned long long)m) - 1;
		const int32_t re = __shfl(re_j, f), qe = __shfl(qe_j, f);
		const bool is_lj = __shfl((int)lj, f) != 0;
		const int32_t bw1 = is_lj ? imax(qe - qs, re - rs) : o.bw_ext;
		put_item<EMIT>(A, c, g, ALN_GAP, R.as1 + i + f, rs, re, qs, qe, R.q_off + (qs - R.qs0), R.t_off + (rs - R.rs0), bw1, o.zdrop, -1, KSW_EZ_APPROX_MAX, lane);
		rs = re; qs = qe;
		i += f + 1;
	}
	if (R.qe < R.qe0 && R.re < R.re0)
		put_item<EMIT>(A, c, g, ALN_RIGHT, R.as1 + R.cnt1 - 1, R.re, R.re0, R.qe, R.qe0, R.q_off + (R.qe - R.qs0), R.t_off + (R.re - R.rs0), o.bw_ext, o.zdrop, o.end_bonus,
		               KSW_EZ_EXTZ_ONLY, lane);
}

__global__ __launch_bounds__(64) void aln_plan(const AlnArgs A)
{
	__shared__ int32_t ldsK[ALN_LDS_GAPS];
	const int lane = threadIdx.x;
	const AlnOpt &o = A.opt;
	for (int64_t g = blockIdx.x; g < A.n_regs; g += gridDim.x) {
		AlnReg R = {};
		int32_t status = ALN_REFUSED;
		RegCtx C;
		do {
			const bool is_sr = (o.flag & ALN_F_SR) != 0;
			if ((o.flag & ALN_F_SPLICE) || (is_sr && (o.idx_flag & ALN_I_HPC))) break;             // :575
			if (!locate(A, g, C)) break;
			const Reg r = A.regs[g];
			if (r.cnt == 0) { status = 0; break; }                                         // :578
			if (r.cnt < 0 || r.as < 0 || (int64_t)r.as + r.cnt > C.na) break;
			ulonglong2 *a = C.a;
			const ulonglong2 a0 = a[r.as], aN = a[r.as + r.cnt - 1];
			const uint64_t key = a0.x >> 32;
			const int64_t rid = (int64_t)(a0.x << 1 >> 33);
			if (rid >= A.n_seq) break;
			const int32_t tlen = (int32_t)A.ref_len[rid];
			if (tlen < 0) break;
			// every anchor on one x >> 32, inside its contig and its read, not running backwards on either axis
			bool bad = false;
			for (int32_t i0 = 0; i0 < r.cnt; i0 += 64) {
				const int32_t i = i0 + lane;
				if (i < r.cnt) {
					const ulonglong2 v = a[r.as + i];
					bad |= v.x >> 32 != key || lo32(v.x) < 0 || lo32(v.x) >= tlen || lo32(v.y) < 0 || lo32(v.y) >= C.qlen;
					if (i > 0) { const ulonglong2 p = a[r.as + i - 1]; bad |= lo32(v.x) < lo32(p.x) || lo32(v.y) < lo32(p.y); }
				}
			}
			if (__ballot(bad)) break;
			// mm_fix_bad_ends (:459-493): two short walks, ended by l >= 2 bw at the latest; every lane walks them
			int32_t as1 = r.as, cnt1 = r.cnt;
			if (is_sr) max_stretch(a, r.as, r.cnt, lane, &as1, &cnt1);
			else if (!(o.flag & ALN_F_NO_END_FLT) && r.cnt >= 3) {
				const int32_t min_match = o.min_chain_score * 2;
				int32_t l, m, i;
				m = l = span_of(a0.y);
				for (i = r.as + 1; i < r.as + r.cnt - 1; ++i) {
					const ulonglong2 v = a[i], p = a[i - 1];
					if (v.y & SEED_LONG_JOIN) break;
					const int32_t q_span = span_of(v.y), lr = lo32(v.x) - lo32(p.x), lq = lo32(v.y) - lo32(p.y), mn = imin(lr, lq), mx = imax(lr, lq);
					if (mx - mn > l >> 1) as1 = i;
					l += mn; m += imin(mn, q_span);
					if (l >= o.bw << 1 || (m >= min_match && m >= o.bw) || m >= r.mlen >> 1) break;
				}
				cnt1 = r.as + r.cnt - as1;
				m = l = span_of(aN.y);
				for (i = r.as + r.cnt - 2; i > as1; --i) {
					const ulonglong2 v = a[i + 1], p = a[i];
					if (v.y & SEED_LONG_JOIN) break;
					const int32_t q_span = span_of(v.y), lr = lo32(v.x) - lo32(p.x), lq = lo32(v.y) - lo32(p.y), mn = imin(lr, lq), mx = imax(lr, lq);
					if (mx - mn > l >> 1) cnt1 = i + 1 - as1;
					l += mn; m += imin(mn, q_span);
					if (l >= o.bw << 1 || (m >= min_match && m >= o.bw) || m >= r.mlen >> 1) break;
				}
			}
			if (cnt1 <= 0) break;                                                          // :600
			const int64_t t0 = (int64_t)A.ref_off[rid];
			const bool rev = a0.x >> 63 != 0;
			int32_t rs, qs, re, qe;
			adjust_minier(A, C, rev, t0, a[as1], &rs, &qs);
			adjust_minier(A, C, rev, t0, a[as1 + cnt1 - 1], &re, &qe);
			if (is_sr) {                                                                   // :584-587
				const ulonglong2 f = a[as1], e = a[as1 + cnt1 - 1];
				rs = lo32(f.x) + 1 - span_of(f.y); qs = lo32(f.y) + 1 - span_of(f.y); re = lo32(e.x) + 1; qe = lo32(e.y) + 1;
			}
			int32_t rs0, qs0, re0, qe0;
			if (is_sr) {                                                                   // the sr form (:613-620)
				int32_t l = qs;
				l += l * o.a + o.end_bonus > o.q ? (l * o.a + o.end_bonus - o.q) / o.e : 0;
				qs0 = 0; qe0 = C.qlen;
				rs0 = rs - l > 0 ? rs - l : 0;
				l = C.qlen - qe;
				l += l * o.a + o.end_bonus > o.q ? (l * o.a + o.end_bonus - o.q) / o.e : 0;
				re0 = re + l < tlen ? re + l : tlen;
			} else {
				// rs0 .. qe0, the general form (:621-676)
				int32_t rs1 = 0, qs1 = 0, re1, qe1, l, x, y;
				rs0 = lo32(a0.x) + 1 - span_of(a0.y); qs0 = lo32(a0.y) + 1 - span_of(a0.y);
				if (rs0 < 0) rs0 = 0;
				if (qs0 < 0) break;                                                            // :626
				if (nearby(a, (int64_t)r.as - 1, C.na, -1, key, rs0, qs0, o.min_cnt, lane, &x, &y)) {
					l = imax(rs0 - x, qs0 - y);
					rs1 = rs0 - l; qs1 = qs0 - l;
					if (rs1 < 0) rs1 = 0;
				}
				if (qs > 0 && rs > 0) {
					l = imin(qs, o.max_gap);
					qs1 = imax(qs1, qs - l);
					qs0 = imin(qs0, qs1);
					l += l * o.a > o.q ? (l * o.a - o.q) / o.e : 0;
					l = imin(l, o.max_gap);
					l = imin(l, rs);
					rs1 = imax(rs1, rs - l);
					rs0 = imin(rs0, rs1);
					rs0 = imin(rs0, rs);
				} else { rs0 = rs; qs0 = qs; }
				re0 = lo32(aN.x) + 1; qe0 = lo32(aN.y) + 1;
				re1 = tlen; qe1 = C.qlen;
				if (nearby(a, (int64_t)r.as + r.cnt, C.na, 1, key, re0, qe0, o.min_cnt, lane, &x, &y)) {
					l = imax(x - re0, y - qe0);
					re1 = re0 + l; qe1 = qe0 + l;
				}
				if (qe < C.qlen && re < tlen) {
					l = imin(C.qlen - qe, o.max_gap);
					qe1 = imin(qe1, qe + l);
					qe0 = imax(qe0, qe1);
					l += l * o.a > o.q ? (l * o.a - o.q) / o.e : 0;
					l = imin(l, o.max_gap);
					l = imin(l, tlen - re);
					re1 = imin(re1, re + l);
					re0 = imax(re0, re1);
				} else { re0 = re; qe0 = qe; }
			}
			if (a0.y & SEED_SELF) {                                                        // :677-684
				int32_t max_ext = r.qs > r.rs ? r.qs - r.rs : r.rs - r.qs;
				if (r.rs - rs0 > max_ext) rs0 = r.rs - max_ext;
				if (r.qs - qs0 > max_ext) qs0 = r.qs - max_ext;
				max_ext = r.qe > r.re ? r.qe - r.re : r.re - r.qe;
				if (re0 - r.re > max_ext) re0 = r.re + max_ext;
				if (qe0 - r.qe > max_ext) qe0 = r.qe + max_ext;
			}
			// what :686, :707 assert and what keeps every length the reference passes on non-negative and inside the read and the contig
			if (!(re0 > rs0) || qs0 < 0 || rs0 < 0 || qs0 > qs || rs0 > rs || qe > qe0 || re > re0 || qe0 > C.qlen || re0 > tlen) break;
			if (is_sr && qe - qs != re - rs) break;                                         // :725
			// the long-gap list: LDS, or the block's scratch slot; the sr form runs no filter
			const int32_t n10 = is_sr ? 0 : long_gaps(a + as1, cnt1, 10, nullptr, lane);
			int32_t *K = ldsK;
			if (n10 > ALN_LDS_GAPS) {
				if ((int64_t)n10 > A.slot_words) { status = ALN_TOO_BIG; break; }
				K = A.scratch + (int64_t)blockIdx.x * A.slot_words;
			}
			// Ordering, stated once: K and the flag words are written by some lanes and read by others of the same wave.  A fence and a barrier behind each fill of K make
			// it visible (it may lie in global scratch); or_range ends in a fence, so a flag range is visible before the next one is merged into it; one fence behind
			// the filters covers the LONG_JOIN words lane 0 wrote last.  Flag words are re-read with ld_y so that no stale line of this CU's L1 is taken for them; the
			// positions and spans, which never change, are read with plain loads.
			if (n10 > 1) {                                                                 // :595
				long_gaps(a + as1, cnt1, 10, K, lane);
				__threadfence(); __syncthreads();
				filter_bad_seeds(a + as1, K, n10, 40, o.max_gap >> 1, 10, lane);
				const int32_t n30 = long_gaps(a + as1, cnt1, 30, nullptr, lane);
				__syncthreads();                                                           // every lane is done with the first list
				if (n30 > 1) {                                                             // :596
					long_gaps(a + as1, cnt1, 30, K, lane);
					__threadfence(); __syncthreads();
					filter_bad_seeds_alt(a + as1, K, n30, o.max_gap >> 1, lane);
				}
				__threadfence();
			}
			R.as1 = as1; R.cnt1 = cnt1; R.rs = rs; R.qs = qs; R.re = re; R.qe = qe; R.rs0 = rs0; R.qs0 = qs0; R.re0 = re0; R.qe0 = qe0;
			R.rev = (int32_t)(a0.x >> 63);
			Cursor c = {0, 0, 0};
			walk<false>(A, C, t0, a, R, (r.flags >> REG_SPLIT_INV_BIT & 1) != 0, g, c, lane);
			R.n_items = (int32_t)c.it; R.n_tasks = (int32_t)c.tk;
			// until aln_scan: the counts where the offsets go
			R.item0 = c.it; R.task0 = c.tk; R.cig0 = c.cig;
			R.q_off = r16(qe0 - qs0) + r16(re0 - rs0) + (qs > 0 && rs > 0 ? r16(qs - qs0) + r16(rs - rs0) : 0);
			status = 0;
		} while (0);
		if (status != 0) R = AlnReg{};
		R.status = status;
		if (lane == 0) {
			A.aregs[g] = R;
			if (status == ALN_REFUSED) atomicAdd(A.flags + 0, 1);
			else if (status == ALN_TOO_BIG) atomicAdd(A.flags + 1, 1);
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(1024) void aln_scan(const AlnArgs A)
{
	__shared__ int64_t sh[4][1024];
	const int tid = threadIdx.x;
	int64_t carry[4] = {0, 0, 0, 0};
	for (int64_t base = 0; base < A.n_regs; base += 1024) {
		const int64_t g = base + tid;
		int64_t v[4] = {0, 0, 0, 0};
		AlnReg R = {};
		if (g < A.n_regs) { R = A.aregs[g]; v[0] = R.item0; v[1] = R.task0; v[2] = R.cig0; v[3] = R.q_off; }
		for (int c = 0; c < 4; ++c) sh[c][tid] = v[c];
		__syncthreads();
		for (int d = 1; d < 1024; d <<= 1) {
			int64_t t[4];
			for (int c = 0; c < 4; ++c) t[c] = tid >= d ? sh[c][tid - d] : 0;
			__syncthreads();
			for (int c = 0; c < 4; ++c) sh[c][tid] += t[c];
			__syncthreads();
		}
		if (g < A.n_regs && R.status == 0) {
			R.item0 = carry[0] + sh[0][tid] - v[0]; R.task0 = carry[1] + sh[1][tid] - v[1]; R.cig0 = carry[2] + sh[2][tid] - v[2];
			R.q_off = carry[3] + sh[3][tid] - v[3];
			R.t_off = R.q_off + r16(R.qe0 - R.qs0);
			R.left_off = R.t_off + r16(R.re0 - R.rs0);
			if (R.item0 + v[0] > A.items_cap || R.task0 + v[1] > A.tasks_cap || R.q_off + v[3] > A.pool_cap) { R.status = ALN_OVER_CAP; atomicAdd(A.flags + 2, 1); }
			A.aregs[g] = R;
		}
		for (int c = 0; c < 4; ++c) carry[c] += sh[c][1023];
		__syncthreads();
	}
	if (tid == 0) {
		for (int c = 0; c < 4; ++c) A.totals[c] = carry[c];
		if (carry[1] <= A.tasks_cap) A.cig_off[carry[1]] = carry[2];
	}
}

__global__ __launch_bounds__(64) void aln_emit(const AlnArgs A)
{
	const int lane = threadIdx.x;
	for (int64_t g = blockIdx.x; g < A.n_regs; g += gridDim.x) {
		const AlnReg R = A.aregs[g];
		RegCtx C;
		if (R.status != 0 || R.n_items == 0 || !locate(A, g, C)) continue;
		Cursor c = {R.item0, R.task0, R.cig0};
		walk<true>(A, C, (int64_t)A.ref_off[(int64_t)(C.a[R.as1].x << 1 >> 33)], C.a, R, (A.regs[g].flags >> REG_SPLIT_INV_BIT & 1) != 0, g, c, lane);
	}
}

__device__ inline uint32_t comp4(uint32_t v)                                             // c < 4 ? 3 - c : 4 (:876) on four codes at once
{
	const uint32_t M = ((v & 0x04040404u) >> 2) * 0xffu;
	return ((v ^ 0x03030303u) & ~M) | (v & M);
}
__device__ inline uint32_t spread4(uint32_t n)                                           // four nibbles -> four bytes
{
	uint32_t x = n & 0xffffu;
	x = (x | x << 8) & 0x00ff00ffu;
	return (x | x << 4) & 0x0f0f0f0fu;
}
__device__ inline void rev16(uint32_t o[4])
{
	const uint32_t a = __builtin_bswap32(o[3]), b = __builtin_bswap32(o[2]), c = __builtin_bswap32(o[1]), d = __builtin_bswap32(o[0]);
	o[0] = a; o[1] = b; o[2] = c; o[3] = d;
}
// 16 bytes from any byte address: two aligned 16-byte loads and a funnel shift.  The caller has made sure that both lie inside the array.
__device__ inline void load16(const uint8_t *p, uint32_t o[4])
{
	const uintptr_t a = (uintptr_t)p;
	const uint4 *q = (const uint4 *)(a & ~(uintptr_t)15);
	const uint4 A = q[0], B = q[1];
	const int bs = (int)(a & 3) << 3;
	uint32_t d0, d1, d2, d3, d4;
	switch ((a >> 2) & 3) {
	case 0: d0 = A.x; d1 = A.y; d2 = A.z; d3 = A.w; d4 = B.x; break;
	case 1: d0 = A.y; d1 = A.z; d2 = A.w; d3 = B.x; d4 = B.y; break;
	case 2: d0 = A.z; d1 = A.w; d2 = B.x; d3 = B.y; d4 = B.z; break;
	default: d0 = A.w; d1 = B.x; d2 = B.y; d3 = B.z; d4 = B.w; break;
	}
	if (bs) { o[0] = d0 >> bs | d1 << (32 - bs); o[1] = d1 >> bs | d2 << (32 - bs); o[2] = d2 >> bs | d3 << (32 - bs); o[3] = d3 >> bs | d4 << (32 - bs); }
	else { o[0] = d0; o[1] = d1; o[2] = d2; o[3] = d3; }
}
// 16 bases of the packed reference from absolute position p on (mm_seq4_get, mmpriv.h:30): two words, three when p is not a multiple of 8; words behind S read as 0
__device__ inline void s16(const AlnArgs &A, int64_t p, uint32_t o[4])
{
	const int64_t w = p >> 3;
	const int sh = (int)(p & 7) << 2;
	const uint64_t w0 = w < A.n_words ? A.S[w] : 0, w1 = w + 1 < A.n_words ? A.S[w + 1] : 0;
	uint64_t v = w0 | w1 << 32;
	if (sh) { const uint64_t w2 = w + 2 < A.n_words ? A.S[w + 2] : 0; v = v >> sh | w2 << (64 - sh); }
	o[0] = spread4((uint32_t)v); o[1] = spread4((uint32_t)(v >> 16)); o[2] = spread4((uint32_t)(v >> 32)); o[3] = spread4((uint32_t)(v >> 48));
}
__device__ inline void put_byte(uint32_t o[4], int b, uint32_t c) { o[b >> 2] = (o[b >> 2] & ~(0xffu << ((b & 3) << 3))) | c << ((b & 3) << 3); }

// a region's four pool segments in units of 16 bases, taken by one workgroup in pieces of 256 units (gridDim.y > 1 would deal them over several workgroups; the
// lookup of the region's context then costs more than it gains, profiles/aln_tasks.md).  A unit is one 16-byte store; its bytes behind the segment's
// end are code 4.  A whole unit takes 16-byte loads: of the read two aligned ones and a funnel shift (backwards and complemented where the strand or the left copy
// asks for it), of S two or three words.  A segment's last, partial unit and a unit whose aligned loads would leave the reads go base by base.
__global__ __launch_bounds__(256) void aln_gather(const AlnArgs A)
{
	__shared__ AlnReg sR;
	__shared__ RegCtx sC;
	__shared__ int64_t s_t0;
	__shared__ int s_ok;
	const uintptr_t rd_lo = ((uintptr_t)A.reads + 15) & ~(uintptr_t)15, rd_hi = ((uintptr_t)A.reads + (uintptr_t)A.reads_cap) & ~(uintptr_t)15;   // whole aligned 16-byte blocks of the reads
	for (int64_t g = blockIdx.x; g < A.n_regs; g += gridDim.x) {
		__syncthreads();
		if (threadIdx.x == 0) {                                                            // the region's record, its read and its contig: found once a workgroup
			sR = A.aregs[g];
			s_ok = sR.status == 0 && sR.cnt1 > 0 && locate(A, g, sC);
			if (s_ok) s_t0 = (int64_t)A.ref_off[(int64_t)(sC.a[sR.as1].x << 1 >> 33)];
		}
		__syncthreads();
		if (!s_ok) continue;
		const AlnReg R = sR;
		const RegCtx C = sC;
		const int64_t t0 = s_t0;
		const bool left = R.qs > 0 && R.rs > 0, rev = R.rev != 0;
		const int64_t nq = R.qe0 - R.qs0, nt = R.re0 - R.rs0, nlq = left ? R.qs - R.qs0 : 0, nlt = left ? R.rs - R.rs0 : 0;
		const int64_t uq = r16(nq) >> 4, ut = r16(nt) >> 4, ulq = r16(nlq) >> 4, ult = r16(nlt) >> 4, U = uq + ut + ulq + ult;
		for (int64_t u = (int64_t)blockIdx.y * 256 + threadIdx.x; u < U; u += (int64_t)gridDim.y * 256) {
			uint32_t o[4] = {0x04040404u, 0x04040404u, 0x04040404u, 0x04040404u};
			int64_t dst;
			if (u < uq || (u >= uq + ut && u < uq + ut + ulq)) {                           // query: the forward span, or the left copy backwards from qs - 1
				const bool lc = u >= uq;
				const int64_t j = (lc ? u - uq - ut : u) << 4, n = lc ? nlq : nq;
				dst = (lc ? R.left_off : R.q_off) + j;
				// the unit's bases are strand[i0 + b] (span) or strand[i0 - b] (left copy); on the reverse strand strand[m] = comp(fwd[qlen - 1 - m])
				const int64_t i0 = lc ? (int64_t)R.qs - 1 - j : R.qs0 + j;
				const bool back = lc != rev;                                               // the unit runs backwards over the forward read
				const int64_t f0 = rev ? C.qlen - 1 - i0 : i0, src = back ? f0 - 15 : f0;  // the forward read's bytes [src, src + 16)
				const uintptr_t pa = (uintptr_t)(C.fwd + src) & ~(uintptr_t)15;
				if (j + 16 <= n && src >= 0 && pa >= rd_lo && pa + 32 <= rd_hi) {
					load16(C.fwd + src, o);
					if (back) rev16(o);
					if (rev) { o[0] = comp4(o[0]); o[1] = comp4(o[1]); o[2] = comp4(o[2]); o[3] = comp4(o[3]); }
				} else {
					for (int b = 0; b < 16 && j + b < n; ++b) put_byte(o, b, qbase(C, rev, (int32_t)(lc ? i0 - b : i0 + b)));
				}
			} else if (u < uq + ut) {                                                      // the target span
				const int64_t j = (u - uq) << 4;
				dst = R.t_off + j;
				s16(A, t0 + R.rs0 + j, o);
				for (int b = (int)(nt - j < 16 ? nt - j : 16); b < 16; ++b) put_byte(o, b, 4);
			} else {                                                                       // the target, the left copy backwards from rs - 1
				const int64_t j = (u - uq - ut - ulq) << 4;
				dst = R.left_off + r16(nlq) + j;
				if (j + 16 <= nlt) { s16(A, t0 + R.rs - 16 - j, o); rev16(o); }
				else for (int b = 0; j + b < nlt; ++b) put_byte(o, b, sget(A.S, t0 + R.rs - 1 - (j + b)));
			}
			*(uint4 *)(A.pool + dst) = make_uint4(o[0], o[1], o[2], o[3]);
		}
	}
}

} // namespace

hipError_t launch_aln_plan(const AlnArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	const int64_t grid = A.n_regs < A.n_slots ? A.n_regs : A.n_slots;
	hipLaunchKernelGGL(aln_plan, dim3((unsigned)grid), dim3(64), 0, st, A);
	hipLaunchKernelGGL(aln_scan, dim3(1), dim3(1024), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_aln_emit(const AlnArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	const int64_t grid = A.n_regs < 8192 ? A.n_regs : 8192;
	hipLaunchKernelGGL(aln_emit, dim3((unsigned)grid), dim3(64), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_aln_gather(const AlnArgs &A, hipStream_t st)
{
	if (A.n_regs <= 0) return hipSuccess;
	const int64_t grid = A.n_regs < 16384 ? A.n_regs : 16384;
	hipLaunchKernelGGL(aln_gather, dim3((unsigned)grid, 1), dim3(256), 0, st, A);
	return hipGetLastError();
}

} // namespace mm2c
