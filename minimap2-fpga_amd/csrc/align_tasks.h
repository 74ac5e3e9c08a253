// align_tasks.h -- argument block and launcher of the step between final regions and base alignment: mm_align1 (align.c:565-733, 767-771) from its first line to
// each mm_align_pair call, as the list of ksw tasks it issues when no task drops, with the sequence pool they read.  align_tasks.hip.
#ifndef MM2C_ALIGN_TASKS_H
#define MM2C_ALIGN_TASKS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "ksw_extd2.h"
#include "chain_regs.h"

namespace mm2c {

constexpr int ALN_LDS_GAPS = 2048;         // MM2C_ALN_LDS_GAPS: the long-gap list K of a region lies in LDS up to this many entries, in the block's scratch slot beyond
constexpr int ALN_MAX_SLOTS = 4096;        // MM2C_ALN_MAX_SLOTS
constexpr int ALN_REFUSED = 1, ALN_TOO_BIG = 2, ALN_OVER_CAP = 3;   // mm2c_aln_reg_t::status
constexpr int ALN_LEFT = 0, ALN_GAP = 1, ALN_RIGHT = 2, ALN_UNGAPPED = 3, ALN_OVER = 16;   // mm2c_aln_item_t::kind; ALN_OVER is or-ed in: beyond max_sw_mat, no ksw task
constexpr int ALN_F_SR = 1, ALN_F_NO_END_FLT = 2, ALN_F_SPLICE = 4, ALN_I_HPC = 1;

struct AlnOpt {                            // mm2c_aln_opt_t
	int32_t a, b, q, e, e2, bw, bw_ext, min_chain_score, max_gap, min_cnt, min_ksw_len, end_bonus, zdrop, zdrop_inv;
	int64_t max_sw_mat;
	int32_t flag, idx_flag, k, reserved;
};
struct AlnReg {                            // mm2c_aln_reg_t
	int32_t as1, cnt1, rs, qs, re, qe, rs0, qs0, re0, qe0, n_items, n_tasks, status, rev;
	int64_t item0, task0, cig0, q_off, t_off, left_off;
};
struct AlnItem { int32_t reg, kind, anchor, rs, re, qs, qe, task, score, reserved; };   // mm2c_aln_item_t
using AlnRegIn = Reg;                      // mm2c_reg_t (chain_regs.h); the name the host files cast to

struct AlnArgs {
	int64_t n_reads, n_regs, items_cap, tasks_cap, pool_cap, b_cap, reads_cap;
	AlnOpt opt;
	int32_t cig_shift;
	const int64_t *u_off;                  // n_reads + 1; region g belongs to the read r with u_off[r] - u_off[0] <= g < u_off[r + 1] - u_off[0]
	const Reg *regs;
	const int64_t *b_off, *n_b;            // the read's anchors start at b[b_off[r]]; n_b (may be NULL): how many it has, else b_off[r + 1] - b_off[r]
	ulonglong2 *b;                         // in/out: MM_SEED_IGNORE / MM_SEED_LONG_JOIN
	const int64_t *read_off;               // n_reads + 1
	const uint8_t *reads;                  // forward codes 0..4
	int64_t n_seq, n_words;
	const uint64_t *ref_off;
	const uint32_t *ref_len, *S;
	AlnReg *aregs;
	AlnItem *items;
	KswTask *tasks;
	int64_t *cig_off;                      // tasks_cap + 1
	uint8_t *pool;
	int32_t *scratch;                      // n_slots slots of slot_words words
	int64_t slot_words;
	int32_t n_slots;
	int32_t *flags;                        // [0]: refused, [1]: too big, [2]: regions beyond a capacity
	int64_t *totals;                       // items, tasks, CIGAR words, pool bytes
};
// The read of region g in a batch (AlnArgs, or CigArgs of align_cigar.h): region g belongs to the read with u_off[read] - u_off[0] <= g < u_off[read + 1] -
// u_off[0]; its anchors are b[b0 .. b0 + na), its bases lie at [r0, r0 + qlen).  false when g belongs to no read or an offset leaves b_cap or int32.
struct RegionRead { int64_t read, b0, na, r0; int32_t qlen; };
template <typename Args>
__device__ inline bool read_of_region(const Args &A, int64_t g, RegionRead &Q)
{
	const int64_t base = A.u_off[0];
	int64_t lo = 0, hi = A.n_reads;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		if (A.u_off[mid + 1] - base <= g) lo = mid + 1; else hi = mid;
	}
	if (lo >= A.n_reads || A.u_off[lo] - base > g) return false;
	const int64_t b0 = A.b_off[lo], na = A.n_b ? A.n_b[lo] : A.b_off[lo + 1] - b0, r0 = A.read_off[lo], r1 = A.read_off[lo + 1];
	if (b0 < 0 || na < 0 || na > INT32_MAX || b0 > A.b_cap - na || r0 < 0 || r1 < r0 || r1 - r0 > INT32_MAX) return false;
	Q.read = lo; Q.b0 = b0; Q.na = na; Q.r0 = r0; Q.qlen = (int32_t)(r1 - r0);
	return true;
}

hipError_t launch_aln_plan(const AlnArgs &A, hipStream_t st);     // aln_plan, then aln_scan
hipError_t launch_aln_emit(const AlnArgs &A, hipStream_t st);     // aln_emit
hipError_t launch_aln_gather(const AlnArgs &A, hipStream_t st);   // aln_gather

} // namespace mm2c
#endif
