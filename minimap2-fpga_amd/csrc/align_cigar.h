// align_cigar.h -- argument block and launchers of the step between the ksw results and mm_update_extra: the rest of mm_align1 (align.c:698-705, 736-764,
// 772-783): the list of second passes, the cut behind the first dropped task, mm_append_cigar with its merge, the dp_score sums, rs1 .. qe1 and the split
// decision.  align_cigar.hip.
#ifndef MM2C_ALIGN_CIGAR_H
#define MM2C_ALIGN_CIGAR_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "align_tasks.h"
#include "align_extra.h"

namespace mm2c {

constexpr int CIG_REFUSED = 1, CIG_INCOMPLETE = 2, CIG_OVER_CAP = 3;   // mm2c_cig_reg_t::status
constexpr int CIG_PIECE = 256;             // MM2C_CIG_PIECE: items and words a workgroup of cig_gather takes at a time
constexpr int CIG_NO_ROOM = -2;            // MM2C_CIG_NO_ROOM: second_of of an item whose second pass left a capacity
constexpr int CIG_LOST = -3;               // MM2C_CIG_LOST: second_of of an sr ungapped item whose bases leave the pool

struct CigOpt { int32_t zdrop, zdrop_inv, bw_ext, min_cnt, flag, cig_shift; };                      // mm2c_cig_opt_t
struct CigReg {                            // mm2c_cig_reg_t
	int32_t status, n_used, dropped, drop_item, zdrop_code, split_n, split_inv, has_p, n_cigar, dp_score, rs1, re1, qs1, qe1, r_qs, r_qe;
	int64_t cig0;
};
struct CigSec { int64_t tk0, cg0; };       // per region, the plan's own: second-pass tasks and their CIGAR words, counts until cig_second_scan, offsets behind it

struct CigArgs {
	int64_t n_reads, n_regs, items_cap, tasks_cap, cig_cap, tasks2_cap, cig2_cap, pool_cap, b_cap, words_cap, extra_cap;
	CigOpt opt;
	int32_t mat[25];
	// what the alignment-task plan, the ksw plan and the z-drop entry leave
	const AlnReg *aregs;
	const AlnItem *items;
	const KswTask *tasks;
	const int64_t *cig_off;                // tasks_cap + 1
	const uint8_t *seq;                    // the pool
	const KswRes *res;
	const uint32_t *cigar;
	const ZdropRes *zres;
	// the batch
	const int64_t *u_off;
	const Reg *regs;
	const int64_t *b_off, *n_b;
	const ulonglong2 *b;
	const int64_t *read_off;
	// the second list: out of the second-pass entry, in to the join entry
	KswTask *tasks2;
	int64_t *cig_off2;                     // tasks2_cap + 1
	int32_t *second_of;                    // items_cap
	const KswRes *res2;
	const uint32_t *cigar2;
	// out of the join entry
	CigReg *cregs;
	uint32_t *cig_out;                     // words_cap
	int64_t *in_off;                       // extra_cap + 1
	ExtraTask *extra;                      // extra_cap
	int32_t *extra_reg;                    // extra_cap
	CigSec *sec;                           // n_regs, the plan's
	int32_t *flags;                        // [0]: refused, [1]: incomplete, [2]: regions beyond a capacity
	int64_t *totals;                       // join: CIGAR words, extra tasks; second: tasks, CIGAR words
};
hipError_t launch_cig_second_count(const CigArgs &A, hipStream_t st);   // cig_second_count, then cig_second_scan
hipError_t launch_cig_second_emit(const CigArgs &A, hipStream_t st);
hipError_t launch_cig_cut(const CigArgs &A, hipStream_t st);
hipError_t launch_cig_scan(const CigArgs &A, hipStream_t st);
hipError_t launch_cig_gather(const CigArgs &A, hipStream_t st);

} // namespace mm2c
#endif
