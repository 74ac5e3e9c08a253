// align_finish.h -- argument blocks and launchers of the last hit-level steps of a read mapped with base alignment (align_finish.hip): fin_apply, what
// mm_align1 leaves in a region with mm_split_reg in its middle (align.c:757-760, 781-783, hit.c:108-123), and fin_select, the tail of mm_align_skeleton
// (align.c:917-918), align_regs (map.c:264-268) and the mm_set_mapq of map.c:361.
#ifndef MM2C_ALIGN_FINISH_H
#define MM2C_ALIGN_FINISH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2c {

constexpr int FIN_LDS_MAX = 128;       // fin_select: reads of up to this many regions keep their tables in LDS, longer ones in the plan's scratch (same code)
constexpr int FIN_WAVES = 4;           // fin_select: reads (= waves) per workgroup; the waves of a workgroup never meet
constexpr int FIN_TAB_ROWS = 17;       // 32-bit table rows per region: ord tmp | qs qe score cnt subsc n_sub parent rid rs re w dp_max dp_max2 pidx idv
constexpr int FIN_SORT_ROW = 2;        // the sort's LDS (576 + 257 + 1 ints) lies over the rows from this one on: they are filled behind the sort
static_assert((FIN_TAB_ROWS - FIN_SORT_ROW) * (FIN_LDS_MAX + 1) >= 576 + 257 + 1 && (FIN_SORT_ROW * (FIN_LDS_MAX + 1)) % 2 == 0, "the sort's LDS fits the rows it lies over, 8-byte aligned");

// mm2c_pext_t: the record of r->p
struct Pext { int32_t dp_score, dp_max, dp_max2; uint32_t ambi_strand; int32_t n_cigar, reserved; int64_t cig0; };
static_assert(sizeof(Pext) == 32, "Pext is mm2c_pext_t");

// mm2c_aln... the records fin_apply reads, field for field (mm2chain.h)
struct FinCigReg { int32_t status, n_used, dropped, drop_item, zdrop_code, split_n, split_inv, has_p, n_cigar, dp_score, rs1, re1, qs1, qe1, r_qs, r_qe; int64_t cig0; };
struct FinExtraRes { int32_t n_cigar, qshift, tshift, blen, mlen, n_ambi, dp_max, status; };
static_assert(sizeof(FinCigReg) == 72 && sizeof(FinExtraRes) == 32, "records of mm2chain.h");

struct FinApplyArgs {
	int64_t n_reads, n_regs, n_b_cap, n_extra, n_child_cap;
	const int64_t *u_off, *b_off, *read_off;   // n_reads + 1 each
	const uint64_t *regs;              // the regions that went into the alignment-task plan, REG_WORDS words each
	const ulonglong2 *b;               // their chain anchors
	const FinCigReg *cig_regs;         // n_regs
	const int32_t *extra_reg;          // n_extra: the region of extra entry k (ascending)
	const FinExtraRes *extra_res;      // n_extra
	const int64_t *out_off;            // n_extra + 1: the extra plan's output offsets
	uint64_t *regs_out;                // n_regs regions as mm_align1 returns them
	Pext *pext;                        // n_regs
	int32_t *status;                   // n_regs: 0, or FIN_APPLY_REFUSED / _INCOMPLETE / _OVER_CAP
	uint64_t *child;                   // n_child_cap regions: r2 of every split region, dense, in region order
	int32_t *child_of;                 // n_child_cap
	int64_t *n_child;                  // one entry: the children the batch has (may exceed n_child_cap)
	int32_t *slot;                     // scratch, n_regs + 1: the child slot of every region
	int32_t *flags;                    // [0]: refused regions, [1]: incomplete regions, [2]: children beyond n_child_cap; zero on entry
};
constexpr int FIN_APPLY_REFUSED = 1, FIN_APPLY_INCOMPLETE = 2, FIN_APPLY_OVER_CAP = 3;
hipError_t launch_fin_apply(const FinApplyArgs &A, hipStream_t st);

struct FinArgs {
	int64_t n_reads, n_u_cap, n_pext_cap;
	// mm_filter_regs
	int32_t min_cnt, min_chain_score, min_dp_max; float max_clip_ratio;
	// mm_set_parent, mm_select_sub
	float mask_level; int32_t mask_len, hard_mask_level, sub_diff; float pri_ratio; int32_t min_diff, best_n;
	// mm_set_mapq
	int32_t match_sc, is_sr, all_chains, max_log_arg;
	const float *logtab, *logtab2;     // L[i] = logf((float)i), L2[i] = logf((float)i / match_sc), 0 <= i <= max_log_arg, by the host's own logf
	const int64_t *f_off;              // n_reads + 1: the regions of read r are in[f_off[r] .. f_off[r] + n_in[r]), in room for f_off[r+1] - f_off[r]
	const int32_t *n_in, *qlen, *rep_len;
	const uint64_t *in;
	uint64_t *out;
	int32_t *n_out;
	Pext *pext;                        // dp_max2 of the surviving primaries is updated in place
	// scratch for reads beyond FIN_LDS_MAX: rows of n_u_cap + n_reads + 1 entries, pq / cov n_u_cap entries
	int32_t *tab;
	int2 *pq, *cov;
	// scratch of the sort of more than 64 regions, n_u_cap entries each
	uint64_t *zkey, *key0, *key1;
	int32_t *val0, *val1, *tiecnt, *stack, *moved;
	int32_t *flags;                    // reads refused: [0] offsets, [1] inv / is_alt, [2] a p that names no record, [3] kept regions with and without p; zero on entry
	unsigned long long *counts;        // [0] final hits of all reads, [1] primaries beyond the table; zero on entry
};
hipError_t launch_fin_select(const FinArgs &A, hipStream_t st);

} // namespace mm2c
#endif
