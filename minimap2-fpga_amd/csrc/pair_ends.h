// pair_ends.h -- argument block and launcher of the pairing of a fragment's two ends (pair_ends.hip): mm_pair with mm_set_pe_thru (pe.c:45-63, 76-177, called at
// map.c:373-374) and the flip of the mate that was reverse-complemented before mapping (map.c:455-466), on the regions fin_select leaves in device memory.
#ifndef MM2C_PAIR_ENDS_H
#define MM2C_PAIR_ENDS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "align_finish.h"

namespace mm2c {

constexpr int PAIR_LDS_MAX = 128;      // pair_select: fragments of up to this many regions (both mates) keep their rows in LDS, longer ones in the plan's scratch (same code)
constexpr int PAIR_WAVES = 4;          // pair_select: fragments (= waves) per workgroup; the waves of a workgroup never meet
constexpr int PAIR_TAB_ROWS = 11;      // 32-bit rows per region: ord tmp par fl | info rid rs re dpmax hash last
constexpr int PAIR_PROPER_SLOTS = 32;   // the count of proper pairs is kept in this many words (a power of two), one per workgroup modulo: the host adds them up
constexpr int PAIR_SORT_ROW = 4;       // the sort's LDS (576 + 257 + 1 ints) lies over the rows from this one on: they are filled behind the sort

struct PairArgs {
	int64_t n_frags, n_u_cap, n_pext_cap;
	int32_t max_gap_ref, pe_bonus, sub_diff, match_sc, pe_ori, flip, max_log_arg;
	const float *logtab;               // L[i] = logf((float)i), 0 <= i <= max_log_arg, by the host's own logf
	const int64_t *f_off;              // 2 * n_frags + 1: the regions of segment read r = 2f + s are regs[f_off[r] .. f_off[r] + n[r]), in room for f_off[r+1] - f_off[r]
	const int32_t *n, *seg_len;        // 2 * n_frags each
	const int32_t *gap_ref;            // n_frags, or NULL: max_gap_ref for every fragment
	uint64_t *regs;                    // updated in place
	const Pext *pext;
	int32_t *status;                   // n_frags: 0, or 1 for a refused fragment
	// scratch for fragments beyond PAIR_LDS_MAX: PAIR_TAB_ROWS rows of n_u_cap entries
	int32_t *tab;
	// scratch of the sort of more than 64 regions, n_u_cap entries each
	uint64_t *zkey, *key0, *key1;
	int32_t *val0, *val1, *tiecnt, *stack, *moved;
	int32_t *flags;                    // [0] fragments refused; zero on entry
	unsigned long long *counts;        // [0] fragments whose n_sub lay beyond the table, [1 .. PAIR_PROPER_SLOTS] fragments with a proper pair; zero on entry
};
hipError_t launch_pair_select(const PairArgs &A, hipStream_t st);

} // namespace mm2c
#endif
