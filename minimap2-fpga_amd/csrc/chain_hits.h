// chain_hits.h -- argument block and launcher of the regions-to-hits step (mm_set_parent hit.c:125-186, mm_select_sub hit.c:255-272), chain_hits.hip.
#ifndef MM2C_CHAIN_HITS_H
#define MM2C_CHAIN_HITS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2c {

constexpr int HITS_LDS_MAX = 128;      // hits_select: reads of up to this many regions keep their tables in LDS, longer ones in the plan's scratch (same code)
constexpr int HITS_TAB_ROWS = 11;      // 32-bit table rows per region: qs qe score cnt subsc n_sub parent rid rs re w; hits_select_multi has one more: rev

struct HitArgs {
	int64_t n_reads, n_u_cap;
	float mask_level; int32_t mask_len, hard_mask_level;   // mm_set_parent
	float pri_ratio; int32_t min_diff, best_n;             // mm_select_sub
	float pri1, pri2; int32_t n_segs, max_gap_ref;         // mm_select_sub_multi (pe.c:6), hits_select_multi only
	const int32_t *seg_len;            // n_reads * n_segs: qlens of fragment r from r * n_segs on (read only when n_segs == 2)
	const int32_t *gap_ref;            // n_reads: max_gap_ref per fragment, or NULL: max_gap_ref for all
	const int64_t *u_off;              // n_reads + 1: the regions of read r are in[u_off[r] .. u_off[r+1])
	const uint64_t *in;                // REG_WORDS words per region
	uint64_t *out;                     // out: the hits of read r from u_off[r] on, n_out[r] of them
	int32_t *n_out;                    // n_reads
	// scratch for reads beyond HITS_LDS_MAX, n_u_cap entries each, indexed like the regions
	int32_t *tab;                      // HITS_TAB_ROWS + 1 rows
	int2 *pq, *cov;                    // (qs, qe) of the primaries in w order / the clipped intervals of one region
	int32_t *flags;                    // [0]: reads whose offsets leave the capacities; zero on entry
	unsigned long long *total;         // hits of all reads; zero on entry
};
hipError_t launch_chain_hits(const HitArgs &A, hipStream_t st);
hipError_t launch_chain_hits_multi(const HitArgs &A, hipStream_t st);

} // namespace mm2c
#endif
