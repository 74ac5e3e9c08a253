// chain_mapq.h -- argument block and launchers of the hits-to-mapping-quality step (mm_join_long hit.c:295-371, mm_set_mapq hit.c:463-508), chain_mapq.hip.
#ifndef MM2C_CHAIN_MAPQ_H
#define MM2C_CHAIN_MAPQ_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2c {

constexpr int MAPQ_LDS_MAX = 128;      // mapq_join: reads of up to this many hits keep their tables in LDS, longer ones in the plan's scratch (same code)
constexpr int MAPQ_TAB_ROWS = 24;      // 32-bit table rows per hit (chain_mapq.hip, MapqTab)
constexpr int MAPQ_JUNC_ROWS = 4;      // 64-bit rows per hit: x and y of the two anchors at a junction
constexpr int MAPQ_SLICE = 4096;       // mapq_gather: anchors of one workgroup step (256 lanes, sixteen 16-byte anchors each)

enum { MAPQ_READ_BAD = 0, MAPQ_READ_COPY = 1, MAPQ_READ_SQUEEZED = 2 };   // MapqArgs::state

struct MapqArgs {
	int64_t n_reads, n_u_cap, n_b_cap;
	int32_t do_join, max_join_long, max_join_short, min_join_flank_sc;   // mm_join_long
	float min_join_flank_ratio;
	int32_t min_cnt, min_chain_score;                                    // mm_filter_regs, mm_set_mapq
	int32_t max_log_arg;               // logtab holds logf((float)i) for 0 <= i <= max_log_arg
	const float *logtab;
	const int64_t *u_off;              // n_reads + 1: the hits of read r are in[u_off[r] .. u_off[r] + n_in[r])
	const uint64_t *in;                // REG_WORDS words per hit
	const int32_t *n_in;               // n_reads
	const int64_t *b_off;              // n_reads + 1: the chain anchors of read r are b[b_off[r] .. b_off[r+1])
	const uint4 *b;                    // never written
	const int32_t *qlen, *rep_len;     // n_reads (qlen is not read: a join needs no mm_reg_set_coor)
	uint64_t *out;                     // the final regions of read r from u_off[r] on, n_out[r] of them
	int32_t *n_out;                    // n_reads
	uint4 *b_out;                      // NULL: no anchor is copied
	int64_t *n_b_out;                  // n_reads, NULL with b_out
	// scratch
	int4 *moves;                       // n_u_cap: per hit in ascending `as` (src, dst, cnt, join), indexed from u_off[r] on
	int32_t *state;                    // n_reads: MAPQ_READ_*
	int32_t *tab;                      // MAPQ_TAB_ROWS rows of n_u_cap + n_reads entries for reads beyond MAPQ_LDS_MAX
	uint64_t *junc;                    // MAPQ_JUNC_ROWS rows of n_u_cap entries
	int32_t *flags;                    // [0]: reads refused for their offsets; zero on entry
	unsigned long long *counts;        // [0]: joins, [1]: primaries beyond the table; zero on entry
};
hipError_t launch_mapq_join(const MapqArgs &A, hipStream_t st);
hipError_t launch_mapq_gather(const MapqArgs &A, hipStream_t st);

} // namespace mm2c
#endif
