// chain_esterr.h -- argument block and launchers of the chain-anchor divergence step (mm_est_err map.c:357, esterr.c), chain_esterr.hip.
#ifndef MM2C_CHAIN_ESTERR_H
#define MM2C_CHAIN_ESTERR_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2c {

constexpr int ERR_READS_LANES = 256;   // err_reads: lanes of the workgroup that takes one read
constexpr int ERR_SLICE = 4096;        // err_walk: anchors of one workgroup step (256 lanes, sixteen anchors each), as MAPQ_SLICE

enum { ERR_READ_BAD = -1, ERR_READ_NO_MINI = -2 };   // ErrArgs::state below zero; from zero on it is the number of entries of the read's table

struct ErrArgs {
	int64_t n_reads, n_u_cap, n_b_cap, n_mini_cap;
	int32_t n_ref;
	const int64_t *u_off;              // n_reads + 1: the final regions of read r are regs[u_off[r] .. u_off[r] + n_in[r])
	const uint64_t *regs;              // REG_WORDS words per region; never written
	const int32_t *n_in;               // n_reads
	const int64_t *b_off;              // n_reads + 1: the regions' `as` index read r's anchors from b_off[r] on, b_off[r+1] - b_off[r] of them
	const uint4 *b;                    // never written
	const int64_t *mini_off;           // n_reads + 1: mini_pos[mini_off[r] .. mini_off[r+1])
	const uint64_t *mini_pos;          // q_span << 32 | q_pos
	const int32_t *qlen;               // n_reads
	const uint32_t *ref_len;           // n_ref: mi->seq[rid].len
	int2 *err;                         // out: (n_match, n_tot) per region, indexed like regs
	float *avg_k;                      // out: n_reads
	// scratch
	int4 *tab;                         // n_u_cap: per region with cnt > 0, in ascending `as`, (as, cnt, region, 0), from u_off[r] on
	int32_t *first_fail;               // n_u_cap: per region the smallest walk index k >= 1 that is not matched, cnt if there is none
	int32_t *state;                    // n_reads
	int32_t *flags;                    // [0]: reads refused; zero on entry
};
hipError_t launch_err_reads(const ErrArgs &A, hipStream_t st);
hipError_t launch_err_walk(const ErrArgs &A, hipStream_t st);
hipError_t launch_err_finish(const ErrArgs &A, hipStream_t st);

} // namespace mm2c
#endif
