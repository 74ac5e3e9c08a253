// chain_regs.h -- argument block and launcher of the chains-to-regions step (mm_gen_regs, hit.c:8-88), chain_regs.hip.
#ifndef MM2C_CHAIN_REGS_H
#define MM2C_CHAIN_REGS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2c {

constexpr int REG_WORDS = 10;          // a region (mm_reg1_t, minimap.h:85-100) is 80 bytes: ten 64-bit words
constexpr int REGS_TS_MAX = 4096;      // regs_sort: reads of up to this many chains replay klib's sort with the arrangement in LDS, longer ones through memory
constexpr int REGS_FILL_ROWS = 16;     // regs_fill: a wave takes a slice of this many rows of 64 chain anchors ...
constexpr int REGS_FILL_WAVES = 4;     // ... and a workgroup this many slices

struct RegArgs {
	int64_t n_reads, n_u_cap, n_b_cap;
	// the device epilogue's compact output: chains of read r are u[u_off[r] .. u_off[r+1]), their anchors b[b_off[r] .. b_off[r+1])
	const int64_t *u_off, *b_off;      // n_reads + 1 each
	const uint64_t *u;
	const ulonglong2 *b;
	const int32_t *qlen;               // per read
	const uint32_t *hash;              // per read (map.c:290-292)
	uint64_t *regs;                    // out: REG_WORDS words per chain, indexed like u
	// scratch, n_u_cap entries each
	uint64_t *zkey, *key0, *key1;      // the sort keys z.x in chain order (never overwritten) / the two buffers of the sorts
	int64_t *cstart, *cend;            // per chain: its anchors are b[cstart .. cend), clamped to the read's extent
	int32_t *val0, *val1, *crank, *tiecnt, *stack, *moved;   // crank: chain -> its region
	int32_t *flags;                    // [0]: reads whose counts or offsets disagree, [1]: reads that hold equal keys, [2]: reads refused for their offsets (regs_fill
	                                   // then goes read by read); four words, zero on entry
};
// ev_mid (optional) is recorded between the two kernels
hipError_t launch_chain_regs(const RegArgs &A, hipStream_t st, hipEvent_t ev_mid, int *n_launches);

} // namespace mm2c
#endif
