// chain_segs.h -- argument block and launchers of the fragment-hits-to-segments step (mm_seg_gen, hit.c:373-427), chain_segs.hip.
#ifndef MM2C_CHAIN_SEGS_H
#define MM2C_CHAIN_SEGS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace mm2c {

constexpr int SEG_MAX = 255;           // MM_MAX_SEG: the per-segment counters of one fragment are in LDS

struct SegArgs {
	int64_t n_frags, n_u_cap, n_b_cap, n_su_cap;
	int32_t n_segs;
	const int64_t *u_off;              // n_frags + 1: the hits of fragment f are regs[u_off[f] .. u_off[f] + n_in[f])
	const uint64_t *regs;              // REG_WORDS words per region; never written
	const int32_t *n_in;               // n_frags
	const int64_t *b_off;              // n_frags + 1: the regions' `as` index fragment f's chain anchors from b_off[f] on
	const uint4 *b;                    // never written
	const int32_t *seg_len;            // n_frags * n_segs: qlens, fragment-major
	const uint32_t *hash;              // n_frags
	const int32_t *rep_len;            // n_frags, or NULL
	// out, per segment read f * n_segs + s
	int64_t *su_off, *sb_off;          // n_frags * n_segs + 1 each
	uint64_t *su;                      // n_su_cap: seg[s].u behind the squeeze of hit.c:399-401
	uint4 *sb;                         // n_b_cap: seg[s].a
	uint32_t *seg_hash;                // the fragment's hash, once per segment
	int32_t *seg_rep_len;              // the fragment's rep_len, once per segment (NULL with rep_len)
	// scratch
	int64_t *cnt_u, *cnt_a;            // n_frags * n_segs + 1 each: chains and anchors per segment read; the last entry stays 0
	int32_t *state;                    // n_frags: below zero when the fragment was refused
	int32_t *flags;                    // [0]: fragments refused, [1]: stores that would have left the capacities; [2..3], [4..5]: su_off / sb_off behind the last segment read, copied there behind the scans
};
size_t seg_scan_bytes(int64_t n_seg_reads);
hipError_t launch_seg_count(const SegArgs &A, hipStream_t st);
hipError_t launch_seg_offsets(const SegArgs &A, void *tmp, size_t tmp_bytes, hipStream_t st);
hipError_t launch_seg_scatter(const SegArgs &A, hipStream_t st);
hipError_t launch_seg_mark(const SegArgs &A, uint64_t *seg_regs, hipStream_t st);

} // namespace mm2c
#endif
