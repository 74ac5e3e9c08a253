// align_extra.h -- argument blocks and launchers of the two CIGAR walks around the base alignment (align.c): mm_update_extra (:240-286, with mm_fix_cigar :91-167 and
// mm_update_cigar_eqx :169-238) for a batch of regions, and mm_test_zdrop (:47-89) over the outputs of a ksw plan.  align_extra.hip.
#ifndef MM2C_ALIGN_EXTRA_H
#define MM2C_ALIGN_EXTRA_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "ksw_extd2.h"

namespace mm2c {

constexpr int EXTRA_LDS_WORDS = 2048;      // MM2C_EXTRA_LDS_WORDS: a CIGAR of up to this many words is worked on in LDS, a longer one in the wave's scratch slot
constexpr int EXTRA_RUN_LANE = 16;         // MM2C_EXTRA_RUN_LANE: an indel's match run is walked by its own lane up to this many bases, by the whole wave beyond
constexpr int EXTRA_MAX_SLOTS = 4096;      // MM2C_EXTRA_MAX_SLOTS
constexpr int EXTRA_REFUSED = 1, EXTRA_TOO_BIG = 2, EXTRA_CIGAR_CUT = 3;   // status of a region or task

struct ExtraTask { int64_t q_off, t_off; int32_t qlen, tlen, n_cigar, rev; };                       // mm2c_extra_task_t
struct ExtraRes { int32_t n_cigar, qshift, tshift, blen, mlen, n_ambi, dp_max, status; };            // mm2c_extra_res_t
struct ZdropOpt { int32_t zdrop, zdrop_inv, max_gap, no_inv; };                                      // mm2c_zdrop_opt_t
struct ZdropRes { int32_t max_zdrop, t0, t1, q0, q1, code, inv_cand, status; };                      // mm2c_zdrop_res_t

struct ExtraArgs {
	int64_t n, seq_cap, in_cap, out_cap;   // in_cap: words of cig_in (update) or of the ksw plan's cigar (zdrop)
	const uint8_t *seq;                    // codes 0..4, never written
	int32_t mat[25];
	int32_t q, e;                          // both >= 0
	// mm_update_extra
	const ExtraTask *tasks;
	const int64_t *in_off, *out_off;       // n and n + 1 entries
	const uint32_t *cig_in;
	uint32_t *cig_out;
	ExtraRes *res;
	int32_t is_eqx;
	// mm_test_zdrop
	const KswTask *ktasks;
	const int64_t *cig_off;
	const KswRes *kres;
	const uint32_t *kcigar;
	ZdropOpt zo;
	ZdropRes *zres;
	// both
	uint32_t *scratch;                     // n_slots slots of 4 * slot_words words: the working arrays of a CIGAR longer than EXTRA_LDS_WORDS
	int64_t slot_words;
	int32_t n_slots;
	int32_t *flags;                        // [0]: refused, [1]: CIGARs beyond LDS and slot, [2]: output CIGARs cut
};
hipError_t launch_extra_update(const ExtraArgs &A, hipStream_t st);
hipError_t launch_extra_zdrop(const ExtraArgs &A, hipStream_t st);

} // namespace mm2c
#endif
