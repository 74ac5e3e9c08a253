// ksw_extd2.h -- argument block and launcher of the base-alignment step (ksw_extd2_sse, ksw2_extd2_sse.c, as a batch of independent tasks), ksw_extd2.hip.
#ifndef MM2C_KSW_EXTD2_H
#define MM2C_KSW_EXTD2_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace mm2c {

constexpr int KSW_MAX_LEN = 1 << 20;       // MM2C_KSW_MAX_LEN: longer queries or targets are refused (t and the lane tag of the exact maximum share one 32-bit key)
constexpr int KSW_LDS_T16 = 2304;          // the array image of a task lies in LDS up to this many padded target bases ...
constexpr int KSW_LDS_Q = 2304;            // ... and this many query bases; beyond either it lies in the task slot's scratch
constexpr int KSW_FLAGS = 0x01 | 0x02 | 0x08 | 0x10 | 0x40 | 0x80;   // SCORE_ONLY, RIGHT, APPROX_MAX, APPROX_DROP, EXTZ_ONLY, REV_CIGAR
constexpr int KSW_REFUSED = 1, KSW_TOO_BIG = 2, KSW_CIGAR_CUT = 3;   // mm2c_ksw_res_t::status

struct KswScore {                          // what ksw2_extd2_sse.c:68-105 derives from the score set, once per call
	int32_t q, e, q2, e2;                  // behind the swap of :78
	int32_t qe0;                           // q + e in front of it (`qe` of :68: H of row 0)
	int32_t mch, mis, sc_n;                // mat[0], mat[1], mat[24] or -e2
	int32_t long_thres, long_diff;
	int32_t early;                         // the return of :100: every task leaves a reset ez
};

struct KswTask { int64_t q_off, t_off; int32_t qlen, tlen, w, zdrop, end_bonus, flag; };     // mm2c_ksw_task_t
struct KswRes { uint32_t max; int32_t zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end, status; };   // mm2c_ksw_res_t

struct KswArgs {
	int64_t n_tasks, seq_cap, cigar_cap;
	const KswTask *tasks;
	const uint8_t *seq;                    // codes 0..4, never written
	const int64_t *cig_off;                // n_tasks + 1: task i owns cigar[cig_off[i] .. cig_off[i + 1])
	KswRes *res;
	uint32_t *cigar;
	char *scratch;                         // n_slots * slot_bytes: per slot [p | off, off_end | the walk's CIGAR | the array image when it does not fit LDS]
	int64_t slot_bytes;
	int32_t n_slots;
	int32_t *flags;                        // [0]: tasks refused, [1]: tasks whose p or image does not fit a slot, [2]: CIGARs cut
	KswScore sc;
};
int64_t ksw_slot_need(int32_t qlen, int32_t tlen, int32_t w, int32_t flag);   // the scratch a task takes (host and device agree on it)
hipError_t launch_ksw_rows(const KswArgs &A, hipStream_t st);

} // namespace mm2c
#endif
