// mm2chain_ksw.cpp -- C-ABI entries of the base-alignment step (include/mm2chain.h): ksw plans (ksw_extd2_sse on the device, ksw_extd2.hip) and the
// host-buffer entry built on them.
#include "plan_common.h"
#include "ksw_extd2.h"
#include <cstddef>

using namespace mm2c_api;

static_assert(sizeof(mm2c_ksw_task_t) == sizeof(mm2c::KswTask) && sizeof(mm2c_ksw_task_t) == 40 && offsetof(mm2c_ksw_task_t, flag) == 36, "layout");
static_assert(sizeof(mm2c_ksw_res_t) == sizeof(mm2c::KswRes) && sizeof(mm2c_ksw_res_t) == 48 && offsetof(mm2c_ksw_res_t, status) == 44, "layout");
static_assert(sizeof(mm2c_ksw_score_t) == 29, "layout");
static_assert(MM2C_KSW_FLAGS == mm2c::KSW_FLAGS && MM2C_KSW_MAX_LEN == mm2c::KSW_MAX_LEN && MM2C_KSW_LDS_LEN == mm2c::KSW_LDS_T16 && MM2C_KSW_LDS_LEN == mm2c::KSW_LDS_Q &&
              MM2C_KSW_REFUSED == mm2c::KSW_REFUSED && MM2C_KSW_TOO_BIG == mm2c::KSW_TOO_BIG && MM2C_KSW_CIGAR_CUT == mm2c::KSW_CIGAR_CUT, "constants of mm2chain.h");

struct mm2c_kswplan : PlanBase {           // d_mem: [flags | scratch]; events: begin, behind ksw_rows
	int64_t n_tasks_cap = 0, seq_cap = 0, cigar_cap = 0, slot_bytes = 0;
	int32_t n_slots = 0;
	mm2c::KswArgs K;
};

// what ksw2_extd2_sse.c:78-105 makes of the score set
static int ksw_score(const mm2c_ksw_score_t *sc, mm2c::KswScore *S)
{
	if (!sc) return fail(MM2C_E_ARG, "score set is NULL");
	int q = sc->q, e = sc->e, q2 = sc->q2, e2 = sc->e2;
	if (q < 0 || e < 0 || q2 < 0 || e2 < 0 || q + e + q2 + e2 > 127) return fail(MM2C_E_ARG, "gap costs must be >= 0 with (q + e) + (q2 + e2) <= 127 (options.c:194)");
	S->qe0 = q + e;
	if (q2 + e2 < q + e) { std::swap(q, q2); std::swap(e, e2); }
	S->q = q; S->e = e; S->q2 = q2; S->e2 = e2;
	S->mch = sc->mat[0]; S->mis = sc->mat[1]; S->sc_n = sc->mat[24] == 0 ? -e2 : sc->mat[24];
	int min_sc = sc->mat[1];
	for (int t = 1; t < 25; ++t) min_sc = std::min<int>(min_sc, sc->mat[t]);
	S->early = -min_sc > 2 * (q + e);
	int lt = e != e2 ? (q2 - q) / (e - e2) - 1 : 0;
	if (q2 + e2 + lt * e2 > q + e + lt * e) ++lt;
	S->long_thres = lt; S->long_diff = lt * (e - e2) - (q2 - q) - e2;
	return 0;
}

// the plan with the caller's cut of the scratch; the code of a failure comes back, not only NULL
static int kswplan_make(int64_t n_tasks_cap, int64_t seq_cap, int64_t cigar_cap, int64_t n_slots, int64_t slot_bytes, mm2c_kswplan **out)
{
	*out = nullptr;
	if (!lib_ready()) return fail_not_ready();
	if (n_tasks_cap < 0 || n_tasks_cap > INT32_MAX || seq_cap < 0 || cigar_cap < 0 || n_slots < 1 || n_slots > MM2C_KSW_MAX_SLOTS || slot_bytes < 0 ||
	    slot_bytes > (INT64_MAX >> 12))
		return fail(MM2C_E_ARG, "bad argument");
	mm2c_kswplan *pl = new mm2c_kswplan();
	pl->n_tasks_cap = n_tasks_cap; pl->seq_cap = seq_cap; pl->cigar_cap = cigar_cap;
	pl->n_slots = (int32_t)n_slots;
	pl->slot_bytes = (slot_bytes + 255) & ~(int64_t)255;
	Layout L;
	const size_t o_fl = L.take(16), o_sc = L.take((size_t)pl->slot_bytes * pl->n_slots + 256);
	const hipError_t e = pl->open(L.at, 2);
	if (e != hipSuccess) {
		const int rc = fail(MM2C_E_HIP, "mm2c_kswplan_create: %s (%lld slots of %lld bytes)", hipGetErrorString(e), (long long)n_slots, (long long)pl->slot_bytes);
		mm2c_kswplan_destroy(pl);
		return rc;
	}
	mm2c::KswArgs &K = pl->K;
	K.seq_cap = seq_cap; K.cigar_cap = cigar_cap; K.flags = (int32_t *)(pl->d_mem + o_fl); K.scratch = pl->d_mem + o_sc; K.slot_bytes = pl->slot_bytes; K.n_slots = pl->n_slots;
	*out = pl;
	return 0;
}

extern "C" {

mm2c_kswplan_t *mm2c_kswplan_create_slots(int64_t n_tasks_cap, int64_t seq_cap, int64_t cigar_cap, int64_t n_slots, int64_t slot_bytes)
{
	mm2c_kswplan_t *pl = nullptr;
	(void)kswplan_make(n_tasks_cap, seq_cap, cigar_cap, n_slots, slot_bytes, &pl);
	return pl;
}

mm2c_kswplan_t *mm2c_kswplan_create(int64_t n_tasks_cap, int64_t seq_cap, int64_t cigar_cap, int64_t scratch_bytes)
{
	if (scratch_bytes < 0) { fail(MM2C_E_ARG, "bad argument"); return nullptr; }
	const int64_t n_slots = std::min<int64_t>(std::max<int64_t>(scratch_bytes / MM2C_KSW_SLOT_BYTES, 1), MM2C_KSW_MAX_SLOTS);   // the default cut: slots of 4 MiB
	return mm2c_kswplan_create_slots(n_tasks_cap, seq_cap, cigar_cap, n_slots, scratch_bytes / n_slots & ~(int64_t)255);
}

void mm2c_kswplan_destroy(mm2c_kswplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int64_t mm2c_kswplan_slot_bytes(const mm2c_kswplan_t *pl) { return pl ? pl->slot_bytes : 0; }
int64_t mm2c_kswplan_n_slots(const mm2c_kswplan_t *pl) { return pl ? pl->n_slots : 0; }
int64_t mm2c_ksw_task_scratch(int32_t qlen, int32_t tlen, int32_t w, int32_t flag) { return mm2c::ksw_slot_need(qlen, tlen, w, flag); }

int mm2c_kswplan_run_device(mm2c_kswplan_t *pl, const mm2c_ksw_score_t *sc, int64_t n_tasks, const mm2c_ksw_task_t *d_tasks, const uint8_t *d_seq,
                            const int64_t *d_cig_off, mm2c_ksw_res_t *d_res, uint32_t *d_cigar, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (n_tasks < 0 || n_tasks > pl->n_tasks_cap) return fail(MM2C_E_ARG, "%lld tasks in a plan for %lld", (long long)n_tasks, (long long)pl->n_tasks_cap);
	mm2c::KswScore S;
	if (const int rc = ksw_score(sc, &S)) return rc;
	if (n_tasks > 0 && (!d_tasks || !d_cig_off || !d_res || (pl->seq_cap > 0 && !d_seq) || (pl->cigar_cap > 0 && !d_cigar))) return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_tasks | (uintptr_t)d_cig_off) & 7) return fail(MM2C_E_ARG, "tasks or CIGAR offsets are not 8-byte aligned");
	if (((uintptr_t)d_res | (uintptr_t)d_cigar) & 3) return fail(MM2C_E_ARG, "results or CIGAR words are not 4-byte aligned");
	mm2c::KswArgs &K = pl->K;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, K.flags, 16)) return rc;
	K.n_tasks = n_tasks; K.tasks = (const mm2c::KswTask *)d_tasks; K.seq = d_seq; K.cig_off = d_cig_off; K.res = (mm2c::KswRes *)d_res; K.cigar = d_cigar; K.sc = S;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_ksw_rows(K, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	return pl->end(n_tasks > 0);
}

int mm2c_kswplan_check(mm2c_kswplan_t *pl, int64_t *n_refused, int64_t *n_too_big)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_too_big) *n_too_big = 0;
	if (!pl->ran) return 0;
	int32_t fl[4] = {};
	if (const int rc = pl->read_flags(1, pl->K.flags, fl, sizeof fl)) return rc;
	if (n_refused) *n_refused = fl[0];
	if (n_too_big) *n_too_big = (int64_t)fl[1] + fl[2];
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d task(s) refused: a flag outside MM2C_KSW_FLAGS, a length above MM2C_KSW_MAX_LEN, offsets or lengths that leave seq_cap, or a CIGAR slot that runs "
	                                        "backwards or leaves cigar_cap", fl[0]);
	if (fl[1] != 0 || fl[2] != 0) return fail(MM2C_E_TOOBIG, "%d task(s) do not fit a scratch slot of %lld bytes and were not run; %d CIGAR(s) longer than their slot were cut",
	                                          fl[1], (long long)pl->slot_bytes, fl[2]);
	return 0;
}

int mm2c_kswplan_last_ms(mm2c_kswplan_t *pl, float *ms)
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(1, {{0, 1, ms}});
}

int mm2c_kswplan_last_kernel_ms(mm2c_kswplan_t *pl, float *rows_ms)
{
	return mm2c_kswplan_last_ms(pl, rows_ms);
}

int mm2c_ksw_extd2_batch_host(const mm2c_ksw_score_t *sc, int64_t n_tasks, const mm2c_ksw_task_t *tasks, int64_t seq_len, const uint8_t *seq,
                              const int64_t *cig_off, mm2c_ksw_res_t *res, uint32_t *cigar, int64_t scratch_bytes)
{
	mm2c::KswScore S;
	if (const int rc = ksw_score(sc, &S)) return rc;
	if (n_tasks < 0 || n_tasks > INT32_MAX || seq_len < 0) return fail(MM2C_E_ARG, "bad argument");
	if (n_tasks == 0) return 0;
	if (!tasks || !cig_off || !res || (seq_len > 0 && !seq)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (cig_off[0] != 0) return fail(MM2C_E_ARG, "cig_off[0] must be 0");
	int64_t need = 0;
	for (int64_t i = 0; i < n_tasks; ++i) {
		const mm2c_ksw_task_t &t = tasks[i];
		if (cig_off[i + 1] < cig_off[i]) return fail(MM2C_E_ARG, "CIGAR offsets not monotone at task %lld", (long long)i);
		if (t.flag & ~MM2C_KSW_FLAGS) return fail(MM2C_E_ARG, "task %lld: flag 0x%x has bits outside MM2C_KSW_FLAGS", (long long)i, t.flag);
		if (t.qlen > MM2C_KSW_MAX_LEN || t.tlen > MM2C_KSW_MAX_LEN) return fail(MM2C_E_ARG, "task %lld: longer than MM2C_KSW_MAX_LEN", (long long)i);
		if (t.qlen <= 0 || t.tlen <= 0) continue;
		if (t.q_off < 0 || t.t_off < 0 || t.q_off > seq_len - t.qlen || t.t_off > seq_len - t.tlen) return fail(MM2C_E_ARG, "task %lld leaves the sequences", (long long)i);
		for (int32_t k = 0; k < t.qlen; ++k) if (seq[t.q_off + k] > 4) return fail(MM2C_E_ARG, "task %lld: query code %d at %d", (long long)i, seq[t.q_off + k], k);
		for (int32_t k = 0; k < t.tlen; ++k) if (seq[t.t_off + k] > 4) return fail(MM2C_E_ARG, "task %lld: target code %d at %d", (long long)i, seq[t.t_off + k], k);
		need = std::max(need, mm2c_ksw_task_scratch(t.qlen, t.tlen, t.w, t.flag));
	}
	const int64_t n_cig = cig_off[n_tasks];
	if (n_cig > 0 && !cigar) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (!lib_ready()) return fail_not_ready();
	// slots of the largest task's size: as many as there are tasks to fill them, up to 1 280 and 4 GiB (scratch_bytes <= 0), or as many as scratch_bytes holds
	need = (std::max<int64_t>(need, 4096) + 255) & ~(int64_t)255;
	int64_t slots = std::min<int64_t>(std::min<int64_t>(n_tasks, 1280), (4ll << 30) / need), slot = need;
	if (scratch_bytes > 0) {
		slots = std::min<int64_t>(scratch_bytes / need, MM2C_KSW_MAX_SLOTS);
		if (slots < 1) slot = scratch_bytes;                                 // the largest task does not fit: one slot of what there is, and it comes back too big
	}
	slots = std::max<int64_t>(slots, 1);
	mm2c_kswplan_t *pl = nullptr;
	if (const int rc = kswplan_make(n_tasks, seq_len, n_cig, slots, slot, &pl)) return rc;
	Staging stage;
	const size_t nt = (size_t)n_tasks;
	// res and cigar go up as well: what a task that is not run leaves is the caller's
	const int i_t = stage.add(tasks, nullptr, nt * sizeof(mm2c_ksw_task_t)), i_s = stage.add(seq, nullptr, (size_t)seq_len, 16), i_co = stage.add(cig_off, nullptr, (nt + 1) * 8),
	          i_r = stage.add(res, res, nt * sizeof(mm2c_ksw_res_t)), i_c = stage.add(cigar, cigar, (size_t)n_cig * 4, 16);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_kswplan_run_device(pl, sc, n_tasks, stage.at<mm2c_ksw_task_t>(i_t), stage.at<uint8_t>(i_s), stage.at<int64_t>(i_co), stage.at<mm2c_ksw_res_t>(i_r), stage.at<uint32_t>(i_c),
		                               MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_kswplan_check(pl, nullptr, nullptr); });
	stage.release();
	mm2c_kswplan_destroy(pl);
	return rc;
}

} // extern "C"
