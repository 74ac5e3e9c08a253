// mm2chain_extra.cpp -- C-ABI entries of the two CIGAR walks around the base alignment (include/mm2chain.h): extra plans (mm_update_extra and mm_test_zdrop on the
// device, align_extra.hip) and the host-buffer entries built on them.
#include "plan_common.h"
#include "align_extra.h"
#include <cstddef>

using namespace mm2c_api;

static_assert(sizeof(mm2c_extra_task_t) == sizeof(mm2c::ExtraTask) && sizeof(mm2c_extra_task_t) == 32 && offsetof(mm2c_extra_task_t, rev) == 28, "layout");
static_assert(sizeof(mm2c_extra_res_t) == sizeof(mm2c::ExtraRes) && sizeof(mm2c_extra_res_t) == 32 && offsetof(mm2c_extra_res_t, status) == 28, "layout");
static_assert(sizeof(mm2c_zdrop_opt_t) == sizeof(mm2c::ZdropOpt) && sizeof(mm2c_zdrop_opt_t) == 16, "layout");
static_assert(sizeof(mm2c_zdrop_res_t) == sizeof(mm2c::ZdropRes) && sizeof(mm2c_zdrop_res_t) == 32 && offsetof(mm2c_zdrop_res_t, status) == 28, "layout");
static_assert(MM2C_EXTRA_LDS_WORDS == mm2c::EXTRA_LDS_WORDS && MM2C_EXTRA_RUN_LANE == mm2c::EXTRA_RUN_LANE && MM2C_EXTRA_MAX_SLOTS == mm2c::EXTRA_MAX_SLOTS &&
              MM2C_EXTRA_REFUSED == mm2c::EXTRA_REFUSED && MM2C_EXTRA_TOO_BIG == mm2c::EXTRA_TOO_BIG && MM2C_EXTRA_CIGAR_CUT == mm2c::EXTRA_CIGAR_CUT, "constants of mm2chain.h");

struct mm2c_extraplan : PlanBase {         // d_mem: [flags | scratch]; events: begin and end of the last update run (0, 1), of the last z-drop run (2, 3)
	int64_t n_cap = 0, seq_cap = 0, cig_in_cap = 0, cig_out_cap = 0, slot_words = 0;
	int32_t n_slots = 0;
	int32_t *d_flags = nullptr;
	uint32_t *d_scratch = nullptr;
	bool did[2] = {false, false};          // update, z-drop: which of the two has run; `ran` is either
	int last = -1;                         // 0: update, 1: z-drop
};

static int extra_score(const mm2c_ksw_score_t *sc, mm2c::ExtraArgs *X)
{
	if (!sc) return fail(MM2C_E_ARG, "score set is NULL");
	if (sc->q < 0 || sc->e < 0) return fail(MM2C_E_ARG, "gap costs q and e must be >= 0 (align.c:268 would wrap in unsigned arithmetic)");
	for (int k = 0; k < 25; ++k) X->mat[k] = sc->mat[k];
	X->q = sc->q; X->e = sc->e;
	return 0;
}

static bool ranges_overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
	const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb;
	return na > 0 && nb > 0 && a0 < b1 && b0 < a1;
}

static int extraplan_make(int64_t n_cap, int64_t seq_cap, int64_t cig_in_cap, int64_t cig_out_cap, int64_t n_slots, int64_t slot_words, mm2c_extraplan **out)
{
	*out = nullptr;
	if (!lib_ready()) return fail_not_ready();
	if (n_slots <= 0) n_slots = 2048;
	if (n_cap < 0 || n_cap > INT32_MAX || seq_cap < 0 || cig_in_cap < 0 || cig_out_cap < 0 || n_slots > MM2C_EXTRA_MAX_SLOTS || slot_words < 0 || slot_words > INT32_MAX)
		return fail(MM2C_E_ARG, "bad argument");
	mm2c_extraplan *pl = new mm2c_extraplan();
	pl->n_cap = n_cap; pl->seq_cap = seq_cap; pl->cig_in_cap = cig_in_cap; pl->cig_out_cap = cig_out_cap;
	pl->n_slots = (int32_t)n_slots; pl->slot_words = slot_words;
	Layout L;
	const size_t o_fl = L.take(16), o_sc = L.take((size_t)slot_words * 16 * (size_t)n_slots + 256);
	const hipError_t e = pl->open(L.at, 4);
	if (e != hipSuccess) {
		const int rc = fail(MM2C_E_HIP, "mm2c_extraplan_create: %s (%lld slots of %lld words)", hipGetErrorString(e), (long long)n_slots, (long long)slot_words);
		mm2c_extraplan_destroy(pl);
		return rc;
	}
	pl->d_flags = (int32_t *)(pl->d_mem + o_fl); pl->d_scratch = (uint32_t *)(pl->d_mem + o_sc);
	*out = pl;
	return 0;
}

static int extra_launch(mm2c_extraplan *pl, mm2c::ExtraArgs &X, int which, void *stream)
{
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, pl->d_flags, 16)) return rc;
	X.seq_cap = pl->seq_cap; X.scratch = pl->d_scratch; X.slot_words = pl->slot_words; X.n_slots = pl->n_slots; X.flags = pl->d_flags;
	HIP_TRY(hipEventRecord(pl->ev[2 * which], st));
	HIP_TRY(which == 0 ? mm2c::launch_extra_update(X, st) : mm2c::launch_extra_zdrop(X, st));
	HIP_TRY(hipEventRecord(pl->ev[2 * which + 1], st));
	pl->did[which] = true; pl->last = which;
	return pl->end(X.n > 0);
}

extern "C" {

mm2c_extraplan_t *mm2c_extraplan_create(int64_t n_cap, int64_t seq_cap, int64_t cig_in_cap, int64_t cig_out_cap, int64_t n_slots, int64_t slot_words)
{
	mm2c_extraplan_t *pl = nullptr;
	(void)extraplan_make(n_cap, seq_cap, cig_in_cap, cig_out_cap, n_slots, slot_words, &pl);
	return pl;
}

void mm2c_extraplan_destroy(mm2c_extraplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_extraplan_run_device(mm2c_extraplan_t *pl, const mm2c_ksw_score_t *sc, int is_eqx, int64_t n_regs, const mm2c_extra_task_t *d_tasks, const uint8_t *d_seq,
                              const int64_t *d_in_off, const uint32_t *d_cig_in, const int64_t *d_out_off, mm2c_extra_res_t *d_res, uint32_t *d_cig_out, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (n_regs < 0 || n_regs > pl->n_cap) return fail(MM2C_E_ARG, "%lld regions in a plan for %lld", (long long)n_regs, (long long)pl->n_cap);
	mm2c::ExtraArgs X = {};
	if (const int rc = extra_score(sc, &X)) return rc;
	if (n_regs > 0 && (!d_tasks || !d_in_off || !d_out_off || !d_res || (pl->seq_cap > 0 && !d_seq) || (pl->cig_in_cap > 0 && !d_cig_in) || (pl->cig_out_cap > 0 && !d_cig_out)))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_tasks | (uintptr_t)d_in_off | (uintptr_t)d_out_off) & 7) return fail(MM2C_E_ARG, "tasks or CIGAR offsets are not 8-byte aligned");
	if (((uintptr_t)d_res | (uintptr_t)d_cig_in | (uintptr_t)d_cig_out) & 3) return fail(MM2C_E_ARG, "results or CIGAR words are not 4-byte aligned");
	if (ranges_overlap(d_cig_in, pl->cig_in_cap * 4, d_cig_out, pl->cig_out_cap * 4)) return fail(MM2C_E_ARG, "the input and output CIGAR buffers overlap");
	X.n = n_regs; X.in_cap = pl->cig_in_cap; X.out_cap = pl->cig_out_cap; X.seq = d_seq; X.tasks = (const mm2c::ExtraTask *)d_tasks; X.in_off = d_in_off; X.out_off = d_out_off;
	X.cig_in = d_cig_in; X.cig_out = d_cig_out; X.res = (mm2c::ExtraRes *)d_res; X.is_eqx = is_eqx != 0;
	return extra_launch(pl, X, 0, stream);
}

int mm2c_extraplan_zdrop_run_device(mm2c_extraplan_t *pl, const mm2c_ksw_score_t *sc, const mm2c_zdrop_opt_t *opt, int64_t n_tasks, const mm2c_ksw_task_t *d_tasks,
                                    const uint8_t *d_seq, const int64_t *d_cig_off, const mm2c_ksw_res_t *d_res, const uint32_t *d_cigar, mm2c_zdrop_res_t *d_zres, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (n_tasks < 0 || n_tasks > pl->n_cap) return fail(MM2C_E_ARG, "%lld tasks in a plan for %lld", (long long)n_tasks, (long long)pl->n_cap);
	mm2c::ExtraArgs X = {};
	if (const int rc = extra_score(sc, &X)) return rc;
	if (!opt) return fail(MM2C_E_ARG, "z-drop options are NULL");
	if (n_tasks > 0 && (!d_tasks || !d_cig_off || !d_res || !d_zres || (pl->seq_cap > 0 && !d_seq) || (pl->cig_in_cap > 0 && !d_cigar))) return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_tasks | (uintptr_t)d_cig_off) & 7) return fail(MM2C_E_ARG, "tasks or CIGAR offsets are not 8-byte aligned");
	if (((uintptr_t)d_res | (uintptr_t)d_cigar | (uintptr_t)d_zres) & 3) return fail(MM2C_E_ARG, "results or CIGAR words are not 4-byte aligned");
	X.n = n_tasks; X.in_cap = pl->cig_in_cap; X.seq = d_seq; X.ktasks = (const mm2c::KswTask *)d_tasks; X.cig_off = d_cig_off; X.kres = (const mm2c::KswRes *)d_res;
	X.kcigar = d_cigar; X.zres = (mm2c::ZdropRes *)d_zres;
	X.zo = mm2c::ZdropOpt{opt->zdrop, opt->zdrop_inv, opt->max_gap, opt->no_inv};
	return extra_launch(pl, X, 1, stream);
}

int mm2c_extraplan_check(mm2c_extraplan_t *pl, int64_t *n_refused, int64_t *n_too_big)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_too_big) *n_too_big = 0;
	if (pl->last < 0) return 0;
	int32_t fl[4] = {};
	if (const int rc = pl->read_flags(2 * pl->last + 1, pl->d_flags, fl, sizeof fl)) return rc;
	if (n_refused) *n_refused = fl[0];
	if (n_too_big) *n_too_big = (int64_t)fl[1] + fl[2];
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d item(s) refused: a CIGAR the reference is not defined on (an op above 3, an empty N, only empty words, lengths that do not add up to the "
	                                        "sequences), offsets or lengths that leave a pool or run backwards, a length above MM2C_KSW_MAX_LEN, or a ksw task whose status is not 0", fl[0]);
	if (fl[1] != 0 || fl[2] != 0) return fail(MM2C_E_TOOBIG, "%d CIGAR(s) longer than MM2C_EXTRA_LDS_WORDS and than a scratch slot of %lld words were not run; %d output CIGAR(s) longer "
	                                                         "than their slot were cut", fl[1], (long long)pl->slot_words, fl[2]);
	return 0;
}

int mm2c_extraplan_last_kernel_ms(mm2c_extraplan_t *pl, float *update_ms, float *zdrop_ms)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (pl->last < 0) return fail(MM2C_E_ARG, "plan has not been run");
	float *const out[2] = {update_ms, zdrop_ms};
	for (int w = 0; w < 2; ++w) {
		if (!out[w]) continue;
		*out[w] = 0.f;
		if (!pl->did[w]) continue;
		if (const int rc = pl->elapsed(2 * w + 1, {{2 * w, 2 * w + 1, out[w]}})) return rc;
	}
	return 0;
}

int mm2c_extraplan_last_ms(mm2c_extraplan_t *pl, float *ms)
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (pl->last < 0) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->last == 0 ? mm2c_extraplan_last_kernel_ms(pl, ms, nullptr) : mm2c_extraplan_last_kernel_ms(pl, nullptr, ms);
}

static int check_codes(int64_t seq_len, const uint8_t *seq)
{
	for (int64_t k = 0; k < seq_len; ++k) if (seq[k] > 4) return fail(MM2C_E_ARG, "base code %d at %lld", seq[k], (long long)k);
	return 0;
}

int mm2c_update_extra_batch_host(const mm2c_ksw_score_t *sc, int is_eqx, int64_t n_regs, const mm2c_extra_task_t *tasks, int64_t seq_len, const uint8_t *seq,
                                 const int64_t *in_off, int64_t n_cig_in, const uint32_t *cig_in, const int64_t *out_off, mm2c_extra_res_t *res, uint32_t *cig_out)
{
	mm2c::ExtraArgs X = {};
	if (const int rc = extra_score(sc, &X)) return rc;
	if (n_regs < 0 || n_regs > INT32_MAX || seq_len < 0 || n_cig_in < 0) return fail(MM2C_E_ARG, "bad argument");
	if (n_regs == 0) return 0;
	if (!tasks || !in_off || !out_off || !res || (seq_len > 0 && !seq) || (n_cig_in > 0 && !cig_in)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (out_off[0] != 0) return fail(MM2C_E_ARG, "out_off[0] must be 0");
	int64_t longest = 0;
	for (int64_t i = 0; i < n_regs; ++i) {
		if (out_off[i + 1] < out_off[i]) return fail(MM2C_E_ARG, "output offsets not monotone at region %lld", (long long)i);
		if (tasks[i].n_cigar < 0 || in_off[i] < 0 || in_off[i] > n_cig_in - tasks[i].n_cigar) return fail(MM2C_E_ARG, "region %lld: its CIGAR leaves the input words", (long long)i);
		longest = std::max<int64_t>(longest, tasks[i].n_cigar);
	}
	const int64_t n_out = out_off[n_regs];
	if (n_out > 0 && !cig_out) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (ranges_overlap(cig_in, n_cig_in * 4, cig_out, n_out * 4)) return fail(MM2C_E_ARG, "the input and output CIGAR buffers overlap");
	if (const int rc = check_codes(seq_len, seq)) return rc;
	if (!lib_ready()) return fail_not_ready();
	const int64_t slot_words = longest > MM2C_EXTRA_LDS_WORDS ? longest : 0;
	const int64_t slots = slot_words ? std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_regs, 2048), (1ll << 30) / (slot_words * 16))) : 0;
	mm2c_extraplan_t *pl = nullptr;
	if (const int rc = extraplan_make(n_regs, seq_len, n_cig_in, n_out, slots, slot_words, &pl)) return rc;
	Staging stage;
	const size_t nr = (size_t)n_regs;
	// res and cig_out go up as well: what a region that is not run leaves is the caller's
	const int i_t = stage.add(tasks, nullptr, nr * sizeof(mm2c_extra_task_t)), i_s = stage.add(seq, nullptr, (size_t)seq_len, 16), i_io = stage.add(in_off, nullptr, nr * 8),
	          i_oo = stage.add(out_off, nullptr, (nr + 1) * 8), i_r = stage.add(res, res, nr * sizeof(mm2c_extra_res_t)), i_ci = stage.add(cig_in, nullptr, (size_t)n_cig_in * 4, 16),
	          i_co = stage.add(cig_out, cig_out, (size_t)n_out * 4, 16);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_extraplan_run_device(pl, sc, is_eqx, n_regs, stage.at<mm2c_extra_task_t>(i_t), stage.at<uint8_t>(i_s), stage.at<int64_t>(i_io), stage.at<uint32_t>(i_ci), stage.at<int64_t>(i_oo),
		                                 stage.at<mm2c_extra_res_t>(i_r), stage.at<uint32_t>(i_co), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_extraplan_check(pl, nullptr, nullptr); });
	stage.release();
	mm2c_extraplan_destroy(pl);
	return rc;
}

int mm2c_test_zdrop_batch_host(const mm2c_ksw_score_t *sc, const mm2c_zdrop_opt_t *opt, int64_t n_tasks, const mm2c_ksw_task_t *tasks, int64_t seq_len, const uint8_t *seq,
                               const int64_t *cig_off, const mm2c_ksw_res_t *kres, const uint32_t *cigar, mm2c_zdrop_res_t *zres)
{
	mm2c::ExtraArgs X = {};
	if (const int rc = extra_score(sc, &X)) return rc;
	if (!opt) return fail(MM2C_E_ARG, "z-drop options are NULL");
	if (n_tasks < 0 || n_tasks > INT32_MAX || seq_len < 0) return fail(MM2C_E_ARG, "bad argument");
	if (n_tasks == 0) return 0;
	if (!tasks || !cig_off || !kres || !zres || (seq_len > 0 && !seq)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (cig_off[0] != 0) return fail(MM2C_E_ARG, "cig_off[0] must be 0");
	int64_t longest = 0;
	for (int64_t i = 0; i < n_tasks; ++i) {
		if (cig_off[i + 1] < cig_off[i]) return fail(MM2C_E_ARG, "CIGAR offsets not monotone at task %lld", (long long)i);
		if (kres[i].status == 0) longest = std::max<int64_t>(longest, kres[i].n_cigar);
	}
	const int64_t n_cig = cig_off[n_tasks];
	if (n_cig > 0 && !cigar) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (const int rc = check_codes(seq_len, seq)) return rc;
	if (!lib_ready()) return fail_not_ready();
	const int64_t slot_words = longest > MM2C_EXTRA_LDS_WORDS ? longest : 0;
	const int64_t slots = slot_words ? std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_tasks, 2048), (1ll << 30) / (slot_words * 16))) : 0;
	mm2c_extraplan_t *pl = nullptr;
	if (const int rc = extraplan_make(n_tasks, seq_len, n_cig, 0, slots, slot_words, &pl)) return rc;
	Staging stage;
	const size_t nt = (size_t)n_tasks;
	const int i_t = stage.add(tasks, nullptr, nt * sizeof(mm2c_ksw_task_t)), i_s = stage.add(seq, nullptr, (size_t)seq_len, 16), i_co = stage.add(cig_off, nullptr, (nt + 1) * 8),
	          i_r = stage.add(kres, nullptr, nt * sizeof(mm2c_ksw_res_t)), i_c = stage.add(cigar, nullptr, (size_t)n_cig * 4, 16), i_z = stage.add(zres, zres, nt * sizeof(mm2c_zdrop_res_t));
	const int rc = stage.through(pl->device, [&] {
		return mm2c_extraplan_zdrop_run_device(pl, sc, opt, n_tasks, stage.at<mm2c_ksw_task_t>(i_t), stage.at<uint8_t>(i_s), stage.at<int64_t>(i_co), stage.at<mm2c_ksw_res_t>(i_r), stage.at<uint32_t>(i_c),
		                                       stage.at<mm2c_zdrop_res_t>(i_z), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_extraplan_check(pl, nullptr, nullptr); });
	stage.release();
	mm2c_extraplan_destroy(pl);
	return rc;
}

} // extern "C"
