// mm2chain_cig.cpp -- C-ABI entries of the step between the ksw results and mm_update_extra (include/mm2chain.h): the plan that lists the second passes and joins
// the results of a region's tasks into its CIGAR, dp_score, coordinates and split decision (the rest of mm_align1 on the device, align_cigar.hip), and the two
// host-buffer entries built on it.
#include "plan_common.h"
#include "align_cigar.h"
#include <cstddef>

using namespace mm2c_api;

static_assert(sizeof(mm2c_cig_opt_t) == sizeof(mm2c::CigOpt) && sizeof(mm2c_cig_opt_t) == 24 && offsetof(mm2c_cig_opt_t, cig_shift) == 20, "layout");
static_assert(sizeof(mm2c_cig_reg_t) == sizeof(mm2c::CigReg) && sizeof(mm2c_cig_reg_t) == 72 && offsetof(mm2c_cig_reg_t, cig0) == 64 && offsetof(mm2c_cig_reg_t, r_qs) == 56, "layout");
static_assert(sizeof(mm2c_zdrop_res_t) == sizeof(mm2c::ZdropRes) && sizeof(mm2c_extra_task_t) == sizeof(mm2c::ExtraTask) && sizeof(mm2c_ksw_res_t) == sizeof(mm2c::KswRes), "layout");
static_assert(MM2C_CIG_REFUSED == mm2c::CIG_REFUSED && MM2C_CIG_INCOMPLETE == mm2c::CIG_INCOMPLETE && MM2C_CIG_OVER_CAP == mm2c::CIG_OVER_CAP && MM2C_CIG_PIECE == mm2c::CIG_PIECE &&
              MM2C_CIG_NO_ROOM == mm2c::CIG_NO_ROOM && MM2C_CIG_LOST == mm2c::CIG_LOST, "constants of mm2chain.h");

struct mm2c_cigplan : PlanBase {           // d_mem: [join: flags, totals | second: flags, totals | per-region scan words]; events: 0-2 the second-pass entry, 3-6 the join entry
	int64_t n_regs_cap = 0, items_cap = 0, tasks_cap = 0, cig_cap = 0, tasks2_cap = 0, cig2_cap = 0, pool_cap = 0, b_cap = 0, words_cap = 0, extra_cap = 0;
	char *d_join = nullptr, *d_second = nullptr;
	mm2c::CigSec *d_sec = nullptr;
	bool did[2] = {false, false};          // the second-pass entry, the join entry
};

static int check_opt(const mm2c_cig_opt_t *opt)
{
	if (!opt) return fail(MM2C_E_ARG, "options are NULL");
	if (opt->cig_shift < 0 || opt->cig_shift > 30 || opt->bw_ext < 0 || opt->min_cnt < 0) return fail(MM2C_E_ARG, "cig_shift, bw_ext or min_cnt out of range");
	if (opt->flag & MM2C_ALN_F_SPLICE) return fail(MM2C_E_ARG, "splice is not built");
	return 0;
}

static bool ranges_overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
	const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb;
	return na > 0 && nb > 0 && a0 < b1 && b0 < a1;
}

static void fill(mm2c::CigArgs &X, const mm2c_cigplan *pl, const mm2c_cig_opt_t *opt, int64_t n_regs)
{
	X.n_regs = n_regs; X.items_cap = pl->items_cap; X.tasks_cap = pl->tasks_cap; X.cig_cap = pl->cig_cap; X.tasks2_cap = pl->tasks2_cap; X.cig2_cap = pl->cig2_cap;
	X.pool_cap = pl->pool_cap; X.b_cap = pl->b_cap; X.words_cap = pl->words_cap; X.extra_cap = pl->extra_cap;
	memcpy(&X.opt, opt, sizeof X.opt);
	X.sec = pl->d_sec;
}

extern "C" {

mm2c_cigplan_t *mm2c_cigplan_create(int64_t n_regs_cap, int64_t n_items_cap, int64_t n_tasks_cap, int64_t cigar_cap, int64_t n_tasks2_cap, int64_t cigar2_cap, int64_t pool_cap,
                                    int64_t n_b_cap, int64_t words_cap, int64_t n_extra_cap)
{
	if (!lib_ready()) { (void)fail_not_ready(); return nullptr; }
	if (n_regs_cap < 0 || n_regs_cap > INT32_MAX || n_items_cap < 0 || n_tasks_cap < 0 || n_tasks_cap > INT32_MAX || cigar_cap < 0 || n_tasks2_cap < 0 || n_tasks2_cap > INT32_MAX ||
	    cigar2_cap < 0 || pool_cap < 0 || n_b_cap < 0 || words_cap < 0 || n_extra_cap < 0 || n_extra_cap > INT32_MAX) {
		(void)fail(MM2C_E_ARG, "bad argument");
		return nullptr;
	}
	mm2c_cigplan *pl = new mm2c_cigplan();
	pl->n_regs_cap = n_regs_cap; pl->items_cap = n_items_cap; pl->tasks_cap = n_tasks_cap; pl->cig_cap = cigar_cap; pl->tasks2_cap = n_tasks2_cap; pl->cig2_cap = cigar2_cap;
	pl->pool_cap = pool_cap; pl->b_cap = n_b_cap; pl->words_cap = words_cap; pl->extra_cap = n_extra_cap;
	Layout L;
	const size_t o_j = L.take(64), o_s = L.take(64), o_c = L.take((size_t)n_regs_cap * sizeof(mm2c::CigSec) + 16);
	const hipError_t e = pl->open(L.at, 7);
	if (e != hipSuccess) {
		(void)fail(MM2C_E_HIP, "mm2c_cigplan_create: %s (%lld regions)", hipGetErrorString(e), (long long)n_regs_cap);
		mm2c_cigplan_destroy(pl);
		return nullptr;
	}
	pl->d_join = pl->d_mem + o_j; pl->d_second = pl->d_mem + o_s; pl->d_sec = (mm2c::CigSec *)(pl->d_mem + o_c);
	return pl;
}

void mm2c_cigplan_destroy(mm2c_cigplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_cigplan_second_run_device(mm2c_cigplan_t *pl, const mm2c_cig_opt_t *opt, const mm2c_ksw_score_t *sc, int64_t n_regs, const mm2c_aln_reg_t *d_aln_regs,
                                   const mm2c_aln_item_t *d_items, const mm2c_ksw_task_t *d_tasks, const mm2c_zdrop_res_t *d_zres, const uint8_t *d_seq,
                                   mm2c_ksw_task_t *d_tasks2, int64_t *d_cig_off2, int32_t *d_second_of, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (const int rc = check_opt(opt)) return rc;
	if (!sc) return fail(MM2C_E_ARG, "score set is NULL");
	if (n_regs < 0 || n_regs > pl->n_regs_cap) return fail(MM2C_E_ARG, "%lld regions in a plan for %lld", (long long)n_regs, (long long)pl->n_regs_cap);
	if (!d_cig_off2) return fail(MM2C_E_ARG, "device pointer is NULL");
	if (n_regs > 0 && (!d_aln_regs || (pl->items_cap > 0 && (!d_items || !d_second_of)) || (pl->tasks_cap > 0 && (!d_tasks || !d_zres)) || (pl->tasks2_cap > 0 && !d_tasks2) ||
	                   ((opt->flag & MM2C_ALN_F_SR) && pl->pool_cap > 0 && !d_seq)))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_aln_regs | (uintptr_t)d_tasks | (uintptr_t)d_tasks2 | (uintptr_t)d_cig_off2) & 7) return fail(MM2C_E_ARG, "regions, tasks or offsets are not 8-byte aligned");
	if (((uintptr_t)d_items | (uintptr_t)d_zres | (uintptr_t)d_second_of) & 3) return fail(MM2C_E_ARG, "items, z-drop records or the map are not 4-byte aligned");
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, pl->d_second, 64)) return rc;
	mm2c::CigArgs X = {};
	fill(X, pl, opt, n_regs);
	for (int i = 0; i < 25; ++i) X.mat[i] = sc->mat[i];
	X.aregs = (const mm2c::AlnReg *)d_aln_regs; X.items = (const mm2c::AlnItem *)d_items; X.tasks = (const mm2c::KswTask *)d_tasks; X.zres = (const mm2c::ZdropRes *)d_zres; X.seq = d_seq;
	X.tasks2 = (mm2c::KswTask *)d_tasks2; X.cig_off2 = d_cig_off2; X.second_of = d_second_of;
	X.flags = (int32_t *)pl->d_second; X.totals = (int64_t *)(pl->d_second + 16);
	if (n_regs == 0) HIP_TRY(hipMemsetAsync(d_cig_off2, 0, 8, st));                        // no kernel runs: the list of 0 tasks still ends at cig_off2[0] = 0
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_cig_second_count(X, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	HIP_TRY(mm2c::launch_cig_second_emit(X, st));
	HIP_TRY(hipEventRecord(pl->ev[2], st));
	pl->did[0] = true;
	return pl->end(n_regs > 0 ? 3 : 0);
}

int mm2c_cigplan_second_check(mm2c_cigplan_t *pl, int64_t *n_refused, int64_t *n_over_cap, int64_t totals[2])
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_over_cap) *n_over_cap = 0;
	if (totals) totals[0] = totals[1] = 0;
	if (!pl->did[0]) return 0;
	int64_t w[4] = {};
	if (const int rc = pl->read_flags(2, pl->d_second, w, sizeof w)) return rc;
	int32_t fl[4];
	memcpy(fl, w, sizeof fl);
	if (n_refused) *n_refused = fl[0];
	if (n_over_cap) *n_over_cap = fl[2];
	if (totals) { totals[0] = w[2]; totals[1] = w[3]; }
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d region(s) or ungapped item(s) refused: offsets leaving a capacity", fl[0]);
	if (fl[2] != 0) return fail(MM2C_E_TOOBIG, "%d region(s) leave a capacity of the second list (the batch takes %lld tasks, %lld CIGAR words)", fl[2], (long long)w[2], (long long)w[3]);
	return 0;
}

int mm2c_cigplan_run_device(mm2c_cigplan_t *pl, const mm2c_cig_opt_t *opt, int64_t n_reads, int64_t n_regs, const int64_t *d_u_off, const mm2c_reg_t *d_regs,
                            const int64_t *d_b_off, const int64_t *d_n_b, const void *d_b, const int64_t *d_read_off, const mm2c_aln_reg_t *d_aln_regs,
                            const mm2c_aln_item_t *d_items, const int64_t *d_cig_off, const mm2c_ksw_res_t *d_res, const uint32_t *d_cigar, const mm2c_zdrop_res_t *d_zres,
                            const int32_t *d_second_of, const int64_t *d_cig_off2, const mm2c_ksw_res_t *d_res2, const uint32_t *d_cigar2, mm2c_cig_reg_t *d_cig_regs,
                            uint32_t *d_cig_out, int64_t *d_in_off, mm2c_extra_task_t *d_extra_tasks, int32_t *d_extra_reg, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (const int rc = check_opt(opt)) return rc;
	if (n_reads < 0 || n_regs < 0 || n_regs > pl->n_regs_cap) return fail(MM2C_E_ARG, "%lld regions in a plan for %lld", (long long)n_regs, (long long)pl->n_regs_cap);
	if (!d_in_off) return fail(MM2C_E_ARG, "device pointer is NULL");
	if (n_regs > 0 && (n_reads == 0 || !d_u_off || !d_regs || !d_b_off || !d_read_off || !d_aln_regs || !d_cig_regs || (pl->b_cap > 0 && !d_b) ||
	                   (pl->items_cap > 0 && (!d_items || !d_second_of)) || (pl->tasks_cap > 0 && (!d_cig_off || !d_res || !d_zres)) || (pl->cig_cap > 0 && !d_cigar) ||
	                   (pl->tasks2_cap > 0 && (!d_cig_off2 || !d_res2)) || (pl->cig2_cap > 0 && !d_cigar2) || (pl->words_cap > 0 && !d_cig_out) ||
	                   (pl->extra_cap > 0 && (!d_extra_tasks || !d_extra_reg))))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_u_off | (uintptr_t)d_regs | (uintptr_t)d_b_off | (uintptr_t)d_n_b | (uintptr_t)d_read_off | (uintptr_t)d_aln_regs | (uintptr_t)d_cig_off | (uintptr_t)d_cig_off2 |
	     (uintptr_t)d_cig_regs | (uintptr_t)d_in_off | (uintptr_t)d_extra_tasks) & 7)
		return fail(MM2C_E_ARG, "offsets, regions or tasks are not 8-byte aligned");
	if ((uintptr_t)d_b & 15) return fail(MM2C_E_ARG, "anchors are not 16-byte aligned");
	if (((uintptr_t)d_items | (uintptr_t)d_res | (uintptr_t)d_cigar | (uintptr_t)d_zres | (uintptr_t)d_second_of | (uintptr_t)d_res2 | (uintptr_t)d_cigar2 | (uintptr_t)d_cig_out |
	     (uintptr_t)d_extra_reg) & 3)
		return fail(MM2C_E_ARG, "items, results or CIGARs are not 4-byte aligned");
	if (pl->words_cap > 0 && (ranges_overlap(d_cigar, pl->cig_cap * 4, d_cig_out, pl->words_cap * 4) || ranges_overlap(d_cigar2, pl->cig2_cap * 4, d_cig_out, pl->words_cap * 4)))
		return fail(MM2C_E_ARG, "the input and output CIGAR buffers overlap");
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, pl->d_join, 64)) return rc;
	mm2c::CigArgs X = {};
	fill(X, pl, opt, n_regs);
	X.n_reads = n_reads; X.u_off = d_u_off; X.regs = (const mm2c::AlnRegIn *)d_regs; X.b_off = d_b_off; X.n_b = d_n_b; X.b = (const ulonglong2 *)d_b; X.read_off = d_read_off;
	X.aregs = (const mm2c::AlnReg *)d_aln_regs; X.items = (const mm2c::AlnItem *)d_items; X.cig_off = d_cig_off; X.res = (const mm2c::KswRes *)d_res; X.cigar = d_cigar;
	X.zres = (const mm2c::ZdropRes *)d_zres; X.second_of = (int32_t *)d_second_of; X.cig_off2 = (int64_t *)d_cig_off2; X.res2 = (const mm2c::KswRes *)d_res2; X.cigar2 = d_cigar2;
	X.cregs = (mm2c::CigReg *)d_cig_regs; X.cig_out = d_cig_out; X.in_off = d_in_off; X.extra = (mm2c::ExtraTask *)d_extra_tasks; X.extra_reg = d_extra_reg;
	X.flags = (int32_t *)pl->d_join; X.totals = (int64_t *)(pl->d_join + 16);
	if (n_regs == 0) HIP_TRY(hipMemsetAsync(d_in_off, 0, 8, st));                          // no kernel runs: the list of 0 CIGARs still ends at in_off[0] = 0
	HIP_TRY(hipEventRecord(pl->ev[3], st));
	HIP_TRY(mm2c::launch_cig_cut(X, st));
	HIP_TRY(hipEventRecord(pl->ev[4], st));
	HIP_TRY(mm2c::launch_cig_scan(X, st));
	HIP_TRY(hipEventRecord(pl->ev[5], st));
	HIP_TRY(mm2c::launch_cig_gather(X, st));
	HIP_TRY(hipEventRecord(pl->ev[6], st));
	pl->did[1] = true;
	return pl->end(n_regs > 0 ? 3 : 0);
}

int mm2c_cigplan_check(mm2c_cigplan_t *pl, int64_t *n_refused, int64_t *n_incomplete, int64_t *n_over_cap, int64_t totals[2])
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_incomplete) *n_incomplete = 0;
	if (n_over_cap) *n_over_cap = 0;
	if (totals) totals[0] = totals[1] = 0;
	if (!pl->did[1]) return 0;
	int64_t w[4] = {};
	if (const int rc = pl->read_flags(6, pl->d_join, w, sizeof w)) return rc;
	int32_t fl[4];
	memcpy(fl, w, sizeof fl);
	if (n_refused) *n_refused = fl[0];
	if (n_incomplete) *n_incomplete = fl[1];
	if (n_over_cap) *n_over_cap = fl[2];
	if (totals) { totals[0] = w[2]; totals[1] = w[3]; }
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d region(s) refused: a region the alignment-task plan did not finish, a z-drop code outside 0 .. 2 or a z-drop record that was refused on a "
	                                        "consumed task, offsets leaving a capacity, a CIGAR whose lengths do not add up to the region, or a region leaving its read or its target span", fl[0]);
	if (fl[1] != 0 || fl[2] != 0) return fail(MM2C_E_TOOBIG, "%d region(s) consume a task that was not run, was cut or has no second pass; %d region(s) leave a capacity (the batch takes "
	                                                         "%lld CIGAR words, %lld extra tasks)", fl[1], fl[2], (long long)w[2], (long long)w[3]);
	return 0;
}

int mm2c_cigplan_last_kernel_ms(mm2c_cigplan_t *pl, float ms[5])
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->did[0] && !pl->did[1]) return fail(MM2C_E_ARG, "plan has not been run");
	for (int i = 0; i < 5; ++i) ms[i] = 0.f;
	if (pl->did[0]) if (const int rc = pl->elapsed(2, {{0, 1, ms}, {1, 2, ms + 1}})) return rc;
	if (pl->did[1]) if (const int rc = pl->elapsed(6, {{3, 4, ms + 2}, {4, 5, ms + 3}, {5, 6, ms + 4}})) return rc;
	return 0;
}

int mm2c_second_pass_batch_host(const mm2c_cig_opt_t *opt, const mm2c_ksw_score_t *sc, int64_t n_regs, const mm2c_aln_reg_t *aln_regs, int64_t n_items,
                                const mm2c_aln_item_t *items, int64_t n_tasks, const mm2c_ksw_task_t *tasks, const mm2c_zdrop_res_t *zres, int64_t pool_len, const uint8_t *pool,
                                int64_t n_tasks2_cap, mm2c_ksw_task_t *tasks2, int64_t *cig_off2, int32_t *second_of, int64_t totals[2])
{
	if (const int rc = check_opt(opt)) return rc;
	if (!sc) return fail(MM2C_E_ARG, "score set is NULL");
	if (n_regs < 0 || n_regs > INT32_MAX || n_items < 0 || n_tasks < 0 || n_tasks > INT32_MAX || pool_len < 0 || n_tasks2_cap < 0 || n_tasks2_cap > INT32_MAX) return fail(MM2C_E_ARG, "bad argument");
	if (!cig_off2) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (totals) totals[0] = totals[1] = 0;
	if (n_regs == 0) { cig_off2[0] = 0; return 0; }
	if (!aln_regs || (n_items > 0 && (!items || !second_of)) || (n_tasks > 0 && (!tasks || !zres)) || (n_tasks2_cap > 0 && !tasks2) || (pool_len > 0 && !pool))
		return fail(MM2C_E_ARG, "host pointer is NULL");
	if (opt->flag & MM2C_ALN_F_SR) for (int64_t k = 0; k < pool_len; ++k) if (pool[k] > 4) return fail(MM2C_E_ARG, "base code %d at %lld", pool[k], (long long)k);
	if (!lib_ready()) return fail_not_ready();
	// the slots of the second list are those of the first list's tasks and of the ungapped items: no more words than the pool has bases, twice over
	int64_t cig2_cap = 0;
	for (int64_t i = 0; i < n_tasks; ++i) cig2_cap += std::max<int64_t>(0, (int64_t)tasks[i].qlen + tasks[i].tlen);
	if (opt->flag & MM2C_ALN_F_SR) for (int64_t i = 0; i < n_items; ++i) cig2_cap += std::max<int64_t>(0, ((int64_t)items[i].qe - items[i].qs) + ((int64_t)items[i].re - items[i].rs));
	mm2c_cigplan_t *pl = mm2c_cigplan_create(n_regs, n_items, n_tasks, 0, n_tasks2_cap, cig2_cap, pool_len, 0, 0, 0);
	if (!pl) return MM2C_E_HIP;
	Staging stage;
	const size_t nt2 = (size_t)n_tasks2_cap;
	const bool sr = (opt->flag & MM2C_ALN_F_SR) != 0;
	// tasks2, cig_off2 and second_of go up as well: what is not written stays the caller's
	const int i_ar = stage.add(aln_regs, nullptr, (size_t)n_regs * sizeof(mm2c_aln_reg_t)), i_it = stage.add(items, nullptr, (size_t)n_items * sizeof(mm2c_aln_item_t)),
	          i_tk = stage.add(tasks, nullptr, (size_t)n_tasks * sizeof(mm2c_ksw_task_t)), i_z = stage.add(zres, nullptr, (size_t)n_tasks * sizeof(mm2c_zdrop_res_t)),
	          i_p = stage.add(sr ? pool : nullptr, nullptr, sr ? (size_t)pool_len : 0, 16), i_t2 = stage.add(tasks2, tasks2, nt2 * sizeof(mm2c_ksw_task_t), 16),
	          i_c2 = stage.add(cig_off2, cig_off2, (nt2 + 1) * 8), i_so = stage.add(second_of, second_of, (size_t)n_items * 4, 16);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_cigplan_second_run_device(pl, opt, sc, n_regs, stage.at<mm2c_aln_reg_t>(i_ar), stage.at<mm2c_aln_item_t>(i_it), stage.at<mm2c_ksw_task_t>(i_tk), stage.at<mm2c_zdrop_res_t>(i_z),
		                                      stage.at<uint8_t>(i_p), stage.at<mm2c_ksw_task_t>(i_t2), stage.at<int64_t>(i_c2), stage.at<int32_t>(i_so), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_cigplan_second_check(pl, nullptr, nullptr, totals); });
	stage.release();
	mm2c_cigplan_destroy(pl);
	return rc;
}

int mm2c_assemble_regions_batch_host(const mm2c_cig_opt_t *opt, int64_t n_reads, const int64_t *u_off, const mm2c_reg_t *regs, const int64_t *b_off, const mm2c_anchor_t *b,
                                     const int64_t *read_off, const mm2c_aln_reg_t *aln_regs, int64_t n_items, const mm2c_aln_item_t *items, int64_t n_tasks, const int64_t *cig_off,
                                     const mm2c_ksw_res_t *res, const uint32_t *cigar, const mm2c_zdrop_res_t *zres, const int32_t *second_of, int64_t n_tasks2,
                                     const int64_t *cig_off2, const mm2c_ksw_res_t *res2, const uint32_t *cigar2, mm2c_cig_reg_t *cig_regs, int64_t words_cap, uint32_t *cig_out,
                                     int64_t n_extra_cap, int64_t *in_off, mm2c_extra_task_t *extra_tasks, int32_t *extra_reg, int64_t totals[2])
{
	if (const int rc = check_opt(opt)) return rc;
	if (n_reads < 0 || n_reads > INT32_MAX || n_items < 0 || n_tasks < 0 || n_tasks > INT32_MAX || n_tasks2 < 0 || n_tasks2 > INT32_MAX || words_cap < 0 || n_extra_cap < 0 ||
	    n_extra_cap > INT32_MAX)
		return fail(MM2C_E_ARG, "bad argument");
	if (!in_off) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (totals) totals[0] = totals[1] = 0;
	if (n_reads == 0) { in_off[0] = 0; return 0; }
	if (!u_off || !b_off || !read_off) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (u_off[0] != 0 || b_off[0] != 0 || read_off[0] != 0) return fail(MM2C_E_ARG, "u_off[0], b_off[0] and read_off[0] must be 0");
	for (int64_t r = 0; r < n_reads; ++r) {
		if (u_off[r + 1] < u_off[r] || b_off[r + 1] < b_off[r] || read_off[r + 1] < read_off[r]) return fail(MM2C_E_ARG, "offsets not monotone at read %lld", (long long)r);
		if (read_off[r + 1] - read_off[r] > INT32_MAX || b_off[r + 1] - b_off[r] > INT32_MAX) return fail(MM2C_E_ARG, "read %lld is too long", (long long)r);
	}
	const int64_t n_regs = u_off[n_reads], n_b = b_off[n_reads];
	if (n_regs > INT32_MAX) return fail(MM2C_E_ARG, "too many regions");
	if (n_regs == 0) { in_off[0] = 0; return 0; }
	if (!regs || !aln_regs || !cig_regs || (n_b > 0 && !b) || (n_items > 0 && (!items || !second_of)) || (n_tasks > 0 && (!cig_off || !res || !zres)) ||
	    (n_tasks2 > 0 && (!cig_off2 || !res2)) || (words_cap > 0 && !cig_out) || (n_extra_cap > 0 && (!extra_tasks || !extra_reg)))
		return fail(MM2C_E_ARG, "host pointer is NULL");
	int64_t n_cig = 0, n_cig2 = 0;
	if (n_tasks > 0) {
		if (cig_off[0] != 0) return fail(MM2C_E_ARG, "cig_off[0] must be 0");
		for (int64_t i = 0; i < n_tasks; ++i) if (cig_off[i + 1] < cig_off[i]) return fail(MM2C_E_ARG, "CIGAR offsets not monotone at task %lld", (long long)i);
		n_cig = cig_off[n_tasks];
	}
	if (n_tasks2 > 0) {
		if (cig_off2[0] != 0) return fail(MM2C_E_ARG, "cig_off2[0] must be 0");
		for (int64_t i = 0; i < n_tasks2; ++i) if (cig_off2[i + 1] < cig_off2[i]) return fail(MM2C_E_ARG, "CIGAR offsets not monotone at second-pass task %lld", (long long)i);
		n_cig2 = cig_off2[n_tasks2];
	}
	if ((n_cig > 0 && !cigar) || (n_cig2 > 0 && !cigar2)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (!lib_ready()) return fail_not_ready();
	mm2c_cigplan_t *pl = mm2c_cigplan_create(n_regs, n_items, n_tasks, n_cig, n_tasks2, n_cig2, 0, n_b, words_cap, n_extra_cap);
	if (!pl) return MM2C_E_HIP;
	Staging stage;
	const size_t nr = (size_t)n_reads, ng = (size_t)n_regs, nt = (size_t)n_tasks, nt2 = (size_t)n_tasks2, nx = (size_t)n_extra_cap;
	// every output goes up as well: what is not written stays the caller's
	const int i_u = stage.add(u_off, nullptr, (nr + 1) * 8), i_g = stage.add(regs, nullptr, ng * sizeof(mm2c_reg_t)), i_bo = stage.add(b_off, nullptr, (nr + 1) * 8),
	          i_b = stage.add(b, nullptr, (size_t)n_b * 16, 16), i_ro = stage.add(read_off, nullptr, (nr + 1) * 8), i_ar = stage.add(aln_regs, nullptr, ng * sizeof(mm2c_aln_reg_t)),
	          i_it = stage.add(items, nullptr, (size_t)n_items * sizeof(mm2c_aln_item_t)), i_co = stage.add(cig_off, nullptr, nt ? (nt + 1) * 8 : 0, 8),
	          i_rs = stage.add(res, nullptr, nt * sizeof(mm2c_ksw_res_t)), i_cg = stage.add(cigar, nullptr, (size_t)n_cig * 4, 16), i_z = stage.add(zres, nullptr, nt * sizeof(mm2c_zdrop_res_t)),
	          i_so = stage.add(second_of, nullptr, (size_t)n_items * 4), i_c2 = stage.add(cig_off2, nullptr, nt2 ? (nt2 + 1) * 8 : 0, 8), i_r2 = stage.add(res2, nullptr, nt2 * sizeof(mm2c_ksw_res_t)),
	          i_g2 = stage.add(cigar2, nullptr, (size_t)n_cig2 * 4, 16), i_cr = stage.add(cig_regs, cig_regs, ng * sizeof(mm2c_cig_reg_t)), i_o = stage.add(cig_out, cig_out, (size_t)words_cap * 4, 16),
	          i_io = stage.add(in_off, in_off, (nx + 1) * 8), i_x = stage.add(extra_tasks, extra_tasks, nx * sizeof(mm2c_extra_task_t), 16), i_xr = stage.add(extra_reg, extra_reg, nx * 4, 16);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_cigplan_run_device(pl, opt, n_reads, n_regs, stage.at<int64_t>(i_u), stage.at<mm2c_reg_t>(i_g), stage.at<int64_t>(i_bo), nullptr, stage.at<char>(i_b), stage.at<int64_t>(i_ro),
		                               stage.at<mm2c_aln_reg_t>(i_ar), stage.at<mm2c_aln_item_t>(i_it), stage.at<int64_t>(i_co), stage.at<mm2c_ksw_res_t>(i_rs), stage.at<uint32_t>(i_cg),
		                               stage.at<mm2c_zdrop_res_t>(i_z), stage.at<int32_t>(i_so), stage.at<int64_t>(i_c2), stage.at<mm2c_ksw_res_t>(i_r2), stage.at<uint32_t>(i_g2),
		                               stage.at<mm2c_cig_reg_t>(i_cr), stage.at<uint32_t>(i_o), stage.at<int64_t>(i_io), stage.at<mm2c_extra_task_t>(i_x), stage.at<int32_t>(i_xr),
		                               MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_cigplan_check(pl, nullptr, nullptr, nullptr, totals); });
	stage.release();
	mm2c_cigplan_destroy(pl);
	return rc;
}

} // extern "C"
