// mm2chain_hits.cpp -- C-ABI entries of the regions-to-hits step (include/mm2chain.h): hit plans (mm_set_parent + mm_select_sub, or mm_select_sub_multi for
// fragments of several segments, on the device, chain_hits.hip) and the host-buffer entries built on them.
#include "plan_common.h"
#include "chain_hits.h"
#include "chain_regs.h"

using namespace mm2c_api;

static_assert(sizeof(mm2c_reg_t) == 8 * mm2c::REG_WORDS && sizeof(mm2c_hit_opt_t) == 24 && sizeof(mm2c_hit_multi_opt_t) == 16, "layout");
static_assert(MM2C_HIT_LDS_REGIONS == mm2c::HITS_LDS_MAX && MM2C_REG_SAM_PRI_BIT == 12, "constants of mm2chain.h");

struct mm2c_hitplan : PlanBase {           // d_mem: [flags, total | tab | pq | cov]; events: begin, end
	int64_t n_reads = 0, n_u_cap = 0;
	mm2c::HitArgs H;
};

extern "C" {

mm2c_hitplan_t *mm2c_hitplan_create(int64_t n_reads, int64_t n_u_cap)
{
	if (!lib_ready()) { fail_not_ready(); return nullptr; }
	if (n_reads < 0 || n_reads > INT32_MAX || n_u_cap < 0 || n_u_cap > INT32_MAX) { fail(MM2C_E_ARG, "bad argument"); return nullptr; }
	mm2c_hitplan *pl = new mm2c_hitplan();
	pl->n_reads = n_reads; pl->n_u_cap = n_u_cap;
	const size_t nu = (size_t)std::max<int64_t>(n_u_cap, 1), row = (size_t)(n_u_cap + n_reads) + 1;
	Layout L;
	const size_t o_fl = L.take(16), o_tab = L.take(row * 4 * (mm2c::HITS_TAB_ROWS + 1)), o_pq = L.take(nu * 8), o_cov = L.take(nu * 8);
	const hipError_t e = pl->open(L.at, 2);
	if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_hitplan_create: %s", hipGetErrorString(e)); mm2c_hitplan_destroy(pl); return nullptr; }
	mm2c::HitArgs &H = pl->H;
	char *b = pl->d_mem;
	H.n_reads = n_reads; H.n_u_cap = n_u_cap;
	H.flags = (int32_t *)(b + o_fl); H.total = (unsigned long long *)(b + o_fl + 8);
	H.tab = (int32_t *)(b + o_tab); H.pq = (int2 *)(b + o_pq); H.cov = (int2 *)(b + o_cov);
	return pl;
}

void mm2c_hitplan_destroy(mm2c_hitplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

// both modes: mopt == NULL is mm_select_sub
static int hitplan_run(mm2c_hitplan_t *pl, const mm2c_hit_opt_t *opt, const mm2c_hit_multi_opt_t *mopt, const int64_t *d_u_off, const int32_t *d_seg_len,
                       const int32_t *d_gap_ref, const mm2c_reg_t *d_regs_in, mm2c_reg_t *d_regs_out, int32_t *d_n_out, void *stream)
{
	if (!pl || !opt) return fail(MM2C_E_ARG, "plan or options are NULL");
	if (!lib_ready()) return fail_not_ready();
	if (pl->n_reads == 0) return 0;
	if (!d_u_off || !d_n_out || (pl->n_u_cap > 0 && (!d_regs_in || !d_regs_out))) return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_regs_in | (uintptr_t)d_regs_out) & 7) return fail(MM2C_E_ARG, "regions are not 8-byte aligned");
	if (pl->n_u_cap > 0 && (const mm2c_reg_t *)d_regs_out == d_regs_in) return fail(MM2C_E_ARG, "d_regs_out must not alias d_regs_in");
	mm2c::HitArgs &H = pl->H;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, H.flags, 16)) return rc;
	H.mask_level = opt->mask_level; H.mask_len = opt->mask_len; H.hard_mask_level = opt->hard_mask_level;
	H.pri_ratio = opt->pri_ratio; H.min_diff = opt->min_diff; H.best_n = opt->best_n;
	H.pri1 = mopt ? mopt->pri1 : 0.0f; H.pri2 = mopt ? mopt->pri2 : 0.0f; H.n_segs = mopt ? mopt->n_segs : 1; H.max_gap_ref = mopt ? mopt->max_gap_ref : 0;
	H.seg_len = d_seg_len; H.gap_ref = d_gap_ref;
	H.u_off = d_u_off; H.in = (const uint64_t *)d_regs_in; H.out = (uint64_t *)d_regs_out; H.n_out = d_n_out;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mopt ? mm2c::launch_chain_hits_multi(H, st) : mm2c::launch_chain_hits(H, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	return pl->end(1);
}

int mm2c_hitplan_run_device(mm2c_hitplan_t *pl, const mm2c_hit_opt_t *opt, const int64_t *d_u_off, const mm2c_reg_t *d_regs_in,
                            mm2c_reg_t *d_regs_out, int32_t *d_n_out, void *stream)
{
	return hitplan_run(pl, opt, nullptr, d_u_off, nullptr, nullptr, d_regs_in, d_regs_out, d_n_out, stream);
}

int mm2c_hitplan_run_device_multi(mm2c_hitplan_t *pl, const mm2c_hit_opt_t *opt, const mm2c_hit_multi_opt_t *mopt, const int64_t *d_u_off, const int32_t *d_seg_len,
                                  const int32_t *d_gap_ref, const mm2c_reg_t *d_regs_in, mm2c_reg_t *d_regs_out, int32_t *d_n_out, void *stream)
{
	if (!mopt) return fail(MM2C_E_ARG, "multi options are NULL");
	if (mopt->n_segs < 1 || mopt->n_segs > MM2C_MAX_SEG) return fail(MM2C_E_ARG, "n_segs %d outside [1, %d]", mopt->n_segs, MM2C_MAX_SEG);
	if (pl && pl->n_reads > 0 && mopt->n_segs == 2 && !d_seg_len) return fail(MM2C_E_ARG, "device pointer is NULL");
	return hitplan_run(pl, opt, mopt, d_u_off, d_seg_len, d_gap_ref, d_regs_in, d_regs_out, d_n_out, stream);
}

int mm2c_hitplan_check(mm2c_hitplan_t *pl, int64_t *n_hits_total)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_hits_total) *n_hits_total = 0;
	if (!pl->ran || pl->n_reads == 0) return 0;
	int64_t fl[2] = {0, 0};
	if (const int rc = pl->read_flags(1, pl->H.flags, fl, sizeof fl)) return rc;
	if ((int32_t)fl[0] != 0) return fail(MM2C_E_ARG, "%d read(s): offsets beyond the plan's capacities", (int32_t)fl[0]);
	if (n_hits_total) *n_hits_total = fl[1];
	return 0;
}

int mm2c_hitplan_last_ms(mm2c_hitplan_t *pl, float *ms)
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(1, {{0, 1, ms}});
}

// both host entries: mopt == NULL is mm_select_sub
static int select_hits_host(int64_t n_reads, const mm2c_hit_opt_t *opt, const mm2c_hit_multi_opt_t *mopt, const int64_t *u_off, const int32_t *seg_len,
                            const int32_t *gap_ref, const mm2c_reg_t *regs_in, mm2c_reg_t *regs_out, int32_t *n_out)
{
	if (n_reads < 0 || n_reads > INT32_MAX || !opt) return fail(MM2C_E_ARG, "bad argument");
	if (mopt && (mopt->n_segs < 1 || mopt->n_segs > MM2C_MAX_SEG)) return fail(MM2C_E_ARG, "n_segs %d outside [1, %d]", mopt->n_segs, MM2C_MAX_SEG);
	if (n_reads == 0) return 0;
	if (!u_off || !n_out || (mopt && mopt->n_segs == 2 && !seg_len)) return fail(MM2C_E_ARG, "host pointer is NULL");
	const int64_t ub = u_off[0];
	for (int64_t r = 0; r < n_reads; ++r)
		if (u_off[r + 1] < u_off[r]) return fail(MM2C_E_ARG, "region offsets not monotone at read %lld", (long long)r);
	const int64_t n_u = u_off[n_reads] - ub;
	if (n_u > INT32_MAX) return fail(MM2C_E_TOOBIG, "%lld regions in one call", (long long)n_u);
	if (n_u > 0 && (!regs_in || !regs_out)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (!lib_ready()) return fail_not_ready();
	std::vector<int64_t> off((size_t)n_reads + 1);
	for (int64_t k = 0; k <= n_reads; ++k) off[(size_t)k] = u_off[k] - ub;
	mm2c_hitplan_t *pl = mm2c_hitplan_create(n_reads, n_u);
	if (!pl) return MM2C_E_HIP;
	const size_t nr = (size_t)n_reads, rb = (size_t)n_u * sizeof(mm2c_reg_t), sb = mopt && seg_len ? nr * (size_t)mopt->n_segs * 4 : 0, gb = mopt && gap_ref ? nr * 4 : 0;
	Staging stage;
	const int i_off = stage.add(off.data(), nullptr, off.size() * 8), i_in = stage.add(n_u > 0 ? regs_in + ub : nullptr, nullptr, rb, 8), i_out = stage.add(nullptr, regs_out, rb, 8),
	          i_n = stage.add(nullptr, n_out, nr * 4), i_sl = stage.add(seg_len, nullptr, sb, 4), i_gr = stage.add(gap_ref, nullptr, gb, 4);
	const int rc = stage.through(pl->device, [&] {
		return mopt ? mm2c_hitplan_run_device_multi(pl, opt, mopt, stage.at<int64_t>(i_off), sb ? stage.at<int32_t>(i_sl) : nullptr, gb ? stage.at<int32_t>(i_gr) : nullptr,
		                                            stage.at<mm2c_reg_t>(i_in), stage.at<mm2c_reg_t>(i_out), stage.at<int32_t>(i_n), MM2C_STREAM_LIBRARY)
		            : mm2c_hitplan_run_device(pl, opt, stage.at<int64_t>(i_off), stage.at<mm2c_reg_t>(i_in), stage.at<mm2c_reg_t>(i_out), stage.at<int32_t>(i_n), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_hitplan_check(pl, nullptr); });
	stage.release();
	mm2c_hitplan_destroy(pl);
	return rc;
}

int mm2c_select_hits_batch_host(int64_t n_reads, const mm2c_hit_opt_t *opt, const int64_t *u_off, const mm2c_reg_t *regs_in, mm2c_reg_t *regs_out, int32_t *n_out)
{
	return select_hits_host(n_reads, opt, nullptr, u_off, nullptr, nullptr, regs_in, regs_out, n_out);
}

int mm2c_select_hits_multi_batch_host(int64_t n_frags, const mm2c_hit_opt_t *opt, const mm2c_hit_multi_opt_t *mopt, const int64_t *u_off, const int32_t *seg_len,
                                      const int32_t *gap_ref, const mm2c_reg_t *regs_in, mm2c_reg_t *regs_out, int32_t *n_out)
{
	if (!mopt) return fail(MM2C_E_ARG, "bad argument");
	return select_hits_host(n_frags, opt, mopt, u_off, seg_len, gap_ref, regs_in, regs_out, n_out);
}

} // extern "C"
