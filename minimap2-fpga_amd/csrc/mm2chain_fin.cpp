// mm2chain_fin.cpp -- C-ABI entries of the last hit-level steps of a read mapped with base alignment (include/mm2chain.h): finish plans (fin_apply: what mm_align1
// leaves in a region, with mm_split_reg; fin_select: mm_filter_regs, mm_hit_sort, mm_set_parent, mm_select_sub, mm_set_sam_pri, mm_set_mapq on the device,
// align_finish.hip), the two tables of the host's own logf they look up, and the host-buffer entries built on them.
#include "plan_common.h"
#include "align_finish.h"
#include "chain_regs.h"
#include <cmath>
#include <map>
#include <mutex>

using namespace mm2c_api;

static_assert(sizeof(mm2c_reg_t) == 8 * mm2c::REG_WORDS && sizeof(mm2c_pext_t) == 32 && sizeof(mm2c_pext_t) == sizeof(mm2c::Pext) && sizeof(mm2c_fin_opt_t) == 56, "layout");
static_assert(offsetof(mm2c_pext_t, dp_score) == 0 && offsetof(mm2c_pext_t, dp_max) == 4 && offsetof(mm2c_pext_t, dp_max2) == 8 && offsetof(mm2c_pext_t, ambi_strand) == 12 &&
              offsetof(mm2c_pext_t, n_cigar) == 16 && offsetof(mm2c_pext_t, reserved) == 20 && offsetof(mm2c_pext_t, cig0) == 24, "mm2c_pext_t");
static_assert(offsetof(mm2c::Pext, dp_max) == 4 && offsetof(mm2c::Pext, dp_max2) == 8 && offsetof(mm2c::Pext, cig0) == 24, "Pext is mm2c_pext_t");
static_assert(sizeof(mm2c_cig_reg_t) == sizeof(mm2c::FinCigReg) && offsetof(mm2c_cig_reg_t, split_n) == offsetof(mm2c::FinCigReg, split_n) &&
              offsetof(mm2c_cig_reg_t, r_qe) == offsetof(mm2c::FinCigReg, r_qe) && offsetof(mm2c_cig_reg_t, cig0) == offsetof(mm2c::FinCigReg, cig0) &&
              sizeof(mm2c_extra_res_t) == sizeof(mm2c::FinExtraRes) && offsetof(mm2c_extra_res_t, status) == offsetof(mm2c::FinExtraRes, status), "records fin_apply reads");
static_assert(MM2C_FIN_LDS_REGIONS == mm2c::FIN_LDS_MAX && MM2C_FIN_REFUSED == mm2c::FIN_APPLY_REFUSED && MM2C_FIN_INCOMPLETE == mm2c::FIN_APPLY_INCOMPLETE &&
              MM2C_FIN_OVER_CAP == mm2c::FIN_APPLY_OVER_CAP, "constants of mm2chain.h");

// d_mem: [select flags (4 x int32), select counts (2 x uint64) | apply flags (4 x int32), n_child (int64) | slot | and, unless the plan was made for the apply entry alone, L | L2 | tab | pq | cov |
// zkey key0 key1 | val0 val1 tiecnt stack moved]; events: in front of and behind fin_apply's kernels, in front of and behind fin_select
struct mm2c_finplan : PlanBase {
	int64_t n_reads = 0, n_u_cap = 0, n_pext_cap = 0;
	int32_t max_log_arg = 0, match_sc = 0;
	int64_t n_child_cap = 0;
	bool ran_apply = false, ran_select = false;
	bool has_select = true;                // false: made for the apply entry alone (the host entry's plan): no tables, no select scratch
	mm2c::FinArgs F;
	mm2c::FinApplyArgs P;
};

// L[i] = logf((float)i) (match_sc 0) or logf((float)i / match_sc) by the host's own libm, the function the reference's hit.o calls on this host (hit.c:487, 496, 498,
// 501): made once per match_sc, grown on demand.  The call goes through a volatile pointer so that no compiler stands a logarithm of its own in for it.
static const float *host_log_table(int32_t match_sc, int32_t max_log_arg)
{
	static std::mutex mu;
	static std::map<int32_t, std::vector<float>> tabs;
	std::lock_guard<std::mutex> hold(mu);
	std::vector<float> &tab = tabs[match_sc];
	if (tab.size() < (size_t)max_log_arg + 1) {
		float (*volatile lf)(float) = ::logf;
		const size_t from = tab.size();
		tab.resize((size_t)max_log_arg + 1);
		for (size_t i = from; i < tab.size(); ++i) tab[i] = match_sc ? lf((float)(int32_t)i / (float)match_sc) : lf((float)(int32_t)i);
	}
	return tab.data();
}

static int fin_opt_check(const mm2c_fin_opt_t *opt)
{
	if (!opt) return fail(MM2C_E_ARG, "options are NULL");
	if (opt->min_dp_max < 1) return fail(MM2C_E_ARG, "min_dp_max %d < 1: a surviving dp_max must be positive (hit.c:487)", opt->min_dp_max);
	if (opt->match_sc < 1) return fail(MM2C_E_ARG, "match_sc %d < 1", opt->match_sc);
	return 0;
}

// select == false: a plan for the apply entry alone, whose device memory is the flag words and the slots
static mm2c_finplan_t *finplan_new(int64_t n_reads, int64_t n_u_cap, int64_t n_pext_cap, int32_t max_log_arg, int32_t match_sc, bool select)
{
	if (n_reads < 0 || n_reads > INT32_MAX || n_u_cap < 0 || n_u_cap > INT32_MAX - 1 || n_pext_cap < 0 || n_pext_cap > INT32_MAX || max_log_arg < 0 ||
	    max_log_arg > MM2C_MAPQ_MAX_LOG_ARG || match_sc < 1) {
		fail(MM2C_E_ARG, "bad argument");
		return nullptr;
	}
	if (!lib_ready()) { fail_not_ready(); return nullptr; }
	mm2c_finplan *pl = new mm2c_finplan();
	pl->n_reads = n_reads; pl->n_u_cap = n_u_cap; pl->n_pext_cap = n_pext_cap; pl->max_log_arg = max_log_arg; pl->match_sc = match_sc;
	const size_t nu = (size_t)std::max<int64_t>(n_u_cap, 1), row = (size_t)(n_u_cap + n_reads) + 1, nl = (size_t)max_log_arg + 1;
	Layout L;
	const size_t o_fl = L.take(64), o_slot = L.take((nu + 1) * 4), o_log = L.take(select ? nl * 4 : 0), o_log2 = L.take(select ? nl * 4 : 0),
	             o_tab = L.take(select ? row * 4 * mm2c::FIN_TAB_ROWS : 0), o_pq = L.take(select ? nu * 8 : 0), o_cov = L.take(select ? nu * 8 : 0),
	             o_k = L.take(select ? nu * 8 * 3 : 0), o_v = L.take(select ? nu * 4 * 5 : 0);
	pl->has_select = select;
	hipError_t e = pl->open(L.at, 4);
	if (e == hipSuccess && select) e = pl->on_device([&] {
		const hipError_t e1 = hipMemcpy(pl->d_mem + o_log, host_log_table(0, max_log_arg), nl * 4, hipMemcpyHostToDevice);
		return e1 != hipSuccess ? e1 : hipMemcpy(pl->d_mem + o_log2, host_log_table(match_sc, max_log_arg), nl * 4, hipMemcpyHostToDevice);
	});
	if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_finplan_create: %s", hipGetErrorString(e)); mm2c_finplan_destroy(pl); return nullptr; }
	char *b = pl->d_mem;
	mm2c::FinArgs &F = pl->F;
	F.n_reads = n_reads; F.n_u_cap = n_u_cap; F.n_pext_cap = n_pext_cap; F.max_log_arg = max_log_arg; F.match_sc = match_sc;
	F.flags = (int32_t *)(b + o_fl); F.counts = (unsigned long long *)(b + o_fl + 16);
	F.logtab = (const float *)(b + o_log); F.logtab2 = (const float *)(b + o_log2);
	F.tab = (int32_t *)(b + o_tab); F.pq = (int2 *)(b + o_pq); F.cov = (int2 *)(b + o_cov);
	F.zkey = (uint64_t *)(b + o_k); F.key0 = F.zkey + nu; F.key1 = F.key0 + nu;
	F.val0 = (int32_t *)(b + o_v); F.val1 = F.val0 + nu; F.tiecnt = F.val1 + nu; F.stack = F.tiecnt + nu; F.moved = F.stack + nu;
	mm2c::FinApplyArgs &P = pl->P;
	P.flags = (int32_t *)(b + o_fl + 32); P.n_child = nullptr; P.slot = (int32_t *)(b + o_slot);
	return pl;
}

extern "C" {

mm2c_finplan_t *mm2c_finplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_pext_cap, int32_t max_log_arg, int32_t match_sc)
{
	return finplan_new(n_reads, n_u_cap, n_pext_cap, max_log_arg, match_sc, true);
}

void mm2c_finplan_destroy(mm2c_finplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_finplan_apply_run_device(mm2c_finplan_t *pl, int64_t n_reads, int64_t n_regs, const int64_t *d_u_off, const mm2c_reg_t *d_regs, const int64_t *d_b_off,
                                  const void *d_b, int64_t n_b_cap, const int64_t *d_read_off, const mm2c_cig_reg_t *d_cig_regs, int64_t n_extra, const int32_t *d_extra_reg,
                                  const mm2c_extra_res_t *d_extra_res, const int64_t *d_out_off, mm2c_reg_t *d_regs_out, mm2c_pext_t *d_pext, int32_t *d_status,
                                  int64_t n_child_cap, mm2c_reg_t *d_child, int32_t *d_child_of, int64_t *d_n_child, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_reads < 0 || n_reads > pl->n_reads || n_regs < 0 || n_regs > pl->n_u_cap || n_regs > pl->n_pext_cap || n_b_cap < 0 || n_extra < 0 || n_extra > n_regs || n_child_cap < 0 ||
	    n_child_cap > INT32_MAX)
		return fail(MM2C_E_ARG, "counts outside the plan's capacities");
	if (!d_n_child) return fail(MM2C_E_ARG, "device pointer is NULL");
	if (n_regs > 0 && (!d_u_off || !d_regs || !d_b_off || !d_read_off || !d_cig_regs || !d_regs_out || !d_pext || !d_status || (n_b_cap > 0 && !d_b) ||
	                   (n_extra > 0 && (!d_extra_reg || !d_extra_res || !d_out_off)) || (n_child_cap > 0 && (!d_child || !d_child_of))))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_regs | (uintptr_t)d_regs_out | (uintptr_t)d_child | (uintptr_t)d_pext | (uintptr_t)d_cig_regs) & 7) return fail(MM2C_E_ARG, "regions are not 8-byte aligned");
	if ((uintptr_t)d_b & 15) return fail(MM2C_E_ARG, "anchors are not 16-byte aligned");
	if (n_regs > 0 && (const mm2c_reg_t *)d_regs_out == d_regs) return fail(MM2C_E_ARG, "d_regs_out must not alias d_regs");
	if (!lib_ready()) return fail_not_ready();
	mm2c::FinApplyArgs &P = pl->P;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, P.flags, 32)) return rc;
	P.n_reads = n_reads; P.n_regs = n_regs; P.n_b_cap = n_b_cap; P.n_extra = n_extra; P.n_child_cap = n_child_cap;
	P.u_off = d_u_off; P.b_off = d_b_off; P.read_off = d_read_off; P.regs = (const uint64_t *)d_regs; P.b = (const ulonglong2 *)d_b;
	P.cig_regs = (const mm2c::FinCigReg *)d_cig_regs; P.extra_reg = d_extra_reg; P.extra_res = (const mm2c::FinExtraRes *)d_extra_res; P.out_off = d_out_off;
	P.regs_out = (uint64_t *)d_regs_out; P.pext = (mm2c::Pext *)d_pext; P.status = d_status; P.child = (uint64_t *)d_child; P.child_of = d_child_of; P.n_child = d_n_child;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_fin_apply(P, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	pl->n_child_cap = n_child_cap;
	pl->ran_apply = true;
	return pl->end(n_regs > 0 ? 3 : 1);
}

int mm2c_finplan_apply_check(mm2c_finplan_t *pl, int64_t *n_refused, int64_t *n_incomplete, int64_t *n_child_beyond)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_incomplete) *n_incomplete = 0;
	if (n_child_beyond) *n_child_beyond = 0;
	if (!pl->ran_apply) return 0;
	int32_t fl[4] = {0, 0, 0, 0};
	if (const int rc = pl->read_flags(1, pl->P.flags, fl, sizeof fl)) return rc;
	if (n_refused) *n_refused = fl[0];
	if (n_incomplete) *n_incomplete = fl[1];
	if (n_child_beyond) *n_child_beyond = fl[2];
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d region(s) refused: a status that is not 0 in front, or offsets that leave the capacities; only their status is written", fl[0]);
	if (fl[1] != 0) return fail(MM2C_E_TOOBIG, "%d region(s) incomplete in front of this plan; only their status is written", fl[1]);
	if (fl[2] != 0) return fail(MM2C_E_TOOBIG, "%d split region(s) beyond n_child_cap %lld; their children are not written", fl[2], (long long)pl->n_child_cap);
	return 0;
}

int mm2c_finplan_run_device(mm2c_finplan_t *pl, const mm2c_fin_opt_t *opt, const int64_t *d_f_off, const mm2c_reg_t *d_regs_in, const int32_t *d_n_in, mm2c_pext_t *d_pext,
                            const int32_t *d_qlen, const int32_t *d_rep_len, mm2c_reg_t *d_regs_out, int32_t *d_n_out, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (const int rc = fin_opt_check(opt)) return rc;
	if (!pl->has_select) return fail(MM2C_E_ARG, "plan was made for the apply entry alone");
	if (opt->match_sc != pl->match_sc) return fail(MM2C_E_ARG, "match_sc %d is not the plan's %d", opt->match_sc, pl->match_sc);
	if (pl->n_reads > 0) {
		if (!d_f_off || !d_n_in || !d_qlen || !d_rep_len || !d_n_out || (pl->n_u_cap > 0 && (!d_regs_in || !d_regs_out)) || (pl->n_pext_cap > 0 && !d_pext))
			return fail(MM2C_E_ARG, "device pointer is NULL");
		if (((uintptr_t)d_regs_in | (uintptr_t)d_regs_out | (uintptr_t)d_pext) & 7) return fail(MM2C_E_ARG, "regions are not 8-byte aligned");
		if (pl->n_u_cap > 0 && (const mm2c_reg_t *)d_regs_out == d_regs_in) return fail(MM2C_E_ARG, "d_regs_out must not alias d_regs_in");
	}
	if (!lib_ready()) return fail_not_ready();
	if (pl->n_reads == 0) return 0;
	mm2c::FinArgs &F = pl->F;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, F.flags, 32)) return rc;
	F.min_cnt = opt->min_cnt; F.min_chain_score = opt->min_chain_score; F.min_dp_max = opt->min_dp_max; F.max_clip_ratio = opt->max_clip_ratio;
	F.mask_level = opt->mask_level; F.mask_len = opt->mask_len; F.hard_mask_level = opt->hard_mask_level; F.sub_diff = opt->sub_diff;
	F.pri_ratio = opt->pri_ratio; F.min_diff = opt->min_diff; F.best_n = opt->best_n; F.is_sr = opt->is_sr != 0; F.all_chains = opt->all_chains != 0;
	F.f_off = d_f_off; F.n_in = d_n_in; F.qlen = d_qlen; F.rep_len = d_rep_len; F.in = (const uint64_t *)d_regs_in; F.out = (uint64_t *)d_regs_out; F.n_out = d_n_out;
	F.pext = (mm2c::Pext *)d_pext;
	HIP_TRY(hipEventRecord(pl->ev[2], st));
	HIP_TRY(mm2c::launch_fin_select(F, st));
	HIP_TRY(hipEventRecord(pl->ev[3], st));
	pl->ran_select = true;
	return pl->end(1);
}

int mm2c_finplan_check(mm2c_finplan_t *pl, int64_t *n_refused, int64_t *n_beyond_table, int64_t *n_hits_total)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_beyond_table) *n_beyond_table = 0;
	if (n_hits_total) *n_hits_total = 0;
	if (!pl->ran_select || pl->n_reads == 0) return 0;
	struct { int32_t fl[4]; int64_t counts[2]; } w = {};
	if (const int rc = pl->read_flags(3, pl->F.flags, &w, sizeof w)) return rc;
	const int64_t refused = (int64_t)w.fl[0] + w.fl[1] + w.fl[2] + w.fl[3];
	if (n_refused) *n_refused = refused;
	if (n_beyond_table) *n_beyond_table = w.counts[1];
	if (n_hits_total) *n_hits_total = w.counts[0];
	if (refused != 0)
		return fail(MM2C_E_ARG, "%lld read(s) refused, nothing of them written: %d offsets beyond the capacities or each other, %d with inv or is_alt set, %d with a p that names no record, "
		                        "%d that mix kept regions with and without p (hit.c:210)", (long long)refused, w.fl[0], w.fl[1], w.fl[2], w.fl[3]);
	if (w.counts[1] != 0) return fail(MM2C_E_TOOBIG, "%lld primary hit(s): dp_max, score or n_sub + 1 beyond the plan's tables of logarithms (max_log_arg %d); their mapq is 0",
	                                  (long long)w.counts[1], pl->max_log_arg);
	return 0;
}

int mm2c_finplan_last_ms(mm2c_finplan_t *pl, float *apply_ms, float *select_ms)
{
	if (!pl || !apply_ms || !select_ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran_apply && !pl->ran_select) return fail(MM2C_E_ARG, "plan has not been run");
	*apply_ms = *select_ms = 0.0f;
	if (pl->ran_apply) if (const int rc = pl->elapsed(1, {{0, 1, apply_ms}})) return rc;
	if (pl->ran_select && pl->n_reads > 0) if (const int rc = pl->elapsed(3, {{2, 3, select_ms}})) return rc;
	return 0;
}

int mm2c_apply_regions_batch_host(int64_t n_reads, const int64_t *u_off, const mm2c_reg_t *regs, const int64_t *b_off, const mm2c_anchor_t *b, const int64_t *read_off,
                                  const mm2c_cig_reg_t *cig_regs, int64_t n_extra, const int32_t *extra_reg, const mm2c_extra_res_t *extra_res, const int64_t *out_off,
                                  mm2c_reg_t *regs_out, mm2c_pext_t *pext, int32_t *status, int64_t n_child_cap, mm2c_reg_t *child, int32_t *child_of, int64_t *n_child)
{
	if (n_reads < 0 || n_reads > INT32_MAX || n_extra < 0 || n_child_cap < 0 || n_child_cap > INT32_MAX || !n_child) return fail(MM2C_E_ARG, "bad argument");
	*n_child = 0;
	if (n_reads == 0) return 0;
	if (!u_off || !b_off || !read_off) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (u_off[0] != 0 || b_off[0] != 0) return fail(MM2C_E_ARG, "offsets must start at 0");
	for (int64_t r = 0; r < n_reads; ++r) {
		if (u_off[r + 1] < u_off[r]) return fail(MM2C_E_ARG, "region offsets not monotone at read %lld", (long long)r);
		if (b_off[r + 1] < b_off[r]) return fail(MM2C_E_ARG, "anchor offsets not monotone at read %lld", (long long)r);
		if (read_off[r + 1] < read_off[r] || read_off[r + 1] - read_off[r] > INT32_MAX) return fail(MM2C_E_ARG, "read offsets not monotone at read %lld", (long long)r);
	}
	const int64_t n_u = u_off[n_reads], n_b = b_off[n_reads];
	if (n_u > INT32_MAX - 1) return fail(MM2C_E_TOOBIG, "%lld regions in one call", (long long)n_u);
	if (n_extra > n_u) return fail(MM2C_E_ARG, "%lld extra entries for %lld regions", (long long)n_extra, (long long)n_u);
	if ((n_u > 0 && (!regs || !cig_regs || !regs_out || !pext || !status)) || (n_b > 0 && !b) || (n_extra > 0 && (!extra_reg || !extra_res || !out_off)) ||
	    (n_child_cap > 0 && (!child || !child_of)))
		return fail(MM2C_E_ARG, "host pointer is NULL");
	for (int64_t k = 0; k < n_extra; ++k)
		if (extra_reg[k] < 0 || extra_reg[k] >= n_u || (k > 0 && extra_reg[k] <= extra_reg[k - 1])) return fail(MM2C_E_ARG, "extra_reg does not ascend inside the regions at entry %lld", (long long)k);
	if (!lib_ready()) return fail_not_ready();
	mm2c_finplan_t *pl = finplan_new(n_reads, n_u, n_u, 0, 1, false);
	if (!pl) return MM2C_E_HIP;
	const size_t nr = (size_t)n_reads + 1, nu = (size_t)n_u, nx = (size_t)n_extra, nc = (size_t)n_child_cap;
	Staging stage;
	const int i_uo = stage.add(u_off, nullptr, nr * 8), i_bo = stage.add(b_off, nullptr, nr * 8), i_ro = stage.add(read_off, nullptr, nr * 8), i_r = stage.add(regs, nullptr, nu * 80, 8),
	          i_b = stage.add(b, nullptr, (size_t)n_b * 16, 16), i_c = stage.add(cig_regs, nullptr, nu * sizeof(mm2c_cig_reg_t), 8), i_xr = stage.add(extra_reg, nullptr, nx * 4, 4),
	          i_xe = stage.add(extra_res, nullptr, nx * sizeof(mm2c_extra_res_t), 8), i_oo = stage.add(out_off, nullptr, n_extra > 0 ? (nx + 1) * 8 : 0, 8),
	          i_ro2 = stage.add(regs_out, regs_out, nu * 80, 8), i_p = stage.add(pext, pext, nu * sizeof(mm2c_pext_t), 8), i_s = stage.add(nullptr, status, nu * 4, 4),
	          i_ch = stage.add(child, child, nc * 80, 8), i_co = stage.add(child_of, child_of, nc * 4, 4), i_nc = stage.add(nullptr, n_child, 8);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_finplan_apply_run_device(pl, n_reads, n_u, stage.at<int64_t>(i_uo), stage.at<mm2c_reg_t>(i_r), stage.at<int64_t>(i_bo), stage.at<char>(i_b), n_b, stage.at<int64_t>(i_ro),
		                                     stage.at<mm2c_cig_reg_t>(i_c), n_extra, stage.at<int32_t>(i_xr), stage.at<mm2c_extra_res_t>(i_xe), stage.at<int64_t>(i_oo),
		                                     stage.at<mm2c_reg_t>(i_ro2), stage.at<mm2c_pext_t>(i_p), stage.at<int32_t>(i_s), n_child_cap, stage.at<mm2c_reg_t>(i_ch),
		                                     stage.at<int32_t>(i_co), stage.at<int64_t>(i_nc), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_finplan_apply_check(pl, nullptr, nullptr, nullptr); });
	stage.release();
	mm2c_finplan_destroy(pl);
	return rc;
}

int mm2c_finish_regions_batch_host(int64_t n_reads, const mm2c_fin_opt_t *opt, int32_t max_log_arg, const int64_t *f_off, const mm2c_reg_t *regs_in, const int32_t *n_in,
                                   int64_t n_pext, mm2c_pext_t *pext, const int32_t *qlen, const int32_t *rep_len, mm2c_reg_t *regs_out, int32_t *n_out)
{
	if (n_reads < 0 || n_reads > INT32_MAX || n_pext < 0 || n_pext > INT32_MAX || max_log_arg < 0 || max_log_arg > MM2C_MAPQ_MAX_LOG_ARG) return fail(MM2C_E_ARG, "bad argument");
	if (const int rc = fin_opt_check(opt)) return rc;
	if (n_reads == 0) return 0;
	if (!f_off || !n_in || !qlen || !rep_len || !n_out || (n_pext > 0 && !pext)) return fail(MM2C_E_ARG, "host pointer is NULL");
	const int64_t ub = f_off[0];
	for (int64_t r = 0; r < n_reads; ++r) {
		if (f_off[r + 1] < f_off[r]) return fail(MM2C_E_ARG, "region offsets not monotone at read %lld", (long long)r);
		if (n_in[r] < 0 || n_in[r] > f_off[r + 1] - f_off[r]) return fail(MM2C_E_ARG, "read %lld: %d regions in room for %lld", (long long)r, n_in[r], (long long)(f_off[r + 1] - f_off[r]));
	}
	const int64_t n_u = f_off[n_reads] - ub;
	if (n_u > INT32_MAX - 1) return fail(MM2C_E_TOOBIG, "%lld regions in one call", (long long)n_u);
	if (n_u > 0 && (!regs_in || !regs_out)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (!lib_ready()) return fail_not_ready();
	std::vector<int64_t> off((size_t)n_reads + 1);
	for (int64_t k = 0; k <= n_reads; ++k) off[(size_t)k] = f_off[k] - ub;
	mm2c_finplan_t *pl = mm2c_finplan_create(n_reads, n_u, n_pext, max_log_arg, opt->match_sc);
	if (!pl) return MM2C_E_HIP;
	const size_t nr = (size_t)n_reads, rb = (size_t)n_u * sizeof(mm2c_reg_t);
	Staging stage;
	const int i_off = stage.add(off.data(), nullptr, off.size() * 8), i_in = stage.add(n_u > 0 ? regs_in + ub : nullptr, nullptr, rb, 8), i_out = stage.add(regs_out, regs_out, rb, 8),
	          i_ni = stage.add(n_in, nullptr, nr * 4), i_no = stage.add(n_out, n_out, nr * 4), i_q = stage.add(qlen, nullptr, nr * 4), i_rep = stage.add(rep_len, nullptr, nr * 4),
	          i_p = stage.add(pext, pext, (size_t)n_pext * sizeof(mm2c_pext_t), 8);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_finplan_run_device(pl, opt, stage.at<int64_t>(i_off), stage.at<mm2c_reg_t>(i_in), stage.at<int32_t>(i_ni), stage.at<mm2c_pext_t>(i_p), stage.at<int32_t>(i_q),
		                               stage.at<int32_t>(i_rep), stage.at<mm2c_reg_t>(i_out), stage.at<int32_t>(i_no), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_finplan_check(pl, nullptr, nullptr, nullptr); });
	stage.release();
	mm2c_finplan_destroy(pl);
	return rc;
}

} // extern "C"
