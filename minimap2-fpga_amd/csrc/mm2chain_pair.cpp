// mm2chain_pair.cpp -- C-ABI entries of the pairing of a fragment's two ends (include/mm2chain.h): pair plans (pair_select: mm_pair with mm_set_pe_thru and the flip of
// map.c:455-466 on the device, pair_ends.hip), the table of the host's own logf they look up, and the host-buffer entry built on them.
#include "plan_common.h"
#include "pair_ends.h"
#include "chain_regs.h"
#include <cmath>
#include <mutex>

using namespace mm2c_api;

static_assert(sizeof(mm2c_pair_opt_t) == 24 && offsetof(mm2c_pair_opt_t, max_gap_ref) == 0 && offsetof(mm2c_pair_opt_t, pe_bonus) == 4 && offsetof(mm2c_pair_opt_t, sub_diff) == 8 &&
              offsetof(mm2c_pair_opt_t, match_sc) == 12 && offsetof(mm2c_pair_opt_t, pe_ori) == 16 && offsetof(mm2c_pair_opt_t, flip) == 20, "mm2c_pair_opt_t");
static_assert(MM2C_PAIR_LDS_REGIONS == mm2c::PAIR_LDS_MAX && MM2C_REG_PROPER_FRAG_BIT == 13 && MM2C_REG_PE_THRU_BIT == 14 && sizeof(mm2c_pext_t) == sizeof(mm2c::Pext), "constants of mm2chain.h");

// d_mem: [flags (4 x int32), counts (1 + PAIR_PROPER_SLOTS x uint64) | L | tab | zkey key0 key1 | val0 val1 tiecnt stack moved]; events: in front of and behind pair_select
constexpr size_t PAIR_FLAG_BYTES = 16 + 8 * (1 + mm2c::PAIR_PROPER_SLOTS);
struct mm2c_pairplan : PlanBase {
	int64_t n_frags = 0, n_u_cap = 0, n_pext_cap = 0;
	int32_t max_log_arg = 0;
	bool ran_select = false;
	mm2c::PairArgs F;
};

// L[i] = logf((float)i) by the host's own libm, the function the reference's pe.o calls on this host (pe.c:159): made once, grown on demand.  The call goes through
// a volatile pointer so that no compiler stands a logarithm of its own in for it.
static std::vector<float> pair_log_table(int32_t max_log_arg)
{
	static std::mutex mu;
	static std::vector<float> tab;
	std::lock_guard<std::mutex> hold(mu);
	if (tab.size() < (size_t)max_log_arg + 1) {
		float (*volatile lf)(float) = ::logf;
		const size_t from = tab.size();
		tab.resize((size_t)max_log_arg + 1);
		for (size_t i = from; i < tab.size(); ++i) tab[i] = lf((float)(int32_t)i);
	}
	return std::vector<float>(tab.begin(), tab.begin() + max_log_arg + 1);     // a copy: the table may grow under another thread
}

static int pair_opt_check(const mm2c_pair_opt_t *opt)
{
	if (!opt) return fail(MM2C_E_ARG, "options are NULL");
	if (opt->sub_diff < 0) return fail(MM2C_E_ARG, "sub_diff %d < 0", opt->sub_diff);
	if (opt->match_sc < 1) return fail(MM2C_E_ARG, "match_sc %d < 1", opt->match_sc);
	if (opt->pe_ori < 0 || opt->pe_ori > 3) return fail(MM2C_E_ARG, "pe_ori %d outside 0..3", opt->pe_ori);
	return 0;
}

// *code: what the failure was when the plan is NULL (the message is the one mm2c_last_error() returns)
static mm2c_pairplan_t *pairplan_new(int64_t n_frags, int64_t n_u_cap, int64_t n_pext_cap, int32_t max_log_arg, int *code)
{
	if (n_frags < 0 || n_frags > INT32_MAX / 2 || n_u_cap < 0 || n_u_cap > INT32_MAX - 1 || n_pext_cap < 0 || n_pext_cap > INT32_MAX || max_log_arg < 0 ||
	    max_log_arg > MM2C_MAPQ_MAX_LOG_ARG) {
		*code = fail(MM2C_E_ARG, "bad argument");
		return nullptr;
	}
	if (!lib_ready()) { *code = fail_not_ready(); return nullptr; }
	mm2c_pairplan *pl = new mm2c_pairplan();
	pl->n_frags = n_frags; pl->n_u_cap = n_u_cap; pl->n_pext_cap = n_pext_cap; pl->max_log_arg = max_log_arg;
	const size_t nu = (size_t)std::max<int64_t>(n_u_cap, 1), nl = (size_t)max_log_arg + 1;
	Layout L;
	const size_t o_fl = L.take(PAIR_FLAG_BYTES), o_log = L.take(nl * 4), o_tab = L.take(nu * 4 * mm2c::PAIR_TAB_ROWS), o_k = L.take(nu * 8 * 3), o_v = L.take(nu * 4 * 5);
	hipError_t e = pl->open(L.at, 2);
	if (e == hipSuccess) e = pl->on_device([&] {
		const std::vector<float> copy = pair_log_table(max_log_arg);
		return hipMemcpy(pl->d_mem + o_log, copy.data(), nl * 4, hipMemcpyHostToDevice);
	});
	if (e != hipSuccess) { *code = fail(MM2C_E_HIP, "mm2c_pairplan_create: %s", hipGetErrorString(e)); pl->close(); delete pl; return nullptr; }
	char *b = pl->d_mem;
	mm2c::PairArgs &F = pl->F;
	F.n_frags = n_frags; F.n_u_cap = n_u_cap; F.n_pext_cap = n_pext_cap; F.max_log_arg = max_log_arg;
	F.flags = (int32_t *)(b + o_fl); F.counts = (unsigned long long *)(b + o_fl + 16);
	F.logtab = (const float *)(b + o_log); F.tab = (int32_t *)(b + o_tab);
	F.zkey = (uint64_t *)(b + o_k); F.key0 = F.zkey + nu; F.key1 = F.key0 + nu;
	F.val0 = (int32_t *)(b + o_v); F.val1 = F.val0 + nu; F.tiecnt = F.val1 + nu; F.stack = F.tiecnt + nu; F.moved = F.stack + nu;
	return pl;
}

extern "C" {

mm2c_pairplan_t *mm2c_pairplan_create(int64_t n_frags, int64_t n_u_cap, int64_t n_pext_cap, int32_t max_log_arg)
{
	int code = 0;
	return pairplan_new(n_frags, n_u_cap, n_pext_cap, max_log_arg, &code);
}

void mm2c_pairplan_destroy(mm2c_pairplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_pairplan_run_device(mm2c_pairplan_t *pl, const mm2c_pair_opt_t *opt, const int64_t *d_f_off, mm2c_reg_t *d_regs, const int32_t *d_n, const mm2c_pext_t *d_pext,
                             const int32_t *d_seg_len, const int32_t *d_gap_ref, int32_t *d_status, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (const int rc = pair_opt_check(opt)) return rc;
	if (pl->n_frags > 0) {
		if (!d_f_off || !d_n || !d_seg_len || !d_status || (pl->n_u_cap > 0 && !d_regs) || (pl->n_pext_cap > 0 && !d_pext)) return fail(MM2C_E_ARG, "device pointer is NULL");
		if (((uintptr_t)d_regs | (uintptr_t)d_pext) & 7) return fail(MM2C_E_ARG, "regions are not 8-byte aligned");
	}
	if (!lib_ready()) return fail_not_ready();
	if (pl->n_frags == 0) return 0;
	mm2c::PairArgs &F = pl->F;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, F.flags, PAIR_FLAG_BYTES)) return rc;
	F.max_gap_ref = opt->max_gap_ref; F.pe_bonus = opt->pe_bonus; F.sub_diff = opt->sub_diff; F.match_sc = opt->match_sc; F.pe_ori = opt->pe_ori; F.flip = opt->flip != 0;
	F.f_off = d_f_off; F.n = d_n; F.seg_len = d_seg_len; F.gap_ref = d_gap_ref; F.regs = (uint64_t *)d_regs; F.pext = (const mm2c::Pext *)d_pext; F.status = d_status;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_pair_select(F, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	pl->ran_select = true;
	return pl->end(1);
}

int mm2c_pairplan_check(mm2c_pairplan_t *pl, int64_t *n_refused, int64_t *n_beyond_table, int64_t *n_proper)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_beyond_table) *n_beyond_table = 0;
	if (n_proper) *n_proper = 0;
	if (!pl->ran_select || pl->n_frags == 0) return 0;
	struct { int32_t fl[4]; int64_t counts[1 + mm2c::PAIR_PROPER_SLOTS]; } w = {};
	static_assert(sizeof w == PAIR_FLAG_BYTES, "flag words");
	if (const int rc = pl->read_flags(1, pl->F.flags, &w, sizeof w)) return rc;
	if (n_refused) *n_refused = w.fl[0];
	if (n_beyond_table) *n_beyond_table = w.counts[0];
	if (n_proper) for (int k = 1; k <= mm2c::PAIR_PROPER_SLOTS; ++k) *n_proper += w.counts[k];
	if (w.fl[0] != 0)
		return fail(MM2C_E_ARG, "%d fragment(s) refused, nothing of them written: offsets or counts beyond the capacities or each other, a p that is 0 or names no record, rid < 0, "
		                        "rs outside 0 .. 2^30 - 1, an id that is not the region's position, or a parent outside the mate", w.fl[0]);
	if (w.counts[0] != 0) return fail(MM2C_E_TOOBIG, "%lld fragment(s): n_sub beyond the plan's table of logarithms (max_log_arg %d); the pair's mapq is left as it came in",
	                                  (long long)w.counts[0], pl->max_log_arg);
	return 0;
}

int mm2c_pairplan_last_ms(mm2c_pairplan_t *pl, float *select_ms)
{
	if (!pl || !select_ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran_select) return fail(MM2C_E_ARG, "plan has not been run");
	*select_ms = 0.0f;
	if (pl->n_frags > 0) if (const int rc = pl->elapsed(1, {{0, 1, select_ms}})) return rc;
	return 0;
}

int mm2c_pair_ends_batch_host(int64_t n_frags, const mm2c_pair_opt_t *opt, int32_t max_log_arg, const int64_t *f_off, mm2c_reg_t *regs, const int32_t *n, int64_t n_pext,
                              const mm2c_pext_t *pext, const int32_t *seg_len, const int32_t *gap_ref, int32_t *status)
{
	if (n_frags < 0 || n_frags > INT32_MAX / 2 || n_pext < 0 || n_pext > INT32_MAX || max_log_arg < 0 || max_log_arg > MM2C_MAPQ_MAX_LOG_ARG) return fail(MM2C_E_ARG, "bad argument");
	if (const int rc = pair_opt_check(opt)) return rc;
	if (n_frags == 0) return 0;
	if (!f_off || !n || !seg_len || !status || (n_pext > 0 && !pext)) return fail(MM2C_E_ARG, "host pointer is NULL");
	const int64_t ub = f_off[0], nr = 2 * n_frags;
	for (int64_t r = 0; r < nr; ++r) {
		if (f_off[r + 1] < f_off[r]) return fail(MM2C_E_ARG, "region offsets not monotone at segment read %lld", (long long)r);
		if (n[r] < 0 || n[r] > f_off[r + 1] - f_off[r]) return fail(MM2C_E_ARG, "segment read %lld: %d regions in room for %lld", (long long)r, n[r], (long long)(f_off[r + 1] - f_off[r]));
	}
	const int64_t n_u = f_off[nr] - ub;
	if (n_u > INT32_MAX - 1) return fail(MM2C_E_TOOBIG, "%lld regions in one call", (long long)n_u);
	if (n_u > 0 && !regs) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (!lib_ready()) return fail_not_ready();
	std::vector<int64_t> off((size_t)nr + 1);
	for (int64_t k = 0; k <= nr; ++k) off[(size_t)k] = f_off[k] - ub;
	int code = 0;
	mm2c_pairplan_t *pl = pairplan_new(n_frags, n_u, n_pext, max_log_arg, &code);
	if (!pl) return code;
	const size_t rb = (size_t)n_u * sizeof(mm2c_reg_t);
	mm2c_reg_t *hr = n_u > 0 ? regs + ub : nullptr;
	Staging stage;
	const int i_off = stage.add(off.data(), nullptr, off.size() * 8), i_r = stage.add(hr, hr, rb, 8), i_n = stage.add(n, nullptr, (size_t)nr * 4),
	          i_p = stage.add(pext, nullptr, (size_t)n_pext * sizeof(mm2c_pext_t), 8), i_q = stage.add(seg_len, nullptr, (size_t)nr * 4),
	          i_g = stage.add(gap_ref, nullptr, gap_ref ? (size_t)n_frags * 4 : 0, 4), i_s = stage.add(status, status, (size_t)n_frags * 4);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_pairplan_run_device(pl, opt, stage.at<int64_t>(i_off), stage.at<mm2c_reg_t>(i_r), stage.at<int32_t>(i_n), stage.at<mm2c_pext_t>(i_p), stage.at<int32_t>(i_q),
		                                gap_ref ? stage.at<int32_t>(i_g) : nullptr, stage.at<int32_t>(i_s), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_pairplan_check(pl, nullptr, nullptr, nullptr); });
	stage.release();
	mm2c_pairplan_destroy(pl);
	return rc;
}

} // extern "C"
