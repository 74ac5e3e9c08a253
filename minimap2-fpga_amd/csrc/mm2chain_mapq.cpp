// mm2chain_mapq.cpp -- C-ABI entries of the hits-to-mapping-quality step (include/mm2chain.h): mapq plans (mm_join_long + mm_set_mapq on the device,
// chain_mapq.hip), the table of the host's own logf they look up, and the host-buffer entry built on them.
#include "plan_common.h"
#include "chain_mapq.h"
#include "chain_regs.h"
#include <cmath>
#include <mutex>

using namespace mm2c_api;

static_assert(sizeof(mm2c_reg_t) == 8 * mm2c::REG_WORDS && sizeof(mm2c_mapq_opt_t) == 28 && sizeof(mm2c_anchor_t) == 16, "layout");
static_assert(MM2C_HIT_LDS_REGIONS == mm2c::MAPQ_LDS_MAX && MM2C_MAPQ_MAX_LOG_ARG == (1 << 24) - 1, "constants of mm2chain.h");

struct mm2c_mapqplan : PlanBase {          // d_mem: [flags, counts | log table | moves | state | tab | junc]; events: in front of mapq_join, behind it, behind mapq_gather
	int64_t n_reads = 0, n_u_cap = 0, n_b_cap = 0;
	mm2c::MapqArgs M;
	bool gathered = false;
};

// L[i] = logf((float)i) by the host's own libm, the function the reference's hit.o calls on this host (hit.c:498, :501): made once, grown on demand.
// The call goes through a volatile pointer so that no compiler stands a logarithm of its own in for it.
static const float *host_log_table(int32_t max_log_arg)
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
	return tab.data();
}

extern "C" {

mm2c_mapqplan_t *mm2c_mapqplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_b_cap, int32_t max_log_arg)
{
	if (!lib_ready()) { fail_not_ready(); return nullptr; }
	if (n_reads < 0 || n_reads > INT32_MAX || n_u_cap < 0 || n_u_cap > INT32_MAX || n_b_cap < 0 || max_log_arg < 0 || max_log_arg > MM2C_MAPQ_MAX_LOG_ARG) {
		fail(MM2C_E_ARG, "bad argument");
		return nullptr;
	}
	mm2c_mapqplan *pl = new mm2c_mapqplan();
	pl->n_reads = n_reads; pl->n_u_cap = n_u_cap; pl->n_b_cap = n_b_cap;
	const size_t nu = (size_t)std::max<int64_t>(n_u_cap, 1), nr = (size_t)std::max<int64_t>(n_reads, 1), row = (size_t)(n_u_cap + n_reads) + 1;
	const size_t nl = (size_t)max_log_arg + 1;
	Layout L;
	const size_t o_fl = L.take(32), o_log = L.take(nl * 4), o_mv = L.take(nu * 16), o_st = L.take(nr * 4), o_tab = L.take(row * 4 * mm2c::MAPQ_TAB_ROWS),
	             o_j = L.take(nu * 8 * mm2c::MAPQ_JUNC_ROWS);
	hipError_t e = pl->open(L.at, 3);
	if (e == hipSuccess) e = pl->on_device([&] { return hipMemcpy(pl->d_mem + o_log, host_log_table(max_log_arg), nl * 4, hipMemcpyHostToDevice); });
	if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_mapqplan_create: %s", hipGetErrorString(e)); mm2c_mapqplan_destroy(pl); return nullptr; }
	mm2c::MapqArgs &M = pl->M;
	char *b = pl->d_mem;
	M.n_reads = n_reads; M.n_u_cap = n_u_cap; M.n_b_cap = n_b_cap; M.max_log_arg = max_log_arg;
	M.flags = (int32_t *)(b + o_fl); M.counts = (unsigned long long *)(b + o_fl + 8);
	M.logtab = (const float *)(b + o_log); M.moves = (int4 *)(b + o_mv); M.state = (int32_t *)(b + o_st); M.tab = (int32_t *)(b + o_tab);
	M.junc = (uint64_t *)(b + o_j);
	return pl;
}

void mm2c_mapqplan_destroy(mm2c_mapqplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_mapqplan_run_device(mm2c_mapqplan_t *pl, const mm2c_mapq_opt_t *opt, const int64_t *d_u_off, const mm2c_reg_t *d_regs_in, const int32_t *d_n_in,
                             const int64_t *d_b_off, const void *d_b, const int32_t *d_qlen, const int32_t *d_rep_len, mm2c_reg_t *d_regs_out,
                             int32_t *d_n_out, void *d_b_out, int64_t *d_n_b_out, void *stream)
{
	if (!pl || !opt) return fail(MM2C_E_ARG, "plan or options are NULL");
	if (!lib_ready()) return fail_not_ready();
	if (pl->n_reads == 0) return 0;
	if (!d_u_off || !d_n_in || !d_b_off || !d_qlen || !d_rep_len || !d_n_out || (pl->n_u_cap > 0 && (!d_regs_in || !d_regs_out)) || (pl->n_b_cap > 0 && !d_b))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if ((d_b_out != nullptr) != (d_n_b_out != nullptr)) return fail(MM2C_E_ARG, "d_b_out and d_n_b_out are given together or not at all");
	if (((uintptr_t)d_regs_in | (uintptr_t)d_regs_out) & 7) return fail(MM2C_E_ARG, "regions are not 8-byte aligned");
	if (((uintptr_t)d_b | (uintptr_t)d_b_out) & 15) return fail(MM2C_E_ARG, "anchors are not 16-byte aligned");
	if (pl->n_u_cap > 0 && (const mm2c_reg_t *)d_regs_out == d_regs_in) return fail(MM2C_E_ARG, "d_regs_out must not alias d_regs_in");
	if (d_b_out && d_b_out == d_b) return fail(MM2C_E_ARG, "d_b_out must not alias d_b");
	mm2c::MapqArgs &M = pl->M;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, M.flags, 32)) return rc;
	M.do_join = opt->do_join != 0; M.max_join_long = opt->max_join_long; M.max_join_short = opt->max_join_short; M.min_join_flank_sc = opt->min_join_flank_sc;
	M.min_join_flank_ratio = opt->min_join_flank_ratio; M.min_cnt = opt->min_cnt; M.min_chain_score = opt->min_chain_score;
	M.u_off = d_u_off; M.in = (const uint64_t *)d_regs_in; M.n_in = d_n_in; M.b_off = d_b_off; M.b = (const uint4 *)d_b; M.qlen = d_qlen; M.rep_len = d_rep_len;
	M.out = (uint64_t *)d_regs_out; M.n_out = d_n_out; M.b_out = (uint4 *)d_b_out; M.n_b_out = d_n_b_out;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_mapq_join(M, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	if (d_b_out) HIP_TRY(mm2c::launch_mapq_gather(M, st));
	HIP_TRY(hipEventRecord(pl->ev[2], st));
	pl->gathered = d_b_out != nullptr;
	return pl->end(d_b_out ? 2 : 1);
}

int mm2c_mapqplan_check(mm2c_mapqplan_t *pl, int64_t *n_joined, int64_t *n_beyond_table)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_joined) *n_joined = 0;
	if (n_beyond_table) *n_beyond_table = 0;
	if (!pl->ran || pl->n_reads == 0) return 0;
	int64_t fl[4] = {0, 0, 0, 0};
	if (const int rc = pl->read_flags(2, pl->M.flags, fl, sizeof fl)) return rc;
	if (n_joined) *n_joined = fl[1];
	if (n_beyond_table) *n_beyond_table = fl[2];
	if ((int32_t)fl[0] != 0) return fail(MM2C_E_ARG, "%d read(s): offsets beyond the plan's capacities or each other", (int32_t)fl[0]);
	if (fl[2] != 0) return fail(MM2C_E_TOOBIG, "%lld primary hit(s): score or n_sub + 1 beyond the plan's table of logarithms (max_log_arg %d); their mapq is 0",
	                            (long long)fl[2], pl->M.max_log_arg);
	return 0;
}

int mm2c_mapqplan_last_ms(mm2c_mapqplan_t *pl, float *ms)
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(2, {{0, 2, ms}});
}

int mm2c_mapqplan_last_kernel_ms(mm2c_mapqplan_t *pl, float *join_ms, float *gather_ms)
{
	if (!pl || !join_ms || !gather_ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	if (const int rc = pl->elapsed(2, {{0, 1, join_ms}})) return rc;
	*gather_ms = 0.0f;
	return pl->gathered ? pl->elapsed(2, {{1, 2, gather_ms}}) : 0;
}

int mm2c_join_mapq_batch_host(int64_t n_reads, const mm2c_mapq_opt_t *opt, int32_t max_log_arg, const int64_t *u_off, const mm2c_reg_t *regs_in,
                              const int32_t *n_in, const int64_t *b_off, const mm2c_anchor_t *b, const int32_t *qlen, const int32_t *rep_len,
                              mm2c_reg_t *regs_out, int32_t *n_out, mm2c_anchor_t *b_out, int64_t *n_b_out)
{
	if (n_reads < 0 || n_reads > INT32_MAX || !opt || max_log_arg < 0 || max_log_arg > MM2C_MAPQ_MAX_LOG_ARG) return fail(MM2C_E_ARG, "bad argument");
	if (n_reads == 0) return 0;
	if (!u_off || !n_in || !b_off || !qlen || !rep_len || !n_out) return fail(MM2C_E_ARG, "host pointer is NULL");
	if ((b_out != nullptr) != (n_b_out != nullptr)) return fail(MM2C_E_ARG, "b_out and n_b_out are given together or not at all");
	const int64_t ub = u_off[0], bb = b_off[0];
	for (int64_t r = 0; r < n_reads; ++r) {
		if (u_off[r + 1] < u_off[r]) return fail(MM2C_E_ARG, "region offsets not monotone at read %lld", (long long)r);
		if (b_off[r + 1] < b_off[r]) return fail(MM2C_E_ARG, "anchor offsets not monotone at read %lld", (long long)r);
		if (n_in[r] < 0 || n_in[r] > u_off[r + 1] - u_off[r]) return fail(MM2C_E_ARG, "read %lld: %d hits in room for %lld", (long long)r, n_in[r], (long long)(u_off[r + 1] - u_off[r]));
	}
	const int64_t n_u = u_off[n_reads] - ub, n_b = b_off[n_reads] - bb;
	if (n_u > INT32_MAX) return fail(MM2C_E_TOOBIG, "%lld regions in one call", (long long)n_u);
	if ((n_u > 0 && (!regs_in || !regs_out)) || (n_b > 0 && !b)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (!lib_ready()) return fail_not_ready();
	std::vector<int64_t> off(2 * ((size_t)n_reads + 1));
	for (int64_t k = 0; k <= n_reads; ++k) { off[(size_t)k] = u_off[k] - ub; off[(size_t)(n_reads + 1 + k)] = b_off[k] - bb; }
	mm2c_mapqplan_t *pl = mm2c_mapqplan_create(n_reads, n_u, n_b, max_log_arg);
	if (!pl) return MM2C_E_HIP;
	const size_t nr = (size_t)n_reads, rb = (size_t)n_u * sizeof(mm2c_reg_t), ab = (size_t)n_b * 16;
	Staging stage;
	const int i_off = stage.add(off.data(), nullptr, off.size() * 8), i_in = stage.add(n_u > 0 ? regs_in + ub : nullptr, nullptr, rb, 8), i_out = stage.add(nullptr, regs_out, rb, 8),
	          i_ni = stage.add(n_in, nullptr, nr * 4), i_no = stage.add(nullptr, n_out, nr * 4), i_q = stage.add(qlen, nullptr, nr * 4), i_rep = stage.add(rep_len, nullptr, nr * 4),
	          i_b = stage.add(n_b > 0 ? b + bb : nullptr, nullptr, ab, 16), i_bo = stage.add(nullptr, b_out, b_out ? ab : 0, 16), i_nb = stage.add(nullptr, n_b_out, nr * 8);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_mapqplan_run_device(pl, opt, stage.at<int64_t>(i_off), stage.at<mm2c_reg_t>(i_in), stage.at<int32_t>(i_ni), stage.at<int64_t>(i_off) + nr + 1, stage.at<char>(i_b), stage.at<int32_t>(i_q),
		                                stage.at<int32_t>(i_rep), stage.at<mm2c_reg_t>(i_out), stage.at<int32_t>(i_no), b_out ? stage.at<char>(i_bo) : nullptr,
		                                b_out ? stage.at<int64_t>(i_nb) : nullptr, MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_mapqplan_check(pl, nullptr, nullptr); });
	stage.release();
	mm2c_mapqplan_destroy(pl);
	return rc;
}

} // extern "C"
