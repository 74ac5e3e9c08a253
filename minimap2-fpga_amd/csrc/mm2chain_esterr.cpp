// mm2chain_esterr.cpp -- C-ABI entries of the chain-anchor divergence step (include/mm2chain.h): est-err plans (the counts of mm_est_err on the device,
// chain_esterr.hip), the one line of esterr.c:62 with the host's own pow, and the host-buffer entry built on them.
#include "plan_common.h"
#include "chain_esterr.h"
#include "chain_regs.h"
#include <cmath>
#include <cstddef>

using namespace mm2c_api;

static_assert(sizeof(mm2c_reg_t) == 8 * mm2c::REG_WORDS && sizeof(mm2c_err_t) == 8 && offsetof(mm2c_err_t, n_tot) == 4 && sizeof(mm2c_anchor_t) == 16, "layout");
static_assert(offsetof(mm2c_reg_t, div) == 68, "layout");

struct mm2c_errplan : PlanBase {           // d_mem: [flags | tab | first_fail | state]; events: in front of err_reads, behind it, behind err_walk, behind err_finish
	int64_t n_reads = 0, n_u_cap = 0, n_b_cap = 0, n_mini_cap = 0;
	mm2c::ErrArgs E;
};

extern "C" {

// esterr.c:62 with the pow of the host's own libm, the function the reference's esterr.o calls on this host.  The call goes through a volatile pointer so that
// no compiler stands a power of its own in for it.
float mm2c_est_err_div(int32_t n_match, int32_t n_tot, float avg_k)
{
	if (n_match <= 0) return -1.0f;
	if (n_match >= n_tot) return 0.0f;
	double (*volatile pw)(double, double) = ::pow;
	return (float)(1.0 - pw((double)n_match / n_tot, 1.0 / avg_k));
}

int mm2c_est_err_apply_host(int64_t n_reads, const int64_t *u_off, const int32_t *n_in, const mm2c_err_t *err, const float *avg_k, mm2c_reg_t *regs)
{
	if (n_reads < 0) return fail(MM2C_E_ARG, "bad argument");
	if (n_reads == 0) return 0;
	if (!u_off || !n_in || !avg_k) return fail(MM2C_E_ARG, "host pointer is NULL");
	for (int64_t r = 0; r < n_reads; ++r)
		if (n_in[r] < 0 || (n_in[r] > 0 && (!err || !regs))) return fail(MM2C_E_ARG, "read %lld: %d regions, or no arrays to hold them", (long long)r, n_in[r]);
	for (int64_t r = 0; r < n_reads; ++r)
		for (int64_t i = u_off[r]; i < u_off[r] + n_in[r]; ++i)
			if (err[i].n_match != -1) regs[i].div = mm2c_est_err_div(err[i].n_match, err[i].n_tot, avg_k[r]);   // -1: no mini_pos, esterr.c:36 leaves div alone
	return 0;
}

mm2c_errplan_t *mm2c_errplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_b_cap, int64_t n_mini_cap)
{
	if (!lib_ready()) { fail_not_ready(); return nullptr; }
	if (n_reads < 0 || n_reads > INT32_MAX || n_u_cap < 0 || n_u_cap > INT32_MAX || n_b_cap < 0 || n_mini_cap < 0) {
		fail(MM2C_E_ARG, "bad argument");
		return nullptr;
	}
	mm2c_errplan *pl = new mm2c_errplan();
	pl->n_reads = n_reads; pl->n_u_cap = n_u_cap; pl->n_b_cap = n_b_cap; pl->n_mini_cap = n_mini_cap;
	const size_t nu = (size_t)std::max<int64_t>(n_u_cap, 1), nr = (size_t)std::max<int64_t>(n_reads, 1);
	Layout L;
	const size_t o_fl = L.take(16), o_tab = L.take(nu * 16), o_ff = L.take(nu * 4), o_st = L.take(nr * 4);
	const hipError_t e = pl->open(L.at, 4);
	if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_errplan_create: %s", hipGetErrorString(e)); mm2c_errplan_destroy(pl); return nullptr; }
	mm2c::ErrArgs &E = pl->E;
	char *b = pl->d_mem;
	E.n_reads = n_reads; E.n_u_cap = n_u_cap; E.n_b_cap = n_b_cap; E.n_mini_cap = n_mini_cap;
	E.flags = (int32_t *)(b + o_fl); E.tab = (int4 *)(b + o_tab); E.first_fail = (int32_t *)(b + o_ff); E.state = (int32_t *)(b + o_st);
	return pl;
}

void mm2c_errplan_destroy(mm2c_errplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_errplan_run_device(mm2c_errplan_t *pl, const int64_t *d_u_off, const mm2c_reg_t *d_regs, const int32_t *d_n_in, const int64_t *d_b_off, const void *d_b,
                            const int64_t *d_mini_off, const uint64_t *d_mini_pos, const int32_t *d_qlen, int32_t n_ref, const uint32_t *d_ref_len,
                            mm2c_err_t *d_err, float *d_avg_k, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (n_ref < 0) return fail(MM2C_E_ARG, "n_ref is negative");
	if (pl->n_reads == 0) return 0;
	if (!d_u_off || !d_n_in || !d_b_off || !d_mini_off || !d_qlen || !d_avg_k || (pl->n_u_cap > 0 && (!d_regs || !d_err)) || (pl->n_b_cap > 0 && !d_b) ||
	    (pl->n_mini_cap > 0 && !d_mini_pos) || (n_ref > 0 && !d_ref_len))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_regs | (uintptr_t)d_err | (uintptr_t)d_mini_pos) & 7) return fail(MM2C_E_ARG, "regions, counts or mini_pos are not 8-byte aligned");
	if ((uintptr_t)d_b & 15) return fail(MM2C_E_ARG, "anchors are not 16-byte aligned");
	mm2c::ErrArgs &E = pl->E;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, E.flags, 16)) return rc;
	E.n_ref = n_ref; E.u_off = d_u_off; E.regs = (const uint64_t *)d_regs; E.n_in = d_n_in; E.b_off = d_b_off; E.b = (const uint4 *)d_b;
	E.mini_off = d_mini_off; E.mini_pos = d_mini_pos; E.qlen = d_qlen; E.ref_len = d_ref_len; E.err = (int2 *)d_err; E.avg_k = d_avg_k;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_err_reads(E, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	HIP_TRY(mm2c::launch_err_walk(E, st));
	HIP_TRY(hipEventRecord(pl->ev[2], st));
	HIP_TRY(mm2c::launch_err_finish(E, st));
	HIP_TRY(hipEventRecord(pl->ev[3], st));
	return pl->end(3);
}

int mm2c_errplan_check(mm2c_errplan_t *pl, int64_t *n_refused)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (!pl->ran || pl->n_reads == 0) return 0;
	int32_t fl[4] = {0, 0, 0, 0};
	if (const int rc = pl->read_flags(3, pl->E.flags, fl, sizeof fl)) return rc;
	if (n_refused) *n_refused = fl[0];
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d read(s): offsets beyond the plan's capacities or each other, mini_pos not strictly increasing, or a region "
	                                        "beyond the read's anchors or the reference sequences", fl[0]);
	return 0;
}

int mm2c_errplan_last_ms(mm2c_errplan_t *pl, float *ms)
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(3, {{0, 3, ms}});
}

int mm2c_errplan_last_kernel_ms(mm2c_errplan_t *pl, float *reads_ms, float *walk_ms, float *finish_ms)
{
	if (!pl || !reads_ms || !walk_ms || !finish_ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(3, {{0, 1, reads_ms}, {1, 2, walk_ms}, {2, 3, finish_ms}});
}

int mm2c_est_err_batch_host(int64_t n_reads, const int64_t *u_off, mm2c_reg_t *regs, const int32_t *n_in, const int64_t *b_off, const mm2c_anchor_t *b,
                            const int64_t *mini_off, const uint64_t *mini_pos, const int32_t *qlen, int32_t n_ref, const uint32_t *ref_len, mm2c_err_t *err,
                            float *avg_k)
{
	if (n_reads < 0 || n_reads > INT32_MAX || n_ref < 0) return fail(MM2C_E_ARG, "bad argument");
	if (n_reads == 0) return 0;
	if (!u_off || !n_in || !b_off || !mini_off || !qlen || (n_ref > 0 && !ref_len)) return fail(MM2C_E_ARG, "host pointer is NULL");
	const int64_t ub = u_off[0], bb = b_off[0], mb = mini_off[0];
	for (int64_t r = 0; r < n_reads; ++r) {
		if (u_off[r + 1] < u_off[r]) return fail(MM2C_E_ARG, "region offsets not monotone at read %lld", (long long)r);
		if (b_off[r + 1] < b_off[r]) return fail(MM2C_E_ARG, "anchor offsets not monotone at read %lld", (long long)r);
		if (mini_off[r + 1] < mini_off[r]) return fail(MM2C_E_ARG, "mini_pos offsets not monotone at read %lld", (long long)r);
		if (n_in[r] < 0 || n_in[r] > u_off[r + 1] - u_off[r]) return fail(MM2C_E_ARG, "read %lld: %d regions in room for %lld", (long long)r, n_in[r], (long long)(u_off[r + 1] - u_off[r]));
	}
	const int64_t n_u = u_off[n_reads] - ub, n_b = b_off[n_reads] - bb, n_m = mini_off[n_reads] - mb;
	if (n_u > INT32_MAX) return fail(MM2C_E_TOOBIG, "%lld regions in one call", (long long)n_u);
	if ((n_u > 0 && !regs) || (n_b > 0 && !b) || (n_m > 0 && !mini_pos)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (!lib_ready()) return fail_not_ready();
	const size_t nr = (size_t)n_reads;
	std::vector<int64_t> off(3 * (nr + 1));
	for (int64_t k = 0; k <= n_reads; ++k) { off[(size_t)k] = u_off[k] - ub; off[nr + 1 + (size_t)k] = b_off[k] - bb; off[2 * (nr + 1) + (size_t)k] = mini_off[k] - mb; }
	std::vector<mm2c_err_t> h_err((size_t)std::max<int64_t>(n_u, 1));
	std::vector<float> h_avg(nr);
	mm2c_errplan_t *pl = mm2c_errplan_create(n_reads, n_u, n_b, n_m);
	if (!pl) return MM2C_E_HIP;
	const size_t rb = (size_t)n_u * sizeof(mm2c_reg_t), ab = (size_t)n_b * 16, mbytes = (size_t)n_m * 8, fb = (size_t)n_ref * 4;
	Staging stage;
	const int i_off = stage.add(off.data(), nullptr, off.size() * 8), i_in = stage.add(n_u > 0 ? regs + ub : nullptr, nullptr, rb, 8), i_ni = stage.add(n_in, nullptr, nr * 4),
	          i_q = stage.add(qlen, nullptr, nr * 4), i_b = stage.add(n_b > 0 ? b + bb : nullptr, nullptr, ab, 16), i_m = stage.add(n_m > 0 ? mini_pos + mb : nullptr, nullptr, mbytes, 8),
	          i_ref = stage.add(ref_len, nullptr, fb, 4), i_err = stage.add(nullptr, h_err.data(), (size_t)n_u * 8, 8), i_avg = stage.add(nullptr, h_avg.data(), nr * 4);
	const int rc = stage.through(pl->device, [&] {
		const int64_t *d_off = stage.at<int64_t>(i_off);
		return mm2c_errplan_run_device(pl, d_off, stage.at<mm2c_reg_t>(i_in), stage.at<int32_t>(i_ni), d_off + nr + 1, stage.at<char>(i_b), d_off + 2 * (nr + 1), stage.at<uint64_t>(i_m),
		                               stage.at<int32_t>(i_q), n_ref, stage.at<uint32_t>(i_ref), stage.at<mm2c_err_t>(i_err), stage.at<float>(i_avg), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_errplan_check(pl, nullptr); });
	stage.release();
	mm2c_errplan_destroy(pl);
	if (rc) return rc;
	if (err && n_u > 0) memcpy(err, h_err.data(), (size_t)n_u * 8);
	if (avg_k) memcpy(avg_k, h_avg.data(), nr * 4);
	return mm2c_est_err_apply_host(n_reads, off.data(), n_in, h_err.data(), h_avg.data(), regs ? regs + ub : regs);
}

} // extern "C"
