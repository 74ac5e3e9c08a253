// mm2chain_regs.cpp -- C-ABI entries of the chains-to-regions step (include/mm2chain.h): region plans (mm_gen_regs on the device, chain_regs.hip),
// the host-buffer entry built on them and the read hash of map.c:290-292.
#include "plan_common.h"
#include "chain_regs.h"

using namespace mm2c_api;

static_assert(sizeof(mm2c_reg_t) == 8 * mm2c::REG_WORDS, "mm2c_reg_t layout");
static_assert(offsetof(mm2c_reg_t, mlen) == 44 && offsetof(mm2c_reg_t, blen) == 48 && offsetof(mm2c_reg_t, flags) == 60 && offsetof(mm2c_reg_t, p) == 72, "mm2c_reg_t layout");

struct mm2c_regplan : PlanBase {           // d_mem: [flags | zkey | key0 | key1 | cstart | cend | val0 | val1 | crank | tiecnt | stack | moved]; events: begin, between the kernels, end
	int64_t n_reads = 0, n_u_cap = 0, n_b_cap = 0;
	mm2c::RegArgs R;
};

extern "C" {

mm2c_regplan_t *mm2c_regplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_b_cap)
{
	if (!lib_ready()) { fail_not_ready(); return nullptr; }
	if (n_reads < 0 || n_reads > INT32_MAX || n_u_cap < 0 || n_u_cap > INT32_MAX || n_b_cap < 0) { fail(MM2C_E_ARG, "bad argument"); return nullptr; }
	mm2c_regplan *pl = new mm2c_regplan();
	pl->n_reads = n_reads; pl->n_u_cap = n_u_cap; pl->n_b_cap = n_b_cap;
	const size_t nu = (size_t)std::max<int64_t>(n_u_cap, 1);
	Layout L;
	const size_t o_fl = L.take(16), o_z = L.take(nu * 8), o_k0 = L.take(nu * 8), o_k1 = L.take(nu * 8), o_cs = L.take(nu * 8), o_ce = L.take(nu * 8),
	             o_v0 = L.take(nu * 4), o_v1 = L.take(nu * 4), o_cr = L.take(nu * 4), o_tc = L.take(nu * 4), o_st = L.take(nu * 4 + 16), o_mv = L.take(nu * 4);
	const hipError_t e = pl->open(L.at, 3);
	if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_regplan_create: %s", hipGetErrorString(e)); mm2c_regplan_destroy(pl); return nullptr; }
	mm2c::RegArgs &R = pl->R;
	char *b = pl->d_mem;
	R.n_reads = n_reads; R.n_u_cap = n_u_cap; R.n_b_cap = n_b_cap;
	R.flags = (int32_t *)(b + o_fl); R.zkey = (uint64_t *)(b + o_z); R.key0 = (uint64_t *)(b + o_k0); R.key1 = (uint64_t *)(b + o_k1);
	R.cstart = (int64_t *)(b + o_cs); R.cend = (int64_t *)(b + o_ce); R.val0 = (int32_t *)(b + o_v0); R.val1 = (int32_t *)(b + o_v1);
	R.crank = (int32_t *)(b + o_cr); R.tiecnt = (int32_t *)(b + o_tc); R.stack = (int32_t *)(b + o_st); R.moved = (int32_t *)(b + o_mv);
	return pl;
}

void mm2c_regplan_destroy(mm2c_regplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_regplan_run_device(mm2c_regplan_t *pl, const int64_t *d_u_off, const uint64_t *d_u, const int64_t *d_b_off, const void *d_b,
                            const int32_t *d_qlen, const uint32_t *d_hash, mm2c_reg_t *d_regs, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (pl->n_reads == 0) return 0;
	if (!d_u_off || !d_b_off || !d_qlen || !d_hash || (pl->n_u_cap > 0 && (!d_u || !d_regs)) || (pl->n_b_cap > 0 && !d_b)) return fail(MM2C_E_ARG, "device pointer is NULL");
	if ((uintptr_t)d_regs & 7) return fail(MM2C_E_ARG, "d_regs is not 8-byte aligned");
	mm2c::RegArgs &R = pl->R;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, R.flags, 16)) return rc;
	R.u_off = d_u_off; R.u = d_u; R.b_off = d_b_off; R.b = (const ulonglong2 *)d_b; R.qlen = d_qlen; R.hash = d_hash; R.regs = (uint64_t *)d_regs;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	int nl = 0;
	HIP_TRY(mm2c::launch_chain_regs(R, st, pl->ev[1], &nl));
	HIP_TRY(hipEventRecord(pl->ev[2], st));
	return pl->end((uint64_t)nl);
}

int mm2c_regplan_check(mm2c_regplan_t *pl, int64_t *n_reads_with_ties)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_reads_with_ties) *n_reads_with_ties = 0;
	if (!pl->ran || pl->n_reads == 0) return 0;
	int32_t fl[2] = {0, 0};
	if (const int rc = pl->read_flags(2, pl->R.flags, fl, sizeof fl)) return rc;
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d read(s): a chain without anchors, counts that do not add up to the read's extent of b, or offsets beyond the plan's capacities", fl[0]);
	if (n_reads_with_ties) *n_reads_with_ties = fl[1];
	return 0;
}

int mm2c_regplan_last_ms(mm2c_regplan_t *pl, float *ms)
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(2, {{0, 2, ms}});
}

int mm2c_regplan_last_kernel_ms(mm2c_regplan_t *pl, float *sort_ms, float *fill_ms)
{
	if (!pl || !sort_ms || !fill_ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(2, {{0, 1, sort_ms}, {1, 2, fill_ms}});
}

int mm2c_gen_regs_batch_host(int64_t n_reads, const int64_t *u_off, const uint64_t *u, const int64_t *b_off, const mm2c_anchor_t *b,
                             const int32_t *qlen, const uint32_t *hash, mm2c_reg_t *regs)
{
	if (n_reads < 0 || n_reads > INT32_MAX) return fail(MM2C_E_ARG, "bad argument");
	if (n_reads == 0) return 0;
	if (!u_off || !b_off || !qlen || !hash) return fail(MM2C_E_ARG, "host pointer is NULL");
	const int64_t ub = u_off[0], bb = b_off[0];
	for (int64_t r = 0; r < n_reads; ++r) {
		if (u_off[r + 1] < u_off[r]) return fail(MM2C_E_ARG, "chain offsets not monotone at read %lld", (long long)r);
		if (b_off[r + 1] < b_off[r]) return fail(MM2C_E_ARG, "anchor offsets not monotone at read %lld", (long long)r);
	}
	const int64_t n_u = u_off[n_reads] - ub, n_b = b_off[n_reads] - bb;
	if (n_u > INT32_MAX) return fail(MM2C_E_TOOBIG, "%lld chains in one call", (long long)n_u);
	if ((n_u > 0 && (!u || !regs)) || (n_b > 0 && !b)) return fail(MM2C_E_ARG, "host pointer is NULL");
	for (int64_t r = 0; r < n_reads; ++r) {
		int64_t sum = 0;
		for (int64_t i = u_off[r]; i < u_off[r + 1]; ++i) {
			const int32_t cnt = (int32_t)u[i];
			if (cnt <= 0) return fail(MM2C_E_ARG, "read %lld: chain %lld has cnt %d", (long long)r, (long long)(i - u_off[r]), cnt);
			sum += cnt;
		}
		if (sum != b_off[r + 1] - b_off[r]) return fail(MM2C_E_ARG, "read %lld: its chains count %lld anchors, its extent of b holds %lld", (long long)r, (long long)sum, (long long)(b_off[r + 1] - b_off[r]));
	}
	if (!lib_ready()) return fail_not_ready();
	if (n_u == 0) return 0;
	std::vector<int64_t> off(2 * ((size_t)n_reads + 1));
	for (int64_t k = 0; k <= n_reads; ++k) { off[(size_t)k] = u_off[k] - ub; off[(size_t)(n_reads + 1 + k)] = b_off[k] - bb; }
	mm2c_regplan_t *pl = mm2c_regplan_create(n_reads, n_u, n_b);
	if (!pl) return MM2C_E_HIP;
	const size_t nr = (size_t)n_reads;
	Staging stage;
	const int i_off = stage.add(off.data(), nullptr, off.size() * 8), i_u = stage.add(u + ub, nullptr, (size_t)n_u * 8), i_b = stage.add(n_b > 0 ? b + bb : nullptr, nullptr, (size_t)n_b * 16),
	          i_q = stage.add(qlen, nullptr, nr * 4), i_h = stage.add(hash, nullptr, nr * 4), i_r = stage.add(nullptr, regs, (size_t)n_u * sizeof(mm2c_reg_t));
	const int rc = stage.through(pl->device, [&] {
		return mm2c_regplan_run_device(pl, stage.at<int64_t>(i_off), stage.at<uint64_t>(i_u), stage.at<int64_t>(i_off) + nr + 1, stage.at<char>(i_b), stage.at<int32_t>(i_q), stage.at<uint32_t>(i_h),
		                               stage.at<mm2c_reg_t>(i_r), MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_regplan_check(pl, nullptr); });
	stage.release();
	mm2c_regplan_destroy(pl);
	return rc;
}

static uint32_t wang_hash(uint32_t key)                                          // khash.h:400-409
{
	key += ~(key << 15);
	key ^=  (key >> 10);
	key +=  (key << 3);
	key ^=  (key >> 6);
	key += ~(key << 11);
	key ^=  (key >> 16);
	return key;
}

uint32_t mm2c_read_hash(const char *qname, int32_t qlen_sum, int32_t seed)
{
	uint32_t h = 0;
	if (qname) {                                                                 // khash.h:383-388; the reference's `char` is signed
		const signed char *s = (const signed char *)qname;
		h = (uint32_t)(int32_t)*s;
		if (h) for (++s; *s; ++s) h = (h << 5) - h + (uint32_t)(int32_t)*s;
	}
	h ^= wang_hash((uint32_t)qlen_sum) + wang_hash((uint32_t)seed);
	return wang_hash(h);
}

} // extern "C"
