// mm2chain_segs.cpp -- C-ABI entries of the fragment-hits-to-segments step (include/mm2chain.h): seg plans (mm_seg_gen on the device: chain_segs.hip for the
// per-segment chains and anchors, chain_regs.hip for their regions) and the host-buffer entry built on them.
#include "plan_common.h"
#include "chain_segs.h"
#include "chain_regs.h"
#include <cstddef>

using namespace mm2c_api;

static_assert(sizeof(mm2c_reg_t) == 8 * mm2c::REG_WORDS && sizeof(mm2c_anchor_t) == 16 && offsetof(mm2c_reg_t, flags) == 60, "layout");
static_assert(MM2C_MAX_SEG == mm2c::SEG_MAX && MM2C_REG_SEG_SPLIT_BIT == 15 && MM2C_REG_SEG_ID_SHIFT == 16, "constants of mm2chain.h");

struct mm2c_segplan : PlanBase {           // d_mem: [flags, the region step's flags | cnt_u | cnt_a | state | scan | the region step's scratch]
	int64_t n_frags = 0, n_u_cap = 0, n_b_cap = 0, n_su_cap = 0;   // events: begin, behind seg_count, the scans, seg_scatter, regs_sort, regs_fill, seg_mark
	int32_t n_segs = 0;
	size_t scan_bytes = 0;
	void *d_scan = nullptr;
	mm2c::SegArgs S;
	mm2c::RegArgs R;                       // chain_regs.hip over the segment reads
};

static int64_t seg_chain_cap(int64_t n_segs, int64_t n_u_cap, int64_t n_b_cap)   // a segment chain holds at least one anchor
{
	return std::min<int64_t>(n_segs * n_u_cap, n_b_cap);
}

extern "C" {

mm2c_segplan_t *mm2c_segplan_create(int64_t n_frags, int32_t n_segs, int64_t n_u_cap, int64_t n_b_cap)
{
	if (!lib_ready()) { fail_not_ready(); return nullptr; }
	if (n_frags < 0 || n_segs < 1 || n_segs > MM2C_MAX_SEG || n_frags * n_segs > INT32_MAX || n_u_cap < 0 || n_u_cap > INT32_MAX || n_b_cap < 0 ||
	    seg_chain_cap(n_segs, n_u_cap, n_b_cap) > INT32_MAX) {
		fail(MM2C_E_ARG, "bad argument");
		return nullptr;
	}
	mm2c_segplan *pl = new mm2c_segplan();
	pl->n_frags = n_frags; pl->n_segs = n_segs; pl->n_u_cap = n_u_cap; pl->n_b_cap = n_b_cap; pl->n_su_cap = seg_chain_cap(n_segs, n_u_cap, n_b_cap);
	const size_t n1 = (size_t)(n_frags * n_segs) + 1, nf = (size_t)std::max<int64_t>(n_frags, 1), nu = (size_t)std::max<int64_t>(pl->n_su_cap, 1);
	pl->scan_bytes = mm2c::seg_scan_bytes(n_frags * n_segs);
	Layout L;
	const size_t o_fl = L.take(48), o_cu = L.take(n1 * 8), o_ca = L.take(n1 * 8), o_st = L.take(nf * 4), o_sc = L.take(pl->scan_bytes + 16);
	const size_t o_z = L.take(nu * 8), o_k0 = L.take(nu * 8), o_k1 = L.take(nu * 8), o_cs = L.take(nu * 8), o_ce = L.take(nu * 8),
	             o_v0 = L.take(nu * 4), o_v1 = L.take(nu * 4), o_cr = L.take(nu * 4), o_tc = L.take(nu * 4), o_sk = L.take(nu * 4 + 16), o_mv = L.take(nu * 4);
	hipError_t e = pl->open(L.at, 7);
	if (e == hipSuccess) e = pl->on_device([&] { return hipMemset(pl->d_mem + o_cu, 0, o_st - o_cu); });   // the entry behind the last segment read stays 0
	if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_segplan_create: %s", hipGetErrorString(e)); mm2c_segplan_destroy(pl); return nullptr; }
	char *b = pl->d_mem;
	mm2c::SegArgs &S = pl->S;
	S.n_frags = n_frags; S.n_segs = n_segs; S.n_u_cap = n_u_cap; S.n_b_cap = n_b_cap; S.n_su_cap = pl->n_su_cap;
	S.flags = (int32_t *)(b + o_fl); S.cnt_u = (int64_t *)(b + o_cu); S.cnt_a = (int64_t *)(b + o_ca); S.state = (int32_t *)(b + o_st);
	pl->d_scan = b + o_sc;
	mm2c::RegArgs &R = pl->R;
	R.n_reads = n_frags * n_segs; R.n_u_cap = pl->n_su_cap; R.n_b_cap = n_b_cap;
	R.flags = (int32_t *)(b + o_fl) + 8; R.zkey = (uint64_t *)(b + o_z); R.key0 = (uint64_t *)(b + o_k0); R.key1 = (uint64_t *)(b + o_k1);
	R.cstart = (int64_t *)(b + o_cs); R.cend = (int64_t *)(b + o_ce); R.val0 = (int32_t *)(b + o_v0); R.val1 = (int32_t *)(b + o_v1);
	R.crank = (int32_t *)(b + o_cr); R.tiecnt = (int32_t *)(b + o_tc); R.stack = (int32_t *)(b + o_sk); R.moved = (int32_t *)(b + o_mv);
	return pl;
}

void mm2c_segplan_destroy(mm2c_segplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int64_t mm2c_segplan_seg_chain_cap(const mm2c_segplan_t *pl)
{
	return pl ? pl->n_su_cap : 0;
}

int mm2c_segplan_run_device(mm2c_segplan_t *pl, const int64_t *d_u_off, const mm2c_reg_t *d_regs, const int32_t *d_n_in, const int64_t *d_b_off, const void *d_b,
                            const int32_t *d_seg_len, const uint32_t *d_hash, const int32_t *d_rep_len, int64_t *d_su_off, uint64_t *d_su, int64_t *d_sb_off,
                            void *d_sb, mm2c_reg_t *d_seg_regs, uint32_t *d_seg_hash, int32_t *d_seg_rep_len, void *stream)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (pl->n_frags == 0) return 0;
	if (!d_u_off || !d_n_in || !d_b_off || !d_seg_len || !d_hash || !d_su_off || !d_sb_off || !d_seg_hash || (pl->n_u_cap > 0 && !d_regs) || (pl->n_b_cap > 0 && (!d_b || !d_sb)) ||
	    (pl->n_su_cap > 0 && (!d_su || !d_seg_regs)) || (d_rep_len && !d_seg_rep_len))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_regs | (uintptr_t)d_seg_regs | (uintptr_t)d_su) & 7) return fail(MM2C_E_ARG, "regions or chains are not 8-byte aligned");
	if (((uintptr_t)d_b | (uintptr_t)d_sb) & 15) return fail(MM2C_E_ARG, "anchors are not 16-byte aligned");
	if (pl->n_b_cap > 0 && d_sb == d_b) return fail(MM2C_E_ARG, "d_sb must not alias d_b");
	mm2c::SegArgs &S = pl->S;
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, S.flags, 48)) return rc;        // its own flags and the region step's
	S.u_off = d_u_off; S.regs = (const uint64_t *)d_regs; S.n_in = d_n_in; S.b_off = d_b_off; S.b = (const uint4 *)d_b; S.seg_len = d_seg_len; S.hash = d_hash;
	S.rep_len = d_rep_len; S.su_off = d_su_off; S.sb_off = d_sb_off; S.su = d_su; S.sb = (uint4 *)d_sb; S.seg_hash = d_seg_hash; S.seg_rep_len = d_seg_rep_len;
	mm2c::RegArgs &R = pl->R;
	R.u_off = d_su_off; R.u = d_su; R.b_off = d_sb_off; R.b = (const ulonglong2 *)d_sb; R.qlen = d_seg_len; R.hash = d_seg_hash; R.regs = (uint64_t *)d_seg_regs;
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_seg_count(S, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	HIP_TRY(mm2c::launch_seg_offsets(S, pl->d_scan, pl->scan_bytes, st));
	HIP_TRY(hipEventRecord(pl->ev[2], st));
	HIP_TRY(mm2c::launch_seg_scatter(S, st));
	HIP_TRY(hipEventRecord(pl->ev[3], st));
	int nl = 4;
	HIP_TRY(mm2c::launch_chain_regs(R, st, pl->ev[4], &nl));
	HIP_TRY(hipEventRecord(pl->ev[5], st));
	HIP_TRY(mm2c::launch_seg_mark(S, (uint64_t *)d_seg_regs, st));
	HIP_TRY(hipEventRecord(pl->ev[6], st));
	return pl->end((uint64_t)nl + 1);
}

int mm2c_segplan_check(mm2c_segplan_t *pl, int64_t *n_refused, int64_t *n_seg_chains, int64_t *n_seg_anchors)
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_seg_chains) *n_seg_chains = 0;
	if (n_seg_anchors) *n_seg_anchors = 0;
	if (!pl->ran || pl->n_frags == 0) return 0;
	int32_t fl[12] = {};
	if (const int rc = pl->read_flags(6, pl->S.flags, fl, sizeof fl)) return rc;
	int64_t tot[2];
	memcpy(tot, fl + 2, 16);
	if (n_refused) *n_refused = fl[0];
	if (n_seg_chains) *n_seg_chains = tot[0];
	if (n_seg_anchors) *n_seg_anchors = tot[1];
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d fragment(s): offsets or n_in beyond the plan's capacities or each other, a region beyond the fragment's anchors, or an "
	                                        "anchor of a segment beyond n_segs", fl[0]);
	if (fl[1] != 0 || fl[8] != 0) return fail(MM2C_E_ARG, "fragments that share anchors: %d store(s) beyond the plan's capacities were left out", fl[1]);
	return 0;
}

int mm2c_segplan_last_ms(mm2c_segplan_t *pl, float *ms)
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(6, {{0, 6, ms}});
}

int mm2c_segplan_last_kernel_ms(mm2c_segplan_t *pl, float *count_ms, float *offsets_ms, float *scatter_ms, float *regs_ms, float *mark_ms)
{
	if (!pl || !count_ms || !offsets_ms || !scatter_ms || !regs_ms || !mark_ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(6, {{0, 1, count_ms}, {1, 2, offsets_ms}, {2, 3, scatter_ms}, {3, 5, regs_ms}, {5, 6, mark_ms}});
}

int mm2c_seg_gen_batch_host(int64_t n_frags, int32_t n_segs, const int64_t *u_off, const mm2c_reg_t *regs, const int32_t *n_in, const int64_t *b_off,
                            const mm2c_anchor_t *b, const int32_t *seg_len, const uint32_t *hash, const int32_t *rep_len, int64_t *su_off, uint64_t *su,
                            int64_t *sb_off, mm2c_anchor_t *sb, mm2c_reg_t *seg_regs, uint32_t *seg_hash, int32_t *seg_rep_len)
{
	if (n_frags < 0 || n_segs < 1 || n_segs > MM2C_MAX_SEG || n_frags * n_segs > INT32_MAX) return fail(MM2C_E_ARG, "bad argument");
	if (n_frags == 0) return 0;
	if (!u_off || !n_in || !b_off || !seg_len || !hash || !su_off || !sb_off || !seg_hash || (rep_len && !seg_rep_len)) return fail(MM2C_E_ARG, "host pointer is NULL");
	const int64_t ub = u_off[0], bb = b_off[0];
	for (int64_t f = 0; f < n_frags; ++f) {
		if (u_off[f + 1] < u_off[f]) return fail(MM2C_E_ARG, "region offsets not monotone at fragment %lld", (long long)f);
		if (b_off[f + 1] < b_off[f]) return fail(MM2C_E_ARG, "anchor offsets not monotone at fragment %lld", (long long)f);
		if (n_in[f] < 0 || n_in[f] > u_off[f + 1] - u_off[f]) return fail(MM2C_E_ARG, "fragment %lld: %d regions in room for %lld", (long long)f, n_in[f], (long long)(u_off[f + 1] - u_off[f]));
	}
	const int64_t n_u = u_off[n_frags] - ub, n_b = b_off[n_frags] - bb, n_sr = n_frags * n_segs;
	if (n_u > INT32_MAX) return fail(MM2C_E_TOOBIG, "%lld regions in one call", (long long)n_u);
	const int64_t n_su = seg_chain_cap(n_segs, n_u, n_b);
	if (n_su > INT32_MAX) return fail(MM2C_E_TOOBIG, "%lld segment chains in one call", (long long)n_su);
	if ((n_u > 0 && !regs) || (n_b > 0 && (!b || !sb)) || (n_su > 0 && (!su || !seg_regs))) return fail(MM2C_E_ARG, "host pointer is NULL");
	for (int64_t f = 0; f < n_frags; ++f) {
		const int64_t bl = b_off[f + 1] - b_off[f];
		int64_t sum = 0;
		for (int64_t i = u_off[f]; i < u_off[f] + n_in[f]; ++i) {
			const mm2c_reg_t &r = regs[i];
			sum += r.cnt > 0 ? r.cnt : 0;
			if (r.cnt < 0 || r.as < 0 || (int64_t)r.as + r.cnt > bl || sum > bl)
				return fail(MM2C_E_ARG, "fragment %lld: region %lld leaves the fragment's anchors", (long long)f, (long long)(i - u_off[f]));
			for (int32_t j = 0; j < r.cnt; ++j)
				if ((int)(b[b_off[f] + r.as + j].y >> 48 & 0xff) >= n_segs)
					return fail(MM2C_E_ARG, "fragment %lld: an anchor of segment %d with n_segs %d", (long long)f, (int)(b[b_off[f] + r.as + j].y >> 48 & 0xff), n_segs);
		}
	}
	if (!lib_ready()) return fail_not_ready();
	const size_t nf = (size_t)n_frags, ns = (size_t)n_sr;
	std::vector<int64_t> off(2 * (nf + 1));
	for (int64_t k = 0; k <= n_frags; ++k) { off[(size_t)k] = u_off[k] - ub; off[nf + 1 + (size_t)k] = b_off[k] - bb; }
	mm2c_segplan_t *pl = mm2c_segplan_create(n_frags, n_segs, n_u, n_b);
	if (!pl) return MM2C_E_HIP;
	const size_t rb = (size_t)n_u * sizeof(mm2c_reg_t), ab = (size_t)n_b * 16, srb = (size_t)n_su * sizeof(mm2c_reg_t);
	Staging stage;
	const int i_off = stage.add(off.data(), nullptr, off.size() * 8), i_in = stage.add(n_u > 0 ? regs + ub : nullptr, nullptr, rb, 8), i_ni = stage.add(n_in, nullptr, nf * 4),
	          i_b = stage.add(n_b > 0 ? b + bb : nullptr, nullptr, ab, 16), i_sl = stage.add(seg_len, nullptr, ns * 4), i_h = stage.add(hash, nullptr, nf * 4), i_rl = stage.add(rep_len, nullptr, nf * 4),
	          i_suo = stage.add(nullptr, su_off, (ns + 1) * 8), i_sbo = stage.add(nullptr, sb_off, (ns + 1) * 8), i_su = stage.add(nullptr, nullptr, (size_t)n_su * 8, 8),
	          i_sb = stage.add(nullptr, nullptr, ab, 16), i_sr = stage.add(nullptr, nullptr, srb, 8), i_sh = stage.add(nullptr, seg_hash, ns * 4),
	          i_srl = stage.add(nullptr, rep_len ? seg_rep_len : nullptr, ns * 4);
	const int rc = stage.through(pl->device, [&] {
		const int64_t *d_off = stage.at<int64_t>(i_off);
		return mm2c_segplan_run_device(pl, d_off, stage.at<mm2c_reg_t>(i_in), stage.at<int32_t>(i_ni), d_off + nf + 1, stage.at<char>(i_b), stage.at<int32_t>(i_sl), stage.at<uint32_t>(i_h),
		                               rep_len ? stage.at<int32_t>(i_rl) : nullptr, stage.at<int64_t>(i_suo), stage.at<uint64_t>(i_su), stage.at<int64_t>(i_sbo), stage.at<char>(i_sb),
		                               stage.at<mm2c_reg_t>(i_sr), stage.at<uint32_t>(i_sh), rep_len ? stage.at<int32_t>(i_srl) : nullptr, MM2C_STREAM_LIBRARY);
	}, [&]() -> int {
		if (const int r = mm2c_segplan_check(pl, nullptr, nullptr, nullptr)) return r;
		const int64_t tu = su_off[n_sr], ta = sb_off[n_sr];                      // only what was made comes back
		if (tu < 0 || tu > n_su || ta < 0 || ta > n_b) return fail(MM2C_E_ARG, "segment totals beyond the capacities");
		if (tu > 0) HIP_TRY(hipMemcpy(su, stage.at<char>(i_su), (size_t)tu * 8, hipMemcpyDeviceToHost));
		if (tu > 0) HIP_TRY(hipMemcpy(seg_regs, stage.at<char>(i_sr), (size_t)tu * sizeof(mm2c_reg_t), hipMemcpyDeviceToHost));
		if (ta > 0) HIP_TRY(hipMemcpy(sb, stage.at<char>(i_sb), (size_t)ta * 16, hipMemcpyDeviceToHost));
		return 0;
	});
	stage.release();
	mm2c_segplan_destroy(pl);
	return rc;
}

} // extern "C"
