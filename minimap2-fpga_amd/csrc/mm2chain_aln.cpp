// mm2chain_aln.cpp -- C-ABI entries of the step between final regions and base alignment (include/mm2chain.h): the resident packed reference, the alignment-task
// plan (mm_align1 up to its mm_align_pair calls on the device, align_tasks.hip) and the host-buffer entry built on them.
#include "plan_common.h"
#include "align_tasks.h"
#include <cstddef>

using namespace mm2c_api;

static_assert(sizeof(mm2c_aln_opt_t) == sizeof(mm2c::AlnOpt) && sizeof(mm2c_aln_opt_t) == 80 && offsetof(mm2c_aln_opt_t, max_sw_mat) == 56 && offsetof(mm2c_aln_opt_t, k) == 72, "layout");
static_assert(sizeof(mm2c_aln_reg_t) == sizeof(mm2c::AlnReg) && sizeof(mm2c_aln_reg_t) == 104 && offsetof(mm2c_aln_reg_t, item0) == 56, "layout");
static_assert(sizeof(mm2c_aln_item_t) == sizeof(mm2c::AlnItem) && sizeof(mm2c_aln_item_t) == 40, "layout");
static_assert(sizeof(mm2c_reg_t) == sizeof(mm2c::AlnRegIn) && offsetof(mm2c_reg_t, flags) == offsetof(mm2c::AlnRegIn, flags) && offsetof(mm2c_reg_t, as) == offsetof(mm2c::AlnRegIn, as), "layout");
static_assert(MM2C_ALN_LDS_GAPS == mm2c::ALN_LDS_GAPS && MM2C_ALN_MAX_SLOTS == mm2c::ALN_MAX_SLOTS && MM2C_ALN_REFUSED == mm2c::ALN_REFUSED && MM2C_ALN_TOO_BIG == mm2c::ALN_TOO_BIG &&
              MM2C_ALN_OVER_CAP == mm2c::ALN_OVER_CAP && MM2C_ALN_OVER == mm2c::ALN_OVER && MM2C_ALN_F_SR == mm2c::ALN_F_SR && MM2C_ALN_F_NO_END_FLT == mm2c::ALN_F_NO_END_FLT &&
              MM2C_ALN_F_SPLICE == mm2c::ALN_F_SPLICE && MM2C_ALN_I_HPC == mm2c::ALN_I_HPC && MM2C_ALN_RIGHT == mm2c::ALN_RIGHT, "constants of mm2chain.h");

struct mm2c_refseq {
	int64_t n_seq = 0, n_words = 0;
	int device = 0;
	char *d_mem = nullptr;                 // [offset | len | S]
	uint64_t *d_off = nullptr;
	uint32_t *d_len = nullptr, *d_S = nullptr;
};

struct mm2c_alnplan : PlanBase {           // d_mem: [flags, totals | scratch]; events: begin, behind aln_scan, behind aln_emit, behind aln_gather
	int64_t n_regs_cap = 0, items_cap = 0, tasks_cap = 0, pool_cap = 0, b_cap = 0, reads_cap = 0, slot_words = 0;
	int32_t n_slots = 0, cig_shift = 0;
	int32_t *d_flags = nullptr;
	int64_t *d_totals = nullptr;
	int32_t *d_scratch = nullptr;
};

static int check_refseq(int64_t n_seq, const uint64_t *offset, const uint32_t *len, const uint32_t *S, int64_t n_words)
{
	if (n_seq < 0 || n_seq > INT32_MAX || n_words < 0 || n_words > (INT64_MAX >> 4)) return fail(MM2C_E_ARG, "bad argument");
	if (n_seq > 0 && (!offset || !len)) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (n_words > 0 && !S) return fail(MM2C_E_ARG, "host pointer is NULL");
	for (int64_t i = 0; i < n_seq; ++i) {
		if (len[i] > (uint32_t)INT32_MAX) return fail(MM2C_E_ARG, "contig %lld: 2^31 bases or more", (long long)i);
		if (offset[i] > (uint64_t)n_words * 8 || (uint64_t)n_words * 8 - offset[i] < len[i]) return fail(MM2C_E_ARG, "contig %lld leaves the %lld words of S", (long long)i, (long long)n_words);
	}
	return 0;
}

static int check_opt(const mm2c_aln_opt_t *opt)
{
	if (!opt) return fail(MM2C_E_ARG, "options are NULL");
	if (opt->e <= 0) return fail(MM2C_E_ARG, "e must be > 0 (align.c:644 divides by it)");
	if (opt->k < 1 || opt->k > 255) return fail(MM2C_E_ARG, "k outside 1 .. 255");
	if (opt->bw < 0 || opt->bw > (1 << 29) || opt->max_gap < 0 || opt->a < 0 || opt->a > (1 << 15) || opt->q < 0) return fail(MM2C_E_ARG, "bw, max_gap, a or q out of range");
	return 0;
}

extern "C" {

mm2c_refseq_t *mm2c_refseq_create(int64_t n_seq, const uint64_t *offset, const uint32_t *len, const uint32_t *S, int64_t n_words)
{
	if (check_refseq(n_seq, offset, len, S, n_words)) return nullptr;
	if (!lib_ready()) { (void)fail_not_ready(); return nullptr; }
	mm2c_refseq *rf = new mm2c_refseq();
	rf->n_seq = n_seq; rf->n_words = n_words;
	Layout L;
	const size_t o_o = L.take((size_t)n_seq * 8 + 16), o_l = L.take((size_t)n_seq * 4 + 16), o_s = L.take((size_t)n_words * 4 + 16);
	rf->device = cur_device();
	DeviceScope on(rf->device);
	hipError_t e = on.err;
	if (e == hipSuccess) e = dev_alloc((void **)&rf->d_mem, L.at);
	if (e == hipSuccess) {
		rf->d_off = (uint64_t *)(rf->d_mem + o_o); rf->d_len = (uint32_t *)(rf->d_mem + o_l); rf->d_S = (uint32_t *)(rf->d_mem + o_s);
		if (n_seq > 0) e = hipMemcpy(rf->d_off, offset, (size_t)n_seq * 8, hipMemcpyHostToDevice);
		if (e == hipSuccess && n_seq > 0) e = hipMemcpy(rf->d_len, len, (size_t)n_seq * 4, hipMemcpyHostToDevice);
		if (e == hipSuccess && n_words > 0) e = hipMemcpy(rf->d_S, S, (size_t)n_words * 4, hipMemcpyHostToDevice);
	}
	if (e != hipSuccess) {
		(void)fail(MM2C_E_HIP, "mm2c_refseq_create: %s (%lld words)", hipGetErrorString(e), (long long)n_words);
		mm2c_refseq_destroy(rf);
		return nullptr;
	}
	return rf;
}

void mm2c_refseq_destroy(mm2c_refseq_t *rf)
{
	if (!rf) return;
	{
		DeviceScope on(rf->device);
		dev_free(rf->d_mem);
	}
	delete rf;
}

mm2c_alnplan_t *mm2c_alnplan_create(int64_t n_regs_cap, int64_t n_items_cap, int64_t n_tasks_cap, int64_t pool_cap, int64_t n_b_cap, int64_t reads_cap, int32_t cig_shift,
                                    int64_t n_slots, int64_t slot_words)
{
	if (!lib_ready()) { (void)fail_not_ready(); return nullptr; }
	if (n_slots <= 0) n_slots = 2048;
	if (n_regs_cap < 0 || n_regs_cap > INT32_MAX || n_items_cap < 0 || n_tasks_cap < 0 || n_tasks_cap > INT32_MAX || pool_cap < 0 || n_b_cap < 0 || reads_cap < 0 || cig_shift < 0 ||
	    cig_shift > 30 || n_slots > MM2C_ALN_MAX_SLOTS || slot_words < 0 || slot_words > INT32_MAX) {
		(void)fail(MM2C_E_ARG, "bad argument");
		return nullptr;
	}
	mm2c_alnplan *pl = new mm2c_alnplan();
	pl->n_regs_cap = n_regs_cap; pl->items_cap = n_items_cap; pl->tasks_cap = n_tasks_cap; pl->pool_cap = pool_cap; pl->b_cap = n_b_cap; pl->reads_cap = reads_cap;
	pl->cig_shift = cig_shift; pl->n_slots = (int32_t)n_slots; pl->slot_words = slot_words;
	Layout L;
	const size_t o_fl = L.take(64), o_sc = L.take((size_t)slot_words * 4 * (size_t)n_slots + 256);
	const hipError_t e = pl->open(L.at, 4);
	if (e != hipSuccess) {
		(void)fail(MM2C_E_HIP, "mm2c_alnplan_create: %s (%lld slots of %lld words)", hipGetErrorString(e), (long long)n_slots, (long long)slot_words);
		mm2c_alnplan_destroy(pl);
		return nullptr;
	}
	pl->d_flags = (int32_t *)(pl->d_mem + o_fl); pl->d_totals = (int64_t *)(pl->d_mem + o_fl + 16); pl->d_scratch = (int32_t *)(pl->d_mem + o_sc);
	return pl;
}

void mm2c_alnplan_destroy(mm2c_alnplan_t *pl)
{
	if (!pl) return;
	pl->close();
	delete pl;
}

int mm2c_alnplan_run_device(mm2c_alnplan_t *pl, const mm2c_aln_opt_t *opt, const mm2c_refseq_t *ref, int64_t n_reads, int64_t n_regs, const int64_t *d_u_off,
                            const mm2c_reg_t *d_regs, const int64_t *d_b_off, const int64_t *d_n_b, void *d_b, const int64_t *d_read_off, const uint8_t *d_reads,
                            mm2c_aln_reg_t *d_aln_regs, mm2c_aln_item_t *d_items, mm2c_ksw_task_t *d_tasks, int64_t *d_cig_off, uint8_t *d_pool, void *stream)
{
	if (!pl || !ref) return fail(MM2C_E_ARG, "plan or reference is NULL");
	if (!lib_ready()) return fail_not_ready();
	if (const int rc = check_opt(opt)) return rc;
	if (ref->device != pl->device) return fail(MM2C_E_ARG, "the reference lives on device %d, the plan on device %d", ref->device, pl->device);
	if (n_reads < 0 || n_regs < 0 || n_regs > pl->n_regs_cap) return fail(MM2C_E_ARG, "%lld regions in a plan for %lld", (long long)n_regs, (long long)pl->n_regs_cap);
	if (n_regs > 0 && (n_reads == 0 || !d_u_off || !d_regs || !d_b_off || !d_read_off || !d_aln_regs || !d_cig_off || (pl->b_cap > 0 && !d_b) || (pl->reads_cap > 0 && !d_reads) ||
	                   (pl->items_cap > 0 && !d_items) || (pl->tasks_cap > 0 && !d_tasks) || (pl->pool_cap > 0 && !d_pool)))
		return fail(MM2C_E_ARG, "device pointer is NULL");
	if (((uintptr_t)d_u_off | (uintptr_t)d_regs | (uintptr_t)d_b_off | (uintptr_t)d_n_b | (uintptr_t)d_read_off | (uintptr_t)d_aln_regs | (uintptr_t)d_tasks | (uintptr_t)d_cig_off) & 7)
		return fail(MM2C_E_ARG, "offsets, regions or tasks are not 8-byte aligned");
	if (((uintptr_t)d_b | (uintptr_t)d_pool) & 15) return fail(MM2C_E_ARG, "anchors or pool are not 16-byte aligned");
	if ((uintptr_t)d_items & 3) return fail(MM2C_E_ARG, "items are not 4-byte aligned");
	DeviceScope on(pl->device);
	hipStream_t st;
	if (const int rc = pl->begin(on, stream, &st, pl->d_flags, 64)) return rc;
	mm2c::AlnArgs X = {};
	X.n_reads = n_reads; X.n_regs = n_regs; X.items_cap = pl->items_cap; X.tasks_cap = pl->tasks_cap; X.pool_cap = pl->pool_cap; X.b_cap = pl->b_cap; X.reads_cap = pl->reads_cap;
	memcpy(&X.opt, opt, sizeof X.opt);
	X.cig_shift = pl->cig_shift; X.u_off = d_u_off; X.regs = (const mm2c::AlnRegIn *)d_regs; X.b_off = d_b_off; X.n_b = d_n_b; X.b = (ulonglong2 *)d_b; X.read_off = d_read_off;
	X.reads = d_reads; X.n_seq = ref->n_seq; X.n_words = ref->n_words; X.ref_off = ref->d_off; X.ref_len = ref->d_len; X.S = ref->d_S;
	X.aregs = (mm2c::AlnReg *)d_aln_regs; X.items = (mm2c::AlnItem *)d_items; X.tasks = (mm2c::KswTask *)d_tasks; X.cig_off = d_cig_off; X.pool = d_pool;
	X.scratch = pl->d_scratch; X.slot_words = pl->slot_words; X.n_slots = pl->n_slots; X.flags = pl->d_flags; X.totals = pl->d_totals;
	if (n_regs == 0 && d_cig_off) HIP_TRY(hipMemsetAsync(d_cig_off, 0, 8, st));            // no kernel runs: the list of 0 tasks still ends at cig_off[0] = 0
	HIP_TRY(hipEventRecord(pl->ev[0], st));
	HIP_TRY(mm2c::launch_aln_plan(X, st));
	HIP_TRY(hipEventRecord(pl->ev[1], st));
	HIP_TRY(mm2c::launch_aln_emit(X, st));
	HIP_TRY(hipEventRecord(pl->ev[2], st));
	HIP_TRY(mm2c::launch_aln_gather(X, st));
	HIP_TRY(hipEventRecord(pl->ev[3], st));
	return pl->end(n_regs > 0 ? 4 : 0);
}

int mm2c_alnplan_check(mm2c_alnplan_t *pl, int64_t *n_refused, int64_t *n_too_big, int64_t totals[4])
{
	if (!pl) return fail(MM2C_E_ARG, "plan is NULL");
	if (n_refused) *n_refused = 0;
	if (n_too_big) *n_too_big = 0;
	if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
	if (!pl->ran) return 0;
	int64_t w[6] = {};
	if (const int rc = pl->read_flags(3, pl->d_flags, w, sizeof w)) return rc;
	int32_t fl[4];
	memcpy(fl, w, sizeof fl);
	if (n_refused) *n_refused = fl[0];
	if (n_too_big) *n_too_big = (int64_t)fl[1] + fl[2];
	if (totals) for (int c = 0; c < 4; ++c) totals[c] = w[2 + c];
	if (fl[0] != 0) return fail(MM2C_E_ARG, "%d region(s) refused: a mode that is not built (splice, sr, HPC), as / cnt leaving the read's anchors, anchors not on one reference strand, "
	                                        "outside their contig or read or running backwards, an input the reference asserts on, or offsets leaving a capacity", fl[0]);
	if (fl[1] != 0 || fl[2] != 0) return fail(MM2C_E_TOOBIG, "%d region(s) with more long gaps than MM2C_ALN_LDS_GAPS and than a scratch slot of %lld words were not run; %d region(s) "
	                                                         "leave a capacity (the batch takes %lld items, %lld tasks, %lld pool bytes)", fl[1], (long long)pl->slot_words, fl[2],
	                                                         (long long)w[2], (long long)w[3], (long long)w[5]);
	return 0;
}

int mm2c_alnplan_last_kernel_ms(mm2c_alnplan_t *pl, float ms[3])
{
	if (!pl || !ms) return fail(MM2C_E_ARG, "NULL argument");
	if (!pl->ran) return fail(MM2C_E_ARG, "plan has not been run");
	return pl->elapsed(3, {{0, 1, ms}, {1, 2, ms + 1}, {2, 3, ms + 2}});
}

int mm2c_align_tasks_batch_host(const mm2c_aln_opt_t *opt, int64_t n_seq, const uint64_t *offset, const uint32_t *len, const uint32_t *S, int64_t n_words,
                                int64_t n_reads, const int64_t *u_off, const mm2c_reg_t *regs, const int64_t *b_off, mm2c_anchor_t *b, const int64_t *read_off,
                                const uint8_t *reads, int32_t cig_shift, mm2c_aln_reg_t *aln_regs, int64_t n_items_cap, mm2c_aln_item_t *items, int64_t n_tasks_cap,
                                mm2c_ksw_task_t *tasks, int64_t *cig_off, int64_t pool_cap, uint8_t *pool, int64_t totals[4])
{
	if (const int rc = check_opt(opt)) return rc;
	if (const int rc = check_refseq(n_seq, offset, len, S, n_words)) return rc;
	if (n_reads < 0 || n_reads > INT32_MAX || n_items_cap < 0 || n_tasks_cap < 0 || n_tasks_cap > INT32_MAX || pool_cap < 0 || cig_shift < 0 || cig_shift > 30) return fail(MM2C_E_ARG, "bad argument");
	if (n_reads == 0) return 0;
	if (!u_off || !b_off || !read_off || !cig_off) return fail(MM2C_E_ARG, "host pointer is NULL");
	if (u_off[0] != 0 || b_off[0] != 0 || read_off[0] != 0) return fail(MM2C_E_ARG, "u_off[0], b_off[0] and read_off[0] must be 0");
	for (int64_t r = 0; r < n_reads; ++r) {
		if (u_off[r + 1] < u_off[r] || b_off[r + 1] < b_off[r] || read_off[r + 1] < read_off[r]) return fail(MM2C_E_ARG, "offsets not monotone at read %lld", (long long)r);
		if (read_off[r + 1] - read_off[r] > INT32_MAX || b_off[r + 1] - b_off[r] > INT32_MAX) return fail(MM2C_E_ARG, "read %lld is too long", (long long)r);
	}
	const int64_t n_regs = u_off[n_reads], n_b = b_off[n_reads], n_bases = read_off[n_reads];
	if (n_regs > INT32_MAX) return fail(MM2C_E_ARG, "too many regions");
	if (n_regs == 0) { if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0; cig_off[0] = 0; return 0; }
	if (!regs || !aln_regs || (n_b > 0 && !b) || (n_bases > 0 && !reads) || (n_items_cap > 0 && !items) || (n_tasks_cap > 0 && !tasks) || (pool_cap > 0 && !pool))
		return fail(MM2C_E_ARG, "host pointer is NULL");
	for (int64_t k = 0; k < n_bases; ++k) if (reads[k] > 4) return fail(MM2C_E_ARG, "base code %d at %lld of the reads", reads[k], (long long)k);
	for (int64_t i = 0; i < n_seq; ++i)
		for (uint64_t p = offset[i]; p < offset[i] + len[i]; ++p)
			if ((S[p >> 3] >> ((p & 7) << 2) & 0xf) > 4) return fail(MM2C_E_ARG, "base code above 4 at %llu of contig %lld", (unsigned long long)(p - offset[i]), (long long)i);
	if (!lib_ready()) return fail_not_ready();
	mm2c_refseq_t *rf = mm2c_refseq_create(n_seq, offset, len, S, n_words);
	if (!rf) return MM2C_E_HIP;
	int64_t longest = 0;                    // a region has fewer long gaps than anchors, and no more anchors than its read: slots of the longest region, so nothing is too big
	for (int64_t r = 0; r < n_reads; ++r)
		for (int64_t g = u_off[r]; g < u_off[r + 1]; ++g) longest = std::max<int64_t>(longest, std::min<int64_t>(regs[g].cnt, b_off[r + 1] - b_off[r]));
	const int64_t slot_words = longest > MM2C_ALN_LDS_GAPS ? longest : 0;
	const int64_t slots = slot_words ? std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_regs, 2048), (1ll << 30) / (slot_words * 4))) : 0;
	mm2c_alnplan_t *pl = mm2c_alnplan_create(n_regs, n_items_cap, n_tasks_cap, pool_cap, n_b, n_bases, cig_shift, slots, slot_words);
	if (!pl) { mm2c_refseq_destroy(rf); return MM2C_E_HIP; }
	Staging stage;
	const size_t nr = (size_t)n_reads, ng = (size_t)n_regs, nt = (size_t)n_tasks_cap;
	// items, tasks, cig_off and pool go up as well: what is not written stays the caller's
	const int i_u = stage.add(u_off, nullptr, (nr + 1) * 8), i_g = stage.add(regs, nullptr, ng * sizeof(mm2c_reg_t)), i_bo = stage.add(b_off, nullptr, (nr + 1) * 8),
	          i_b = stage.add(b, b, (size_t)n_b * 16, 16), i_ro = stage.add(read_off, nullptr, (nr + 1) * 8), i_rd = stage.add(reads, nullptr, (size_t)n_bases, 16),
	          i_ar = stage.add(nullptr, aln_regs, ng * sizeof(mm2c_aln_reg_t)), i_it = stage.add(items, items, (size_t)n_items_cap * sizeof(mm2c_aln_item_t), 16),
	          i_tk = stage.add(tasks, tasks, nt * sizeof(mm2c_ksw_task_t), 16), i_co = stage.add(cig_off, cig_off, (nt + 1) * 8), i_p = stage.add(pool, pool, (size_t)pool_cap, 16);
	const int rc = stage.through(pl->device, [&] {
		return mm2c_alnplan_run_device(pl, opt, rf, n_reads, n_regs, stage.at<int64_t>(i_u), stage.at<mm2c_reg_t>(i_g), stage.at<int64_t>(i_bo), nullptr, stage.at<char>(i_b), stage.at<int64_t>(i_ro),
		                               stage.at<uint8_t>(i_rd), stage.at<mm2c_aln_reg_t>(i_ar), stage.at<mm2c_aln_item_t>(i_it), stage.at<mm2c_ksw_task_t>(i_tk), stage.at<int64_t>(i_co), stage.at<uint8_t>(i_p),
		                               MM2C_STREAM_LIBRARY);
	}, [&] { return mm2c_alnplan_check(pl, nullptr, nullptr, totals); });
	stage.release();
	mm2c_alnplan_destroy(pl);
	mm2c_refseq_destroy(rf);
	return rc;
}

} // extern "C"
