// api_internal.h -- shared between the translation units of the C-ABI shim (mm2chain_api.cpp: init, plans; mm2chain_host.cpp: host-buffer
// paths; mm2chain_seeds.cpp: seed-hit entries; mm2chain_sketch.cpp: reads-in entries).  Not installed; include/mm2chain.h is the public interface.
#ifndef MM2C_API_INTERNAL_H
#define MM2C_API_INTERNAL_H
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <mutex>
#include <numeric>
#include <vector>
#include "mm2chain.h"
#include "chain_kernel.h"

namespace mm2c_api {

extern thread_local char g_err[512];
int fail(int code, const char *fmt, ...);      // records the message mm2c_last_error() returns, hands back `code`

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
	return ::mm2c_api::fail(MM2C_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

struct ThreadCtx;

struct Global {
	std::mutex mu;
	std::atomic<bool> ready{false};         // written under `mu`; read without it by lib_ready()
	int device = -1;                        // primary device (= devices[0])
	std::vector<int> devices;               // every device the library drives (mm2c_init_devices); entries may repeat
	// tuning knobs: written by mm2c_tune / mm2c_init under `mu`, read by compute entries on other threads (atomics: no torn or stale-forever reads).  The ones with a
	// key are declared from csrc/knobs.def, which holds each one's key, environment variable, range, default and meaning
#define KNOB(type, member, key, env, lo, hi, dflt, flags, meaning) std::atomic<type> member{dflt};
#include "knobs.def"
#undef KNOB
	// ... and the ones without
	std::atomic<size_t> stage_max_anchors{1u << 21};     // host paths: calls up to this many anchors go through pinned staging buffers
	std::atomic<int64_t> cut_below_tasks{4096};         // host paths: passes with at least this many tasks are not cut (they fill the GPU anyway)
	std::atomic<size_t> direct_max_anchors{1u << 18};   // direct passes (direct_pass): passes of up to this many anchors
	hipStream_t stream = nullptr;           // library stream for plan runs with stream == NULL
	std::vector<ThreadCtx *> thread_ctxs;   // owned; released in mm2c_shutdown
	std::atomic<uint64_t> tasks{0}, anchors{0}, launches{0}, segments{0}, host_call_ns{0}, passes{0};
	uint64_t epoch = 0;                     // bumped by shutdown so stale thread-local pointers are dropped
};
extern Global G;
// the tuning knobs a DP launch goes by (mm2c::launch_chain_dp).  cls_arrays: the launch has class arrays of its own (LaunchArgs::d_cls, d_cls_stat) -- the knobs of the
// ring-size classes and of the wide share go with them
inline void knobs_into(mm2c::LaunchArgs &L, bool cls_arrays = true)
{
	L.ring_class = G.ring_class; L.force_tab = G.force_tab; L.compact = G.compact_ring; L.q24 = G.q24_ring; L.noskip_loop = G.noskip_loop; L.score_exit = G.score_bound_exit;
	L.coop_w8_above = G.coop_w8_above.load(); L.fuse_st = G.fuse_st.load();
	if (cls_arrays) { L.far_ring = G.far_ring; L.far_thr10 = G.far_thr10; L.wide_pct = G.wide_pct; }
}
// mm2c_init_async: the initialisation runs on a thread of its own while the host does something else (a minimap2 host loads its index, main.c:371-399, before the
// first chaining call); every entry that needs the device joins that thread first.  async_init_join is a no-op when none is pending and on the thread itself.
void async_init_join();
inline bool lib_ready() { async_init_join(); return G.ready; }
int fail_not_ready();                          // MM2C_E_NODEVICE with the reason: never initialised, or the asynchronous initialisation's own error

// mm2c_stage_stats_t, as atomics (the entries run on many host threads)
struct StageStats {
	std::atomic<uint64_t> calls{0}, chunks{0}, total_ns{0}, alloc_ns{0}, n_alloc{0}, free_ns{0}, n_free{0}, setup_ns{0}, h2d_ns{0}, seed_ns{0}, dp_ns{0},
	                      epi_ns{0}, d2h_ns{0}, wait_ns{0};
};
extern StageStats SS;
struct ScopedNs {                        // adds the wall time of its scope to a counter
	std::atomic<uint64_t> &acc; std::chrono::steady_clock::time_point t0;
	explicit ScopedNs(std::atomic<uint64_t> &a) : acc(a), t0(std::chrono::steady_clock::now()) {}
	~ScopedNs() { acc += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};

// one chunk in flight of mm2c_mm_chain_dp_batch_host (anchors up, DP, epilogue, chains down); grow-only arenas
struct WholeSlot {
	hipStream_t st = nullptr;
	char *d_in = nullptr, *d_work = nullptr, *d_res = nullptr, *h_meta = nullptr;
	size_t cap_in = 0, cap_work = 0, cap_res = 0, cap_hmeta = 0;
	int64_t k0 = 0, k1 = 0;                    // tasks of the chunk in flight
	size_t o_res_u = 0, o_res_b = 0, o_hres = 0;
	bool busy = false;
	void release()
	{
		if (d_in) (void)hipFree(d_in); if (d_work) (void)hipFree(d_work); if (d_res) (void)hipFree(d_res);
		if (h_meta) (void)hipHostFree(h_meta); if (st) (void)hipStreamDestroy(st);
		*this = WholeSlot();
	}
};

// one chunk in flight of mm2c_seed_chain_batch_host / _pool (matches up, seed hits -> anchors, DP, epilogue, chains down)
struct SeedSlot {
	hipStream_t st = nullptr;
	hipEvent_t ev[6] = {};                    // begin, uploaded, anchors made, DP done, chains made, offsets downloaded
	char *d_buf = nullptr, *h_meta = nullptr; // grow-only arena [matches | hits | qlen | (q_lo | q_eq: skip_seed) | anchors | f | p | u_off | b_off | u | b | (packed anchor_off)];
	                                          // pinned [u_off | b_off | (packed anchor_off)]
	size_t cap_buf = 0, cap_hmeta = 0;
	void *seedplan = nullptr, *plan = nullptr;   // the chunk's plans (their workspace comes from the device cache)
	int64_t k0 = 0, k1 = 0;
	size_t o_u = 0, o_b = 0;                  // where the chains of the chunk in flight lie in the arena
	bool busy = false, timed = false;
	void release()
	{
		if (d_buf) (void)hipFree(d_buf); if (h_meta) (void)hipHostFree(h_meta);
		for (auto &e : ev) if (e) (void)hipEventDestroy(e);
		if (st) (void)hipStreamDestroy(st);
		*this = SeedSlot();
	}
};

// per host thread: stream + grow-only buffers (the reference keeps one buffer set per FPGA kernel,
// chain_hardware.cpp:13-16,379-397, and serialises callers on a mutex).  One device arena for everything that is uploaded
// ([anchors | piece offsets | launch order | p base | avg | status]) and one for everything that is downloaded ([f | p]), each
// mirrored by a pinned host staging buffer, so that a call is one H2D copy, the kernels, one D2H copy and one sync.
struct ThreadCtx {
	int device = -1;                           // >= 0: the context belongs to this device whoever runs on it (a lane of a device slot's call combiner)
	WholeSlot whole[2];
	SeedSlot seed[2];
	hipStream_t st = nullptr, st2 = nullptr;   // st2: second compute stream of the pipelined big-batch path
	hipStream_t st3 = nullptr, st_up = nullptr;   // ... its third compute stream and its upload stream
	std::vector<hipEvent_t> evs;               // ... and its events (one per chunk in flight), kept for the next call
	hipEvent_t ev = nullptr;
	mm2c::LaunchInfo last_info = {};           // which instantiation the context's last DP launch chose (copied to the process-wide record, mm2c_last_host_variant)
	char *d_in = nullptr, *d_out = nullptr, *d_scratch = nullptr;   // device
	char *h_in = nullptr, *h_out = nullptr;                          // pinned host
	unsigned *h_flag = nullptr;                                      // pinned host: the word stage_out raises when a direct pass is done (host_stage.hip)
	unsigned seq = 0;                                                // number of the context's last direct pass (the value the flag takes)
	unsigned *d_cnt = nullptr;                                       // device: the counter of finished workgroups of a direct pass (zero between passes: whoever counts last puts it back)
	size_t cap_in = 0, cap_out = 0, cap_scratch = 0, cap_hin = 0, cap_hout = 0;
	void release()
	{
		if (d_in) (void)hipFree(d_in); if (d_out) (void)hipFree(d_out); if (d_scratch) (void)hipFree(d_scratch);
		if (h_in) (void)hipHostFree(h_in); if (h_out) (void)hipHostFree(h_out); if (h_flag) (void)hipHostFree(h_flag); if (d_cnt) (void)hipFree(d_cnt);
		if (st) (void)hipStreamDestroy(st); if (st2) (void)hipStreamDestroy(st2); if (ev) (void)hipEventDestroy(ev);
		if (st3) (void)hipStreamDestroy(st3); if (st_up) (void)hipStreamDestroy(st_up);
		for (hipEvent_t e : evs) (void)hipEventDestroy(e);
		whole[0].release(); whole[1].release();
		seed[0].release(); seed[1].release();
		*this = ThreadCtx();
	}
};

// "chain_dp_tile<...> loop=asm ... compact=1": the text of mm2c_plan_last_variant / mm2c_last_host_variant (score_exit: they add " score_exit=0|1" for the tile
// kernel; the route table of tests/route_dump.cpp is printed without it)
inline void format_variant(const mm2c::LaunchInfo &I, char *buf, size_t len, bool score_exit = false)
{
	if (I.tile && I.coop) snprintf(buf, len, "chain_dp_coop<W=%d,NX=%d,NF=%d,GS1=%d,FAR=%d,TAB=%d> loop=%s classes=0 cut=0 compact=0 coop=%d st=%s", I.coop, I.nx, I.nf, I.gs1,
	                               I.far_, I.tab, I.asm_loop ? "asm" : "c++", I.coop, I.fused_st ? "kernel" : "prepass");
	else if (I.tile) snprintf(buf, len, "chain_dp_tile<NX=%d,NF=%d,SKIP=%d,GEN=%d,GS1=%d,FAR=%d,TAB=%d> loop=%s classes=%d cut=%d compact=%d q24=%d packed_fp=%d", I.nx, I.nf, I.skip, I.gen, I.gs1,
	                     I.far_, I.tab, I.asm_loop ? "asm" : "c++", I.classes, I.cut, I.c16, I.q24, I.packed);
	else snprintf(buf, len, "chain_dp_wave<R=%d,SKIP=%d,GEN=%d,GS1=%d,FAR=%d> loop=c++ classes=0 cut=%d", I.r, I.skip, I.gen, I.gs1, I.far_, I.cut);
	if (score_exit && I.tile && !I.coop) { const size_t k = strlen(buf); snprintf(buf + k, len - k, " score_exit=%d", I.score_exit); }
}
void note_host_variant(const mm2c::LaunchInfo &I);   // mm2chain_host.cpp

int get_thread_ctx(ThreadCtx **out);
// context of the big-batch entries: the worker of a split batch gets the context of its device slot (as get_thread_ctx); every other caller gets
// ONE shared context, locked for the duration of the call -- a host whose mini-batches arrive on different pipeline threads (kt_pipeline,
// map.c:529-620) then reuses the same arenas instead of growing a set per thread
int get_batch_ctx(ThreadCtx **out, std::unique_lock<std::mutex> &hold);
int cur_device();                                    // device of the calling thread: a worker of a split batch drives its own, everyone else the primary
int n_devices();
bool in_split_worker();
// runs fn(part, k0, k1) for the contiguous task ranges mm2c_split_tasks gives, each on its own host thread bound to its own device context;
// returns the first non-zero code.  Only used when more than one device is configured and the caller is not itself such a worker.
bool should_split(int64_t total_anchors);
int run_split(int64_t n_tasks, const int64_t *h_offsets, const std::function<int(int, int64_t, int64_t)> &fn);
hipError_t create_partner_stream(hipStream_t *st);
int grow_device(char **p, size_t *cap, size_t need);
int grow_pinned(char **p, size_t *cap, size_t need, bool gpu_addressed = false);
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
// offsets of the pieces of one arena, each on a 256-byte boundary; `at` ends up as the arena's size
struct Layout {
	size_t at = 0;
	size_t take(size_t bytes) { const size_t o = at; at = (at + bytes + 255) & ~(size_t)255; return o; }
};
int check_params(const mm2c_params_t *p);
mm2c::KParams to_kparams(const mm2c_params_t *p);
int check_offsets(int64_t n_tasks, const int64_t *off);
int build_order(int64_t n_tasks, const int64_t *off, std::vector<int32_t> &order);
size_t layout_epilogue(mm2c::EpiArgs &E, char *base, size_t tot, size_t nt, size_t sort_tmp);
int epilogue_debug_phases();
hipError_t dev_alloc(void **out, size_t bytes);   // cached device memory for plans and one-shot calls (of the calling thread's current device)
void dev_free(void *p);                           // waits for the block's device first (as hipFree would), then parks the block in that device's cache
void dev_free_synced(void *p);                    // the caller has already made sure nothing is in flight on the block (one wait for many blocks)

// makes `dev` the calling thread's current device for the lifetime of the object and puts the caller's device back afterwards: an entry point
// must not change the current device of a host thread that also drives other GPUs (a torch caller, a worker of another library)
struct DeviceScope {
	int prev = -1; bool changed = false; hipError_t err = hipSuccess;
	explicit DeviceScope(int dev)
	{
		if (hipGetDevice(&prev) != hipSuccess) prev = -1;
		if (prev != dev) { err = hipSetDevice(dev); changed = err == hipSuccess; }
	}
	~DeviceScope() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
	DeviceScope(const DeviceScope &) = delete;
	DeviceScope &operator=(const DeviceScope &) = delete;
};
// the stream a stream argument of the C ABI stands for; MM2C_STREAM_LIBRARY is the library's stream, which lives on the primary device
inline int resolve_stream(void *stream, int device, hipStream_t *out)
{
	if (stream == MM2C_STREAM_LIBRARY) {
		if (device != G.device) return fail(MM2C_E_ARG, "MM2C_STREAM_LIBRARY belongs to the primary device %d; this plan lives on device %d: pass a stream of that device", G.device, device);
		*out = G.stream;
	} else *out = (hipStream_t)stream;             // NULL = the HIP null stream (what a default-stream caller such as PyTorch works on)
	return 0;
}
// the devices the library drives, each once, in configured order (G.devices may name a device twice)
inline std::vector<int> distinct_devices(const std::vector<int> &devs)
{
	std::vector<int> out;
	for (int dv : devs) if (std::find(out.begin(), out.end(), dv) == out.end()) out.push_back(dv);
	return out;
}
// something resident with one copy per device the library drives (a split batch reads the copy of its own device)
struct PerDevice {
	std::vector<int> dev;
	std::vector<void *> d;
	hipError_t add(int device, size_t bytes)             // the copy of `device`, which the caller has made current; not filled yet
	{
		void *p = nullptr;
		ScopedNs timed(SS.alloc_ns); ++SS.n_alloc;
		const hipError_t e = hipMalloc(&p, bytes);
		if (e == hipSuccess) { dev.push_back(device); d.push_back(p); }
		return e;
	}
	void *on(int device) const
	{
		for (size_t j = 0; j < dev.size(); ++j) if (dev[j] == device) return d[j];
		return nullptr;
	}
	void destroy()                                       // each copy after whatever its device still runs; the owner goes with them
	{
		for (size_t j = 0; j < dev.size(); ++j) { DeviceScope on(dev[j]); ScopedNs timed(SS.free_ns); ++SS.n_free; (void)hipDeviceSynchronize(); (void)hipFree(d[j]); }
	}
};
void dev_cache_release();
void release_combiner();                            // mm2chain_host.cpp
int get_slot_stats(int slot, uint64_t *passes, uint64_t *calls, uint64_t *anchors);   // per-device combiner counters (mm2chain_host.cpp)
int book_pred(int tid, float hw_ms, float sw_ms);   // path A's decline: the slot that books the call, or -1 (mm2chain_host.cpp)
void release_pred(int slot, float hw_ms);
void release_seed_aux();                            // mm2chain_seeds.cpp
// a pooled set of helper streams (distinct priorities = hardware queues of their own) and fork / join events, kept between plans (mm2chain_seeds.cpp)
struct AuxSet { hipStream_t aux[3] = {}; hipEvent_t fork[4] = {}; int device = -1; uint64_t epoch = 0; };   // epoch: G.epoch when the set was made (a set of an earlier one is destroyed, not pooled)
hipError_t aux_acquire(int device, AuxSet *out);
void aux_release(const AuxSet &a);
// for callers that have already waited for the stream(s) the plan ran on: no device-wide wait (chunks of a pipelined batch overlap)
void plan_destroy_synced(mm2c_plan_t *pl);          // mm2chain_api.cpp
void seedplan_destroy_synced(mm2c_seedplan_t *pl);  // mm2chain_seeds.cpp

// ---- shared by the matches-in entries (mm2chain_seeds.cpp, where all of this lives) and the reads-in entries (mm2chain_sketch.cpp)
const uint64_t *hitpool_on(const mm2c_hitpool_t *hp, int device);
// a pool from copies that are on the devices already (mm2c_minidx_build: the sorted y column); the pool takes them over.  max_rid: the largest rid among the hits, -1 without hits
mm2c_hitpool_t *hitpool_adopt(int64_t n_hits, int64_t max_rid, PerDevice &copies);
int check_skip_pool(const mm2c_seed_skip_host_t *skip, int64_t n_reads, const mm2c_hitpool_t *pool);   // skip_seed against a resident pool, before any kernel runs
// skip_seed from the host description to the device.  The rules, written once: without ref_rank no name is compared and nothing goes up; the two reference arrays
// hold max(n_ref, 1) entries each; ref_len may be NULL (only NO_DIAG / NO_DUAL read it, and check_skip refuses them without); q_lo / q_eq go up when both are given.
inline size_t skip_n_ref(const mm2c_seed_skip_host_t *skip) { return skip && skip->ref_rank ? (size_t)std::max<int32_t>(skip->n_ref, 1) : 0; }
inline bool skip_per_read(const mm2c_seed_skip_host_t *skip) { return skip && skip->ref_rank && skip->q_lo && skip->q_eq; }
hipError_t skip_upload_refs(const mm2c_seed_skip_host_t *skip, int32_t *d_rank, int32_t *d_len, hipStream_t st);   // enqueues ref_rank / ref_len (once per call)
// enqueues q_lo / q_eq of reads [k0, k1) and fills the description the seed plan of those reads runs with
hipError_t skip_upload_reads(const mm2c_seed_skip_host_t *skip, int64_t k0, int64_t k1, const int32_t *d_rank, const int32_t *d_len, int32_t *d_lo, int32_t *d_eq,
                             hipStream_t st, mm2c_seed_skip_t *sk);
// One chunk of whole reads on the device.  The part of its arena both paths lay out alike, behind whatever the caller has taken from `L` before ...
struct ChunkLayout { size_t o_q, o_lo, o_eq, o_a, o_f, o_p, o_uo, o_bo, o_u, o_b, o_ao; };   // qlen | (q_lo | q_eq) | anchors | f | p | u_off | b_off | u | b | (packed anchor_off)
ChunkLayout chunk_layout(Layout &L, size_t nr, size_t tot, bool per_read, bool packed_off);
// ... and everything from the seed hits to the offsets' way down, enqueued on `st`: seed plan (sk != NULL: with skip_seed, and the chain plan then goes by the packed
// offsets) -> DP -> epilogue -> h_off = [u_off | b_off | (packed anchor_off)] on the host.  qlen, q_lo, q_eq are in the arena `d` already, the matches wherever the
// caller has them on the device.  ev_seed / ev_dp / ev_epi are recorded behind the stage they name; any of them may be NULL.
int chunk_step(mm2c_seedplan_t *sp, mm2c_plan_t *pl, const mm2c_match_t *d_matches, const uint64_t *d_hits, int64_t n_hits, const mm2c_seed_skip_t *sk, char *d,
               const ChunkLayout &o, int min_cnt, int min_sc, hipStream_t st, hipEvent_t ev_seed, hipEvent_t ev_dp, hipEvent_t ev_epi, int64_t *h_off);

} // namespace mm2c_api
#endif
