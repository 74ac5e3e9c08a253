// plan_common.h -- the host side the stand-alone device plans share (mm2chain_regs / _hits / _mapq / _esterr / _segs / _ksw / _extra / _aln.cpp): the life of a plan
// (device, one block of device memory, events, "has run") and the staging of a *_batch_host entry's arrays around one run of its plan.  What a plan computes, its
// argument checks and its messages stay in its own file.  Not installed; no device code includes this header.
#ifndef MM2C_PLAN_COMMON_H
#define MM2C_PLAN_COMMON_H
#include <initializer_list>
#include "api_internal.h"

namespace mm2c_api {

struct PlanBase {
	int device = 0;
	char *d_mem = nullptr;                 // the plan's own device memory: its flag words in front, then its scratch
	hipEvent_t ev[8] = {};                 // the events the plan records around its kernels; the largest plan has 7
	bool ran = false;

	// the calling thread's device becomes the plan's; `bytes` of device memory and the first n_events events.  The caller words the failure and closes the plan.
	hipError_t open(size_t bytes, int n_events)
	{
		device = cur_device();
		DeviceScope on(device);
		hipError_t e = on.err;
		if (e == hipSuccess) e = dev_alloc((void **)&d_mem, bytes);
		for (int i = 0; i < n_events && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
		return e;
	}
	// what a create does on the plan's device behind open(): a table to upload, counters to zero
	template <class F> hipError_t on_device(F f)
	{
		DeviceScope on(device);
		return on.err != hipSuccess ? on.err : f();
	}
	// also of a plan whose open failed half way.  Only a plan that ran has something in flight to wait for.
	void close()
	{
		DeviceScope on(device);
		if (ran) { ScopedNs timed(SS.free_ns); (void)hipDeviceSynchronize(); }
		dev_free_synced(d_mem);
		for (auto &e : ev) if (e) (void)hipEventDestroy(e);
	}
	// the head of a run, under the caller's DeviceScope of the plan's device: the stream the argument stands for, and the plan's flag words zeroed on it
	int begin(const DeviceScope &on, void *stream, hipStream_t *st, void *d_flags, size_t flag_bytes)
	{
		HIP_TRY(on.err);
		if (const int rc = resolve_stream(stream, device, st)) return rc;
		HIP_TRY(hipMemsetAsync(d_flags, 0, flag_bytes, *st));
		return 0;
	}
	int end(uint64_t n_launches)
	{
		ran = true;
		G.launches += n_launches;
		return 0;
	}
	// waits for event `last`, then brings the flag words to the host
	int read_flags(int last, const void *d_flags, void *dst, size_t bytes)
	{
		DeviceScope on(device);
		HIP_TRY(on.err);
		HIP_TRY(hipEventSynchronize(ev[last]));
		HIP_TRY(hipMemcpy(dst, d_flags, bytes, hipMemcpyDeviceToHost));
		return 0;
	}
	// waits for event `last`, then *ms = the time from event `from` to event `to`, span by span
	struct Span { int from, to; float *ms; };
	int elapsed(int last, std::initializer_list<Span> spans)
	{
		DeviceScope on(device);
		HIP_TRY(on.err);
		HIP_TRY(hipEventSynchronize(ev[last]));
		for (const Span &s : spans) HIP_TRY(hipEventElapsedTime(s.ms, ev[s.from], ev[s.to]));
		return 0;
	}
};

// The arrays of a *_batch_host entry on the device: pieces of ONE block of cached device memory, each on a 256-byte boundary in the order they are added.  A piece
// with `up` is copied to the device before the run, one with `down` back to the host after it (an output that is both keeps what the run does not write: it stays
// the caller's); a piece of 0 bytes is not copied.  Everything is enqueued on the library's stream.
struct Staging {
	struct Piece { const void *up; void *down; size_t bytes, off; };
	std::vector<Piece> pieces;
	Layout L;
	char *d = nullptr;

	int add(const void *up, void *down, size_t bytes, size_t pad = 0)          // -> the piece's number; pad: bytes of room behind it
	{
		pieces.push_back(Piece{up, down, bytes, L.take(bytes + pad)});
		return (int)pieces.size() - 1;
	}
	template <class T> T *at(int piece) const { return (T *)(d + pieces[(size_t)piece].off); }   // valid inside run() and after()
	// allocation, uploads, run() -- the plan's run_device on MM2C_STREAM_LIBRARY --, downloads, the wait for them, after() -- the plan's check.  The first failure ends it.
	template <class Run, class After> int through(int device, Run run, After after)
	{
		DeviceScope on(device);
		HIP_TRY(on.err);
		HIP_TRY(dev_alloc((void **)&d, L.at));
		hipStream_t st = G.stream;
		for (const Piece &p : pieces) if (p.up && p.bytes) HIP_TRY(hipMemcpyAsync(d + p.off, p.up, p.bytes, hipMemcpyHostToDevice, st));
		if (const int r = run()) return r;
		for (const Piece &p : pieces) if (p.down && p.bytes) HIP_TRY(hipMemcpyAsync(p.down, d + p.off, p.bytes, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		return after();
	}
	void release() { dev_free(d); d = nullptr; }                               // on every path, before the plan is destroyed
};

} // namespace mm2c_api
#endif
