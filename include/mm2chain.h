/*
 * mm2chain.h -- C ABI of the MI355X (gfx950) chaining library, libmm2chain_hip.so.
 *
 * Drop-in boundary for ONE hot path of kisarur/minimap2-fpga: the predecessor-scan DP that fills f[] / p[]
 * inside mm_chain_dp (chain.c:184-238), which the reference offloads through run_chaining_on_hw
 * (chain_hardware.h:68, chain_hardware.cpp:27-197, kernel device/minimap2_opencl.cl:24-182) -- and, for batched callers, the
 * steps either side of it inside mm_map_frag: collect_seed_hits before (map.c:215-247, "seed hits -> sorted anchors") and the rest
 * of mm_chain_dp after (chain.c:348-422, "f/p -> chains").
 *
 * Plain C: pointers and sizes only, no torch / C++ types.  All entry points return 0 on success and a
 * negative MM2C_E_* code on failure unless stated otherwise; mm2c_last_error() gives the message.  There is
 * NO CPU fallback anywhere behind this header: if no HIP device is usable every compute entry fails.
 *
 * Preconditions shared by every chaining entry (they are the reference caller's guarantees):
 *   - anchors of one task are sorted ascending by x (map.c:245); x = strand<<63 | rid<<32 | rpos (map.c:228-241) is compared as a
 *     64-bit value, no layout inside it is assumed
 *   - 0 <= max_dist_x, and every task has n < 2^31 - 64 anchors (chain.c:30 "TODO" holds here too)
 */
#ifndef MM2CHAIN_H
#define MM2CHAIN_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* same layout as mm128_t (minimap.h:53): 16 bytes, x then y */
typedef struct { uint64_t x, y; } mm2c_anchor_t;

enum {
	MM2C_OK = 0,
	MM2C_E_NODEVICE = -1,  /* no usable HIP device / mm2c_init not called (cf. hardware_init false, main.c:367) */
	MM2C_E_ARG = -2,       /* bad argument (negative n, NULL pointer, negative max_dist_x, ...) */
	MM2C_E_TOOBIG = -3,    /* task larger than the supported maximum (cf. chain_hardware.cpp:34-37): see MM2C_MAX_TASK_ANCHORS */
	MM2C_E_HIP = -4        /* HIP runtime error (cf. checkError, chain_hardware.cpp:208-235) */
};

/* flags for mm2c_params_t.flags */
#define MM2C_F_IGNORE_SEG  0x1  /* treat all anchors as one segment (what the FPGA kernel does, .cl:116-127) */
#define MM2C_F_FORCE_GENERAL 0x2 /* always run the general (segment / cDNA aware) kernel variant */

/*
 * Scalars of one mm_chain_dp call (mmpriv.h:65 arguments 1-5, 8-10).  q_span_override >= 0 replaces the
 * per-anchor span (a[i].y>>32 & 0xff, chain.c:189) by one value, which is what the reference's device
 * interface carries (chain_hardware.h:68 argument q_span, chain.c:91-96).
 */
typedef struct {
	int32_t max_dist_x, max_dist_y, bw;
	int32_t max_skip, max_iter;
	float   gap_scale;
	int32_t is_cdna, n_segs;
	int32_t q_span_override;   /* -1: per-anchor span */
	int32_t flags;             /* MM2C_F_* */
} mm2c_params_t;

/* ---- lifecycle: replaces hardware_init(BUFFER_N, XCLBIN_FILE) / cleanup() (chain_hardware.h:70-71, main.c:367,430) ---- */
int  mm2c_init(int device_ordinal);           /* -1: current device -- or, when the environment variable MM2C_DEVICES is set ("all" or a
                                               * comma-separated list of ordinals), those devices as with mm2c_init_devices: the route for a host
                                               * whose init hook carries no ordinals (hardware_init, chain_hardware.h:69).  Idempotent. */
/* mm2c_init on a thread of its own: returns at once, the runtime start-up (about 0.2 s) and the loading of the kernels' code objects run while the host
 * does its own start-up work -- a minimap2 host reads or builds its index between hardware_init (main.c:367) and the first chaining call (main.c:371-406).
 * Every entry that needs the device waits for that thread first; a failure shows there (and in mm2c_init_wait) as MM2C_E_NODEVICE with the reason, the way
 * a runtime error of the reference surfaces at the call (chain_hardware.cpp:208-235).  mm2c_init_wait: 0 once the library is ready.  mm2c_warm_up: loads
 * the code objects onto every configured device now instead of at each translation unit's first launch (what the asynchronous form does after its init). */
int  mm2c_init_async(int device_ordinal);
int  mm2c_init_wait(void);
int  mm2c_warm_up(void);
/* Several devices in one process (the reference scaffolds NUM_HW_KERNELS command queues / buffer sets / locks, chain_hardware.cpp:9-23,
 * chain_hardware.h:57): mm2c_init_devices instead of mm2c_init.  ordinals[0] is the primary device (plans run there); the per-read entries (run_chaining_on_hw, mm_chain_dp,
 * mm2c_chain_task_host) go to the device slot with the least work inside it, every slot with a call combiner of its own (mm2c_get_slot_stats); the host-batch entries (mm2c_chain_batch_host, mm2c_mm_chain_dp_batch_host, mm2c_seed_chain_batch_host)
 * split a batch of at least "multi_min_anchors" anchors (mm2c_tune, default 2^20) into one contiguous range of tasks per device with
 * about equal anchor counts (mm2c_split_tasks) and run the ranges side by side, each on its own stream set and arenas.  Chaining tasks
 * are independent (chain.c:42-45), so there is no exchange between devices.  An ordinal may be listed more than once. */
int  mm2c_init_devices(int n, const int *ordinals);
int  mm2c_device_count(void);
/* Host feed of several devices from one process: the worker thread of every device slot is persistent and pinned to the CPUs of the NUMA node its device hangs
 * off ("pin_workers", default 1), so that the page-locked staging buffers it allocates and the copies it drives stay on that socket.  mm2c_numa_cpulist reads
 * the mapping the way the workers do -- <sysfs_root>/bus/pci/devices/<pci bus id>/numa_node, then <sysfs_root>/devices/system/node/node<N>/cpulist -- and returns
 * the node (cpulist text in buf) or -1 when there is no NUMA information; it touches no device (sysfs_root "/sys"; tests hand it a made-up tree).
 * mm2c_slot_worker_node: the node slot's worker was pinned to, -1 = not started or not pinned. */
int  mm2c_numa_cpulist(const char *sysfs_root, const char *pci_bus_id, char *buf, size_t len);
int  mm2c_slot_worker_node(int slot);
int  mm2c_split_tasks(int64_t n_tasks, const int64_t *offsets, int n_parts, int64_t *bounds /* n_parts + 1 */);
void mm2c_shutdown(void);                     /* not while another thread is inside a compute entry */
const char *mm2c_last_error(void);            /* thread-local message of the last failing call */
int  mm2c_device_info(char *name, size_t name_len, int *cu_count, size_t *hbm_bytes);
/* which physical device the calling thread's library device is: its HIP ordinal, PCI bus id ("0000:c1:00.0") and architecture name.  A multi-GPU
 * launcher prints one per rank and refuses to report a scaling figure when two ranks sit on the same card (bench.py); the reference's counterpart is
 * the device list of hardware_init (chain_hardware.cpp:278-330: platform / device enumeration before the queues are made). */
int  mm2c_device_identity(int *ordinal, char *pci_bus_id, size_t bus_len, char *arch, size_t arch_len);
/* tuning knobs (key, value): "ring_class" 3 = the tile-aligned DP kernel (default; env MM2C_RING_CLASS; the segment / cDNA variant runs in the
 * first-generation kernel, which is faster for it), 4 = the tile kernel for every variant, 0/1/2 = the first-generation kernel with
 * 256/512/1024 anchors of LDS ring per task; "far_ring" 1 = plans give tasks with the 32-bit LDS ring (see "compact_ring") whose scans are expected to go far beyond the 448-anchor
 * LDS ring of the tile kernel an instantiation with a ring twice as long (chosen per task by the prepass; default; env MM2C_FAR_RING), 0 = never,
 * 2 = every task; "epi_fused" 1 = the device epilogue keeps the per-anchor state of tasks of up to
 * 7 680 anchors in LDS (default; env MM2C_EPI_FUSED), 0 = in HBM for every task; "compact_ring" 1 = tasks whose query positions span at most 65535 - min(max_dist_x, max_dist_y) (reads of up to about 55-60 kb) run
 * an instantiation of the tile kernel whose LDS ring keeps the low 16 bits of x and q only (16 tiles of look-back in the LDS of 8; default; env MM2C_COMPACT_RING),
 * 0 = never; "split_streams" 1 = a plan whose tasks differ in size runs the instantiations its batch is split over side by side on two streams (default;
 * env MM2C_SPLIT_STREAMS), 2 = every plan, 0 = never; "wide_share_threshold" = when the tasks that need the 32-bit ring hold more than this percentage of the
 * batch's anchors every task takes it (default 40); "force_tab" 1 = the tile kernel reads the gap
 * cost from its LDS table also when gap_scale is 1 (default 0: computed; tests); "seg_min" = shortest piece (anchors) a task is cut into at
 * empty-window positions (default 256, 0 = never cut); "plan_cut" 0/1 = plans cut their tasks of at least "plan_cut_min" anchors (default
 * 8192) into such pieces on the device before the DP (default 1); "pipeline_chunk_anchors" = chunk size of the two-stream pipeline used for
 * host batches of at least twice that size (default 20 Mi anchors); "multi_min_anchors" = smallest host batch that is split across the
 * devices of mm2c_init_devices (default 2^20); "trim" = give the cached device memory back to the runtime.  Results never depend on a knob.  "coop_waves" > 1 (default 16, the only width built: any value above 1 means 16) = a host-buffer pass of at most "coop_max_tasks" (1024) pieces gives every piece a workgroup of
 * 16 waves that share its LDS rings (csrc/chain_dp_coop.h: candidates counted and the older tiles reduced in parallel, the exact scan only where the early exit of chain.c:231 can fire;
 * env MM2C_COOP_WAVES), 0 = one wave per piece always; "coop_plans" 1 = plans of few tasks take that kernel too (tests); "combiner_lanes" 1..16 = passes the call combiner of the per-read
 * entries may have in flight at once on each device (default 4; env MM2C_COMBINER_LANES), "combine_max_anchors" = a call of more anchors than this runs alone (env MM2C_COMBINE_MAX);
 * "packed_fp" 1 = plan tasks of the compact ring with at most 8192 anchors and a span sum of at most 131071 run an instantiation that keeps f and p of a ring anchor in one word
 * (four tiles of f / p in the LDS of two, deeper ones from a side array with one load; default; a plan that holds a task of more than 8192 anchors, or whose gap_scale is negative -- the gap cost is then a gain and f is not bounded by the span sum --,
 * runs without it, and mm2c_plan_last_variant says so), 0 = never;
 * "score_bound_exit" 1 = the hand-written loop of the tile kernel ends an anchor's scan once the largest f before its tile plus its span cannot beat its best (the rest of such a scan only
 * decides where the scan ends, chain.c:231: same f / p; default; a call with gap_scale < 0 runs without it, and the variant text says score_exit=0), 0 = never. */
int  mm2c_tune(const char *key, int value);
/* What mm2c_tune set, and the table it goes by (csrc/knobs.def: each knob's key, environment variable, range, default and meaning).  Neither needs a device.
 * mm2c_tune_get: the knob's current value and its default (either pointer may be NULL), so that a caller can put back what it found; MM2C_E_ARG for an unknown key
 * ("trim" is a command, not a knob).  mm2c_tune_key: key and environment variable of knob i = 0 .. n-1 (*env is NULL for a knob without one); MM2C_E_ARG beyond the table. */
int  mm2c_tune_get(const char *key, int64_t *value, int64_t *dflt);
int  mm2c_tune_key(int i, const char **key, const char **env);

/* HW/SW split model of the reference for this hardware (chain.c:80-81,101; constants in the form of chain_hardware.h:19-30 live in
 * include/mm2chain_split.h): hw_ms = k1_hw * n + k2_hw * total_subparts + c_hw for one synchronous per-read call into this library,
 * sw_ms = k_sw * total_trip_count + c_sw for chain.c's loop on one host core.  preset: "map-ont" or "asm20".  The library itself never
 * declines a task; a host that keeps the reference's predictor loads K1_HW .. C_SW (options.c:6,95-99) from here. */
int  mm2c_split_model(const char *preset, float *k1_hw, float *k2_hw, float *c_hw, float *k_sw, float *c_sw);

/* defaults of `minimap2 -x map-ont` (options.c:24-31,93-99; map.c:305-316) */
void mm2c_params_map_ont(mm2c_params_t *p);
/* V2 = what the FPGA kernel computes for a run_chaining_on_hw call */
void mm2c_params_fpga_v2(mm2c_params_t *p, int32_t max_dist_x, int32_t max_dist_y, int32_t bw, int32_t q_span);

/* ---- batched, HBM-resident path ------------------------------------------------------------------------------ */
/*
 * A plan describes one batch of independent chaining tasks in CSR form: task k owns anchors
 * [offsets[k], offsets[k+1]) of the concatenated arrays.  Creating a plan uploads offsets and the
 * longest-first launch order and reserves the device workspace; it can be run many times.
 */
typedef struct mm2c_plan mm2c_plan_t;
mm2c_plan_t *mm2c_plan_create(const mm2c_params_t *par, int64_t n_tasks, const int64_t *h_offsets);
void mm2c_plan_destroy(mm2c_plan_t *plan);
int64_t mm2c_plan_total_anchors(const mm2c_plan_t *plan);

/* stream arguments: a hipStream_t passed as void*.  NULL is the HIP null stream (what a default-stream caller such as PyTorch works on,
 * so the call is ordered with the caller's own work); MM2C_STREAM_LIBRARY asks for the library's private non-blocking stream. */
#define MM2C_STREAM_LIBRARY ((void *)(intptr_t)-1)

/*
 * Enqueue the DP for every task of the plan on `stream`.  All pointers are DEVICE pointers: d_anchors[total] (16 B each), d_f[total], d_p[total].
 * d_avg_qspan is either NULL (the kernel computes avg_qspan_scaled per task exactly as chain.c:48-49) or
 * n_tasks floats.  p[] is task-relative, -1 = no predecessor, exactly as chain.c:236.  Asynchronous.
 * A plan owns one workspace: do not run the same plan concurrently with itself (different plans and different streams are fine).
 */
int mm2c_plan_run_device(mm2c_plan_t *plan, const void *d_anchors, const float *d_avg_qspan,
                         int32_t *d_f, int32_t *d_p, void *stream);

/* Task sizes that only the device knows (anchors made by mm2c_seedplan_run_device_skip): from now on the plan's kernels take the CSR
 * offsets from d_offsets (n_tasks + 1 entries, device memory, offsets[0] = 0, every task no longer than the plan was created for);
 * NULL goes back to the plan's own.  The buffers handed to the run / chains entries keep the plan's (capacity) extents. */
int mm2c_plan_set_device_offsets(mm2c_plan_t *plan, const int64_t *d_offsets);

/* Chaining distances per task: from now on task k is chained with max_dist_x = d_dists[2 k] and max_dist_y = d_dists[2 k + 1] (2 * n_tasks int32 in device
 * memory, read when a run executes) in the place of par's two scalars.  The values should be >= 0: they cannot be checked on the host, so the kernels take a
 * negative one as 0 (par's own max_dist_x < 0 is refused) -- the window start (chain.c:192), the filters of chain.c:202-206 and
 * the places where a long task is cut into pieces all go by the task's own pair.  Such a run takes the general variant of the one-wave kernel
 * (chain_dp_wave<.., GEN=1, ..>, as mm2c_plan_last_variant says), which computes the same f / p as the simple one for single-segment tasks; the tile and the
 * cooperative kernels stay per call.  NULL goes back to par's scalars and to the kernels the plan ran before. */
int mm2c_plan_set_task_dists(mm2c_plan_t *plan, const int32_t *d_dists);

/* The same with the extent of every buffer stated (elements, not bytes): MM2C_E_TOOBIG when one is shorter than the plan needs, the way
 * the reference refuses n > BUFFER_N (chain_hardware.cpp:34-37).  The entries without _n trust the caller. */
int mm2c_plan_run_device_n(mm2c_plan_t *plan, const void *d_anchors, int64_t n_anchors, const float *d_avg_qspan, int64_t n_avg,
                           int32_t *d_f, int64_t n_f, int32_t *d_p, int64_t n_p, void *stream);

/* milliseconds between HIP events recorded (on the run's stream) around the DP kernel (chain_dp_wave) of the most
 * recent mm2c_plan_run_device; synchronises on the end event.  _prepass_ms: the same for the window-start kernel
 * (chain_window_start) that runs just before it. */
int mm2c_plan_last_kernel_ms(mm2c_plan_t *plan, float *ms);
/* Round 6: which of the two DP kernels took the pieces of the most recent run.  A batch of few long pieces -- fewer pieces than the GPU has wave slots, BASELINE config 5's
 * long reads -- runs with sixteen (or eight) waves per piece (chain_dp_coop, the analogue of the reference's one deep pipeline per task, device/minimap2_opencl.cl:49,71), anything
 * else with one wave per piece; with long tasks cut into pieces on the device the choice is made there (chain_route), so this call waits for the run and reads it back.
 * pieces = the tasks, or the pieces they were cut into; one_wave_pieces + coop_pieces = pieces.  mm2c_tune("coop_plans", 0 | 1 | 2): never / every small plan / per run. */
int mm2c_plan_last_route(mm2c_plan_t *plan, int64_t *pieces, int64_t *one_wave_pieces, int64_t *coop_pieces);
/* The rule itself (pure arithmetic, no device): waves per piece -- 16, 8 or 1 -- that a batch of `pieces` pieces, the longest of `longest` anchors, `total` anchors in all, is
 * given under "coop_plans" 2.  One wave per piece is bound by its longest piece (about 0.7 us per anchor), several waves per piece by the anchors a CU is dealt (about
 * 0.1 us per anchor: total / 256 + the longest piece at worst): several when pieces <= 2048 and 1450 * longest > total; of these sixteen (one workgroup per CU) up to
 * mm2c_tune("coop_w8_above", 256) pieces, eight (two workgroups per CU, each filling the other's waits) beyond -- where pieces of at least 8 192 anchors also take
 * them when 2300 * longest > total (profiles/r6_long_reads.md). */
int mm2c_route_pieces(int64_t pieces, int64_t longest, int64_t total);
/* Which kernel instantiation the most recent mm2c_plan_run_device launched for the tasks' first pass, as text, e.g.
 * "chain_dp_tile<NX=8,NF=2,SKIP=1,GEN=0,GS1=1,FAR=1,TAB=0> loop=asm classes=1 cut=0" (loop=asm: the hand-written per-tile loop, loop=c++: its
 * C++ restatement; chain_dp_wave<...>: the first-generation kernel).  For tests and logs: results never depend on the instantiation. */
int mm2c_plan_last_variant(mm2c_plan_t *plan, char *buf, size_t len);
/* the class byte the prepass of the last run gave each task of the plan (n = its number of tasks): bit 0 the long LDS ring, bit 1 the 32-bit x / q ring,
 * bit 2 a query position beyond the q24 ring, bit 3 the task fits the packed f / p ring ("packed_fp") -- which instantiation took which task (tests) */
int mm2c_plan_last_classes(mm2c_plan_t *plan, unsigned char *cls, int64_t n);
/* the same text for the last DP launch of a host-buffer entry (mm2c_chain_task_host, mm2c_chain_batch_host, mm2c_mm_chain_dp_batch_host), process-wide:
 * those entries give their passes the prepass classes too, so tasks whose q values allow it take the compact ring there as in plans */
int  mm2c_last_host_variant(char *buf, size_t len);
/* test instrumentation: how often the hand-written anchor loop of the DP kernel (csrc/chain_dp_tile.h, MM2C_SCAN_TILE_ASM) passed each of its labels, 8 rows
 * (compact ring << 2 | gap-cost table << 1 | far instantiation) x 32 label bits (MM2C_LB_*), since the last reset.  Only the build with -DMM2C_LABEL_COUNT
 * (minimap2-fpga_amd/variants/labelcount.so, loaded through MM2C_LIB_PATH by tests/test_gpu_labels.py) counts; the shipped library returns MM2C_E_ARG. */
int  mm2c_debug_label_hits(unsigned long long *hits /* 256 */, int reset);
int mm2c_plan_last_prepass_ms(mm2c_plan_t *plan, float *ms);

/*
 * The reference's HW/SW prediction pass (chain.c:53-78) for every task of the plan, on the GPU: num_subparts[total]
 * (uint8, what chain.c:76 stores and run_chaining_on_hw receives), and per task total_subparts (chain.c:77) and
 * total_trip_count (chain.c:69), the inputs of the two linear time models of chain.c:80-81.  Any output may be NULL.
 */
int mm2c_plan_predict_device(mm2c_plan_t *plan, const void *d_anchors, uint8_t *d_num_subparts,
                             int64_t *d_total_subparts, int64_t *d_total_trip_count, void *stream);

/* ---- host-buffer paths (PCIe included) ---------------------------------------------------------------------- */
/* whole batch from pageable host memory: staging, H2D, DP, D2H, sync */
int mm2c_chain_batch_host(const mm2c_params_t *par, int64_t n_tasks, const int64_t *h_offsets,
                          const mm2c_anchor_t *h_anchors, const float *h_avg_qspan /* or NULL */,
                          int32_t *h_f, int32_t *h_p);

/* page-locked host memory for callers that want full PCIe rate on the host-buffer paths (any pointer works there; pageable
 * memory is staged by the runtime at roughly a quarter of the rate).  NULL on failure. */
void *mm2c_pinned_alloc(size_t bytes);
void  mm2c_pinned_free(void *ptr);

/*
 * THE LARGEST TASK (round 6).  The reference sizes its device buffers for BUFFER_N = 332 000 000 / 2 / 32 = 5 187 500 anchors per call (chain_hardware.h:62-64) and ends
 * the process on a longer one (chain_hardware.cpp:34-37).  Here buffers grow on demand and indices, stamps and p bases are 32 bits wide:
 *   - every entry that takes tasks (plans, batch entries, mm2c_chain_task_host[_pred], mm_chain_dp) accepts a task of up to MM2C_MAX_TASK_ANCHORS anchors and answers
 *     MM2C_E_TOOBIG for a longer one -- nothing wraps;
 *   - the device epilogue (mm2c_plan_chains_device, mm2c_mm_chain_dp_batch_host) takes batches (or pipeline chunks) of fewer than 2^31 anchors in all;
 *   - run_chaining_on_hw (the reference's symbol) additionally keeps the reference's own contract for the size its host states in hardware_init(buf_size, ...):
 *     n > buf_size -> "Error: The size of the call ..." on stderr and exit(1).
 * Tested at the reference's limit: one task of 5 187 500 anchors through run_chaining_on_hw, one of 2 000 000 through mm2c_chain_task_host, element-wise against the
 * oracle (tests/test_gpu_long_reads.py).
 */
#define MM2C_MAX_TASK_ANCHORS ((int64_t)2147483582)   /* 2^31 - 66 */

/*
 * One task, synchronous, V1 (stock CPU) semantics: the EXTENDED form of run_chaining_on_hw
 * (chain_hardware.h:68) that also carries max_skip / max_iter / gap_scale / is_cdna / n_segs, which the
 * reference interface cannot express.  Re-entrant from many host threads (map.c:561); `tid` as chain.c:103.
 * Always returns 0 (= "computed on device", chain_hardware.cpp:195) or a negative error; never 1.
 */
int mm2c_chain_task_host(const mm2c_params_t *par, int64_t n, const mm2c_anchor_t *a, float avg_qspan_scaled,
                         int32_t *f, int32_t *p, int tid);

/*
 * The same call with the reference's busy protocol (chain_hardware.cpp:54-75, PROCESS_ON_SW_IF_HW_BUSY, chain_hardware.h:50): the caller hands in the two
 * predictions chain.c:80-81 computes (milliseconds).  OFF BY DEFAULT since round 6 ("decline_when_busy" 0: every call is accepted) -- a chain.o built without
 * PROCESS_ON_SW_IF_HW_BUSY ignores the answer 1 (chain.c:105,163-169) and would chain from uninitialised f / p, and on the measured end-to-end run no decline rule
 * beat never declining (profiles/r6_per_read.md).  A host that HAS the software loop opts in (environment MM2C_DECLINE_WHEN_BUSY or mm2c_tune):
 *   1: declined when (calls inside the device slot / passes it runs at once + 1) x (what a pass of that slot has taken lately) > sw_time_pred -- the measured thing;
 *   2: round 5's rule: (predicted device time booked on the slot) / (passes at once) + hw_time_pred >= sw_time_pred;
 * the slots are tried from tid % n, the call RUNS on the slot that accepted it (chain_hardware.cpp:58-72), and when none will it returns 1 = "declined": nothing was
 * computed, f / p are untouched, the caller runs its own loop (chain.c:106,112-164).  This library's own mm_chain_dp (path B) never declines -- it has no software DP.
 * Predictions that are not both positive never decline.
 */
int mm2c_chain_task_host_pred(const mm2c_params_t *par, int64_t n, const mm2c_anchor_t *a, float avg_qspan_scaled,
                              int32_t *f, int32_t *p, int tid, float hw_time_pred, float sw_time_pred);

/* Per device slot (the order of mm2c_init_devices / MM2C_DEVICES; slot 0 = the primary device): what its call combiner has served since mm2c_init --
 * the reference keeps a queue, a lock and a buffer set per kernel (chain_hardware.cpp:9-23); here every device has its own, and a per-read call goes to
 * the slot with the least anchors outstanding.  declined: calls mm2c_chain_task_host_pred turned away (counted on slot 0). */
typedef struct { int32_t device; int32_t reserved; uint64_t passes, calls, anchors, declined; } mm2c_slot_stats_t;
int mm2c_get_slot_stats(int slot, mm2c_slot_stats_t *out);
/* the routing rule on its own (pure; no device is touched): given the anchors outstanding on each of n_slots device slots, the slot a call from worker `tid` goes to
 * -- the least loaded one, ties to the first such slot at or after tid % n_slots (so idle devices are taken in turn, chain_hardware.cpp:58-72 scans its kernels
 * from 0 instead).  A negative tid counts as 0. */
int mm2c_route_slot(int n_slots, const int64_t *outstanding, int tid);

/* ---- host mirror of the reference function around the path ------------------------------------------------------ */
/*
 * mm_chain_dp with the reference's exact signature and ownership rules (mmpriv.h:65, chain.c:29-423): frees `a`
 * with kfree(km, a); returns b[] and *_u allocated with kmalloc(km, ...).  The DP (f[], p[]) runs on the GPU
 * through mm2c_chain_task_host; v[] and the backtrack run on the calling thread.  Needs the host program's
 * kmalloc/kfree (kalloc.h:14,17) at link/load time.  Declared here with mm2c_anchor_t == mm128_t.
 */
#ifndef MM2C_NO_MM_CHAIN_DP_DECL   /* define it in a host that already includes mmpriv.h (same function, mm128_t spelling) */
mm2c_anchor_t *mm_chain_dp(int max_dist_x, int max_dist_y, int bw, int max_skip, int max_iter, int min_cnt,
                           int min_sc, float gap_scale, int is_cdna, int n_segs, int64_t n, mm2c_anchor_t *a,
                           int *n_u_, uint64_t **_u, void *km, int tid);
#endif

/* ---- whole mm_chain_dp for a batch: DP + epilogue (chain.c:106-111,348-422) ----
 * Outputs are compact: the chains of task k are u[u_off[k] .. u_off[k+1]) (score<<32 | count, in the order mm_chain_dp returns
 * them, chain.c:385-388,406-420) and their anchors b[b_off[k] .. b_off[k+1]); u_off / b_off have n_tasks+1 entries, u and b need
 * room for every anchor of the batch.  Results equal mm_chain_dp called task by task. */

/* the epilogue on the GPU, after mm2c_plan_run_device on the same stream; all pointers are device memory; needs
 * mm2c_plan_total_anchors < 2^31 */
int mm2c_plan_chains_device(mm2c_plan_t *plan, const void *d_anchors, const int32_t *d_f, const int32_t *d_p, int min_cnt, int min_sc,
                            int64_t *d_u_off, uint64_t *d_u, int64_t *d_b_off, void *d_b, void *stream);
int mm2c_plan_chains_device_n(mm2c_plan_t *plan, const void *d_anchors, int64_t n_anchors, const int32_t *d_f, int64_t n_f, const int32_t *d_p, int64_t n_p,
                              int min_cnt, int min_sc, int64_t *d_u_off, int64_t n_u_off, uint64_t *d_u, int64_t n_u, int64_t *d_b_off, int64_t n_b_off,
                              void *d_b, int64_t n_b, void *stream);
int mm2c_plan_last_epilogue_ms(mm2c_plan_t *plan, float *ms);

/* the epilogue on n_threads host threads from f[] / p[] in host memory (what the reference does on the calling thread) */
int mm2c_chain_epilogue_host(int min_cnt, int min_sc, int64_t n_tasks, const int64_t *h_offsets, const mm2c_anchor_t *h_anchors,
                             const int32_t *h_f, const int32_t *h_p, int n_threads, int64_t *u_off, uint64_t *u, int64_t *b_off,
                             mm2c_anchor_t *b);

/* host buffers in, chains out.  epilogue_threads == 0: DP and epilogue on the GPU, only chains come back over PCIe;
 * epilogue_threads > 0: DP on the GPU, f[] / p[] come back and the epilogue runs on that many host threads. */
int mm2c_mm_chain_dp_batch_host(const mm2c_params_t *par, int min_cnt, int min_sc, int64_t n_tasks, const int64_t *h_offsets,
                                const mm2c_anchor_t *h_anchors, int epilogue_threads, int64_t *u_off, uint64_t *u, int64_t *b_off,
                                mm2c_anchor_t *b);

/* ---- chains -> regions on the GPU (mm_gen_regs, hit.c:52-88: the line of mm_map_frag behind mm_chain_dp, map.c:344) ----
 * mm2c_reg_t has the fields of mm_reg1_t (minimap.h:85-100) in the same order at the same offsets, 80 bytes: the bit-field word is `flags`
 * (mapq bits 0-7, split bits 8-9, rev bit 10, ... as GCC lays out minimap.h:96) and the pointer p is a uint64_t, always 0 here.  The regions the
 * entries below write are, byte for byte, the calloc'ed array mm_gen_regs returns: a host may memcpy them into its mm_reg1_t[]. */
typedef struct {
	int32_t id, cnt, rid, score;
	int32_t qs, qe, rs, re;
	int32_t parent, subsc;
	int32_t as;
	int32_t mlen, blen;
	int32_t n_sub;
	int32_t score0;
	uint32_t flags;
	uint32_t hash;
	float div;
	uint64_t p;
} mm2c_reg_t;
#define MM2C_REG_REV_BIT 10
#define MM2C_REG_SPLIT_INV_BIT 24

/* A plan for batches of up to n_reads reads, n_u_cap chains and n_b_cap chain anchors in all (its scratch, 64 bytes per chain, is sized from the capacities).
 * The input is the compact output of the device epilogue (mm2c_plan_chains_device): d_u_off / d_b_off (n_reads + 1 entries each), d_u, d_b, plus per
 * read d_qlen (the qlen argument of mm_gen_regs: the summed length of the fragment's segments) and d_hash (map.c:290-292, mm2c_read_hash).  The regions
 * of read r are d_regs[u_off[r] .. u_off[r+1]) in the reference's order: regions are indexed like u, and d_regs (8-byte aligned) has room for n_u_cap of
 * them.  All pointers are device memory; the call is asynchronous on `stream` (NULL / MM2C_STREAM_LIBRARY as everywhere) and may follow
 * mm2c_plan_chains_device on the same stream with that call's outputs, the host never having seen u_off.
 * Preconditions (mm_chain_dp guarantees them): every chain has cnt = (int32_t)u[i] >= 1, and the counts of a read add up to b_off[r+1] - b_off[r].
 * A read that breaks them -- or whose offsets leave the capacities -- gets unspecified regions and mm2c_regplan_check answers MM2C_E_ARG; nothing is read
 * outside [b_off[r], b_off[r+1]) for read r whatever u holds, and the regions of the other reads are not affected.  mm_mark_alt / mm_hit_sort (indices
 * with ALT contigs) are not part of this. */
typedef struct mm2c_regplan mm2c_regplan_t;
mm2c_regplan_t *mm2c_regplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_b_cap);
void mm2c_regplan_destroy(mm2c_regplan_t *plan);
int mm2c_regplan_run_device(mm2c_regplan_t *plan, const int64_t *d_u_off, const uint64_t *d_u, const int64_t *d_b_off, const void *d_b,
                            const int32_t *d_qlen, const uint32_t *d_hash, mm2c_reg_t *d_regs, void *stream);
/* waits for the last run; MM2C_E_ARG if a read's counts disagreed.  *n_reads_with_ties: reads in which two chains had the same sort key (hit.c:65) */
int mm2c_regplan_check(mm2c_regplan_t *plan, int64_t *n_reads_with_ties);
/* milliseconds of the last run between HIP events on its stream; _kernel_ms: the same for the sort kernel (keys, order, fields) and the fill kernel (mlen, blen) */
int mm2c_regplan_last_ms(mm2c_regplan_t *plan, float *ms);
int mm2c_regplan_last_kernel_ms(mm2c_regplan_t *plan, float *sort_ms, float *fill_ms);
/* host arrays in, regions out (regs: room for u_off[n_reads] - u_off[0] regions).  Checks the offsets, cnt >= 1 and the count sums first (MM2C_E_ARG,
 * before any device work), then uploads, runs, downloads and waits. */
int mm2c_gen_regs_batch_host(int64_t n_reads, const int64_t *u_off, const uint64_t *u, const int64_t *b_off, const mm2c_anchor_t *b,
                             const int32_t *qlen, const uint32_t *hash, mm2c_reg_t *regs);
/* the hash mm_map_frag hands to mm_gen_regs (map.c:290-292): X31 string hash of the read name (0 for NULL) ^ (Wang(qlen_sum) + Wang(seed)), then Wang again.
 * seed = mm_mapopt_t::seed (11 by default).  Host only, needs no device. */
uint32_t mm2c_read_hash(const char *qname, int32_t qlen_sum, int32_t seed);

/* ---- regions -> hits on the GPU (chain_post for one-segment reads, map.c:249-258: mm_set_parent hit.c:125-186, then mm_select_sub hit.c:255-272 with
 * mm_sync_regs / mm_set_sam_pri hit.c:220-253) ----
 * Which regions are primary, which stay as secondary, and the subsc / n_sub the mapping quality is later made of.  The regions of read r are
 * d_regs_in[u_off[r] .. u_off[r+1]) exactly as mm2c_regplan_run_device wrote them; the same u_off indexes d_regs_out, whose first d_n_out[r] entries from
 * u_off[r] on are, byte for byte, the array the reference holds after the two calls on that read (d_n_out[r] is *n_ after mm_select_sub); the entries behind
 * them up to u_off[r+1] are unspecified.  With pri_ratio <= 0 mm_select_sub does nothing: n_out = n and the regions carry mm_set_parent's changes only.
 * The fields p, is_alt and inv are always 0 in these regions, so the reference's branches on them (hit.c:168, 171-176, 261, 266-267: ALT contigs, alignment
 * extras, inversions) are dead and are not built; sub_diff and alt_diff_frac therefore have no counterpart in mm2c_hit_opt_t.
 * The float tests (hit.c:165, :263) are evaluated in IEEE single precision as written.  mm_select_sub compacts in place while it still reads r[p]: a child is
 * judged against whatever region lies at its parent's position by then, and so it is here.
 * d_regs_out must not alias d_regs_in; both 8-byte aligned with room for n_u_cap regions, d_n_out for n_reads.  The call is asynchronous on `stream` (NULL /
 * MM2C_STREAM_LIBRARY as everywhere) and may follow mm2c_regplan_run_device on the same stream, the host never having seen u_off.  A read whose offsets leave
 * the capacities touches nothing and mm2c_hitplan_check answers MM2C_E_ARG.  Reads of up to MM2C_HIT_LDS_REGIONS regions are worked in on-chip memory, longer
 * ones in the plan's scratch (64 bytes per region), with the same result.  mm_select_sub_multi (fragments of several segments) is the plan's second mode,
 * mm2c_hitplan_run_device_multi below. */
typedef struct {
	float mask_level; int32_t mask_len; int32_t hard_mask_level;   /* mm_set_parent: opt->mask_level, opt->mask_len, opt->flag & MM_F_HARD_MLEVEL */
	float pri_ratio; int32_t min_diff; int32_t best_n;             /* mm_select_sub: opt->pri_ratio, mi->k * 2, opt->best_n */
} mm2c_hit_opt_t;
#define MM2C_REG_SAM_PRI_BIT 12
#define MM2C_REG_PROPER_FRAG_BIT 13    /* set by the pair plan (mm_pair, pe.c:138) */
#define MM2C_REG_PE_THRU_BIT 14        /* set by the pair plan (mm_set_pe_thru, pe.c:60) */
#define MM2C_HIT_LDS_REGIONS 128
typedef struct mm2c_hitplan mm2c_hitplan_t;
mm2c_hitplan_t *mm2c_hitplan_create(int64_t n_reads, int64_t n_u_cap);
void mm2c_hitplan_destroy(mm2c_hitplan_t *plan);
int mm2c_hitplan_run_device(mm2c_hitplan_t *plan, const mm2c_hit_opt_t *opt, const int64_t *d_u_off, const mm2c_reg_t *d_regs_in,
                            mm2c_reg_t *d_regs_out, int32_t *d_n_out, void *stream);
/* waits for the last run; MM2C_E_ARG if a read's offsets left the capacities.  *n_hits_total: the sum of n_out */
int mm2c_hitplan_check(mm2c_hitplan_t *plan, int64_t *n_hits_total);
/* milliseconds of the last run between HIP events on its stream */
int mm2c_hitplan_last_ms(mm2c_hitplan_t *plan, float *ms);
/* host arrays in, hits out (regs_out: room for u_off[n_reads] - u_off[0] regions, read r from u_off[r] - u_off[0] on).  Checks the offsets first
 * (MM2C_E_ARG, before any device work), then uploads, runs, downloads and waits. */
int mm2c_select_hits_batch_host(int64_t n_reads, const mm2c_hit_opt_t *opt, const int64_t *u_off, const mm2c_reg_t *regs_in, mm2c_reg_t *regs_out,
                                int32_t *n_out);
/* The second mode, for fragments of several segments (map.c:252-254): mm_set_parent as above, then mm_select_sub_multi (pe.c:6-43) in the place of mm_select_sub.
 * A "read" of the plan is a fragment; d_seg_len holds the qlens, fragment-major (n_segs per fragment; read only when n_segs == 2), d_gap_ref the max_chain_gap_ref
 * of every fragment (map.c:309-314: under -x sr it is max(max_frag_len - qlen_sum, max_gap) and differs from fragment to fragment; the first of each pair of
 * mm2c_read_result_task_dists), or NULL for mopt->max_gap_ref everywhere.  Everything is as pe.c writes it: max_dist = n_segs == 2 ? qlens[0] + qlens[1] +
 * max_gap_ref : 0 in wrapping int; score + min_diff >= parent's score first, an integer test; then q->re - p->rs < max_dist && p->re - q->rs < max_dist (strict,
 * integer) with equal rev and rid choose pri1, otherwise pri_ratio, or pri2 when the parent spans both segments (qs < qlens[0] < qe) and the child does not; the
 * score test is (float)score >= (float)pscore * ratio in IEEE single precision; the parent is read from the array being compacted in place; every secondary that
 * passed counts against best_n, kept or not; there is no identical-hit test; mm_sync_regs and sam_pri only when something was dropped; with pri_ratio <= 0 nothing
 * happens beyond mm_set_parent.  mm2c_hitplan_check and _last_ms serve both modes. */
#define MM2C_MAX_SEG 255                                           /* MM_MAX_SEG */
typedef struct { float pri1, pri2; int32_t n_segs; int32_t max_gap_ref; } mm2c_hit_multi_opt_t;   /* map.c:254: 0.2f, 0.7f */
int mm2c_hitplan_run_device_multi(mm2c_hitplan_t *plan, const mm2c_hit_opt_t *opt, const mm2c_hit_multi_opt_t *mopt, const int64_t *d_u_off,
                                  const int32_t *d_seg_len, const int32_t *d_gap_ref, const mm2c_reg_t *d_regs_in, mm2c_reg_t *d_regs_out, int32_t *d_n_out,
                                  void *stream);
/* host arrays, as mm2c_select_hits_batch_host: seg_len n_frags * n_segs, gap_ref n_frags or NULL */
int mm2c_select_hits_multi_batch_host(int64_t n_frags, const mm2c_hit_opt_t *opt, const mm2c_hit_multi_opt_t *mopt, const int64_t *u_off, const int32_t *seg_len,
                                      const int32_t *gap_ref, const mm2c_reg_t *regs_in, mm2c_reg_t *regs_out, int32_t *n_out);

/* ---- hits -> mapping quality on the GPU (the rest of chain_post and the mapq of one-segment reads mapped without CIGAR: mm_join_long map.c:255-256,
 * hit.c:295-371; mm_set_mapq map.c:361, hit.c:463-508) ----
 * The hits of read r are d_regs_in[u_off[r] .. u_off[r] + d_n_in[r]) exactly as mm2c_hitplan_run_device wrote them (its d_regs_out / d_n_out), its chain anchors
 * d_b[b_off[r] .. b_off[r+1]) as the region plan got them; d_qlen and d_rep_len (collect_matches' rep_len, map.c:342) are per read.  The first d_n_out[r] entries
 * of d_regs_out from u_off[r] on are, byte for byte, the array the reference holds after mm_join_long (only with do_join) and
 * mm_set_mapq(km, n, regs, min_chain_score, match_sc, rep_len[r], is_sr); the entries behind them are unspecified.  p, inv and is_alt are always 0 in these regions,
 * so hit.c:484-491, 494-496, 504 and mm_set_inv_mapq are dead and not built, and match_sc / is_sr have no counterpart here.  `div` passes through: mm_est_err
 * (map.c:357), which writes nothing else, is the est-err plan's further down (its counts on the device, its one pow on the host).  Every other field of the
 * final mm_reg1_t is the reference's.
 * Anchors: mm_join_long starts with mm_squeeze_a whenever a read has two hits or more -- the anchors of the hits that are left, in ascending as, are packed to the
 * front of the read's a[] and as is renumbered -- and a join sets MM_SEED_LONG_JOIN (bit 40 of y) on the first anchor of the absorbed chain.  The as in d_regs_out
 * are always the reference's (squeezed).  With d_b_out, read r's segment from b_off[r] on holds d_n_b_out[r] anchors that are the reference's a[] byte for byte:
 * the sum of cnt for a squeezed read, the whole segment for a read of fewer than two hits or with do_join == 0.  With d_b_out == NULL (and d_n_b_out NULL with
 * it) no anchor is copied and the join bit is recorded nowhere; a host that needs neither a[] nor the bit saves the copy.  d_b is never written.
 * The logarithms: mm_set_mapq calls logf on two integers, and libms differ in the last bit.  The plan holds a table L[i] = logf((float)i), 0 <= i <= max_log_arg
 * (at most MM2C_MAPQ_MAX_LOG_ARG, where every integer still is a float), which the HOST fills at creation by calling its own logf: what the reference computes on
 * that host, on whatever libm is installed.  The float arithmetic around the lookup is evaluated in IEEE single precision as written.  A primary hit whose score
 * or n_sub + 1 exceeds max_log_arg gets mapq 0 and is counted; mm2c_mapqplan_check then answers MM2C_E_TOOBIG with the count.  Nothing wraps, nothing else changes.
 * Preconditions (the hit plan guarantees them): id == index in every read, cnt >= 1, chains that do not overlap in a[].  The reference sizes mm_sync_regs' table
 * by the largest id left and reads beyond it when a dropped parent has a larger one; here such a parent gives MM_PARENT_UNSET.
 * d_regs_out must not alias d_regs_in, nor d_b_out d_b; regions 8-byte, anchors 16-byte aligned.  Asynchronous on `stream`; may follow mm2c_hitplan_run_device
 * on the same stream, the host never having seen u_off or n_out.  A read whose u_off / b_off / n_in leave the capacities or each other, or a hit of which leaves
 * the read's anchors, touches nothing and mm2c_mapqplan_check answers MM2C_E_ARG; the reads beside it are not affected. */
typedef struct {
	int32_t do_join;                                            /* !(opt->flag & (MM_F_SPLICE|MM_F_SR|MM_F_NO_LJOIN)), map.c:255 */
	int32_t max_join_long, max_join_short, min_join_flank_sc;   /* options.c:38-40 */
	float   min_join_flank_ratio;                               /* options.c:41 */
	int32_t min_cnt;                                            /* mm_filter_regs, hit.c:280 */
	int32_t min_chain_score;                                    /* mm_set_mapq's min_chain_sc */
} mm2c_mapq_opt_t;
#define MM2C_MAPQ_MAX_LOG_ARG 16777215
#define MM2C_SEED_LONG_JOIN_BIT 40
typedef struct mm2c_mapqplan mm2c_mapqplan_t;
mm2c_mapqplan_t *mm2c_mapqplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_b_cap, int32_t max_log_arg);
void mm2c_mapqplan_destroy(mm2c_mapqplan_t *plan);
int mm2c_mapqplan_run_device(mm2c_mapqplan_t *plan, const mm2c_mapq_opt_t *opt, const int64_t *d_u_off, const mm2c_reg_t *d_regs_in, const int32_t *d_n_in,
                             const int64_t *d_b_off, const void *d_b, const int32_t *d_qlen, const int32_t *d_rep_len, mm2c_reg_t *d_regs_out,
                             int32_t *d_n_out, void *d_b_out, int64_t *d_n_b_out, void *stream);
/* waits for the last run.  MM2C_E_ARG if a read was refused for its offsets; else MM2C_E_TOOBIG if a primary lay beyond the table.  *n_joined: joins made;
 * *n_beyond_table: primaries beyond the table (both filled in either way; either pointer may be NULL) */
int mm2c_mapqplan_check(mm2c_mapqplan_t *plan, int64_t *n_joined, int64_t *n_beyond_table);
/* milliseconds of the last run between HIP events on its stream; _kernel_ms: the same for mapq_join and for mapq_gather (0 when no anchors were asked for) */
int mm2c_mapqplan_last_ms(mm2c_mapqplan_t *plan, float *ms);
int mm2c_mapqplan_last_kernel_ms(mm2c_mapqplan_t *plan, float *join_ms, float *gather_ms);
/* host arrays in and out (regs_out: room for u_off[n_reads] - u_off[0] regions, read r from u_off[r] - u_off[0] on; b_out / n_b_out: NULL, or room for
 * b_off[n_reads] - b_off[0] anchors and n_reads counts).  Checks the offsets and n_in first (MM2C_E_ARG, before any device work), then uploads, runs,
 * downloads and waits; with MM2C_E_TOOBIG the outputs are complete all the same. */
int mm2c_join_mapq_batch_host(int64_t n_reads, const mm2c_mapq_opt_t *opt, int32_t max_log_arg, const int64_t *u_off, const mm2c_reg_t *regs_in,
                              const int32_t *n_in, const int64_t *b_off, const mm2c_anchor_t *b, const int32_t *qlen, const int32_t *rep_len,
                              mm2c_reg_t *regs_out, int32_t *n_out, mm2c_anchor_t *b_out, int64_t *n_b_out);

/* ---- chain-anchor divergence on the GPU (mm_est_err map.c:357, esterr.c: the `div` of a final region, the dv:f: tag) ----
 * mm_est_err writes only div; it reads the read's mini_pos (q_span << 32 | q_pos of every kept minimizer, as mm2c_sketch_match_batch and the reads-in entries
 * lay it out: mini_off / mini_pos) and the chain anchors of every final region.  The plan stands behind the mapq plan on the same stream: its regions are that
 * plan's d_regs_out / d_n_out, its anchors that plan's d_b_out (with do_join == 0 the device epilogue's d_b does as well), both read-only here.
 * The split: div = n_match >= n_tot ? 0 : (float)(1 - pow((double)n_match / n_tot, 1.0 / avg_k)) (esterr.c:62) calls pow, libms differ in the last bit, and
 * 1 - p cancels, so a device pow would need a tolerance nobody can derive.  The device therefore makes what is exact by construction -- per region the integers
 * d_err[u_off[r] + i] = {n_match, n_tot}, per read the float d_avg_k[r] = (float)sum of spans / n (one integer-to-float conversion, one IEEE division) -- and
 * mm2c_est_err_div applies the one line with the HOST's own pow: what the reference's esterr.o computes on that host.  There is no device-side div.
 *   n_match >= 1 : the counts of esterr.c:53-61
 *   n_match == 0 : div = -1 (cnt == 0, or the first anchor of the walk is not in mini_pos, esterr.c:44-51)
 *   n_match == -1: the read has no mini_pos; esterr.c:36 returns before it touches anything and div stays as it was
 * Entries behind d_n_in[r] are unspecified.  Everything is evaluated as esterr.c writes it (wrapping int32_t, the strand bit of the anchor itself in
 * get_for_qpos, qlen - r->qs in the second flank test, int-against-float compares in float); l_ref = (int32_t)d_ref_len[rid], n_ref entries (mi->seq[].len).
 * Preconditions: mini_pos of a read increases strictly in (int32_t)mini_pos[j] (mm_sketch emits at most one minimizer per position; the kernels rely on it
 * to test every anchor on its own), and the regions of a read do not overlap in a[] (the mapq plan guarantees it).  A read's regions are ranked by counting,
 * n^2 loads of one wave for n regions: meant for the few regions mm_select_sub leaves, not for thousands of unfiltered ones per read.
 * A read (1) whose u_off / b_off / mini_off / n_in leave the capacities or each other, (2) whose mini_pos does not increase strictly, or (3) with a region
 * whose [as, as + cnt) leaves the read's anchors or whose rid is outside [0, n_ref) touches nothing and is counted; mm2c_errplan_check then answers MM2C_E_ARG,
 * and the reads beside it are exact.  Regions 8-byte, anchors 16-byte aligned.  Asynchronous on `stream`; may follow mm2c_mapqplan_run_device on the same
 * stream, the host never having seen u_off or n_out.  A host then downloads 8 bytes per final region and 4 per read. */
typedef struct { int32_t n_match, n_tot; } mm2c_err_t;
typedef struct mm2c_errplan mm2c_errplan_t;
mm2c_errplan_t *mm2c_errplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_b_cap, int64_t n_mini_cap);
void mm2c_errplan_destroy(mm2c_errplan_t *plan);
int mm2c_errplan_run_device(mm2c_errplan_t *plan, const int64_t *d_u_off, const mm2c_reg_t *d_regs, const int32_t *d_n_in, const int64_t *d_b_off, const void *d_b,
                            const int64_t *d_mini_off, const uint64_t *d_mini_pos, const int32_t *d_qlen, int32_t n_ref, const uint32_t *d_ref_len,
                            mm2c_err_t *d_err, float *d_avg_k, void *stream);
/* waits for the last run.  MM2C_E_ARG if a read was refused; *n_refused (may be NULL): how many */
int mm2c_errplan_check(mm2c_errplan_t *plan, int64_t *n_refused);
/* milliseconds of the last run between HIP events on its stream; _kernel_ms: the same for err_reads, err_walk and err_finish */
int mm2c_errplan_last_ms(mm2c_errplan_t *plan, float *ms);
int mm2c_errplan_last_kernel_ms(mm2c_errplan_t *plan, float *reads_ms, float *walk_ms, float *finish_ms);
/* esterr.c:62 with the host's own pow; needs no device.  n_match <= 0 gives -1.0f, n_match >= n_tot gives 0.0f */
float mm2c_est_err_div(int32_t n_match, int32_t n_tot, float avg_k);
/* writes div into the host's regions: regs[u_off[r] + i].div for i < n_in[r] from err[u_off[r] + i] and avg_k[r]; a region with n_match == -1 is left alone.
 * Host only. */
int mm2c_est_err_apply_host(int64_t n_reads, const int64_t *u_off, const int32_t *n_in, const mm2c_err_t *err, const float *avg_k, mm2c_reg_t *regs);
/* host arrays in, div written in place: the regions of read r are regs[u_off[r] .. u_off[r] + n_in[r]), its anchors b[b_off[r] .. b_off[r+1]), its minimizers
 * mini_pos[mini_off[r] .. mini_off[r+1]).  Checks the offsets and n_in first (MM2C_E_ARG, before any device work), then uploads, runs, downloads, waits and
 * applies; behind it div is byte for byte the reference's.  err / avg_k: NULL, or room for u_off[n_reads] - u_off[0] counts (read r from u_off[r] - u_off[0]
 * on) and n_reads floats.  When a read is refused on the device the answer is MM2C_E_ARG and no region is written. */
int mm2c_est_err_batch_host(int64_t n_reads, const int64_t *u_off, mm2c_reg_t *regs, const int32_t *n_in, const int64_t *b_off, const mm2c_anchor_t *b,
                            const int64_t *mini_off, const uint64_t *mini_pos, const int32_t *qlen, int32_t n_ref, const uint32_t *ref_len, mm2c_err_t *err,
                            float *avg_k);

/* ---- the hits of a fragment -> regions per segment on the GPU (mm_seg_gen map.c:365, hit.c:373-427: fragments of several segments mapped without CIGAR) ----
 * Behind mm_select_sub_multi the reference splits every hit of a fragment by the segment of its anchors (bits 48-55 of y): segment s gets the chains u (the hit's
 * score << 32 | its anchors in s, hits without one squeezed out, hit order kept) and the anchors a (in (hit, j) order, y turned into the segment's own coordinates
 * by the 64-bit subtraction of hit.c:414 with the anchor's own strand bit), and mm_gen_regs(hash, qlens[s], ...) makes regs[s] of them, seg_split set and
 * seg_id = s.  The plan does the same for a batch.  Input per fragment f: its hits d_regs[u_off[f] .. u_off[f] + d_n_in[f]) as mm2c_hitplan_run_device_multi
 * wrote them (its d_regs_out / d_n_out), its chain anchors d_b[b_off[f] .. b_off[f+1]) as the region plan got them (`as` counts from b_off[f]), d_seg_len
 * (n_frags * n_segs qlens, fragment-major), d_hash and optionally d_rep_len per fragment.  Output per "segment read" f * n_segs + s, in the CSR shape every plan
 * above consumes, so that they run behind it unchanged with n_reads = n_frags * n_segs: d_su_off / d_su (seg[s].u), d_sb_off / d_sb (seg[s].a), d_seg_regs
 * (indexed like d_su: byte for byte regs[s] of hit.c:419-424, klib's order among equal sort keys included), d_seg_hash and, with d_rep_len, d_seg_rep_len (the
 * fragment's values once per segment; d_seg_len itself is the qlen of the segment reads).  Then: the hit plan with pri_ratio <= 0 is map.c:368, the mapq plan
 * with do_join = 0 is map.c:370.
 * Room: d_su_off / d_sb_off n_frags * n_segs + 1 entries, d_seg_hash / d_seg_rep_len n_frags * n_segs, d_sb n_b_cap anchors, d_su and d_seg_regs
 * mm2c_segplan_seg_chain_cap() = min(n_segs * n_u_cap, n_b_cap) entries (a segment chain holds at least one anchor).  Regions and chains 8-byte, anchors
 * 16-byte aligned; d_sb must not alias d_b.  Asynchronous on `stream`; may follow mm2c_hitplan_run_device_multi on the same stream, the host never having seen
 * u_off or n_out.  A fragment (1) whose u_off / b_off / n_in leave the capacities or each other, (2) with a hit whose [as, as + cnt) leaves the fragment's
 * anchors, or whose hits count more anchors than the fragment has, or (3) with an anchor whose segment is >= n_segs (the reference would write out of bounds)
 * touches nothing and is counted: its segment reads are empty, so the CSR stays sound, mm2c_segplan_check answers MM2C_E_ARG and the fragments beside it are
 * exact.  A fragment without hits, and a segment without anchors, give empty segment reads. */
#define MM2C_REG_SEG_SPLIT_BIT 15
#define MM2C_REG_SEG_ID_SHIFT 16
typedef struct mm2c_segplan mm2c_segplan_t;
mm2c_segplan_t *mm2c_segplan_create(int64_t n_frags, int32_t n_segs, int64_t n_u_cap, int64_t n_b_cap);
void mm2c_segplan_destroy(mm2c_segplan_t *plan);
int64_t mm2c_segplan_seg_chain_cap(const mm2c_segplan_t *plan);
int mm2c_segplan_run_device(mm2c_segplan_t *plan, const int64_t *d_u_off, const mm2c_reg_t *d_regs, const int32_t *d_n_in, const int64_t *d_b_off, const void *d_b,
                            const int32_t *d_seg_len, const uint32_t *d_hash, const int32_t *d_rep_len, int64_t *d_su_off, uint64_t *d_su, int64_t *d_sb_off,
                            void *d_sb, mm2c_reg_t *d_seg_regs, uint32_t *d_seg_hash, int32_t *d_seg_rep_len, void *stream);
/* waits for the last run.  MM2C_E_ARG if a fragment was refused; *n_refused: how many; *n_seg_chains / *n_seg_anchors: su_off / sb_off of the last segment
 * read's end (all three filled in either way; any may be NULL) */
int mm2c_segplan_check(mm2c_segplan_t *plan, int64_t *n_refused, int64_t *n_seg_chains, int64_t *n_seg_anchors);
/* milliseconds of the last run between HIP events on its stream; _kernel_ms: the same for seg_count, the two scans, seg_scatter, the region kernels and seg_mark */
int mm2c_segplan_last_ms(mm2c_segplan_t *plan, float *ms);
int mm2c_segplan_last_kernel_ms(mm2c_segplan_t *plan, float *count_ms, float *offsets_ms, float *scatter_ms, float *regs_ms, float *mark_ms);
/* host arrays in and out, room as above with the capacities u_off[n_frags] - u_off[0] and b_off[n_frags] - b_off[0].  Checks the offsets, n_in, every hit's
 * anchors and their segments first (MM2C_E_ARG, before any device work), then uploads, runs, downloads and waits. */
int mm2c_seg_gen_batch_host(int64_t n_frags, int32_t n_segs, const int64_t *u_off, const mm2c_reg_t *regs, const int32_t *n_in, const int64_t *b_off,
                            const mm2c_anchor_t *b, const int32_t *seg_len, const uint32_t *hash, const int32_t *rep_len, int64_t *su_off, uint64_t *su,
                            int64_t *sb_off, mm2c_anchor_t *sb, mm2c_reg_t *seg_regs, uint32_t *seg_hash, int32_t *seg_rep_len);

/* ---- base alignment on the GPU: ksw_extd2_sse (ksw2_extd2_sse.c), the dual-affine banded DP mm_align_pair calls when q != q2 || e != e2 (align.c:313-339) ----
 * A stand-alone plan: a batch of independent tasks in, ksw_extz_t and CIGAR out, byte for byte what the reference's SSE4.1 build gives (DESIGN.md 3.17 says what
 * that takes).  Wired into nothing; max_sw_mat (align.c:323) and everything of mm_align1 around the call stay with the caller.
 * One score set per call (m = 5: mat as ksw_gen_simple_mat makes it, align.c:9-22).  Sequences are codes 0..4 in one byte pool of seq_cap bytes; task i reads
 * seq[q_off .. q_off + qlen) and seq[t_off .. t_off + tlen).  PRECONDITION: no code above 4 (nothing indexes with a code, so the device does not look; the host
 * entry does).  flag: the KSW_EZ_* bits of MM2C_KSW_FLAGS -- everything align.c:697,733,737,771,828 passes.  Task i's CIGAR goes to
 * cigar[cig_off[i] .. cig_off[i + 1]) (BAM words, forward, or reversed with REV_CIGAR, as the reference leaves them).
 * status of a task: 0; MM2C_KSW_REFUSED -- a flag bit outside MM2C_KSW_FLAGS, a length above MM2C_KSW_MAX_LEN, offsets or lengths that leave seq_cap, or a
 * CIGAR slot that is negative or leaves cigar_cap: counted, nothing but the status word is written, mm2c_kswplan_check answers MM2C_E_ARG;
 * MM2C_KSW_TOO_BIG -- the task's p matrix (and, beyond MM2C_KSW_LDS_LEN bases, its array image) does not fit a task slot of the scratch
 * (mm2c_kswplan_slot_bytes; mm2c_ksw_task_scratch says what a task takes): not run, nothing but the status word is written, MM2C_E_TOOBIG;
 * MM2C_KSW_CIGAR_CUT -- the CIGAR is longer than its slot: the first words that fit are written, every scalar (n_cigar too) is exact, MM2C_E_TOOBIG.
 * The tasks beside any of these are exact.  qlen <= 0 || tlen <= 0 leaves the reset ez of ksw_reset_extz and status 0.
 * Scratch: the plan owns n_slots equal slots of slot_bytes; one wave per slot works the tasks slot, slot + n_slots, ... in turn, so the scratch bounds how many tasks
 * are resident, not how many a call may hold.  A task runs only in a slot of at least mm2c_ksw_task_scratch(qlen, tlen, w, flag) bytes: about
 * (qlen + tlen) * (min(qlen, tlen, w + 1) + 32) bytes for its p matrix (nothing with SCORE_ONLY), e.g. 2.2 MB for 2 000 x 2 100 at w = 500, 8.1 MiB for 2 000 x 2 000
 * at w = 2 000.  That is the only ceiling on a task's size below MM2C_KSW_MAX_LEN.  mm2c_kswplan_create_slots takes the cut from the caller (1 <= n_slots <=
 * MM2C_KSW_MAX_SLOTS, any slot_bytes the device can hold n_slots times; rounded up to 256); mm2c_kswplan_create(scratch_bytes) is the default cut for tasks of up
 * to MM2C_KSW_SLOT_BYTES = 4 MiB: n_slots = clamp(scratch_bytes / 4 MiB, 1, MM2C_KSW_MAX_SLOTS) slots of scratch_bytes / n_slots.  A host with larger tasks (-x ava-*:
 * bw = 2 000) sizes the slots itself. */
#define MM2C_KSW_FLAGS 0xdb            /* KSW_EZ_SCORE_ONLY 0x01, RIGHT 0x02, APPROX_MAX 0x08, APPROX_DROP 0x10, EXTZ_ONLY 0x40, REV_CIGAR 0x80 */
#define MM2C_KSW_MAX_LEN (1 << 20)
#define MM2C_KSW_LDS_LEN 2304          /* tasks up to this target (padded to 16) and query length keep their arrays on chip */
#define MM2C_KSW_SLOT_BYTES (4ll << 20)
#define MM2C_KSW_MAX_SLOTS 2048
#define MM2C_KSW_REFUSED 1
#define MM2C_KSW_TOO_BIG 2
#define MM2C_KSW_CIGAR_CUT 3
typedef struct { int8_t mat[25]; int8_t q, e, q2, e2; } mm2c_ksw_score_t;            /* m = 5 */
typedef struct { int64_t q_off, t_off; int32_t qlen, tlen, w, zdrop, end_bonus, flag; } mm2c_ksw_task_t;
typedef struct { uint32_t max; int32_t zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end, status; } mm2c_ksw_res_t;
typedef struct mm2c_kswplan mm2c_kswplan_t;
mm2c_kswplan_t *mm2c_kswplan_create(int64_t n_tasks_cap, int64_t seq_cap, int64_t cigar_cap, int64_t scratch_bytes);
mm2c_kswplan_t *mm2c_kswplan_create_slots(int64_t n_tasks_cap, int64_t seq_cap, int64_t cigar_cap, int64_t n_slots, int64_t slot_bytes);
void mm2c_kswplan_destroy(mm2c_kswplan_t *plan);
int64_t mm2c_kswplan_slot_bytes(const mm2c_kswplan_t *plan);
int64_t mm2c_kswplan_n_slots(const mm2c_kswplan_t *plan);
int64_t mm2c_ksw_task_scratch(int32_t qlen, int32_t tlen, int32_t w, int32_t flag);   /* bytes of a slot the task takes */
/* All pointers are device memory (d_tasks, d_cig_off 8-byte aligned, d_res, d_cigar 4-byte); asynchronous on `stream` (NULL / MM2C_STREAM_LIBRARY as everywhere). */
int mm2c_kswplan_run_device(mm2c_kswplan_t *plan, const mm2c_ksw_score_t *sc, int64_t n_tasks, const mm2c_ksw_task_t *d_tasks, const uint8_t *d_seq,
                            const int64_t *d_cig_off, mm2c_ksw_res_t *d_res, uint32_t *d_cigar, void *stream);
/* waits for the last run.  MM2C_E_ARG if a task was refused, else MM2C_E_TOOBIG if one did not fit a slot or a CIGAR was cut.  *n_too_big counts both kinds. */
int mm2c_kswplan_check(mm2c_kswplan_t *plan, int64_t *n_refused, int64_t *n_too_big);
/* milliseconds of the last run between HIP events on its stream; _kernel_ms: the same for ksw_rows (rows and backtrack are one kernel) */
int mm2c_kswplan_last_ms(mm2c_kswplan_t *plan, float *ms);
int mm2c_kswplan_last_kernel_ms(mm2c_kswplan_t *plan, float *rows_ms);
/* host arrays in and out: res has n_tasks entries, cigar cig_off[n_tasks] words.  Checks the score set, every task's flag, lengths, offsets and slot, and every
 * base it reads (a code above 4) first (MM2C_E_ARG, before any device work), then uploads, runs, downloads and waits.  Its slots have the size of the call's
 * largest task, so no task of the call is too big for them: with scratch_bytes <= 0 as many slots as there are tasks, up to 1 280 slots and 4 GiB (one slot if the
 * largest task alone is beyond that); with scratch_bytes > 0 as many as scratch_bytes holds, and if it does not hold one, a single slot of scratch_bytes: the tasks
 * beyond it come back MM2C_KSW_TOO_BIG.  With MM2C_E_TOOBIG the outputs are complete all the same. */
int mm2c_ksw_extd2_batch_host(const mm2c_ksw_score_t *sc, int64_t n_tasks, const mm2c_ksw_task_t *tasks, int64_t seq_len, const uint8_t *seq,
                              const int64_t *cig_off, mm2c_ksw_res_t *res, uint32_t *cigar, int64_t scratch_bytes);

/* ---- an aligned region finished on the GPU: mm_update_extra (align.c:240-286, with mm_fix_cigar :91-167 and mm_update_cigar_eqx :169-238) and mm_test_zdrop
 * (align.c:47-89) ----
 * A stand-alone plan with two entries, byte for byte what the reference's functions give.  One score set per call: mat, q and e of a
 * mm2c_ksw_score_t are read (q2, e2 are not).  Behind a gap word the reference clamps the running score but does not update the maximum (:268-269); the plan does the
 * same.  q < 0 or e < 0 is refused at the entry all the same (MM2C_E_ARG): there `s -= q + e * len` is evaluated in unsigned arithmetic and wraps, which no preset
 * asks for and the plan does not follow; with 0 <= q, e <= 127 and lengths up to MM2C_KSW_MAX_LEN nothing wraps.  Sequences are codes 0..4 in one pool of seq_cap bytes.
 *
 * mm2c_extraplan_run_device: mm_update_extra for n_regs regions.  Region i: qlen = r->qe - r->qs and tlen = r->re - r->rs at entry, the sequences of :787-788 at
 * q_off / t_off, its CIGAR in cig_in[in_off[i] .. in_off[i] + n_cigar), its output slot cig_out[out_off[i] .. out_off[i + 1]).  The two CIGAR buffers may not
 * overlap (MM2C_E_ARG).  rev is carried for the caller; the results do not depend on it.  Result: the final n_cigar and CIGAR words, blen, mlen, n_ambi (what the
 * call adds to p->n_ambi), dp_max, and the leading I / D the function stripped (:157-166): the caller does rs += tshift, and qe -= qshift if rev, else qs += qshift.
 * Without is_eqx the result never has more words than the input; with is_eqx it may: a result longer than its slot is cut to the words that fit, every scalar
 * (n_cigar too) is exact, nothing is written behind the slot, status MM2C_EXTRA_CIGAR_CUT, MM2C_E_TOOBIG from mm2c_extraplan_check.
 * MM2C_EXTRA_REFUSED (counted, MM2C_E_ARG, nothing but the status word written): inputs the reference is not defined on -- an op code above 3, a zero-length word
 * with op 3, two or more words whose lengths are all zero, op lengths that do not add up to qlen and tlen -- and offsets or lengths that leave a pool or run
 * backwards, or a length above MM2C_KSW_MAX_LEN.  Base codes above 4 are not looked for on the device (the host entries refuse them).
 * A CIGAR of up to MM2C_EXTRA_LDS_WORDS words is worked on in LDS; a longer one in one of the plan's n_slots scratch slots of slot_words words (16 bytes a word):
 * beyond both, MM2C_EXTRA_TOO_BIG (counted, not run, MM2C_E_TOOBIG).  n_slots is also the number of waves resident (<= 0: 2 048; at most MM2C_EXTRA_MAX_SLOTS).
 * The sequences stay in global memory.  The items beside a refused, too big or cut one are exact.
 *
 * mm2c_extraplan_zdrop_run_device: mm_test_zdrop on the arrays of a ksw plan, unchanged and without a download in between (cig_in_cap of the plan is the ksw plan's
 * cigar_cap).  zdrop_opt.no_inv stands for opt->flag & (MM_F_SPLICE | MM_F_SR | MM_F_FOR_ONLY | MM_F_REV_ONLY) of :72.  Per task: max_zdrop; t0, t1, q0, q1 =
 * pos[0][0], pos[0][1], pos[1][0], pos[1][1] (-1 when nothing dropped); code = max_zdrop > zdrop (:88); inv_cand = 1 exactly when the condition of :72 holds.  The
 * ksw_ll_i16 call behind it stays with the host: for a task with inv_cand, run ksw_ll_i16 on the reverse complement of query [q0, q1) against target [t0, t1) as
 * :76-82 do; the function's return is 2 if that score passes :85, else code.  A task whose ksw status is not 0 gets MM2C_EXTRA_REFUSED and nothing else (counted);
 * so does one whose CIGAR leaves its slot or its sequences.  n_cigar == 0 gives max_zdrop 0 and positions -1. */
#define MM2C_EXTRA_LDS_WORDS 2048
#define MM2C_EXTRA_RUN_LANE 16         /* an indel's match run is walked by one lane up to this many bases, by the whole wave beyond */
#define MM2C_EXTRA_MAX_SLOTS 4096
#define MM2C_EXTRA_REFUSED 1
#define MM2C_EXTRA_TOO_BIG 2
#define MM2C_EXTRA_CIGAR_CUT 3
typedef struct { int64_t q_off, t_off; int32_t qlen, tlen; int32_t n_cigar; int32_t rev; } mm2c_extra_task_t;
typedef struct { int32_t n_cigar, qshift, tshift, blen, mlen, n_ambi, dp_max, status; } mm2c_extra_res_t;
typedef struct { int32_t zdrop, zdrop_inv, max_gap, no_inv; } mm2c_zdrop_opt_t;
typedef struct { int32_t max_zdrop, t0, t1, q0, q1, code, inv_cand, status; } mm2c_zdrop_res_t;
typedef struct mm2c_extraplan mm2c_extraplan_t;
mm2c_extraplan_t *mm2c_extraplan_create(int64_t n_cap, int64_t seq_cap, int64_t cig_in_cap, int64_t cig_out_cap, int64_t n_slots, int64_t slot_words);
void mm2c_extraplan_destroy(mm2c_extraplan_t *plan);
/* asynchronous on `stream`; all pointers are device memory except sc and opt */
int mm2c_extraplan_run_device(mm2c_extraplan_t *plan, const mm2c_ksw_score_t *sc, int is_eqx, int64_t n_regs, const mm2c_extra_task_t *d_tasks, const uint8_t *d_seq,
                              const int64_t *d_in_off, const uint32_t *d_cig_in, const int64_t *d_out_off, mm2c_extra_res_t *d_res, uint32_t *d_cig_out, void *stream);
int mm2c_extraplan_zdrop_run_device(mm2c_extraplan_t *plan, const mm2c_ksw_score_t *sc, const mm2c_zdrop_opt_t *opt, int64_t n_tasks, const mm2c_ksw_task_t *d_tasks,
                                    const uint8_t *d_seq, const int64_t *d_cig_off, const mm2c_ksw_res_t *d_res, const uint32_t *d_cigar, mm2c_zdrop_res_t *d_zres, void *stream);
/* waits for the plan's last run (of either entry); n_too_big: CIGARs beyond LDS and slot plus output CIGARs cut */
int mm2c_extraplan_check(mm2c_extraplan_t *plan, int64_t *n_refused, int64_t *n_too_big);
/* milliseconds of the last run between HIP events on its stream; _kernel_ms: of the last extra_update and the last extra_zdrop run (0 for one that has not run) */
int mm2c_extraplan_last_ms(mm2c_extraplan_t *plan, float *ms);
int mm2c_extraplan_last_kernel_ms(mm2c_extraplan_t *plan, float *update_ms, float *zdrop_ms);
/* host arrays in and out: check the score set, the offsets and every base code first (MM2C_E_ARG before any device work), then upload, run, download and wait.
 * Scratch slots take the call's longest CIGAR, so nothing is too big.  With MM2C_E_TOOBIG (a CIGAR cut) the outputs are complete all the same. */
int mm2c_update_extra_batch_host(const mm2c_ksw_score_t *sc, int is_eqx, int64_t n_regs, const mm2c_extra_task_t *tasks, int64_t seq_len, const uint8_t *seq,
                                 const int64_t *in_off, int64_t n_cig_in, const uint32_t *cig_in, const int64_t *out_off, mm2c_extra_res_t *res, uint32_t *cig_out);
int mm2c_test_zdrop_batch_host(const mm2c_ksw_score_t *sc, const mm2c_zdrop_opt_t *opt, int64_t n_tasks, const mm2c_ksw_task_t *tasks, int64_t seq_len, const uint8_t *seq,
                               const int64_t *cig_off, const mm2c_ksw_res_t *res, const uint32_t *cigar, mm2c_zdrop_res_t *zres);

/* ---- final regions -> ksw tasks and their sequence pool on the GPU (mm_align1, align.c:565-733, 767-771, up to each mm_align_pair call) ----
 * mm2c_refseq_t: the packed reference mi->S as the host has it (mm_seq4_set, 8 bases a word) with offset and len of every mi->seq[], resident on the device.
 *
 * mm2c_alnplan_t, a stand-alone plan wired into nothing.  Under MM2C_ALN_F_SR it runs mm_max_stretch, the sr form of rs0 .. qe0 (:613-620) and emits
 * one ungapped item between the extensions instead of what follows.  Otherwise per region it runs mm_fix_bad_ends (unless MM2C_ALN_F_NO_END_FLT), mm_filter_bad_seeds and
 * mm_filter_bad_seeds_alt with the arguments of :595-596 -- MM_SEED_IGNORE / MM_SEED_LONG_JOIN are written into the caller's anchors, and a LONG_JOIN that is set
 * already is honoured --, mm_adjust_minier (both forms: k >> 1, and the homopolymer walks under MM2C_ALN_I_HPC), rs0 .. qe0 (:621-684) and then emits the list of calls mm_align1 issues WHEN NO TASK DROPS, in call
 * order: left extension, gap fills, right extension.  A consumer cuts the list behind the first task the z-drop entry reports as dropped (an item over
 * max_sw_mat counts as dropped, :323-325).  Outputs: one mm2c_aln_reg_t per region; the items; mm2c_ksw_task_t[] with cig_off[] as mm2c_kswplan_run_device takes
 * them (a task's CIGAR slot: min(qlen + tlen, ((qlen + tlen) >> cig_shift) + 16) words); and ONE sequence pool that is directly the d_seq of the ksw plan and of
 * the extra plan.  Per region the pool holds, each from a multiple of 16 on and padded with code 4: the query span [qs0, qe0) on the region's strand at q_off, the
 * target span [rs0, re0) at t_off, and -- if there is a left extension -- the reversed query [qs0, qs) at left_off and the reversed target [rs0, rs) at left_off +
 * round16(qs - qs0).  Gap and right-extension tasks point into the spans; [qs1, qe1) x [rs1, re1) of mm_update_extra is q_off + (qs1 - qs0), t_off + (rs1 - rs0).
 * status: MM2C_ALN_REFUSED (counted, MM2C_E_ARG from _check; only the status is written, the anchors are untouched): MM2C_ALN_F_SPLICE, MM2C_ALN_F_SR
 * together with MM2C_ALN_I_HPC (:575), an sr stretch whose two lengths differ (:725), as / cnt leaving the read's anchors, anchors not on one x >> 32, rid >= n_seq, an anchor beyond its contig or read or running
 * backwards, an input on which an assert of :600, 626, 686, 707 would fire or a length would be negative, offsets leaving a capacity.  MM2C_ALN_TOO_BIG: more
 * long gaps (:367) than MM2C_ALN_LDS_GAPS and than slot_words (counted, not run, MM2C_E_TOOBIG).  MM2C_ALN_OVER_CAP: the region's items, tasks or pool bytes leave
 * a capacity: counted, MM2C_E_TOOBIG, no item, task or pool byte of it is written and nothing behind a capacity; totals[] of _check still say what the batch needs.  Its
 * anchors DO carry the flags of its filters already (they are written before the offsets are known); running it again with more room gives the same as1 / cnt1 and
 * flags, since the filters only add bits and mm_fix_bad_ends sees a LONG_JOIN only behind the ends it has chosen.  With n_regs == 0 only cig_off[0] = 0 is written. */
#define MM2C_ALN_LDS_GAPS 2048
#define MM2C_ALN_MAX_SLOTS 4096
#define MM2C_ALN_REFUSED 1
#define MM2C_ALN_TOO_BIG 2
#define MM2C_ALN_OVER_CAP 3
#define MM2C_ALN_F_SR 1
#define MM2C_ALN_F_NO_END_FLT 2
#define MM2C_ALN_F_SPLICE 4
#define MM2C_ALN_I_HPC 1
#define MM2C_ALN_LEFT 0
#define MM2C_ALN_GAP 1
#define MM2C_ALN_RIGHT 2
#define MM2C_ALN_UNGAPPED 3            /* the sr gap fill (:724-731): no ksw task, `score` is its ungapped score, qe - qs its one CIGAR word */
#define MM2C_ALN_OVER 16               /* or-ed into kind: beyond max_sw_mat, no ksw task (task == -1) */
typedef struct {
	int32_t a, b, q, e, e2, bw, bw_ext;            /* bw_ext = (int)(opt->bw * 1.5 + 1.), computed by the host (:580) */
	int32_t min_chain_score, max_gap, min_cnt, min_ksw_len, end_bonus, zdrop, zdrop_inv;
	int64_t max_sw_mat;
	int32_t flag, idx_flag, k, reserved;           /* MM2C_ALN_F_*, MM2C_ALN_I_*, mi->k */
} mm2c_aln_opt_t;
typedef struct {
	int32_t as1, cnt1, rs, qs, re, qe, rs0, qs0, re0, qe0, n_items, n_tasks, status, rev;
	int64_t item0, task0, cig0, q_off, t_off, left_off;
} mm2c_aln_reg_t;
typedef struct { int32_t reg, kind, anchor, rs, re, qs, qe, task, score, reserved; } mm2c_aln_item_t;   /* anchor: index into the read's anchors; task: index into the task list */
typedef struct mm2c_refseq mm2c_refseq_t;
typedef struct mm2c_alnplan mm2c_alnplan_t;
/* host arrays; NULL on failure: a contig whose [offset, offset + len) leaves the n_words words, a len of 2^31 or more (MM2C_E_ARG) */
mm2c_refseq_t *mm2c_refseq_create(int64_t n_seq, const uint64_t *offset, const uint32_t *len, const uint32_t *S, int64_t n_words);
void mm2c_refseq_destroy(mm2c_refseq_t *ref);
/* capacities: regions, items, tasks, pool bytes, anchors and read bases of a batch.  n_slots (<= 0: 2 048) waves are resident, each with a slot of slot_words words */
mm2c_alnplan_t *mm2c_alnplan_create(int64_t n_regs_cap, int64_t n_items_cap, int64_t n_tasks_cap, int64_t pool_cap, int64_t n_b_cap, int64_t reads_cap, int32_t cig_shift,
                                    int64_t n_slots, int64_t slot_words);
void mm2c_alnplan_destroy(mm2c_alnplan_t *plan);
/* asynchronous on `stream`; all pointers are device memory except opt.  d_u_off, d_b_off, d_read_off: n_reads + 1 entries; d_n_b (may be NULL): anchors per read,
 * as the mapq plan's d_n_b_out.  d_b is in/out.  d_cig_off: n_tasks_cap + 1 entries; d_pool: pool_cap bytes, 16-byte aligned.  Regions 8-byte, anchors 16-byte aligned. */
int mm2c_alnplan_run_device(mm2c_alnplan_t *plan, const mm2c_aln_opt_t *opt, const mm2c_refseq_t *ref, int64_t n_reads, int64_t n_regs, const int64_t *d_u_off,
                            const mm2c_reg_t *d_regs, const int64_t *d_b_off, const int64_t *d_n_b, void *d_b, const int64_t *d_read_off, const uint8_t *d_reads,
                            mm2c_aln_reg_t *d_aln_regs, mm2c_aln_item_t *d_items, mm2c_ksw_task_t *d_tasks, int64_t *d_cig_off, uint8_t *d_pool, void *stream);
/* waits for the last run; totals (may be NULL): items, tasks, CIGAR words and pool bytes the batch takes; n_too_big counts MM2C_ALN_TOO_BIG and MM2C_ALN_OVER_CAP */
int mm2c_alnplan_check(mm2c_alnplan_t *plan, int64_t *n_refused, int64_t *n_too_big, int64_t totals[4]);
/* milliseconds between HIP events of the last run: aln_plan with aln_scan, aln_emit, aln_gather */
int mm2c_alnplan_last_kernel_ms(mm2c_alnplan_t *plan, float ms[3]);
/* host arrays in and out.  Checks the offsets and every base code (reads: 0..4; S: nibbles 0..4 inside the contigs) first (MM2C_E_ARG before any device work), then
 * uploads, runs, downloads and waits.  b comes back with its flags; the capacities are those of the arrays given; totals as _check. */
int mm2c_align_tasks_batch_host(const mm2c_aln_opt_t *opt, int64_t n_seq, const uint64_t *offset, const uint32_t *len, const uint32_t *S, int64_t n_words,
                                int64_t n_reads, const int64_t *u_off, const mm2c_reg_t *regs, const int64_t *b_off, mm2c_anchor_t *b, const int64_t *read_off,
                                const uint8_t *reads, int32_t cig_shift, mm2c_aln_reg_t *aln_regs, int64_t n_items_cap, mm2c_aln_item_t *items, int64_t n_tasks_cap,
                                mm2c_ksw_task_t *tasks, int64_t *cig_off, int64_t pool_cap, uint8_t *pool, int64_t totals[4]);

/* ---- ksw results -> aligned regions on the GPU: the rest of mm_align1 (align.c:698-705, 736-764, 772-783) ----
 * mm2c_cigplan_t, a stand-alone plan wired into nothing, with two entries.  Both read the arrays of the alignment-task plan (d_aln_regs, d_items, d_tasks, d_cig_off,
 * the pool), of the ksw plan (d_res, d_cigar) and of the z-drop entry (d_zres: only status and code are read) where those plans left them.  code is 0, 1 or 2: a host
 * that has run ksw_ll_i16 on an inv_cand task writes 2 there before the call.
 *
 * mm2c_cigplan_second_run_device: the list of second passes (:736-737).  Every MM2C_ALN_GAP item with a ksw task, a z-drop status of 0 and code 1 or 2 gets a copy of
 * its first-pass task with KSW_EZ_APPROX_MAX cleared and zdrop = (code == 2 ? zdrop_inv : zdrop), in item order, in d_tasks2 with d_cig_off2 (the slot rule of the
 * first list, with opt->cig_shift); d_second_of[item] is its index there, -1 for an item without one, MM2C_CIG_NO_ROOM for one whose region's tasks or slots leave
 * n_tasks2_cap or cigar2_cap (counted, MM2C_E_TOOBIG; nothing of that region is written).  The entries of a region the
 * entry does not walk -- status not 0, item offsets leaving a capacity -- stay untouched; the join refuses such a region on its own.  The ksw plan runs the list unchanged on the same pool.  The list holds a
 * second pass for EVERY such item, not only for those in front of its region's first drop: the reference issues a subset of them, and the join entry ignores the rest.
 * Under MM2C_ALN_F_SR the MM2C_ALN_UNGAPPED item has no first-pass task, so its mm_test_zdrop (one M word of qe - qs bases over mat; :72 is off, the code is 0 or 1)
 * is made here; with 1 it gets the task {reg.q_off + (qs - qs0), reg.t_off + (rs - rs0), qe - qs, re - rs, bw_ext, opt->zdrop, -1, 0}.  An ungapped item whose
 * bases leave the pool is counted as refused, gets no task and MM2C_CIG_LOST in d_second_of, on which the join refuses its region.
 *
 * mm2c_cigplan_run_device: per region the cut behind the first dropped gap item, mm_append_cigar over the used items with its merge at every boundary (:303-306),
 * dp_score, rs1 / qs1 / re1 / qe1, r->qs / r->qe on the read's strand and the split decision.  An item's ez is the second list's where d_second_of names one, else
 * the first pass's; the reset ez with zdropped = 1 for an item over max_sw_mat; score and the word (qe - qs) << 4 for an sr ungapped item without a second pass.
 * Outputs: one mm2c_cig_reg_t per region (n_used: items consumed; drop_item: the dropped item's index in the region, -1; split_n: the argument of mm_split_reg,
 * 0 when the region is not split; has_p: r->p is set); the appended CIGARs in d_cig_out at cig0; and, dense and in region order for the regions that have words,
 * d_in_off[k], d_extra_tasks[k] and d_extra_reg[k] (the region of entry k), which mm2c_extraplan_run_device takes unchanged with d_cig_out as its cig_in;
 * d_in_off[n] is the number of words.  A region with cnt == 0 (:578) comes back with status 0, r_qs / r_qe / rs1 / re1 as the region has them and everything else 0.
 * mm_split_reg itself is the finish plan's (mm2c_finplan_apply_run_device, below); mm_align1_inv, ksw_ll_i16, ksw_extz2_sse and splice stay with the host.
 * status (only the status word of such a region is written; its neighbours are exact): MM2C_CIG_REFUSED (counted, MM2C_E_ARG) -- an mm2c_aln_reg_t whose status is
 * not 0; on a consumed item a code outside 0 .. 2, a z-drop record whose status is not 0, a second pass where the code is 0; item, task or CIGAR offsets leaving a
 * capacity; an appended CIGAR whose op lengths do not add up to qe1 - qs1 and re1 - rs1 (:284); qs1 < 0, rs1 < 0, qe1 > qlen or re1 - rs1 > re0 - rs0 (:707, 779, 785).
 * MM2C_CIG_INCOMPLETE (counted, MM2C_E_TOOBIG) -- a consumed task whose ksw status is not 0, an n_cigar beyond its slot, a code that is not 0 without a second pass.
 * A task behind the cut may have any status.  MM2C_CIG_OVER_CAP (counted, MM2C_E_TOOBIG): the region's words or extra task leave words_cap or n_extra_cap; its record
 * holds what the region came to (cig0 is 0), none of its words and no extra task is written, nothing is written behind a capacity and totals[] say what the batch takes.  With n_regs == 0 only in_off[0] = 0 is written. */
#define MM2C_CIG_REFUSED 1
#define MM2C_CIG_INCOMPLETE 2
#define MM2C_CIG_OVER_CAP 3
#define MM2C_CIG_PIECE 256             /* items and CIGAR words a workgroup of cig_gather takes at a time */
#define MM2C_CIG_NO_ROOM (-2)
#define MM2C_CIG_LOST (-3)
typedef struct { int32_t zdrop, zdrop_inv, bw_ext, min_cnt, flag, cig_shift; } mm2c_cig_opt_t;    /* flag: MM2C_ALN_F_*; cig_shift: that of the alignment-task plan */
typedef struct {
	int32_t status, n_used, dropped, drop_item, zdrop_code, split_n, split_inv, has_p, n_cigar, dp_score, rs1, re1, qs1, qe1, r_qs, r_qe;
	int64_t cig0;
} mm2c_cig_reg_t;
typedef struct mm2c_cigplan mm2c_cigplan_t;
/* capacities: regions, items, first-list tasks and CIGAR words (the ksw plan's cigar_cap), second-list tasks and CIGAR words, pool bytes, anchors, output words,
 * extra tasks */
mm2c_cigplan_t *mm2c_cigplan_create(int64_t n_regs_cap, int64_t n_items_cap, int64_t n_tasks_cap, int64_t cigar_cap, int64_t n_tasks2_cap, int64_t cigar2_cap, int64_t pool_cap,
                                    int64_t n_b_cap, int64_t words_cap, int64_t n_extra_cap);
void mm2c_cigplan_destroy(mm2c_cigplan_t *plan);
/* asynchronous on `stream`; all pointers are device memory except opt and sc (mat is read).  d_cig_off2: n_tasks2_cap + 1 entries; d_second_of: n_items_cap; d_seq is
 * read under MM2C_ALN_F_SR only */
int mm2c_cigplan_second_run_device(mm2c_cigplan_t *plan, const mm2c_cig_opt_t *opt, const mm2c_ksw_score_t *sc, int64_t n_regs, const mm2c_aln_reg_t *d_aln_regs,
                                   const mm2c_aln_item_t *d_items, const mm2c_ksw_task_t *d_tasks, const mm2c_zdrop_res_t *d_zres, const uint8_t *d_seq,
                                   mm2c_ksw_task_t *d_tasks2, int64_t *d_cig_off2, int32_t *d_second_of, void *stream);
/* waits for the last second-pass run; totals (may be NULL): tasks and CIGAR words of the second list */
int mm2c_cigplan_second_check(mm2c_cigplan_t *plan, int64_t *n_refused, int64_t *n_over_cap, int64_t totals[2]);
/* asynchronous on `stream`.  d_u_off, d_b_off, d_read_off: n_reads + 1 entries; d_n_b may be NULL; d_b is read only.  d_in_off: n_extra_cap + 1 entries.  d_cig_out may
 * overlap neither d_cigar nor d_cigar2 (MM2C_E_ARG) */
int mm2c_cigplan_run_device(mm2c_cigplan_t *plan, const mm2c_cig_opt_t *opt, int64_t n_reads, int64_t n_regs, const int64_t *d_u_off, const mm2c_reg_t *d_regs,
                            const int64_t *d_b_off, const int64_t *d_n_b, const void *d_b, const int64_t *d_read_off, const mm2c_aln_reg_t *d_aln_regs,
                            const mm2c_aln_item_t *d_items, const int64_t *d_cig_off, const mm2c_ksw_res_t *d_res, const uint32_t *d_cigar, const mm2c_zdrop_res_t *d_zres,
                            const int32_t *d_second_of, const int64_t *d_cig_off2, const mm2c_ksw_res_t *d_res2, const uint32_t *d_cigar2, mm2c_cig_reg_t *d_cig_regs,
                            uint32_t *d_cig_out, int64_t *d_in_off, mm2c_extra_task_t *d_extra_tasks, int32_t *d_extra_reg, void *stream);
/* waits for the last join run; totals (may be NULL): CIGAR words and extra tasks the batch takes */
int mm2c_cigplan_check(mm2c_cigplan_t *plan, int64_t *n_refused, int64_t *n_incomplete, int64_t *n_over_cap, int64_t totals[2]);
/* milliseconds between HIP events of the last runs: cig_second_count with its scan, cig_second_emit, cig_cut, cig_scan, cig_gather; 0 for an entry that has not run */
int mm2c_cigplan_last_kernel_ms(mm2c_cigplan_t *plan, float ms[5]);
/* host arrays in and out; argument checks (under MM2C_ALN_F_SR every base code of the pool too) come before any device work.  cig_off2: n_tasks2_cap + 1 entries */
int mm2c_second_pass_batch_host(const mm2c_cig_opt_t *opt, const mm2c_ksw_score_t *sc, int64_t n_regs, const mm2c_aln_reg_t *aln_regs, int64_t n_items,
                                const mm2c_aln_item_t *items, int64_t n_tasks, const mm2c_ksw_task_t *tasks, const mm2c_zdrop_res_t *zres, int64_t pool_len, const uint8_t *pool,
                                int64_t n_tasks2_cap, mm2c_ksw_task_t *tasks2, int64_t *cig_off2, int32_t *second_of, int64_t totals[2]);
int mm2c_assemble_regions_batch_host(const mm2c_cig_opt_t *opt, int64_t n_reads, const int64_t *u_off, const mm2c_reg_t *regs, const int64_t *b_off, const mm2c_anchor_t *b,
                                     const int64_t *read_off, const mm2c_aln_reg_t *aln_regs, int64_t n_items, const mm2c_aln_item_t *items, int64_t n_tasks, const int64_t *cig_off,
                                     const mm2c_ksw_res_t *res, const uint32_t *cigar, const mm2c_zdrop_res_t *zres, const int32_t *second_of, int64_t n_tasks2,
                                     const int64_t *cig_off2, const mm2c_ksw_res_t *res2, const uint32_t *cigar2, mm2c_cig_reg_t *cig_regs, int64_t words_cap, uint32_t *cig_out,
                                     int64_t n_extra_cap, int64_t *in_off, mm2c_extra_task_t *extra_tasks, int32_t *extra_reg, int64_t totals[2]);

/* ---- aligned regions -> final hits on the GPU: what mm_align1 leaves in r with mm_split_reg (align.c:757-760, 781-783; hit.c:108-123), then
 * mm_filter_regs and mm_hit_sort (align.c:917-918), mm_set_parent, mm_select_sub and mm_set_sam_pri (map.c:264-268) and mm_set_mapq (map.c:361) ----
 * A stand-alone plan with two entries, byte for byte the reference's.  It is the only plan whose regions carry r->p: mm2c_pext_t stands for mm_extra_t without its
 * CIGAR (ambi_strand: n_ambi:30 | trans_strand:2, as GCC lays out minimap.h:80; cig0: the first word of the region's final CIGAR in the extra plan's output), and in
 * the regions this plan writes and reads mm2c_reg_t.p is 0 for r->p == NULL, otherwise 1 + the index of the region's mm2c_pext_t in the batch.
 *
 * mm2c_finplan_apply_run_device (kernels fin_apply, fin_slots, fin_children).  In, exactly as the producing plans leave them: d_u_off / d_regs (the regions that went
 * into the alignment-task plan; d_u_off[0] == 0), d_b_off / d_b, d_read_off (for qlen), d_cig_regs of mm2c_cigplan_run_device, and n_extra, d_extra_reg, d_extra_res and
 * the output offsets d_out_off of mm2c_extraplan_run_device.  Out: d_regs_out[g], the region as mm_align1 returns it -- rs = rs1 + tshift, re = re1, qs / qe from
 * r_qs / r_qe with qshift on the side the extra plan names, blen, mlen from the extra result, p = g + 1; of a split region also cnt -= r2->cnt, score -= r2->score,
 * split |= 1 -- and d_pext[g] (dp_score, n_cigar, dp_max, n_ambi from the two records, dp_max2 = 0, trans_strand = 0, cig0 = d_out_off[k]); a region with has_p == 0
 * keeps p = 0 and gets the coordinates only (its d_pext[g] is zero).  The children r2 of mm_split_reg come dense and in region order: d_child[k], d_child_of[k] (the
 * region it was split from), *d_n_child of them.  r2 is *r as it stood in the middle of mm_align1 -- chain-level hash, div, subsc, the split bits before |= 1 -- with
 * id = -1, sam_pri = 0, p = 0, cnt = r->cnt - n, score = (int32_t)(r->score * ((float)r2->cnt / r->cnt) + .499) (a float quotient, a float product, a double add),
 * as += n, parent = MM_PARENT_TMP_PRI iff r->parent == r->id, mm_reg_set_coor over its own anchors (coordinates, rid, rev, mlen, blen), split |= 2 and
 * split_inv as the CIGAR-join plan decided it (zdrop_code == 2).  The order of the children across alignment rounds (mm_insert_reg: a child directly behind its
 * parent) is index arithmetic on d_child_of and stays with the caller.
 * d_status[g]: 0, or -- only the status word of such a region is written, its neighbours are exact -- MM2C_FIN_REFUSED (counted, MM2C_E_ARG from _apply_check): an
 * mm2c_cig_reg_t or extra result with status 1, has_p without an extra entry, a region outside d_u_off, read extents that leave n_b_cap, a child whose anchors leave
 * the read's; MM2C_FIN_INCOMPLETE (counted, MM2C_E_TOOBIG): any other status in front.  MM2C_FIN_OVER_CAP (counted, MM2C_E_TOOBIG): the region's child lies beyond
 * n_child_cap; the region itself is written, the child is not, nothing is written behind the capacity and *d_n_child says what the batch takes.
 *
 * mm2c_finplan_run_device (kernel fin_select, one wave per read).  The regions of read r are d_regs_in[f_off[r] .. f_off[r] + d_n_in[r]) in the order
 * mm_align_skeleton holds them behind its loop, every child directly behind its parent, in room for f_off[r+1] - f_off[r]; d_qlen and d_rep_len per read.  The first
 * d_n_out[r] entries of d_regs_out from f_off[r] on are, byte for byte, the reference's array behind map.c:361; dp_max2 of the surviving regions is updated in d_pext
 * in place and the p of every surviving region still names its record (a dropped region's record is simply no longer named).  With all_chains (MM_F_ALL_CHAINS) the
 * three calls of map.c:265-267 are skipped.  The logarithms: two tables the HOST fills at creation with its own logf, L[i] = logf((float)i) and
 * L2[i] = logf((float)i / match_sc), 0 <= i <= max_log_arg; a primary whose dp_max (with p), score (without) or n_sub + 1 lies beyond them gets mapq 0 and is
 * counted (MM2C_E_TOOBIG from _check); nothing else changes.  min_dp_max < 1 or match_sc < 1 is MM2C_E_ARG: every surviving dp_max is then >= 1 and logf never sees 0.
 * Refused and counted per read (MM2C_E_ARG from _check; nothing of that read is written, d_n_out[r] included, and its neighbours are exact): a region with inv or
 * is_alt set (mm_align1_inv, ALT contigs, mm_set_inv_mapq and mm_alt_score are not built: nothing the device can make today sets them, and alt_drop has no counterpart
 * in the options); offsets or d_n_in that leave the capacities or each other; a p that names no record; a read of more than one region that mixes kept regions with
 * and without p, or keeps none with cnt > 0 (the reference asserts there, hit.c:210).  Reads of up to MM2C_FIN_LDS_REGIONS regions are worked in on-chip memory,
 * longer ones in the plan's scratch.  d_regs_out must not alias d_regs_in; regions and records 8-byte, anchors 16-byte aligned.  Both entries are asynchronous on
 * `stream`.  Still the host's: mm_align1_inv with ksw_ll_i16, the interleave across alignment rounds, ALT contigs, splice; mm_pair is the pair
 * plan's (mm2c_pairplan_run_device, below). */
typedef struct { int32_t dp_score, dp_max, dp_max2; uint32_t ambi_strand; int32_t n_cigar, reserved; int64_t cig0; } mm2c_pext_t;
typedef struct {
	int32_t min_cnt, min_chain_score, min_dp_max; float max_clip_ratio;    /* mm_filter_regs, hit.c:280-284 */
	float mask_level; int32_t mask_len, hard_mask_level, sub_diff;         /* mm_set_parent; sub_diff = opt->a * 2 + opt->b (map.c:265) */
	float pri_ratio; int32_t min_diff, best_n;                             /* mm_select_sub; min_diff = 2k */
	int32_t match_sc, is_sr, all_chains;                                   /* mm_set_mapq's opt->a and is_sr; MM_F_ALL_CHAINS */
} mm2c_fin_opt_t;
#define MM2C_FIN_LDS_REGIONS 128
#define MM2C_FIN_REFUSED 1
#define MM2C_FIN_INCOMPLETE 2
#define MM2C_FIN_OVER_CAP 3
typedef struct mm2c_finplan mm2c_finplan_t;
/* capacities: reads, regions (of either entry), mm2c_pext_t records; the tables' largest argument (at most MM2C_MAPQ_MAX_LOG_ARG) and opt->a */
mm2c_finplan_t *mm2c_finplan_create(int64_t n_reads, int64_t n_u_cap, int64_t n_pext_cap, int32_t max_log_arg, int32_t match_sc);
void mm2c_finplan_destroy(mm2c_finplan_t *plan);
int mm2c_finplan_apply_run_device(mm2c_finplan_t *plan, int64_t n_reads, int64_t n_regs, const int64_t *d_u_off, const mm2c_reg_t *d_regs, const int64_t *d_b_off,
                                  const void *d_b, int64_t n_b_cap, const int64_t *d_read_off, const mm2c_cig_reg_t *d_cig_regs, int64_t n_extra, const int32_t *d_extra_reg,
                                  const mm2c_extra_res_t *d_extra_res, const int64_t *d_out_off, mm2c_reg_t *d_regs_out, mm2c_pext_t *d_pext, int32_t *d_status,
                                  int64_t n_child_cap, mm2c_reg_t *d_child, int32_t *d_child_of, int64_t *d_n_child, void *stream);
/* waits for the last apply run.  MM2C_E_ARG if a region was refused, else MM2C_E_TOOBIG if one was incomplete or a child lay beyond n_child_cap (all three counts
 * are filled in either way; any pointer may be NULL) */
int mm2c_finplan_apply_check(mm2c_finplan_t *plan, int64_t *n_refused, int64_t *n_incomplete, int64_t *n_child_beyond);
int mm2c_finplan_run_device(mm2c_finplan_t *plan, const mm2c_fin_opt_t *opt, const int64_t *d_f_off, const mm2c_reg_t *d_regs_in, const int32_t *d_n_in, mm2c_pext_t *d_pext,
                            const int32_t *d_qlen, const int32_t *d_rep_len, mm2c_reg_t *d_regs_out, int32_t *d_n_out, void *stream);
/* waits for the last run.  MM2C_E_ARG if a read was refused, else MM2C_E_TOOBIG if a primary lay beyond the tables.  *n_hits_total: the sum of n_out */
int mm2c_finplan_check(mm2c_finplan_t *plan, int64_t *n_refused, int64_t *n_beyond_table, int64_t *n_hits_total);
/* milliseconds of the last runs between HIP events on their streams: the three kernels of the apply entry, fin_select; 0 for an entry that has not run */
int mm2c_finplan_last_ms(mm2c_finplan_t *plan, float *apply_ms, float *select_ms);
/* host arrays in and out; argument and offset checks (MM2C_E_ARG) come before any device work; u_off[0] and b_off[0] must be 0.  What the run does not write stays the
 * caller's; with MM2C_E_TOOBIG the outputs are complete all the same. */
int mm2c_apply_regions_batch_host(int64_t n_reads, const int64_t *u_off, const mm2c_reg_t *regs, const int64_t *b_off, const mm2c_anchor_t *b, const int64_t *read_off,
                                  const mm2c_cig_reg_t *cig_regs, int64_t n_extra, const int32_t *extra_reg, const mm2c_extra_res_t *extra_res, const int64_t *out_off,
                                  mm2c_reg_t *regs_out, mm2c_pext_t *pext, int32_t *status, int64_t n_child_cap, mm2c_reg_t *child, int32_t *child_of, int64_t *n_child);
int mm2c_finish_regions_batch_host(int64_t n_reads, const mm2c_fin_opt_t *opt, int32_t max_log_arg, const int64_t *f_off, const mm2c_reg_t *regs_in, const int32_t *n_in,
                                   int64_t n_pext, mm2c_pext_t *pext, const int32_t *qlen, const int32_t *rep_len, mm2c_reg_t *regs_out, int32_t *n_out);

/* ---- the two ends of a fragment paired on the GPU: mm_pair with mm_set_pe_thru (pe.c:45-63, 76-177; map.c:373-374) and the flip of the mate that
 * was reverse-complemented before mapping (map.c:455-466) ----
 * A stand-alone plan (kernel pair_select, one wave per fragment), byte for byte the reference's, wired into nothing.  Fragment f is the two segment reads 2f and
 * 2f + 1 (the numbering f * n_segs + s of the fragment plans).  In: the final regions of segment read r, d_regs[d_f_off[r] .. d_f_off[r] + d_n[r]) in room for
 * d_f_off[r+1] - d_f_off[r], as mm2c_finplan_run_device wrote them (its d_regs_out / d_n_out, with the f_off it took); d_pext, the records their p names (read
 * only); d_seg_len[r], the qlens; d_gap_ref[f], max_chain_gap_ref per fragment, or NULL for opt->max_gap_ref (the convention of mm2c_hitplan_run_device_multi).
 * Out: the regions in place -- only parent and the bits mapq, sam_pri, proper_frag, pe_thru of flags change, and with opt->flip qs, qe and rev of the mate j with
 * (j == 0 && pe_ori >> 1 & 1) || (j == 1 && pe_ori & 1) (qs, qe = qlen - qe, qlen - qs; map.c:455-466) -- and d_status[f].  The flip runs last, whether or not a
 * pair was found and also when one mate has no region; a fragment with one mate empty is otherwise untouched (pe.c:97-100: mm_set_pe_thru is behind the return).
 * logf((float)n_sub) of pe.c:159 comes from a table the HOST fills at creation with its own logf, 0 <= i <= max_log_arg; a fragment whose n_sub lies beyond it
 * keeps both winners' mapq as they came in, everything else of it is done, and it is counted (MM2C_E_TOOBIG from _check).
 * Refused at the entry (MM2C_E_ARG): sub_diff < 0, match_sc < 1, pe_ori outside 0..3.
 * Refused and counted per fragment (d_status[f] = 1, MM2C_E_ARG from _check; nothing else of that fragment is written and its neighbours are exact), whether or not
 * both mates have regions: a region with p == 0 or a p that names no record (the reference dereferences it); rid < 0; rs < 0 or rs >= 2^30 (the int shift of the
 * key); id not equal to the region's position, or parent outside the mate (the reference indexes regs[s][parent]); offsets or counts that leave the capacities or
 * each other.  Fragments of up to MM2C_PAIR_LDS_REGIONS regions (both mates) are worked in on-chip memory, longer ones in the plan's scratch.  Regions and records
 * 8-byte aligned; asynchronous on `stream`.  Not built: MM_F_INDEPEND_SEG, fragments of more than two segments (the reference does not pair them). */
typedef struct {
	int32_t max_gap_ref, pe_bonus;         /* opt->max_gap_ref (one scalar, when d_gap_ref is NULL), opt->pe_bonus */
	int32_t sub_diff, match_sc;            /* opt->a * 2 + opt->b, opt->a (map.c:374) */
	int32_t pe_ori, flip;                  /* opt->pe_ori; flip != 0: run map.c:455-466 */
} mm2c_pair_opt_t;
#define MM2C_PAIR_LDS_REGIONS 128
typedef struct mm2c_pairplan mm2c_pairplan_t;
/* capacities: fragments, regions, mm2c_pext_t records; the table's largest argument (at most MM2C_MAPQ_MAX_LOG_ARG) */
mm2c_pairplan_t *mm2c_pairplan_create(int64_t n_frags, int64_t n_u_cap, int64_t n_pext_cap, int32_t max_log_arg);
void mm2c_pairplan_destroy(mm2c_pairplan_t *plan);
int mm2c_pairplan_run_device(mm2c_pairplan_t *plan, const mm2c_pair_opt_t *opt, const int64_t *d_f_off, mm2c_reg_t *d_regs, const int32_t *d_n, const mm2c_pext_t *d_pext,
                             const int32_t *d_seg_len, const int32_t *d_gap_ref, int32_t *d_status, void *stream);
/* waits for the last run.  MM2C_E_ARG if a fragment was refused, else MM2C_E_TOOBIG if an n_sub lay beyond the table.  *n_proper: fragments with a proper pair */
int mm2c_pairplan_check(mm2c_pairplan_t *plan, int64_t *n_refused, int64_t *n_beyond_table, int64_t *n_proper);
/* milliseconds of the last run between HIP events on its stream */
int mm2c_pairplan_last_ms(mm2c_pairplan_t *plan, float *select_ms);
/* host arrays in and out (regs in place); argument and offset checks (MM2C_E_ARG) come before any device work.  With MM2C_E_TOOBIG, or MM2C_E_ARG for fragments
 * refused on the device, the rest is complete all the same. */
int mm2c_pair_ends_batch_host(int64_t n_frags, const mm2c_pair_opt_t *opt, int32_t max_log_arg, const int64_t *f_off, mm2c_reg_t *regs, const int32_t *n, int64_t n_pext,
                              const mm2c_pext_t *pext, const int32_t *seg_len, const int32_t *gap_ref, int32_t *status);

/* ---- seed hits -> sorted anchors on the GPU (collect_seed_hits, map.c:215-247) ----
 * One match = one query minimizer found in the index (mm_match_t, map.c:76-81, as collect_matches map.c:84-120 fills it); its hits
 * are hits[cr_off .. cr_off + n) of a hit pool (the arrays mm_idx_get returns: rid<<32 | pos<<1 | strand).  The anchors of read r are
 * written to anchors[anchor_off[r] .. anchor_off[r+1]) exactly as collect_seed_hits leaves them for mm_chain_dp (encoding map.c:232-241,
 * order of radix_sort_128x including its order among equal x), ready for mm2c_plan_run_device with the same offsets.
 * mm2c_seedplan_run_device(_n) covers the flag-free case (no MM_F_NO_DIAG / NO_DUAL / FOR_ONLY / REV_ONLY), which is map-ont;
 * mm2c_seedplan_run_device_skip adds skip_seed (map.c:122-147) for ava-ont and the strand-restricted modes. */
typedef struct {
	int64_t cr_off;
	uint32_t n;          /* mm_match_t.n */
	uint32_t q_pos;      /* query position << 1 | strand (mm128_t.y low word of the minimizer) */
	uint32_t q_span;     /* mm128_t.x & 0xff */
	uint32_t seg_tandem; /* seg_id << 1 | is_tandem (map.c:112-115) */
} mm2c_match_t;
typedef struct mm2c_seedplan mm2c_seedplan_t;
/* h_anchor_off[r+1] - h_anchor_off[r] must equal the sum of n over the matches of read r (checked on the device: mm2c_seedplan_check) */
mm2c_seedplan_t *mm2c_seedplan_create(int64_t n_reads, const int64_t *h_match_off, const int64_t *h_anchor_off);
void mm2c_seedplan_destroy(mm2c_seedplan_t *plan);
/* asynchronous on `stream`; all pointers are device memory; d_anchors needs room for h_anchor_off[n_reads] anchors */
int mm2c_seedplan_run_device(mm2c_seedplan_t *plan, const mm2c_match_t *d_matches, const uint64_t *d_hits, const int32_t *d_qlen,
                             void *d_anchors, void *stream);
/* the same with the extents of the buffers stated; a match that points outside hits[0 .. n_hits) is detected on the device and reported by
 * mm2c_seedplan_check (its read is not expanded) */
int mm2c_seedplan_run_device_n(mm2c_seedplan_t *plan, const mm2c_match_t *d_matches, int64_t n_matches, const uint64_t *d_hits, int64_t n_hits,
                               const int32_t *d_qlen, int64_t n_qlen, void *d_anchors, int64_t n_anchors, void *stream);
/* With skip_seed (map.c:122-147): all-vs-all and strand-restricted modes drop hits, so a read keeps FEWER anchors than its matches have hits.
 * flag: MM_F_NO_DIAG 0x001 | MM_F_NO_DUAL 0x002 | MM_F_FOR_ONLY 0x100000 | MM_F_REV_ONLY 0x200000 (minimap.h:8-9,28-29; -x ava-ont sets the
 * first two, options.c:84).  The name comparison strcmp(qname, name[rid]) of map.c:128 travels as ranks: d_ref_rank[rid] = rank of the
 * reference sequence's name among the DISTINCT reference names in strcmp order, d_ref_len[rid] = its length (mm_idx_seq_t.len), and per read
 * d_q_lo = number of those names below the read's name, d_q_eq = 1 when the read's name is one of them (cmp > 0 <=> rank < q_lo,
 * cmp == 0 <=> q_eq && rank == q_lo); d_ref_rank == NULL stands for qname == NULL (map.c:125).  All arrays are device memory.
 * The plan's anchor offsets are then capacities; the anchors of read r are written packed to d_anchors[off[r] .. off[r+1]) with
 * off = d_anchor_off_out (n_reads + 1 entries, device) -- hand it to mm2c_plan_set_device_offsets to chain them.  MM_SEED_SELF (map.c:241) is set. */
typedef struct {
	int32_t flag;
	const int32_t *d_ref_rank, *d_ref_len;   /* per reference sequence */
	const int32_t *d_q_lo, *d_q_eq;          /* per read */
} mm2c_seed_skip_t;
int mm2c_seedplan_run_device_skip(mm2c_seedplan_t *plan, const mm2c_match_t *d_matches, int64_t n_matches, const uint64_t *d_hits, int64_t n_hits,
                                  const int32_t *d_qlen, int64_t n_qlen, const mm2c_seed_skip_t *skip, void *d_anchors, int64_t n_anchors,
                                  int64_t *d_anchor_off_out, void *stream);
/* MM_F_HEAP_SORT (minimap.h:30; --heap-sort, main.c:245; set by -x sr, options.c:125): the following runs of the plan leave the anchors as
 * collect_seed_hits_heap does (map.c:149-213) -- the same anchors, ascending in x, but anchors with EQUAL x in the order the reference's binary heap pops
 * them instead of the order radix_sort_128x leaves.  Works with and without skip_seed. */
int mm2c_seedplan_set_heap_sort(mm2c_seedplan_t *plan, int on);   /* mm2c_tune("heap_sort", 1): the default of the seed plans created afterwards, those of
                                                                    * mm2c_seed_hits_batch_host / mm2c_seed_chain_batch_host / _pool included (a host that maps with MM_F_HEAP_SORT) */
int mm2c_seedplan_check(mm2c_seedplan_t *plan, int64_t *n_reads_with_ties);   /* waits; MM2C_E_ARG if a read's counts disagreed */
int mm2c_seedplan_last_ms(mm2c_seedplan_t *plan, float *ms);
/* *n_reads = the reads the plan's last run expanded on the sixteen waves of a workgroup (reads of more than 16 384 anchors of capacity and at most 2^20 matches,
 * with and without skip_seed; none when the environment switch MM2C_MW_SORT=0 was set as the plan was made); 0 before the first run */
int mm2c_seedplan_last_expand_mw(mm2c_seedplan_t *plan, int64_t *n_reads);
/* host buffers in, anchors out (computes the anchor offsets itself): anchor_off[n_reads+1], anchors with room for the sum of all n */
int mm2c_seed_hits_batch_host(int64_t n_reads, const int64_t *h_match_off, const mm2c_match_t *h_matches, const uint64_t *h_hits,
                              int64_t n_hits, const int32_t *h_qlen, int64_t *anchor_off, mm2c_anchor_t *anchors);

/* The index's position arrays resident in HBM (the arrays mm_idx_get, index.c, hands out pointers into: rid<<32 | pos<<1 | strand): uploaded
 * once per index, shared by every later call -- a 288 GB device holds the positions of a human genome index (about 10 GB) beside the batches.
 * With a resident pool a match's cr_off is an offset into THAT pool and no hit crosses PCIe per read any more. */
typedef struct mm2c_hitpool mm2c_hitpool_t;
mm2c_hitpool_t *mm2c_hitpool_create(const uint64_t *h_hits, int64_t n_hits);   /* NULL on failure */
int64_t mm2c_hitpool_size(const mm2c_hitpool_t *pool);
void mm2c_hitpool_destroy(mm2c_hitpool_t *pool);                                 /* not while a call that uses it is running */

/* matches in, chains out: collect_seed_hits + mm_chain_dp for a batch of reads (map.c:295-316) with the anchors staying on the GPU.
 * Big batches run in chunks of whole reads ("pipeline_chunk_anchors") on two streams: the upload of one chunk, the kernels of the
 * one before and the download of the chains of the one before that overlap; every buffer the chunks use is kept for the next call.
 * anchor_off[n_reads+1] is filled with the anchor counts' prefix sums (= the sum of n per read); u / b as mm2c_mm_chain_dp_batch_host
 * (room for one entry per anchor of the batch). */
int mm2c_seed_chain_batch_host(const mm2c_params_t *par, int min_cnt, int min_sc, int64_t n_reads, const int64_t *h_match_off,
                               const mm2c_match_t *h_matches, const uint64_t *h_hits, int64_t n_hits, const int32_t *h_qlen,
                               int64_t *anchor_off, int64_t *u_off, uint64_t *u, int64_t *b_off, mm2c_anchor_t *b);
/* the same with the hits taken from a resident pool: h_matches[i].cr_off points into `pool` */
int mm2c_seed_chain_batch_pool(const mm2c_params_t *par, int min_cnt, int min_sc, int64_t n_reads, const int64_t *h_match_off,
                               const mm2c_match_t *h_matches, const mm2c_hitpool_t *pool, const int32_t *h_qlen,
                               int64_t *anchor_off, int64_t *u_off, uint64_t *u, int64_t *b_off, mm2c_anchor_t *b);

/* ---- the host-buffer entries with skip_seed (map.c:122-147): -x ava-ont (NO_DIAG | NO_DUAL) and the strand-restricted modes (FOR_ONLY / REV_ONLY) ----
 * The skip description of mm2c_seed_skip_t with host arrays.  Names travel as ranks, as there: ref_rank[rid] = rank of reference rid's name among the distinct
 * reference names in strcmp order, ref_len[rid] = its length; per read q_lo = number of those names below the read's name, q_eq = 1 when the read's name is one of
 * them.  ref_rank == NULL stands for qname == NULL (map.c:125): no name comparison.  Every hit's rid must be below n_ref when ref_rank is given (checked before any
 * kernel runs; a resident pool records its largest rid when it is made).
 * Capacity sizes the buffers: anchors, u and b need room for the sum of all hits (n over every match).  On return anchor_off[r+1] - anchor_off[r] is the number of
 * anchors read r KEPT -- its anchors are anchors[anchor_off[r] ..) for the seed-hit entry --, and u / b hold what mm_chain_dp returns on the anchors collect_seed_hits
 * leaves with these flags.  flag == 0 gives the results of the entries above.  Flag bits other than these four are refused, as are NO_DIAG / NO_DUAL with
 * ref_rank but without ref_len, q_lo or q_eq.  mm2c_tune("heap_sort", 1) applies (collect_seed_hits_heap). */
typedef struct {
	int32_t flag;                              /* MM_F_NO_DIAG 0x001 | MM_F_NO_DUAL 0x002 | MM_F_FOR_ONLY 0x100000 | MM_F_REV_ONLY 0x200000 */
	int32_t n_ref;                             /* entries of ref_rank / ref_len */
	const int32_t *ref_rank, *ref_len;         /* host, per reference sequence; ref_rank == NULL: qname == NULL (map.c:125) */
	const int32_t *q_lo, *q_eq;                /* host, per read (required when ref_rank != NULL and flag has 0x001 | 0x002) */
} mm2c_seed_skip_host_t;
int mm2c_seed_hits_batch_host_skip(int64_t n_reads, const int64_t *h_match_off, const mm2c_match_t *h_matches, const uint64_t *h_hits,
                                   int64_t n_hits, const int32_t *h_qlen, const mm2c_seed_skip_host_t *skip,
                                   int64_t *anchor_off, mm2c_anchor_t *anchors);
int mm2c_seed_chain_batch_host_skip(const mm2c_params_t *par, int min_cnt, int min_sc, int64_t n_reads, const int64_t *h_match_off,
                                    const mm2c_match_t *h_matches, const uint64_t *h_hits, int64_t n_hits, const int32_t *h_qlen,
                                    const mm2c_seed_skip_host_t *skip,
                                    int64_t *anchor_off, int64_t *u_off, uint64_t *u, int64_t *b_off, mm2c_anchor_t *b);
int mm2c_seed_chain_batch_pool_skip(const mm2c_params_t *par, int min_cnt, int min_sc, int64_t n_reads, const int64_t *h_match_off,
                                    const mm2c_match_t *h_matches, const mm2c_hitpool_t *pool, const int32_t *h_qlen,
                                    const mm2c_seed_skip_host_t *skip,
                                    int64_t *anchor_off, int64_t *u_off, uint64_t *u, int64_t *b_off, mm2c_anchor_t *b);

/* ---- reads in: mm_sketch (sketch.c:77-143) and collect_matches (map.c:90-123) on the device ------------------------------
 * Reads are raw bytes, concatenated: read r is seq[seq_off[r] .. seq_off[r+1]) (seq_off: n_reads + 1 entries, seq_off[0] = 0, monotone).  Every byte value is
 * legal; the nucleotide table of sketch.c:9-26 applies.  A read of length 0 has no minimizers.  In the three entries mm2c_sketch_batch, mm2c_sketch_match_batch and
 * mm2c_read_chain_batch every read is ONE segment with rid 0, as collect_minimizers (map.c:64-77) with n_segs = 1; paired and multi-segment reads (n_segs > 1,
 * --frag, -x sr) and the max_occ re-chaining of map.c:318-340 (-x sr sets mid_occ = 1000, max_occ = 5000, options.c:138-139) go through the fragment entries
 * further down.  Results are bit for bit those of the reference, in its order (minimizers, matches, mini_pos).  A read is a fragment of one segment, for
 * which the tagging step has nothing to do and is skipped: the sketch and the sketch-and-match entries of the two families are one code path each.
 * Out of scope here -- a host that needs one of these keeps its own sketching for those reads:
 *   - SDUST masking (sdust_thres > 0, map.c:73-74; no preset sets it, options.c:22);
 *   - alignment.
 * The index itself is built here too (mm2c_minidx_build, below).  Two parts of mm_idx_t stay with the host: the packed reference sequence mi->S with the
 * sequence names (a host that aligns or prints names keeps its own), and .mmi files (mm_idx_dump / mm_idx_load); multi-part indices (-I) are not built. */

/* A minimizer index resident on every configured device (as mm2c_hitpool_create keeps the pool): one row per indexed minimizer, keys[i] = the minimizer
 * (mm128_t.x >> 8), its hits pool[cr_off[i] .. cr_off[i] + n[i]).  A lookup returns exactly what mm_idx_get (index.c:81-98) returns: (cr_off, n) for a key that
 * is present, n = 0 for an absent one.  MM2C_E_ARG (NULL returned, mm2c_last_error says why): k outside 1..28, w outside 1..255, a duplicate key,
 * a key >= 2^(2k), an offset + n outside the pool.  A minimap2 host rebuilds each key from its hash buckets: (kh_key >> 1) << b | bucket; a kh_key & 1 row
 * has n = 1 and its one hit in the value (put it into the pool). */
typedef struct mm2c_minidx mm2c_minidx_t;
mm2c_minidx_t *mm2c_minidx_create(const mm2c_hitpool_t *pool, int k, int w, int is_hpc, int64_t n_keys, const uint64_t *keys,
                                  const int64_t *cr_off, const uint32_t *n);
void mm2c_minidx_destroy(mm2c_minidx_t *idx);                                    /* not while a call that uses it is running */
/* the lookups on their own (tests): n_q keys in, (cr_off, n) out, on the primary device */
int mm2c_minidx_lookup(const mm2c_minidx_t *idx, int64_t n_q, const uint64_t *keys, int64_t *cr_off, uint32_t *n);

/* The index built on the device from the sequences themselves: what mm_idx_gen + worker_post (index.c:191-233) yield, as the rows
 * above -- keys = x >> 8 ascending, each once (the span in x's low 8 bits is dropped: two minimizers that differ only in span are one key); a key's hits
 * are its y values ascending, y = rid << 32 | pos << 1 | strand with rid = the sequence's number; one pool slot per hit, singletons included.  Sequences
 * are laid out as the reads of the reads-in entries (seq_off: n_seqs + 1 entries); a sequence of length 0 is legal and contributes nothing; every byte
 * value is legal.  They are sketched in chunks of whole sequences of up to mm2c_tune("index_chunk_bases", default 2^27) bases -- a longer sequence is a
 * chunk of its own -- at about 20 bytes of device memory per base of a chunk, plus about 50 bytes per minimizer of the whole list while it is sorted.
 * The index owns its pool (mm2c_minidx_pool; mm2c_minidx_destroy frees it, which it does NOT do for the caller's pool of mm2c_minidx_create), and both
 * are replicated to every configured device.  *mid_occ (may be NULL) = mm2c_minidx_cal_max_occ(idx, mid_occ_frac).
 * NULL on failure; mm2c_last_error then starts with the code's name.  Refused before any device work: k outside 1..28, w outside 1..255, seq_off[0] != 0 or
 * seq_off not monotone (MM2C_E_ARG); a sequence of 2^31 bases or more (pos << 1 must fit 32 bits), more than 2^31 - 1 sequences (MM2C_E_TOOBIG).  More
 * than 2^32 - 1 keys: MM2C_E_TOOBIG, as mm2c_minidx_create. */
mm2c_minidx_t *mm2c_minidx_build(int k, int w, int is_hpc, int64_t n_seqs, const int64_t *seq_off, const uint8_t *seq,
                                 float mid_occ_frac, int *mid_occ);
int64_t mm2c_minidx_n_keys(const mm2c_minidx_t *idx);
int64_t mm2c_minidx_n_hits(const mm2c_minidx_t *idx);                  /* sum of n over the rows (a built index: the size of its pool) */
const mm2c_hitpool_t *mm2c_minidx_pool(const mm2c_minidx_t *idx);      /* for mm2c_seed_chain_batch_pool(_skip); never destroy the pool of a built index */
/* mm_idx_cal_max_occ (index.c:164-185) on the device, also for an index made by mm2c_minidx_create: the (uint32_t)((1. - f) * n_keys)-th smallest n
 * (from 0) plus 1, f the float widened to double; INT32_MAX for f <= 0.  An index without keys gives INT32_MAX (the reference is undefined there: it
 * reads a[0] of an empty array).  A negative MM2C_E_* code on failure. */
int mm2c_minidx_cal_max_occ(const mm2c_minidx_t *idx, float frac);
/* download: keys / cr_off / n (mm2c_minidx_n_keys entries each) and pool (mm2c_minidx_n_hits entries); any pointer may be NULL.  For an index made by
 * mm2c_minidx_create this is the caller's table sorted by key, and `pool` is left untouched (the pool is the caller's). */
int mm2c_minidx_export(const mm2c_minidx_t *idx, uint64_t *keys, int64_t *cr_off, uint32_t *n, uint64_t *pool);
/* what mm2c_minidx_build processed and where its time went, summed since mm2c_init or the last reset.  h2d_ns and sketch_ns (sketch and tagging) are device
 * time between HIP events; sort_ns, group_ns, occ_ns and replicate_ns are host time around stages that end in a stream synchronise */
typedef struct { uint64_t calls, chunks, bases, minimizers, keys, h2d_ns, sketch_ns, sort_ns, group_ns, occ_ns, replicate_ns; } mm2c_index_stats_t;
void mm2c_get_index_stats(mm2c_index_stats_t *out);
void mm2c_reset_index_stats(void);

/* Results of the reads-in entries: LIBRARY-OWNED and reusable (the counts are only known once the device has run).  Create one, hand it to as many calls
 * as you like (each overwrites it; the arrays stay valid until the next call on the same object or mm2c_read_result_free).  Fields an entry does not fill
 * have count 0.  Offsets have n_reads + 1 entries. */
typedef struct {
	int64_t n_reads;
	/* mm2c_sketch_batch: the mm128_t list mm_sketch appends per read, x = hash << 8 | span, y = pos << 1 | strand (rid 0) */
	int64_t n_sketch; int64_t *sketch_off; mm2c_anchor_t *sketch;
	/* mm2c_sketch_match_batch: collect_matches per read -- matches in minimizer order, their anchor counts' prefix sums */
	int64_t n_matches; int64_t *match_off; mm2c_match_t *matches;
	/* both reads-in entries: anchor_off (mm2c_sketch_match_batch: sum of n per read; mm2c_read_chain_batch: the anchors each read KEPT), rep_len per read
	 * (map.c:104-110,120) and mini_pos per read (q_span << 32 | q_pos >> 1 of every kept match, what mm_est_err / mm_set_mapq read) */
	int64_t n_anchors; int64_t *anchor_off;
	int32_t *rep_len;
	int64_t n_mini_pos; int64_t *mini_off; uint64_t *mini_pos;
	/* mm2c_read_chain_batch: what mm_chain_dp returns per read, as mm2c_mm_chain_dp_batch_host lays it out */
	int64_t n_u, n_b; int64_t *u_off; uint64_t *u; int64_t *b_off; mm2c_anchor_t *b;
	void *priv;
	/* mm2c_frag_chain_batch (behind priv: every field above keeps its offset): the fragments whose chains come from the second pass with max_occ, and one
	 * byte per fragment saying so.  0 / NULL after every other entry */
	int64_t n_rechained; uint8_t *rechained;
} mm2c_read_result_t;
mm2c_read_result_t *mm2c_read_result_create(void);
void mm2c_read_result_free(mm2c_read_result_t *res);

/* mm_sketch for every read of a batch with w (1..255), k (1..28), is_hpc (MM_I_HPC) -> res->sketch_off / sketch.  This entry and mm2c_sketch_match_batch take the
 * batch in one pass: about 20 bytes of device memory per base (a host with more bases than that calls them per mini-batch; mm2c_read_chain_batch chunks itself). */
int mm2c_sketch_batch(int k, int w, int is_hpc, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, mm2c_read_result_t *res);
/* reads in, matches out: mm_sketch with the index's k / w / is_hpc, then collect_matches with max_occ = mid_occ.  Every minimizer with t < mid_occ gives a
 * match, t = 0 included; is_tandem compares with the neighbours in the unfiltered list; cr_off points into the index's pool.  Fills match_off / matches,
 * anchor_off, rep_len, mini_off / mini_pos (the sketch fields stay empty). */
int mm2c_sketch_match_batch(const mm2c_minidx_t *idx, int mid_occ, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, mm2c_read_result_t *res);
/* reads in, chains out: sketch -> matches -> seed hits -> DP -> epilogue on the device, in chunks of whole reads ("read_chunk_bases", mm2c_tune, default
 * 2^27 bases); per chunk only the per-read counts come back before the chains.  par / min_cnt / min_sc as mm2c_seed_chain_batch_pool; skip as
 * mm2c_seed_chain_batch_pool_skip (NULL: no skip_seed); mm2c_tune("heap_sort", 1) applies.  Fills anchor_off, u_off / u, b_off / b, rep_len,
 * mini_off / mini_pos; the results equal mm2c_seed_chain_batch_pool(_skip) fed the matches of mm2c_sketch_match_batch. */
int mm2c_read_chain_batch(const mm2c_params_t *par, int min_cnt, int min_sc, const mm2c_minidx_t *idx, int mid_occ, int64_t n_reads,
                          const int64_t *seq_off, const uint8_t *seq, const mm2c_seed_skip_host_t *skip, mm2c_read_result_t *res);

/* ---- fragments: paired and multi-segment reads (mm_map_frag with n_segs > 1, map.c:272-340) ----
 * The batch is laid out as above -- n_reads SEGMENTS concatenated, with seq_off -- and frag_off (n_frags + 1 entries, frag_off[0] = 0, monotone, last = n_reads)
 * groups consecutive segments into fragments: fragment g holds the segments frag_off[g] .. frag_off[g+1]), with the segment ids 0 .. n - 1 in that order.
 * As collect_minimizers (map.c:64-77) does, each segment is sketched with rid = its id and its positions are shifted by the lengths of the segments before it
 * (y += (uint64_t)seg << 32 | sum << 1); the fragment's minimizer list is its segments' lists one after another, and collect_matches runs over that one list:
 * is_tandem compares neighbours across a segment boundary too, the rep_len recurrence runs on through it, seg_id = y >> 32 goes into seg_tandem, and qlen is the
 * sum of the segment lengths.  A segment of length 0 contributes nothing but keeps its id; a fragment whose total length is 0 yields nothing (map.c:287).
 * RESULTS ARE PER FRAGMENT: res->n_reads is n_frags and every offset array has n_frags + 1 entries.
 * Refused before any device work: a malformed frag_off, an empty fragment, a fragment of more than MM_MAX_SEG = 255 segments (MM2C_E_ARG); a fragment whose total
 * length does not fit 31 bits, or a non-empty segment that starts 2^30 bases or more into its fragment -- `sum << 1` (map.c:72) overflows the reference's int there
 * and would spill into the segment id (MM2C_E_TOOBIG). */
/* collect_minimizers for every fragment -> res->sketch_off / sketch */
int mm2c_sketch_frag_batch(int k, int w, int is_hpc, int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq,
                           mm2c_read_result_t *res);
/* fragments in, matches out: collect_matches with max_occ = occ over every fragment's joined list; fills what mm2c_sketch_match_batch fills */
int mm2c_sketch_match_frag_batch(const mm2c_minidx_t *idx, int occ, int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off,
                                 const uint8_t *seq, mm2c_read_result_t *res);
/* fragments in, chains out, with the re-chain of map.c:318-340: every fragment is chained with mid_occ; a kernel then decides per fragment, from the chains on the
 * device, rechain = (max_occ > mid_occ && rep_len > 0) && (no chain || the best chain -- the FIRST with the strictly largest score -- does not span all n_segs
 * segments); the flagged fragments' minimizers are compacted on the device (the sketch is not redone) and run through lookups, seed hits, DP and epilogue a second
 * time with max_occ.  For exactly those fragments anchor_off, rep_len, mini_pos, u and b are the second pass's; the output is in fragment order, as if one pass
 * had made it.  max_occ <= mid_occ switches the second pass off.  Chunks of "read_chunk_bases" bases are cut between fragments, never inside one.
 * Every fragment must have exactly par->n_segs segments (mm_chain_dp gets the fragment's own n_segs, chain.c:206; MM2C_E_ARG otherwise): a host with fragments of
 * different segment counts makes one call per count.  par->max_dist_x / max_dist_y are the call's: under -x sr they depend on the fragment's total length
 * (max_dist_y = max(qlen_sum, max_gap), max_dist_x = max(max_frag_len - qlen_sum, max_gap), map.c:306-314): fixed-length pairs are one call of this entry,
 * fragments of mixed lengths one call of mm2c_frag_chain_batch_gaps below, which makes the two distances per fragment.  skip: its per-read arrays are per fragment.  mm2c_tune("heap_sort", 1) applies (-x sr sets MM_F_HEAP_SORT). */
int mm2c_frag_chain_batch(const mm2c_params_t *par, int min_cnt, int min_sc, const mm2c_minidx_t *idx, int mid_occ, int max_occ, int64_t n_frags,
                          const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, const mm2c_seed_skip_host_t *skip,
                          mm2c_read_result_t *res);
/* The same with the chaining distances of map.c:305-314 made PER FRAGMENT, on the device, from the fragment's total length qlen_sum and four scalars of the
 * mapping options:
 *     max_dist_y = is_sr ? max(qlen_sum, max_gap) : max_gap
 *     max_dist_x = max_gap_ref > 0 ? max_gap_ref : max_frag_len > 0 ? max(max_frag_len - qlen_sum, max_gap) : max_gap
 * par->max_dist_x / max_dist_y are not used for chaining, but par is checked as a whole as in every entry (max_dist_x >= 0); everything else -- par->n_segs (one call per segment count), the results, the re-chain (a re-chained fragment keeps
 * its pair), the chunks -- is mm2c_frag_chain_batch's.  The DP runs through mm2c_plan_set_task_dists.  Refused before any device work: gaps == NULL,
 * max_gap < 0, and whatever mm2c_frag_chain_batch refuses. */
typedef struct { int32_t is_sr, max_gap, max_gap_ref, max_frag_len; } mm2c_frag_gaps_t;
int mm2c_frag_chain_batch_gaps(const mm2c_params_t *par, int min_cnt, int min_sc, const mm2c_minidx_t *idx, int mid_occ, int max_occ, const mm2c_frag_gaps_t *gaps,
                               int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq,
                               const mm2c_seed_skip_host_t *skip, mm2c_read_result_t *res);
/* the pairs the last mm2c_frag_chain_batch_gaps call on `res` chained with: dists[2 g] = max_dist_x (the reference's frag_gap, map.c:341), dists[2 g + 1] =
 * max_dist_y of fragment g, as the device made them; library-owned like the arrays of the result.  NULL / 0 after every other entry. */
int mm2c_read_result_task_dists(const mm2c_read_result_t *res, const int32_t **dists, int64_t *n_frags);
/* the fragment entries since mm2c_init or the last reset: calls, fragments processed, fragments re-chained, and the time of the second pass on the call's
 * stream.  rechain_ns is the time ELAPSED between two HIP events, one in front of the decision kernel and one behind the second pass's epilogue: it holds the
 * decision, the compaction, the second lookups -> epilogue AND the gaps in which the stream waits for the host (the counts coming down, the second pass's seed
 * and chain plans being set up).  It is what the second pass adds to a call, not the busy time of its kernels. */
typedef struct { uint64_t calls, fragments, rechained, rechain_ns; } mm2c_frag_stats_t;
void mm2c_get_frag_stats(mm2c_frag_stats_t *out);
void mm2c_reset_frag_stats(void);
/* device time of the sketch and of the lookups (HIP events around them, summed since mm2c_init or the last reset), and what they processed */
typedef struct { uint64_t calls, chunks, bases, minimizers, matches, h2d_ns, sketch_ns, lookup_ns; } mm2c_sketch_stats_t;
void mm2c_get_sketch_stats(mm2c_sketch_stats_t *out);
void mm2c_reset_sketch_stats(void);

/* ---- anchor streams on disk (csrc/anchor_stream.c documents the layout) ------------------------ */
typedef struct {
	mm2c_params_t par;            /* scalars of the mm_chain_dp calls the tasks came from */
	int32_t min_cnt, min_sc;      /* mm_chain_dp arguments 6-7, used by the backtrack only */
	int64_t n_tasks, total;
	int64_t *offsets;             /* n_tasks + 1, offsets[0] = 0; malloc'ed by the readers */
	mm2c_anchor_t *anchors;       /* total */
} mm2c_stream_t;
int  mm2c_stream_write(const char *path, const mm2c_params_t *par, int min_cnt, int min_sc, int64_t n_tasks,
                       const int64_t *offsets, const mm2c_anchor_t *anchors);
int  mm2c_stream_read(const char *path, mm2c_stream_t *out);
/* import what `minimap2 --print-seeds` prints before chaining (RS / SD lines, map.c:298-303) */
int  mm2c_stream_from_seed_dump(const char *text_path, const mm2c_params_t *par, int min_cnt, int min_sc, mm2c_stream_t *out);
void mm2c_stream_free(mm2c_stream_t *s);

/* statistics since mm2c_init: tasks, anchors, and kernel launches issued through any entry point */
typedef struct { uint64_t tasks, anchors, launches, segments, host_call_ns, passes; } mm2c_stats_t;   /* segments: pieces the host
   paths cut tasks into; host_call_ns: wall time inside the host-buffer entry points, summed over calling threads; passes: GPU
   passes they issued (concurrent small calls are combined into one pass) */
void mm2c_get_stats(mm2c_stats_t *out);

/* Where the time of the host-batch entries goes (mm2c_seed_chain_batch_host / _pool, mm2c_mm_chain_dp_batch_host, mm2c_chain_batch_host), summed
 * since mm2c_init or the last mm2c_reset_stage_stats.  Host stages are wall time of the calling thread(s); device stages are HIP-event time on
 * the stream of each chunk (chunks of one call overlap on two streams, so the device stages may add up to more than total_ns). */
typedef struct {
	uint64_t calls, chunks;      /* entries served, and the chunks their batches were pipelined in */
	uint64_t total_ns;           /* wall time inside the entries */
	uint64_t alloc_ns, n_alloc;  /* hipMalloc / hipHostMalloc: device-cache misses, arena growth, pinned staging (whole library) */
	uint64_t free_ns, n_free;    /* hipFree / hipHostFree and the device waits in front of them (whole library) */
	uint64_t setup_ns;           /* host: checking the offsets, launch orders, plan objects and their small synchronous uploads */
	uint64_t h2d_ns;             /* device: uploads (matches, hits or anchors, per-read metadata) */
	uint64_t seed_ns;            /* device: seed hits -> sorted anchors */
	uint64_t dp_ns;              /* device: window prepass + chaining DP (the reads-in and fragment entries add their chain plans' own timers here) */
	uint64_t epi_ns;             /* device: v[], backtrack, chain order */
	uint64_t d2h_ns;             /* device: downloads of offsets and chains (or f / p) */
	uint64_t wait_ns;            /* host: blocked on a stream or an event */
} mm2c_stage_stats_t;
void mm2c_get_stage_stats(mm2c_stage_stats_t *out);
void mm2c_reset_stage_stats(void);

#ifdef __cplusplus
}
#endif

/*
 * C++-linkage symbols with the reference's exact prototypes are defined in csrc/mm2chain_dropin.cpp
 * (chain_hardware.h:68-71; the reference compiles every .c with $(CXX), Makefile:184-185, so its objects import
 * _Z18run_chaining_on_hwliiiifP7mm128_tPiS1_Phliff, _Z13hardware_initlPc, _Z7cleanupv):
 *   int  run_chaining_on_hw(long n, int max_dist_x, int max_dist_y, int bw, int q_span, float avg_qspan, mm128_t *a,
 *                           int *f, int *p, unsigned char *num_subparts, long total_subparts, int tid,
 *                           float hw_time_pred, float sw_time_pred);   // computes V2 = what the FPGA kernel computes
 *   bool hardware_init(long, char *);
 *   void cleanup();
 */

#endif /* MM2CHAIN_H */
