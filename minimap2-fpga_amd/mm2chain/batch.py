"""Host-side mirror of the reference's dispatch surface for the chaining DP, over the C ABI.

ChainPlan   : a CSR batch of tasks resident in HBM (the throughput path; north-star "many reads in flight").
chain_task  : one task from host memory, the extended run_chaining_on_hw (chain_hardware.h:68 + the five scalars).
run_chaining_on_hw / hardware_init / cleanup : the reference's own entry points, called through their C++ symbols.
mm_chain_dp : the whole reference function (mmpriv.h:65), DP on the GPU, epilogue on the host.
torch is plumbing only: device memory, streams.
"""
import contextlib
import ctypes as C
import os
import numpy as np
import torch

from . import _native as N
from .params import Params

_inited = False


def init(device=None):
    """hardware_init equivalent (main.c:367).  Raises when no HIP device is usable."""
    global _inited
    lib = N.load()
    if device is None:
        # (MM2C_DEVICES in the environment names the devices when the caller names none: mm2c_init(-1), as for a host whose init hook carries no ordinals)
        device = torch.cuda.current_device() if torch.cuda.is_available() and not os.environ.get("MM2C_DEVICES") else -1
    N.check(lib.mm2c_init(int(device)), "mm2c_init")
    _inited = True


def init_devices(ordinals):
    """several devices in one process (the reference's NUM_HW_KERNELS scaffolding, chain_hardware.cpp:9-23): ordinals[0] is the primary
    device; the host-batch entries split big batches across all of them.  An ordinal may repeat."""
    global _inited
    arr = (C.c_int * len(ordinals))(*[int(d) for d in ordinals])
    N.check(N.load().mm2c_init_devices(len(ordinals), arr), "mm2c_init_devices")
    _inited = True


def device_count():
    return N.load().mm2c_device_count()


def split_tasks(offsets, n_parts):
    """mm2c_split_tasks: bounds of n_parts contiguous task ranges with about equal anchor counts (no GPU involved)"""
    off = _i64(offsets)
    bounds = np.zeros(n_parts + 1, dtype=np.int64)
    N.check(N.load().mm2c_split_tasks(off.size - 1, off.ctypes.data, int(n_parts), bounds.ctypes.data), "mm2c_split_tasks")
    return bounds


def split_model(preset="map-ont"):
    """the HW/SW split constants for this hardware (chain.c:80-81; include/mm2chain_split.h) as a dict K1_HW, K2_HW, C_HW, K_SW, C_SW"""
    v = [C.c_float(0) for _ in range(5)]
    N.check(N.load().mm2c_split_model(preset.encode(), *[C.byref(x) for x in v]), "mm2c_split_model")
    return dict(zip(("K1_HW", "K2_HW", "C_HW", "K_SW", "C_SW"), [x.value for x in v]))


def shutdown():
    """cleanup() equivalent (main.c:430)"""
    global _inited
    if _inited:
        N.load().mm2c_shutdown()
        _inited = False


def tune(key, value):
    N.check(N.load().mm2c_tune(key.encode(), int(value)), "mm2c_tune")


def tune_get(key):
    """(value, default) of a tuning knob; needs no device"""
    value, dflt = C.c_int64(0), C.c_int64(0)
    N.check(N.load().mm2c_tune_get(key.encode(), C.byref(value), C.byref(dflt)), "mm2c_tune_get")
    return value.value, dflt.value


def tune_keys():
    """{key: environment variable or None} of every tuning knob, in the order of the library's table (csrc/knobs.def)"""
    lib, keys, k = N.load(), {}, 0
    key, env = C.c_char_p(), C.c_char_p()
    while lib.mm2c_tune_key(k, C.byref(key), C.byref(env)) == 0:
        keys[key.value.decode()] = env.value.decode() if env.value else None
        k += 1
    return keys


@contextlib.contextmanager
def tuned(**knobs):
    """with tuned(coop_plans=1, fuse_st=0): ... -- sets the knobs in the order given and, on the way out (also by an exception, also when a later knob of the
    list is refused), puts back in reverse order what each of them held before"""
    with contextlib.ExitStack() as undo:
        for key, value in knobs.items():
            before = tune_get(key)[0]
            tune(key, value)
            undo.callback(tune, key, before)
        yield


def device_info():
    lib = N.load()
    name = C.create_string_buffer(256)
    cu, mem = C.c_int(0), C.c_size_t(0)
    N.check(lib.mm2c_device_info(name, 256, C.byref(cu), C.byref(mem)), "mm2c_device_info")
    return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}


def last_host_variant():
    """which DP instantiation the last host-buffer entry launched ("chain_dp_tile<...> loop=asm ... compact=1")"""
    buf = C.create_string_buffer(256)
    N.check(N.load().mm2c_last_host_variant(buf, 256), "mm2c_last_host_variant")
    return buf.value.decode()


def device_identity():
    """{"ordinal", "pci_bus_id", "arch"} of the calling thread's library device (mm2c_device_identity)"""
    lib = N.load()
    o = C.c_int(-1); bus = C.create_string_buffer(64); arch = C.create_string_buffer(256)
    N.check(lib.mm2c_device_identity(C.byref(o), bus, 64, arch, 256), "mm2c_device_identity")
    return {"ordinal": o.value, "pci_bus_id": bus.value.decode(), "arch": arch.value.decode()}


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _stream(stream):
    """the stream argument of a run: the caller's, or torch's current stream (so torch.cuda.Event timing and torch.cuda.synchronize see the run)"""
    return stream if stream is not None else torch.cuda.current_stream().cuda_stream


def _out(t, shape, dtype, device, need_bytes, same="bytes"):
    """an output tensor of a run: the given one, or a new one of `shape` and `dtype`; on the device, contiguous and of at least need_bytes bytes; same="dtype": of
    that dtype, same="width": of that (integer) dtype's element size"""
    if t is None:
        t = torch.empty(shape, dtype=dtype, device=device)
    assert t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= need_bytes
    assert same == "bytes" or (t.dtype == dtype if same == "dtype" else t.element_size() * 8 == torch.iinfo(dtype).bits)
    return t


def _i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


def _reg_rows(regs):
    """regions (REG_DTYPE or their bytes) as uint8 [., 80]"""
    return np.ascontiguousarray(regs).view(np.uint8).reshape(-1, REG_DTYPE.itemsize)


def _anchor_rows(b):
    return np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 2)


def _fit(n, *pairs):
    """the fit test of the host entries: every (offsets, rows of the array they index) pair of a batch of n reads stays inside its array"""
    return n <= 0 or all(o[0] >= 0 and o.max() <= rows for o, rows in pairs)


class _Handle:
    """owner of one native handle: create or raise, close() (more than once is fine; handle is None afterwards), and a __del__ that swallows"""
    _destroy = None                                                            # the C entry that frees the handle

    def _create(self, fn, *args, code=-1, what=None):
        self.lib = N.load()
        self.handle = getattr(self.lib, fn)(*args)
        if not self.handle:
            N.check(code, what or fn)

    def _ms(self, fn, n=1):
        """n floats out of the C entry `fn`, which takes n float pointers behind the handle"""
        v = [C.c_float(0) for _ in range(n)]
        N.check(getattr(self.lib, fn)(self.handle, *[C.byref(x) for x in v]), fn)
        return tuple(x.value for x in v)

    def close(self):
        if self.handle:
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ChainPlan(_Handle):
    """mm2c_plan_t: offsets + longest-first order + workspace on the device; run() enqueues the DP."""

    _destroy = "mm2c_plan_destroy"

    def __init__(self, params: Params, offsets):
        off = _i64(offsets)
        self.n_tasks = off.size - 1
        self.params = params
        self._create("mm2c_plan_create", C.byref(params), self.n_tasks, _np_ptr(off))
        self.total = self.lib.mm2c_plan_total_anchors(self.handle)

    def run(self, anchors: torch.Tensor, f: torch.Tensor, p: torch.Tensor, avg: torch.Tensor = None, stream=None):
        """anchors: int64 [total, 2] on the GPU; f, p: int32 [total] on the GPU.  Asynchronous on `stream`
        (default: torch's current stream, so torch.cuda.Event timing and torch.cuda.synchronize see it)."""
        assert anchors.is_cuda and f.is_cuda and p.is_cuda, "HBM-resident path needs device tensors"
        assert anchors.dtype == torch.int64 and anchors.is_contiguous() and f.dtype == torch.int32 and p.dtype == torch.int32
        assert f.is_contiguous() and p.is_contiguous()
        if avg is not None:
            assert avg.is_cuda and avg.dtype == torch.float32 and avg.is_contiguous()
        st = _stream(stream)
        # the extents of the tensors go with the pointers: the library refuses buffers shorter than the plan (cf. chain_hardware.cpp:34-37)
        N.check(self.lib.mm2c_plan_run_device_n(self.handle, anchors.data_ptr(), anchors.numel() // 2, avg.data_ptr() if avg is not None else None,
                                                avg.numel() if avg is not None else 0, f.data_ptr(), f.numel(), p.data_ptr(), p.numel(), st),
                "mm2c_plan_run_device_n")

    def set_device_offsets(self, offsets: torch.Tensor = None):
        """task sizes that only the device knows (SeedPlan.run_skip): the kernels take the CSR offsets from this int64 device tensor
        [n_tasks + 1]; None goes back to the plan's own.  The tensor must stay alive while the plan uses it."""
        if offsets is not None:
            assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.numel() == self.n_tasks + 1 and offsets.is_contiguous()
        self._dev_off = offsets
        N.check(self.lib.mm2c_plan_set_device_offsets(self.handle, offsets.data_ptr() if offsets is not None else None), "mm2c_plan_set_device_offsets")

    def set_task_dists(self, dists: torch.Tensor = None):
        """chaining distances per task: an int32 device tensor [n_tasks, 2] of (max_dist_x, max_dist_y), every value >= 0, in the place of the
        params' two scalars; None goes back to them.  The tensor is read when a run executes and must stay alive while the plan uses it."""
        if dists is not None:
            assert dists.is_cuda and dists.dtype == torch.int32 and dists.numel() == 2 * self.n_tasks and dists.is_contiguous()
        self._task_dists = dists
        N.check(self.lib.mm2c_plan_set_task_dists(self.handle, dists.data_ptr() if dists is not None else None), "mm2c_plan_set_task_dists")

    def predict(self, anchors: torch.Tensor, stream=None):
        """chain.c:53-78 on the GPU: returns (num_subparts uint8 [total], total_subparts int64 [n_tasks],
        total_trip_count int64 [n_tasks]) as device tensors"""
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.numel() == 2 * self.total
        ns = torch.empty(self.total, dtype=torch.uint8, device=anchors.device)
        ts = torch.empty(self.n_tasks, dtype=torch.int64, device=anchors.device)
        tt = torch.empty(self.n_tasks, dtype=torch.int64, device=anchors.device)
        st = _stream(stream)
        N.check(self.lib.mm2c_plan_predict_device(self.handle, anchors.data_ptr(), ns.data_ptr(), ts.data_ptr(), tt.data_ptr(), st),
                "mm2c_plan_predict_device")
        return ns, ts, tt

    def chains(self, anchors: torch.Tensor, f: torch.Tensor, p: torch.Tensor, min_cnt: int, min_sc: int, stream=None):
        """the epilogue of mm_chain_dp (chain.c:106-111,348-422) on the GPU, after run() on the same stream.  Returns device
        tensors (u_off int64 [n_tasks+1], u int64 [total], b_off int64 [n_tasks+1], b int64 [total, 2]); only the first
        u_off[-1] / b_off[-1] entries of u / b are defined."""
        assert anchors.is_cuda and anchors.dtype == torch.int64 and f.dtype == torch.int32 and p.dtype == torch.int32
        dev = anchors.device
        u_off = torch.empty(self.n_tasks + 1, dtype=torch.int64, device=dev)
        b_off = torch.empty(self.n_tasks + 1, dtype=torch.int64, device=dev)
        u = torch.empty(max(self.total, 1), dtype=torch.int64, device=dev)
        b = torch.empty((max(self.total, 1), 2), dtype=torch.int64, device=dev)
        st = _stream(stream)
        N.check(self.lib.mm2c_plan_chains_device_n(self.handle, anchors.data_ptr(), anchors.numel() // 2, f.data_ptr(), f.numel(), p.data_ptr(), p.numel(),
                                                   min_cnt, min_sc, u_off.data_ptr(), u_off.numel(), u.data_ptr(), u.numel(), b_off.data_ptr(),
                                                   b_off.numel(), b.data_ptr(), b.numel() // 2, st), "mm2c_plan_chains_device_n")
        return u_off, u, b_off, b

    def last_epilogue_ms(self):
        return self._ms("mm2c_plan_last_epilogue_ms")[0]

    def last_kernel_ms(self):
        return self._ms("mm2c_plan_last_kernel_ms")[0]

    def last_route(self):
        """(pieces, pieces run with one wave each, pieces run with sixteen waves each) of the last run -- mm2c_plan_last_route"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        N.check(self.lib.mm2c_plan_last_route(self.handle, C.byref(a), C.byref(b), C.byref(c)), "mm2c_plan_last_route")
        return int(a.value), int(b.value), int(c.value)

    def last_variant(self):
        """text naming the kernel instantiation the last run launched (mm2c_plan_last_variant)"""
        buf = C.create_string_buffer(192)
        N.check(self.lib.mm2c_plan_last_variant(self.handle, buf, len(buf)), "mm2c_plan_last_variant")
        return buf.value.decode()

    def last_classes(self):
        """class byte per task from the prepass of the last run (mm2c_plan_last_classes): bit 1 the 32-bit ring, bit 3 the packed f / p ring"""
        buf = (C.c_ubyte * max(self.n_tasks, 1))()
        N.check(self.lib.mm2c_plan_last_classes(self.handle, buf, self.n_tasks), "mm2c_plan_last_classes")
        return bytes(buf)[:self.n_tasks]

    def last_prepass_ms(self):
        return self._ms("mm2c_plan_last_prepass_ms")[0]


class PinnedArray:
    """numpy view of page-locked host memory from mm2c_pinned_alloc (freed when the object dies)"""

    def __init__(self, shape, dtype):
        self.lib = N.load()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = self.lib.mm2c_pinned_alloc(self.nbytes)
        if not self.ptr:
            N.check(-1, "mm2c_pinned_alloc")
        buf = (C.c_char * max(self.nbytes, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def __del__(self):
        try:
            if self.ptr:
                self.array = None
                self.lib.mm2c_pinned_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def chain_batch_host_into(params: Params, offsets, anchors, f, p, avg=None):
    """as chain_batch_host, but into caller-provided int32 arrays (e.g. PinnedArray.array); anchors may be pinned too"""
    lib = N.load()
    off = _i64(offsets)
    a = anchors.view(np.uint64).reshape(-1, 2)
    assert a.flags.c_contiguous and f.flags.c_contiguous and p.flags.c_contiguous and f.dtype == np.int32 and p.dtype == np.int32
    if off.size and (off[0] < 0 or off[-1] > a.shape[0] or off[-1] > f.size or off[-1] > p.size):
        raise ValueError("offsets do not fit the arrays")
    avg_p = None
    if avg is not None:
        avg = np.ascontiguousarray(avg, dtype=np.float32)
        avg_p = _np_ptr(avg)
    N.check(lib.mm2c_chain_batch_host(C.byref(params), off.size - 1, _np_ptr(off), _np_ptr(a), avg_p, _np_ptr(f), _np_ptr(p)),
            "mm2c_chain_batch_host")


def chain_batch_host(params: Params, offsets, anchors, avg=None):
    """Whole batch from host numpy arrays (uint64 [total,2]); returns (f, p) int32 arrays.  PCIe included."""
    lib = N.load()
    off = _i64(offsets)
    a = np.ascontiguousarray(anchors).view(np.uint64).reshape(-1, 2)
    total = int(off[-1] - off[0]) if off.size else 0
    if off.size and (off[0] < 0 or off[-1] > a.shape[0]):
        raise ValueError("offsets do not fit the anchor array")
    f = np.empty(int(off[-1]) if off.size else 0, dtype=np.int32)
    p = np.empty_like(f)
    avg_p = None
    if avg is not None:
        avg = np.ascontiguousarray(avg, dtype=np.float32)
        avg_p = _np_ptr(avg)
    N.check(lib.mm2c_chain_batch_host(C.byref(params), off.size - 1, _np_ptr(off), _np_ptr(a), avg_p, _np_ptr(f), _np_ptr(p)),
            "mm2c_chain_batch_host")
    del total
    return f, p


def chain_task(params: Params, anchors, avg_qspan_scaled, tid=0):
    """One task, synchronous, stock-CPU (V1) semantics: the extended run_chaining_on_hw."""
    lib = N.load()
    a = np.ascontiguousarray(anchors).view(np.uint64).reshape(-1, 2)
    n = a.shape[0]
    f = np.empty(n, dtype=np.int32)
    p = np.empty(n, dtype=np.int32)
    N.check(lib.mm2c_chain_task_host(C.byref(params), n, _np_ptr(a), float(avg_qspan_scaled), _np_ptr(f), _np_ptr(p), tid),
            "mm2c_chain_task_host")
    return f, p


def chain_task_pred(params: Params, anchors, avg_qspan_scaled, tid, hw_time_pred, sw_time_pred):
    """mm2c_chain_task_host_pred: the same call under the reference's busy protocol (chain_hardware.cpp:54-75).  Returns (ret, f, p); ret 1 = declined, f / p untouched."""
    lib = N.load()
    a = np.ascontiguousarray(anchors).view(np.uint64).reshape(-1, 2)
    n = a.shape[0]
    f = np.full(n, -77, dtype=np.int32)
    p = np.full(n, -77, dtype=np.int32)
    rc = lib.mm2c_chain_task_host_pred(C.byref(params), n, _np_ptr(a), float(avg_qspan_scaled), _np_ptr(f), _np_ptr(p), tid, float(hw_time_pred), float(sw_time_pred))
    if rc != 1:
        N.check(rc, "mm2c_chain_task_host_pred")
    return rc, f, p


def slot_stats(slot):
    """mm2c_get_slot_stats as a dict: what the call combiner of device slot `slot` has served since init"""
    st = N.SlotStats()
    N.check(N.load().mm2c_get_slot_stats(int(slot), C.byref(st)), "mm2c_get_slot_stats")
    return {k: int(getattr(st, k)) for k, _ in st._fields_ if k != "reserved"}


def _split_chains(n_tasks, u_off, u, b_off, b):
    return [(u[u_off[k]:u_off[k + 1]].copy(), b[b_off[k]:b_off[k + 1]].copy()) for k in range(n_tasks)]


def mm_chain_dp_batch(params: Params, min_cnt, min_sc, offsets, anchors, epilogue_threads=0):
    """mm2c_mm_chain_dp_batch_host: per-task list [(u uint64 [n_u], b uint64 [n_b, 2]), ...]; epilogue_threads == 0 runs the
    epilogue on the GPU, > 0 on that many host threads"""
    lib = N.load()
    off = _i64(offsets)
    a = np.ascontiguousarray(anchors).view(np.uint64).reshape(-1, 2)
    n_tasks, total = off.size - 1, int(off[-1] - off[0])
    if off[-1] > a.shape[0] or off[0] < 0:
        raise ValueError("offsets reach beyond the anchor array")
    u_off = np.zeros(n_tasks + 1, np.int64); b_off = np.zeros(n_tasks + 1, np.int64)
    u = np.zeros(max(total, 1), np.uint64); b = np.zeros((max(total, 1), 2), np.uint64)
    N.check(lib.mm2c_mm_chain_dp_batch_host(C.byref(params), min_cnt, min_sc, n_tasks, _np_ptr(off), _np_ptr(a), epilogue_threads,
                                            _np_ptr(u_off), _np_ptr(u), _np_ptr(b_off), _np_ptr(b)), "mm2c_mm_chain_dp_batch_host")
    return _split_chains(n_tasks, u_off, u, b_off, b)


def chain_epilogue_host(min_cnt, min_sc, offsets, anchors, f, p, n_threads=4):
    """mm2c_chain_epilogue_host: the epilogue on host threads from f[] / p[] (no GPU involved)"""
    lib = N.load()
    off = _i64(offsets)
    a = np.ascontiguousarray(anchors).view(np.uint64).reshape(-1, 2)
    f = np.ascontiguousarray(f, dtype=np.int32); p = np.ascontiguousarray(p, dtype=np.int32)
    n_tasks, total = off.size - 1, int(off[-1] - off[0])
    if off[-1] > a.shape[0] or off[0] < 0 or f.size < off[-1] or p.size < off[-1]:
        raise ValueError("offsets reach beyond the arrays")
    u_off = np.zeros(n_tasks + 1, np.int64); b_off = np.zeros(n_tasks + 1, np.int64)
    u = np.zeros(max(total, 1), np.uint64); b = np.zeros((max(total, 1), 2), np.uint64)
    N.check(lib.mm2c_chain_epilogue_host(min_cnt, min_sc, n_tasks, _np_ptr(off), _np_ptr(a), _np_ptr(f), _np_ptr(p), n_threads,
                                         _np_ptr(u_off), _np_ptr(u), _np_ptr(b_off), _np_ptr(b)), "mm2c_chain_epilogue_host")
    return _split_chains(n_tasks, u_off, u, b_off, b)


REG_DTYPE = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0")] +
                     [("flags", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("p", "<u8")])   # mm2c_reg_t = mm_reg1_t, 80 bytes


class RegPlan(_Handle):
    """mm2c_regplan_t: chains -> regions on the GPU (mm_gen_regs, hit.c:52-88) for batches of up to n_reads reads, n_u_cap chains, n_b_cap chain anchors"""

    _destroy = "mm2c_regplan_destroy"

    def __init__(self, n_reads, n_u_cap, n_b_cap):
        self.n_reads, self.n_u_cap, self.n_b_cap = int(n_reads), int(n_u_cap), int(n_b_cap)
        self._create("mm2c_regplan_create", self.n_reads, self.n_u_cap, self.n_b_cap)

    def run(self, u_off: torch.Tensor, u: torch.Tensor, b_off: torch.Tensor, b: torch.Tensor, qlen: torch.Tensor, hash: torch.Tensor, regs: torch.Tensor = None,
            stream=None):
        """the device epilogue's compact output (u_off / b_off int64 [n_reads + 1], u int64, b int64 [., 2]) plus qlen int32 and hash (32-bit integers) per read, all on
        the GPU; returns regs: uint8 [n_u_cap, 80], the regions of read r in rows u_off[r] .. u_off[r+1] (view the host copy as REG_DTYPE).  Asynchronous."""
        for t in (u_off, u, b_off, b, qlen, hash):
            assert t.is_cuda and t.is_contiguous()
        assert u_off.dtype == torch.int64 and b_off.dtype == torch.int64 and u_off.numel() == self.n_reads + 1 and b_off.numel() == self.n_reads + 1
        assert u.element_size() == 8 and u.numel() >= self.n_u_cap and b.element_size() == 8 and b.numel() >= 2 * self.n_b_cap
        assert qlen.dtype == torch.int32 and qlen.numel() == self.n_reads and hash.element_size() == 4 and hash.numel() == self.n_reads
        regs = _out(regs, (max(self.n_u_cap, 1), REG_DTYPE.itemsize), torch.uint8, u.device, self.n_u_cap * REG_DTYPE.itemsize)
        st = _stream(stream)
        N.check(self.lib.mm2c_regplan_run_device(self.handle, u_off.data_ptr(), u.data_ptr(), b_off.data_ptr(), b.data_ptr(), qlen.data_ptr(), hash.data_ptr(),
                                                 regs.data_ptr(), st), "mm2c_regplan_run_device")
        return regs

    def check(self):
        """waits for the run; raises if a read's chain counts disagreed with its extent of b; returns the number of reads that held equal sort keys"""
        n = C.c_int64(0)
        N.check(self.lib.mm2c_regplan_check(self.handle, C.byref(n)), "mm2c_regplan_check")
        return n.value

    def last_ms(self):
        return self._ms("mm2c_regplan_last_ms")[0]

    def last_kernel_ms(self):
        """(sort kernel, fill kernel) of the last run"""
        return self._ms("mm2c_regplan_last_kernel_ms", 2)


def gen_regs_batch(u_off, u, b_off, b, qlen, hash):
    """mm2c_gen_regs_batch_host: host arrays in, the regions of every read out (REG_DTYPE [u_off[-1] - u_off[0]], indexed like u)"""
    lib = N.load()
    uo = _i64(u_off); bo = _i64(b_off)
    uu = np.ascontiguousarray(u, dtype=np.uint64)
    bb = _anchor_rows(b)
    q = np.ascontiguousarray(qlen, dtype=np.int32); h = np.ascontiguousarray(hash, dtype=np.uint32)
    n_reads = uo.size - 1
    if bo.size != uo.size or q.size != n_reads or h.size != n_reads or not _fit(n_reads, (uo, uu.size), (bo, bb.shape[0])):
        raise ValueError("offsets do not fit the arrays")
    regs = np.zeros(max(int(uo[-1] - uo[0]), 1) if n_reads > 0 else 1, REG_DTYPE)
    N.check(lib.mm2c_gen_regs_batch_host(n_reads, _np_ptr(uo), _np_ptr(uu), _np_ptr(bo), _np_ptr(bb), _np_ptr(q), _np_ptr(h), _np_ptr(regs)),
            "mm2c_gen_regs_batch_host")
    return regs[:int(uo[-1] - uo[0]) if n_reads > 0 else 0]


def read_hash(name, qlen_sum, seed=11):
    """mm2c_read_hash: the hash mm_map_frag hands to mm_gen_regs (map.c:290-292); name: str, bytes or None.  Needs no device."""
    if isinstance(name, str):
        name = name.encode()
    return int(N.load().mm2c_read_hash(name, int(qlen_sum), int(seed)))


class HitPlan(_Handle):
    """mm2c_hitplan_t: regions -> hits on the GPU (mm_set_parent hit.c:125-186, then mm_select_sub hit.c:255-272) for batches of up to n_reads reads and n_u_cap
    regions; it stands behind a RegPlan on the same stream"""

    _destroy = "mm2c_hitplan_destroy"

    def __init__(self, n_reads, n_u_cap):
        self.n_reads, self.n_u_cap = int(n_reads), int(n_u_cap)
        self._create("mm2c_hitplan_create", self.n_reads, self.n_u_cap)

    def run(self, opt, u_off: torch.Tensor, regs_in: torch.Tensor, regs_out: torch.Tensor = None, n_out: torch.Tensor = None, stream=None):
        """opt: params.hit_opts(); u_off int64 [n_reads + 1] and regs_in (what RegPlan.run returned) on the GPU.  Returns (regs_out uint8 [n_u_cap, 80], n_out int32
        [n_reads]): the hits of read r are rows u_off[r] .. u_off[r] + n_out[r]; the rows behind them are unspecified.  Asynchronous."""
        assert u_off.is_cuda and u_off.is_contiguous() and u_off.dtype == torch.int64 and u_off.numel() == self.n_reads + 1
        assert regs_in.is_cuda and regs_in.is_contiguous() and regs_in.numel() * regs_in.element_size() >= self.n_u_cap * REG_DTYPE.itemsize
        regs_out = _out(regs_out, (max(self.n_u_cap, 1), REG_DTYPE.itemsize), torch.uint8, u_off.device, self.n_u_cap * REG_DTYPE.itemsize)
        n_out = _out(n_out, max(self.n_reads, 1), torch.int32, u_off.device, self.n_reads * 4, "dtype")
        st = _stream(stream)
        N.check(self.lib.mm2c_hitplan_run_device(self.handle, C.byref(opt), u_off.data_ptr(), regs_in.data_ptr(), regs_out.data_ptr(), n_out.data_ptr(), st),
                "mm2c_hitplan_run_device")
        return regs_out, n_out[:self.n_reads]

    def run_multi(self, opt, mopt, u_off: torch.Tensor, seg_len: torch.Tensor, regs_in: torch.Tensor, gap_ref: torch.Tensor = None, regs_out: torch.Tensor = None,
                  n_out: torch.Tensor = None, stream=None):
        """mm2c_hitplan_run_device_multi: mm_set_parent, then mm_select_sub_multi (pe.c:6-43) for fragments of mopt.n_segs segments.  mopt: params.hit_multi_opts();
        seg_len int32 [n_frags * n_segs] (qlens, fragment-major); gap_ref int32 [n_frags] (max_chain_gap_ref per fragment) or None for mopt.max_gap_ref everywhere.
        Everything else as run()."""
        assert u_off.is_cuda and u_off.is_contiguous() and u_off.dtype == torch.int64 and u_off.numel() == self.n_reads + 1
        assert regs_in.is_cuda and regs_in.is_contiguous() and regs_in.numel() * regs_in.element_size() >= self.n_u_cap * REG_DTYPE.itemsize
        assert seg_len.is_cuda and seg_len.is_contiguous() and seg_len.dtype == torch.int32 and seg_len.numel() >= self.n_reads * mopt.n_segs
        assert gap_ref is None or (gap_ref.is_cuda and gap_ref.is_contiguous() and gap_ref.dtype == torch.int32 and gap_ref.numel() >= self.n_reads)
        regs_out = _out(regs_out, (max(self.n_u_cap, 1), REG_DTYPE.itemsize), torch.uint8, u_off.device, self.n_u_cap * REG_DTYPE.itemsize)
        n_out = _out(n_out, max(self.n_reads, 1), torch.int32, u_off.device, self.n_reads * 4, "dtype")
        st = _stream(stream)
        N.check(self.lib.mm2c_hitplan_run_device_multi(self.handle, C.byref(opt), C.byref(mopt), u_off.data_ptr(), seg_len.data_ptr(),
                                                       gap_ref.data_ptr() if gap_ref is not None else None, regs_in.data_ptr(), regs_out.data_ptr(), n_out.data_ptr(), st),
                "mm2c_hitplan_run_device_multi")
        return regs_out, n_out[:self.n_reads]

    def check(self):
        """waits for the run; raises if a read's offsets left the capacities; returns the number of hits of all reads"""
        n = C.c_int64(0)
        N.check(self.lib.mm2c_hitplan_check(self.handle, C.byref(n)), "mm2c_hitplan_check")
        return n.value

    def last_ms(self):
        return self._ms("mm2c_hitplan_last_ms")[0]


def select_hits_batch(opt, u_off, regs):
    """mm2c_select_hits_batch_host: host arrays in -> (regs_out REG_DTYPE [u_off[-1] - u_off[0]], n_out int32 [n_reads]); the hits of read r are
    regs_out[u_off[r] - u_off[0] :][:n_out[r]]"""
    lib = N.load()
    uo = _i64(u_off)
    rr = _reg_rows(regs)
    n_reads = uo.size - 1
    if not _fit(n_reads, (uo, rr.shape[0])):
        raise ValueError("offsets do not fit the arrays")
    n_u = int(uo[-1] - uo[0]) if n_reads > 0 else 0
    out = np.zeros(max(n_u, 1), REG_DTYPE)
    n_out = np.zeros(max(n_reads, 1), np.int32)
    N.check(lib.mm2c_select_hits_batch_host(n_reads, C.byref(opt), _np_ptr(uo), _np_ptr(rr), _np_ptr(out), _np_ptr(n_out)), "mm2c_select_hits_batch_host")
    return out[:n_u], n_out[:n_reads]


def select_hits_multi_batch(opt, mopt, u_off, seg_len, regs, gap_ref=None):
    """mm2c_select_hits_multi_batch_host: host arrays in -> (regs_out, n_out) as select_hits_batch, with mm_select_sub_multi in the place of mm_select_sub"""
    lib = N.load()
    uo = _i64(u_off)
    rr = _reg_rows(regs)
    sl = np.ascontiguousarray(seg_len, dtype=np.int32).reshape(-1)
    gr = None if gap_ref is None else np.ascontiguousarray(gap_ref, dtype=np.int32)
    n_reads = uo.size - 1
    if not _fit(n_reads, (uo, rr.shape[0])) or sl.size != n_reads * mopt.n_segs or (gr is not None and gr.size != n_reads):
        raise ValueError("offsets do not fit the arrays")
    n_u = int(uo[-1] - uo[0]) if n_reads > 0 else 0
    out = np.zeros(max(n_u, 1), REG_DTYPE)
    n_out = np.zeros(max(n_reads, 1), np.int32)
    N.check(lib.mm2c_select_hits_multi_batch_host(n_reads, C.byref(opt), C.byref(mopt), _np_ptr(uo), _np_ptr(sl), _np_ptr(gr) if gr is not None else None,
                                                  _np_ptr(rr), _np_ptr(out), _np_ptr(n_out)), "mm2c_select_hits_multi_batch_host")
    return out[:n_u], n_out[:n_reads]


class SegPlan(_Handle):
    """mm2c_segplan_t: the hits of fragments of n_segs segments -> chains, anchors and regions per segment on the GPU (mm_seg_gen hit.c:373-427) for batches of up
    to n_frags fragments, n_u_cap hits and n_b_cap chain anchors; it stands behind HitPlan.run_multi on the same stream, and a HitPlan (pri_ratio 0) and a MapqPlan
    (do_join 0) over n_frags * n_segs "segment reads" stand behind it."""

    _destroy = "mm2c_segplan_destroy"

    def __init__(self, n_frags, n_segs, n_u_cap, n_b_cap):
        self.n_frags, self.n_segs, self.n_u_cap, self.n_b_cap = int(n_frags), int(n_segs), int(n_u_cap), int(n_b_cap)
        self._create("mm2c_segplan_create", self.n_frags, self.n_segs, self.n_u_cap, self.n_b_cap)
        self.n_seg_reads = self.n_frags * self.n_segs
        self.n_su_cap = int(self.lib.mm2c_segplan_seg_chain_cap(self.handle))

    def run(self, u_off: torch.Tensor, regs: torch.Tensor, n_in: torch.Tensor, b_off: torch.Tensor, b: torch.Tensor, seg_len: torch.Tensor, hash: torch.Tensor,
            rep_len: torch.Tensor = None, out: dict = None, stream=None):
        """u_off, regs and n_in as HitPlan.run_multi took and returned them, b_off / b the fragments' chain anchors, seg_len int32 [n_frags * n_segs], hash (32-bit)
        and optionally rep_len int32 per fragment, all on the GPU.  Returns a dict of GPU tensors (out: one from an earlier run, to write into again): su_off /
        sb_off int64 [n_seg_reads + 1], su int64 [n_su_cap], sb int64 [n_b_cap, 2], seg_regs uint8 [n_su_cap, 80], seg_hash int32 [n_seg_reads], seg_rep_len int32
        [n_seg_reads] or None.  Asynchronous."""
        for t in (u_off, regs, n_in, b_off, b, seg_len, hash) + ((rep_len,) if rep_len is not None else ()):
            assert t.is_cuda and t.is_contiguous()
        assert u_off.dtype == torch.int64 and b_off.dtype == torch.int64 and u_off.numel() == self.n_frags + 1 and b_off.numel() == self.n_frags + 1
        assert regs.numel() * regs.element_size() >= self.n_u_cap * REG_DTYPE.itemsize and b.element_size() == 8 and b.numel() >= 2 * self.n_b_cap
        assert n_in.dtype == torch.int32 and n_in.numel() >= self.n_frags and seg_len.dtype == torch.int32 and seg_len.numel() >= self.n_seg_reads
        assert hash.element_size() == 4 and hash.numel() >= self.n_frags and (rep_len is None or (rep_len.dtype == torch.int32 and rep_len.numel() >= self.n_frags))
        dev, ns = u_off.device, max(self.n_seg_reads, 1)
        if out is None:
            out = dict(su_off=torch.empty(ns + 1, dtype=torch.int64, device=dev), sb_off=torch.empty(ns + 1, dtype=torch.int64, device=dev),
                       su=torch.empty(max(self.n_su_cap, 1), dtype=torch.int64, device=dev), sb=torch.empty((max(self.n_b_cap, 1), 2), dtype=torch.int64, device=dev),
                       seg_regs=torch.empty((max(self.n_su_cap, 1), REG_DTYPE.itemsize), dtype=torch.uint8, device=dev),
                       seg_hash=torch.empty(ns, dtype=torch.int32, device=dev), seg_rep_len=None)
        if rep_len is not None and out.get("seg_rep_len") is None:
            out["seg_rep_len"] = torch.empty(ns, dtype=torch.int32, device=dev)
        assert out["su_off"].numel() >= self.n_seg_reads + 1 and out["sb_off"].numel() >= self.n_seg_reads + 1 and out["su"].numel() >= self.n_su_cap
        assert out["sb"].numel() >= 2 * self.n_b_cap and out["seg_regs"].numel() >= self.n_su_cap * REG_DTYPE.itemsize and out["seg_hash"].numel() >= self.n_seg_reads
        for t in out.values():
            assert t is None or (t.is_cuda and t.is_contiguous())
        st = _stream(stream)
        N.check(self.lib.mm2c_segplan_run_device(self.handle, u_off.data_ptr(), regs.data_ptr(), n_in.data_ptr(), b_off.data_ptr(), b.data_ptr(), seg_len.data_ptr(),
                                                 hash.data_ptr(), rep_len.data_ptr() if rep_len is not None else None, out["su_off"].data_ptr(), out["su"].data_ptr(),
                                                 out["sb_off"].data_ptr(), out["sb"].data_ptr(), out["seg_regs"].data_ptr(), out["seg_hash"].data_ptr(),
                                                 out["seg_rep_len"].data_ptr() if rep_len is not None else None, st), "mm2c_segplan_run_device")
        return out

    def counts(self):
        """waits for the run -> (return code, fragments refused, segment chains, segment anchors) without raising"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = self.lib.mm2c_segplan_check(self.handle, C.byref(a), C.byref(b), C.byref(c))
        return rc, a.value, b.value, c.value

    def check(self):
        """waits for the run; raises (code -2) if a fragment was refused; returns (segment chains, segment anchors) of the batch"""
        rc, _, nu, na = self.counts()
        N.check(rc, "mm2c_segplan_check")
        return nu, na

    def last_ms(self):
        return self._ms("mm2c_segplan_last_ms")[0]

    def last_kernel_ms(self):
        """(seg_count, the two scans, seg_scatter, the region kernels, seg_mark) of the last run"""
        return self._ms("mm2c_segplan_last_kernel_ms", 5)


def seg_gen_batch(n_segs, u_off, regs, n_in, b_off, b, seg_len, hash, rep_len=None):
    """mm2c_seg_gen_batch_host: host arrays in -> dict(su_off, su uint64, sb_off, sb uint64 [., 2], seg_regs REG_DTYPE, seg_hash uint32, seg_rep_len int32 or None);
    segment read f * n_segs + s owns su[su_off[k] : su_off[k+1]] (and seg_regs likewise) and sb[sb_off[k] : sb_off[k+1]]"""
    lib = N.load()
    uo = _i64(u_off); bo = _i64(b_off)
    rr = _reg_rows(regs)
    bb = _anchor_rows(b)
    ni = np.ascontiguousarray(n_in, dtype=np.int32); sl = np.ascontiguousarray(seg_len, dtype=np.int32).reshape(-1); h = np.ascontiguousarray(hash, dtype=np.uint32)
    rl = None if rep_len is None else np.ascontiguousarray(rep_len, dtype=np.int32)
    n_frags, n_segs = uo.size - 1, int(n_segs)
    if bo.size != uo.size or ni.size != n_frags or h.size != n_frags or sl.size != n_frags * n_segs or (rl is not None and rl.size != n_frags) or \
            not _fit(n_frags, (uo, rr.shape[0]), (bo, bb.shape[0])):
        raise ValueError("offsets do not fit the arrays")
    n_u = int(uo[-1] - uo[0]) if n_frags > 0 else 0
    n_b = int(bo[-1] - bo[0]) if n_frags > 0 else 0
    ns, n_su = max(n_frags * n_segs, 0), min(n_segs * n_u, n_b)
    su_off = np.zeros(ns + 1, np.int64); sb_off = np.zeros(ns + 1, np.int64)
    su = np.zeros(max(n_su, 1), np.uint64); sb = np.zeros((max(n_b, 1), 2), np.uint64); seg_regs = np.zeros(max(n_su, 1), REG_DTYPE)
    seg_hash = np.zeros(max(ns, 1), np.uint32); seg_rl = np.zeros(max(ns, 1), np.int32) if rl is not None else None
    N.check(lib.mm2c_seg_gen_batch_host(n_frags, n_segs, _np_ptr(uo), _np_ptr(rr), _np_ptr(ni), _np_ptr(bo), _np_ptr(bb), _np_ptr(sl), _np_ptr(h),
                                        _np_ptr(rl) if rl is not None else None, _np_ptr(su_off), _np_ptr(su), _np_ptr(sb_off), _np_ptr(sb), _np_ptr(seg_regs),
                                        _np_ptr(seg_hash), _np_ptr(seg_rl) if rl is not None else None), "mm2c_seg_gen_batch_host")
    tu, ta = int(su_off[-1]), int(sb_off[-1])
    return dict(su_off=su_off, su=su[:tu], sb_off=sb_off, sb=sb[:ta], seg_regs=seg_regs[:tu], seg_hash=seg_hash[:ns], seg_rep_len=(seg_rl[:ns] if rl is not None else None))


KSW_TASK_DTYPE = np.dtype([("q_off", "<i8"), ("t_off", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"), ("w", "<i4"), ("zdrop", "<i4"), ("end_bonus", "<i4"), ("flag", "<i4")])
KSW_RES_DTYPE = np.dtype([("max", "<u4"), ("zdropped", "<i4"), ("max_q", "<i4"), ("max_t", "<i4"), ("mqe", "<i4"), ("mqe_t", "<i4"), ("mte", "<i4"), ("mte_q", "<i4"),
                          ("score", "<i4"), ("n_cigar", "<i4"), ("reach_end", "<i4"), ("status", "<i4")])
KSW_REFUSED, KSW_TOO_BIG, KSW_CIGAR_CUT = 1, 2, 3


def _ksw_score_bytes(score):
    """(mat int8 [25], q, e, q2, e2) or the dict params.ksw_scores() makes -> the 29 bytes of mm2c_ksw_score_t"""
    if isinstance(score, dict):
        score = (score["mat"], score["q"], score["e"], score["q2"], score["e2"])
    mat, q, e, q2, e2 = score
    mat = np.asarray(mat, dtype=np.int8).reshape(-1)
    if mat.size != 25:
        raise ValueError("mat must hold 5 x 5 scores")
    return np.ascontiguousarray(np.concatenate([mat, np.array([q, e, q2, e2], np.int8)]))


def ksw_task_scratch(qlen, tlen, w, flag):
    """bytes of a scratch slot a task takes (mm2c_ksw_task_scratch)"""
    return int(N.load().mm2c_ksw_task_scratch(int(qlen), int(tlen), int(w), int(flag)))


class KswPlan(_Handle):
    """mm2c_kswplan_t: ksw_extd2_sse (ksw2_extd2_sse.c) on the GPU for batches of up to n_tasks_cap independent tasks over a pool of seq_cap bases and cigar_cap
    CIGAR words, one wave per scratch slot.  Either scratch_bytes (the default cut into slots of 4 MiB, for tasks up to that size) or n_slots and slot_bytes (the
    caller's cut: a task runs in a slot of at least ksw_task_scratch(...) bytes).  Byte for byte the reference's ksw_extz_t and CIGAR."""

    _destroy = "mm2c_kswplan_destroy"

    def __init__(self, n_tasks_cap, seq_cap, cigar_cap, scratch_bytes=None, n_slots=None, slot_bytes=None):
        self.n_tasks_cap, self.seq_cap, self.cigar_cap = int(n_tasks_cap), int(seq_cap), int(cigar_cap)
        if (scratch_bytes is None) == (n_slots is None or slot_bytes is None):
            raise ValueError("give scratch_bytes, or n_slots and slot_bytes")
        if scratch_bytes is not None:
            self._create("mm2c_kswplan_create", self.n_tasks_cap, self.seq_cap, self.cigar_cap, int(scratch_bytes))
        else:
            self._create("mm2c_kswplan_create_slots", self.n_tasks_cap, self.seq_cap, self.cigar_cap, int(n_slots), int(slot_bytes), what="mm2c_kswplan_create")
        self.slot_bytes, self.n_slots = int(self.lib.mm2c_kswplan_slot_bytes(self.handle)), int(self.lib.mm2c_kswplan_n_slots(self.handle))

    def run(self, score, n_tasks, tasks: torch.Tensor, seq: torch.Tensor, cig_off: torch.Tensor, res: torch.Tensor = None, cigar: torch.Tensor = None, stream=None):
        """tasks: the bytes of KSW_TASK_DTYPE [n_tasks], seq uint8 [>= seq_cap], cig_off int64 [n_tasks + 1], all on the GPU.  Returns (res, cigar): uint8
        [n_tasks, 48] (KSW_RES_DTYPE) and int32 [cigar_cap] GPU tensors (given ones are written into).  Asynchronous."""
        n_tasks = int(n_tasks)
        for t in (tasks, seq, cig_off):
            assert t.is_cuda and t.is_contiguous()
        assert tasks.numel() * tasks.element_size() >= n_tasks * KSW_TASK_DTYPE.itemsize and seq.element_size() == 1 and seq.numel() >= self.seq_cap
        assert cig_off.dtype == torch.int64 and cig_off.numel() >= n_tasks + 1 and 0 <= n_tasks <= self.n_tasks_cap
        res = _out(res, (max(n_tasks, 1), KSW_RES_DTYPE.itemsize), torch.uint8, tasks.device, n_tasks * KSW_RES_DTYPE.itemsize)
        cigar = _out(cigar, max(self.cigar_cap, 1), torch.int32, tasks.device, self.cigar_cap * 4, "width")
        sc = _ksw_score_bytes(score)
        st = _stream(stream)
        N.check(self.lib.mm2c_kswplan_run_device(self.handle, _np_ptr(sc), n_tasks, tasks.data_ptr(), seq.data_ptr(), cig_off.data_ptr(), res.data_ptr(),
                                                 cigar.data_ptr(), st), "mm2c_kswplan_run_device")
        return res, cigar

    def counts(self):
        """waits for the run -> (return code, tasks refused, tasks too big or CIGARs cut) without raising"""
        a, b = C.c_int64(0), C.c_int64(0)
        rc = self.lib.mm2c_kswplan_check(self.handle, C.byref(a), C.byref(b))
        return rc, a.value, b.value

    def check(self):
        """waits for the run; raises (code -2) if a task was refused, (code -3) if one did not fit a slot or a CIGAR was cut"""
        N.check(self.counts()[0], "mm2c_kswplan_check")

    def last_ms(self):
        return self._ms("mm2c_kswplan_last_ms")[0]

    def last_kernel_ms(self):
        """(ksw_rows,) of the last run: rows and backtrack are one kernel"""
        return self._ms("mm2c_kswplan_last_kernel_ms")


def ksw_extd2_batch(score, tasks, seq, cig_off, scratch_bytes=0, res=None, cigar=None):
    """mm2c_ksw_extd2_batch_host: host arrays in (tasks KSW_TASK_DTYPE, seq uint8 codes 0..4, cig_off int64 [n + 1] from 0) -> (res KSW_RES_DTYPE [n], cigar uint32
    [cig_off[n]]); task i's CIGAR is cigar[cig_off[i] : cig_off[i] + min(n_cigar, its slot)].  Raises before any device work for a bad task; with code -3 (a task
    beyond the scratch, a CIGAR cut) the arrays given as res / cigar are complete all the same."""
    lib = N.load()
    tk = np.ascontiguousarray(tasks, dtype=KSW_TASK_DTYPE); sq = np.ascontiguousarray(seq, dtype=np.uint8); co = np.ascontiguousarray(cig_off, dtype=np.int64)
    n = tk.size
    if co.size != n + 1:
        raise ValueError("cig_off must hold n_tasks + 1 offsets")
    res = np.zeros(max(n, 1), KSW_RES_DTYPE) if res is None else res
    cigar = np.zeros(max(int(co[-1]), 1), np.uint32) if cigar is None else cigar
    assert res.dtype == KSW_RES_DTYPE and res.size >= n and cigar.dtype == np.uint32 and cigar.size >= int(co[-1]) and res.flags.c_contiguous and cigar.flags.c_contiguous
    sc = _ksw_score_bytes(score)
    N.check(lib.mm2c_ksw_extd2_batch_host(_np_ptr(sc), n, _np_ptr(tk), sq.size, _np_ptr(sq), _np_ptr(co), _np_ptr(res), _np_ptr(cigar), int(scratch_bytes)),
            "mm2c_ksw_extd2_batch_host")
    return res[:n], cigar[:int(co[-1])]


EXTRA_TASK_DTYPE = np.dtype([("q_off", "<i8"), ("t_off", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"), ("n_cigar", "<i4"), ("rev", "<i4")])
EXTRA_RES_DTYPE = np.dtype([("n_cigar", "<i4"), ("qshift", "<i4"), ("tshift", "<i4"), ("blen", "<i4"), ("mlen", "<i4"), ("n_ambi", "<i4"), ("dp_max", "<i4"), ("status", "<i4")])
ZDROP_OPT_DTYPE = np.dtype([("zdrop", "<i4"), ("zdrop_inv", "<i4"), ("max_gap", "<i4"), ("no_inv", "<i4")])
ZDROP_RES_DTYPE = np.dtype([("max_zdrop", "<i4"), ("t0", "<i4"), ("t1", "<i4"), ("q0", "<i4"), ("q1", "<i4"), ("code", "<i4"), ("inv_cand", "<i4"), ("status", "<i4")])
EXTRA_REFUSED, EXTRA_TOO_BIG, EXTRA_CIGAR_CUT = 1, 2, 3
EXTRA_LDS_WORDS = 2048


def _zdrop_opt_bytes(opt):
    """(zdrop, zdrop_inv, max_gap, no_inv) or the dict params.zdrop_opts() makes -> the 16 bytes of mm2c_zdrop_opt_t"""
    if isinstance(opt, dict):
        opt = (opt["zdrop"], opt["zdrop_inv"], opt["max_gap"], opt["no_inv"])
    return np.ascontiguousarray(np.array([int(x) for x in opt], np.int32))


class ExtraPlan(_Handle):
    """mm2c_extraplan_t: mm_update_extra (align.c:240-286) for batches of regions and mm_test_zdrop (align.c:47-89) on a KswPlan's device outputs, one wave per item,
    byte for byte the reference.  n_cap items, a pool of seq_cap bases, cig_in_cap input CIGAR words (for z-drop runs: the ksw plan's cigar_cap), cig_out_cap output
    words; CIGARs beyond EXTRA_LDS_WORDS words need one of n_slots scratch slots of slot_words words."""

    _destroy = "mm2c_extraplan_destroy"

    def __init__(self, n_cap, seq_cap, cig_in_cap, cig_out_cap=0, n_slots=0, slot_words=0):
        self.n_cap, self.seq_cap, self.cig_in_cap, self.cig_out_cap = int(n_cap), int(seq_cap), int(cig_in_cap), int(cig_out_cap)
        self._create("mm2c_extraplan_create", self.n_cap, self.seq_cap, self.cig_in_cap, self.cig_out_cap, int(n_slots), int(slot_words))

    def update(self, score, is_eqx, n_regs, tasks: torch.Tensor, seq: torch.Tensor, in_off: torch.Tensor, cig_in: torch.Tensor, out_off: torch.Tensor,
               res: torch.Tensor = None, cig_out: torch.Tensor = None, stream=None):
        """tasks: the bytes of EXTRA_TASK_DTYPE [n_regs], seq uint8 [>= seq_cap], in_off int64 [n_regs], cig_in int32 [>= cig_in_cap], out_off int64 [n_regs + 1], all on
        the GPU.  Returns (res, cig_out): uint8 [n_regs, 32] (EXTRA_RES_DTYPE) and int32 [cig_out_cap] GPU tensors (given ones are written into).  Asynchronous."""
        n = int(n_regs)
        for t in (tasks, seq, in_off, cig_in, out_off):
            assert t.is_cuda and t.is_contiguous()
        assert tasks.numel() * tasks.element_size() >= n * EXTRA_TASK_DTYPE.itemsize and seq.element_size() == 1 and seq.numel() >= self.seq_cap and 0 <= n <= self.n_cap
        assert in_off.dtype == torch.int64 and in_off.numel() >= n and out_off.dtype == torch.int64 and out_off.numel() >= n + 1
        assert cig_in.element_size() == 4 and cig_in.numel() >= self.cig_in_cap
        res = _out(res, (max(n, 1), EXTRA_RES_DTYPE.itemsize), torch.uint8, tasks.device, n * EXTRA_RES_DTYPE.itemsize)
        cig_out = _out(cig_out, max(self.cig_out_cap, 1), torch.int32, tasks.device, self.cig_out_cap * 4, "width")
        sc = _ksw_score_bytes(score)
        st = _stream(stream)
        N.check(self.lib.mm2c_extraplan_run_device(self.handle, _np_ptr(sc), int(bool(is_eqx)), n, tasks.data_ptr(), seq.data_ptr(), in_off.data_ptr(), cig_in.data_ptr(),
                                                   out_off.data_ptr(), res.data_ptr(), cig_out.data_ptr(), st), "mm2c_extraplan_run_device")
        return res, cig_out

    def zdrop(self, score, opt, n_tasks, tasks: torch.Tensor, seq: torch.Tensor, cig_off: torch.Tensor, kres: torch.Tensor, cigar: torch.Tensor, zres: torch.Tensor = None,
              stream=None):
        """the arrays of KswPlan.run as they lie on the GPU (tasks, seq, cig_off in; res, cigar out) -> zres uint8 [n_tasks, 32] (ZDROP_RES_DTYPE).  Asynchronous."""
        n = int(n_tasks)
        for t in (tasks, seq, cig_off, kres, cigar):
            assert t.is_cuda and t.is_contiguous()
        assert tasks.numel() * tasks.element_size() >= n * KSW_TASK_DTYPE.itemsize and seq.element_size() == 1 and seq.numel() >= self.seq_cap and 0 <= n <= self.n_cap
        assert cig_off.dtype == torch.int64 and cig_off.numel() >= n + 1 and kres.numel() * kres.element_size() >= n * KSW_RES_DTYPE.itemsize
        assert cigar.element_size() == 4 and cigar.numel() >= self.cig_in_cap
        zres = _out(zres, (max(n, 1), ZDROP_RES_DTYPE.itemsize), torch.uint8, tasks.device, n * ZDROP_RES_DTYPE.itemsize)
        sc, zo = _ksw_score_bytes(score), _zdrop_opt_bytes(opt)
        st = _stream(stream)
        N.check(self.lib.mm2c_extraplan_zdrop_run_device(self.handle, _np_ptr(sc), _np_ptr(zo), n, tasks.data_ptr(), seq.data_ptr(), cig_off.data_ptr(), kres.data_ptr(),
                                                         cigar.data_ptr(), zres.data_ptr(), st), "mm2c_extraplan_zdrop_run_device")
        return zres

    def counts(self):
        """waits for the last run -> (return code, items refused, CIGARs too big or cut) without raising"""
        a, b = C.c_int64(0), C.c_int64(0)
        rc = self.lib.mm2c_extraplan_check(self.handle, C.byref(a), C.byref(b))
        return rc, a.value, b.value

    def check(self):
        """waits for the last run; raises (code -2) if an item was refused, (code -3) if a CIGAR fits neither LDS nor a slot or an output was cut"""
        N.check(self.counts()[0], "mm2c_extraplan_check")

    def last_ms(self):
        return self._ms("mm2c_extraplan_last_ms")[0]

    def last_kernel_ms(self):
        """(extra_update, extra_zdrop) of their last runs; 0 for one that has not run"""
        return self._ms("mm2c_extraplan_last_kernel_ms", 2)


def update_extra_batch(score, is_eqx, tasks, seq, in_off, cig_in, out_off, res=None, cig_out=None):
    """mm2c_update_extra_batch_host: host arrays in (tasks EXTRA_TASK_DTYPE, seq uint8 codes 0..4, in_off int64 [n], cig_in uint32, out_off int64 [n + 1] from 0) ->
    (res EXTRA_RES_DTYPE [n], cig_out uint32 [out_off[n]]); region i's CIGAR is cig_out[out_off[i] : out_off[i] + min(n_cigar, its slot)].  With code -3 (a CIGAR cut)
    the arrays given as res / cig_out are complete all the same."""
    lib = N.load()
    tk = np.ascontiguousarray(tasks, dtype=EXTRA_TASK_DTYPE); sq = np.ascontiguousarray(seq, dtype=np.uint8)
    io = np.ascontiguousarray(in_off, dtype=np.int64); ci = np.ascontiguousarray(cig_in, dtype=np.uint32); oo = np.ascontiguousarray(out_off, dtype=np.int64)
    n = tk.size
    if oo.size != n + 1 or io.size != n:
        raise ValueError("in_off must hold n_regs and out_off n_regs + 1 offsets")
    res = np.zeros(max(n, 1), EXTRA_RES_DTYPE) if res is None else res
    cig_out = np.zeros(max(int(oo[-1]), 1), np.uint32) if cig_out is None else cig_out
    assert res.dtype == EXTRA_RES_DTYPE and res.size >= n and cig_out.dtype == np.uint32 and cig_out.size >= int(oo[-1]) and res.flags.c_contiguous and cig_out.flags.c_contiguous
    sc = _ksw_score_bytes(score)
    N.check(lib.mm2c_update_extra_batch_host(_np_ptr(sc), int(bool(is_eqx)), n, _np_ptr(tk), sq.size, _np_ptr(sq), _np_ptr(io), ci.size, _np_ptr(ci), _np_ptr(oo), _np_ptr(res),
                                             _np_ptr(cig_out)), "mm2c_update_extra_batch_host")
    return res[:n], cig_out[:int(oo[-1])]


def test_zdrop_batch(score, opt, tasks, seq, cig_off, kres, cigar, zres=None):
    """mm2c_test_zdrop_batch_host: the host arrays of ksw_extd2_batch (tasks, seq, cig_off in; res, cigar out) -> zres ZDROP_RES_DTYPE [n]"""
    lib = N.load()
    tk = np.ascontiguousarray(tasks, dtype=KSW_TASK_DTYPE); sq = np.ascontiguousarray(seq, dtype=np.uint8); co = np.ascontiguousarray(cig_off, dtype=np.int64)
    kr = np.ascontiguousarray(kres, dtype=KSW_RES_DTYPE); cg = np.ascontiguousarray(cigar, dtype=np.uint32)
    n = tk.size
    if co.size != n + 1 or kr.size < n:
        raise ValueError("cig_off must hold n_tasks + 1 offsets and kres n_tasks results")
    zres = np.zeros(max(n, 1), ZDROP_RES_DTYPE) if zres is None else zres
    assert zres.dtype == ZDROP_RES_DTYPE and zres.size >= n and zres.flags.c_contiguous and cg.size >= int(co[-1])
    sc, zo = _ksw_score_bytes(score), _zdrop_opt_bytes(opt)
    N.check(lib.mm2c_test_zdrop_batch_host(_np_ptr(sc), _np_ptr(zo), n, _np_ptr(tk), sq.size, _np_ptr(sq), _np_ptr(co), _np_ptr(kr), _np_ptr(cg), _np_ptr(zres)),
            "mm2c_test_zdrop_batch_host")
    return zres[:n]


test_zdrop_batch.__test__ = False      # a library function, not a test


ALN_OPT_DTYPE = np.dtype([(n, "<i4") for n in ("a", "b", "q", "e", "e2", "bw", "bw_ext", "min_chain_score", "max_gap", "min_cnt", "min_ksw_len", "end_bonus", "zdrop", "zdrop_inv")] +
                         [("max_sw_mat", "<i8"), ("flag", "<i4"), ("idx_flag", "<i4"), ("k", "<i4"), ("reserved", "<i4")])
ALN_REG_DTYPE = np.dtype([(n, "<i4") for n in ("as1", "cnt1", "rs", "qs", "re", "qe", "rs0", "qs0", "re0", "qe0", "n_items", "n_tasks", "status", "rev")] +
                         [(n, "<i8") for n in ("item0", "task0", "cig0", "q_off", "t_off", "left_off")])
ALN_ITEM_DTYPE = np.dtype([(n, "<i4") for n in ("reg", "kind", "anchor", "rs", "re", "qs", "qe", "task", "score", "reserved")])
ALN_REFUSED, ALN_TOO_BIG, ALN_OVER_CAP = 1, 2, 3
ALN_LDS_GAPS = 2048
ALN_LEFT, ALN_GAP, ALN_RIGHT, ALN_UNGAPPED, ALN_OVER = 0, 1, 2, 3, 16


def _aln_opt_bytes(opt):
    """the dict params.aln_opts() makes (or an ALN_OPT_DTYPE record) -> the 80 bytes of mm2c_aln_opt_t"""
    if isinstance(opt, dict):
        o = np.zeros(1, ALN_OPT_DTYPE)
        for k, v in opt.items():
            o[k] = int(v)
        return o
    return np.ascontiguousarray(np.asarray(opt, dtype=ALN_OPT_DTYPE).reshape(1))


class RefSeq(_Handle):
    """mm2c_refseq_t: the packed reference mi->S (uint32 words, 8 bases each) with offset (uint64) and len (uint32) of every mi->seq[], resident on the GPU"""

    _destroy = "mm2c_refseq_destroy"

    def __init__(self, offset, length, S):
        off = np.ascontiguousarray(offset, dtype=np.uint64); ln = np.ascontiguousarray(length, dtype=np.uint32); S = np.ascontiguousarray(S, dtype=np.uint32)
        if off.size != ln.size:
            raise ValueError("offset and len must have one entry per sequence")
        self.n_seq, self.n_words = int(off.size), int(S.size)
        self._create("mm2c_refseq_create", self.n_seq, _np_ptr(off), _np_ptr(ln), _np_ptr(S), self.n_words, code=-2)


class AlnPlan(_Handle):
    """mm2c_alnplan_t: final regions -> the ksw tasks mm_align1 (align.c:565-771) issues when no task drops, with their items and ONE sequence pool that is the d_seq
    of a KswPlan and of an ExtraPlan, byte for byte the reference.  Capacities: regions, items, tasks, pool bytes, anchors, read bases."""

    _destroy = "mm2c_alnplan_destroy"

    def __init__(self, n_regs_cap, n_items_cap, n_tasks_cap, pool_cap, n_b_cap, reads_cap, cig_shift=0, n_slots=0, slot_words=0):
        self.n_regs_cap, self.n_items_cap, self.n_tasks_cap, self.pool_cap = int(n_regs_cap), int(n_items_cap), int(n_tasks_cap), int(pool_cap)
        self.n_b_cap, self.reads_cap, self.cig_shift = int(n_b_cap), int(reads_cap), int(cig_shift)
        self._create("mm2c_alnplan_create", self.n_regs_cap, self.n_items_cap, self.n_tasks_cap, self.pool_cap, self.n_b_cap, self.reads_cap, self.cig_shift, int(n_slots),
                     int(slot_words), code=-2)

    def run(self, opt, ref: RefSeq, n_reads, n_regs, u_off: torch.Tensor, regs: torch.Tensor, b_off: torch.Tensor, b: torch.Tensor, read_off: torch.Tensor, reads: torch.Tensor,
            n_b: torch.Tensor = None, aln_regs: torch.Tensor = None, items: torch.Tensor = None, tasks: torch.Tensor = None, cig_off: torch.Tensor = None,
            pool: torch.Tensor = None, stream=None):
        """u_off, b_off, read_off int64 [n_reads + 1], regs the bytes of REG_DTYPE [n_regs], b the anchors (16 bytes each, in/out: the seed flags), reads uint8 forward
        codes, n_b int64 [n_reads] or None, all on the GPU.  Returns (aln_regs uint8 [n_regs, 104], items uint8 [n_items_cap, 40], tasks uint8 [n_tasks_cap, 40],
        cig_off int64 [n_tasks_cap + 1], pool uint8 [pool_cap]) GPU tensors (given ones are written into).  Asynchronous."""
        n_reads, n = int(n_reads), int(n_regs)
        for t in (u_off, regs, b_off, b, read_off, reads):
            assert t.is_cuda and t.is_contiguous()
        assert all(t.dtype == torch.int64 and t.numel() >= n_reads + 1 for t in (u_off, b_off, read_off)) and 0 <= n <= self.n_regs_cap
        assert regs.numel() * regs.element_size() >= n * REG_DTYPE.itemsize and b.numel() * b.element_size() >= 16 * self.n_b_cap and reads.element_size() == 1 and reads.numel() >= self.reads_cap
        dev = regs.device
        aln_regs = _out(aln_regs, (max(n, 1), ALN_REG_DTYPE.itemsize), torch.uint8, dev, n * ALN_REG_DTYPE.itemsize)
        items = _out(items, (max(self.n_items_cap, 1), ALN_ITEM_DTYPE.itemsize), torch.uint8, dev, self.n_items_cap * ALN_ITEM_DTYPE.itemsize)
        tasks = _out(tasks, (max(self.n_tasks_cap, 1), KSW_TASK_DTYPE.itemsize), torch.uint8, dev, self.n_tasks_cap * KSW_TASK_DTYPE.itemsize)
        cig_off = _out(cig_off, self.n_tasks_cap + 1, torch.int64, dev, (self.n_tasks_cap + 1) * 8, "dtype")
        pool = _out(pool, max(self.pool_cap, 16), torch.uint8, dev, self.pool_cap, "width")
        assert n_b is None or (n_b.is_cuda and n_b.dtype == torch.int64 and n_b.numel() >= n_reads)
        o = _aln_opt_bytes(opt)
        st = _stream(stream)
        N.check(self.lib.mm2c_alnplan_run_device(self.handle, _np_ptr(o), ref.handle, n_reads, n, u_off.data_ptr(), regs.data_ptr(), b_off.data_ptr(),
                                                 n_b.data_ptr() if n_b is not None else None, b.data_ptr(), read_off.data_ptr(), reads.data_ptr(), aln_regs.data_ptr(),
                                                 items.data_ptr(), tasks.data_ptr(), cig_off.data_ptr(), pool.data_ptr(), st), "mm2c_alnplan_run_device")
        return aln_regs, items, tasks, cig_off, pool

    def counts(self):
        """waits for the last run -> (return code, regions refused, regions too big or beyond a capacity, (items, tasks, CIGAR words, pool bytes) the batch takes)"""
        a, b, t = C.c_int64(0), C.c_int64(0), (C.c_int64 * 4)()
        rc = self.lib.mm2c_alnplan_check(self.handle, C.byref(a), C.byref(b), t)
        return rc, a.value, b.value, tuple(int(x) for x in t)

    def check(self):
        """waits for the last run; raises (code -2) if a region was refused, (code -3) if one was too big or left a capacity; returns the totals"""
        rc, _, _, tot = self.counts()
        N.check(rc, "mm2c_alnplan_check")
        return tot

    def last_kernel_ms(self):
        """(aln_plan with aln_scan, aln_emit, aln_gather) of the last run"""
        ms = (C.c_float * 3)()
        N.check(self.lib.mm2c_alnplan_last_kernel_ms(self.handle, ms), "mm2c_alnplan_last_kernel_ms")
        return tuple(float(x) for x in ms)

    def last_ms(self):
        return sum(self.last_kernel_ms())


def align_tasks_batch(opt, ref_offset, ref_len, S, u_off, regs, b_off, b, read_off, reads, n_items_cap, n_tasks_cap, pool_cap, cig_shift=0, fill=None):
    """mm2c_align_tasks_batch_host: host arrays in (ref_offset uint64, ref_len uint32, S uint32; u_off, b_off, read_off int64 [n_reads + 1] from 0; regs REG_DTYPE; b uint64
    [n, 2] anchors; reads uint8 forward codes 0..4) -> dict(aln_regs, items, tasks, cig_off, pool, b, totals, rc): b is a copy with the seed flags, totals what the batch
    takes, rc the return code (0, or -3 when something was too big: the arrays are complete up to the capacities all the same).  Raises for any other failure.
    fill: a byte the output arrays are filled with beforehand (tests)."""
    lib = N.load()
    off = np.ascontiguousarray(ref_offset, dtype=np.uint64); ln = np.ascontiguousarray(ref_len, dtype=np.uint32); S = np.ascontiguousarray(S, dtype=np.uint32)
    uo = np.ascontiguousarray(u_off, dtype=np.int64); bo = np.ascontiguousarray(b_off, dtype=np.int64); ro = np.ascontiguousarray(read_off, dtype=np.int64)
    rg = np.ascontiguousarray(regs, dtype=REG_DTYPE); bb = np.array(b, dtype=np.uint64, order="C", copy=True).reshape(-1, 2); rd = np.ascontiguousarray(reads, dtype=np.uint8)
    n_reads = uo.size - 1
    if bo.size != n_reads + 1 or ro.size != n_reads + 1 or off.size != ln.size:
        raise ValueError("u_off, b_off and read_off must hold n_reads + 1 offsets")
    n_regs = int(uo[-1]) if n_reads > 0 else 0
    if rg.size < n_regs or bb.shape[0] < int(bo[-1]) or rd.size < int(ro[-1]):
        raise ValueError("an array is shorter than its offsets say")
    f = 0 if fill is None else int(fill)
    aln_regs = np.full(max(n_regs, 1) * ALN_REG_DTYPE.itemsize, f, np.uint8).view(ALN_REG_DTYPE)
    items = np.full(max(int(n_items_cap), 1) * ALN_ITEM_DTYPE.itemsize, f, np.uint8).view(ALN_ITEM_DTYPE)
    tasks = np.full(max(int(n_tasks_cap), 1) * KSW_TASK_DTYPE.itemsize, f, np.uint8).view(KSW_TASK_DTYPE)
    cig_off = np.full((int(n_tasks_cap) + 1) * 8, f, np.uint8).view(np.int64)
    pool = np.full(max(int(pool_cap), 1), f, np.uint8)
    tot = (C.c_int64 * 4)()
    o = _aln_opt_bytes(opt)
    rc = lib.mm2c_align_tasks_batch_host(_np_ptr(o), off.size, _np_ptr(off), _np_ptr(ln), _np_ptr(S), S.size, n_reads, _np_ptr(uo), _np_ptr(rg), _np_ptr(bo), _np_ptr(bb), _np_ptr(ro),
                                         _np_ptr(rd), int(cig_shift), _np_ptr(aln_regs), int(n_items_cap), _np_ptr(items), int(n_tasks_cap), _np_ptr(tasks), _np_ptr(cig_off),
                                         int(pool_cap), _np_ptr(pool), tot)
    if rc not in (0, -3):
        N.check(rc, "mm2c_align_tasks_batch_host")
    return dict(aln_regs=aln_regs[:n_regs], items=items[:int(n_items_cap)], tasks=tasks[:int(n_tasks_cap)], cig_off=cig_off, pool=pool[:int(pool_cap)], b=bb,
                totals=tuple(int(x) for x in tot), rc=rc)


CIG_OPT_DTYPE = np.dtype([(n, "<i4") for n in ("zdrop", "zdrop_inv", "bw_ext", "min_cnt", "flag", "cig_shift")])
CIG_REG_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_used", "dropped", "drop_item", "zdrop_code", "split_n", "split_inv", "has_p", "n_cigar", "dp_score", "rs1", "re1",
                                               "qs1", "qe1", "r_qs", "r_qe")] + [("cig0", "<i8")])
CIG_REFUSED, CIG_INCOMPLETE, CIG_OVER_CAP = 1, 2, 3
CIG_PIECE = 256
CIG_NO_ROOM = -2
CIG_LOST = -3


def _cig_opt_bytes(opt):
    """a dict with the fields of CIG_OPT_DTYPE (those an aln_opts() dict has are taken from it; cig_shift defaults to 0) or a record -> the 24 bytes of mm2c_cig_opt_t"""
    if isinstance(opt, dict):
        o = np.zeros(1, CIG_OPT_DTYPE)
        for k in CIG_OPT_DTYPE.names:
            o[k] = int(opt.get(k, 0))
        return o
    return np.ascontiguousarray(np.asarray(opt, dtype=CIG_OPT_DTYPE).reshape(1))


class CigPlan(_Handle):
    """mm2c_cigplan_t: the rest of mm_align1 (align.c:698-705, 736-764, 772-783) on the arrays an AlnPlan, a KswPlan and ExtraPlan.zdrop leave on the GPU: second() lists
    the second passes, join() cuts each region behind its first drop, appends and merges the CIGARs, sums dp_score, takes rs1 .. qe1 and decides the split; its extra
    tasks, in_off and CIGAR buffer go into ExtraPlan.update unchanged.  Capacities: regions, items, first-list tasks and CIGAR words, second-list tasks and CIGAR
    words, pool bytes, anchors, output words, extra tasks."""

    _destroy = "mm2c_cigplan_destroy"

    def __init__(self, n_regs_cap, n_items_cap, n_tasks_cap, cigar_cap, n_tasks2_cap, cigar2_cap, pool_cap, n_b_cap, words_cap, n_extra_cap):
        self.n_regs_cap, self.n_items_cap, self.n_tasks_cap, self.cigar_cap = int(n_regs_cap), int(n_items_cap), int(n_tasks_cap), int(cigar_cap)
        self.n_tasks2_cap, self.cigar2_cap, self.pool_cap, self.n_b_cap = int(n_tasks2_cap), int(cigar2_cap), int(pool_cap), int(n_b_cap)
        self.words_cap, self.n_extra_cap = int(words_cap), int(n_extra_cap)
        self._create("mm2c_cigplan_create", self.n_regs_cap, self.n_items_cap, self.n_tasks_cap, self.cigar_cap, self.n_tasks2_cap, self.cigar2_cap, self.pool_cap, self.n_b_cap,
                     self.words_cap, self.n_extra_cap, code=-2)

    def second(self, opt, score, n_regs, aln_regs: torch.Tensor, items: torch.Tensor, tasks: torch.Tensor, zres: torch.Tensor, seq: torch.Tensor = None,
               tasks2: torch.Tensor = None, cig_off2: torch.Tensor = None, second_of: torch.Tensor = None, stream=None):
        """the arrays of AlnPlan.run (aln_regs, items, tasks, pool as seq) and of ExtraPlan.zdrop (zres) as they lie on the GPU -> (tasks2 uint8 [n_tasks2_cap, 40],
        cig_off2 int64 [n_tasks2_cap + 1], second_of int32 [n_items_cap]) GPU tensors (given ones are written into).  Asynchronous."""
        n = int(n_regs)
        for t in (aln_regs, items, tasks, zres):
            assert t.is_cuda and t.is_contiguous()
        assert 0 <= n <= self.n_regs_cap and aln_regs.numel() * aln_regs.element_size() >= n * ALN_REG_DTYPE.itemsize
        assert items.numel() * items.element_size() >= self.n_items_cap * ALN_ITEM_DTYPE.itemsize and tasks.numel() * tasks.element_size() >= self.n_tasks_cap * KSW_TASK_DTYPE.itemsize
        assert zres.numel() * zres.element_size() >= self.n_tasks_cap * ZDROP_RES_DTYPE.itemsize
        assert seq is None or (seq.is_cuda and seq.element_size() == 1 and seq.numel() >= self.pool_cap)
        dev = aln_regs.device
        tasks2 = _out(tasks2, (max(self.n_tasks2_cap, 1), KSW_TASK_DTYPE.itemsize), torch.uint8, dev, self.n_tasks2_cap * KSW_TASK_DTYPE.itemsize)
        cig_off2 = _out(cig_off2, self.n_tasks2_cap + 1, torch.int64, dev, (self.n_tasks2_cap + 1) * 8, "dtype")
        second_of = _out(second_of, max(self.n_items_cap, 1), torch.int32, dev, self.n_items_cap * 4, "dtype")
        o, sc = _cig_opt_bytes(opt), _ksw_score_bytes(score)
        st = _stream(stream)
        N.check(self.lib.mm2c_cigplan_second_run_device(self.handle, _np_ptr(o), _np_ptr(sc), n, aln_regs.data_ptr(), items.data_ptr(), tasks.data_ptr(), zres.data_ptr(),
                                                        seq.data_ptr() if seq is not None else None, tasks2.data_ptr(), cig_off2.data_ptr(), second_of.data_ptr(), st),
                "mm2c_cigplan_second_run_device")
        return tasks2, cig_off2, second_of

    def join(self, opt, n_reads, n_regs, u_off: torch.Tensor, regs: torch.Tensor, b_off: torch.Tensor, b: torch.Tensor, read_off: torch.Tensor, aln_regs: torch.Tensor,
             items: torch.Tensor, cig_off: torch.Tensor, res: torch.Tensor, cigar: torch.Tensor, zres: torch.Tensor, second_of: torch.Tensor, cig_off2: torch.Tensor,
             res2: torch.Tensor, cigar2: torch.Tensor, n_b: torch.Tensor = None, cig_regs: torch.Tensor = None, cig_out: torch.Tensor = None, in_off: torch.Tensor = None,
             extra_tasks: torch.Tensor = None, extra_reg: torch.Tensor = None, stream=None):
        """the batch (u_off, regs, b_off, b, read_off), the arrays of AlnPlan.run, KswPlan.run and ExtraPlan.zdrop, and those of second() with the KswPlan.run over its list,
        all on the GPU -> (cig_regs uint8 [n_regs, 72], cig_out int32 [words_cap], in_off int64 [n_extra_cap + 1], extra_tasks uint8 [n_extra_cap, 32], extra_reg int32
        [n_extra_cap]) GPU tensors (given ones are written into).  Asynchronous."""
        n_reads, n = int(n_reads), int(n_regs)
        for t in (u_off, regs, b_off, b, read_off, aln_regs, items, cig_off, res, cigar, zres, second_of, cig_off2, res2, cigar2):
            assert t.is_cuda and t.is_contiguous()
        assert all(t.dtype == torch.int64 and t.numel() >= n_reads + 1 for t in (u_off, b_off, read_off)) and 0 <= n <= self.n_regs_cap
        assert regs.numel() * regs.element_size() >= n * REG_DTYPE.itemsize and b.numel() * b.element_size() >= 16 * self.n_b_cap
        assert aln_regs.numel() * aln_regs.element_size() >= n * ALN_REG_DTYPE.itemsize and items.numel() * items.element_size() >= self.n_items_cap * ALN_ITEM_DTYPE.itemsize
        assert cig_off.dtype == torch.int64 and cig_off.numel() >= self.n_tasks_cap + 1 and cig_off2.dtype == torch.int64 and cig_off2.numel() >= self.n_tasks2_cap + 1
        assert res.numel() * res.element_size() >= self.n_tasks_cap * KSW_RES_DTYPE.itemsize and res2.numel() * res2.element_size() >= self.n_tasks2_cap * KSW_RES_DTYPE.itemsize
        assert zres.numel() * zres.element_size() >= self.n_tasks_cap * ZDROP_RES_DTYPE.itemsize and second_of.dtype == torch.int32 and second_of.numel() >= self.n_items_cap
        assert cigar.element_size() == 4 and cigar.numel() >= self.cigar_cap and cigar2.element_size() == 4 and cigar2.numel() >= self.cigar2_cap
        assert n_b is None or (n_b.is_cuda and n_b.dtype == torch.int64 and n_b.numel() >= n_reads)
        dev = regs.device
        cig_regs = _out(cig_regs, (max(n, 1), CIG_REG_DTYPE.itemsize), torch.uint8, dev, n * CIG_REG_DTYPE.itemsize)
        cig_out = _out(cig_out, max(self.words_cap, 1), torch.int32, dev, self.words_cap * 4, "width")
        in_off = _out(in_off, self.n_extra_cap + 1, torch.int64, dev, (self.n_extra_cap + 1) * 8, "dtype")
        extra_tasks = _out(extra_tasks, (max(self.n_extra_cap, 1), EXTRA_TASK_DTYPE.itemsize), torch.uint8, dev, self.n_extra_cap * EXTRA_TASK_DTYPE.itemsize)
        extra_reg = _out(extra_reg, max(self.n_extra_cap, 1), torch.int32, dev, self.n_extra_cap * 4, "dtype")
        o = _cig_opt_bytes(opt)
        st = _stream(stream)
        N.check(self.lib.mm2c_cigplan_run_device(self.handle, _np_ptr(o), n_reads, n, u_off.data_ptr(), regs.data_ptr(), b_off.data_ptr(), n_b.data_ptr() if n_b is not None else None,
                                                 b.data_ptr(), read_off.data_ptr(), aln_regs.data_ptr(), items.data_ptr(), cig_off.data_ptr(), res.data_ptr(), cigar.data_ptr(),
                                                 zres.data_ptr(), second_of.data_ptr(), cig_off2.data_ptr(), res2.data_ptr(), cigar2.data_ptr(), cig_regs.data_ptr(),
                                                 cig_out.data_ptr(), in_off.data_ptr(), extra_tasks.data_ptr(), extra_reg.data_ptr(), st), "mm2c_cigplan_run_device")
        return cig_regs, cig_out, in_off, extra_tasks, extra_reg

    def second_counts(self):
        """waits for the last second() -> (return code, refused, regions beyond a capacity, (tasks, CIGAR words) of the second list)"""
        a, b, t = C.c_int64(0), C.c_int64(0), (C.c_int64 * 2)()
        rc = self.lib.mm2c_cigplan_second_check(self.handle, C.byref(a), C.byref(b), t)
        return rc, a.value, b.value, tuple(int(x) for x in t)

    def second_check(self):
        rc, _, _, tot = self.second_counts()
        N.check(rc, "mm2c_cigplan_second_check")
        return tot

    def counts(self):
        """waits for the last join() -> (return code, regions refused, incomplete, beyond a capacity, (CIGAR words, extra tasks) the batch takes)"""
        a, b, c, t = C.c_int64(0), C.c_int64(0), C.c_int64(0), (C.c_int64 * 2)()
        rc = self.lib.mm2c_cigplan_check(self.handle, C.byref(a), C.byref(b), C.byref(c), t)
        return rc, a.value, b.value, c.value, tuple(int(x) for x in t)

    def check(self):
        """waits for the last join(); raises (code -2) if a region was refused, (code -3) if one was incomplete or left a capacity; returns the totals"""
        rc, _, _, _, tot = self.counts()
        N.check(rc, "mm2c_cigplan_check")
        return tot

    def last_kernel_ms(self):
        """(cig_second_count with its scan, cig_second_emit, cig_cut, cig_scan, cig_gather) of the last runs; 0 for an entry that has not run"""
        ms = (C.c_float * 5)()
        N.check(self.lib.mm2c_cigplan_last_kernel_ms(self.handle, ms), "mm2c_cigplan_last_kernel_ms")
        return tuple(float(x) for x in ms)

    def last_ms(self):
        return sum(self.last_kernel_ms())


def second_pass_batch(opt, score, aln_regs, items, tasks, zres, pool, n_tasks2_cap, fill=None):
    """mm2c_second_pass_batch_host: host arrays in (aln_regs ALN_REG_DTYPE, items ALN_ITEM_DTYPE, tasks KSW_TASK_DTYPE, zres ZDROP_RES_DTYPE, pool uint8) ->
    dict(tasks2, cig_off2, second_of, totals, rc); rc is 0 or -3 (the second list leaves n_tasks2_cap).  Raises for any other failure.  fill: a byte the outputs are
    filled with beforehand (tests)."""
    lib = N.load()
    ar = np.ascontiguousarray(aln_regs, dtype=ALN_REG_DTYPE); it = np.ascontiguousarray(items, dtype=ALN_ITEM_DTYPE); tk = np.ascontiguousarray(tasks, dtype=KSW_TASK_DTYPE)
    zr = np.ascontiguousarray(zres, dtype=ZDROP_RES_DTYPE); pl = np.ascontiguousarray(pool, dtype=np.uint8)
    if zr.size < tk.size:
        raise ValueError("zres must hold one record per task")
    f = 0 if fill is None else int(fill)
    cap = int(n_tasks2_cap)
    tasks2 = np.full(max(cap, 1) * KSW_TASK_DTYPE.itemsize, f, np.uint8).view(KSW_TASK_DTYPE)
    cig_off2 = np.full((cap + 1) * 8, f, np.uint8).view(np.int64)
    second_of = np.full(max(it.size, 1) * 4, f, np.uint8).view(np.int32)
    tot = (C.c_int64 * 2)()
    o, sc = _cig_opt_bytes(opt), _ksw_score_bytes(score)
    rc = lib.mm2c_second_pass_batch_host(_np_ptr(o), _np_ptr(sc), ar.size, _np_ptr(ar), it.size, _np_ptr(it), tk.size, _np_ptr(tk), _np_ptr(zr), pl.size, _np_ptr(pl), cap,
                                         _np_ptr(tasks2), _np_ptr(cig_off2), _np_ptr(second_of), tot)
    if rc not in (0, -3):
        N.check(rc, "mm2c_second_pass_batch_host")
    return dict(tasks2=tasks2[:cap], cig_off2=cig_off2, second_of=second_of[:it.size], totals=tuple(int(x) for x in tot), rc=rc)


def assemble_regions_batch(opt, u_off, regs, b_off, b, read_off, aln_regs, items, cig_off, res, cigar, zres, second_of, cig_off2, res2, cigar2, words_cap, n_extra_cap, fill=None):
    """mm2c_assemble_regions_batch_host: host arrays in -> dict(cig_regs CIG_REG_DTYPE, cig_out uint32 [words_cap], in_off int64 [n_extra_cap + 1], extra_tasks
    EXTRA_TASK_DTYPE, extra_reg int32, totals, rc); rc is 0 or -3 (a region incomplete or beyond a capacity: the rest is complete all the same).  Raises for any other
    failure.  fill: a byte the outputs are filled with beforehand (tests)."""
    lib = N.load()
    uo = np.ascontiguousarray(u_off, dtype=np.int64); bo = np.ascontiguousarray(b_off, dtype=np.int64); ro = np.ascontiguousarray(read_off, dtype=np.int64)
    rg = np.ascontiguousarray(regs, dtype=REG_DTYPE); bb = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 2)
    ar = np.ascontiguousarray(aln_regs, dtype=ALN_REG_DTYPE); it = np.ascontiguousarray(items, dtype=ALN_ITEM_DTYPE)
    co = np.ascontiguousarray(cig_off, dtype=np.int64); rs = np.ascontiguousarray(res, dtype=KSW_RES_DTYPE); cg = np.ascontiguousarray(cigar, dtype=np.uint32)
    zr = np.ascontiguousarray(zres, dtype=ZDROP_RES_DTYPE); so = np.ascontiguousarray(second_of, dtype=np.int32)
    c2 = np.ascontiguousarray(cig_off2, dtype=np.int64); r2 = np.ascontiguousarray(res2, dtype=KSW_RES_DTYPE); g2 = np.ascontiguousarray(cigar2, dtype=np.uint32)
    n_reads = uo.size - 1
    if bo.size != n_reads + 1 or ro.size != n_reads + 1:
        raise ValueError("u_off, b_off and read_off must hold n_reads + 1 offsets")
    n_regs = int(uo[-1]) if n_reads > 0 else 0
    n_tasks, n_tasks2 = rs.size, r2.size
    if rg.size < n_regs or ar.size < n_regs or bb.shape[0] < int(bo[-1]) or co.size < n_tasks + 1 or c2.size < n_tasks2 + 1 or zr.size < n_tasks or so.size < it.size:
        raise ValueError("an array is shorter than its offsets say")
    if cg.size < int(co[n_tasks]) or g2.size < int(c2[n_tasks2]):
        raise ValueError("a CIGAR buffer is shorter than its offsets say")
    f = 0 if fill is None else int(fill)
    wc, xc = int(words_cap), int(n_extra_cap)
    cig_regs = np.full(max(n_regs, 1) * CIG_REG_DTYPE.itemsize, f, np.uint8).view(CIG_REG_DTYPE)
    cig_out = np.full(max(wc, 1) * 4, f, np.uint8).view(np.uint32)
    in_off = np.full((xc + 1) * 8, f, np.uint8).view(np.int64)
    extra_tasks = np.full(max(xc, 1) * EXTRA_TASK_DTYPE.itemsize, f, np.uint8).view(EXTRA_TASK_DTYPE)
    extra_reg = np.full(max(xc, 1) * 4, f, np.uint8).view(np.int32)
    tot = (C.c_int64 * 2)()
    o = _cig_opt_bytes(opt)
    rc = lib.mm2c_assemble_regions_batch_host(_np_ptr(o), n_reads, _np_ptr(uo), _np_ptr(rg), _np_ptr(bo), _np_ptr(bb), _np_ptr(ro), _np_ptr(ar), it.size, _np_ptr(it), n_tasks,
                                              _np_ptr(co), _np_ptr(rs), _np_ptr(cg), _np_ptr(zr), _np_ptr(so), n_tasks2, _np_ptr(c2), _np_ptr(r2), _np_ptr(g2), _np_ptr(cig_regs),
                                              wc, _np_ptr(cig_out), xc, _np_ptr(in_off), _np_ptr(extra_tasks), _np_ptr(extra_reg), tot)
    if rc not in (0, -3):
        N.check(rc, "mm2c_assemble_regions_batch_host")
    return dict(cig_regs=cig_regs[:n_regs], cig_out=cig_out[:wc], in_off=in_off, extra_tasks=extra_tasks[:xc], extra_reg=extra_reg[:xc], totals=tuple(int(x) for x in tot), rc=rc)


class MapqPlan(_Handle):
    """mm2c_mapqplan_t: hits -> final regions with mapping quality on the GPU (mm_join_long hit.c:295-371, mm_set_mapq hit.c:463-508) for batches of up to n_reads
    reads, n_u_cap regions and n_b_cap chain anchors; it stands behind a HitPlan on the same stream.  max_log_arg: the largest score (and n_sub + 1) whose logf the
    plan's table holds -- the host's own logf, filled at creation; 2^22 (16 MB) by default, at most 2^24 - 1."""

    _destroy = "mm2c_mapqplan_destroy"

    def __init__(self, n_reads, n_u_cap, n_b_cap, max_log_arg=1 << 22):
        self.n_reads, self.n_u_cap, self.n_b_cap, self.max_log_arg = int(n_reads), int(n_u_cap), int(n_b_cap), int(max_log_arg)
        self._create("mm2c_mapqplan_create", self.n_reads, self.n_u_cap, self.n_b_cap, self.max_log_arg)

    def run(self, opt, u_off: torch.Tensor, regs_in: torch.Tensor, n_in: torch.Tensor, b_off: torch.Tensor, b: torch.Tensor, qlen: torch.Tensor,
            rep_len: torch.Tensor, regs_out: torch.Tensor = None, n_out: torch.Tensor = None, anchors=False, b_out: torch.Tensor = None,
            n_b_out: torch.Tensor = None, stream=None):
        """opt: params.mapq_opts(); u_off, regs_in and n_in as HitPlan.run took and returned them, b_off / b the device epilogue's chain anchors, qlen and rep_len
        int32 per read, all on the GPU.  Returns (regs_out uint8 [n_u_cap, 80], n_out int32 [n_reads], b_out, n_b_out): the final regions of read r are rows
        u_off[r] .. u_off[r] + n_out[r].  With anchors=True (or b_out given) b_out int64 [n_b_cap, 2] holds, from b_off[r] on, the n_b_out[r] anchors of the
        reference's a[] behind mm_join_long; otherwise both are None, no anchor is copied and the join bit is not recorded.  Asynchronous."""
        for t in (u_off, regs_in, n_in, b_off, b, qlen, rep_len):
            assert t.is_cuda and t.is_contiguous()
        assert u_off.dtype == torch.int64 and b_off.dtype == torch.int64 and u_off.numel() == self.n_reads + 1 and b_off.numel() == self.n_reads + 1
        assert regs_in.numel() * regs_in.element_size() >= self.n_u_cap * REG_DTYPE.itemsize and b.element_size() == 8 and b.numel() >= 2 * self.n_b_cap
        assert n_in.dtype == torch.int32 and n_in.numel() >= self.n_reads and qlen.dtype == torch.int32 and qlen.numel() == self.n_reads
        assert rep_len.dtype == torch.int32 and rep_len.numel() == self.n_reads
        dev = u_off.device
        regs_out = _out(regs_out, (max(self.n_u_cap, 1), REG_DTYPE.itemsize), torch.uint8, dev, self.n_u_cap * REG_DTYPE.itemsize)
        n_out = _out(n_out, max(self.n_reads, 1), torch.int32, dev, self.n_reads * 4, "dtype")
        if anchors or b_out is not None or n_b_out is not None:
            b_out = _out(b_out, (max(self.n_b_cap, 1), 2), torch.int64, dev, self.n_b_cap * 16, "width")
            n_b_out = _out(n_b_out, max(self.n_reads, 1), torch.int64, dev, self.n_reads * 8, "dtype")
        st = _stream(stream)
        N.check(self.lib.mm2c_mapqplan_run_device(self.handle, C.byref(opt), u_off.data_ptr(), regs_in.data_ptr(), n_in.data_ptr(), b_off.data_ptr(), b.data_ptr(),
                                                  qlen.data_ptr(), rep_len.data_ptr(), regs_out.data_ptr(), n_out.data_ptr(),
                                                  b_out.data_ptr() if b_out is not None else None, n_b_out.data_ptr() if b_out is not None else None, st),
                "mm2c_mapqplan_run_device")
        return regs_out, n_out[:self.n_reads], b_out, (n_b_out[:self.n_reads] if b_out is not None else None)

    def counts(self):
        """waits for the run -> (return code, joins made, primaries beyond the table) without raising"""
        nj, nb = C.c_int64(0), C.c_int64(0)
        rc = self.lib.mm2c_mapqplan_check(self.handle, C.byref(nj), C.byref(nb))
        return rc, nj.value, nb.value

    def check(self):
        """waits for the run; raises if a read was refused for its offsets (code -2) or a primary lay beyond the table (code -3); returns the number of joins"""
        rc, nj, _ = self.counts()
        N.check(rc, "mm2c_mapqplan_check")
        return nj

    def last_ms(self):
        return self._ms("mm2c_mapqplan_last_ms")[0]

    def last_kernel_ms(self):
        """(mapq_join, mapq_gather) of the last run; the second is 0 when no anchors were asked for"""
        return self._ms("mm2c_mapqplan_last_kernel_ms", 2)


def join_mapq_batch(opt, u_off, regs, n_in, b_off, b, qlen, rep_len, anchors=True, max_log_arg=1 << 22):
    """mm2c_join_mapq_batch_host: host arrays in -> (regs_out REG_DTYPE [u_off[-1] - u_off[0]], n_out int32 [n_reads], b_out uint64 [b_off[-1] - b_off[0], 2] or
    None, n_b_out int64 [n_reads] or None); the final regions of read r are regs_out[u_off[r] - u_off[0] :][:n_out[r]], its anchors
    b_out[b_off[r] - b_off[0] :][:n_b_out[r]].  Raises with code -3 when a primary lay beyond the table of max_log_arg entries."""
    lib = N.load()
    uo = _i64(u_off); bo = _i64(b_off)
    rr = _reg_rows(regs)
    bb = _anchor_rows(b)
    ni = np.ascontiguousarray(n_in, dtype=np.int32); q = np.ascontiguousarray(qlen, dtype=np.int32); rl = np.ascontiguousarray(rep_len, dtype=np.int32)
    n_reads = uo.size - 1
    if bo.size != uo.size or ni.size != n_reads or q.size != n_reads or rl.size != n_reads or \
            not _fit(n_reads, (uo, rr.shape[0]), (bo, bb.shape[0])):
        raise ValueError("offsets do not fit the arrays")
    n_u = int(uo[-1] - uo[0]) if n_reads > 0 else 0
    n_b = int(bo[-1] - bo[0]) if n_reads > 0 else 0
    out = np.zeros(max(n_u, 1), REG_DTYPE)
    n_out = np.zeros(max(n_reads, 1), np.int32)
    b_out = np.zeros((max(n_b, 1), 2), np.uint64) if anchors else None
    n_b_out = np.zeros(max(n_reads, 1), np.int64) if anchors else None
    N.check(lib.mm2c_join_mapq_batch_host(n_reads, C.byref(opt), int(max_log_arg), _np_ptr(uo), _np_ptr(rr), _np_ptr(ni), _np_ptr(bo), _np_ptr(bb), _np_ptr(q),
                                          _np_ptr(rl), _np_ptr(out), _np_ptr(n_out), _np_ptr(b_out) if anchors else None, _np_ptr(n_b_out) if anchors else None),
            "mm2c_join_mapq_batch_host")
    return out[:n_u], n_out[:n_reads], (b_out[:n_b] if anchors else None), (n_b_out[:n_reads] if anchors else None)


PEXT_DTYPE = np.dtype([("dp_score", "<i4"), ("dp_max", "<i4"), ("dp_max2", "<i4"), ("ambi_strand", "<u4"), ("n_cigar", "<i4"), ("reserved", "<i4"), ("cig0", "<i8")])   # mm2c_pext_t
FIN_REFUSED, FIN_INCOMPLETE, FIN_OVER_CAP = 1, 2, 3


class FinPlan(_Handle):
    """mm2c_finplan_t: aligned regions -> final hits on the GPU for batches of up to n_reads reads, n_u_cap regions and n_pext_cap mm2c_pext_t records.  apply():
    what mm_align1 leaves in a region, with mm_split_reg (align.c:757-760, 781-783; hit.c:108-123).  run(): mm_filter_regs, mm_hit_sort, mm_set_parent, mm_select_sub,
    mm_set_sam_pri and mm_set_mapq (align.c:917-918, map.c:264-268, 361).  max_log_arg: the largest dp_max, score and n_sub + 1 whose logf the plan's two tables hold
    -- the host's own logf, filled at creation; match_sc: opt->a, the divisor of the second table."""

    _destroy = "mm2c_finplan_destroy"

    def __init__(self, n_reads, n_u_cap, n_pext_cap, max_log_arg=1 << 20, match_sc=2):
        self.n_reads, self.n_u_cap, self.n_pext_cap, self.max_log_arg, self.match_sc = int(n_reads), int(n_u_cap), int(n_pext_cap), int(max_log_arg), int(match_sc)
        self._create("mm2c_finplan_create", self.n_reads, self.n_u_cap, self.n_pext_cap, self.max_log_arg, self.match_sc, code=-2)

    def apply(self, n_reads, n_regs, u_off: torch.Tensor, regs: torch.Tensor, b_off: torch.Tensor, b: torch.Tensor, read_off: torch.Tensor, cig_regs: torch.Tensor,
              n_extra, extra_reg: torch.Tensor, extra_res: torch.Tensor, out_off: torch.Tensor, n_child_cap, regs_out: torch.Tensor = None, pext: torch.Tensor = None,
              status: torch.Tensor = None, child: torch.Tensor = None, child_of: torch.Tensor = None, n_child: torch.Tensor = None, stream=None):
        """u_off, regs, b_off, b, read_off as AlnPlan.run took them, cig_regs as CigPlan.join wrote them, extra_reg (CigPlan.join), extra_res and out_off (ExtraPlan.update)
        of the first n_extra entries; all on the GPU.  Returns (regs_out uint8 [n_regs, 80], pext uint8 [n_regs, 32], status int32 [n_regs], child uint8
        [n_child_cap, 80], child_of int32 [n_child_cap], n_child int64 [1]).  Asynchronous."""
        n_reads, n_regs, n_extra, cap = int(n_reads), int(n_regs), int(n_extra), int(n_child_cap)
        for t in (u_off, regs, b_off, b, read_off, cig_regs, extra_reg, extra_res, out_off):
            assert t.is_cuda and t.is_contiguous()
        assert u_off.dtype == torch.int64 and b_off.dtype == torch.int64 and read_off.dtype == torch.int64 and out_off.dtype == torch.int64 and extra_reg.dtype == torch.int32
        assert u_off.numel() >= n_reads + 1 and b_off.numel() >= n_reads + 1 and read_off.numel() >= n_reads + 1 and out_off.numel() >= n_extra + 1 and extra_reg.numel() >= n_extra
        assert regs.numel() * regs.element_size() >= n_regs * REG_DTYPE.itemsize and cig_regs.numel() * cig_regs.element_size() >= n_regs * CIG_REG_DTYPE.itemsize
        assert extra_res.numel() * extra_res.element_size() >= n_extra * EXTRA_RES_DTYPE.itemsize and b.element_size() == 8
        dev = u_off.device
        regs_out = _out(regs_out, (max(n_regs, 1), REG_DTYPE.itemsize), torch.uint8, dev, n_regs * REG_DTYPE.itemsize)
        pext = _out(pext, (max(n_regs, 1), PEXT_DTYPE.itemsize), torch.uint8, dev, n_regs * PEXT_DTYPE.itemsize)
        status = _out(status, max(n_regs, 1), torch.int32, dev, n_regs * 4, "dtype")
        child = _out(child, (max(cap, 1), REG_DTYPE.itemsize), torch.uint8, dev, cap * REG_DTYPE.itemsize)
        child_of = _out(child_of, max(cap, 1), torch.int32, dev, cap * 4, "dtype")
        n_child = _out(n_child, 1, torch.int64, dev, 8, "dtype")
        N.check(self.lib.mm2c_finplan_apply_run_device(self.handle, n_reads, n_regs, u_off.data_ptr(), regs.data_ptr(), b_off.data_ptr(), b.data_ptr(), b.numel() // 2,
                                                       read_off.data_ptr(), cig_regs.data_ptr(), n_extra, extra_reg.data_ptr(), extra_res.data_ptr(), out_off.data_ptr(),
                                                       regs_out.data_ptr(), pext.data_ptr(), status.data_ptr(), cap, child.data_ptr(), child_of.data_ptr(), n_child.data_ptr(),
                                                       _stream(stream)), "mm2c_finplan_apply_run_device")
        return regs_out[:n_regs], pext[:n_regs], status[:n_regs], child[:cap], child_of[:cap], n_child

    def run(self, opt, f_off: torch.Tensor, regs_in: torch.Tensor, n_in: torch.Tensor, pext: torch.Tensor, qlen: torch.Tensor, rep_len: torch.Tensor,
            regs_out: torch.Tensor = None, n_out: torch.Tensor = None, stream=None):
        """opt: params.fin_opts(); the regions of read r are rows f_off[r] .. f_off[r] + n_in[r] of regs_in, every child directly behind its parent; pext the
        mm2c_pext_t records their p names (dp_max2 is updated in place); qlen and rep_len int32 per read; all on the GPU.  Returns (regs_out uint8 [n_u_cap, 80],
        n_out int32 [n_reads]): the final hits of read r are rows f_off[r] .. f_off[r] + n_out[r].  Asynchronous."""
        for t in (f_off, regs_in, n_in, pext, qlen, rep_len):
            assert t.is_cuda and t.is_contiguous()
        assert f_off.dtype == torch.int64 and f_off.numel() == self.n_reads + 1 and n_in.dtype == torch.int32 and n_in.numel() >= self.n_reads
        assert regs_in.numel() * regs_in.element_size() >= self.n_u_cap * REG_DTYPE.itemsize and pext.numel() * pext.element_size() >= self.n_pext_cap * PEXT_DTYPE.itemsize
        assert qlen.dtype == torch.int32 and qlen.numel() == self.n_reads and rep_len.dtype == torch.int32 and rep_len.numel() == self.n_reads
        dev = f_off.device
        regs_out = _out(regs_out, (max(self.n_u_cap, 1), REG_DTYPE.itemsize), torch.uint8, dev, self.n_u_cap * REG_DTYPE.itemsize)
        n_out = _out(n_out, max(self.n_reads, 1), torch.int32, dev, self.n_reads * 4, "dtype")
        N.check(self.lib.mm2c_finplan_run_device(self.handle, C.byref(opt), f_off.data_ptr(), regs_in.data_ptr(), n_in.data_ptr(), pext.data_ptr(), qlen.data_ptr(),
                                                 rep_len.data_ptr(), regs_out.data_ptr(), n_out.data_ptr(), _stream(stream)), "mm2c_finplan_run_device")
        return regs_out, n_out[:self.n_reads]

    def counts(self):
        """waits for the last run() -> (return code, reads refused, primaries beyond the tables, final hits of all reads) without raising"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = self.lib.mm2c_finplan_check(self.handle, C.byref(a), C.byref(b), C.byref(c))
        return rc, a.value, b.value, c.value

    def apply_counts(self):
        """waits for the last apply() -> (return code, regions refused, regions incomplete, children beyond n_child_cap) without raising"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = self.lib.mm2c_finplan_apply_check(self.handle, C.byref(a), C.byref(b), C.byref(c))
        return rc, a.value, b.value, c.value

    def check(self):
        """waits for the last run(); raises if a read was refused (code -2) or a primary lay beyond the tables (code -3); returns the number of final hits"""
        rc, _, _, n = self.counts()
        N.check(rc, "mm2c_finplan_check")
        return n

    def apply_check(self):
        rc = self.apply_counts()[0]
        N.check(rc, "mm2c_finplan_apply_check")

    def last_ms(self):
        """(the apply entry's kernels, fin_select) of the last runs; 0 for an entry that has not run"""
        return self._ms("mm2c_finplan_last_ms", 2)


def apply_regions_batch(u_off, regs, b_off, b, read_off, cig_regs, extra_reg, extra_res, out_off, n_child_cap, fill=None):
    """mm2c_apply_regions_batch_host: host arrays in -> dict(regs REG_DTYPE, pext PEXT_DTYPE, status int32, child REG_DTYPE [n_child_cap], child_of int32, n_child, rc);
    rc is 0, -2 (a region refused) or -3 (a region incomplete, or children beyond n_child_cap): the rest is complete all the same.  Raises for any other failure, an argument
    refused before the device ran included.  fill: a byte the outputs are filled with beforehand (tests)."""
    lib = N.load()
    uo = _i64(u_off); bo = _i64(b_off); ro = _i64(read_off); oo = _i64(out_off)
    rg = np.ascontiguousarray(regs, dtype=REG_DTYPE); bb = _anchor_rows(b); cr = np.ascontiguousarray(cig_regs, dtype=CIG_REG_DTYPE)
    xr = np.ascontiguousarray(extra_reg, dtype=np.int32); xe = np.ascontiguousarray(extra_res, dtype=EXTRA_RES_DTYPE)
    n_reads = uo.size - 1
    if bo.size != n_reads + 1 or ro.size != n_reads + 1:
        raise ValueError("u_off, b_off and read_off must hold n_reads + 1 offsets")
    n_regs = int(uo[-1]) if n_reads > 0 else 0
    n_extra = xr.size
    if rg.size < n_regs or cr.size < n_regs or (n_reads > 0 and bb.shape[0] < int(bo[-1])) or xe.size < n_extra or (n_extra > 0 and oo.size < n_extra + 1):
        raise ValueError("an array is shorter than its offsets say")
    f = 0 if fill is None else int(fill)
    cap = int(n_child_cap)
    out = np.full(max(n_regs, 1) * REG_DTYPE.itemsize, f, np.uint8).view(REG_DTYPE)
    pext = np.full(max(n_regs, 1) * PEXT_DTYPE.itemsize, f, np.uint8).view(PEXT_DTYPE)
    status = np.full(max(n_regs, 1) * 4, f, np.uint8).view(np.int32)
    child = np.full(max(cap, 1) * REG_DTYPE.itemsize, f, np.uint8).view(REG_DTYPE)
    child_of = np.full(max(cap, 1) * 4, f, np.uint8).view(np.int32)
    n_child = np.zeros(1, np.int64)
    rc = lib.mm2c_apply_regions_batch_host(n_reads, _np_ptr(uo), _np_ptr(rg), _np_ptr(bo), _np_ptr(bb), _np_ptr(ro), _np_ptr(cr), n_extra, _np_ptr(xr), _np_ptr(xe), _np_ptr(oo),
                                           _np_ptr(out), _np_ptr(pext), _np_ptr(status), cap, _np_ptr(child), _np_ptr(child_of), _np_ptr(n_child))
    if rc not in (0, -3) and not (rc == -2 and b"only their status is written" in (lib.mm2c_last_error() or b"")):
        N.check(rc, "mm2c_apply_regions_batch_host")
    return dict(regs=out[:n_regs], pext=pext[:n_regs], status=status[:n_regs], child=child[:cap], child_of=child_of[:cap], n_child=int(n_child[0]), rc=rc)


def interleave_rounds(rounds):
    """The order mm_align_skeleton holds a read's regions in behind its loop (mm_insert_reg, align.c:905: a child directly behind its parent, a grandchild behind the
    child), from the outputs of FinPlan.apply / apply_regions_batch over the alignment rounds: index arithmetic on child_of, on the host.
    rounds: one dict per round, in order: u_off (int64 [n_reads + 1]: the round's regions per read; round 0's are the reads' own, a later round's are the children of the
    round before, in order), regs (REG_DTYPE [n]: as apply wrote them, p = index + 1 or 0), pext (PEXT_DTYPE [n]) and child_of (int32 [n_child]: the region of this
    round every child was split from; absent or empty in the last round).  A region whose apply status is not 0 has no place in a list: the caller leaves such a
    read out or mends it first.
    -> (f_off int64 [n_reads + 1], regs REG_DTYPE, pext PEXT_DTYPE): the lists FinPlan.run / finish_regions_batch take (n_in = f_off[1:] - f_off[:-1]); pext is
    the rounds' records one after another, and every p is 1 + its record's index there."""
    if not rounds:
        return np.zeros(1, np.int64), np.zeros(0, REG_DTYPE), np.zeros(0, PEXT_DTYPE)
    R = [np.ascontiguousarray(r["regs"]).reshape(-1).view(REG_DTYPE) for r in rounds]
    P = [np.ascontiguousarray(r["pext"]).reshape(-1).view(PEXT_DTYPE) for r in rounds]
    base = np.concatenate([[0], np.cumsum([r.size for r in R])])
    child = []                                                                 # per round: region -> its child in the next round, -1
    for k, r in enumerate(rounds):
        c = np.full(R[k].size, -1, np.int64)
        of = np.asarray(r.get("child_of", ()), np.int64).reshape(-1)
        if of.size:
            if k + 1 >= len(rounds) or of.size != R[k + 1].size or (of < 0).any() or (of >= R[k].size).any() or (np.diff(of) <= 0).any():
                raise ValueError(f"round {k}: child_of does not name the regions of round {k + 1} in ascending order")
            c[of] = np.arange(of.size)
        child.append(c)
    u_off = _i64(rounds[0]["u_off"])
    n_reads = u_off.size - 1
    order, f_off = [], [0]
    for rd in range(n_reads):
        for g in range(int(u_off[rd]), int(u_off[rd + 1])):
            k = 0
            while g >= 0:
                order.append(int(base[k]) + g)
                g, k = int(child[k][g]), k + 1
        f_off.append(len(order))
    if len(order) != int(base[-1]):
        raise ValueError("regions of a later round that no child_of names")
    allr, order = np.concatenate(R), np.array(order, np.int64)
    src_base = base[np.searchsorted(base, order, side="right") - 1]
    out = allr[order].copy()
    has = out["p"] != 0
    out["p"][has] += src_base[has].astype(np.uint64)
    return np.array(f_off, np.int64), out, np.concatenate(P)


def finish_regions_batch(opt, f_off, regs, n_in, pext, qlen, rep_len, max_log_arg=1 << 20, fill=None):
    """mm2c_finish_regions_batch_host: host arrays in -> dict(regs REG_DTYPE [f_off[-1] - f_off[0]], n_out int32 [n_reads], pext (a copy, dp_max2 updated), rc); the final
    hits of read r are regs[f_off[r] - f_off[0] :][:n_out[r]].  rc is 0, -2 (a read refused on the device: nothing of it is written) or -3 (a primary beyond the
    tables): the rest is complete all the same.  Raises for any other failure.  fill: a byte regs and n_out are filled with beforehand (tests)."""
    lib = N.load()
    fo = _i64(f_off)
    rr = _reg_rows(regs)
    ni = np.ascontiguousarray(n_in, dtype=np.int32); q = np.ascontiguousarray(qlen, dtype=np.int32); rl = np.ascontiguousarray(rep_len, dtype=np.int32)
    px = np.array(pext, dtype=PEXT_DTYPE, copy=True).reshape(-1)
    n_reads = fo.size - 1
    if ni.size != n_reads or q.size != n_reads or rl.size != n_reads or not _fit(n_reads, (fo, rr.shape[0])):
        raise ValueError("offsets do not fit the arrays")
    n_u = int(fo[-1] - fo[0]) if n_reads > 0 else 0
    f = 0 if fill is None else int(fill)
    out = np.full(max(n_u, 1) * REG_DTYPE.itemsize, f, np.uint8).view(REG_DTYPE)
    n_out = np.full(max(n_reads, 1) * 4, f, np.uint8).view(np.int32)
    pp = px if px.size else np.zeros(1, PEXT_DTYPE)
    rc = lib.mm2c_finish_regions_batch_host(n_reads, C.byref(opt), int(max_log_arg), _np_ptr(fo), _np_ptr(rr), _np_ptr(ni), px.size, _np_ptr(pp), _np_ptr(q), _np_ptr(rl),
                                            _np_ptr(out), _np_ptr(n_out))
    if rc not in (0, -3) and not (rc == -2 and b"refused, nothing of them written" in (lib.mm2c_last_error() or b"")):
        N.check(rc, "mm2c_finish_regions_batch_host")
    return dict(regs=out[:n_u], n_out=n_out[:n_reads], pext=px, rc=rc)


class PairPlan(_Handle):
    """mm2c_pairplan_t: the two ends of a fragment paired on the GPU for batches of up to n_frags two-segment fragments, n_u_cap final regions and n_pext_cap
    mm2c_pext_t records: mm_pair with mm_set_pe_thru (pe.c:45-63, 76-177) and the flip of map.c:455-466, in place on the regions FinPlan.run wrote.  max_log_arg:
    the largest n_sub whose logf the plan's table holds -- the host's own logf, filled at creation."""

    _destroy = "mm2c_pairplan_destroy"

    def __init__(self, n_frags, n_u_cap, n_pext_cap, max_log_arg=1 << 16):
        self.n_frags, self.n_u_cap, self.n_pext_cap, self.max_log_arg = int(n_frags), int(n_u_cap), int(n_pext_cap), int(max_log_arg)
        self._create("mm2c_pairplan_create", self.n_frags, self.n_u_cap, self.n_pext_cap, self.max_log_arg, code=-2)

    def run(self, opt, f_off: torch.Tensor, regs: torch.Tensor, n: torch.Tensor, pext: torch.Tensor, seg_len: torch.Tensor, gap_ref: torch.Tensor = None,
            status: torch.Tensor = None, stream=None):
        """opt: params.pair_opts(); fragment f is the segment reads 2f and 2f + 1, the final regions of segment read r are rows f_off[r] .. f_off[r] + n[r] of regs
        (FinPlan.run's regs_out and n_out with the f_off it took); pext the records their p names; seg_len int32 per segment read; gap_ref int32 per fragment or
        None for opt.max_gap_ref; all on the GPU.  regs is updated in place.  Returns status int32 [n_frags]: 1 for a refused fragment.  Asynchronous."""
        for t in (f_off, regs, n, pext, seg_len) + (() if gap_ref is None else (gap_ref,)):
            assert t.is_cuda and t.is_contiguous()
        nr = 2 * self.n_frags
        assert f_off.dtype == torch.int64 and f_off.numel() == nr + 1 and n.dtype == torch.int32 and n.numel() >= nr and seg_len.dtype == torch.int32 and seg_len.numel() >= nr
        assert regs.numel() * regs.element_size() >= self.n_u_cap * REG_DTYPE.itemsize and pext.numel() * pext.element_size() >= self.n_pext_cap * PEXT_DTYPE.itemsize
        assert gap_ref is None or (gap_ref.dtype == torch.int32 and gap_ref.numel() >= self.n_frags)
        status = _out(status, max(self.n_frags, 1), torch.int32, f_off.device, self.n_frags * 4, "dtype")
        N.check(self.lib.mm2c_pairplan_run_device(self.handle, C.byref(opt), f_off.data_ptr(), regs.data_ptr(), n.data_ptr(), pext.data_ptr(), seg_len.data_ptr(),
                                                  None if gap_ref is None else gap_ref.data_ptr(), status.data_ptr(), _stream(stream)), "mm2c_pairplan_run_device")
        return status[:self.n_frags]

    def counts(self):
        """waits for the last run() -> (return code, fragments refused, fragments with n_sub beyond the table, fragments with a proper pair) without raising"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = self.lib.mm2c_pairplan_check(self.handle, C.byref(a), C.byref(b), C.byref(c))
        return rc, a.value, b.value, c.value

    def check(self):
        """waits for the last run(); raises if a fragment was refused (code -2) or an n_sub lay beyond the table (code -3); returns the number of proper pairs"""
        rc, _, _, n = self.counts()
        N.check(rc, "mm2c_pairplan_check")
        return n

    def last_ms(self):
        return self._ms("mm2c_pairplan_last_ms", 1)[0]


def pair_ends_batch(opt, f_off, regs, n, pext, seg_len, gap_ref=None, max_log_arg=1 << 16, fill=None):
    """mm2c_pair_ends_batch_host: host arrays in -> dict(regs REG_DTYPE [f_off[-1] - f_off[0]] (a copy, updated), status int32 [n_frags], rc); the regions of segment
    read r are regs[f_off[r] - f_off[0] :][:n[r]].  rc is 0, -2 (a fragment refused on the device: nothing of it is written but its status) or -3 (an n_sub beyond
    the table): the rest is complete all the same.  Raises for any other failure, an argument refused before the device ran included.  fill: a byte status is
    filled with beforehand (tests)."""
    lib = N.load()
    fo = _i64(f_off)
    rr = np.array(_reg_rows(regs), copy=True)
    nn = np.ascontiguousarray(n, dtype=np.int32); q = np.ascontiguousarray(seg_len, dtype=np.int32)
    px = np.ascontiguousarray(pext, dtype=PEXT_DTYPE).reshape(-1)
    if fo.size % 2 != 1:
        raise ValueError("f_off must hold 2 * n_frags + 1 offsets")
    n_frags = (fo.size - 1) // 2
    g = None if gap_ref is None else np.ascontiguousarray(gap_ref, dtype=np.int32)
    if nn.size != 2 * n_frags or q.size != 2 * n_frags or (g is not None and g.size != n_frags) or not _fit(n_frags, (fo, rr.shape[0])):
        raise ValueError("offsets do not fit the arrays")
    f = 0 if fill is None else int(fill)
    status = np.full(max(n_frags, 1) * 4, f, np.uint8).view(np.int32)
    pp = px if px.size else np.zeros(1, PEXT_DTYPE)
    rp = rr if rr.size else np.zeros((1, REG_DTYPE.itemsize), np.uint8)
    rc = lib.mm2c_pair_ends_batch_host(n_frags, C.byref(opt), int(max_log_arg), _np_ptr(fo), _np_ptr(rp), _np_ptr(nn), px.size, _np_ptr(pp), _np_ptr(q),
                                       None if g is None else _np_ptr(g), _np_ptr(status))
    if rc not in (0, -3) and not (rc == -2 and b"refused, nothing of them written" in (lib.mm2c_last_error() or b"")):
        N.check(rc, "mm2c_pair_ends_batch_host")
    lo = int(fo[0]) if n_frags > 0 else 0
    hi = int(fo[-1]) if n_frags > 0 else 0
    return dict(regs=rr.reshape(-1).view(REG_DTYPE)[lo:hi], status=status[:n_frags], rc=rc)


ERR_DTYPE = np.dtype([("n_match", "<i4"), ("n_tot", "<i4")])                   # mm2c_err_t


class EstErrPlan(_Handle):
    """mm2c_errplan_t: the counts of mm_est_err (map.c:357, esterr.c) on the GPU for batches of up to n_reads reads, n_u_cap final regions, n_b_cap chain anchors
    and n_mini_cap minimizer positions; it stands behind a MapqPlan on the same stream.  The device makes (n_match, n_tot) per region and avg_k per read, which
    are exact by construction; est_err_apply / est_err_div turn them into div with the host's own pow."""

    _destroy = "mm2c_errplan_destroy"

    def __init__(self, n_reads, n_u_cap, n_b_cap, n_mini_cap):
        self.n_reads, self.n_u_cap, self.n_b_cap, self.n_mini_cap = int(n_reads), int(n_u_cap), int(n_b_cap), int(n_mini_cap)
        self._create("mm2c_errplan_create", self.n_reads, self.n_u_cap, self.n_b_cap, self.n_mini_cap)

    def run(self, u_off: torch.Tensor, regs: torch.Tensor, n_in: torch.Tensor, b_off: torch.Tensor, b: torch.Tensor, mini_off: torch.Tensor,
            mini_pos: torch.Tensor, qlen: torch.Tensor, ref_len: torch.Tensor, err: torch.Tensor = None, avg_k: torch.Tensor = None, stream=None):
        """u_off, regs and n_in as MapqPlan.run took and returned them (regs_out / n_out), b_off with that run's b_out (or the epilogue's b when nothing was
        joined), mini_off int64 [n_reads + 1] / mini_pos int64 or uint64 as the reads-in entries return them, qlen int32 per read, ref_len int32 or uint32 per
        reference sequence, all on the GPU.  Returns (err int32 [n_u_cap, 2], avg_k float32 [n_reads]): row u_off[r] + i holds (n_match, n_tot) of region i of
        read r.  Nothing of the input is written.  Asynchronous."""
        for t in (u_off, regs, n_in, b_off, b, mini_off, mini_pos, qlen, ref_len):
            assert t.is_cuda and t.is_contiguous()
        assert u_off.dtype == torch.int64 and b_off.dtype == torch.int64 and mini_off.dtype == torch.int64
        assert u_off.numel() == self.n_reads + 1 and b_off.numel() == self.n_reads + 1 and mini_off.numel() == self.n_reads + 1
        assert regs.numel() * regs.element_size() >= self.n_u_cap * REG_DTYPE.itemsize and b.element_size() == 8 and b.numel() >= 2 * self.n_b_cap
        assert mini_pos.element_size() == 8 and mini_pos.numel() >= self.n_mini_cap and ref_len.element_size() == 4
        assert n_in.dtype == torch.int32 and n_in.numel() >= self.n_reads and qlen.dtype == torch.int32 and qlen.numel() == self.n_reads
        err = _out(err, (max(self.n_u_cap, 1), 2), torch.int32, u_off.device, self.n_u_cap * 8, "dtype")
        avg_k = _out(avg_k, max(self.n_reads, 1), torch.float32, u_off.device, self.n_reads * 4, "dtype")
        st = _stream(stream)
        N.check(self.lib.mm2c_errplan_run_device(self.handle, u_off.data_ptr(), regs.data_ptr(), n_in.data_ptr(), b_off.data_ptr(), b.data_ptr(), mini_off.data_ptr(),
                                                 mini_pos.data_ptr(), qlen.data_ptr(), int(ref_len.numel()), ref_len.data_ptr(), err.data_ptr(), avg_k.data_ptr(), st),
                "mm2c_errplan_run_device")
        return err, avg_k[:self.n_reads]

    def refused(self):
        """waits for the run -> (return code, reads refused) without raising"""
        n = C.c_int64(0)
        rc = self.lib.mm2c_errplan_check(self.handle, C.byref(n))
        return rc, n.value

    def check(self):
        """waits for the run; raises (code -2) if a read was refused for its offsets, its mini_pos or a region"""
        N.check(self.refused()[0], "mm2c_errplan_check")

    def last_ms(self):
        return self._ms("mm2c_errplan_last_ms")[0]

    def last_kernel_ms(self):
        """(err_reads, err_walk, err_finish) of the last run"""
        return self._ms("mm2c_errplan_last_kernel_ms", 3)


def est_err_div(n_match, n_tot, avg_k):
    """mm2c_est_err_div: esterr.c:62 with the host's own pow -> float32; needs no device"""
    return np.float32(N.load().mm2c_est_err_div(int(n_match), int(n_tot), float(np.float32(avg_k))))


def est_err_apply(u_off, n_in, err, avg_k, regs):
    """mm2c_est_err_apply_host: writes div into regs (REG_DTYPE, or uint8 rows of 80, contiguous and writable) in place; rows u_off[r] .. u_off[r] + n_in[r] of
    err and regs belong to read r; a region with n_match == -1 is left alone.  Needs no device."""
    lib = N.load()
    uo = np.ascontiguousarray(u_off, dtype=np.int64); ni = np.ascontiguousarray(n_in, dtype=np.int32)
    ee = np.ascontiguousarray(err).view(np.int32).reshape(-1, 2); ak = np.ascontiguousarray(avg_k, dtype=np.float32)
    assert regs.flags["C_CONTIGUOUS"] and regs.flags["WRITEABLE"]
    rows = regs.size * regs.itemsize // REG_DTYPE.itemsize
    n_reads = ni.size
    if uo.size < n_reads or ak.size < n_reads or (n_reads > 0 and (uo[:n_reads].min() < 0 or (uo[:n_reads] + np.maximum(ni, 0)).max() > min(rows, ee.shape[0]))):
        raise ValueError("offsets do not fit the arrays")
    N.check(lib.mm2c_est_err_apply_host(n_reads, _np_ptr(uo), _np_ptr(ni), _np_ptr(ee), _np_ptr(ak), _np_ptr(regs)), "mm2c_est_err_apply_host")
    return regs


def est_err_batch(u_off, regs, n_in, b_off, b, mini_off, mini_pos, qlen, ref_len):
    """mm2c_est_err_batch_host: host arrays in -> (regs REG_DTYPE [u_off[-1] - u_off[0]], a copy with div written, err ERR_DTYPE of the same length,
    avg_k float32 [n_reads]); the regions of read r are regs[u_off[r] - u_off[0] :][:n_in[r]]"""
    lib = N.load()
    uo = _i64(u_off); bo = _i64(b_off)
    mo = _i64(mini_off)
    rr = np.array(_reg_rows(regs))
    bb = _anchor_rows(b); mp = np.ascontiguousarray(mini_pos, dtype=np.uint64).reshape(-1)
    ni = np.ascontiguousarray(n_in, dtype=np.int32); q = np.ascontiguousarray(qlen, dtype=np.int32); rl = np.ascontiguousarray(ref_len, dtype=np.uint32)
    n_reads = uo.size - 1
    if bo.size != uo.size or mo.size != uo.size or ni.size != n_reads or q.size != n_reads or \
            not _fit(n_reads, (uo, rr.shape[0]), (bo, bb.shape[0]), (mo, mp.size)):
        raise ValueError("offsets do not fit the arrays")
    n_u = int(uo[-1] - uo[0]) if n_reads > 0 else 0
    err = np.zeros(max(n_u, 1), ERR_DTYPE)
    avg_k = np.zeros(max(n_reads, 1), np.float32)
    N.check(lib.mm2c_est_err_batch_host(n_reads, _np_ptr(uo), _np_ptr(rr), _np_ptr(ni), _np_ptr(bo), _np_ptr(bb), _np_ptr(mo), _np_ptr(mp), _np_ptr(q),
                                        int(rl.size), _np_ptr(rl), _np_ptr(err), _np_ptr(avg_k)), "mm2c_est_err_batch_host")
    lo = int(uo[0]) if n_reads > 0 else 0
    return rr[lo:lo + n_u].reshape(-1).view(REG_DTYPE), err[:n_u], avg_k[:n_reads]


MATCH_DTYPE = np.dtype([("cr_off", "<i8"), ("n", "<u4"), ("q_pos", "<u4"), ("q_span", "<u4"), ("seg_tandem", "<u4")])   # mm2c_match_t


class SeedPlan(_Handle):
    """mm2c_seedplan_t: seed hits -> sorted anchors on the GPU (collect_seed_hits, map.c:215-247) for a batch of reads"""

    _destroy = "mm2c_seedplan_destroy"

    def __init__(self, match_off, anchor_off):
        mo = _i64(match_off); ao = _i64(anchor_off)
        assert mo.size == ao.size
        self.n_reads, self.total = mo.size - 1, int(ao[-1] - ao[0])
        self._create("mm2c_seedplan_create", self.n_reads, _np_ptr(mo), _np_ptr(ao))

    def run(self, matches: torch.Tensor, hits: torch.Tensor, qlen: torch.Tensor, anchors: torch.Tensor = None, stream=None):
        """matches: uint8 view of mm2c_match_t records on the GPU; hits: int64 pool; qlen: int32 [n_reads]; returns anchors int64 [total, 2]"""
        assert matches.is_cuda and hits.is_cuda and qlen.is_cuda and qlen.dtype == torch.int32 and qlen.numel() == self.n_reads
        if anchors is None:
            anchors = torch.empty((max(self.total, 1), 2), dtype=torch.int64, device=hits.device)
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.numel() >= 2 * self.total
        st = _stream(stream)
        N.check(self.lib.mm2c_seedplan_run_device_n(self.handle, matches.data_ptr(), matches.numel() * matches.element_size() // 24, hits.data_ptr(),
                                                    hits.numel(), qlen.data_ptr(), qlen.numel(), anchors.data_ptr(), anchors.numel() // 2, st),
                "mm2c_seedplan_run_device_n")
        return anchors

    def run_skip(self, matches, hits, qlen, flag, ref_rank, ref_len, q_lo, q_eq, anchors=None, stream=None):
        """collect_seed_hits with skip_seed (map.c:122-147; -x ava-ont: flag = NO_DIAG | NO_DUAL): the reads keep fewer anchors than they have
        hits.  ref_rank / ref_len: int32 per reference sequence, q_lo / q_eq: int32 per read (device tensors; names as ranks, mm2chain.h).
        Returns (anchors int64 [capacity, 2] packed, offsets int64 [n_reads + 1] on the device)."""
        assert matches.is_cuda and hits.is_cuda and qlen.is_cuda and qlen.dtype == torch.int32 and qlen.numel() == self.n_reads
        for t in (ref_rank, ref_len, q_lo, q_eq):
            assert t is None or (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous())
        if anchors is None:
            anchors = torch.empty((max(self.total, 1), 2), dtype=torch.int64, device=hits.device)
        off = torch.empty(self.n_reads + 1, dtype=torch.int64, device=hits.device)
        sk = N.SeedSkip(int(flag), ref_rank.data_ptr() if ref_rank is not None else None, ref_len.data_ptr() if ref_len is not None else None,
                        q_lo.data_ptr() if q_lo is not None else None, q_eq.data_ptr() if q_eq is not None else None)
        st = _stream(stream)
        N.check(self.lib.mm2c_seedplan_run_device_skip(self.handle, matches.data_ptr(), matches.numel() * matches.element_size() // 24, hits.data_ptr(),
                                                       hits.numel(), qlen.data_ptr(), qlen.numel(), C.byref(sk), anchors.data_ptr(),
                                                       anchors.numel() // 2, off.data_ptr(), st), "mm2c_seedplan_run_device_skip")
        return anchors, off

    def set_heap_sort(self, on=True):
        """MM_F_HEAP_SORT (--heap-sort, -x sr): later runs leave the order of collect_seed_hits_heap (map.c:149-213) among anchors with equal x"""
        N.check(self.lib.mm2c_seedplan_set_heap_sort(self.handle, 1 if on else 0), "mm2c_seedplan_set_heap_sort")

    def check(self):
        """waits for the run; raises if a read's hit counts did not add up to its anchor range; returns the number of reads with equal x"""
        n = C.c_int64(0)
        N.check(self.lib.mm2c_seedplan_check(self.handle, C.byref(n)), "mm2c_seedplan_check")
        return n.value

    def last_ms(self):
        return self._ms("mm2c_seedplan_last_ms")[0]

    def last_expand_mw(self):
        """the reads the last run expanded on sixteen waves (mm2c_seedplan_last_expand_mw)"""
        n = C.c_int64(0)
        N.check(self.lib.mm2c_seedplan_last_expand_mw(self.handle, C.byref(n)), "mm2c_seedplan_last_expand_mw")
        return int(n.value)


def seed_hits_batch(match_off, matches, hits, qlen):
    """mm2c_seed_hits_batch_host: returns (anchor_off int64 [n_reads+1], anchors uint64 [total, 2])"""
    lib = N.load()
    mo = _i64(match_off)
    m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
    h = np.ascontiguousarray(hits, dtype=np.uint64)
    q = np.ascontiguousarray(qlen, dtype=np.int32)
    n_reads = mo.size - 1
    if q.size != n_reads or mo[-1] > m.size or mo[0] < 0:
        raise ValueError("offsets do not fit the arrays")
    ao = np.zeros(n_reads + 1, np.int64)
    a = np.zeros((max(int(m["n"][mo[0]:mo[-1]].sum()), 1), 2), np.uint64)
    N.check(lib.mm2c_seed_hits_batch_host(n_reads, _np_ptr(mo), _np_ptr(m), _np_ptr(h), h.size, _np_ptr(q), _np_ptr(ao), _np_ptr(a)),
            "mm2c_seed_hits_batch_host")
    return ao, a[:ao[-1]]


def seed_chain_batch(params: Params, min_cnt, min_sc, match_off, matches, hits, qlen):
    """mm2c_seed_chain_batch_host: matches in, per-read chains out [(u, b), ...] (anchors never leave the GPU)"""
    lib = N.load()
    mo = _i64(match_off)
    m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
    h = np.ascontiguousarray(hits, dtype=np.uint64)
    q = np.ascontiguousarray(qlen, dtype=np.int32)
    n_reads = mo.size - 1
    if q.size != n_reads or mo[-1] > m.size or mo[0] < 0:
        raise ValueError("offsets do not fit the arrays")
    total = max(int(m["n"][mo[0]:mo[-1]].sum()), 1)
    ao = np.zeros(n_reads + 1, np.int64); u_off = np.zeros(n_reads + 1, np.int64); b_off = np.zeros(n_reads + 1, np.int64)
    u = np.zeros(total, np.uint64); b = np.zeros((total, 2), np.uint64)
    N.check(lib.mm2c_seed_chain_batch_host(C.byref(params), min_cnt, min_sc, n_reads, _np_ptr(mo), _np_ptr(m), _np_ptr(h), h.size, _np_ptr(q),
                                           _np_ptr(ao), _np_ptr(u_off), _np_ptr(u), _np_ptr(b_off), _np_ptr(b)), "mm2c_seed_chain_batch_host")
    return _split_chains(n_reads, u_off, u, b_off, b)


class SeedSkip:
    """skip_seed (map.c:122-147) for the host-buffer entries (mm2c_seed_skip_host_t).  flag: NO_DIAG | NO_DUAL (-x ava-ont), FOR_ONLY, REV_ONLY.  Names as ranks
    (include/mm2chain.h): ref_rank / ref_len per reference sequence, q_lo / q_eq per read; ref_rank None: no name comparison (qname == NULL, map.c:125)."""
    NO_DIAG, NO_DUAL, FOR_ONLY, REV_ONLY = 0x001, 0x002, 0x100000, 0x200000      # minimap.h:8-9,28-29

    def __init__(self, flag, ref_rank=None, ref_len=None, q_lo=None, q_eq=None):
        as_i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.int32)).reshape(-1)
        self.flag = int(flag)
        self.ref_rank, self.ref_len, self.q_lo, self.q_eq = as_i32(ref_rank), as_i32(ref_len), as_i32(q_lo), as_i32(q_eq)
        if self.flag & ~(self.NO_DIAG | self.NO_DUAL | self.FOR_ONLY | self.REV_ONLY):
            raise ValueError(f"skip flag {self.flag:#x} has bits other than NO_DIAG, NO_DUAL, FOR_ONLY, REV_ONLY")
        if self.ref_rank is None:
            if self.ref_len is not None:
                raise ValueError("ref_len without ref_rank")
            return
        if self.ref_len is not None and self.ref_len.size != self.ref_rank.size:
            raise ValueError(f"ref_len has {self.ref_len.size} entries, ref_rank {self.ref_rank.size}")
        if (self.q_lo is None) != (self.q_eq is None) or (self.q_lo is not None and self.q_lo.size != self.q_eq.size):
            raise ValueError("q_lo and q_eq go together, one entry per read each")
        if self.flag & (self.NO_DIAG | self.NO_DUAL) and (self.ref_len is None or self.q_lo is None):
            raise ValueError("NO_DIAG / NO_DUAL with ref_rank need ref_len, q_lo and q_eq")

    def _native(self, n_reads):
        """the C struct for a batch of n_reads reads (checks the per-read lengths; the arrays must outlive the call)"""
        if self.q_lo is not None and self.q_lo.size != n_reads:
            raise ValueError(f"q_lo / q_eq have {self.q_lo.size} entries for {n_reads} reads")
        p = lambda a: None if a is None else a.ctypes.data
        return N.SeedSkipHost(self.flag, 0 if self.ref_rank is None else self.ref_rank.size, p(self.ref_rank), p(self.ref_len), p(self.q_lo), p(self.q_eq))


def _seed_args(match_off, matches, qlen):
    mo = _i64(match_off)
    m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
    q = np.ascontiguousarray(qlen, dtype=np.int32)
    n_reads = mo.size - 1
    if q.size != n_reads or mo[-1] > m.size or mo[0] < 0:
        raise ValueError("offsets do not fit the arrays")
    return mo, m, q, n_reads, max(int(m["n"][mo[0]:mo[-1]].sum()), 1)


def seed_hits_batch_skip(match_off, matches, hits, qlen, skip: SeedSkip):
    """mm2c_seed_hits_batch_host_skip: collect_seed_hits with skip_seed.  Returns (anchor_off int64 [n_reads+1] of the KEPT anchors, anchors uint64 [kept, 2])"""
    mo, m, q, n_reads, cap = _seed_args(match_off, matches, qlen)
    sk = skip._native(n_reads)
    h = np.ascontiguousarray(hits, dtype=np.uint64)
    ao = np.zeros(n_reads + 1, np.int64)
    a = np.zeros((cap, 2), np.uint64)
    N.check(N.load().mm2c_seed_hits_batch_host_skip(n_reads, _np_ptr(mo), _np_ptr(m), _np_ptr(h), h.size, _np_ptr(q), C.byref(sk), _np_ptr(ao), _np_ptr(a)),
            "mm2c_seed_hits_batch_host_skip")
    return ao, a[:ao[-1]]


def seed_chain_batch_skip(params: Params, min_cnt, min_sc, match_off, matches, hits, qlen, skip: SeedSkip):
    """mm2c_seed_chain_batch_host_skip: seed_chain_batch with skip_seed.  Returns (anchor_off of the kept anchors, [(u, b), ...])"""
    mo, m, q, n_reads, cap = _seed_args(match_off, matches, qlen)
    sk = skip._native(n_reads)
    h = np.ascontiguousarray(hits, dtype=np.uint64)
    ao = np.zeros(n_reads + 1, np.int64); u_off = np.zeros(n_reads + 1, np.int64); b_off = np.zeros(n_reads + 1, np.int64)
    u = np.zeros(cap, np.uint64); b = np.zeros((cap, 2), np.uint64)
    N.check(N.load().mm2c_seed_chain_batch_host_skip(C.byref(params), min_cnt, min_sc, n_reads, _np_ptr(mo), _np_ptr(m), _np_ptr(h), h.size, _np_ptr(q), C.byref(sk),
                                                     _np_ptr(ao), _np_ptr(u_off), _np_ptr(u), _np_ptr(b_off), _np_ptr(b)), "mm2c_seed_chain_batch_host_skip")
    return ao, _split_chains(n_reads, u_off, u, b_off, b)


class HitPool(_Handle):
    """mm2c_hitpool_t: the index's position arrays resident in HBM (uploaded once per index)"""

    _destroy = "mm2c_hitpool_destroy"

    def __init__(self, hits):
        h = np.ascontiguousarray(hits, dtype=np.uint64)
        self._create("mm2c_hitpool_create", _np_ptr(h), h.size, code=-4)
        self.size = h.size

    _owned = True

    @classmethod
    def _view(cls, handle, size):
        """a pool that belongs to something else (the pool of MinimizerIndex.build): never destroyed from here"""
        self = cls.__new__(cls)
        self.lib, self.handle, self.size, self._owned = N.load(), handle, int(size), False
        return self

    def close(self):
        if not self._owned:
            self.handle = None
        super().close()


def seed_chain_batch_pool(params: Params, min_cnt, min_sc, match_off, matches, pool: HitPool, qlen):
    """mm2c_seed_chain_batch_pool: as seed_chain_batch with the hits taken from a resident pool (cr_off points into it)"""
    lib = N.load()
    mo = _i64(match_off)
    m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
    q = np.ascontiguousarray(qlen, dtype=np.int32)
    n_reads = mo.size - 1
    if q.size != n_reads or mo[-1] > m.size or mo[0] < 0:
        raise ValueError("offsets do not fit the arrays")
    total = max(int(m["n"][mo[0]:mo[-1]].sum()), 1)
    ao = np.zeros(n_reads + 1, np.int64); u_off = np.zeros(n_reads + 1, np.int64); b_off = np.zeros(n_reads + 1, np.int64)
    u = np.zeros(total, np.uint64); b = np.zeros((total, 2), np.uint64)
    N.check(lib.mm2c_seed_chain_batch_pool(C.byref(params), min_cnt, min_sc, n_reads, _np_ptr(mo), _np_ptr(m), pool.handle, _np_ptr(q),
                                           _np_ptr(ao), _np_ptr(u_off), _np_ptr(u), _np_ptr(b_off), _np_ptr(b)), "mm2c_seed_chain_batch_pool")
    return _split_chains(n_reads, u_off, u, b_off, b)


def seed_chain_batch_pool_skip(params: Params, min_cnt, min_sc, match_off, matches, pool: HitPool, qlen, skip: SeedSkip):
    """mm2c_seed_chain_batch_pool_skip: seed_chain_batch_skip with the hits taken from a resident pool"""
    mo, m, q, n_reads, cap = _seed_args(match_off, matches, qlen)
    sk = skip._native(n_reads)
    ao = np.zeros(n_reads + 1, np.int64); u_off = np.zeros(n_reads + 1, np.int64); b_off = np.zeros(n_reads + 1, np.int64)
    u = np.zeros(cap, np.uint64); b = np.zeros((cap, 2), np.uint64)
    N.check(N.load().mm2c_seed_chain_batch_pool_skip(C.byref(params), min_cnt, min_sc, n_reads, _np_ptr(mo), _np_ptr(m), pool.handle, _np_ptr(q), C.byref(sk),
                                                     _np_ptr(ao), _np_ptr(u_off), _np_ptr(u), _np_ptr(b_off), _np_ptr(b)), "mm2c_seed_chain_batch_pool_skip")
    return ao, _split_chains(n_reads, u_off, u, b_off, b)


def _reads_args(seqs):
    """reads as (seq_off int64 [n+1], seq uint8): a list of bytes / str / uint8 arrays, or such a pair already"""
    if isinstance(seqs, tuple) and len(seqs) == 2:
        off = np.ascontiguousarray(np.asarray(seqs[0], dtype=np.int64))
        seq = np.ascontiguousarray(np.asarray(seqs[1], dtype=np.uint8)).reshape(-1)
    else:
        parts = [np.frombuffer(x.encode() if isinstance(x, str) else bytes(x), dtype=np.uint8) for x in seqs]
        off = np.zeros(len(parts) + 1, np.int64)
        off[1:] = np.cumsum([p.size for p in parts]) if parts else []
        seq = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if off.size < 1 or off[0] != 0 or off[-1] > seq.size:
        raise ValueError("sequence offsets do not fit the bases")
    return off, np.ascontiguousarray(seq) if seq.size else np.zeros(1, np.uint8)


def _arr(ptr, n, dtype):
    """copy n elements of a library-owned array"""
    dt = np.dtype(dtype)
    if n == 0 or not ptr:
        return np.zeros(n, dt)
    return np.frombuffer(C.string_at(ptr, n * dt.itemsize), dtype=dt).copy()


class _Result:
    """mm2c_read_result_t, kept for the reads-in calls of one object"""

    def __init__(self):
        self.lib = N.load()
        self.p = self.lib.mm2c_read_result_create()

    def __del__(self):
        try:
            self.lib.mm2c_read_result_free(self.p)
        except Exception:
            pass


class MinimizerIndex(_Handle):
    """mm2c_minidx_t: a minimizer index resident on every configured device.  keys = minimizers (x >> 8), their hits pool[cr_off : cr_off + n] of a HitPool
    (or of `hits`, uploaded as a pool owned by the index).  Lookups return what mm_idx_get returns (n = 0 for an absent key)."""

    _destroy = "mm2c_minidx_destroy"

    def __init__(self, k, w, is_hpc, keys, cr_off, n, pool: "HitPool" = None, hits=None):
        self.lib = N.load()
        if pool is None:
            if hits is None:
                raise ValueError("give a HitPool or the hits")
            pool = HitPool(hits)
        self.pool, self.k, self.w, self.is_hpc = pool, int(k), int(w), int(bool(is_hpc))
        kk = np.ascontiguousarray(keys, dtype=np.uint64)
        cr = np.ascontiguousarray(cr_off, dtype=np.int64)
        nn = np.ascontiguousarray(n, dtype=np.uint32)
        if not (kk.size == cr.size == nn.size):
            raise ValueError("keys, cr_off and n differ in length")
        self._create("mm2c_minidx_create", pool.handle, self.k, self.w, self.is_hpc, kk.size, _np_ptr(kk), _np_ptr(cr), _np_ptr(nn), code=-2)
        self.size = kk.size

    @classmethod
    def build(cls, seqs, k, w, is_hpc=False, mid_occ_frac=2e-4):
        """mm2c_minidx_build: the index of `seqs` (a list of bytes / str / uint8 arrays, or (seq_off, seq)) made on the device, as mm_idx_gen makes it.
        The index owns its pool: .pool is a view that does not free it.  .mid_occ = mm_idx_cal_max_occ(mid_occ_frac)"""
        off, seq = _reads_args(seqs)
        self = cls.__new__(cls)
        self.lib = N.load()
        self.k, self.w, self.is_hpc = int(k), int(w), int(bool(is_hpc))
        occ = C.c_int(0)
        self.handle = self.lib.mm2c_minidx_build(self.k, self.w, self.is_hpc, off.size - 1, _np_ptr(off), _np_ptr(seq), float(mid_occ_frac), C.byref(occ))
        if not self.handle:
            msg = (self.lib.mm2c_last_error() or b"").decode()
            code = {"MM2C_E_NODEVICE": -1, "MM2C_E_ARG": -2, "MM2C_E_TOOBIG": -3}.get(msg.split(":")[0], -4)
            N.check(code, "mm2c_minidx_build")
        self.mid_occ = int(occ.value)
        self.size = self.n_keys
        self.pool = HitPool._view(self.lib.mm2c_minidx_pool(self.handle), self.n_hits)
        return self

    @property
    def n_keys(self):
        return int(self.lib.mm2c_minidx_n_keys(self.handle))

    @property
    def n_hits(self):
        return int(self.lib.mm2c_minidx_n_hits(self.handle))

    def cal_max_occ(self, frac=2e-4):
        """mm_idx_cal_max_occ on the device"""
        occ = self.lib.mm2c_minidx_cal_max_occ(self.handle, float(frac))
        if occ < 0:
            N.check(occ, "mm2c_minidx_cal_max_occ")
        return int(occ)

    def export(self):
        """(keys uint64, cr_off int64, n uint32, pool uint64) downloaded; pool is empty for an index made over a caller's HitPool"""
        nk = self.n_keys
        built = not self.pool._owned
        keys = np.zeros(nk, np.uint64); cr = np.zeros(nk, np.int64); n = np.zeros(nk, np.uint32)
        pool = np.zeros(self.n_hits if built else 0, np.uint64)
        N.check(self.lib.mm2c_minidx_export(self.handle, _np_ptr(keys), _np_ptr(cr), _np_ptr(n), _np_ptr(pool) if pool.size else None), "mm2c_minidx_export")
        return keys, cr, n, pool

    def lookup(self, keys):
        """(cr_off int64, n uint32) per key"""
        q = np.ascontiguousarray(keys, dtype=np.uint64)
        cr = np.zeros(q.size, np.int64); n = np.zeros(q.size, np.uint32)
        N.check(self.lib.mm2c_minidx_lookup(self.handle, q.size, _np_ptr(q), _np_ptr(cr), _np_ptr(n)), "mm2c_minidx_lookup")
        return cr, n

    def close(self):
        if self.handle and not self.pool._owned:        # a built index takes its pool with it
            self.pool.handle = None
        super().close()


# what the reads-in entries return, from their result r = mm2c_read_result_t over n reads or fragments (a read is a fragment of one segment)
def _sketch_out(r, n):
    return _arr(r.sketch_off, n + 1, np.int64), _arr(r.sketch, 2 * r.n_sketch, np.uint64).reshape(-1, 2)


def _match_dict(r, n):
    return {"match_off": _arr(r.match_off, n + 1, np.int64), "matches": _arr(r.matches, r.n_matches, MATCH_DTYPE),
            "anchor_off": _arr(r.anchor_off, n + 1, np.int64), "rep_len": _arr(r.rep_len, n, np.int32),
            "mini_off": _arr(r.mini_off, n + 1, np.int64), "mini_pos": _arr(r.mini_pos, r.n_mini_pos, np.uint64)}


def sketch_batch(seqs, k, w, is_hpc=False):
    """mm2c_sketch_batch: mm_sketch per read.  seqs: list of reads (bytes / str) or (seq_off, seq).  Returns (off int64 [n+1], minimizers uint64 [m, 2] = x, y)"""
    off, seq = _reads_args(seqs)
    R = _Result()
    N.check(R.lib.mm2c_sketch_batch(int(k), int(w), int(bool(is_hpc)), off.size - 1, _np_ptr(off), _np_ptr(seq), R.p), "mm2c_sketch_batch")
    return _sketch_out(R.p.contents, off.size - 1)


def sketch_match_batch(seqs, idx: MinimizerIndex, mid_occ):
    """mm2c_sketch_match_batch: reads in, matches out.  Returns a dict of numpy arrays: match_off, matches (MATCH_DTYPE), anchor_off, rep_len, mini_off, mini_pos"""
    off, seq = _reads_args(seqs)
    R = _Result()
    N.check(R.lib.mm2c_sketch_match_batch(idx.handle, int(mid_occ), off.size - 1, _np_ptr(off), _np_ptr(seq), R.p), "mm2c_sketch_match_batch")
    return _match_dict(R.p.contents, off.size - 1)


def read_chain_batch(params: Params, min_cnt, min_sc, seqs, idx: MinimizerIndex, mid_occ, skip: SeedSkip = None):
    """mm2c_read_chain_batch: reads in, chains out (sketch, lookups, seed hits, DP and epilogue on the device).  Returns a dict: anchor_off, u_off, u, b_off,
    b (uint64 [n_b, 2]), rep_len, mini_off, mini_pos, and chains = [(u, b), ...] per read"""
    off, seq = _reads_args(seqs)
    nr = off.size - 1
    sk = skip._native(nr) if skip is not None else None
    R = _Result()
    N.check(R.lib.mm2c_read_chain_batch(C.byref(params), int(min_cnt), int(min_sc), idx.handle, int(mid_occ), nr, _np_ptr(off), _np_ptr(seq),
                                        C.byref(sk) if sk is not None else None, R.p), "mm2c_read_chain_batch")
    r = R.p.contents
    out = {"anchor_off": _arr(r.anchor_off, nr + 1, np.int64), "u_off": _arr(r.u_off, nr + 1, np.int64), "u": _arr(r.u, r.n_u, np.uint64),
           "b_off": _arr(r.b_off, nr + 1, np.int64), "b": _arr(r.b, 2 * r.n_b, np.uint64).reshape(-1, 2), "rep_len": _arr(r.rep_len, nr, np.int32),
           "mini_off": _arr(r.mini_off, nr + 1, np.int64), "mini_pos": _arr(r.mini_pos, r.n_mini_pos, np.uint64)}
    out["chains"] = _split_chains(nr, out["u_off"], out["u"], out["b_off"], out["b"])
    return out


def _frags_args(frags):
    """fragments as (frag_off int64 [n_frags+1], seq_off, seq): a list of fragments, each a list of segments (bytes / str / uint8 arrays), or (frag_off, seq_off, seq)"""
    def offsets(x):
        """a 1-D array of integers, which no fragment (a list of segments) is"""
        if isinstance(x, (bytes, str)):
            return False
        try:
            a = np.asarray(x)
        except ValueError:                                     # segments of different lengths
            return False
        return a.ndim == 1 and a.dtype.kind in "iu" and a.dtype != np.uint8
    if isinstance(frags, tuple) and len(frags) == 3 and offsets(frags[0]) and offsets(frags[1]):
        off, seq = _reads_args((frags[1], frags[2]))
        return np.ascontiguousarray(np.asarray(frags[0], dtype=np.int64)), off, seq
    fo = np.zeros(len(frags) + 1, np.int64)
    fo[1:] = np.cumsum([len(f) for f in frags]) if len(frags) else []
    off, seq = _reads_args([s for f in frags for s in f])
    return fo, off, seq


def sketch_frag_batch(frags, k, w, is_hpc=False):
    """mm2c_sketch_frag_batch: collect_minimizers per fragment (segment ids in y's high word, positions shifted by the earlier segments' lengths).
    Returns (off int64 [n_frags+1], minimizers uint64 [m, 2])"""
    fo, off, seq = _frags_args(frags)
    R = _Result()
    N.check(R.lib.mm2c_sketch_frag_batch(int(k), int(w), int(bool(is_hpc)), fo.size - 1, _np_ptr(fo), off.size - 1, _np_ptr(off), _np_ptr(seq), R.p),
            "mm2c_sketch_frag_batch")
    return _sketch_out(R.p.contents, fo.size - 1)


def sketch_match_frag_batch(frags, idx: MinimizerIndex, occ):
    """mm2c_sketch_match_frag_batch: fragments in, matches out; the dict of sketch_match_batch, per fragment"""
    fo, off, seq = _frags_args(frags)
    R = _Result()
    N.check(R.lib.mm2c_sketch_match_frag_batch(idx.handle, int(occ), fo.size - 1, _np_ptr(fo), off.size - 1, _np_ptr(off), _np_ptr(seq), R.p),
            "mm2c_sketch_match_frag_batch")
    return _match_dict(R.p.contents, fo.size - 1)


def frag_gaps(is_sr=1, max_gap=100, max_gap_ref=-1, max_frag_len=800):
    """mm2c_frag_gaps_t; the defaults are the option values of -x sr (options.c)"""
    return N.FragGaps(int(is_sr), int(max_gap), int(max_gap_ref), int(max_frag_len))


def _result_task_dists(R, nf):
    """mm2c_read_result_task_dists: the (max_dist_x, max_dist_y) the call chained every fragment with, int32 [n_frags, 2] (a copy)"""
    ptr, n = C.c_void_p(), C.c_int64()
    N.check(R.lib.mm2c_read_result_task_dists(R.p, C.byref(ptr), C.byref(n)), "mm2c_read_result_task_dists")
    assert n.value == nf
    return _arr(ptr.value, 2 * nf, np.int32).reshape(-1, 2)


def frag_chain_batch(params: Params, min_cnt, min_sc, frags, idx: MinimizerIndex, mid_occ, max_occ, skip: SeedSkip = None, gaps=None):
    """mm2c_frag_chain_batch: fragments of params.n_segs segments in, chains out, with the max_occ re-chain of map.c:318-340.  Returns the dict of
    read_chain_batch per fragment, plus rechained (uint8 per fragment) and n_rechained.
    gaps (frag_gaps(...)): mm2c_frag_chain_batch_gaps -- params.max_dist_x / max_dist_y are ignored, every fragment is chained with the pair map.c:305-314
    gives for its total length; the dict then also holds task_dists, int32 [n_frags, 2] of (max_dist_x, max_dist_y) as the device made them"""
    fo, off, seq = _frags_args(frags)
    nf = fo.size - 1
    sk = skip._native(nf) if skip is not None else None
    R = _Result()
    if gaps is not None:
        N.check(R.lib.mm2c_frag_chain_batch_gaps(C.byref(params), int(min_cnt), int(min_sc), idx.handle, int(mid_occ), int(max_occ), C.byref(gaps), nf, _np_ptr(fo),
                                                 off.size - 1, _np_ptr(off), _np_ptr(seq), C.byref(sk) if sk is not None else None, R.p), "mm2c_frag_chain_batch_gaps")
    else:
        N.check(R.lib.mm2c_frag_chain_batch(C.byref(params), int(min_cnt), int(min_sc), idx.handle, int(mid_occ), int(max_occ), nf, _np_ptr(fo), off.size - 1,
                                            _np_ptr(off), _np_ptr(seq), C.byref(sk) if sk is not None else None, R.p), "mm2c_frag_chain_batch")
    r = R.p.contents
    out = {"anchor_off": _arr(r.anchor_off, nf + 1, np.int64), "u_off": _arr(r.u_off, nf + 1, np.int64), "u": _arr(r.u, r.n_u, np.uint64),
           "b_off": _arr(r.b_off, nf + 1, np.int64), "b": _arr(r.b, 2 * r.n_b, np.uint64).reshape(-1, 2), "rep_len": _arr(r.rep_len, nf, np.int32),
           "mini_off": _arr(r.mini_off, nf + 1, np.int64), "mini_pos": _arr(r.mini_pos, r.n_mini_pos, np.uint64),
           "rechained": _arr(r.rechained, nf, np.uint8), "n_rechained": int(r.n_rechained)}
    if gaps is not None:
        out["task_dists"] = _result_task_dists(R, nf)
    out["chains"] = _split_chains(nf, out["u_off"], out["u"], out["b_off"], out["b"])
    return out


def frag_chain_batch_gaps(params: Params, min_cnt, min_sc, frags, idx: MinimizerIndex, mid_occ, max_occ, gaps, skip: SeedSkip = None):
    """mm2c_frag_chain_batch_gaps: frag_chain_batch with per-fragment chaining distances (gaps: frag_gaps(...), required)"""
    if gaps is None:
        raise N.Mm2cError("mm2c_frag_chain_batch_gaps: gaps is None (frag_chain_batch takes the distances from params)")
    return frag_chain_batch(params, min_cnt, min_sc, frags, idx, mid_occ, max_occ, skip, gaps)


def frag_stats(reset=False):
    """mm2c_get_frag_stats as a dict (ns and counts); reset=True clears the counters afterwards"""
    lib = N.load()
    st = N.FragStats()
    lib.mm2c_get_frag_stats(C.byref(st))
    if reset:
        lib.mm2c_reset_frag_stats()
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def sketch_stats(reset=False):
    """mm2c_get_sketch_stats as a dict (ns and counts); reset=True clears the counters afterwards"""
    lib = N.load()
    st = N.SketchStats()
    lib.mm2c_get_sketch_stats(C.byref(st))
    if reset:
        lib.mm2c_reset_sketch_stats()
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def index_stats(reset=False):
    """mm2c_get_index_stats as a dict (ns and counts); reset=True clears the counters afterwards"""
    lib = N.load()
    st = N.IndexStats()
    lib.mm2c_get_index_stats(C.byref(st))
    if reset:
        lib.mm2c_reset_index_stats()
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def stage_stats(reset=False):
    """mm2c_get_stage_stats as a dict (ns and counts); reset=True clears the counters afterwards"""
    lib = N.load()
    st = N.StageStats()
    lib.mm2c_get_stage_stats(C.byref(st))
    if reset:
        lib.mm2c_reset_stage_stats()
    return {k: int(getattr(st, k)) for k, _ in st._fields_}


def hardware_init(buf_size=0, binary_name=b""):
    """the reference symbol bool hardware_init(long, char*) (chain_hardware.h:70)"""
    return bool(getattr(N.load(), "_Z13hardware_initlPc")(buf_size, binary_name))


def cleanup():
    """the reference symbol void cleanup() (chain_hardware.h:71)"""
    getattr(N.load(), "_Z7cleanupv")()


def run_chaining_on_hw(n, max_dist_x, max_dist_y, bw, q_span, avg_qspan, anchors, num_subparts=None, total_subparts=0, tid=0,
                       hw_time_pred=0.0, sw_time_pred=0.0):
    """the reference symbol (chain_hardware.h:68), same argument order; returns (ret, f, p)"""
    a = np.ascontiguousarray(anchors).view(np.uint64).reshape(-1, 2)
    f = np.empty(n, dtype=np.int32)
    p = np.empty(n, dtype=np.int32)
    ns = _np_ptr(np.ascontiguousarray(num_subparts, dtype=np.uint8)) if num_subparts is not None else None
    ret = getattr(N.load(), "_Z18run_chaining_on_hwliiiifP7mm128_tPiS1_Phliff")(
        n, max_dist_x, max_dist_y, bw, q_span, avg_qspan, _np_ptr(a), _np_ptr(f), _np_ptr(p), ns, total_subparts, tid,
        hw_time_pred, sw_time_pred)
    return ret, f, p


def mm_chain_dp(max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, gap_scale, is_cdna, n_segs, anchors, tid=0):
    """mm_chain_dp (mmpriv.h:65) through the library's host mirror.  km = NULL (malloc arena, as kalloc.c does).
    Returns (u uint64 [n_u], b uint64 [sum cnt, 2])."""
    lib = N.load()
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    a = np.ascontiguousarray(anchors).view(np.uint64).reshape(-1, 2)
    n = a.shape[0]
    a_own = libc.malloc(max(n, 1) * 16)       # mm_chain_dp frees its input (chain.c:39,421)
    C.memmove(a_own, a.ctypes.data, n * 16)
    n_u = C.c_int(0)
    u = C.c_void_p(0)
    b = lib.mm_chain_dp(max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, gap_scale, is_cdna, n_segs,
                        n, a_own if n else None, C.byref(n_u), C.byref(u), None, tid)
    if n == 0:
        libc.free(a_own)
    if not b or n_u.value == 0:
        if b:
            libc.free(b)
        if u.value:
            libc.free(u)
        return np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64)
    u_np = np.ctypeslib.as_array(C.cast(u, C.POINTER(C.c_uint64)), shape=(n_u.value,)).copy()
    nb = int((u_np & 0xFFFFFFFF).sum())
    b_np = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_uint64)), shape=(nb, 2)).copy()
    libc.free(b)
    libc.free(u)
    return u_np, b_np
