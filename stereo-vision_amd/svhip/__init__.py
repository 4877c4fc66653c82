"""ctypes binding of libsvhip.so (C-ABI: include/svh.h).

Python is plumbing here: the product is the shared library (HIP kernels for
gfx950 + C++ host engine).  This module mirrors the reference's class surface
(`Elas(parameters).process(I1, I2, D1, D2, dims)`, libelas/src/elas.h:151-165) so
parity tests read like reference call sites.  There is NO CPU fallback: a
missing library or a missing GPU raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVH_LIB: another build of the library (A/B measurements of kernel changes)
LIB_PATH = os.environ.get("SVH_LIB") or os.path.join(os.path.dirname(_HERE), "libsvhip.so")

OK, ERR_FEW_SUPPORT, ERR_BAD_ARG, ERR_HIP, ERR_UNSUPPORTED, ERR_NO_DEVICE = 0, 1, -1, -2, -3, -4
ERR_BAD_DIMS = -7    # Matcher::pushBack / prefetch with bad dimensions (the reference's message, call ignored)
ROBOTICS, MIDDLEBURY = 0, 1


class ElasParams(C.Structure):
    """svh_elas_params == Elas::parameters (libelas/src/elas.h:59-148)."""
    _fields_ = [
        ("disp_min", C.c_int32), ("disp_max", C.c_int32),
        ("support_threshold", C.c_float), ("support_texture", C.c_int32),
        ("candidate_stepsize", C.c_int32), ("incon_window_size", C.c_int32),
        ("incon_threshold", C.c_int32), ("incon_min_support", C.c_int32),
        ("add_corners", C.c_int32), ("grid_size", C.c_int32),
        ("beta", C.c_float), ("gamma", C.c_float), ("sigma", C.c_float), ("sradius", C.c_float),
        ("match_texture", C.c_int32), ("lr_threshold", C.c_int32),
        ("speckle_sim_threshold", C.c_float), ("speckle_size", C.c_int32),
        ("ipol_gap_width", C.c_int32), ("filter_median", C.c_int32),
        ("filter_adaptive_mean", C.c_int32), ("postprocess_only_left", C.c_int32),
        ("subsampling", C.c_int32),
    ]


class Config(C.Structure):
    """svh_config (include/svh.h): the process-wide settings svh_init fixes."""
    _fields_ = [("size", C.c_uint32), ("hw_queues", C.c_int32), ("elas_workers", C.c_int32),
                ("elas_pairs_per_launch", C.c_int32), ("elas_stage", C.c_int32), ("wait_us", C.c_int32),
                ("read_env", C.c_int32), ("reserved_", C.c_int32 * 9)]


class RuntimeInfo(C.Structure):
    """svh_runtime_info (include/svh.h)"""
    _fields_ = [("initialised", C.c_int32), ("implicit", C.c_int32), ("hw_queues_asked", C.c_int32),
                ("hw_queues_state", C.c_int32), ("hw_queues_env", C.c_int32), ("hip_started_before", C.c_int32),
                ("env_modified", C.c_int32), ("read_env", C.c_int32), ("reserved_", C.c_int32 * 8)]

    def as_dict(self):
        names = {0: "none", 1: "applied", 2: "caller_set", 3: "too_late", 4: "hands_off"}
        d = {n: getattr(self, n) for n, _ in self._fields_[:-1]}
        d["hw_queues_state"] = names.get(self.hw_queues_state, self.hw_queues_state)
        return d


def init(**fields):
    """svh_init(&cfg) with the given svh_config fields over the defaults.  Call it before anything in the process
    starts the HIP runtime (e.g. before `import torch`): the hardware-queue count can only be asked for until then."""
    cfg = Config()
    lib().svh_config_default(C.byref(cfg))
    for k, v in fields.items():
        setattr(cfg, k, v)
    rc = lib().svh_init(C.byref(cfg))
    if rc < 0:
        raise SvhError(rc, "svh_init: bad configuration")
    return runtime_info()


class DeviceTopology(C.Structure):
    """svh_device_topology (include/svh.h)"""
    _fields_ = [("device", C.c_int32), ("numa_node", C.c_int32), ("n_cpus", C.c_int32), ("reserved_", C.c_int32),
                ("pci_bus_id", C.c_char * 32), ("cpulist", C.c_char * 256), ("cpu_mask", C.c_uint64 * 16)]


def device_topology(device):
    """PCI bus id, NUMA node and the node's CPUs of a HIP device (svh_get_device_topology)"""
    t = DeviceTopology()
    rc = lib().svh_get_device_topology(int(device), C.byref(t))
    if rc < 0:
        raise SvhError(rc, "svh_get_device_topology")
    return {"device": t.device, "pci_bus_id": t.pci_bus_id.decode(), "numa_node": t.numa_node, "cpus_of_node": t.n_cpus,
            "cpulist": t.cpulist.decode()}


def bind_host_to_device(device, max_cpus=0):
    """restrict this process (and the threads it creates from now on) to the CPUs next to the GPU; returns how many"""
    return int(lib().svh_bind_host_to_device(int(device), int(max_cpus)))


def elas_settings():
    """svh_elas_get_settings: workers, pairs per launch (0 = automatic), stage, poll interval [us]"""
    out = (C.c_int32 * 4)()
    lib().svh_elas_get_settings(out)
    return dict(workers=out[0], pairs_per_launch=out[1], stage=out[2], wait_us=out[3])


def runtime_info():
    ri = RuntimeInfo()
    lib().svh_get_runtime_info(C.byref(ri))
    return ri.as_dict()


DISP_F32, DISP_U16 = 0, 1
MAPS_BOTH, MAPS_LEFT = 0, 1


class ElasOutput(C.Structure):
    """svh_elas_output (include/svh.h): what a host entry returns"""
    _fields_ = [("format", C.c_int32), ("maps", C.c_int32)]


def _output(out, maps):
    """(svh_elas_output, numpy dtype of a map, D2 wanted) of out = "f32" | "u16" and maps = "both" | "left" """
    try:
        o = ElasOutput({"f32": DISP_F32, "u16": DISP_U16}[out], {"both": MAPS_BOTH, "left": MAPS_LEFT}[maps])
    except KeyError:
        raise ValueError("out must be 'f32' or 'u16' and maps 'both' or 'left', not %r / %r" % (out, maps))
    return o, (np.uint16 if o.format == DISP_U16 else np.float32), o.maps == MAPS_BOTH


class SvhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsvhip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load libsvhip.so; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libsvhip.so not built (run __graft_entry__.build()): " + LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.svh_version.restype = C.c_char_p
        L.svh_last_error.restype = C.c_char_p
        L.svh_elas_create.restype = C.c_void_p
        L.svh_elas_create.argtypes = [C.POINTER(ElasParams)]
        L.svh_elas_destroy.argtypes = [C.c_void_p]
        L.svh_elas_params_default.argtypes = [C.POINTER(ElasParams), C.c_int32]
        L.svh_elas_process.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.svh_elas_process_batch.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        L.svh_elas_process_batch_device.argtypes = [
            C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
            C.c_size_t, C.c_void_p, C.c_void_p]
        L.svh_elas_stream_open.restype = C.c_void_p
        L.svh_elas_stream_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_elas_stream_push.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_uint64)]
        L.svh_elas_stream_push_device.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_uint64)]
        L.svh_elas_stream_flush.argtypes = [C.c_void_p]
        L.svh_elas_stream_pop.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_int32]
        L.svh_elas_stream_close.argtypes = [C.c_void_p]
        L.svh_elas_stream_push_device_n.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        L.svh_elas_stream_pop_n.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
        L.svh_elas_stream_push_n.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(C.c_uint64)]
        L.svh_elas_set_taps.argtypes = [C.c_void_p, C.c_int32]
        L.svh_elas_get_stage.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]
        L.svh_elas_last_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_delaunay.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_elas_process_out.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.POINTER(ElasOutput)]
        L.svh_elas_process_batch_out.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.POINTER(ElasOutput)]
        L.svh_elas_stream_open_out.restype = C.c_void_p
        L.svh_elas_stream_open_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ElasOutput)]
        L.svh_elas_stream_push_out.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_uint64)]
        L.svh_elas_stream_push_out_n.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(C.c_uint64)]
        L.svh_disparity_pack_u16.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32]
        L.svh_disparity_unpack_u16.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        _lib = L
    return _lib


SVH_ERR_EMPTY, SVH_ERR_TIMEOUT = -5, -6


class SvhTimeout(SvhError):
    """svh_elas_stream_pop: the next pair was not done within timeout_ms (it stays queued)"""


class ElasStream:
    """svh_elas_stream_*: a bounded, ordered queue of pairs in front of the engine's lanes
    (include/svh.h).  Host arrays pushed here must stay alive until their pair is popped: the
    stream keeps a reference to them."""

    def __init__(self, elas, w, h, pitch, depth=0, out="f32", maps="both"):
        dims = (C.c_int32 * 3)(w, h, pitch)
        self._out, self.dtype, self._both = _output(out, maps)
        self._plain = (out, maps) == ("f32", "both")
        if self._plain:
            self._h = lib().svh_elas_stream_open(elas._h, dims, depth)
        else:
            self._h = lib().svh_elas_stream_open_out(elas._h, dims, depth, C.byref(self._out))
        if not self._h:
            raise SvhError(-1, last_error())
        self._keep = {}

    def _maps_ok(self, Ds):
        for D in Ds:
            if D is not None and np.asarray(D).dtype != self.dtype:
                raise ValueError("this stream writes %s maps" % np.dtype(self.dtype).name)

    def push(self, I1, I2, D1, D2=None):
        """host arrays (uint8 [H,W] with the stream's pitch; maps of the stream's dtype -- float32, or uint16 with
        out="u16" -- written in place; D2 may be None with maps="left")"""
        t = C.c_uint64(0)
        self._maps_ok((D1, D2))
        if self._plain:
            rc = lib().svh_elas_stream_push(self._h, I1.ctypes.data, I2.ctypes.data, D1.ctypes.data,
                                            D2.ctypes.data, C.byref(t))
        else:
            rc = lib().svh_elas_stream_push_out(self._h, I1.ctypes.data, I2.ctypes.data, D1.ctypes.data,
                                                D2.ctypes.data if D2 is not None else None, C.byref(t))
        if rc < 0:
            raise SvhError(rc, last_error())
        self._keep[t.value] = (I1, I2, D1, D2)
        return t.value

    def push_device(self, dI1, dI2, dD1, dD2):
        """raw device pointers (ints)"""
        t = C.c_uint64(0)
        rc = lib().svh_elas_stream_push_device(self._h, dI1, dI2, dD1, dD2, C.byref(t))
        if rc < 0:
            raise SvhError(rc, last_error())
        return t.value

    def push_device_n(self, n, dI1, dI2, in_stride, dD1, dD2, out_stride):
        """n consecutive device-resident pairs in one call (blocks while the stream is full)"""
        t = C.c_uint64(0)
        rc = lib().svh_elas_stream_push_device_n(self._h, n, dI1, dI2, in_stride, dD1, dD2, out_stride, C.byref(t))
        if rc < 0:
            raise SvhError(rc, last_error())
        return t.value

    def push_n(self, I1s, I2s, D1s, D2s=None):
        """n host pairs in one call: arrays [n,H,W] (uint8 images, maps of the stream's dtype written in place; D2s may
        be None with maps="left"); they must stay alive and unread until popped -- the stream keeps a reference"""
        n = len(I1s)
        arr = C.c_void_p * n
        self._maps_ok((D1s, D2s))
        a = [arr(*[int(X[i].ctypes.data) for i in range(n)]) if X is not None else None for X in (I1s, I2s, D1s, D2s)]
        t = C.c_uint64(0)
        push = lib().svh_elas_stream_push_n if self._plain else lib().svh_elas_stream_push_out_n
        rc = push(self._h, n, a[0], a[1], a[2], a[3], C.byref(t))
        if rc < 0:
            raise SvhError(rc, last_error())
        self._keep[("n", t.value)] = (I1s, I2s, D1s, D2s)
        return t.value

    def push_n_raw(self, n, a1, a2, d1, d2):
        """the same with ready-made ctypes pointer arrays (no per-call marshalling); the caller keeps the buffers alive"""
        t = C.c_uint64(0)
        push = lib().svh_elas_stream_push_n if self._plain else lib().svh_elas_stream_push_out_n
        rc = push(self._h, n, a1, a2, d1, d2, C.byref(t))
        if rc < 0:
            raise SvhError(rc, last_error())
        return t.value

    def pop_n(self, n):
        """statuses of the next n pairs (blocks until they are done)"""
        st = (C.c_int32 * n)()
        got = C.c_int32(0)
        rc = lib().svh_elas_stream_pop_n(self._h, n, st, C.byref(got))
        if rc < 0:
            raise SvhError(rc, last_error())
        return list(st)[:got.value]

    def flush(self):
        lib().svh_elas_stream_flush(self._h)

    def pop(self, timeout_ms=-1):
        """(ticket, status) of the next pair in submission order; None when nothing is in flight"""
        t, st = C.c_uint64(0), C.c_int32(0)
        rc = lib().svh_elas_stream_pop(self._h, C.byref(t), C.byref(st), timeout_ms)
        if rc == SVH_ERR_EMPTY:
            return None
        if rc == SVH_ERR_TIMEOUT:
            raise SvhTimeout(rc, "timeout")
        if rc < 0:
            raise SvhError(rc, last_error())
        self._keep.pop(t.value, None)
        return t.value, st.value

    def close(self):
        h, self._h = self._h, None
        if h:
            lib().svh_elas_stream_close(h)
        self._keep.clear()

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            self.close()


def last_error():
    return lib().svh_last_error().decode()


def default_params(setting=ROBOTICS, **kw):
    p = ElasParams()
    lib().svh_elas_params_default(C.byref(p), setting)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def delaunay(pts):
    """svh_delaunay: Triangle-1.6-"zQB"-compatible triangulation (host side)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    cap = 2 * len(pts) + 16
    tri = np.empty((cap, 3), np.int32)
    n = lib().svh_delaunay(pts.ctypes.data, len(pts), tri.ctypes.data, cap)
    if n < 0:
        raise SvhError(n, "svh_delaunay failed")
    return tri[:n].copy()


def _as_params(params):
    """accept any ctypes struct with the svh_elas_params layout"""
    if isinstance(params, ElasParams):
        return params
    return ElasParams.from_buffer_copy(bytes(params))


class Elas:
    """Drop-in for the reference class (libelas/src/elas.h:151-165)."""

    def __init__(self, params=None):
        self._p = _as_params(params) if params is not None else default_params()
        self._h = lib().svh_elas_create(C.byref(self._p))
        if not self._h:
            raise RuntimeError("svh_elas_create failed")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.svh_elas_destroy(h)

    @property
    def params(self):
        return self._p

    def _dshape(self, h, w):
        return (h // 2, w // 2) if self._p.subsampling else (h, w)

    def process(self, I1, I2, D1=None, D2=None, out="f32", maps="both"):
        """Elas::process(I1,I2,D1,D2,dims).  Returns (status, D1, D2); on status 1
        (<3 support points) D1/D2 are left untouched, like the reference.
        out="u16": the maps come back as uint16, value x 256, 0 = invalid (svh_elas_process_out); maps="left": only D1
        is copied down, and the D2 returned is the one passed in (None by default)."""
        o, dtype, both = _output(out, maps)
        I1 = np.asarray(I1, np.uint8)
        I2 = np.asarray(I2, np.uint8)
        assert I1.shape == I2.shape and I1.ndim == 2
        h, w = I1.shape
        # dims[2] is a forward pitch >= width: anything else (reversed / broadcast / column views)
        # is copied first
        if I1.strides[1] != 1 or I2.strides != I1.strides or I1.strides[0] < w:
            I1 = np.ascontiguousarray(I1)
            I2 = np.ascontiguousarray(I2)
        dims = (C.c_int32 * 3)(w, h, I1.strides[0])
        if D1 is None:
            D1 = np.zeros(self._dshape(h, w), dtype)
        if D2 is None and both:
            D2 = np.zeros(self._dshape(h, w), dtype)
        for name, D in (("D1", D1), ("D2", D2)):
            # the library writes h*w packed maps through the raw pointer
            if D is None and not both:
                continue
            if not (isinstance(D, np.ndarray) and D.dtype == dtype and D.flags.c_contiguous
                    and D.flags.writeable and D.shape == self._dshape(h, w)):
                raise ValueError("%s must be a writable C-contiguous %s array of shape %s"
                                 % (name, np.dtype(dtype).name, (self._dshape(h, w),)))
        if (out, maps) == ("f32", "both"):
            rc = lib().svh_elas_process(self._h, I1.ctypes.data, I2.ctypes.data, D1.ctypes.data,
                                        D2.ctypes.data, dims)
        else:
            rc = lib().svh_elas_process_out(self._h, I1.ctypes.data, I2.ctypes.data, D1.ctypes.data,
                                            D2.ctypes.data if D2 is not None else None, dims, C.byref(o))
        if rc < 0:
            raise SvhError(rc, last_error())
        return rc, D1, D2

    def process_batch(self, I1s, I2s, out="f32", maps="both"):
        """n independent pairs (host arrays [n,H,W]) pipelined over the engine lanes.  Returns (statuses, D1, D2);
        out="u16": uint16 maps (value x 256, 0 = invalid); maps="left": D2 is None."""
        o, dtype, both = _output(out, maps)
        I1s = np.ascontiguousarray(I1s, np.uint8)
        I2s = np.ascontiguousarray(I2s, np.uint8)
        n, h, w = I1s.shape
        dh, dw = self._dshape(h, w)
        D1 = np.zeros((n, dh, dw), dtype)
        D2 = np.zeros((n, dh, dw), dtype) if both else None
        arr = C.c_void_p * n
        a1 = arr(*[I1s[i].ctypes.data for i in range(n)])
        a2 = arr(*[I2s[i].ctypes.data for i in range(n)])
        d1 = arr(*[D1[i].ctypes.data for i in range(n)])
        d2 = arr(*[D2[i].ctypes.data for i in range(n)]) if both else None
        st = (C.c_int32 * n)()
        dims = (C.c_int32 * 3)(w, h, w)
        if (out, maps) == ("f32", "both"):
            rc = lib().svh_elas_process_batch(self._h, n, a1, a2, d1, d2, dims, st)
        else:
            rc = lib().svh_elas_process_batch_out(self._h, n, a1, a2, d1, d2, dims, st, C.byref(o))
        if rc < 0:
            raise SvhError(rc, last_error())
        return list(st), D1, D2

    def process_batch_device(self, n, dI1, dI2, in_stride, dD1, dD2, out_stride, w, h, pitch):
        """device-resident batch: raw device pointers (ints), see include/svh.h"""
        st = (C.c_int32 * n)()
        dims = (C.c_int32 * 3)(w, h, pitch)
        rc = lib().svh_elas_process_batch_device(self._h, n, dI1, dI2, in_stride, dD1, dD2,
                                                 out_stride, dims, st)
        if rc < 0:
            raise SvhError(rc, last_error())
        return list(st)

    def stream(self, w, h, pitch=None, depth=0, out="f32", maps="both"):
        """streaming submission (svh_elas_stream_*): pairs in one at a time, results in order"""
        return ElasStream(self, w, h, pitch if pitch is not None else w, depth, out, maps)

    # ---- parity taps -----------------------------------------------------
    def set_taps(self, enable=True):
        lib().svh_elas_set_taps(self._h, 1 if enable else 0)

    def stage(self, stage, dtype):
        n = C.c_size_t(0)
        lib().svh_elas_get_stage(self._h, stage, None, 0, C.byref(n))
        buf = np.empty(n.value, np.uint8)
        if n.value:
            rc = lib().svh_elas_get_stage(self._h, stage, buf.ctypes.data, n.value, C.byref(n))
            if rc < 0:
                raise SvhError(rc, last_error())
        return buf.view(dtype)

    def last_timing(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = lib().svh_elas_last_timing(self._h, names, ms, 16)
        return [(names[i].decode(), ms[i]) for i in range(n)]


def set_lanes(n):
    """batch workers per device (each double-buffered: two HIP streams + buffer sets)"""
    return lib().svh_elas_set_lanes(n)


def set_group(n):
    """pairs pushed through each kernel launch by one lane (1..32)"""
    return lib().svh_elas_set_group(n)


def set_stage(where):
    """E5-E7 (lattice filters, support list, Delaunay x2): 1 device, 0 host, -1 automatic"""
    return lib().svh_elas_set_stage(where)


def set_queue_plan(plan):
    """svh_elas_set_queue_plan: -1 automatic (4 where GPU_MAX_HW_QUEUES is below 2 x workers, else 0), 0 one stream per
    lane, 4 second lanes on a low-priority stream; 1 stage chain high, 2 plan 1 + second lanes low, 3 by phase (slower,
    kept for A/B runs).  Lanes are built with it when created (trim() first for the idle ones).  Returns the value stored."""
    return lib().svh_elas_set_queue_plan(int(plan))


def queue_plan():
    """svh_elas_get_queue_plan: what a lane created now gets"""
    p, s, c = C.c_int32(-9), C.c_int32(-9), C.c_int32(-9)
    lib().svh_elas_get_queue_plan(C.byref(p), C.byref(s), C.byref(c))
    return dict(plan=p.value, streams_per_lane=s.value, classes=c.value)


def feed_stats():
    """svh_elas_feed_stats: how the last batch call fed its workers and what the device's lane pool holds"""
    nw = 64
    out = (C.c_int64 * (8 + 2 * nw))()
    lib().svh_elas_feed_stats(out)
    w = int(out[0])
    return dict(workers=w, groups=int(out[1]), call_us=int(out[2]), out_of_turn=int(out[3]), lanes=int(out[4]),
                streams=dict(normal=int(out[5]), high=int(out[6]), low=int(out[7])),
                taken=[int(out[8 + 2 * k]) for k in range(min(w, nw))],
                finish_us=[int(out[9 + 2 * k]) for k in range(min(w, nw))])


def trim():
    """release the pooled lanes that are idle (device + pinned memory, streams); returns the count"""
    lib().svh_elas_trim.restype = C.c_int64
    return lib().svh_elas_trim()


def stage_stats():
    """(groups through the device stage, groups it handed back to the host path)"""
    a, b = C.c_int64(0), C.c_int64(0)
    lib().svh_elas_stage_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def device_count():
    return lib().svh_device_count()


def pack_u16(D):
    """float disparities -> uint16, value x 256, 0 = invalid, on the device (svh_disparity_pack_u16, k_disp_pack_u16)"""
    D = np.ascontiguousarray(D, np.float32)
    out = np.empty(D.shape, np.uint16)
    rc = lib().svh_disparity_pack_u16(D.ctypes.data, 0, D.size, out.ctypes.data, 0)
    if rc < 0:
        raise SvhError(rc, last_error())
    return out


def unpack_u16(v):
    """the inverse on the host: v / 256 as float32, -1 where v == 0 (svh_disparity_unpack_u16)"""
    v = np.ascontiguousarray(v, np.uint16)
    out = np.empty(v.shape, np.float32)
    rc = lib().svh_disparity_unpack_u16(v.ctypes.data, v.size, out.ctypes.data)
    if rc < 0:
        raise SvhError(rc, last_error())
    return out


# ---------------------------------------------------------------------------
# VisualOdometryMono (svh_vo_mono_*, include/svh.h; libviso2/src/viso_mono.h)
# ---------------------------------------------------------------------------
class MatcherParams(C.Structure):
    """svh_matcher_params == Matcher::parameters (libviso2/src/matcher.h:41-69)"""
    _fields_ = [
        ("nms_n", C.c_int32), ("nms_tau", C.c_int32), ("match_binsize", C.c_int32),
        ("match_radius", C.c_int32), ("match_disp_tolerance", C.c_int32),
        ("outlier_disp_tolerance", C.c_int32), ("outlier_flow_tolerance", C.c_int32),
        ("multi_stage", C.c_int32), ("half_resolution", C.c_int32), ("refinement", C.c_int32),
        ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double), ("base", C.c_double),
    ]


class VoMonoParams(C.Structure):
    """svh_vo_mono_params == VisualOdometryMono::parameters (libviso2/src/viso_mono.h:30-45)"""
    _fields_ = [
        ("match", MatcherParams), ("bucket_max_features", C.c_int32), ("bucket_width", C.c_double),
        ("bucket_height", C.c_double), ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double),
        ("height", C.c_double), ("pitch", C.c_double), ("ransac_iters", C.c_int32),
        ("inlier_threshold", C.c_double), ("motion_threshold", C.c_double),
    ]


# Matcher::p_match (libviso2/src/matcher.h:87-102) == svh_p_match
P_MATCH = np.dtype([("u1p", "f4"), ("v1p", "f4"), ("i1p", "i4"), ("u2p", "f4"), ("v2p", "f4"), ("i2p", "i4"),
                    ("u1c", "f4"), ("v1c", "f4"), ("i1c", "i4"), ("u2c", "f4"), ("v2c", "f4"), ("i2c", "i4")])


def vo_mono_params(**kw):
    """VisualOdometryMono::parameters() (viso_mono.h:38-44) with the given fields replaced"""
    p = VoMonoParams()
    L = lib()
    L.svh_vo_mono_params_default.argtypes = [C.POINTER(VoMonoParams)]
    L.svh_vo_mono_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class VoMono:
    """Drop-in for the reference class VisualOdometryMono (libviso2/src/viso_mono.h): process(I, replace) runs
    pushBack, matchFeatures(0), bucketFeatures and the motion estimate on the device.  private_rand=seed: draw the
    bucketing and RANSAC samples from a private generator with glibc's srand(seed) sequence instead of libc rand()."""

    def __init__(self, params=None, private_rand=None):
        L = self.lib = lib()
        L.svh_vo_mono_create.restype = C.c_void_p
        L.svh_vo_mono_create.argtypes = [C.POINTER(VoMonoParams)]
        L.svh_vo_mono_process.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_vo_mono_get_votes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_vo_mono_set_timing.argtypes = [C.c_void_p, C.c_int32]
        L.svh_vo_mono_get_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_vo_destroy.argtypes = [C.c_void_p]
        L.svh_vo_process_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_vo_estimate_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.svh_vo_get_motion.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_vo_get_inliers.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_vo_get_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_vo_num_matches.argtypes = [C.c_void_p]
        L.svh_vo_set_private_rand.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
        self.params = params if params is not None else vo_mono_params()
        self.h = L.svh_vo_mono_create(C.byref(self.params))
        if not self.h:
            raise SvhError(ERR_BAD_ARG, last_error())
        if private_rand is not None:
            L.svh_vo_set_private_rand(self.h, 1, private_rand)

    def close(self):
        if getattr(self, "h", None):
            self.lib.svh_vo_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc < 0:
            raise SvhError(rc, last_error())
        return bool(rc)

    def process(self, I, replace=False):
        """bool VisualOdometryMono::process(I, dims, replace) -- viso_mono.cpp:32-38"""
        I = np.ascontiguousarray(I, np.uint8)
        dims = (C.c_int32 * 3)(I.shape[1], I.shape[0], I.shape[1])
        return self._check(self.lib.svh_vo_mono_process(self.h, _ptr(I), dims, int(replace)))

    def process_matches(self, matches):
        """bool VisualOdometry::process(p_matched) -- viso.h:87-91"""
        m = np.ascontiguousarray(matches, P_MATCH)
        return self._check(self.lib.svh_vo_process_matches(self.h, _ptr(m), len(m)))

    def estimate_motion(self, matches):
        """estimateMotion(p_matched): (ok, [rx, ry, rz, tx, ty, tz])"""
        m = np.ascontiguousarray(matches, P_MATCH)
        tr = np.zeros(6, np.float64)
        return self._check(self.lib.svh_vo_estimate_motion(self.h, _ptr(m), len(m), _ptr(tr))), tr

    def motion(self):
        """getDeltaMotion(): 4x4"""
        T = np.zeros((4, 4), np.float64)
        self.lib.svh_vo_get_motion(self.h, _ptr(T))
        return T

    def inliers(self):
        n = self.lib.svh_vo_get_inliers(self.h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        self.lib.svh_vo_get_inliers(self.h, _ptr(out), n)
        return out[:n]

    def matches(self):
        n = self.lib.svh_vo_get_matches(self.h, None, 0)
        out = np.zeros(max(n, 1), P_MATCH)
        self.lib.svh_vo_get_matches(self.h, _ptr(out), n)
        return out[:n]

    def num_matches(self):
        return self.lib.svh_vo_num_matches(self.h)

    def votes(self):
        """inlier count of every RANSAC hypothesis of the last estimate (test tap)"""
        n = self.lib.svh_vo_mono_get_votes(self.h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        self.lib.svh_vo_mono_get_votes(self.h, _ptr(out), n)
        return out[:n]

    # ---- K objects in lockstep (svh_vo_mono_*_batch): static methods over a list of VoMono objects
    @staticmethod
    def _batch_args(objs):
        L = objs[0].lib if objs else lib()
        K = len(objs)
        return L, K, (C.c_void_p * max(K, 1))(*[o.h for o in objs])

    @staticmethod
    def _frames(frames, hold):
        """K contiguous uint8 images as a pointer array + dims; `hold` keeps the arrays alive (a frame handed over
        early is read by the library until it is taken)"""
        ims = [np.ascontiguousarray(f, np.uint8) for f in frames]
        hold[:] = ims
        dims = (C.c_int32 * 3)(ims[0].shape[1], ims[0].shape[0], ims[0].shape[1])
        return (C.c_void_p * len(ims))(*[a.ctypes.data for a in ims]), dims

    @staticmethod
    def _replace(replace, K):
        if replace is None:
            return None
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(replace, np.int32), (K,)))
        return r

    @staticmethod
    def process_batch(objs, frames, replace=None, shape=None):
        """svh_vo_mono_process_batch: one frame per object; replace: per object (or one value, or None).  frames=None
        (+ shape=(h, w)): the objects take the frame handed over by prefetch_batch.  Returns the list of per-object
        results (bool)."""
        L, K, hs = VoMono._batch_args(objs)
        hold = []
        if frames is not None:
            ptrs, dims = VoMono._frames(frames, hold)
        else:
            ptrs, dims = None, (C.c_int32 * 3)(shape[1], shape[0], shape[1])
        r = VoMono._replace(replace, K)
        ok = np.zeros(max(K, 1), np.int32)
        L.svh_vo_mono_process_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.svh_vo_mono_process_batch(hs, K, ptrs, dims, None if r is None else _ptr(r), _ptr(ok))
        if rc < 0:
            raise SvhError(rc, last_error())
        return [bool(x) for x in ok[:K]]

    @staticmethod
    def prefetch_batch(objs, frames):
        """svh_vo_mono_prefetch_batch: the next frame of every object handed over early (returns at once)"""
        L, K, hs = VoMono._batch_args(objs)
        hold = []
        ptrs, dims = VoMono._frames(frames, hold)
        for o in objs:
            o._next_frames = hold
        L.svh_vo_mono_prefetch_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        rc = L.svh_vo_mono_prefetch_batch(hs, K, ptrs, dims)
        if rc < 0:
            raise SvhError(rc, last_error())

    @staticmethod
    def process_next_batch(objs, next_frames, shape, replace=None):
        """svh_vo_mono_process_next_batch: process the frame handed over before, hand over next_frames (None after
        the last frame); shape = (h, w) of the images"""
        L, K, hs = VoMono._batch_args(objs)
        hold = []
        ptrs = None
        dims = (C.c_int32 * 3)(shape[1], shape[0], shape[1])
        if next_frames is not None:
            ptrs, dims = VoMono._frames(next_frames, hold)
        r = VoMono._replace(replace, K)
        ok = np.zeros(max(K, 1), np.int32)
        L.svh_vo_mono_process_next_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]
        rc = L.svh_vo_mono_process_next_batch(hs, K, ptrs, dims, None if r is None else _ptr(r), _ptr(ok))
        for o in objs:   # (the frame taken by this call is no longer read; the new one is held instead)
            o._next_frames = hold
        if rc < 0:
            raise SvhError(rc, last_error())
        return [bool(x) for x in ok[:K]]

    @staticmethod
    def process_matches_batch(objs, matches):
        """svh_vo_mono_process_matches_batch: VisualOdometry::process(p_matched) per object, each with its own list"""
        L, K, hs = VoMono._batch_args(objs)
        ms = [np.ascontiguousarray(m, P_MATCH) for m in matches]
        ptrs = (C.c_void_p * max(K, 1))(*[m.ctypes.data if len(m) else None for m in ms])
        n = np.array([len(m) for m in ms] + [0], np.int32)
        ok = np.zeros(max(K, 1), np.int32)
        L.svh_vo_mono_process_matches_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.svh_vo_mono_process_matches_batch(hs, K, ptrs, _ptr(n), _ptr(ok))
        if rc < 0:
            raise SvhError(rc, last_error())
        return [bool(x) for x in ok[:K]]

    def set_timing(self, on=True):
        self.lib.svh_vo_mono_set_timing(self.h, int(on))

    def timing(self):
        """device ms of the last estimate's phases: RANSAC, chirality, plane vote"""
        ms = np.zeros(3, np.float64)
        self.lib.svh_vo_mono_get_timing(self.h, _ptr(ms))
        return ms


# ---------------------------------------------------------------------------
# Reconstruction (svh_recon_*, include/svh.h; libviso2/src/reconstruction.h)
# ---------------------------------------------------------------------------
RECON_CODES = ["TOO_SHORT", "INIT_FAILED", "TYPE_BELOW", "REFINE_FAILED", "TOO_FAR", "ANGLE_SMALL", "ACCEPTED"]
RECON_ACCEPTED = 6


class Reconstruction:
    """Drop-in for the reference class Reconstruction (libviso2/src/reconstruction.h): set_calibration(f, cu, cv)
    once, update(matches, Tr, ...) per frame pair, points().  The tracks live on the host, or with resident=True in
    device memory (svh_recon_create_resident: the association runs as kernels, and K such objects are updated in
    lockstep by Reconstruction.update_batch); every lost track is triangulated, refined and tested on the device and
    the accepted points stay there.  Both forms give the same results."""

    def __init__(self, resident=False):
        L = self.lib = lib()
        L.svh_recon_create.restype = C.c_void_p
        L.svh_recon_create_resident.restype = C.c_void_p
        L.svh_recon_update_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                              C.c_int32, C.c_double, C.c_double]
        L.svh_recon_update_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_double, C.c_double, C.c_void_p]
        self.resident = bool(resident)
        L.svh_recon_destroy.argtypes = [C.c_void_p]
        L.svh_recon_set_calibration.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
        L.svh_recon_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_double, C.c_double]
        L.svh_recon_num_points.argtypes = [C.c_void_p]
        L.svh_recon_get_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_recon_get_points_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.svh_recon_num_tracks.argtypes = [C.c_void_p]
        L.svh_recon_get_outcomes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_recon_set_timing.argtypes = [C.c_void_p, C.c_int32]
        L.svh_recon_get_timing.argtypes = [C.c_void_p, C.c_void_p]
        self.h = L.svh_recon_create_resident() if resident else L.svh_recon_create()
        if not self.h:
            raise SvhError(ERR_BAD_ARG, last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.svh_recon_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc < 0:
            raise SvhError(rc, last_error())
        return rc

    def set_calibration(self, f, cu, cv):
        """setCalibration(f, cu, cv); a second call is refused (SvhError, ERR_BAD_ARG)"""
        self._check(self.lib.svh_recon_set_calibration(self.h, f, cu, cv))

    def update(self, matches, Tr, point_type=1, min_track_length=2, max_dist=30.0, min_angle=2.0):
        """update(p_matched, Tr, point_type, min_track_length, max_dist, min_angle) -- reconstruction.cpp:59-151"""
        m = np.ascontiguousarray(matches, P_MATCH)
        T = np.ascontiguousarray(Tr, np.float64)
        if T.shape != (4, 4):
            raise SvhError(ERR_BAD_ARG, "Tr must be 4x4")
        self._check(self.lib.svh_recon_update(self.h, _ptr(m) if len(m) else None, len(m), _ptr(T), int(point_type),
                                              int(min_track_length), float(max_dist), float(min_angle)))

    def update_device(self, d_matches, n, max_index, Tr, point_type=1, min_track_length=2, max_dist=30.0,
                      min_angle=2.0):
        """svh_recon_update_device (resident objects): d_matches is the device address of n svh_p_match records whose
        feature indices lie in [0, max_index)"""
        T = np.ascontiguousarray(Tr, np.float64)
        if T.shape != (4, 4):
            raise SvhError(ERR_BAD_ARG, "Tr must be 4x4")
        self._check(self.lib.svh_recon_update_device(self.h, d_matches, int(n), int(max_index), _ptr(T),
                                                     int(point_type), int(min_track_length), float(max_dist),
                                                     float(min_angle)))

    @staticmethod
    def update_batch(objs, matches, Trs, point_type=1, min_track_length=2, max_dist=30.0, min_angle=2.0):
        """svh_recon_update_batch: K resident objects in lockstep.  matches[i]: the matches of object i, or None for an
        object that sits this update out; Trs: K 4x4 motions (the entry of an object that sits out is not read).
        Returns the per-object status list; raises SvhError when the call as a whole is refused or fails."""
        L = objs[0].lib if objs else lib()
        K = len(objs)
        hs = (C.c_void_p * max(K, 1))(*[o.h for o in objs])
        ms = [None if m is None else np.ascontiguousarray(m, P_MATCH) for m in matches]
        hold = [np.zeros(1, P_MATCH) if m is not None and len(m) == 0 else m for m in ms]   # (empty: still non-NULL)
        ptrs = (C.c_void_p * max(K, 1))(*[None if m is None else m.ctypes.data for m in hold])
        n = np.array([0 if m is None else len(m) for m in ms] + [0], np.int32)
        T = np.ascontiguousarray(np.stack([np.eye(4) if t is None else np.asarray(t, np.float64) for t in Trs])
                                 if K else np.zeros((1, 4, 4)), np.float64)
        if T.shape != (max(K, 1), 4, 4):
            raise SvhError(ERR_BAD_ARG, "Trs must be K 4x4 matrices")
        status = np.zeros(max(K, 1), np.int32)
        rc = L.svh_recon_update_batch(hs, ptrs, _ptr(n), _ptr(T), K, int(point_type), int(min_track_length),
                                      float(max_dist), float(min_angle), _ptr(status))
        if rc < 0:
            raise SvhError(rc, last_error())
        return [int(x) for x in status[:K]]

    def num_points(self):
        return self.lib.svh_recon_num_points(self.h)

    def num_tracks(self):
        """active tracks"""
        return self.lib.svh_recon_num_tracks(self.h)

    def points(self):
        """getPoints(): (n, 3) float32, copied from the device"""
        n = self.num_points()
        out = np.zeros((max(n, 1), 3), np.float32)
        self._check(self.lib.svh_recon_get_points(self.h, _ptr(out), n))
        return out[:n]

    def points_device(self):
        """(device address of the resident x y z array, number of points); valid until the next update"""
        p = C.c_void_p()
        n = self._check(self.lib.svh_recon_get_points_device(self.h, C.byref(p)))
        return p.value, n

    def outcomes(self):
        """the tracks lost in the last update, in order: (codes int32, points (n, 3) float32)"""
        n = self.lib.svh_recon_get_outcomes(self.h, None, None, 0)
        code, xyz = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 3), np.float32)
        self.lib.svh_recon_get_outcomes(self.h, _ptr(code), _ptr(xyz), n)
        return code[:n], xyz[:n]

    def set_timing(self, on=True):
        self.lib.svh_recon_set_timing(self.h, int(on))

    def timing(self):
        """ms of the last update: host bookkeeping, device (uploads + kernels), copy-back of the outcomes"""
        ms = np.zeros(3, np.float64)
        self.lib.svh_recon_get_timing(self.h, _ptr(ms))
        return ms


# ---------------------------------------------------------------------------
# PlaneEstimation (svh_plane_*, include/svh_plane.h; stereomapper/planeestimation.h)
# ---------------------------------------------------------------------------
PLANE_NO_POINTS, PLANE_FEW_INLIERS = 2, 3


class PlaneParams(C.Structure):
    """svh_plane_params (include/svh_plane.h): the reference's constants as parameters"""
    _fields_ = [("num_samples", C.c_int32), ("step_size", C.c_int32), ("max_draws", C.c_int32),
                ("roi", C.c_int32 * 4), ("min_dist", C.c_float), ("d_threshold", C.c_double)]


def _plane_bind(L):
    if getattr(L, "_plane_bound", False):
        return
    L.svh_plane_params_default.argtypes = [C.c_void_p]
    L.svh_plane_params_default.restype = None
    L.svh_plane_create.restype = C.c_void_p
    L.svh_plane_create.argtypes = [C.c_void_p]
    L.svh_plane_destroy.argtypes = [C.c_void_p]
    L.svh_plane_destroy.restype = None
    L.svh_plane_release.argtypes = [C.c_void_p]
    L.svh_plane_release.restype = C.c_int64
    L.svh_plane_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                     C.c_float, C.c_float, C.c_float, C.c_uint32]
    L.svh_plane_estimate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    for name in ("svh_plane_get_plane_dsi", "svh_plane_get_plane_euclidean", "svh_plane_get_transformation"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        getattr(L, name).restype = None
    L.svh_plane_get_pitch.argtypes = [C.c_void_p]
    L.svh_plane_get_pitch.restype = C.c_float
    L.svh_plane_get_list.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.svh_plane_get_hypotheses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    L.svh_plane_get_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    L.svh_plane_set_timing.argtypes = [C.c_void_p, C.c_int32]
    L.svh_plane_set_timing.restype = None
    L.svh_plane_get_timing.argtypes = [C.c_void_p, C.c_void_p]
    L._plane_bound = True


class PlaneEstimation:
    """Drop-in for the reference class PlaneEstimation (stereomapper/planeestimation.h): estimate(D, ...) is
    computeTransformationFromDisparityMap with the draws of srand(seed); D is a host array or a device address."""

    def __init__(self, **params):
        L = self.lib = lib()
        _plane_bind(L)
        P = PlaneParams()
        L.svh_plane_params_default(C.byref(P))
        for k, v in params.items():
            if k == "roi":
                P.roi = (C.c_int32 * 4)(*[int(x) for x in v])
            else:
                setattr(P, k, v)
        self.h = L.svh_plane_create(C.byref(P))
        if not self.h:
            raise SvhError(ERR_BAD_ARG, last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.svh_plane_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def estimate(self, D, width=None, height=None, step=None, f=721.5, cu=609.6, cv=172.9, base=0.54, seed=0):
        """D: (height, step) float32 host array, or an int device address (then width, height and step are needed).
        Returns OK, PLANE_NO_POINTS or PLANE_FEW_INLIERS; raises SvhError on a negative status."""
        if isinstance(D, (int, np.integer)):
            addr, dev = int(D), 1
        else:
            self._keep = D = np.ascontiguousarray(D, np.float32)
            height = D.shape[0] if height is None else height
            step = D.shape[1] if step is None else step
            width = step if width is None else width
            addr, dev = D.ctypes.data, 0
        rc = self.lib.svh_plane_estimate(self.h, addr, dev, int(width), int(height), int(step), f, cu, cv, base,
                                         int(seed) & 0xFFFFFFFF)
        if rc < 0:
            raise SvhError(rc, last_error())
        return rc

    @staticmethod
    def estimate_batch(objs, addrs, width, height, step, f=721.5, cu=609.6, cv=172.9, base=0.54, seeds=None):
        """svh_plane_estimate_batch over device-resident maps; returns the list of statuses"""
        n = len(objs)
        L = objs[0].lib
        hs = (C.c_void_p * n)(*[o.h for o in objs])
        ds = (C.c_void_p * n)(*[int(a) for a in addrs])
        sd = np.ascontiguousarray(seeds if seeds is not None else np.zeros(n), np.uint32)
        st = np.zeros(n, np.int32)
        rc = L.svh_plane_estimate_batch(hs, ds, n, int(width), int(height), int(step), f, cu, cv, base, _ptr(sd),
                                        _ptr(st))
        if rc < 0:
            raise SvhError(rc, last_error())
        return st.tolist()

    def _vec(self, fn, n):
        out = np.zeros(n, np.float64)
        fn(self.h, _ptr(out))
        return out

    def plane_dsi(self):
        return self._vec(self.lib.svh_plane_get_plane_dsi, 3)

    def plane_euclidean(self):
        return self._vec(self.lib.svh_plane_get_plane_euclidean, 3)

    def transformation(self):
        return self._vec(self.lib.svh_plane_get_transformation, 16).reshape(4, 4)

    def pitch(self):
        return np.float32(self.lib.svh_plane_get_pitch(self.h))

    def taps(self):
        """the last call as a dict shaped like the reference harness' record (tests/plane_ref.py)"""
        L = self.lib
        n = L.svh_plane_get_list(self.h, None, 0)
        lst = np.zeros((max(n, 1), 3), np.float32)
        L.svh_plane_get_list(self.h, _ptr(lst), n)
        S = L.svh_plane_get_hypotheses(self.h, None, None, None, 0)
        planes = np.zeros((max(S, 1), 3), np.float64)
        draws, votes = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32)
        L.svh_plane_get_hypotheses(self.h, _ptr(planes), _ptr(draws), _ptr(votes), S)
        best = C.c_int32(-1)
        nin = L.svh_plane_get_best(self.h, C.byref(best), None, 0)
        inl = np.zeros(max(nin, 1), np.int32)
        L.svh_plane_get_best(self.h, C.byref(best), _ptr(inl), nin)
        return {"plane_d": self.plane_dsi(), "plane_e": self.plane_euclidean(), "H": self.transformation(),
                "pitch": self.pitch(), "list": lst[:n], "planes": planes[:S], "draws": draws[:S], "votes": votes[:S],
                "best": best.value, "inliers": inl[:nin]}

    def release(self):
        return self.lib.svh_plane_release(self.h)

    def set_timing(self, on=True):
        self.lib.svh_plane_set_timing(self.h, int(on))

    def timing(self):
        """ms of the last call: see svh_plane_get_timing (include/svh_plane.h)"""
        ms = np.zeros(7, np.float64)
        self.lib.svh_plane_get_timing(self.h, _ptr(ms))
        return ms
