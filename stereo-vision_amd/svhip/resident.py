"""ctypes binding of the device-frame entries of libsvhip.so: the Matcher, the visual odometry (stereo and mono) and the
map fusion fed with frames that are already in device memory (include/svh.h svh_matcher_push_back_device,
svh_vo_process_device, svh_vo_mono_process_device; include/svh_map.h svh_map_add_device), their lockstep forms for K
objects (svh_matcher_push_back_batch_device, svh_vo_process_batch_device, svh_vo_mono_process_batch_device,
svh_vo_get_gain_batch, svh_map_add_batch_device), and the test-access functions of that path (csrc/hip_guard.h).

The functions work on the handles the existing wrappers hold: pass the wrapper (anything with a `.h` or `._h` handle:
svhip.VoMono, svhip.mapper.Mapper, the test drivers over svh_matcher_* / svh_vo_*) or the raw handle.  Device pointers
are raw addresses (ints).  A frame is `h` rows of `w` bytes, `pitch` bytes apart, at any byte alignment."""
import ctypes as C

import numpy as np

from . import P_MATCH, SvhError, last_error, lib

PREV_LEFT, PREV_RIGHT, CUR_LEFT, CUR_RIGHT = range(4)   # svh_test_matcher_image: view = 2 * current + right
GAIN_HOST, GAIN_DEVICE = 0, 1                           # svh_test_matcher_gain: path

SYMBOLS = ("svh_matcher_push_back_device", "svh_vo_process_device", "svh_vo_mono_process_device", "svh_map_add_device",
           "svh_test_pack_rows", "svh_test_matcher_image", "svh_test_matcher_gain")
# the lockstep forms over device frames, and the tap that shows a call ran in lockstep
LOCKSTEP_SYMBOLS = ("svh_matcher_push_back_batch_device", "svh_vo_process_batch_device",
                    "svh_vo_mono_process_batch_device", "svh_vo_get_gain_batch", "svh_map_add_batch_device",
                    "svh_test_lockstep_counts")


def _bind():
    L = lib()
    if not getattr(L, "_resident_bound", False):
        P, I = C.c_void_p, C.c_int32
        L.svh_matcher_push_back_device.argtypes = [P, P, P, P, I]
        L.svh_vo_process_device.argtypes = [P, P, P, P, I]
        L.svh_vo_mono_process_device.argtypes = [P, P, P, I]
        L.svh_map_add_device.argtypes = [P, P, P, P, P, C.c_float]
        L.svh_test_pack_rows.argtypes = [P, I, I, I, I, P]
        L.svh_test_matcher_image.restype = C.c_int64
        L.svh_test_matcher_image.argtypes = [P, I, P, C.c_size_t]
        L.svh_test_matcher_gain.restype = C.c_float
        L.svh_test_matcher_gain.argtypes = [P, P, I, P, I, I]
        L.svh_matcher_get_gain.restype = C.c_float
        L.svh_matcher_get_gain.argtypes = [P, P, I]
        L.svh_matcher_push_back_batch_device.argtypes = [P, I, P, P, P, I]
        L.svh_vo_process_batch_device.argtypes = [P, I, P, P, P, I, P]
        L.svh_vo_mono_process_batch_device.argtypes = [P, I, P, P, P, P]
        L.svh_vo_get_gain_batch.argtypes = [P, I, P, P, P]
        L.svh_map_add_batch_device.argtypes = [P, I, P, P, P, P, P]
        L.svh_test_lockstep_counts.restype = None
        L.svh_test_lockstep_counts.argtypes = [P]
        L._resident_bound = True
    return L


def _handle(obj):
    for name in ("h", "_h"):
        if hasattr(obj, name):
            return getattr(obj, name)
    return obj


def _dims(w, h, pitch):
    return (C.c_int32 * 3)(w, h, w if pitch is None else pitch)


def _check(rc):
    if rc < 0:
        raise SvhError(rc, last_error())
    return rc


def bpl_of(w):
    """the Matcher's aligned row length (matcher.cpp:173): +16 even when w is a multiple of 16"""
    return w + 16 - w % 16


def matcher_push_back(matcher, dI1, dI2, w, h, pitch=None, replace=False, check=True):
    """svh_matcher_push_back_device; dI2 may be None.  check=False returns the code instead of raising"""
    rc = _bind().svh_matcher_push_back_device(_handle(matcher), dI1, dI2, _dims(w, h, pitch), int(replace))
    return _check(rc) if check else rc


def vo_process(vo, dI1, dI2, w, h, pitch=None, replace=False):
    """svh_vo_process_device: 1 (motion updated), 0 (estimate failed); raises on a negative code"""
    return _check(_bind().svh_vo_process_device(_handle(vo), dI1, dI2, _dims(w, h, pitch), int(replace)))


def vo_mono_process(vo, dI, w, h, pitch=None, replace=False):
    """svh_vo_mono_process_device"""
    return _check(_bind().svh_vo_mono_process_device(_handle(vo), dI, _dims(w, h, pitch), int(replace)))


def map_add(mapper, dD1, dI1, w, h, H_total, gain=0.0, pitch=None):
    """svh_map_add_device: D1 (w * h floats, rows packed) and I1 both in device memory"""
    H = np.ascontiguousarray(H_total, np.float64)
    _check(_bind().svh_map_add_device(_handle(mapper), dD1, dI1, _dims(w, h, pitch), H.ctypes.data, gain))
    if hasattr(mapper, "_shape"):
        mapper._shape = (h, w)


def matcher_gain(matcher, inliers):
    """svh_matcher_get_gain on a raw Matcher handle"""
    a = np.ascontiguousarray(inliers, np.int32)
    return float(_bind().svh_matcher_get_gain(_handle(matcher), a.ctypes.data, len(a)))


# ---- K objects in lockstep
def _table(items):
    """K pointers (handles or device addresses; None stays NULL) as a C array"""
    return (C.c_void_p * len(items))(*[None if x is None else _handle(x) for x in items])


def matcher_push_back_batch(matchers, dI1, dI2, w, h, pitch=None, replace=False, check=True):
    """svh_matcher_push_back_batch_device: dI1 / dI2 are K device addresses each (dI2 may be None)"""
    rc = _bind().svh_matcher_push_back_batch_device(_table(matchers), len(matchers), _table(dI1),
                                                    None if dI2 is None else _table(dI2), _dims(w, h, pitch),
                                                    int(replace))
    return _check(rc) if check else rc


def vo_process_batch(vos, dI1, dI2, w, h, pitch=None, replace=False):
    """svh_vo_process_batch_device: the per-object return values (1 motion updated, 0 estimate failed)"""
    ok = (C.c_int32 * len(vos))()
    _check(_bind().svh_vo_process_batch_device(_table(vos), len(vos), _table(dI1), _table(dI2), _dims(w, h, pitch),
                                               int(replace), ok))
    return list(ok)


def vo_mono_process_batch(vos, dI, w, h, pitch=None, replace=None):
    """svh_vo_mono_process_batch_device; replace: None or K flags"""
    ok = (C.c_int32 * len(vos))()
    rep = None if replace is None else (C.c_int32 * len(vos))(*[int(r) for r in replace])
    _check(_bind().svh_vo_mono_process_batch_device(_table(vos), len(vos), _table(dI), _dims(w, h, pitch), rep, ok))
    return list(ok)


def vo_gain_batch(vos, inliers):
    """svh_vo_get_gain_batch: inliers = K index lists; K float32 gains"""
    arrs = [np.ascontiguousarray(a, np.int32) for a in inliers]
    n = (C.c_int32 * len(vos))(*[len(a) for a in arrs])
    gain = np.zeros(len(vos), np.float32)
    _check(_bind().svh_vo_get_gain_batch(_table(vos), len(vos), _table([a.ctypes.data if len(a) else None for a in arrs]),
                                         n, gain.ctypes.data))
    return gain


def map_add_batch(mappers, dD1, dI1, w, h, H_total, gain=None, pitch=None, check=True):
    """svh_map_add_batch_device: K device disparity maps and images, K poses, K gains (None: no gain correction)"""
    Hs = [np.ascontiguousarray(H, np.float64) for H in H_total]
    g = np.zeros(len(mappers), np.float32) if gain is None else np.ascontiguousarray(gain, np.float32)
    rc = _bind().svh_map_add_batch_device(_table(mappers), len(mappers), _table(dD1), _table(dI1), _dims(w, h, pitch),
                                          _table([H.ctypes.data for H in Hs]), g.ctypes.data)
    if rc >= 0:
        for m in mappers:
            if hasattr(m, "_shape"):
                m._shape = (h, w)
    return _check(rc) if check else rc


def lockstep_counts():
    """svh_test_lockstep_counts: (phases flushed as batched launches, phases run one by one, batched launches)"""
    out = (C.c_int64 * 3)()
    _bind().svh_test_lockstep_counts(out)
    return tuple(out)


# ---- test access (t_*: over svh_test_*)
def t_pack_rows(src_dev, w, h, pitch, bpl):
    """k_pack_rows alone: [h, bpl] uint8, as it would lie in a view"""
    out = np.full((h, bpl), 0x55, np.uint8)
    _check(_bind().svh_test_pack_rows(src_dev, w, h, pitch, bpl, out.ctypes.data))
    return out


def t_matcher_image(matcher, view):
    """the packed image of a view on the device: h * bpl bytes, flat (None: the view holds no frame)"""
    L = _bind()
    n = _check(L.svh_test_matcher_image(_handle(matcher), view, None, 0))
    if n == 0:
        return None
    buf = np.zeros(n, np.uint8)
    _check(L.svh_test_matcher_image(_handle(matcher), view, buf.ctypes.data, n))
    return buf


def t_matcher_gain(matcher, matches, inliers, path):
    """Matcher::getGain over the object's two left frames for caller-given matches; NaN raises"""
    m = np.ascontiguousarray(matches, P_MATCH)
    a = np.ascontiguousarray(inliers, np.int32)
    g = float(_bind().svh_test_matcher_gain(_handle(matcher), m.ctypes.data if len(m) else None, len(m),
                                            a.ctypes.data if len(a) else None, len(a), path))
    if g != g:
        raise SvhError(-1, last_error())
    return np.float32(g)
