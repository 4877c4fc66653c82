"""ctypes binding of the device-frame entries of libsvhip.so: the Matcher, the visual odometry (stereo and mono) and the
map fusion fed with frames that are already in device memory (include/svh.h svh_matcher_push_back_device,
svh_vo_process_device, svh_vo_mono_process_device; include/svh_map.h svh_map_add_device), and the three test-access
functions of that path (csrc/hip_guard.h).

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
