"""ctypes binding of the rectification in libsvhip.so (C-ABI: include/svh_rectify.h): what stereomapper's capture thread
does with a raw frame before the stereo pipeline sees it (framecapturethread.cpp:100-131, 328-349), on the device."""
import ctypes as C

import numpy as np

from . import ERR_BAD_ARG, SvhError, last_error, lib
from .kitti import Calib

WRAP, ZERO = 0, 1


class RectifyCamera(C.Structure):
    """svh_rectify_camera: K, D = (k1 k2 p1 p2 k3), R, P (3x4), row major"""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 5), ("R", C.c_double * 9), ("P", C.c_double * 12)]


class RectifyParams(C.Structure):
    """svh_rectify_params"""
    _fields_ = [("src_width", C.c_int32), ("src_height", C.c_int32), ("dst_width", C.c_int32),
                ("dst_height", C.c_int32), ("border", C.c_int32), ("cameras", C.c_int32), ("cam", RectifyCamera * 2)]


def _bind():
    L = lib()
    if not getattr(L, "_rectify_bound", False):
        L.svh_rectify_params_default.argtypes = [C.POINTER(RectifyParams)]
        L.svh_rectify_params_default.restype = None
        L.svh_rectify_from_kitti.argtypes = [C.POINTER(Calib), C.c_int32, C.c_int32, C.c_int32, C.POINTER(RectifyParams)]
        L.svh_rectify_create.restype = C.c_void_p
        L.svh_rectify_create.argtypes = [C.POINTER(RectifyParams)]
        L.svh_rectify_destroy.argtypes = [C.c_void_p]
        L.svh_rectify_destroy.restype = None
        L.svh_rectify_release.argtypes = [C.c_void_p]
        L.svh_rectify_release.restype = C.c_int64
        L.svh_rectify_get_maps.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t]
        L.svh_rectify_get_maps.restype = C.c_int64
        L.svh_rectify_remap.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                        C.c_int32]
        L.svh_rectify_pairs_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t]
        L.svh_rectify_set_timing.argtypes = [C.c_void_p, C.c_int32]
        L.svh_rectify_set_timing.restype = None
        L.svh_rectify_get_timing.argtypes = [C.c_void_p, C.c_void_p]
        L._rectify_bound = True
    return L


def default_params():
    p = RectifyParams()
    _bind().svh_rectify_params_default(C.byref(p))
    return p


def params(src_size, dst_size, cams, border=WRAP):
    """src_size, dst_size: (width, height); cams: one or two dicts / objects with K (9), D (5), R (9), P (12)"""
    p = default_params()
    (p.src_width, p.src_height), (p.dst_width, p.dst_height) = src_size, dst_size
    p.border, p.cameras = border, len(cams)
    for c, cam in enumerate(cams[:2]):
        for name, n in (("K", 9), ("D", 5), ("R", 9), ("P", 12)):
            v = np.asarray(cam[name], np.float64).ravel()
            if v.size != n:
                raise SvhError(ERR_BAD_ARG, "%s must have %d entries" % (name, n))
            setattr(p.cam[c], name, (C.c_double * n)(*v))
    return p


def params_from_kitti(calib, cam_left=0, cam_right=1, border=WRAP):
    """svh_rectify_from_kitti: calib is a kitti.Calib (kitti.read_cam_to_cam); cam_right = -1 for one camera"""
    p = RectifyParams()
    rc = _bind().svh_rectify_from_kitti(C.byref(calib), cam_left, cam_right, border, C.byref(p))
    if rc:
        raise SvhError(rc, last_error())
    return p


class Rectifier:
    """r = Rectifier(params); r.remap(cam, raw) per frame, or r.pairs_device(...) for pairs resident in device memory"""

    def __init__(self, prm):
        self._L = _bind()
        self.params = prm
        self._h = self._L.svh_rectify_create(C.byref(prm))
        if not self._h:
            raise SvhError(ERR_BAD_ARG, last_error())

    @property
    def dst_shape(self):
        return self.params.dst_height, self.params.dst_width

    def _check(self, rc):
        if rc < 0:
            raise SvhError(rc, last_error())
        return rc

    def maps(self, cam):
        """(mx, my): float32 [dst_height, dst_width], from the device when there is one"""
        mx, my = np.zeros(self.dst_shape, np.float32), np.zeros(self.dst_shape, np.float32)
        self._check(self._L.svh_rectify_get_maps(self._h, cam, mx.ctypes.data, my.ctypes.data, mx.size))
        return mx, my

    def remap(self, cam, src, dst=None):
        """one host image: src uint8 [src_height, >= src_width] rows; dst (optional) is written in place and returned"""
        src = np.asarray(src, np.uint8)
        if src.ndim != 2 or src.strides[1] != 1 or src.strides[0] < src.shape[1]:
            src = np.ascontiguousarray(src)
        if src.shape != (self.params.src_height, self.params.src_width):
            raise SvhError(ERR_BAD_ARG, "the source is not src_height x src_width")
        if dst is None:
            dst = np.zeros(self.dst_shape, np.uint8)
        if dst.dtype != np.uint8 or dst.shape != self.dst_shape or dst.strides[1] != 1 or dst.strides[0] < dst.shape[1]:
            raise SvhError(ERR_BAD_ARG, "dst must be a uint8 array of dst_height rows of dst_width bytes")
        self._check(self._L.svh_rectify_remap(self._h, cam, src.ctypes.data, 0, src.strides[0], dst.ctypes.data, 0,
                                              dst.strides[0]))
        return dst

    def remap_raw(self, cam, src, src_on_device, src_row_stride, dst, dst_on_device, dst_row_stride):
        """svh_rectify_remap with raw addresses (ints)"""
        return self._check(self._L.svh_rectify_remap(self._h, cam, src, int(src_on_device), src_row_stride, dst,
                                                     int(dst_on_device), dst_row_stride))

    def pairs_device(self, n, dS1, dS2, src_row_stride, src_image_stride, dI1, dI2, dst_row_stride, dst_image_stride):
        """svh_rectify_pairs_device: raw device addresses (ints), see include/svh_rectify.h"""
        return self._check(self._L.svh_rectify_pairs_device(self._h, n, dS1, dS2, src_row_stride, src_image_stride,
                                                            dI1, dI2, dst_row_stride, dst_image_stride))

    def release(self):
        return self._L.svh_rectify_release(self._h)

    def set_timing(self, on=True):
        self._L.svh_rectify_set_timing(self._h, int(on))

    def timing(self):
        """device ms of the last call: the remap, the map kernel (when that call built the maps)"""
        ms = np.zeros(2, np.float64)
        self._L.svh_rectify_get_timing(self._h, ms.ctypes.data)
        return ms

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.svh_rectify_destroy(h)

    def __del__(self):
        self.close()
