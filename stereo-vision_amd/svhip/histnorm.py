"""ctypes binding of the histogram normalisation in libsvhip.so (C-ABI: include/svh_histnorm.h): what
StereoImage::histogramNormalization does to an 8-bit frame (stereomapper/stereoimage.cpp:94-134), in place, on the
device.  The byte wrap of the reference's map is part of the contract (see the header)."""
import ctypes as C

import numpy as np

from . import ERR_BAD_ARG, SvhError, last_error, lib

MAX_SEGMENTS = 192


def _bind():
    L = lib()
    if not getattr(L, "_histnorm_bound", False):
        L.svh_histnorm_create.restype = C.c_void_p
        L.svh_histnorm_create.argtypes = [C.c_int32, C.c_int32]
        L.svh_histnorm_destroy.argtypes = [C.c_void_p]
        L.svh_histnorm_destroy.restype = None
        L.svh_histnorm_release.argtypes = [C.c_void_p]
        L.svh_histnorm_release.restype = C.c_int64
        L.svh_histnorm_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.svh_histnorm_images_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_size_t]
        L.svh_histnorm_pairs_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t]
        L.svh_histnorm_get_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_histnorm_table_host.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svh_histnorm_segments.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_histnorm_chain.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_histnorm_set_timing.argtypes = [C.c_void_p, C.c_int32]
        L.svh_histnorm_set_timing.restype = None
        L.svh_histnorm_get_timing.argtypes = [C.c_void_p, C.c_void_p]
        L._histnorm_bound = True
    return L


def _check(rc):
    if rc < 0:
        raise SvhError(rc, last_error())
    return rc


def table_host(width, height, counts):
    """(cdf float32 [256], map uint8 [256]) of an image of width x height pixels with these counts; needs no device"""
    counts = np.ascontiguousarray(counts, np.int32)
    if counts.shape != (256,):
        raise SvhError(ERR_BAD_ARG, "counts must have 256 entries")
    cdf, m = np.zeros(256, np.float32), np.zeros(256, np.uint8)
    _check(_bind().svh_histnorm_table_host(width, height, counts.ctypes.data, cdf.ctypes.data, m.ctypes.data))
    return cdf, m


def segments(width, height):
    """(n0 int32 [k], f float32 [k], inc float32 [k]): the linear segments of the float chain f for this image size"""
    n0, f, inc = np.zeros(MAX_SEGMENTS, np.int32), np.zeros(MAX_SEGMENTS, np.float32), np.zeros(MAX_SEGMENTS, np.float32)
    k = _check(_bind().svh_histnorm_segments(width, height, n0.ctypes.data, f.ctypes.data, inc.ctypes.data, MAX_SEGMENTS))
    return n0[:k].copy(), f[:k].copy(), inc[:k].copy()


def chain(width, height, n):
    """f(n) for an array of n in 0..width*height, from the segment table"""
    n = np.ascontiguousarray(n, np.int32)
    out = np.zeros(n.shape, np.float32)
    _check(_bind().svh_histnorm_chain(width, height, n.ctypes.data, n.size, out.ctypes.data))
    return out


class HistNorm:
    """h = HistNorm(width, height); h.apply(image) equalises a host image in place, h.images_device(...) /
    h.pairs_device(...) images resident in device memory"""

    def __init__(self, width, height):
        self._L = _bind()
        self.width, self.height = width, height
        self._h = self._L.svh_histnorm_create(width, height)
        if not self._h:
            raise SvhError(ERR_BAD_ARG, last_error())

    def apply(self, image):
        """one host image, uint8 [height, >= width] rows with unit pixel stride, in place; returns it"""
        a = image
        if (not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 2 or a.shape != (self.height, self.width)
                or a.strides[1] != 1 or a.strides[0] < self.width or not a.flags.writeable):
            raise SvhError(ERR_BAD_ARG, "the image must be a writable uint8 array of height rows of width bytes")
        _check(self._L.svh_histnorm_apply(self._h, a.ctypes.data, 0, a.strides[0]))
        return a

    def apply_raw(self, addr, on_device, row_stride):
        """svh_histnorm_apply with a raw address (int)"""
        return _check(self._L.svh_histnorm_apply(self._h, addr, int(on_device), row_stride))

    def images_device(self, n, dI, row_stride, image_stride):
        """svh_histnorm_images_device: raw device address (int)"""
        return _check(self._L.svh_histnorm_images_device(self._h, n, dI, row_stride, image_stride))

    def pairs_device(self, n, dI1, dI2, row_stride, image_stride):
        """svh_histnorm_pairs_device: raw device addresses (ints); what svh_rectify_pairs_device leaves"""
        return _check(self._L.svh_histnorm_pairs_device(self._h, n, dI1, dI2, row_stride, image_stride))

    def tables(self):
        """(counts int32 [n, 256], cdf float32 [n, 256], map uint8 [n, 256]) of the last call's n images"""
        n = _check(self._L.svh_histnorm_get_tables(self._h, None, None, None, 0))
        counts, cdf, m = np.zeros((n, 256), np.int32), np.zeros((n, 256), np.float32), np.zeros((n, 256), np.uint8)
        if n:
            _check(self._L.svh_histnorm_get_tables(self._h, counts.ctypes.data, cdf.ctypes.data, m.ctypes.data, n))
        return counts, cdf, m

    def release(self):
        return self._L.svh_histnorm_release(self._h)

    def set_timing(self, on=True):
        self._L.svh_histnorm_set_timing(self._h, int(on))

    def timing(self):
        """device ms of the last call: the whole call, count + table, apply"""
        ms = np.zeros(3, np.float64)
        self._L.svh_histnorm_get_timing(self._h, ms.ctypes.data)
        return ms

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.svh_histnorm_destroy(h)

    def __del__(self):
        self.close()
