"""ctypes binding of the 2-D panes in libsvhip.so (C-ABI: include/svh_view2d.h): what stereomapper's View2D shows of the
images, matches and disparity maps MainDialog hands it (maindialog.cpp:451-452, 506-511, 588-598; view2d.cpp), rendered
on the device."""
import ctypes as C

import numpy as np

from . import ERR_BAD_ARG, SvhError, last_error, lib

P_MATCH = np.dtype([("u1p", "f4"), ("v1p", "f4"), ("i1p", "i4"), ("u2p", "f4"), ("v2p", "f4"), ("i2p", "i4"),
                    ("u1c", "f4"), ("v1c", "f4"), ("i1c", "i4"), ("u2c", "f4"), ("v2c", "f4"), ("i2c", "i4")])


def _bind():
    L = lib()
    if not getattr(L, "_view2d_bound", False):
        L.svh_view2d_create.restype = C.c_void_p
        L.svh_view2d_create.argtypes = [C.c_int32, C.c_int32]
        L.svh_view2d_destroy.argtypes = [C.c_void_p]
        L.svh_view2d_destroy.restype = None
        L.svh_view2d_resize.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.svh_view2d_set_image.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_view2d_set_color_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.svh_view2d_set_disparity.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.svh_view2d_set_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        L.svh_view2d_set_matches_indexed.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        L.svh_view2d_clear_matches.argtypes = [C.c_void_p]
        L.svh_view2d_clear_matches.restype = None
        L.svh_view2d_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L._view2d_bound = True
    return L


class View2D:
    """p = View2D(width, height); p.set_image(I); p.set_matches(m, inliers, left=True); img = p.render()

    Every source may be a numpy array on the host or, with the *_device forms, a raw device address (int)."""

    def __init__(self, width, height):
        self._L = _bind()
        self._h = self._L.svh_view2d_create(width, height)
        if not self._h:
            raise SvhError(ERR_BAD_ARG, last_error())
        self.width, self.height = width, height

    def _check(self, rc):
        if rc < 0:
            raise SvhError(int(rc), last_error())
        return rc

    def resize(self, width, height):
        self._check(self._L.svh_view2d_resize(self._h, width, height))
        self.width, self.height = width, height

    def set_image(self, I):
        """setImage: an [h, w] uint8 image (rows may be strided); clears the matches"""
        I = np.asarray(I, np.uint8)
        if I.ndim != 2 or I.strides[1] != 1 or I.strides[0] < I.shape[1]:
            I = np.ascontiguousarray(I, np.uint8).reshape(I.shape[0], -1)
        dims = (C.c_int32 * 3)(I.shape[1], I.shape[0], I.strides[0])
        self._check(self._L.svh_view2d_set_image(self._h, I.ctypes.data, dims, 0))

    def set_image_device(self, ptr, w, h, pitch=None):
        dims = (C.c_int32 * 3)(w, h, w if pitch is None else pitch)
        self._check(self._L.svh_view2d_set_image(self._h, ptr, dims, 1))

    def set_color_image(self, rgb):
        """setColorImage: [h, w, 3] float32; the matches stay"""
        rgb = np.ascontiguousarray(rgb, np.float32)
        self._check(self._L.svh_view2d_set_color_image(self._h, rgb.ctypes.data, rgb.shape[1], rgb.shape[0], 0))

    def set_color_image_device(self, ptr, w, h):
        self._check(self._L.svh_view2d_set_color_image(self._h, ptr, w, h, 1))

    def set_disparity(self, D):
        """the colour-coded disparity map of an [h, w] float32 map; the matches stay"""
        D = np.ascontiguousarray(D, np.float32)
        self._check(self._L.svh_view2d_set_disparity(self._h, D.ctypes.data, D.shape[1], D.shape[0], 0))

    def set_disparity_device(self, ptr, w, h):
        self._check(self._L.svh_view2d_set_disparity(self._h, ptr, w, h, 1))

    def set_matches(self, matches, inliers, left=True):
        """setMatches: P_MATCH records and one flag per match (0 = outlier)"""
        m = np.ascontiguousarray(matches, P_MATCH).reshape(-1)
        f = np.ascontiguousarray(np.asarray(inliers) != 0, np.uint8).reshape(-1)
        if len(f) != len(m):
            raise SvhError(ERR_BAD_ARG, "one inlier flag per match")
        self._check(self._L.svh_view2d_set_matches(self._h, m.ctypes.data if len(m) else None, len(m),
                                                   f.ctypes.data if len(m) else None, int(bool(left)), 0))

    def set_matches_device(self, m_ptr, n, inlier_ptr, left=True):
        self._check(self._L.svh_view2d_set_matches(self._h, m_ptr, n, inlier_ptr, int(bool(left)), 1))

    def set_matches_indexed(self, matches, inlier_idx, left=True):
        """setMatches with the inliers as getInlierIndices gives them (visualodometrythread.cpp:109-119)"""
        m = np.ascontiguousarray(matches, P_MATCH).reshape(-1)
        idx = np.ascontiguousarray(inlier_idx, np.int32).reshape(-1)
        self._check(self._L.svh_view2d_set_matches_indexed(self._h, m.ctypes.data if len(m) else None, len(m),
                                                           idx.ctypes.data if len(idx) else None, len(idx),
                                                           int(bool(left))))

    def clear_matches(self):
        self._L.svh_view2d_clear_matches(self._h)

    def render(self, device_ptr=None):
        """[height, width, 3] uint8, row 0 on top; with device_ptr the image is written there and None returned"""
        if device_ptr is not None:
            self._check(self._L.svh_view2d_render(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.height, self.width, 3), np.uint8)
        self._check(self._L.svh_view2d_render(self._h, img.ctypes.data, 0))
        return img

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.svh_view2d_destroy(h)

    def __del__(self):
        self.close()


def write_ppm(path, img):
    """binary PPM (P6) of an [h, w, 3] uint8 image"""
    img = np.ascontiguousarray(img, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())
