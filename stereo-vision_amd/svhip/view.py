"""ctypes binding of the map view in libsvhip.so (C-ABI: include/svh_view.h): what stereomapper's View3D does with the
point lists and poses MainDialog hands it (maindialog.cpp:602-606, view3d.cpp), accumulated and rendered on the device."""
import ctypes as C

import numpy as np

from . import ERR_BAD_ARG, SvhError, last_error, lib

LISTS, POINTS, CAMERAS, CAPACITY = 0, 1, 2, 3


class Pose(C.Structure):
    """svh_view_pose: View3D::pose"""
    _fields_ = [("zoom", C.c_float), ("rotx", C.c_float), ("roty", C.c_float), ("tx", C.c_float), ("ty", C.c_float),
                ("tz", C.c_float)]

    def astuple(self):
        return tuple(np.float32(getattr(self, n)) for n, _ in self._fields_)


class Flags(C.Structure):
    """svh_view_flags"""
    _fields_ = [("show_cams", C.c_int32), ("show_grid", C.c_int32), ("white", C.c_int32)]


class ThinStats(C.Structure):
    """svh_view_thin_stats"""
    _fields_ = [("before", C.c_int64), ("after", C.c_int64), ("unplaced", C.c_int64)]

    def __repr__(self):
        return "ThinStats(before=%d, after=%d, unplaced=%d)" % (self.before, self.after, self.unplaced)


def _bind():
    L = lib()
    if not getattr(L, "_view_bound", False):
        L.svh_view_create.restype = C.c_void_p
        L.svh_view_create.argtypes = [C.c_int32, C.c_int32]
        L.svh_view_destroy.argtypes = [C.c_void_p]
        L.svh_view_destroy.restype = None
        L.svh_view_clear.argtypes = [C.c_void_p]
        L.svh_view_clear.restype = None
        L.svh_view_resize.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.svh_view_pose_default.argtypes = [C.POINTER(Pose)]
        L.svh_view_pose_default.restype = None
        L.svh_view_set_pose.argtypes = [C.c_void_p, C.POINTER(Pose)]
        L.svh_view_set_flags.argtypes = [C.c_void_p, C.POINTER(Flags)]
        L.svh_view_add_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.svh_view_add_map.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_view_add_camera.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int32]
        L.svh_view_count.argtypes = [C.c_void_p, C.c_int32]
        L.svh_view_count.restype = C.c_int64
        L.svh_view_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_view_play_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32]
        L.svh_view_play_poses.restype = C.c_int64
        L.svh_view_play_sequence.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        L.svh_view_play_sequence.restype = C.c_int64
        L.svh_view_thin.argtypes = [C.c_void_p, C.c_float, C.POINTER(ThinStats)]
        L.svh_view_get_points.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32]
        L.svh_view_get_points.restype = C.c_int64
        L.svh_view_list_len.argtypes = [C.c_void_p, C.c_int32]
        L.svh_view_list_len.restype = C.c_int64
        L.svh_test_thin_keys.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L._view_bound = True
    return L


def thin_keys(xyzv, voxel):
    """(key uint64 [n], home uint32 [n], capacity): the thinning's arithmetic (csrc/view_thin_core.h) evaluated on the
    host for n points -- the library's test entry svh_test_thin_keys; needs no device.  A point that falls into no voxel
    has the key 2^64 - 1 and the home 2^32 - 1; the homes are those of the table a store of n points gets"""
    L = _bind()
    p = np.ascontiguousarray(xyzv, np.float32).reshape(-1, 4)
    key, home, cap = np.zeros(len(p), np.uint64), np.zeros(len(p), np.uint32), C.c_uint64(0)
    rc = L.svh_test_thin_keys(p.ctypes.data if len(p) else None, len(p), voxel, key.ctypes.data, home.ctypes.data, C.byref(cap))
    if rc < 0:
        raise SvhError(int(rc), last_error())
    return key, home, int(cap.value)


def default_pose():
    p = Pose()
    _bind().svh_view_pose_default(C.byref(p))
    return p


def _pose_array(poses):
    return (Pose * len(poses))(*[p if isinstance(p, Pose) else Pose(*p) for p in poses])


def play_sequence(poses):
    """the poses play_poses renders (playPoses' loop, view3d.cpp:418-458), as a list of Pose; needs no device"""
    L = _bind()
    arr = _pose_array(poses)
    n = L.svh_view_play_sequence(arr, len(poses), None, 0)
    if n < 0:
        raise SvhError(int(n), last_error())
    out = (Pose * max(int(n), 1))()
    L.svh_view_play_sequence(arr, len(poses), out, n)
    return [out[k] for k in range(int(n))]


def human_poses(pose):
    """recordHuman's three poses around `pose` (view3d.cpp:403-414)"""
    a, b = Pose(*pose.astuple()), Pose(*pose.astuple())
    a.roty = np.float32(a.roty) - np.float32(45)
    b.roty = np.float32(b.roty) + np.float32(45)
    return [a, b, a]


class View:
    """v = View(width, height); v.add_camera(H_total); v.add_map(mapper) or v.add_points([...]); img = v.render()"""

    def __init__(self, width, height):
        self._L = _bind()
        self._h = self._L.svh_view_create(width, height)
        if not self._h:
            raise SvhError(ERR_BAD_ARG, last_error())
        self.width, self.height = width, height
        self.pose = default_pose()
        self.flags = Flags(1, 1, 0)

    def _check(self, rc):
        if rc < 0:
            raise SvhError(int(rc), last_error())
        return rc

    def resize(self, width, height):
        self._check(self._L.svh_view_resize(self._h, width, height))
        self.width, self.height = width, height

    def set_pose(self, pose):
        pose = pose if isinstance(pose, Pose) else Pose(*pose)
        self._check(self._L.svh_view_set_pose(self._h, C.byref(pose)))
        self.pose = pose

    def set_flags(self, show_cams=None, show_grid=None, white=None):
        f = Flags(self.flags.show_cams, self.flags.show_grid, self.flags.white)
        for name, val in (("show_cams", show_cams), ("show_grid", show_grid), ("white", white)):
            if val is not None:
                setattr(f, name, int(bool(val)))
        self._check(self._L.svh_view_set_flags(self._h, C.byref(f)))
        self.flags = f

    def add_points(self, lists):
        """addPoints: a sequence of [n, 4] float32 arrays (x, y, z, val) on the host"""
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in lists]
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if len(a) else None for a in arrs])
        n = (C.c_int64 * max(len(arrs), 1))(*[len(a) for a in arrs])
        self._check(self._L.svh_view_add_points(self._h, ptrs, n, len(arrs), 0))

    def add_points_device(self, ptrs, counts):
        """the same with raw device addresses (ints)"""
        p = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        n = (C.c_int64 * max(len(ptrs), 1))(*counts)
        self._check(self._L.svh_view_add_points(self._h, p, n, len(ptrs), 1))

    def add_map(self, mapper):
        """the lists of the frame mapper.add has just processed, device to device (mapper: svhip.mapper.Mapper)"""
        self._check(self._L.svh_view_add_map(self._h, mapper._h))

    def add_camera(self, H_total, s=0.1, keyframe=True):
        H = np.ascontiguousarray(H_total, np.float64)
        if H.shape != (4, 4):
            raise SvhError(ERR_BAD_ARG, "H_total must be 4x4")
        self._check(self._L.svh_view_add_camera(self._h, H.ctypes.data, s, int(bool(keyframe))))

    def count(self, what):
        return int(self._L.svh_view_count(self._h, what))

    def clear(self):
        self._L.svh_view_clear(self._h)

    def thin(self, voxel):
        """keep the first-drawn point of every cube of side `voxel`; ThinStats (before, after, unplaced)"""
        st = ThinStats()
        self._check(self._L.svh_view_thin(self._h, voxel, C.byref(st)))
        return st

    def list_len(self, i):
        return int(self._check(self._L.svh_view_list_len(self._h, i)))

    def points(self, list=-1, cap=None, device_ptr=None):
        """the points of one list, or (-1) of the whole store, as [n, 4] float32 (x, y, z, val); at most `cap` of them.
        With device_ptr they are written there and their number in the list is returned"""
        n = int(self._check(self._L.svh_view_get_points(self._h, list, None, 0, 0)))
        m = n if cap is None else min(n, cap)
        if device_ptr is not None:
            return int(self._check(self._L.svh_view_get_points(self._h, list, device_ptr, m, 1)))
        out = np.zeros((m, 4), np.float32)
        self._check(self._L.svh_view_get_points(self._h, list, out.ctypes.data if m else None, m, 0))
        return out

    def render(self, device_ptr=None):
        """[height, width, 3] uint8, row 0 on top; with device_ptr the image is written there and None returned"""
        if device_ptr is not None:
            self._check(self._L.svh_view_render(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.height, self.width, 3), np.uint8)
        self._check(self._L.svh_view_render(self._h, img.ctypes.data, 0))
        return img

    def play_poses(self, poses, cap=None):
        """playPoses: (frames, images [min(frames, cap), height, width, 3]); the pose afterwards is the last rendered"""
        arr = _pose_array(poses)
        frames = 51 * max(len(poses) - 1, 0)
        keep = frames if cap is None else min(cap, frames)
        out = np.zeros((keep, self.height, self.width, 3), np.uint8)
        n = self._check(self._L.svh_view_play_poses(self._h, arr, len(poses), out.ctypes.data if keep else None, keep, 0))
        if n > 0:
            self.pose = play_sequence(poses)[-1]
        return int(n), out

    def record_human(self, cap=None):
        """recordHuman: the fly-through -45 deg .. +45 deg .. -45 deg around the current pose"""
        return self.play_poses(human_poses(self.pose), cap)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.svh_view_destroy(h)

    def __del__(self):
        self.close()


def write_ppm(path, img):
    """binary PPM (P6) of an [h, w, 3] uint8 image"""
    img = np.ascontiguousarray(img, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def write_ply(path, pts):
    """binary little-endian PLY of [n, 4] float32 points: the float properties x, y, z, val"""
    pts = np.ascontiguousarray(pts, "<f4").reshape(-1, 4)
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                b"property float z\nproperty float val\nend_header\n" % len(pts))
        f.write(pts.tobytes())
