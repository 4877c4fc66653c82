"""The arithmetic of the ground grid (stereo-vision_amd/csrc/grid_core.h; include/svh_grid.h) restated in numpy: fp32 in
the order written -- numpy rounds every float32 operation once --, IEEE division, np.rint (round half even), integer sums.
tests/test_grid.py pins this restatement by hand and compares the header itself with it; tests/test_grid_gpu.py compares
the device with it, bit for bit."""
import numpy as np

import view2d_ref as V2

F = np.float32
LOW, OVERHEAD, OUTSIDE, UNPLACED = range(4)
UNKNOWN, FREE, OBSTACLE, DROP, OVERHANG = 0, 1, 2, 3, 0x80
M_CLASS, M_HEIGHT, M_INTENSITY = range(3)
NO_CELL = np.uint32(0xFFFFFFFF)
KMIN_EMPTY, KMAX_EMPTY = np.uint32(0xFFFFFFFF), np.uint32(0)
NAN_BITS = np.uint32(0x7FC00000)
H_LIMIT = F(1048576.0)
PLANES = ("count", "overhead", "hmin", "hmax", "hmean", "intensity", "cls")


def frame_camera(cam_height):
    return np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, cam_height]], np.float64)


class Params:
    """svh_grid_params with T rounded to float32, as svh_grid_create rounds it"""

    def __init__(self, nx=256, nz=256, cell=0.2, x0=-25.6, z0=0.0, T=None, min_points=3, step=0.2, drop=0.3, clearance=2.0,
                 render_h_lo=0.0, render_h_hi=2.0):
        self.nx, self.nz, self.min_points = int(nx), int(nz), int(min_points)
        self.cell, self.x0, self.z0 = F(cell), F(x0), F(z0)
        self.T = np.asarray(frame_camera(1.65) if T is None else T, np.float64).reshape(3, 4).astype(F)
        self.step, self.drop, self.clearance = F(step), F(drop), F(clearance)
        self.h_lo, self.h_hi = F(render_h_lo), F(render_h_hi)


def key_of(h):
    b = np.ascontiguousarray(h, F).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def height_of(key):
    key = np.ascontiguousarray(key, np.uint32)
    return np.where(key >> np.uint32(31), key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(F)


def q8(val):
    with np.errstate(all="ignore"):
        v = np.ascontiguousarray(val, F)
        lo = np.where(v < F(0), F(0), v)
        hi = np.where(lo > F(1), F(1), lo)
        r = np.rint(hi * F(255.0))
    return np.where(v == v, r, F(0)).astype(np.uint8)


def place(P, pts):
    """per point: fate int32, cell uint32 (NO_CELL: outside or unplaced), and for a low point (else 0) key uint32,
    q int32, v uint8"""
    p = np.ascontiguousarray(pts, F).reshape(-1, 4)
    x, y, z, val = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    with np.errstate(all="ignore"):
        a, b, h = (((t[0] * x + t[1] * y) + t[2] * z) + t[3] for t in P.T)
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(a) & np.isfinite(b) & np.isfinite(h)
        ca, cb = np.floor((a - P.x0) / P.cell), np.floor((b - P.z0) / P.cell)
        assert ca.dtype == F and h.dtype == F
        inside = (ca >= F(0)) & (ca < F(P.nx)) & (cb >= F(0)) & (cb < F(P.nz)) & (np.abs(h) < H_LIMIT)
        h = np.where(h == F(0), F(0), h).astype(F)            # -0.0 -> +0.0
        over = h > P.clearance
        fate = np.where(~fin, UNPLACED, np.where(~inside, OUTSIDE, np.where(over, OVERHEAD, LOW))).astype(np.int32)
        placed, low = fate <= OVERHEAD, fate == LOW
        cell = np.where(placed, np.where(placed, cb, 0).astype(np.int64) * P.nx + np.where(placed, ca, 0).astype(np.int64),
                        int(NO_CELL)).astype(np.uint32)
        hl = np.where(low, h, F(0)).astype(F)
        key = np.where(low, key_of(hl), 0).astype(np.uint32)
        q = np.rint(hl * F(1024.0)).astype(np.int32)
        v = np.where(low, q8(val), 0).astype(np.uint8)
    return fate, cell, key, q, v


def finalise(P, count, overhead, kmin, kmax, hsum, vsum):
    """(hmin, hmax, hmean float32; intensity, cls uint8) of accumulated cells, any shape"""
    count, overhead = np.asarray(count, np.int32), np.asarray(overhead, np.int32)
    has = count > 0
    n = np.where(has, count, 1).astype(np.int64)
    nan = np.full(count.shape, NAN_BITS, np.uint32).view(F)
    hmin = np.where(has, height_of(kmin).reshape(count.shape), nan).astype(F)
    hmax = np.where(has, height_of(kmax).reshape(count.shape), nan).astype(F)
    hmean = np.where(has, (np.asarray(hsum, np.int64).astype(np.float64) / (1024.0 * n.astype(np.float64))).astype(F), nan).astype(F)
    vs = np.asarray(vsum, np.uint64).astype(np.int64)       # at most 255 * 2^31
    intensity = np.where(has, (2 * vs + n) // (2 * n), 0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        cls = np.where(count < P.min_points, UNKNOWN, np.where(hmax > P.step, OBSTACLE, np.where(hmin < -P.drop, DROP, FREE)))
    cls = (cls | np.where(overhead >= P.min_points, OVERHANG, 0)).astype(np.uint8)
    # the NaN planes carry one bit pattern
    for a in (hmin, hmax, hmean):
        a.view(np.uint32)[~has] = NAN_BITS
    return hmin, hmax, hmean, intensity, cls


_height_cache = {}


def height_colour(P, hmax):
    """HEIGHT mode of one cell with COUNT > 0: three bytes"""
    k = (F(hmax).tobytes(), P.h_lo.tobytes(), P.h_hi.tobytes())
    if k not in _height_cache:
        with np.errstate(all="ignore"):
            q = F(F(F(hmax) - P.h_lo) / F(P.h_hi - P.h_lo))
        t = F(0) if q < F(0) else (F(1) if q > F(1) else q)
        _height_cache[k] = tuple(V2.byte_of(c) for c in V2.disparity_colour(F(F(200.0) * t)))
    return _height_cache[k]


def colours(P, mode, count, hmax, intensity, cls):
    """[..., 3] uint8 in cell order (no row flip)"""
    count = np.asarray(count)
    rgb = np.zeros(count.shape + (3,), np.uint8)
    if mode == M_CLASS:
        c = cls & 3
        rgb[c == UNKNOWN] = (32, 32, 32)
        rgb[..., 1] = np.where(c == FREE, 64 + 3 * intensity.astype(np.int64) // 4, rgb[..., 1])
        rgb[c == OBSTACLE] = (255, 0, 0)
        rgb[c == DROP] = (0, 0, 160)
        rgb[..., 2] = np.where(cls & OVERHANG, 255, rgb[..., 2])
    elif mode == M_HEIGHT:
        for idx in zip(*np.nonzero(count > 0)):
            rgb[idx] = height_colour(P, hmax[idx])
    else:
        rgb[...] = np.where(count > 0, intensity, 0)[..., None]
    return rgb


class Grid:
    """the accumulating object: add(points) any number of times, then the planes, the stats, the renders"""

    def __init__(self, P):
        self.P = P
        self.clear()

    def clear(self):
        n = self.P.nx * self.P.nz
        self.count, self.over = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.kmin, self.kmax = np.full(n, KMIN_EMPTY, np.uint32), np.full(n, KMAX_EMPTY, np.uint32)
        self.hsum, self.vsum = np.zeros(n, np.int64), np.zeros(n, np.uint64)
        self.stats = dict(added=0, binned=0, overhead=0, outside=0, unplaced=0)

    def set_window(self, x0, z0):
        self.P.x0, self.P.z0 = F(x0), F(z0)
        self.clear()

    def add(self, pts):
        fate, cell, key, q, v = place(self.P, pts)
        low, ov = fate == LOW, fate == OVERHEAD
        c = cell[low].astype(np.int64)
        np.add.at(self.count, c, 1)
        np.minimum.at(self.kmin, c, key[low])
        np.maximum.at(self.kmax, c, key[low])
        np.add.at(self.hsum, c, q[low].astype(np.int64))
        np.add.at(self.vsum, c, v[low].astype(np.uint64))
        np.add.at(self.over, cell[ov].astype(np.int64), 1)
        for name, f in (("binned", LOW), ("overhead", OVERHEAD), ("outside", OUTSIDE), ("unplaced", UNPLACED)):
            self.stats[name] += int((fate == f).sum())
        self.stats["added"] += len(fate)
        return self

    def planes(self):
        """dict of [nz, nx] arrays: count, overhead, hmin, hmax, hmean, intensity, cls"""
        sh = (self.P.nz, self.P.nx)
        fin = finalise(self.P, self.count, self.over, self.kmin, self.kmax, self.hsum, self.vsum)
        return dict(zip(PLANES, [a.reshape(sh) for a in (self.count.copy(), self.over.copy()) + fin]))

    def render(self, mode):
        """[nz, nx, 3] uint8, row 0 = ib nz - 1"""
        pl = self.planes()
        return colours(self.P, mode, pl["count"], pl["hmax"], pl["intensity"], pl["cls"])[::-1].copy()


def same_planes(a, b):
    """bit for bit, NaN patterns included"""
    for k in PLANES:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True
