"""numpy restatement of the map view (include/svh_view.h; the C++ form is stereo-vision_amd/csrc/view_core.h): the list
semantics of View3D::addPoints, the render of paintGL and the pose loop of playPoses as this project defines them.

Every fp32 operation is an explicit np.float32 operation in the order view_core.h performs it (on arrays where many
primitives share it: the same operations, element by element); the double matrices use Python floats and math.sin /
math.cos, i.e. the C library the product calls.  The depth and overlay layers are plain loops in draw order: a pixel
of the depth layer is replaced only by a strictly smaller depth (GL_LESS, first drawn wins a tie), a pixel of the
overlay by whatever is drawn later.  Equality with an OpenGL implementation is not claimed anywhere."""
import math

import numpy as np

F = np.float32
GRID_SEGS = 162
RED, GREEN, BLUE, YELLOW = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)
PALETTE = [(0, 0, 0), RED, GREEN, BLUE, YELLOW]
FLT_MAX = F(np.finfo(np.float32).max)

DEFAULT_POSE = (F(-1.5), F(180), F(0), F(0), F(0), F(-1.5))   # zoom, rotx, roty, tx, ty, tz (view3d.cpp:13-18)


# ---------------------------------------------------------------------------------------------------- host, double
def mul4(A, B):
    return [[((A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c]) + A[r][3] * B[3][c] for c in range(4)]
            for r in range(4)]


def translate4(x, y, z):
    T = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    T[0][3], T[1][3], T[2][3] = x, y, z
    return T


class Frame:
    """MVP (16 float32, row major), the image size and glViewport's square"""

    def __init__(self, pose, W, H):
        zoom, rotx, roty, tx, ty, tz = [float(F(v)) for v in pose]
        ax, ay = rotx * math.pi / 180.0, roty * math.pi / 180.0
        cx, sx, cy, sy = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay)
        Rx, Ry = translate4(0.0, 0.0, 0.0), translate4(0.0, 0.0, 0.0)
        Rx[1][1], Rx[1][2], Rx[2][1], Rx[2][2] = cx, -sx, sx, cx
        Ry[0][0], Ry[0][2], Ry[2][0], Ry[2][2] = cy, sy, -sy, cy
        M = mul4(mul4(mul4(translate4(0.0, 0.0, zoom), Rx), Ry), translate4(tx, ty, tz))
        half = 45.0 / 2.0 * math.pi / 180.0
        ct, zn, zf = math.cos(half) / math.sin(half), 0.1, 10000.0
        P = [[0.0] * 4 for _ in range(4)]
        P[0][0] = ct / 1.0
        P[1][1] = ct
        P[2][2] = -(zf + zn) / (zf - zn)
        P[2][3] = -2.0 * zn * zf / (zf - zn)
        P[3][2] = -1.0
        self.m = np.array(mul4(P, M), np.float64).astype(np.float32).ravel()
        self.W, self.H = W, H
        self.side = max(W, H)
        self.ox = -((self.side - W) // 2)    # C division of (W - side) / 2: towards zero
        self.oy = -((self.side - H) // 2)


def make_camera(H_total, s, keyframe):
    """addCamera: (10 x 3 float32 outline, keyframe)"""
    Ht = np.asarray(H_total, np.float64)
    s = float(F(s))
    h, o = 0.5 * s, 1.0 * s
    C = [(-h, -h, o), (h, -h, o), (h, h, o), (-h, h, o), (-h, -h, o), (0.0, 0.0, 0.0), (h, -h, o), (h, h, o),
         (0.0, 0.0, 0.0), (-h, h, o)]
    p = np.zeros((10, 3), np.float32)
    for i in range(10):
        for j in range(3):
            p[i, j] = F(((float(Ht[j, 0]) * C[i][0] + float(Ht[j, 1]) * C[i][1]) + float(Ht[j, 2]) * C[i][2])
                        + float(Ht[j, 3]) * 1.0)
    return p, bool(keyframe)


def play_sequence(poses):
    """playPoses: the list of poses (6 float32 each) that are rendered"""
    out = []
    step = F(0.02)
    for i in range(len(poses) - 1):
        a, b = [F(v) for v in poses[i]], [F(v) for v in poses[i + 1]]
        pos = F(0)
        while pos <= F(1):
            pos2 = (1 + math.sin(-math.pi / 2 + float(pos) * math.pi)) / 2
            out.append(tuple(F(float(a[k]) + float(F(b[k] - a[k])) * pos2) for k in range(6)))
            pos = F(pos + step)
    return out


def human_poses(pose):
    a, b = list(pose), list(pose)
    a[2], b[2] = F(F(pose[2]) - F(45)), F(F(pose[2]) + F(45))
    return [tuple(a), tuple(b), tuple(a)]


# ------------------------------------------------------------------------------------------------ per primitive, fp32
def clip_coords(m, x, y, z):
    """x, y, z: float32 scalars or arrays; rows of m as ((m0 x + m1 y) + m2 z) + m3"""
    return [F(F(F(F(m[4 * r] * x) + F(m[4 * r + 1] * y)) + F(m[4 * r + 2] * z)) + m[4 * r + 3]) for r in range(4)]


def in_volume(c):
    w = c[3]
    ok = (w > 0) & (w <= FLT_MAX)
    for k in range(3):
        ok = ok & (-w <= c[k]) & (c[k] <= w)
    return ok


def to_window(f, c):
    half = F(0.5)
    nx, ny, nz = c[0] / c[3], c[1] / c[3], c[2] / c[3]
    xw = (nx * half + half) * F(f.side) + F(f.ox)
    yw = (ny * half + half) * F(f.side) + F(f.oy)
    zw = nz * half + half
    return xw, yw, zw


def depth_bits(zw):
    zw = np.asarray(zw, np.float32)
    return np.where(zw > 0, zw.view(np.uint32), np.uint32(0)).astype(np.int64)


def grey_of(val):
    val = np.asarray(val, np.float32)
    with np.errstate(all="ignore"):
        lo = np.where(val < 0, F(0), val)
        hi = np.where(lo > 1, F(1), lo)
        g = np.floor(hi * F(255.0) + F(0.5))
        return np.where(val == val, g, F(0)).astype(np.uint8)


def point_windows(f, xyz, round_half=True):
    """(drawn mask, ix, iy, depth bits) of [n, 3] float32 points"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = clip_coords(f.m, xyz[:, 0], xyz[:, 1], xyz[:, 2])
        ok = in_volume(c)
        c = [np.where(ok, v, F(1)) for v in c]
        xw, yw, zw = to_window(f, c)
        h = F(0.5) if round_half else F(0)
        ix = np.floor(xw + h).astype(np.int64)
        iy = np.floor(yw + h).astype(np.int64)
    return ok, ix, iy, depth_bits(zw)


def finite(v):
    return abs(v) <= FLT_MAX


def clip_segment(A, B):
    """Liang-Barsky against -x, +x, -y, +y, -z, +z; A, B lists of 4 float32; returns the clipped ends or None"""
    for i in range(4):
        if not finite(A[i]) or not finite(B[i]):
            return None
    t0, t1 = F(0), F(1)
    for pl in range(6):
        ax = pl >> 1
        da = F(A[3] - A[ax]) if pl & 1 else F(A[3] + A[ax])
        db = F(B[3] - B[ax]) if pl & 1 else F(B[3] + B[ax])
        if da < 0 and db < 0:
            return None
        if da < 0:
            t = F(da / F(da - db))
            t0 = t if t > t0 else t0
        elif db < 0:
            t = F(da / F(da - db))
            t1 = t if t < t1 else t1
    if not t0 <= t1:
        return None
    a, b = [], []
    for i in range(4):
        d = F(B[i] - A[i])
        a.append(F(A[i] + F(t0 * d)))
        b.append(F(A[i] + F(t1 * d)))
    if not (a[3] > 0 and b[3] > 0 and finite(a[3]) and finite(b[3])):
        return None
    return a, b


def first_cell(v, lim):
    c = np.ceil(F(v - F(0.5)))
    return (int(c) if c < F(lim) else lim) if c > 0 else 0


def segment_pixels(f, a, b, wide):
    """[(window x, window y, depth bits)] in the order they are plotted"""
    with np.errstate(all="ignore"):
        A = clip_coords(f.m, F(a[0]), F(a[1]), F(a[2]))
        B = clip_coords(f.m, F(b[0]), F(b[1]), F(b[2]))
        cl = clip_segment(A, B)
        if cl is None:
            return []
        xa, ya, za = to_window(f, cl[0])
        xb, yb, zb = to_window(f, cl[1])
        dx, dy, dz = F(xb - xa), F(yb - ya), F(zb - za)
        xmajor = abs(dx) >= abs(dy)
        ma, mb, dm = (xa, xb, dx) if xmajor else (ya, yb, dy)
        na, dn = (ya, dy) if xmajor else (xa, dx)
        if not dm != 0 or not finite(dm):
            return []
        lim, nlim = (f.W, f.H) if xmajor else (f.H, f.W)
        p0, p1 = first_cell(min(ma, mb), lim), first_cell(max(ma, mb), lim)
        if p1 <= p0:
            return []
        p = np.arange(p0, p1, dtype=np.int64)
        t = ((p.astype(np.float32) + F(0.5)) - ma) / dm
        nf = np.floor(na + t * dn)
        z = za + t * dz
        keep = (nf >= F(-2)) & (nf <= F(F(nlim) + F(1)))
        zb_ = depth_bits(z)
    out = []
    w = 1 if wide else 0
    for k in range(len(p)):
        if not keep[k]:
            continue
        q = int(nf[k])
        for d in range(-w, w + 1):
            x, y = (int(p[k]), q + d) if xmajor else (q + d, int(p[k]))
            if 0 <= x < f.W and 0 <= y < f.H:
                out.append((x, y, int(zb_[k])))
    return out


def grid_segments():
    out = []
    r, h = F(200), F(2)
    x = F(-200)
    while float(x) <= float(r) + 0.001:
        out.append(((x, h, -r), (x, h, r)))
        out.append(((-r, h, x), (r, h, x)))
        x = F(x + F(5))
    assert len(out) == GRID_SEGS
    return out


# --------------------------------------------------------------------------------------------------------- the object
class View:
    """The restated object: lists (float32 [n, 4] arrays in sequence order), cameras, pose, flags."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.lists, self.cams = [], []
        self.pose = DEFAULT_POSE
        self.show_cams, self.show_grid, self.white = True, True, False

    def add_points(self, lists):
        lists = [np.asarray(a, np.float32).reshape(-1, 4) for a in lists]
        if len(lists) > 1 and self.lists:
            self.lists.pop()
        self.lists += lists[max(len(lists) - 2, 0):]

    def add_camera(self, H_total, s=0.1, keyframe=True):
        self.cams.append(make_camera(H_total, s, keyframe))

    def clear(self):
        self.lists, self.cams = [], []

    def count(self, what):
        return (len(self.lists), sum(len(a) for a in self.lists), len(self.cams))[what]

    def overlay_segments(self):
        """(a, b, colour, wide) in paintGL's order"""
        out, col = [], RED
        for p, key in self.cams:
            col = RED if key else YELLOW
            out += [(p[i], p[i + 1], col, False) for i in range(9)]
        out += [(self.cams[c][0][5], self.cams[c + 1][0][5], col, False) for c in range(len(self.cams) - 1)]
        s, o = F(0.3), F(0)
        out += [((o, o, o), (s, o, o), RED, True), ((o, o, o), (o, s, o), GREEN, True), ((o, o, o), (o, o, s), BLUE, True)]
        return out

    def render(self):
        f = Frame(self.pose, self.W, self.H)
        W, H = self.W, self.H
        EMPTY = (1 << 64) - 1
        depth = [EMPTY] * (W * H)          # keys depth bits << 32 | draw index, image order (row 0 on top)
        overlay = [0] * (W * H)            # index into PALETTE, 0 = nothing
        pts = np.concatenate(self.lists) if self.lists else np.zeros((0, 4), np.float32)

        def depth_plot(x, y, zb, index):
            at = (H - 1 - y) * W + x
            key = (zb << 32) | index
            if key < depth[at]:            # GL_LESS; at equal depth the smaller draw index was drawn first
                depth[at] = key

        if self.show_grid:
            for k, (a, b) in enumerate(grid_segments()):
                for x, y, zb in segment_pixels(f, a, b, False):
                    depth_plot(x, y, zb, k)
        ok, ix, iy, zb = point_windows(f, pts[:, :3])
        for i in np.flatnonzero(ok):
            for y in (int(iy[i]) - 1, int(iy[i])):
                for x in (int(ix[i]) - 1, int(ix[i])):
                    if 0 <= x < W and 0 <= y < H:
                        depth_plot(x, y, int(zb[i]), GRID_SEGS + int(i))
        anchor = None
        if self.show_cams:
            for a, b, col, wide in self.overlay_segments():
                for x, y, _ in segment_pixels(f, a, b, wide):
                    overlay[(H - 1 - y) * W + x] = PALETTE.index(col)
            anchor = GRID_SEGS + len(pts)
            tx, ty, tz = F(self.pose[3]), F(self.pose[4]), F(self.pose[5])
            ok, ix, iy, zb = point_windows(f, np.array([[-tx, -ty, -tz]], np.float32), round_half=False)
            if ok[0]:
                for y in range(int(iy[0]) - 1, int(iy[0]) + 2):
                    for x in range(int(ix[0]) - 1, int(ix[0]) + 2):
                        if 0 <= x < W and 0 <= y < H:
                            depth_plot(x, y, int(zb[0]), anchor)
        # resolve: the anchor where it won, else the overlay, else the depth winner's colour, else the background
        key = np.array(depth, np.uint64)
        has = key != np.uint64(EMPTY)
        idx = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        img = np.full((H * W, 3), 255 if self.white else 0, np.uint8)
        img[has & (idx < GRID_SEGS)] = 128
        from_point = has & (idx >= GRID_SEGS) & (idx != (-1 if anchor is None else anchor))
        img[from_point] = grey_of(pts[:, 3])[idx[from_point] - GRID_SEGS][:, None]
        code = np.array(overlay, np.int64)
        img[code > 0] = np.array(PALETTE, np.uint8)[code[code > 0]]
        if anchor is not None:
            img[has & (idx == anchor)] = RED
        return img.reshape(H, W, 3)

    def play_poses(self, poses):
        """the images of playPoses, one per pose of play_sequence"""
        out = []
        for q in play_sequence(poses):
            self.pose = q
            out.append(self.render())
        return out
