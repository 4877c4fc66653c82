"""numpy restatement of the rectification arithmetic (include/svh_rectify.h, stereo-vision_amd/csrc/rectify_core.h):
the undistort-and-rectify maps in float64, their float32 form, the 1/32-pixel fixed-point sample and the 8-bit bilinear
remap with the two border modes.  Every line is one IEEE operation per element in the order the header states (numpy
fuses nothing), so the C++ core and the kernels are expected to agree with it bit for bit.

It is a RESTATEMENT, not the reference: OpenCV is not available here, and tests/golden/rectify.npz is produced by this
file.  What pins the arithmetic independently are the hand-derived known answers and the round trip of
tests/test_rectify.py."""
import os
import struct

import numpy as np

import helpers as H

GOLDEN = os.path.join(H.GOLDEN, "rectify.npz")
WRAP, ZERO = 0, 1
NO_SAMPLE = -2 ** 31


def camera(K=None, D=None, R=None, P=None):
    """one svh_rectify_camera as a dict of float64 arrays (defaults: K = R = I, P = [I | 0], D = 0)"""
    P34 = np.zeros((3, 4))
    P34[:, :3] = np.eye(3)
    return {"K": np.array(np.eye(3) if K is None else K, np.float64).reshape(3, 3),
            "D": np.array(np.zeros(5) if D is None else D, np.float64).reshape(5),
            "R": np.array(np.eye(3) if R is None else R, np.float64).reshape(3, 3),
            "P": np.array(P34 if P is None else P, np.float64).reshape(3, 4)}


def inverse_pr(cam):
    """ir = (P[:3,:3] R)^-1 by the adjugate over the determinant, None when singular"""
    P, R = cam["P"], cam["R"]
    A = np.zeros(9)
    with np.errstate(all="ignore"):
        return _inverse(A, P, R)


def _inverse(A, P, R):
    for r in range(3):
        for c in range(3):
            A[3 * r + c] = (P[r, 0] * R[0, c] + P[r, 1] * R[1, c]) + P[r, 2] * R[2, c]
    c0 = A[4] * A[8] - A[5] * A[7]
    c1 = A[5] * A[6] - A[3] * A[8]
    c2 = A[3] * A[7] - A[4] * A[6]
    det = (A[0] * c0 + A[1] * c1) + A[2] * c2
    if det == 0.0 or not np.isfinite(det):
        return None
    adj = np.array([c0, A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                    c1, A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                    c2, A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]])
    return adj / det


def maps64(cam, dw, dh):
    """(u, v) in float64 for every output pixel, [dh, dw] each"""
    ir = inverse_pr(cam)
    assert ir is not None
    K, (k1, k2, p1, p2, k3) = cam["K"], cam["D"]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    i, j = np.mgrid[0:dh, 0:dw].astype(np.float64)
    with np.errstate(all="ignore"):
        X = (j * ir[0] + i * ir[1]) + ir[2]
        Y = (j * ir[3] + i * ir[4]) + ir[5]
        W = (j * ir[6] + i * ir[7]) + ir[8]
        w = 1.0 / W
        x = X * w
        y = Y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        u = fx * ((x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)) + cx
        v = fy * ((y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2) + cy
    return u, v


def maps(cam, dw, dh):
    u, v = maps64(cam, dw, dh)
    with np.errstate(all="ignore"):
        return u.astype(np.float32), v.astype(np.float32)


def fixed(m, size, border):
    """sx (or sy) of a float32 map: rint(m * 32) with ties to even, reduced for WRAP; NO_SAMPLE where it yields 0"""
    with np.errstate(all="ignore"):
        ok = np.abs(m) < np.float32(1048576.0)          # (False for NaN)
        s = np.rint(np.where(ok, m, np.float32(0)) * np.float32(32.0)).astype(np.int64)
    if border == WRAP:
        s = (np.mod(s >> 5, size) << 5) | (s & 31)
    return s, ok


def remap(S, mx, my, border):
    """S: [sh, sw] uint8 (any strides) -> [dh, dw] uint8"""
    sh, sw = S.shape
    sx, okx = fixed(mx, sw, border)
    sy, oky = fixed(my, sh, border)
    ok = okx & oky
    x0, a, y0, b = sx >> 5, sx & 31, sy >> 5, sy & 31

    def tap(y, x):
        if border == WRAP:
            y, x = np.mod(y, sh), np.mod(x, sw)
            inside = ok
        else:
            inside = ok & (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        return np.where(inside, S[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64), 0)

    out = ((32 - a) * (32 - b) * tap(y0, x0) + a * (32 - b) * tap(y0, x0 + 1) + (32 - a) * b * tap(y0 + 1, x0)
           + a * b * tap(y0 + 1, x0 + 1) + 512) >> 10
    return np.where(ok, out, 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# the independent round trip: shares nothing with maps64
# ---------------------------------------------------------------------------------------------------------------
def round_trip(cam, u, v, rounds=20):
    """undistort (u, v) by fixed-point iteration of the distortion model, rotate by R, project by P: -> (j, i)"""
    K, (k1, k2, p1, p2, k3) = cam["K"], cam["D"]
    xd = (u - K[0, 2]) / K[0, 0]
    yd = (v - K[1, 2]) / K[1, 1]
    x, y = xd.copy(), yd.copy()
    for _ in range(rounds):
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (xd - dx) / radial
        y = (yd - dy) / radial
    ray = np.stack([x, y, np.ones_like(x)], -1)          # in the raw camera
    rect = ray @ cam["R"].T                              # rotate by R
    pix = rect @ cam["P"][:, :3].T
    return pix[..., 0] / pix[..., 2], pix[..., 1] / pix[..., 2]


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
def source(w, h, seed=0):
    """a deterministic source of texture with no two equal neighbours in a row (no generator state involved)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return ((x * 37 + y * 101 + (x * y + seed * 7919) % 61 * 3 + ((x >> 3) ^ (y >> 2)) * 11) & 255).astype(np.uint8)


def distinct_source(w, h):
    """distinct bytes (w * h <= 256), for the hand-derived cases"""
    assert w * h <= 256
    return ((np.arange(w * h) * 37 + 11) % 256).astype(np.uint8).reshape(h, w)


def shifted(cx, cy):
    P = np.zeros((3, 4))
    P[:, :3] = np.eye(3)
    P[0, 2], P[1, 2] = cx, cy
    return camera(P=P)


HAND_W, HAND_H = 16, 12


def hand_cases():
    """name -> camera; source HAND_W x HAND_H of distinct bytes, destination of the same size, D = 0"""
    w0 = camera(P=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 1, -2, 0]])    # W = (i - 1) / 2: zero on row 1
    return [("identity", camera()), ("shift", shifted(-3.0, -2.0)), ("half", shifted(-0.5, 0.0)),
            ("tie1", shifted(-1.0 / 64, 0.0)), ("tie3", shifted(-3.0 / 64, 0.0)), ("w0", w0)]


def rodrigues(rx, ry, rz):
    t = np.sqrt(rx * rx + ry * ry + rz * rz)
    k = np.array([[0, -rz, ry], [rz, 0, -rx], [-ry, rx, 0]]) / t
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


def generic_camera(sw, sh, dw, dh, zoom=0.8, off=(0.0, 0.0)):
    """a distorted, slightly rotated camera whose rectified view is wider than the source, so borders are sampled"""
    f = 0.9 * max(sw, sh, 2)
    K = [[f, 0, sw / 2 + 0.3], [0, f * 1.01, sh / 2 - 0.2], [0, 0, 1]]
    fp = zoom * f * max(dw, 2) / max(sw, 2)
    P = [[fp, 0, dw / 2 + off[0], 0], [0, fp, dh / 2 + off[1], 0], [0, 0, 1, 0]]
    return camera(K, [-0.2, 0.05, 1e-3, -5e-4, 0.01], rodrigues(0.01, -0.02, 0.015), P)


# destinations at the edges of k_rect_remap's tiling (a wave covers 256 columns minus the row's misalignment, a
# workgroup four rows), each with a source smaller ("s") or larger ("l") than itself
SHAPES = [(1, 1, "l"), (3, 2, "s"), (61, 7, "l"), (63, 1, "s"), (64, 8, "l"), (65, 9, "s"), (65, 9, "l"),
          (253, 5, "s"), (255, 15, "l"), (256, 16, "s"), (257, 17, "l"), (257, 17, "s"), (1242, 5, "l")]


def shape_cases():
    """name -> (camera, sw, sh, dw, dh)"""
    out = []
    for dw, dh, kind in SHAPES:
        sw, sh = (dw + 7, dh + 5) if kind == "l" else (max(1, (dw * 3 + 4) // 5), max(1, (dh * 3 + 4) // 5))
        out.append(("shape_%dx%d_%s" % (dw, dh, kind), (generic_camera(sw, sh, dw, dh), sw, sh, dw, dh)))
    # maps wholly outside the source, and maps that straddle the wrap seam in both axes
    out.append(("outside", (shifted(-500.0, -300.0), 40, 30, 70, 11)))
    out.append(("seam", (shifted(-30.25, -21.5), 40, 30, 70, 23)))
    return out


# the KITTI-like rig: a 2011_09_26-style calibration of the two gray cameras, as plain numbers
RIG_SRC, RIG_DST = (1392, 512), (1242, 375)
RIG = [
    camera(K=[9.842439e+02, 0, 6.900000e+02, 0, 9.808141e+02, 2.331966e+02, 0, 0, 1],
           D=[-3.728755e-01, 2.037299e-01, 2.219027e-03, 1.383707e-03, -7.233722e-02],
           R=[9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03,
              7.402527e-03, 4.351614e-03, 9.999631e-01],
           P=[7.215377e+02, 0, 6.095593e+02, 0, 0, 7.215377e+02, 1.728540e+02, 0, 0, 0, 1, 0]),
    camera(K=[9.895267e+02, 0, 7.020000e+02, 0, 9.878386e+02, 2.455590e+02, 0, 0, 1],
           D=[-3.644661e-01, 1.790019e-01, 1.148107e-03, -6.298563e-04, -5.314062e-02],
           R=[9.996878e-01, -8.976826e-03, 2.331651e-02, 8.876121e-03, 9.999508e-01, 4.418952e-03,
              -2.335503e-02, -4.210612e-03, 9.997184e-01],
           P=[7.215377e+02, 0, 6.095593e+02, -3.875744e+02, 0, 7.215377e+02, 1.728540e+02, 0, 0, 0, 1, 0]),
]
RIG_WINDOW = (1140, 330, 96, 40)   # x0, y0, w, h: the lower right, where the distortion is largest


def window(a):
    x0, y0, w, h = RIG_WINDOW
    return a[y0:y0 + h, x0:x0 + w]


def load_golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------------------
# the stand-alone check program tests/rectify/rectify_core_check.cpp
# ---------------------------------------------------------------------------------------------------------------
def write_job(path, cam, S, dw, dh, border, stride=None):
    sh, sw = S.shape
    stride = sw if stride is None else stride
    buf = np.zeros((sh, stride), np.uint8)
    buf[:, :sw] = S
    with open(path, "wb") as fh:
        fh.write(struct.pack("<6i", sw, sh, stride, dw, dh, border))
        fh.write(np.concatenate([cam["K"].ravel(), cam["D"], cam["R"].ravel(), cam["P"].ravel()]).astype("<f8").tobytes())
        fh.write(buf.tobytes())


def parse_run(blob, dw, dh):
    """-> None when the program found P R singular, else (mx, my, out)"""
    ok, = struct.unpack_from("<i", blob, 0)
    if not ok:
        return None
    n = dw * dh
    assert len(blob) == 4 + 9 * n
    mx = np.frombuffer(blob, "<f4", n, 4).reshape(dh, dw)
    my = np.frombuffer(blob, "<f4", n, 4 + 4 * n).reshape(dh, dw)
    return mx, my, np.frombuffer(blob, np.uint8, n, 4 + 8 * n).reshape(dh, dw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
