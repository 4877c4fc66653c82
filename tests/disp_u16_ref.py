"""The 16-bit form of a disparity map (SVH_DISP_U16, stereo-vision_amd/csrc/disp_core.h) restated in plain numpy, the
table of edge values the tests of that form share, and the answers for the table derived by hand.

    u16(d) = 0 when !(d >= 0) (negative, -inf, NaN), otherwise max(1, trunc(min(d * 256, 65535)))
    f32(v) = v / 256 when v != 0, otherwise -1

The restatement works in float64, where d * 256 is exact for every float32 d, and floors (d >= 0 there, so floor is the
truncation of the C conversion).  Expected 16-bit maps everywhere are the float path's maps passed through pack()."""
import numpy as np


def pack(d):
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(d >= 0, np.clip(np.floor(d.astype(np.float64) * 256), 1, 65535), 0)
    return v.astype(np.uint16)


def unpack(v):
    v = np.asarray(v, np.uint16)
    return np.where(v != 0, v.astype(np.float32) / np.float32(256), np.float32(-1)).astype(np.float32)


def _f(x):
    return np.float32(x)


def _next(x, direction):
    return np.nextafter(_f(x), _f(direction), dtype=np.float32)


TOP = _f(255.99609375)          # 65535 / 256: the smallest value that saturates
# (value, answer, why)
TABLE = [
    (_f(-10), 0, "negative"),
    (_f(-1), 0, "negative: the float maps' own 'invalid'"),
    (_f(-1e-30), 0, "negative, however small"),
    (_f(-0.0), 1, "-0.0 >= 0 holds; -0.0 * 256 converts to 0, raised to 1"),
    (_f(0.0), 1, "a valid disparity of zero must not read as invalid"),
    (np.array([1], np.uint32).view(np.float32)[0], 1, "the smallest denormal: 256 times it truncates to 0, raised to 1"),
    (_next(1 / 256, 0), 1, "just below 1/256: truncates to 0, raised to 1"),
    (_f(1 / 256), 1, "exactly one step"),
    (_next(1 / 256, 1), 1, "just above 1/256 truncates to 1"),
    (_next(2 / 256, 0), 1, "just below 2/256 truncates to 1"),
    (_f(2 / 256), 2, "exactly two steps"),
    (_next(TOP, 0), 65534, "one ulp (2^-16) below 65535/256: times 256 is 65535 - 2^-8"),
    (TOP, 65535, "65535/256 exactly"),
    (_next(TOP, 1e9), 65535, "above 65535/256: the clamp, in float, before the conversion"),
    (_f(256), 65535, "saturates"),
    (_f(4095), 65535, "the largest disp_max saturates"),
    (_f(1e9), 65535, "far outside the range of a uint32 after the multiplication: clamped first"),
    (_f(np.inf), 65535, "+inf >= 0 holds; min(inf, 65535)"),
    (_f(-np.inf), 0, "negative"),
    (_f(np.nan), 0, "NaN fails d >= 0"),
]
EDGES = np.array([t[0] for t in TABLE], np.float32)
ANSWERS = np.array([t[1] for t in TABLE], np.uint16)


def content(n, seed):
    """n floats: the edge table repeated (twice, or as much as fits), then seeded values over and around the range"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-8, 300, n).astype(np.float32)
    d[rng.random(n) < 0.2] = -1
    k = min(n, 2 * len(EDGES))
    d[:k] = np.tile(EDGES, 2)[:k]
    return d
