"""Shared by the tests of the device-frame lockstep entries (tests/test_lockstep_device_gpu.py,
tests/test_map_lockstep_gpu.py): device allocations that hold a frame at a byte offset and a pitch, per-object variants
of the golden quad, the lockstep counters, and what is compared between two Matcher / visual-odometry objects."""
import ctypes as C
import os

import numpy as np

import helpers as H


def hip_runtime():
    return C.CDLL("libamdhip64.so")


class Dev:
    """a device allocation holding a copy of a host array"""

    def __init__(self, hip, a):
        self.hip, self.p = hip, C.c_void_p()
        a = np.ascontiguousarray(a)
        self.nbytes = a.nbytes
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0   # HostToDevice
        self.addr = self.p.value

    def __del__(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = None


def embed(img, pitch, offset):
    """the bytes of a buffer of 0xAA that holds `img` at `offset`, its rows `pitch` apart"""
    h, w = img.shape
    buf = np.full(offset + pitch * (h - 1) + w + 32, 0xAA, np.uint8)
    for v in range(h):
        buf[offset + v * pitch: offset + v * pitch + w] = img[v]
    return buf


def on_device(hip, img, pitch=None, offset=0):
    """(allocation, address of the frame) of `img` at a pitch and a byte offset into a larger buffer of 0xAA"""
    pitch = img.shape[1] if pitch is None else pitch
    d = Dev(hip, embed(np.ascontiguousarray(img), pitch, offset))
    return d, d.addr + offset


def frames_on_device(hip, imgs, pitch=None):
    """object i's frame at byte offset i mod 4 of an allocation of its own: (allocations to keep, addresses)"""
    held, addrs = [], []
    for i, img in enumerate(imgs):
        d, a = on_device(hip, img, pitch, i % 4)
        held.append(d)
        addrs.append(a)
    return held, addrs


def quad():
    return [H.read_pgm(os.path.join(H.GOLDEN, "viso_%s.pgm" % n)) for n in ("I1p", "I2p", "I1c", "I2c")]


def variant(im, k):
    """object k's images: shifted by 3k columns (stereo geometry kept), every other one mirrored top-down, so that the
    K objects differ in every table and a job that read another object's frame would show"""
    out = [np.roll(a, 3 * k, axis=1) for a in im]
    if k % 2:
        out = [a[::-1] for a in out]
    return [np.ascontiguousarray(a) for a in out]


def crop(im, w, h=230):
    return [np.ascontiguousarray(q[:h, :w]) for q in im]


def drive(q):
    """the 4-frame sequence of the pipeline tests: the reference's two consecutive quad pairs, twice"""
    return [(q[0], q[1]), (q[2], q[3]), (q[0], q[1]), (q[2], q[3])]


def plain_matcher(prm):
    m = H.ProductMatcher(prm)
    m.lib.svh_matcher_set_taps(C.c_void_p(m.h), 0)   # taps keep every stage and force the one-by-one path
    return m


def matcher_state(RS, m):
    """everything the parity tests compare of a Matcher: the eight feature tables, the four packed images as they lie
    on the device (None: a view without a frame), the matches"""
    return ([m.features(tb).copy() for tb in range(8)], [RS.t_matcher_image(m, v) for v in range(4)],
            m.matches().copy())


def assert_same_matcher_state(got, want, where):
    for tb, (x, y) in enumerate(zip(got[0], want[0])):
        assert x.shape == y.shape and np.array_equal(x, y), (where, "table", H.M_TABLES[tb])
    for v, (x, y) in enumerate(zip(got[1], want[1])):
        assert (x is None) == (y is None), (where, "view", v)
        assert x is None or np.array_equal(x, y), (where, "image", v)
    assert got[2].shape == want[2].shape and got[2].tobytes() == want[2].tobytes(), (where, "matches")


def vo_state(vo, ok):
    return int(ok), vo.motion().tobytes(), vo.inliers().copy(), vo.matches().copy()


def assert_same_vo_state(got, want, where):
    assert got[0] == want[0], (where, "ok", got[0], want[0])
    assert got[1] == want[1], (where, "motion")
    assert np.array_equal(got[2], want[2]), (where, "inliers")
    assert got[3].shape == want[3].shape and got[3].tobytes() == want[3].tobytes(), (where, "matches")


class Counts:
    """the lockstep counters since the object was made (or since mark()): flushed phases, one-by-one phases, batched
    launches"""

    def __init__(self, RS):
        self.RS = RS
        self.mark()

    def mark(self):
        self.at = self.RS.lockstep_counts()

    def delta(self):
        now = self.RS.lockstep_counts()
        d = tuple(int(b - a) for a, b in zip(self.at, now))
        self.at = now
        return d


def bits(x):
    return np.float32(x).tobytes()
