"""numpy restatement of StereoImage::histogramNormalization (stereomapper/stereoimage.cpp:94-134), the cases of the
golden fixture tests/golden/histnorm.npz, and the build of the reference itself into a temporary directory (used by
tests/golden/make_goldens_histnorm.py and the live check in tests/test_histnorm.py; the GPU tests read only the
committed fixture).

The restatement performs the reference's float operations in its order: np.add.accumulate over float32 adds strictly
one after the other (test_histnorm.py checks it against a scalar loop), so the whole chain f(0..N) of one image size is
one call.  The map's byte wrap is restated as the x86-64 build performs it: truncation to int32, low byte.

The driver (tests/histnorm/ref_histnorm_harness.cpp) and the QObject stand-in (tests/histnorm/qt_stub/QObject) are this
project's text; the reference's stereoimage.cpp is compiled unchanged.  The fixture stores recorded results only: the
inputs are committed crops of tests/golden or closed integer formulas."""
import functools
import hashlib
import os
import struct
import subprocess

import numpy as np

import helpers as H

REF = os.environ.get("REF", "/root/reference")
HERE = os.path.join(H.ROOT, "tests", "histnorm")
REFFLAGS = ["-O3", "-DNDEBUG", "-msse3", "-fPIC", "-w", "-std=c++11"]   # oracle/Makefile
GOLDEN = os.path.join(H.GOLDEN, "histnorm.npz")


# ----------------------------------------------------------------------------------------------------- restatement
def fraction(w, h):
    return np.float32(1.0 / float(np.float32(w * h)))


@functools.lru_cache(maxsize=3)
def chain(w, h):
    """f(0..N): N float additions of the fraction, one after the other"""
    a = np.full(w * h + 1, fraction(w, h), np.float32)
    a[0] = 0
    f = np.add.accumulate(a, dtype=np.float32)
    f.setflags(write=False)
    return f


def table(counts, w, h):
    """(cdf float32 [256], map uint8 [256]) for these counts"""
    p = chain(w, h)[np.asarray(counts, np.int64)]
    cdf = np.add.accumulate(p, dtype=np.float32)
    m = ((cdf.astype(np.float64) * 255.0).astype(np.int32) & 255).astype(np.uint8)   # the wrap
    return cdf, m


def counts_of(img):
    return np.bincount(np.asarray(img, np.uint8).ravel(), minlength=256).astype(np.int32)


def normalize(img):
    """(image, counts, cdf, map)"""
    h, w = img.shape
    counts = counts_of(img)
    cdf, m = table(counts, w, h)
    return m[img], counts, cdf, m


def breakpoints(w, h):
    """every n >= 1 at which the chain's step changes: f(n+1) - f(n) != f(n) - f(n-1), from the chain itself"""
    f = chain(w, h).astype(np.float64)
    d = np.diff(f)
    return (np.flatnonzero(d[1:] != d[:-1]) + 1).astype(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ images
def pattern(w, h, mul=1):
    """a fixed pattern with an uneven histogram over 0..254: an integer hash of (u, v), squared"""
    v, u = np.mgrid[0:h, 0:w].astype(np.int64)
    k = (u * 7919 + v * 104729 + (u * v) % 8191 * 31 * mul) % 1000
    return ((k * k) // 3922).astype(np.uint8)


def ramp(w, h):
    """every grey level occurs"""
    v, u = np.mgrid[0:h, 0:w].astype(np.int64)
    return ((u * 7 + v * 13) % 256).astype(np.uint8)


def flat(w, h, value=100):
    return np.full((h, w), value, np.uint8)


def two_level(w, h):
    """the first third of the pixels 10, the rest 200"""
    a = np.full(w * h, 200, np.uint8)
    a[:w * h // 3] = 10
    return a.reshape(h, w)


def from_counts(counts, w, h):
    """the image whose pixels are the grey levels in ascending order, counts[g] of each"""
    counts = np.asarray(counts, np.int64)
    assert counts.sum() == w * h and (counts >= 0).all()
    return np.repeat(np.arange(256, dtype=np.uint8), counts).reshape(h, w)


def boundary_counts(w, h, first=0, every=1):
    """counts b-1, b, b+1 in consecutive bins for the chain's breakpoints b (from `first`, every `every`-th) while the
    pixels last; the rest goes to the last bin"""
    N, counts, g = w * h, np.zeros(256, np.int64), 0
    for b in breakpoints(w, h)[first::every]:
        want = [int(b) - 1, int(b), int(b) + 1]
        if g + 3 >= 255 or counts.sum() + sum(want) > N:
            break
        counts[g:g + 3] = want
        g += 3
    counts[255] = N - counts.sum()
    return counts


def split_counts(w, h, n, lo=3, hi=250):
    """two bins: n pixels of level lo, the others of level hi"""
    counts = np.zeros(256, np.int64)
    counts[lo], counts[hi] = n, w * h - n
    return counts


def crop(name):
    return H.read_pgm(os.path.join(H.GOLDEN, name + ".pgm"))


def cases():
    """[(name, image, step, keep)]: keep = the fixture stores the output image (small cases), else its SHA-256"""
    out = [("flat_1392x512", flat(1392, 512), 1392, False),
           ("flat_1242x375", flat(1242, 375), 1242, False),
           ("two_1392x512", two_level(1392, 512), 1392, False),
           ("urban1_left", crop("urban1_1242x375_left"), 1242, False),
           ("urban3_small_right", crop("urban3_640x240_right"), 640, False),
           ("boundary_1242x375", from_counts(boundary_counts(1242, 375), 1242, 375), 1242, False),
           ("pattern_4097x4096", pattern(4097, 4096), 4097, False),
           ("ramp_257x5", ramp(257, 5), 257, True),
           ("pattern_17x5", pattern(17, 5), 17, True),
           ("pattern_65x4_step68", pattern(65, 4, 3), 68, True),
           ("pattern_15x1", pattern(15, 1), 15, True),
           ("one_1x1", flat(1, 1, 7), 1, True)]
    return out


# ----------------------------------------------------------------------------------------------------------- harness
def have_ref():
    return os.path.isfile(os.path.join(REF, "stereomapper", "stereoimage.cpp"))


def build_harness(tmp):
    """compile the reference's stereoimage.cpp (unchanged) and the driver into tmp; returns the program's path"""
    sm = os.path.join(REF, "stereomapper")
    inc = ["-I" + os.path.join(HERE, "qt_stub"), "-I" + sm]
    obj = os.path.join(tmp, "stereoimage.o")
    subprocess.check_call(["g++"] + REFFLAGS + inc + ["-c", os.path.join(sm, "stereoimage.cpp"), "-o", obj])
    exe = os.path.join(tmp, "ref_histnorm_harness")
    subprocess.check_call(["g++"] + REFFLAGS + inc + [os.path.join(HERE, "ref_histnorm_harness.cpp"), obj, "-o", exe])
    return exe


def run_reference(exe, tmp, images):
    """images: [(image [h, w], step)]; returns the images after the reference's call.  Bytes between the rows are
    painted 0x5A and must come back untouched."""
    path = os.path.join(tmp, "job.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(images)))
        for img, step in images:
            h, w = img.shape
            buf = np.full((h, step), 0x5A, np.uint8)
            buf[:, :w] = img
            f.write(struct.pack("<iii", w, h, step))
            f.write(buf.tobytes())
    b = subprocess.run([exe, path], check=True, capture_output=True).stdout
    out, at = [], 0
    for img, step in images:
        h, w = img.shape
        buf = np.frombuffer(b, np.uint8, h * step, at).reshape(h, step)
        at += h * step
        assert (buf[:, w:] == 0x5A).all()
        out.append(buf[:, :w].copy())
    assert at == len(b)
    return out


def observed_map(before, after):
    """the reference's map as its output shows it: map[g] for every level that occurs, and for a level that does not
    the entry below it (p[g] = 0 leaves cdf[g] = cdf[g-1]; 0 below the first level that occurs)"""
    m = np.zeros(256, np.uint8)
    seen = np.zeros(256, bool)
    b, a = before.ravel(), after.ravel()
    first = np.unique(b, return_index=True)
    m[first[0]] = a[first[1]]
    seen[first[0]] = True
    assert np.array_equal(m[b], a), "the reference's output is not a map of its input"
    for g in range(256):
        if not seen[g]:
            m[g] = m[g - 1] if g else 0
    return m


# ----------------------------------------------------------------------------------------------------------- fixture
def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
