"""Generated scenes for the Matcher's edge tests (test_matcher_edges.py on the oracle alone,
test_matcher_edges_gpu.py on the device): seeded images whose feature tables, match counts, ties and
saturation reach the code the KITTI quad cannot.  A quad is one image I seen four times:

    previous left = I, previous right = I moved left by a disparity, current pair = both moved by a small flow,

cut from one wider canvas, so the four frames share their content and differ at the borders only.
"""
import os

import numpy as np

import helpers as H

MARGIN = 9          # matcher.cpp:56  margin = 8 + 1
DISP, FLOW = 6, (2, 1)


# ----------------------------------------------------------------------------------------------- images
def _cells(rng, w, h, cell, draw):
    a = draw(rng, ((h + cell - 1) // cell, (w + cell - 1) // cell))
    return np.ascontiguousarray(np.kron(a, np.ones((cell, cell), a.dtype))[:h, :w].astype(np.uint8))


def noise(w, h, cell=1, seed=0):
    """uniform random bytes, each repeated cell x cell"""
    return _cells(np.random.default_rng(seed), w, h, cell, lambda r, s: r.integers(0, 256, s))


def binary(w, h, cell=3, seed=0):
    """cells of 0 or 255: the blob filter's extremes (+-4080) and long flat runs"""
    return _cells(np.random.default_rng(seed), w, h, cell, lambda r, s: 255 * r.integers(0, 2, s))


def levels(w, h, k=3, cell=1, seed=0):
    """noise quantised to k grey levels: equal f1 / f2 values inside one NMS block"""
    step = 255 // (k - 1)
    return _cells(np.random.default_rng(seed), w, h, cell, lambda r, s: step * r.integers(0, k, s))


def periodic(w, h, p=24, seed=0):
    """one random p x p tile repeated: many features share their 32-byte descriptor"""
    t = np.random.default_rng(seed).integers(0, 256, (p, p))
    return np.ascontiguousarray(np.tile(t, ((h + p - 1) // p, (w + p - 1) // p))[:h, :w].astype(np.uint8))


def constant(w, h, value=128):
    return np.full((h, w), value, np.uint8)


def quad_of(gen, w, h, disp=DISP, flow=FLOW, **kw):
    """the four frames (I1p, I2p, I1c, I2c), w x h each, cut out of one (w + disp + fu) x (h + fv) canvas of `gen`:
    what np.roll by (disp, flow) followed by cropping the wrapped border gives"""
    fu, fv = flow
    big = gen(w + disp + fu, h + fv, **kw)
    cut = lambda x, y: np.ascontiguousarray(big[y:y + h, x:x + w])
    return cut(0, 0), cut(disp, 0), cut(fu, fv), cut(disp + fu, fv)


def patch(w, h, box=(40, 40, 200, 100), seed=0):
    """a noise rectangle (x, y, w, h) on a constant image: few features in all, many in a few bins"""
    I = constant(w, h)
    x, y, bw, bh = box
    I[y:y + bh, x:x + bw] = noise(bw, bh, 1, seed)
    return I


def natural_quad(w, h, x0=100):
    """the KITTI quad of tests/golden cut to w columns from x0 and extended to h rows by its own first rows: a natural
    image of a given size, whose features come in clumps"""
    out = []
    for k in ("I1p", "I2p", "I1c", "I2c"):
        a = H.read_pgm(os.path.join(H.GOLDEN, "viso_%s.pgm" % k))[:, x0:x0 + w]
        out.append(np.ascontiguousarray(np.vstack([a, a[:h - a.shape[0]]])))
    return tuple(out)


def bar_quad(w, h, vertical, at, width=16):
    """a 0 | 255 | 0 bar (vertical: along a column) -- both extremes of the Sobel responses"""
    I = np.zeros((h, w), np.uint8)
    if vertical:
        I[:, at:at + width] = 255
    else:
        I[at:at + width, :] = 255
    return I, I.copy(), I.copy(), I.copy()


# ----------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, gen, w, h, kw=None, prm=None, disp=DISP, flow=FLOW):
        self.name, self.gen, self.w, self.h = name, gen, w, h
        self.kw, self.prm, self.disp, self.flow = kw or {}, prm or {}, disp, flow
        self._quad = None

    def quad(self):
        if self._quad is None:
            if self.gen is natural_quad:
                self._quad = natural_quad(self.w, self.h, **self.kw)
            else:
                self._quad = quad_of(self.gen, self.w, self.h, self.disp, self.flow, **self.kw)
            for a in self._quad:
                a.setflags(write=False)
        return self._quad

    def params(self, **more):
        d = dict(self.prm)
        d.update(more)
        return H.matcher_defaults(**d)

    def __repr__(self):
        return self.name


FULL = {"half_resolution": 0, "nms_n": 2}

CASES = {c.name: c for c in [
    # --- size-switched paths (thresholds: test_matcher_edges.py)
    Case("big", noise, 640, 480, {"cell": 1, "seed": 1}, FULL),
    Case("middle", noise, 480, 320, {"cell": 1, "seed": 2}, FULL),
    Case("natural", natural_quad, 640, 480, {}, FULL),
    Case("small", noise, 320, 200, {"cell": 1, "seed": 3}, FULL),
    Case("under", noise, 1024, 512, {"cell": 2, "seed": 4}),
    Case("ranked_off", patch, 1100, 340, {"seed": 5}, {"match_binsize": 25, "half_resolution": 0, "nms_n": 1}),
    Case("ranked_on", noise, 320, 240, {"cell": 1, "seed": 6}, {"half_resolution": 0}),
    # --- ties and saturation
    Case("periodic", periodic, 320, 240, {"p": 24, "seed": 7}, {"half_resolution": 0}, disp=5, flow=(1, 1)),
    Case("periodic16", periodic, 320, 240, {"p": 16, "seed": 8}, {"half_resolution": 0}, disp=5, flow=(1, 1)),
    Case("binary3", binary, 320, 240, {"cell": 3, "seed": 9}, {"half_resolution": 0}),
    Case("binary8", binary, 320, 240, {"cell": 8, "seed": 10}, {"half_resolution": 0}),
    Case("levels3", levels, 320, 240, {"k": 3, "seed": 11}, {"half_resolution": 0}),
    Case("levels4c2", levels, 320, 240, {"k": 4, "cell": 2, "seed": 12}, {"half_resolution": 0}),
    # --- starved frames
    Case("constant", lambda w, h: constant(w, h), 320, 240),
    Case("tiny16", noise, 16, 16, {"seed": 13}, {"half_resolution": 0}),
    Case("tiny16h", noise, 16, 16, {"seed": 13}),
    Case("tiny24", noise, 24, 20, {"seed": 14}, {"half_resolution": 0}),
    Case("tiny24h", noise, 24, 20, {"seed": 14}),
    Case("dense_only", noise, 33, 31, {"seed": 15}, {"half_resolution": 0}, disp=2, flow=(1, 0)),
    Case("half_of_33x31", noise, 33, 31, {"seed": 15}, {}, disp=2, flow=(1, 0)),
    Case("handful", noise, 64, 48, {"seed": 16}, {"half_resolution": 0}, disp=2, flow=(1, 0)),
]}


def blank_right(case):
    """the case's frames with a constant right camera"""
    a, b, c, d = case.quad()
    return a, constant(case.w, case.h), c, constant(case.w, case.h)


# filter-kernel geometry: a block is 256 columns x 32 rows, a thread owns 4 columns x 8 rows, bpl = w rounded up to 16.
# (w, h, half_resolution): w % 16 in {0, 1, 15}; 255 / 256 / 257 / 1025; h % 8 in {0, 1, 7}; 31 / 32 / 33; odd w and h
# at half resolution
FILTER_SIZES = [(255, 31, 0), (256, 32, 0), (257, 33, 0), (1025, 39, 0), (271, 40, 0), (255, 65, 1), (257, 63, 1),
                (513, 67, 1), (1025, 71, 1)]


def nms_blocks(extent, n, margin=MARGIN):
    """blocks of the non-maximum suppression along one axis (matcher.cpp:419-420)"""
    c, i = 0, n + margin
    while i < extent - n - margin:
        c += 1
        i += n + 1
    return c


def sparse_n(nms_n):
    """the sparse pass's radius (matcher.cpp:824-828)"""
    ns = 3 * nms_n
    return max(nms_n, 10) if ns > 10 else ns


def nslots(w, h, n):
    return 4 * nms_blocks(w, n) * nms_blocks(h, n)


# slot-compaction sizes at half_resolution = 0: (w, h, nms_n, name).  nslots = 4 ni nj of the table the name says:
# 1, 2, 3 blocks; 1 020 (under one slot per thread); 1 200 (two slots per thread rounded up to a chunk of four);
# 65 536 = 4 x 128 x 128 (the last masked size) and 66 048 = 4 x 129 x 128 (the first unmasked one that an image has)
SLOT_SIZES = [(25, 25, 3, "dense1"), (29, 25, 3, "dense2"), (33, 25, 3, "dense3"),
              (37, 37, 3, "sparse1"), (47, 37, 3, "sparse2"), (57, 37, 3, "sparse3"),
              (81, 89, 3, "under1024"), (101, 81, 3, "ragged_chunk"),
              (533, 533, 3, "masked_last"), (537, 533, 3, "unmasked_first")]


def slot_case(size):
    w, h, n, what = size
    return Case("slots_" + what, noise, w, h, {"seed": 100 + w + h}, {"half_resolution": 0, "nms_n": n},
                disp=2, flow=(1, 0))


def run(driver, quad, method=2, tr=None, intr=None):
    if intr:
        driver.set_intrinsics(*intr)
    driver.push_back(quad[0], quad[1])
    driver.push_back(quad[2], quad[3])
    rc = driver.match(method, tr)
    assert rc in (0, None), rc
    return driver
