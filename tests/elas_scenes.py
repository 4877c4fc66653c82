"""Generated scenes for the ELAS edge tests (test_elas_edges.py on the reference and the oracle, test_elas_edges_gpu.py on
the device): seeded pairs whose ties, saturated Sobel bytes, starved support sets and empty triangulations reach the code
that helpers.synth_pair and the natural crops cannot.

A scene is one wide canvas and a piecewise-planar disparity map d (up to DMAX): left = the canvas cut to w columns,
right(x) = canvas(x + d(x)) at the nearest pixel, optionally with +-1 noise on the right image.  Images are cached and
read-only.
"""
import ctypes as C

import numpy as np

import helpers as H

DMAX = 40


# ----------------------------------------------------------------------------------------------- canvases
def _cells(rng, w, h, cell, draw):
    a = draw(rng, ((h + cell - 1) // cell, (w + cell - 1) // cell))
    return np.kron(a, np.ones((cell, cell), a.dtype))[:h, :w].astype(np.uint8)


def binary(w, h, seed, cell=3):
    """cells of 0 or 255: every Sobel byte at an edge clamps to 0 or 255, flat runs between"""
    return _cells(np.random.default_rng(seed), w, h, cell, lambda r, s: 255 * r.integers(0, 2, s))


def levels(w, h, seed, k=2, cell=4):
    """cells of k grey levels from 0 to 255"""
    step = 255 // (k - 1)
    return _cells(np.random.default_rng(seed), w, h, cell, lambda r, s: step * r.integers(0, k, s))


def lowc(w, h, seed, amp=3):
    """128 +- amp noise: descriptors of a few values around 128, just above the texture thresholds"""
    return (128 + np.random.default_rng(seed).integers(-amp, amp + 1, (h, w))).astype(np.uint8)


def vstripes(w, h, seed):
    """one random row repeated: no vertical gradient at all"""
    return np.tile(np.random.default_rng(seed).integers(0, 256, w).astype(np.uint8), (h, 1))


def _patches(I, rng, n, size):
    h, w = I.shape
    for _ in range(n):
        x, y = int(rng.integers(8, w - size - 8)), int(rng.integers(8, h - size - 8))
        I[y:y + size, x:x + size] = rng.integers(0, 256, (size, size))
    return I


def hstripes(w, h, seed, n=6, size=30):
    """one random column repeated -- every disparity of a support search costs the same -- plus n noise patches"""
    rng = np.random.default_rng(seed)
    I = np.tile(rng.integers(0, 256, h).astype(np.uint8)[:, None], (1, w))
    return _patches(I, rng, n, size)


def periodic(w, h, seed, p=16, n=8, size=24):
    """one random p x p tile repeated (the support search's best and second best tie) plus n noise patches"""
    t = np.random.default_rng(seed).integers(0, 256, (p, p))
    I = np.tile(t, ((h + p - 1) // p, (w + p - 1) // p))[:h, :w].astype(np.uint8)
    return _patches(I, np.random.default_rng(seed + 3), n, size)


def flat(w, h, seed, value=128, n=5, size=20):
    """a constant image with n noise patches: a few support points, very large triangles, almost no valid pixel"""
    return _patches(np.full((h, w), value, np.uint8), np.random.default_rng(seed + 3), n, size)


def thin_row(w, h, seed, y0=40):
    """one noise row on a constant image, on a row of the support lattice: all support points share their v"""
    I = np.full((h, w), 128, np.uint8)
    I[y0] = np.random.default_rng(seed).integers(0, 256, w)
    return I


def _planes(w, h, seed, dmax, planes, slant):
    rng = np.random.default_rng(seed + 1000)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    b = np.concatenate([[0], np.sort(rng.integers(0, w, planes - 1)), [w]])
    d = np.zeros((h, w), np.float32)
    for i in range(planes):
        sl = slice(b[i], b[i + 1])
        d[:, sl] = np.clip(rng.uniform(4, dmax - 4) + rng.uniform(-slant, slant) * (xx[:, sl] - b[i])
                           + rng.uniform(-slant, slant) * (yy[:, sl] - h / 2), 1, dmax)
    return d


def make_pair(gen, w, h, seed, dmax=DMAX, planes=4, slant=0.02, noise_r=0, **kw):
    big = gen(w + dmax + 8, h, seed=seed, **kw)
    d = _planes(w, h, seed, dmax, planes, slant)
    xr = np.clip(np.rint(np.arange(w)[None, :] + d).astype(np.int64), 0, big.shape[1] - 1)
    left = np.ascontiguousarray(big[:, :w])
    right = np.take_along_axis(big, xr, axis=1)
    if noise_r:
        rng = np.random.default_rng(seed + 7)
        right = np.clip(right.astype(int) + rng.integers(-noise_r, noise_r + 1, right.shape), 0, 255)
    return left, np.ascontiguousarray(right.astype(np.uint8))


# ----------------------------------------------------------------------------------------------- scenes
# name: (canvas, seed, make_pair keywords).  Seeds are chosen so that the counts test_elas_edges.py claims hold.
SCENES = {
    # ties of the dense arg-min (two evaluated candidates with the same cost)
    "levels2c4": (levels, 2, dict(k=2, cell=4)),
    "binary3": (binary, 3, dict(cell=3)),
    "binary8": (binary, 21, dict(cell=8)),          # also: most support searches end with e1 == e2
    "vstripes": (vstripes, 8, {}),
    "lowc3": (lowc, 16, dict(amp=3)),
    # ties of the support search (best and second-best energy equal)
    "hstripes": (hstripes, 9, {}),
    "per16": (periodic, 6, dict(p=16)),
    # starved frames
    "flat128_5": (flat, 10, {}),
    "flat0_5": (flat, 11, dict(value=0)),
    "flat255_5": (flat, 12, dict(value=255)),
    "flat128_2": (flat, 13, dict(n=2, size=12)),
    "tiny": (flat, 14, dict(n=1, size=10)),         # 4 support points, 2 + 2 triangles
    # 11 support points on one lattice row: Triangle returns no triangle, status 0, all-invalid maps
    "collinear": (thin_row, 18, dict(planes=1, slant=0)),
    # fewer than 3 support points: status 1
    "constant": (flat, 1, dict(n=0)),
    "periodic_pure": (periodic, 6, dict(p=16, n=0)),
}
TIE, SUPPORT_TIE = ("levels2c4", "binary3", "binary8", "vstripes", "lowc3"), ("hstripes", "per16")
STARVED = ("flat128_5", "flat0_5", "flat255_5", "flat128_2", "tiny")

_pairs = {}


def pair(scene, w=320, h=200):
    key = (scene, w, h)
    if key not in _pairs:
        gen, seed, kw = SCENES[scene]
        _pairs[key] = make_pair(gen, w, h, seed, **kw)
        for a in _pairs[key]:
            a.setflags(write=False)
    return _pairs[key]


# ----------------------------------------------------------------------------------------------- kernel forms
def forms(prm, w, h):
    """(support kernel, dense matcher) that launch_support / launch_match of csrc/elas_kernels.hip pick for these
    parameters and this size -- a restatement of support_strip, match_list_usable and match_keyed_usable for the default
    environment, so that every form set below can say which kernel it is there for"""
    stride = lambda x: ((x + 2) & ~3) + 1                                   # support_stride
    step = prm.candidate_stepsize + (prm.candidate_stepsize % 2 if prm.subsampling else 0)

    def strip(sb):
        span = (sb - 1) * step
        wl, wr = min(w, span + 2 * prm.disp_max + 5), min(w, span + prm.disp_max + 5)
        return 2 * (stride(wl) + stride(wr)) * 16, wr
    sb = 32 if strip(64)[0] + 2 * w + 16 + 512 > 65536 else 64
    lds, wr = strip(sb)
    support = "k_support_lds" if lds + 2 * wr + 16 + 512 <= 65536 else "k_support"
    dw = w // 2 if prm.subsampling else w
    radius = int(max(np.ceil(np.float32(prm.sigma) * np.float32(prm.sradius)), 2.0))
    keyed_ok = prm.disp_max < 512 and radius <= 15 and prm.grid_size > 1      # (prior_absmax: 14 .. 50 here)
    gwords = (prm.disp_max + 1 + 31) // 32
    if keyed_ok and gwords <= 8 and dw <= 8 * 256:
        match = "k_match_list"
    elif keyed_ok and 2 * w * 16 + 2 * dw * 4 + 256 <= 96 * 1024:
        match = "k_match_keyed"
    elif w * 16 + 256 <= 65536:
        match = "k_match<true>"
    else:
        match = "k_match<false>"
    return support, match


# form sets: parameter overrides, the size they run at, and the kernels they are there for
FORMS = {
    #  name         overrides                                              (w, h)       support kernel,  dense matcher
    "default":     ({},                                                    (320, 200), ("k_support_lds", "k_match_list")),
    # disp_max + 1 = 301 bits = 10 grid words > 8: no candidate lists
    "d300":        ({"disp_max": 300},                                     (320, 200), ("k_support_lds", "k_match_keyed")),
    # disp_max >= 512: the packed (cost, rank) key has no room, ordered scan over an LDS row
    "d600":        ({"disp_max": 600},                                     (320, 200), ("k_support_lds", "k_match<true>")),
    # plane radius ceil(3 * 6) = 18 > 15: ordered scan, and the widest band (37 disparities)
    "wide_band":   ({"sradius": 6.0, "sigma": 3.0},                        (320, 200), ("k_support_lds", "k_match<true>")),
    # a row of 4100 descriptors (65 600 B) exceeds 64 KB of LDS, DW > 2048: ordered scan from global memory
    "w4100":       ({},                                                    (4100, 60), ("k_support_lds", "k_match<false>")),
    # two rows of both strips exceed 64 KB at disp_max 800 once the row is 1 010 px wide: global-memory support search
    "d800":        ({"disp_max": 800},                                     (1100, 64), ("k_support", "k_match<true>")),
    "sub_both":    ({"subsampling": 1, "postprocess_only_left": 0},        (322, 201), ("k_support_lds", "k_match_list")),
    "median":      ({"filter_median": 1, "filter_adaptive_mean": 0},       (320, 200), ("k_support_lds", "k_match_list")),
    "gap_corners": ({"ipol_gap_width": 5000, "add_corners": 1},            (320, 200), ("k_support_lds", "k_match_list")),
    "ragged":      ({"postprocess_only_left": 0},                          (333, 117), ("k_support_lds", "k_match_list")),
    "corners":     ({"add_corners": 1},                                    (320, 200), ("k_support_lds", "k_match_list")),
    "middlebury":  ("middlebury",                                          (320, 200), ("k_support_lds", "k_match_list")),
}


class Case:
    def __init__(self, scene, form, status=0):
        self.scene, self.form, self.status = scene, form, status
        self.name = scene if form == "default" else scene + "-" + form
        self.over, (self.w, self.h), self.kernels = FORMS[form]

    def pair(self):
        return pair(self.scene, self.w, self.h)

    def params(self):
        return H.middlebury() if self.over == "middlebury" else H.robotics(**self.over)

    def __repr__(self):
        return self.name


def _cases():
    out = []
    for s in TIE:
        out += [Case(s, f) for f in ("default", "d300", "d600", "wide_band", "sub_both", "median", "gap_corners")]
    out += [Case(s, "w4100") for s in ("binary3", "levels2c4")]
    out += [Case(s, "d800") for s in ("binary8", "hstripes", "per16")]
    out += [Case(s, "ragged") for s in ("binary3", "hstripes")]
    for s in SUPPORT_TIE:
        out += [Case(s, f) for f in ("default", "d300", "d600")]
    out += [Case(s, "default") for s in STARVED]
    out += [Case("flat128_5", "middlebury"), Case("flat255_5", "sub_both"), Case("tiny", "gap_corners")]
    out += [Case("collinear", "default"), Case("collinear", "corners"), Case("collinear", "sub_both")]
    out += [Case("constant", "default", status=1), Case("periodic_pure", "default", status=1)]
    return out


CASES = {c.name: c for c in _cases()}


# ----------------------------------------------------------------------------------------------- runs
def triangulator():
    """the oracle's triangulator: the real Triangle of oracle/_ref where it is built (None = helpers' default), else the
    library's host triangulation svh_delaunay, which test_oracle_elas.py and test_dt_core.py pin to Triangle's output
    order"""
    if H.have_ref_elas():
        return None
    import svhip
    return C.cast(svhip.lib().svh_delaunay, C.c_void_p)


class Counts:
    """what one oracle run reached: support points, triangles of both images, valid share of D1, tie counters"""

    def __init__(self, run, ties):
        n3 = lambda s: len(run[s]) // 3 if s in run else 0
        self.status = run.status
        self.support, self.tri = n3(H.SUPPORT), (n3(H.TRI1), n3(H.TRI2))
        self.valid = float((run[H.D1_FINAL] >= 0).mean()) if H.D1_FINAL in run else 0.0
        self.__dict__.update(ties)

    def row(self):
        return (self.support, self.tri[0], self.tri[1], round(self.valid, 3), self.support_searches, self.support_ties,
                self.dense_matched, self.dense_ties, self.dense_not_lowest, self.dense_unevaluated)


_runs = {}


def oracle_run(case):
    """(StageRun, Counts) of the oracle on a case, computed once"""
    if case.name not in _runs:
        l, r = case.pair()
        run = H.oracle_elas_run(case.params(), l, r, triangulator())
        for a in run.stages.values():
            a.setflags(write=False)
        _runs[case.name] = (run, Counts(run, H.oracle_tie_stats()))
    return _runs[case.name]


# What every case reaches on the reference side (oracle == live reference on all of them), measured once and asserted as
# floors by test_elas_edges.py::test_recorded_counts:
#   support points, triangles left, triangles right, valid share of D1,
#   support searches, of those with e1 == e2,
#   find_match calls with a match, of those with the minimum attained twice, of those won by a d that is not the lowest,
#   find_match calls where no candidate was evaluated
# (left and right pass summed; a pixel two triangles cover counts twice).  Subsampling reaches about a quarter of the
# ties; under the wide band most ties fall inside it, where the scan is ascending, so a higher d wins between 0
# (levels2c4) and 602 times (binary3); the 1100 x 64 and 4100 x 60 images have few dense ties: those sets are there for
# the support search and the kernel form.
REACHED = {
    "levels2c4": (209, 379, 385, 0.745, 4011, 148, 97114, 3242, 331, 0),
    "levels2c4-d300": (209, 379, 385, 0.745, 4011, 149, 97114, 3242, 331, 0),
    "levels2c4-d600": (209, 379, 385, 0.745, 4011, 149, 97114, 3242, 331, 0),
    "levels2c4-wide_band": (209, 379, 385, 0.742, 4011, 148, 97114, 4352, 0, 0),
    "levels2c4-sub_both": (124, 218, 220, 0.759, 2875, 95, 24966, 821, 94, 0),
    "levels2c4-median": (209, 379, 385, 0.744, 4011, 148, 97114, 3242, 331, 0),
    "levels2c4-gap_corners": (215, 422, 422, 1.0, 4011, 148, 111064, 3412, 316, 6400),
    "binary3": (184, 328, 332, 0.778, 4202, 113, 105801, 3108, 267, 0),
    "binary3-d300": (184, 328, 332, 0.778, 4203, 113, 105801, 3108, 267, 0),
    "binary3-d600": (184, 328, 332, 0.778, 4203, 113, 105801, 3108, 267, 0),
    "binary3-wide_band": (184, 328, 332, 0.766, 4202, 113, 105801, 4150, 602, 0),
    "binary3-sub_both": (137, 238, 241, 0.766, 2993, 80, 26764, 903, 59, 0),
    "binary3-median": (184, 328, 332, 0.775, 4202, 113, 105801, 3108, 267, 0),
    "binary3-gap_corners": (190, 372, 372, 1.0, 4202, 113, 120534, 3340, 267, 3493),
    "binary8": (127, 238, 240, 0.414, 1897, 1093, 56762, 3138, 530, 0),
    "binary8-d300": (113, 215, 215, 0.395, 1888, 1117, 53856, 3172, 530, 0),
    "binary8-d600": (113, 215, 215, 0.395, 1888, 1117, 53856, 3172, 530, 0),
    "binary8-wide_band": (127, 238, 240, 0.4, 1897, 1093, 56762, 3610, 69, 0),
    "binary8-sub_both": (98, 179, 179, 0.462, 1314, 746, 13219, 652, 61, 0),
    "binary8-median": (127, 238, 240, 0.391, 1897, 1093, 56762, 3138, 530, 0),
    "binary8-gap_corners": (133, 258, 258, 1.0, 1897, 1093, 73859, 3784, 530, 3210),
    "vstripes": (178, 317, 321, 0.771, 4369, 34, 108710, 1401, 169, 0),
    "vstripes-d300": (178, 317, 321, 0.771, 4369, 34, 108710, 1401, 169, 0),
    "vstripes-d600": (178, 317, 321, 0.771, 4369, 34, 108710, 1401, 169, 0),
    "vstripes-wide_band": (178, 317, 321, 0.78, 4369, 34, 108710, 1429, 18, 0),
    "vstripes-sub_both": (113, 191, 197, 0.779, 3025, 35, 27410, 334, 51, 0),
    "vstripes-median": (178, 317, 321, 0.769, 4369, 34, 108710, 1401, 169, 0),
    "vstripes-gap_corners": (184, 360, 360, 1.0, 4369, 34, 122559, 1468, 169, 3217),
    "lowc3": (165, 289, 289, 0.818, 4372, 56, 108597, 1849, 173, 0),
    "lowc3-d300": (165, 289, 289, 0.818, 4372, 56, 108597, 1849, 173, 0),
    "lowc3-d600": (165, 289, 289, 0.818, 4372, 56, 108597, 1849, 173, 0),
    "lowc3-wide_band": (165, 289, 289, 0.815, 4372, 56, 108597, 2023, 224, 0),
    "lowc3-sub_both": (109, 180, 184, 0.815, 3043, 60, 27171, 466, 57, 0),
    "lowc3-median": (165, 289, 289, 0.817, 4372, 56, 108597, 1849, 173, 0),
    "lowc3-gap_corners": (171, 334, 334, 1.0, 4372, 56, 124056, 2272, 179, 1714),
    "binary3-w4100": (561, 842, 842, 0.74, 15875, 72, 360850, 541, 15, 0),
    "levels2c4-w4100": (755, 1240, 1240, 0.722, 14865, 794, 342847, 743, 47, 0),
    "binary8-d800": (3, 1, 1, 0.003, 1533, 1307, 999, 0, 0, 0),
    "hstripes-d800": (47, 79, 79, 0.465, 2667, 2074, 67502, 131, 1, 439),
    "per16-d800": (38, 63, 63, 0.412, 2734, 2053, 62872, 35, 1, 28),
    "binary3-ragged": (126, 216, 218, 0.772, 2580, 63, 63125, 1532, 166, 0),
    "hstripes-ragged": (42, 68, 68, 0.409, 1625, 1114, 32845, 1370, 377, 0),
    "hstripes": (49, 85, 85, 0.323, 2559, 1972, 45057, 2065, 977, 7),
    "hstripes-d300": (49, 85, 85, 0.323, 2559, 1972, 45057, 2065, 977, 7),
    "hstripes-d600": (49, 85, 85, 0.323, 2559, 1972, 45057, 2065, 977, 7),
    "per16": (36, 61, 61, 0.33, 2719, 1965, 47391, 35, 6, 0),
    "per16-d300": (36, 61, 61, 0.33, 2719, 1965, 47391, 35, 6, 0),
    "per16-d600": (36, 61, 61, 0.33, 2719, 1965, 47391, 35, 6, 0),
    "flat128_5": (18, 26, 26, 0.028, 165, 6, 3527, 0, 0, 0),
    "flat0_5": (20, 29, 29, 0.037, 200, 0, 4844, 1, 0, 0),
    "flat255_5": (16, 22, 22, 0.036, 200, 0, 4907, 163, 29, 0),
    "flat128_2": (8, 8, 8, 0.004, 42, 0, 841, 0, 0, 0),
    "tiny": (4, 2, 2, 0.0, 18, 0, 200, 0, 0, 0),
    "flat128_5-middlebury": (24, 40, 40, 1.0, 167, 6, 114657, 3, 0, 11111),
    "flat255_5-sub_both": (21, 30, 31, 0.035, 156, 2, 1255, 54, 11, 0),
    "tiny-gap_corners": (10, 12, 12, 1.0, 18, 0, 3874, 0, 0, 558),
    "collinear": (11, 0, 0, 0.0, 119, 0, 0, 0, 0, 0),
    "collinear-corners": (17, 26, 26, 0.061, 119, 0, 7424, 0, 0, 878),
    "collinear-sub_both": (9, 0, 0, 0.0, 99, 0, 0, 0, 0, 0),
    "constant": (0, 0, 0, 0.0, 0, 0, 0, 0, 0, 0),
    "periodic_pure": (0, 0, 0, 0.0, 2454, 2242, 0, 0, 0, 0),
}
