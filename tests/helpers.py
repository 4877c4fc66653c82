"""Shared test plumbing: ctypes bindings for the three libraries under test.

  * product   stereo-vision_amd/libsvhip.so      (HIP path, C-ABI include/svh.h)
  * oracle    oracle/liboracle.so                (scalar CPU restatement)
  * reference oracle/_ref/libref_{elas,viso}.so  (the real reference, compiled
              from /root/reference by oracle/Makefile; travels prebuilt)

Nothing here reads /root/reference at run time.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stereo-vision_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
GOLDEN = os.path.join(ROOT, "tests", "golden")


class ElasParams(C.Structure):
    """svh_elas_params (include/svh.h) == Elas::parameters (libelas/src/elas.h:59-148)."""
    _fields_ = [
        ("disp_min", C.c_int32), ("disp_max", C.c_int32),
        ("support_threshold", C.c_float), ("support_texture", C.c_int32),
        ("candidate_stepsize", C.c_int32), ("incon_window_size", C.c_int32),
        ("incon_threshold", C.c_int32), ("incon_min_support", C.c_int32),
        ("add_corners", C.c_int32), ("grid_size", C.c_int32),
        ("beta", C.c_float), ("gamma", C.c_float), ("sigma", C.c_float), ("sradius", C.c_float),
        ("match_texture", C.c_int32), ("lr_threshold", C.c_int32),
        ("speckle_sim_threshold", C.c_float), ("speckle_size", C.c_int32),
        ("ipol_gap_width", C.c_int32), ("filter_median", C.c_int32),
        ("filter_adaptive_mean", C.c_int32), ("postprocess_only_left", C.c_int32),
        ("subsampling", C.c_int32),
    ]

    def copy(self, **kw):
        q = ElasParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q


def robotics(**kw):
    """Elas::parameters(ROBOTICS) -- libelas/src/elas.h:91-116."""
    p = ElasParams(0, 255, 0.85, 10, 5, 5, 5, 5, 0, 20, 0.02, 3.0, 1.0, 2.0, 1, 2, 1.0, 200, 3,
                   0, 1, 1, 0)
    return p.copy(**kw)


def middlebury(**kw):
    """Elas::parameters(MIDDLEBURY) -- libelas/src/elas.h:119-145."""
    p = ElasParams(0, 255, 0.95, 10, 5, 5, 5, 5, 1, 20, 0.02, 5.0, 1.0, 3.0, 0, 2, 1.0, 200, 5000,
                   1, 0, 0, 0)
    return p.copy(**kw)


# stage ids: enum svh_elas_stage (include/svh.h)
(DESC1, DESC2, DCAN_RAW, SUPPORT, TRI1, TRI2, PLANES1, PLANES2, GRID1, GRID2, D1_RAW, D2_RAW,
 D1_LR, D2_LR, D1_SEG, D2_SEG, D1_GAP, D2_GAP, STAGE_COUNT) = range(19)
D1_FINAL, D2_FINAL = STAGE_COUNT, STAGE_COUNT + 1

STAGE_DTYPE = {
    DESC1: np.uint8, DESC2: np.uint8, DCAN_RAW: np.int16, SUPPORT: np.int32, TRI1: np.int32,
    TRI2: np.int32, PLANES1: np.float32, PLANES2: np.float32, GRID1: np.int32, GRID2: np.int32,
}


def stage_dtype(stage):
    return STAGE_DTYPE.get(stage, np.float32)


def _p(a, t=C.c_void_p):
    return a.ctypes.data_as(t)


def dims_of(img):
    h, w = img.shape
    return (C.c_int32 * 3)(w, h, img.strides[0])


# ----------------------------------------------------------------------------- reference
_ref_elas = None


def ref_elas_path():
    return os.path.join(ROOT, "oracle", "_ref", "libref_elas.so")


def have_ref_elas():
    return os.path.exists(ref_elas_path())


def ref_elas():
    global _ref_elas
    if _ref_elas is None:
        lib = C.CDLL(ref_elas_path())
        lib.ref_init(1)
        lib.ref_elas_run.restype = C.c_void_p
        lib.ref_elas_run.argtypes = [C.POINTER(ElasParams), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ref_elas_run_free.argtypes = [C.c_void_p]
        lib.ref_elas_run_status.argtypes = [C.c_void_p]
        lib.ref_elas_run_get.restype = C.c_int64
        lib.ref_elas_run_get.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        lib.ref_triangulate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        _ref_elas = lib
    return _ref_elas


class StageRun:
    """dict-like view of all intermediates of one staged run."""

    def __init__(self, status, stages):
        self.status = status
        self.stages = stages

    def __getitem__(self, k):
        return self.stages[k]

    def __contains__(self, k):
        return k in self.stages


def ref_elas_run(params, I1, I2):
    """All intermediates of the reference's Elas::process on one pair."""
    lib = ref_elas()
    I1 = np.ascontiguousarray(I1, np.uint8)
    I2 = np.ascontiguousarray(I2, np.uint8)
    h = lib.ref_elas_run(C.byref(params), _p(I1), _p(I2), dims_of(I1))
    try:
        st = {}
        for s in list(range(STAGE_COUNT)) + [D1_FINAL, D2_FINAL]:
            n = lib.ref_elas_run_get(h, s, None, 0)
            if n <= 0:
                continue
            buf = np.empty(n, np.uint8)
            lib.ref_elas_run_get(h, s, _p(buf), n)
            st[s] = buf.view(stage_dtype(s))
        return StageRun(lib.ref_elas_run_status(h), st)
    finally:
        lib.ref_elas_run_free(h)


def ref_elas_process(params, I1, I2):
    lib = ref_elas()
    I1 = np.ascontiguousarray(I1, np.uint8)
    I2 = np.ascontiguousarray(I2, np.uint8)
    h, w = I1.shape
    if params.subsampling:
        h, w = h // 2, w // 2
    D1 = np.full((h, w), -7.0, np.float32)
    D2 = np.full((h, w), -7.0, np.float32)
    lib.ref_elas_process(C.byref(params), _p(I1), _p(I2), _p(D1), _p(D2), dims_of(I1))
    return D1, D2


def ref_triangulate(pts):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    cap = 2 * len(pts) + 16
    tri = np.empty((cap, 3), np.int32)
    n = ref_elas().ref_triangulate(_p(pts), len(pts), _p(tri), cap)
    return tri[:n].copy()


# ----------------------------------------------------------------------------- images
def read_pgm(path):
    with open(path, "rb") as f:
        data = f.read()
    assert data[:2] == b"P5"
    toks, pos = [], 2
    while len(toks) < 3:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            while data[pos:pos + 1] != b"\n":
                pos += 1
            continue
        e = pos
        while not data[e:e + 1].isspace():
            e += 1
        toks.append(int(data[pos:e]))
        pos = e
    pos += 1
    w, h, mx = toks
    assert mx == 255
    return np.frombuffer(data, np.uint8, w * h, pos).reshape(h, w).copy()


def write_pgm(path, img):
    img = np.ascontiguousarray(img, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def synth_pair(w, h, seed, dmax=64, planes=6, noise=2):
    """Seeded synthetic rectified pair: smooth random
    texture, piecewise-planar disparity, right = left warped by -d + noise."""
    rng = np.random.default_rng(seed)

    def value_noise(step):
        gh, gw = h // step + 3, w // step + 3
        g = rng.random((gh, gw)).astype(np.float32)
        ys = np.arange(h, dtype=np.float32) / step
        xs = np.arange(w, dtype=np.float32) / step
        y0 = ys.astype(np.int32)
        x0 = xs.astype(np.int32)
        fy = (ys - y0)[:, None]
        fx = (xs - x0)[None, :]
        a = g[y0][:, x0]
        b = g[y0][:, x0 + 1]
        c = g[y0 + 1][:, x0]
        d = g[y0 + 1][:, x0 + 1]
        return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy

    tex = 0.5 * value_noise(16) + 0.3 * value_noise(5) + 0.2 * value_noise(2)
    tex = (tex - tex.mean()) / (tex.std() + 1e-6)
    wide = w + dmax + 8
    # texture for a wider canvas so that the right view has content everywhere
    texw = np.concatenate([tex, tex[:, ::-1][:, :wide - w]], axis=1) if wide > w else tex
    left_wide = np.clip(128 + 40 * texw, 0, 255)
    # disparity: random slanted planes over vertical stripes/blocks
    disp = np.zeros((h, w), np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    bounds = np.sort(rng.integers(0, w, planes - 1))
    bounds = np.concatenate([[0], bounds, [w]])
    for i in range(planes):
        d0 = rng.uniform(4, dmax - 4)
        ax = rng.uniform(-0.02, 0.02)
        ay = rng.uniform(-0.02, 0.02)
        sl = slice(bounds[i], bounds[i + 1])
        disp[:, sl] = np.clip(d0 + ax * (xx[:, sl] - bounds[i]) + ay * (yy[:, sl] - h / 2), 1, dmax)
    left = left_wide[:, :w]
    # right(x) = left(x + d): sample the left canvas at nearest pixel
    xr = np.clip(np.rint(xx + disp).astype(np.int32), 0, wide - 1)
    right = np.take_along_axis(left_wide, xr, axis=1)
    n1 = rng.integers(-noise, noise + 1, (h, w))
    n2 = rng.integers(-noise, noise + 1, (h, w))
    I1 = np.clip(np.rint(left) + n1, 0, 255).astype(np.uint8)
    I2 = np.clip(np.rint(right) + n2, 0, 255).astype(np.uint8)
    return I1, I2


def golden_pair(name):
    """Committed input pair under tests/golden (PGM crops of the reference's own images)."""
    l = read_pgm(os.path.join(GOLDEN, name + "_left.pgm"))
    r = read_pgm(os.path.join(GOLDEN, name + "_right.pgm"))
    return l, r


def disparity_agreement(D, Dref):
    """Fraction of reference-valid pixels whose value is within +-1 (and valid) in D."""
    valid = Dref >= 0
    ok = valid & (D >= 0) & (np.abs(D - Dref) <= 1.0)
    return ok.sum() / max(int(valid.sum()), 1)


# ----------------------------------------------------------------------------- oracle
_oracle = None
TRI_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32)


def oracle_path():
    return os.path.join(ROOT, "oracle", "liboracle.so")


def oracle():
    global _oracle
    if _oracle is None:
        lib = C.CDLL(oracle_path())
        lib.orc_elas_run.restype = C.c_void_p
        lib.orc_elas_run.argtypes = [C.POINTER(ElasParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
        lib.orc_elas_run_free.argtypes = [C.c_void_p]
        lib.orc_elas_run_status.argtypes = [C.c_void_p]
        lib.orc_elas_run_get.restype = C.c_int64
        lib.orc_elas_run_get.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        _oracle = lib
    return _oracle


def ref_triangulator():
    """address of the real Triangle (oracle/_ref) as an orc_triangulate_fn"""
    return C.cast(ref_elas().ref_triangulate, C.c_void_p)


def fixture_triangulator(tri_lists):
    """orc_triangulate_fn that replays golden triangle lists in call order."""
    it = iter(tri_lists)

    def fn(pts, n, tri, cap):
        t = np.ascontiguousarray(next(it), np.int32).reshape(-1, 3)
        C.memmove(tri, t.ctypes.data, t.nbytes)
        return len(t)

    cb = TRI_FN(fn)
    return cb


def oracle_elas_run(params, I1, I2, tri_fn=None):
    """All intermediates of the oracle restatement on one pair."""
    lib = oracle()
    I1 = np.ascontiguousarray(I1, np.uint8)
    I2 = np.ascontiguousarray(I2, np.uint8)
    if tri_fn is None:
        tri_fn = ref_triangulator()
    fn = tri_fn if isinstance(tri_fn, C.c_void_p) else C.cast(tri_fn, C.c_void_p)
    h = lib.orc_elas_run(C.byref(params), _p(I1), _p(I2), dims_of(I1), fn)
    try:
        st = {}
        for s in list(range(STAGE_COUNT)) + [D1_FINAL, D2_FINAL]:
            n = lib.orc_elas_run_get(h, s, None, 0)
            if n <= 0:
                continue
            buf = np.empty(n, np.uint8)
            lib.orc_elas_run_get(h, s, _p(buf), n)
            st[s] = buf.view(stage_dtype(s))
        return StageRun(lib.orc_elas_run_status(h), st)
    finally:
        lib.orc_elas_run_free(h)


TIE_FIELDS = ("support_searches", "support_ties", "dense_matched", "dense_ties", "dense_not_lowest", "dense_unevaluated")


def oracle_tie_stats():
    """orc_elas_tie_stats: the tie counters of the last oracle_elas_run (oracle/oracle.h), as a dict"""
    out = (C.c_int64 * 6)()
    oracle().orc_elas_tie_stats(out)
    return dict(zip(TIE_FIELDS, [int(x) for x in out]))


STAGE_NAMES = {
    DESC1: "desc1", DESC2: "desc2", DCAN_RAW: "dcan_raw", SUPPORT: "support", TRI1: "tri1",
    TRI2: "tri2", PLANES1: "planes1", PLANES2: "planes2", GRID1: "grid1", GRID2: "grid2",
    D1_RAW: "d1_raw", D2_RAW: "d2_raw", D1_LR: "d1_lr", D2_LR: "d2_lr", D1_SEG: "d1_seg",
    D2_SEG: "d2_seg", D1_GAP: "d1_gap", D2_GAP: "d2_gap", D1_FINAL: "d1", D2_FINAL: "d2",
}


def compare_runs(a, b, stages=None, skip=()):
    """list of (stage name, n_mismatch) for stages present in both runs"""
    out = []
    for s in (stages or sorted(STAGE_NAMES)):
        if s in skip or s not in a or s not in b:
            continue
        x, y = a[s], b[s]
        if x.shape != y.shape:
            out.append((STAGE_NAMES[s], -1))
        else:
            out.append((STAGE_NAMES[s], int((x.view(np.uint8) != y.view(np.uint8)).sum())
                        if x.dtype != np.float32 else int((x != y).sum())))
    return out


# ----------------------------------------------------------------------------- libviso2 Matcher
class MatcherParams(C.Structure):
    """svh_matcher_params (include/svh.h) == Matcher::parameters (libviso2/src/matcher.h:41-69)."""
    _fields_ = [
        ("nms_n", C.c_int32), ("nms_tau", C.c_int32), ("match_binsize", C.c_int32),
        ("match_radius", C.c_int32), ("match_disp_tolerance", C.c_int32),
        ("outlier_disp_tolerance", C.c_int32), ("outlier_flow_tolerance", C.c_int32),
        ("multi_stage", C.c_int32), ("half_resolution", C.c_int32), ("refinement", C.c_int32),
        ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double), ("base", C.c_double),
    ]

    def copy(self, **kw):
        q = MatcherParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q


def matcher_defaults(**kw):
    """Matcher::parameters() -- libviso2/src/matcher.h:56-68"""
    return MatcherParams(3, 50, 50, 200, 2, 5, 5, 1, 1, 1, 0.0, 0.0, 0.0, 0.0).copy(**kw)


P_MATCH = np.dtype([("u1p", "f4"), ("v1p", "f4"), ("i1p", "i4"), ("u2p", "f4"), ("v2p", "f4"),
                    ("i2p", "i4"), ("u1c", "f4"), ("v1c", "f4"), ("i1c", "i4"), ("u2c", "f4"),
                    ("v2c", "f4"), ("i2c", "i4")])
(M_SPARSE_RAW, M_SPARSE, M_RANGES, M_DENSE_RAW, M_DENSE_REFINED, M_DENSE, M_STAGE_COUNT) = range(7)
M_STAGE_NAMES = ["sparse_raw", "sparse", "ranges", "dense_raw", "dense_refined", "dense"]
M_TABLES = ["1p1", "1p2", "2p1", "2p2", "1c1", "1c2", "2c1", "2c2"]

_ref_viso = None


def ref_viso_path():
    return os.path.join(ROOT, "oracle", "_ref", "libref_viso.so")


def have_ref_viso():
    return os.path.exists(ref_viso_path())


def ref_viso():
    global _ref_viso
    if _ref_viso is None:
        lib = C.CDLL(ref_viso_path())
        lib.ref_init(1)
        lib.ref_matcher_create.restype = C.c_void_p
        lib.ref_matcher_create.argtypes = [C.POINTER(MatcherParams)]
        for f in ("ref_matcher_destroy", "ref_matcher_push_back", "ref_matcher_match",
                  "ref_matcher_match_staged", "ref_matcher_get_stage", "ref_matcher_get_features",
                  "ref_matcher_get_filter", "ref_matcher_set_intrinsics", "ref_matcher_get_matches",
                  "ref_matcher_bucket", "ref_matcher_gain"):
            getattr(lib, f)
        lib.ref_matcher_destroy.argtypes = [C.c_void_p]
        lib.ref_matcher_push_back.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        lib.ref_matcher_match.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.ref_matcher_match_staged.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.ref_matcher_get_stage.restype = C.c_int64
        lib.ref_matcher_get_stage.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        lib.ref_matcher_get_features.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        lib.ref_matcher_get_filter.restype = C.c_int64
        lib.ref_matcher_get_filter.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        lib.ref_matcher_set_intrinsics.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
        lib.ref_matcher_get_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.ref_matcher_bucket.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float]
        lib.ref_matcher_gain.restype = C.c_float
        lib.ref_matcher_gain.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.ref_viso_triangulate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        _ref_viso = lib
    return _ref_viso


class MatcherBase:
    """shared driver over the three Matcher implementations (prefix = ref_/orc_/svh_)"""

    def __init__(self, lib, prefix, params):
        self.lib, self.px = lib, prefix
        self.params = params
        self.h = getattr(lib, prefix + "matcher_create")(C.byref(params))

    def __del__(self):
        if getattr(self, "h", None):
            getattr(self.lib, self.px + "matcher_destroy")(self.h)
            self.h = None

    def _f(self, name):
        return getattr(self.lib, self.px + "matcher_" + name)

    def set_intrinsics(self, f, cu, cv, base):
        self._f("set_intrinsics")(self.h, f, cu, cv, base)

    def push_back(self, I1, I2=None, replace=False):
        I1 = np.ascontiguousarray(I1, np.uint8)
        p2 = None
        if I2 is not None:
            I2 = np.ascontiguousarray(I2, np.uint8)
            p2 = _p(I2)
        return self._f("push_back")(self.h, _p(I1), p2, dims_of(I1), 1 if replace else 0)

    def features(self, table):
        n = self._f("get_features")(self.h, table, None, 0)
        out = np.zeros((max(n, 0), 12), np.int32)
        if n > 0:
            self._f("get_features")(self.h, table, _p(out), n)
        return out

    def filter_image(self, which):
        dims = (C.c_int32 * 3)()
        if self.px == "svh_":
            sz = C.c_size_t(0)
            self._f("get_filter")(self.h, which, None, 0, C.byref(sz), dims)
            buf = np.zeros(sz.value, np.uint8)
            self._f("get_filter")(self.h, which, _p(buf), sz.value, C.byref(sz), dims)
        else:
            n = self._f("get_filter")(self.h, which, None, 0, dims)
            buf = np.zeros(max(n, 0), np.uint8)
            self._f("get_filter")(self.h, which, _p(buf), n, dims)
        a = buf.view(np.int16 if which >= 4 else np.uint8)
        return a.reshape(dims[1], dims[2])[:, :dims[0]], tuple(dims)

    def stage(self, stage):
        if self.px == "svh_":
            sz = C.c_size_t(0)
            self._f("get_stage")(self.h, stage, None, 0, C.byref(sz))
            buf = np.zeros(sz.value, np.uint8)
            if sz.value:
                self._f("get_stage")(self.h, stage, _p(buf), sz.value, C.byref(sz))
        else:
            n = self._f("get_stage")(self.h, stage, None, 0)
            buf = np.zeros(max(n, 0), np.uint8)
            if n > 0:
                self._f("get_stage")(self.h, stage, _p(buf), n)
        return buf.view(np.float32) if stage == M_RANGES else buf.view(P_MATCH)

    def matches(self):
        n = self._f("get_matches")(self.h, None, 0)
        out = np.zeros(max(n, 0), P_MATCH)
        if n > 0:
            self._f("get_matches")(self.h, _p(out), n)
        return out


class RefMatcher(MatcherBase):
    def __init__(self, params):
        super().__init__(ref_viso(), "ref_", params)

    def match(self, method, Tr=None, staged=True):
        t = None if Tr is None else _p(np.ascontiguousarray(Tr, np.float64))
        (self.lib.ref_matcher_match_staged if staged else self.lib.ref_matcher_match)(self.h, method, t)

    def bucket(self, max_features, bw, bh):
        return self.lib.ref_matcher_bucket(self.h, max_features, bw, bh)

    def gain(self, inliers):
        a = np.ascontiguousarray(inliers, np.int32)
        return self.lib.ref_matcher_gain(self.h, _p(a), len(a))


class OracleMatcher(MatcherBase):
    def __init__(self, params, tri_fn=None):
        lib = oracle()
        lib.orc_matcher_create.restype = C.c_void_p
        lib.orc_matcher_create.argtypes = [C.POINTER(MatcherParams)]
        lib.orc_matcher_destroy.argtypes = [C.c_void_p]
        lib.orc_matcher_set_triangulator.argtypes = [C.c_void_p, C.c_void_p]
        lib.orc_matcher_set_intrinsics.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
        lib.orc_matcher_push_back.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        lib.orc_matcher_match_features.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.orc_matcher_get_stage.restype = C.c_int64
        lib.orc_matcher_get_stage.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        lib.orc_matcher_get_features.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        lib.orc_matcher_get_filter.restype = C.c_int64
        lib.orc_matcher_get_filter.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        lib.orc_matcher_get_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.orc_matcher_bucket_features.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float]
        lib.orc_matcher_get_gain.restype = C.c_float
        lib.orc_matcher_get_gain.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        super().__init__(lib, "orc_", params)
        if tri_fn is None:
            tri_fn = C.cast(ref_viso().ref_viso_triangulate, C.c_void_p)
        self._tri = tri_fn   # keep callbacks alive
        lib.orc_matcher_set_triangulator(self.h, tri_fn if isinstance(tri_fn, C.c_void_p)
                                         else C.cast(tri_fn, C.c_void_p))

    def match(self, method, Tr=None, staged=True):
        t = None if Tr is None else _p(np.ascontiguousarray(Tr, np.float64))
        return self.lib.orc_matcher_match_features(self.h, method, t)

    def bucket(self, max_features, bw, bh):
        return self.lib.orc_matcher_bucket_features(self.h, max_features, bw, bh)

    def gain(self, inliers):
        a = np.ascontiguousarray(inliers, np.int32)
        return self.lib.orc_matcher_get_gain(self.h, _p(a), len(a))


def compare_matchers(a, b, method=2):
    """list of (what, n_mismatch) between two matcher drivers after push_back x2 + match"""
    out = []
    for tb in range(8):
        x, y = a.features(tb), b.features(tb)
        out.append(("table_" + M_TABLES[tb], -1 if x.shape != y.shape else int((x != y).sum())))
    for s in range(M_STAGE_COUNT):
        x, y = a.stage(s), b.stage(s)
        if s == M_RANGES:
            # only the stages the method uses are defined (matcher.cpp:1003-1025)
            ns = 4 if method == 2 else 2
            x = x.reshape(-1, 4, 4)[:, :, :ns] if len(x) else x
            y = y.reshape(-1, 4, 4)[:, :, :ns] if len(y) else y
        out.append((M_STAGE_NAMES[s], -1 if x.shape != y.shape else int((x != y).sum())))
    return out


class ProductMatcher(MatcherBase):
    """svh_matcher_* through the C-ABI of libsvhip.so (the HIP path)"""

    def __init__(self, params):
        import svhip
        lib = svhip.lib()
        lib.svh_matcher_create.restype = C.c_void_p
        lib.svh_matcher_create.argtypes = [C.POINTER(MatcherParams)]
        lib.svh_matcher_destroy.argtypes = [C.c_void_p]
        lib.svh_matcher_set_intrinsics.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
        lib.svh_matcher_push_back.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        lib.svh_matcher_match_features.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.svh_matcher_get_stage.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                              C.POINTER(C.c_size_t)]
        lib.svh_matcher_get_features.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        lib.svh_matcher_get_filter.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                               C.POINTER(C.c_size_t), C.c_void_p]
        lib.svh_matcher_get_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.svh_matcher_bucket_features.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float]
        lib.svh_matcher_get_gain.restype = C.c_float
        lib.svh_matcher_get_gain.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        self._svhip = svhip
        super().__init__(lib, "svh_", params)
        lib.svh_matcher_set_taps(C.c_void_p(self.h), 1)   # parity tests read every stage

    def push_back(self, I1, I2=None, replace=False):
        rc = super().push_back(I1, I2, replace)
        if rc < 0:
            raise self._svhip.SvhError(rc, self._svhip.last_error())
        return rc

    def match(self, method, Tr=None, staged=True):
        t = None if Tr is None else _p(np.ascontiguousarray(Tr, np.float64))
        rc = self.lib.svh_matcher_match_features(self.h, method, t)
        if rc < 0:
            raise self._svhip.SvhError(rc, self._svhip.last_error())
        return rc

    def bucket(self, max_features, bw, bh):
        return self.lib.svh_matcher_bucket_features(self.h, max_features, bw, bh)

    def gain(self, inliers):
        a = np.ascontiguousarray(inliers, np.int32)
        return self.lib.svh_matcher_get_gain(self.h, _p(a), len(a))

# ---------------------------------------------------------------------------
# VisualOdometryStereo drivers (reference / oracle / product share one C-ABI shape)
# ---------------------------------------------------------------------------
class VoParams(C.Structure):
    """svh_vo_params (include/svh.h) == VisualOdometryStereo::parameters (viso_stereo.h:30-44)."""
    _fields_ = [
        ("match", MatcherParams), ("bucket_max_features", C.c_int32), ("bucket_width", C.c_double),
        ("bucket_height", C.c_double), ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double),
        ("base", C.c_double), ("ransac_iters", C.c_int32), ("inlier_threshold", C.c_double),
        ("reweighting", C.c_int32),
    ]

    def copy(self, **kw):
        q = VoParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q


def vo_defaults(**kw):
    """VisualOdometryStereo::parameters() with the calibration of libviso2/src/demo.cpp:54-58"""
    p = VoParams()
    p.match = matcher_defaults()
    p.bucket_max_features, p.bucket_width, p.bucket_height = 2, 50.0, 50.0
    p.f, p.cu, p.cv, p.base = 645.24, 635.96, 194.13, 0.5707
    p.ransac_iters, p.inlier_threshold, p.reweighting = 200, 2.0, 1
    return p.copy(**kw)


class VoBase:
    """shared driver over the three VisualOdometryStereo implementations (ref_/orc_/svh_)"""

    def __init__(self, lib, prefix, params):
        self.lib, self.px, self.params = lib, prefix, params
        g = lambda n: getattr(lib, prefix + "vo_" + n)
        g("create").restype = C.c_void_p
        g("create").argtypes = [C.POINTER(VoParams)]
        g("destroy").argtypes = [C.c_void_p]
        g("process").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        g("process_matches").argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        g("estimate_motion").argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        g("get_motion").argtypes = [C.c_void_p, C.c_void_p]
        g("get_inliers").argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        g("get_matches").argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        g("num_matches").argtypes = [C.c_void_p]
        g("get_gain").restype = C.c_float
        g("get_gain").argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        self.h = g("create")(C.byref(params))

    def __del__(self):
        if getattr(self, "h", None):
            getattr(self.lib, self.px + "vo_destroy")(self.h)
            self.h = None

    def _f(self, name):
        return getattr(self.lib, self.px + "vo_" + name)

    def process(self, I1, I2, replace=False):
        I1 = np.ascontiguousarray(I1, np.uint8)
        I2 = np.ascontiguousarray(I2, np.uint8)
        dims = (C.c_int32 * 3)(I1.shape[1], I1.shape[0], I1.shape[1])
        return self._f("process")(self.h, _p(I1), _p(I2), dims, int(replace))

    def process_matches(self, matches):
        m = np.ascontiguousarray(matches, P_MATCH)
        return self._f("process_matches")(self.h, _p(m), len(m))

    def estimate_motion(self, matches):
        m = np.ascontiguousarray(matches, P_MATCH)
        tr = np.zeros(6, np.float64)
        ok = self._f("estimate_motion")(self.h, _p(m), len(m), _p(tr))
        return ok, tr

    def motion(self):
        T = np.zeros((4, 4), np.float64)
        self._f("get_motion")(self.h, _p(T))
        return T

    def inliers(self):
        n = self._f("get_inliers")(self.h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        self._f("get_inliers")(self.h, _p(out), n)
        return out[:n]

    def matches(self):
        n = self._f("get_matches")(self.h, None, 0)
        out = np.zeros(max(n, 1), P_MATCH)
        self._f("get_matches")(self.h, _p(out), n)
        return out[:n]

    def num_matches(self):
        return self._f("num_matches")(self.h)

    def gain(self, inliers):
        inl = np.ascontiguousarray(inliers, np.int32)
        return float(self._f("get_gain")(self.h, _p(inl), len(inl)))

    def hypotheses(self):
        """(votes [n] int32, -1 = FAILED; vectors [n, 6]) of every RANSAC hypothesis of the last stereo estimate
        (svh_vo_get_hypotheses / orc_vo_get_hypotheses; the reference has no such tap)"""
        f = self._f("get_hypotheses")
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        n = f(self.h, None, None, 0)
        assert n >= 0, n
        votes = np.full(max(n, 1), -99, np.int32)
        tr = np.full((max(n, 1), 6), np.nan, np.float64)
        assert f(self.h, _p(votes), _p(tr), n) == n
        return votes[:n], tr[:n]


class RefVo(VoBase):
    def __init__(self, params):
        lib = ref_viso()
        lib.ref_init(1)
        VoBase.__init__(self, lib, "ref_", params)


class OracleVo(VoBase):
    def __init__(self, params, tri_fn=None):
        lib = oracle()
        VoBase.__init__(self, lib, "orc_", params)
        if tri_fn is None:
            tri_fn = C.cast(ref_viso().ref_viso_triangulate, C.c_void_p)
        self._tri = tri_fn
        lib.orc_vo_set_triangulator.argtypes = [C.c_void_p, C.c_void_p]
        lib.orc_vo_set_triangulator(self.h, tri_fn if isinstance(tri_fn, C.c_void_p)
                                    else C.cast(tri_fn, C.c_void_p))

    def set_trig_mode(self, mode, seed=1):
        """orc_vo_set_trig_mode: the linearisation's sines / cosines exact (0), one ulp up (1), down (2), mixed (3)"""
        self.lib.orc_vo_set_trig_mode.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
        self.lib.orc_vo_set_trig_mode(self.h, mode, seed)


class ProductVo(VoBase):
    def __init__(self, params, private_rand=None):
        import svhip as S
        VoBase.__init__(self, S.lib(), "svh_", params)
        if private_rand is not None:   # own generator with glibc's srand(seed) sequence instead of libc rand()
            self.lib.svh_vo_set_private_rand.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
            self.lib.svh_vo_set_private_rand(self.h, 1, private_rand)

def _ptr_array(arrs):
    return (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])


def product_vo_process_batch(vos, I1s, I2s, replace=False, shape=None):
    """svh_vo_process_batch: one frame for K ProductVo objects; returns (n_ok, per-object return values).
    I1s = I2s = None (+ shape = (h, w)): the objects take the frame handed over by product_vo_prefetch_batch"""
    import svhip as S
    lib = S.lib()
    lib.svh_vo_process_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p]
    K = len(vos)
    p1 = p2 = None
    if I1s is not None:
        I1s = [np.ascontiguousarray(a, np.uint8) for a in I1s]
        I2s = [np.ascontiguousarray(a, np.uint8) for a in I2s]
        shape = I1s[0].shape
        p1, p2 = _ptr_array(I1s), _ptr_array(I2s)
    dims = (C.c_int32 * 3)(shape[1], shape[0], shape[1])
    hs = (C.c_void_p * K)(*[v.h for v in vos])
    ok = np.full(K, -99, np.int32)
    rc = lib.svh_vo_process_batch(hs, K, p1, p2, dims, int(replace), _p(ok))
    if rc < 0:
        raise S.SvhError(rc, S.last_error())
    return rc, ok


def _held(arrs):
    """images of a frame handed over early are read by the library until the frame is taken: they must be the
    caller's own contiguous uint8 arrays (a temporary copy made here would be freed too early)"""
    for a in arrs:
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous):
            raise ValueError("hand-over needs contiguous uint8 arrays that the caller keeps alive")
    return list(arrs)


def product_vo_process_next_batch(vos, next_I1s, next_I2s, shape, replace=False):
    """svh_vo_process_next_batch: process the frame handed over before, hand over the next one (or None)"""
    import svhip as S
    lib = S.lib()
    lib.svh_vo_process_next_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p]
    K = len(vos)
    p1 = p2 = None
    if next_I1s is not None:
        next_I1s, next_I2s = _held(next_I1s), _held(next_I2s)
        p1, p2 = _ptr_array(next_I1s), _ptr_array(next_I2s)
    dims = (C.c_int32 * 3)(shape[1], shape[0], shape[1])
    hs = (C.c_void_p * K)(*[v.h for v in vos])
    ok = np.full(K, -99, np.int32)
    rc = lib.svh_vo_process_next_batch(hs, K, p1, p2, dims, int(replace), _p(ok))
    if rc < 0:
        raise S.SvhError(rc, S.last_error())
    return rc, ok


def product_vo_prefetch_batch(vos, I1s, I2s):
    """svh_vo_prefetch_batch: the NEXT frame of K ProductVo objects, handed over early (returns at once)"""
    import svhip as S
    lib = S.lib()
    lib.svh_vo_prefetch_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    K = len(vos)
    I1s, I2s = _held(I1s), _held(I2s)
    dims = (C.c_int32 * 3)(I1s[0].shape[1], I1s[0].shape[0], I1s[0].shape[1])
    hs = (C.c_void_p * K)(*[v.h for v in vos])
    rc = lib.svh_vo_prefetch_batch(hs, K, _ptr_array(I1s), _ptr_array(I2s), dims)
    if rc < 0:
        raise S.SvhError(rc, S.last_error())
    return rc


def product_matcher_prefetch(ms, I1s, I2s):
    """svh_matcher_prefetch_batch"""
    import svhip as S
    lib = S.lib()
    lib.svh_matcher_prefetch_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    K = len(ms)
    hs = (C.c_void_p * K)(*[m.h for m in ms])
    I1s = _held(I1s)
    I2s = None if I2s is None else _held(I2s)
    dims = (C.c_int32 * 3)(I1s[0].shape[1], I1s[0].shape[0], I1s[0].shape[1])
    rc = lib.svh_matcher_prefetch_batch(hs, K, _ptr_array(I1s), None if I2s is None else _ptr_array(I2s), dims)
    if rc < 0:
        raise S.SvhError(rc, S.last_error())
    return rc


def product_matcher_take_prefetched(ms, shape, replace=False):
    """svh_matcher_push_back_batch without images: the objects take their prefetched frame"""
    import svhip as S
    lib = S.lib()
    lib.svh_matcher_push_back_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    K = len(ms)
    hs = (C.c_void_p * K)(*[m.h for m in ms])
    dims = (C.c_int32 * 3)(shape[1], shape[0], shape[1])
    rc = lib.svh_matcher_push_back_batch(hs, K, None, None, dims, int(replace))
    if rc < 0:
        raise S.SvhError(rc, S.last_error())
    return rc


def product_matcher_batch(ms, I1s, I2s, method, Trs=None, replace=False, push=True):
    """svh_matcher_push_back_batch (+ svh_matcher_match_features_batch when method is not None)"""
    import svhip as S
    lib = S.lib()
    lib.svh_matcher_push_back_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.svh_matcher_match_features_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    K = len(ms)
    hs = (C.c_void_p * K)(*[m.h for m in ms])
    if push:
        I1s = [np.ascontiguousarray(a, np.uint8) for a in I1s]
        I2s = None if I2s is None else [None if a is None else np.ascontiguousarray(a, np.uint8) for a in I2s]
        dims = (C.c_int32 * 3)(I1s[0].shape[1], I1s[0].shape[0], I1s[0].shape[1])
        rc = lib.svh_matcher_push_back_batch(hs, K, _ptr_array(I1s), None if I2s is None else _ptr_array(I2s),
                                             dims, int(replace))
        if rc < 0:
            raise S.SvhError(rc, S.last_error())
    if method is not None:
        trs = None
        if Trs is not None:
            keep = [None if t is None else np.ascontiguousarray(t, np.float64) for t in Trs]
            trs = _ptr_array(keep)
        rc = lib.svh_matcher_match_features_batch(hs, K, method, trs)
        if rc < 0:
            raise S.SvhError(rc, S.last_error())
    return 0


def synth_vo_matches(n, seed=0, motion=(0.004, -0.01, 0.002, 0.03, -0.01, -0.8), outliers=0.25,
                     noise=0.3, calib=(645.24, 635.96, 194.13, 0.5707), size=(1344, 391)):
    """quad matches of random 3-D points seen before / after a known rigid motion (the model of
    viso_stereo.cpp:113-131, 379-475), with pixel noise and a fraction of gross outliers"""
    rng = np.random.default_rng(seed)
    f, cu, cv, base = calib
    rx, ry, rz, tx, ty, tz = motion
    sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    R = np.array([[cy * cz, -cy * sz, sy],
                  [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                  [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]])
    out = np.zeros(n, P_MATCH)
    k = 0
    while k < n:
        Z = rng.uniform(4, 60)
        u1p, v1p = rng.uniform(20, size[0] - 20), rng.uniform(20, size[1] - 20)
        X, Y = (u1p - cu) * Z / f, (v1p - cv) * Z / f
        Xc = R @ np.array([X, Y, Z]) + np.array([tx, ty, tz])
        if Xc[2] < 1:
            continue
        u1c, v1c = f * Xc[0] / Xc[2] + cu, f * Xc[1] / Xc[2] + cv
        u2p, u2c = u1p - f * base / Z, u1c - f * base / Xc[2]
        m = np.array([u1p, v1p, u2p, v1p, u1c, v1c, u2c, v1c]) + rng.normal(0, noise, 8)
        if rng.uniform() < outliers:
            m[4:] += rng.uniform(-40, 40, 4)
        if not (0 < m[4] < size[0] and 0 < m[5] < size[1]):
            continue
        out[k] = (m[0], m[1], k, m[2], m[3], k, m[4], m[5], k, m[6], m[7], k)
        k += 1
    return out

def fuzz_elas_params(seed):
    """a seeded random point of Elas::parameters inside the ranges the reference handles
    (elas.h:59-148): every field moves, both filters / corner points / subsampling toggle"""
    rng = np.random.default_rng(seed)
    base = robotics() if rng.uniform() < 0.5 else middlebury()
    prm = base.copy(
        disp_max=int(rng.integers(24, 200)),
        support_threshold=float(rng.uniform(0.7, 0.98)),
        support_texture=int(rng.integers(0, 40)),
        candidate_stepsize=int(rng.integers(3, 8)),
        incon_window_size=int(rng.integers(3, 8)),
        incon_threshold=int(rng.integers(2, 8)),
        incon_min_support=int(rng.integers(2, 8)),
        add_corners=int(rng.integers(0, 2)),
        grid_size=int(rng.integers(10, 32)),
        beta=float(rng.uniform(0.01, 0.05)),
        gamma=float(rng.uniform(1.0, 8.0)),
        sigma=float(rng.uniform(0.6, 2.0)),
        sradius=float(rng.uniform(1.5, 3.5)),
        match_texture=int(rng.integers(0, 4)),
        lr_threshold=int(rng.integers(1, 4)),
        speckle_sim_threshold=float(rng.uniform(0.5, 2.5)),
        speckle_size=int(rng.integers(20, 400)),
        ipol_gap_width=int(rng.integers(2, 12)),
        filter_median=int(rng.integers(0, 2)),
        filter_adaptive_mean=int(rng.integers(0, 2)),
        postprocess_only_left=int(rng.integers(0, 2)),
        subsampling=int(rng.uniform() < 0.25),
    )
    # round 6: disp_min (elas.h:61, elas.cpp:384-396) moves too, -8 .. 40; drawn last so that every other field of
    # a seed keeps the value it had in the earlier rounds' fuzz records.  Two thirds of the points: the rest keep 0
    dmin = int(rng.integers(-8, 41))
    if rng.uniform() < 2.0 / 3.0:
        prm = prm.copy(disp_min=min(dmin, prm.disp_max - 12))
    return prm

def fuzz_matcher_case(seed):
    """a seeded random point of Matcher::parameters (matcher.h:41-69), a matching method, a crop of
    the quad (ragged widths) and optionally a predicted motion + intrinsics"""
    rng = np.random.default_rng(seed)
    prm = matcher_defaults(
        nms_n=int(rng.integers(2, 7)), nms_tau=int(rng.integers(20, 90)),
        match_binsize=int(rng.integers(25, 90)), match_radius=int(rng.integers(60, 260)),
        match_disp_tolerance=int(rng.integers(1, 4)), outlier_disp_tolerance=int(rng.integers(2, 9)),
        outlier_flow_tolerance=int(rng.integers(2, 9)), multi_stage=int(rng.integers(0, 2)),
        half_resolution=int(rng.integers(0, 2)), refinement=int(rng.integers(0, 3)))
    method = int(rng.integers(0, 3))
    x0, y0 = int(rng.integers(0, 200)), int(rng.integers(0, 40))
    w, h = int(rng.integers(600, 1100)), int(rng.integers(220, 340))
    tr = None
    if method == 2 and rng.uniform() < 0.5:
        prm = prm.copy(f=645.24, cu=635.96 - x0, cv=194.13 - y0, base=0.5707)
        tr = np.eye(4)
        tr[:3, 3] = rng.uniform(-0.05, 0.05, 3)
        tr[2, 3] -= 0.7
    return prm, method, (slice(y0, y0 + h), slice(x0, x0 + w)), tr

def fuzz_vo_params(seed):
    """a seeded random point of VisualOdometryStereo::parameters (viso_stereo.h:30-44, viso.h:30-66)"""
    rng = np.random.default_rng(seed)
    p = vo_defaults(
        bucket_max_features=int(rng.integers(1, 6)), bucket_width=float(rng.integers(30, 90)),
        bucket_height=float(rng.integers(30, 90)), ransac_iters=int(rng.integers(20, 260)),
        inlier_threshold=float(rng.uniform(1.0, 3.0)), reweighting=int(rng.integers(0, 2)))
    m = p.match
    m.nms_n = int(rng.integers(2, 5))
    m.match_binsize = int(rng.integers(30, 70))
    m.refinement = int(rng.integers(0, 3))
    m.half_resolution = int(rng.integers(0, 2))
    m.outlier_flow_tolerance = int(rng.integers(3, 8))
    p.match = m
    return p


# ----------------------------------------------------------------------------- full-size fixtures
def _unfilter_rows(d):
    """inverse of the horizontal difference filter the full-size image fixtures are stored with"""
    return np.cumsum(d, axis=1, dtype=np.uint8)


def full_image(name):
    """one full-size gray image under tests/golden/full (make_goldens_full.py): uint8 (h, w)"""
    with np.load(os.path.join(GOLDEN, "full", name + ".npz")) as z:
        return _unfilter_rows(z["rows"])


def full_pair(name):
    """a full-size ELAS pair of the reference's (urban1-4, cones, aloe, raindeer)"""
    return full_image(name + "_left"), full_image(name + "_right")


def mono_frames():
    """the seven frames I1_000000..6 of the reference's mono sequence, gray"""
    return [full_image("I1_%06d" % k) for k in range(7)]


def stage_sha256(a):
    """sha256 of a stage's bytes; float arrays with -0.0 taken as +0.0 (the float compares are value compares)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        a = np.where(a == 0, np.float32(0), a).astype(np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def full_case(case):
    """golden record of one full-size ELAS case: (npz, params, left, right)"""
    z = np.load(os.path.join(GOLDEN, "full", "elas_" + case + ".npz"))
    prm = ElasParams.from_buffer_copy(z["params"].tobytes())
    l, r = full_pair(str(z["pair"]))
    return z, prm, l, r
