"""The reference's VisualOdometryMono, built from the reference sources into a temporary directory, and the
inputs of the mono golden fixture (tests/golden/vo_mono.npz).  Used by tests/golden/make_goldens_mono.py and by the
live check in tests/test_vo_mono.py; the GPU tests read only the committed fixture.

The driver (tests/mono/ref_mono_harness.cpp) is this project's text.  It is linked against the reference's
libviso2/src/{matcher,filter,matrix,triangle,viso}.cpp, built with the flags of oracle/Makefile, and against
viso_mono.cpp, built with tests/mono/mono_prelude.h force-included (see there)."""
import os
import struct
import subprocess

import numpy as np

import helpers as H

REF = os.environ.get("REF", "/root/reference")
HERE = os.path.join(H.ROOT, "tests", "mono")
REFFLAGS = ["-O3", "-DNDEBUG", "-msse3", "-fPIC", "-w", "-std=c++11"]   # oracle/Makefile
GOLDEN = os.path.join(H.GOLDEN, "vo_mono.npz")

# parameter vector of the harness: f cu cv height pitch ransac_iters inlier_threshold motion_threshold
# max_features bucket_width bucket_height
DEMO = dict(f=645.2, cu=635.9, cv=194.1, height=1.6, pitch=-0.08, ransac_iters=2000, inlier_threshold=1e-5,
            motion_threshold=100.0, max_features=2, bucket_width=50.0, bucket_height=50.0)
PARAM_ORDER = ["f", "cu", "cv", "height", "pitch", "ransac_iters", "inlier_threshold", "motion_threshold",
               "max_features", "bucket_width", "bucket_height"]

# the three sequence runs: (name, parameters, demo_viso_mono.m's replace logic)
SEQUENCES = [
    ("demo", dict(DEMO), True),
    ("still", dict(DEMO, motion_threshold=1e6), False),
    ("alt", dict(DEMO, ransac_iters=500, inlier_threshold=1e-4, motion_threshold=1e6, max_features=3,
                 bucket_width=40.0, bucket_height=30.0), True),
]


def have_ref():
    return os.path.isfile(os.path.join(REF, "libviso2", "src", "viso_mono.cpp"))


def param_vector(p):
    return np.array([float(p[k]) for k in PARAM_ORDER], np.float64)


def param_args(vec):
    out = []
    for k, v in zip(PARAM_ORDER, vec):
        out.append(str(int(v)) if k in ("ransac_iters", "max_features") else repr(float(v)))
    return out


def build_harness(tmp):
    """compile the reference objects and the driver into tmp; returns the program's path"""
    src = os.path.join(REF, "libviso2", "src")
    objs = []
    for name in ("matcher", "filter", "matrix", "triangle", "viso"):
        o = os.path.join(tmp, name + ".o")
        subprocess.check_call(["g++"] + REFFLAGS + ["-I" + src, "-c", os.path.join(src, name + ".cpp"), "-o", o])
        objs.append(o)
    o = os.path.join(tmp, "viso_mono.o")
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + src, "-include", os.path.join(HERE, "mono_prelude.h"), "-c",
                           os.path.join(src, "viso_mono.cpp"), "-o", o])
    objs.append(o)
    exe = os.path.join(tmp, "ref_mono_harness")
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + src, os.path.join(HERE, "ref_mono_harness.cpp")] + objs +
                          ["-o", exe])
    return exe


def write_frames(tmp):
    for k, img in enumerate(H.mono_frames()):
        H.write_pgm(os.path.join(tmp, "I1_%06d.pgm" % k), img)


class _Reader:
    def __init__(self, b):
        self.b, self.at = b, 0

    def i32(self):
        v = struct.unpack_from("<i", self.b, self.at)[0]
        self.at += 4
        return v

    def arr(self, dtype, n):
        dt = np.dtype(dtype)
        a = np.frombuffer(self.b, dt, n, self.at).copy()
        self.at += dt.itemsize * n
        return a

    def state(self):
        inl = self.arr(np.int32, self.i32())
        return inl, self.arr(np.float64, 16).reshape(4, 4)


def run_sequence(exe, tmp, params, demo_replace):
    """per frame: (ok, bucketed matches, inlier indices, 4x4 motion)"""
    b = subprocess.run([exe, "seq", tmp, str(int(demo_replace))] + param_args(param_vector(params)),
                       check=True, capture_output=True).stdout
    r, out = _Reader(b), []
    for _ in range(7):
        ok = r.i32()
        m = r.arr(H.P_MATCH, r.i32())
        inl, T = r.state()
        out.append((ok, m, inl, T))
    return out


def run_estimate(exe, tmp, pvec, matches):
    """VisualOdometry::process(p_matched) on a fresh object: (ok, inliers, motion, per-hypothesis votes)"""
    path = os.path.join(tmp, "matches.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(matches)))
        f.write(np.ascontiguousarray(matches, H.P_MATCH).tobytes())
    b = subprocess.run([exe, "est", path] + param_args(pvec), check=True, capture_output=True).stdout
    r = _Reader(b)
    ok = r.i32()
    inl, T = r.state()
    votes = r.arr(np.int32, r.i32())
    return ok, inl, T, votes


def synth_scene(n, seed, ground=0.6, noise=0.3, outliers=0.2, above=False, rot=(0.004, 0.012, -0.003),
                t=(0.05, -0.02, -1.1), p=DEMO):
    """two views of ground-plane points (y = height in the first camera, y pointing down) and free 3-D points,
    moved by a known R|t, with pixel noise and a share of outliers (random pixel pairs).  above=True: free points
    only, all above the camera (no point passes the plane vote's d > median/motion_threshold at pitch 0)."""
    rng = np.random.default_rng(seed)
    f, cu, cv, h = p["f"], p["cu"], p["cv"], p["height"]
    ng = 0 if above else int(round(n * ground))
    X = np.empty((n, 3))
    X[:ng, 0] = rng.uniform(-12, 12, ng)
    X[:ng, 1] = h
    X[:ng, 2] = rng.uniform(4, 40, ng)
    nf = n - ng
    X[ng:, 0] = rng.uniform(-15, 15, nf)
    X[ng:, 1] = rng.uniform(-6, -0.5, nf) if above else rng.uniform(-6, 1.2, nf)
    X[ng:, 2] = rng.uniform(5, 60, nf)
    rx, ry, rz = rot
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    Xc = X @ (Rx @ Ry @ Rz).T + np.asarray(t)
    up, vp = f * X[:, 0] / X[:, 2] + cu, f * X[:, 1] / X[:, 2] + cv
    uc, vc = f * Xc[:, 0] / Xc[:, 2] + cu, f * Xc[:, 1] / Xc[:, 2] + cv
    up, vp, uc, vc = (a + rng.normal(0, noise, n) for a in (up, vp, uc, vc))
    bad = rng.random(n) < outliers
    nb = int(bad.sum())
    up[bad], uc[bad] = rng.uniform(0, 1240, nb), rng.uniform(0, 1240, nb)
    vp[bad], vc[bad] = rng.uniform(0, 375, nb), rng.uniform(0, 375, nb)
    m = np.zeros(n, H.P_MATCH)
    m["u1p"], m["v1p"], m["u1c"], m["v1c"] = up, vp, uc, vc
    m["i1p"] = m["i1c"] = np.arange(n)
    return m


def estimate_cases():
    """(name, parameter vector, matches) of the estimate-only cases: synthetic scenes and degenerate inputs"""
    cases = []
    for n, seed in ((9, 1), (10, 2), (200, 3), (2000, 4), (5000, 5)):
        cases.append(("syn%d" % n, param_vector(DEMO), synth_scene(n, seed, outliers=0.0 if n <= 10 else 0.2)))
    cases.append(("syn350_alt", param_vector(dict(DEMO, ransac_iters=500, inlier_threshold=1e-4,
                                                  motion_threshold=1e6)), synth_scene(350, 6)))
    same = synth_scene(50, 7)
    for k in ("u1p", "v1p", "u1c", "v1c"):
        same[k] = same[k][0]
    cases.append(("identical", param_vector(DEMO), same))          # normalizeFeaturePoints fails
    cases.append(("few_positive", param_vector(dict(DEMO, inlier_threshold=1e3)),
                  synth_scene(12, 8, outliers=1.0)))                # random pairs, every match an inlier: fails in the tail
    cases.append(("no_plane", param_vector(dict(DEMO, pitch=0.0, motion_threshold=1e6)),
                  synth_scene(300, 9, above=True, outliers=0.0)))   # no d > median/threshold: best_idx stays 0
    return cases


# ------------------------------------------------------------------------------------------------------------ edges
# tests/golden/vo_mono_edges.npz (make_goldens_mono_edges.py): estimate-only cases at the sizes the kernels of
# vo_mono_kernels.hip stride by, and cases in which several RANSAC hypotheses reach the largest inlier count.
EDGE_GOLDEN = os.path.join(H.GOLDEN, "vo_mono_edges.npz")
EDGE_N = (63, 64, 65, 255, 256, 257, 1024)          # k_mono_vote strides N by 64, k_mono_select / k_mono_pick by 256
EDGE_ITERS = (0, 1, 31, 32, 33, 255, 256, 257)      # k_mono_hyp packs 32 hypotheses, k_mono_select strides by 256
EDGE_ITERS_N = 300
# (name, N, seed, inlier_threshold): noiseless inliers, half the matches random pairs.  The seeds were searched on the
# reference (make_goldens_mono_edges.py --search) until its votes met tie_of() below and
# tests/test_vo_mono_edges.py found the tied hypotheses' inlier sets different
EDGE_TIES = (("tie_low", 200, 256, 1e-4), ("tie_high", 200, 161, 1e-4), ("tie_loose", 120, 168, 1e-3))


def tie_of(votes):
    """(h0, h1, count, how many reach it): h0 the first hypothesis with the most inliers, h1 the first later one with
    as many in a lower lane of k_mono_select (h1 % 256 < h0 % 256); None when there is no such h1.  A reduction that
    prefers the lower lane to the lower index returns h1."""
    if len(votes) == 0:
        return None
    most = np.flatnonzero(votes == votes.max())
    later = [int(h) for h in most[1:] if h % 256 < most[0] % 256]
    return (int(most[0]), later[0], int(votes.max()), len(most)) if later else None


def lane_winners(votes, lanes=256):
    """what a reduction over `lanes` lanes returns when it breaks ties by lane instead of by index: every lane keeps
    the first of its maxima, then the lowest lane wins, or the highest"""
    most = np.flatnonzero(votes == votes.max())
    kept = {}
    for h in most:
        kept.setdefault(int(h) % lanes, int(h))
    return kept[min(kept)], kept[max(kept)]


def edge_cases():
    """(name, parameter vector, matches) of vo_mono_edges.npz"""
    cases = []
    for k, n in enumerate(EDGE_N):
        cases.append(("n%d" % n, param_vector(DEMO), synth_scene(n, 40 + k)))
    for it in EDGE_ITERS:
        cases.append(("iters%d" % it, param_vector(dict(DEMO, ransac_iters=it)), synth_scene(EDGE_ITERS_N, 60, noise=0.1)))
    for name, n, seed, thr in EDGE_TIES:
        cases.append((name, param_vector(dict(DEMO, inlier_threshold=thr, motion_threshold=1e6)),
                      synth_scene(n, seed, ground=0.3, noise=0.0, outliers=0.5)))
    return cases
