"""The reference's PlaneEstimation, built from the reference sources into a temporary directory, and the cases of
the ground-plane golden fixture (tests/golden/plane.npz).  Used by tests/golden/make_goldens_plane.py and by the live
check in tests/test_plane.py; the GPU tests read only committed fixtures.

The driver (tests/plane/ref_plane_harness.cpp) is this project's text.  It is linked against the reference's
libviso2/src/matrix.cpp and stereomapper/planeestimation.cpp, both compiled unchanged with the flags of
oracle/Makefile, the latter with tests/plane/plane_prelude.h force-included (see there).

The fixture stores recorded results only.  The inputs are the `d1` maps of committed goldens or are derived here from
closed integer / float32 formulas (no library random generator)."""
import hashlib
import os
import struct
import subprocess

import numpy as np

import helpers as H

REF = os.environ.get("REF", "/root/reference")
HERE = os.path.join(H.ROOT, "tests", "plane")
REFFLAGS = ["-O3", "-DNDEBUG", "-msse3", "-fPIC", "-w", "-std=c++11"]   # oracle/Makefile
GOLDEN = os.path.join(H.GOLDEN, "plane.npz")
CALIB = (721.5, 609.6, 172.9, 0.54)     # f, cu, cv, base of the probe in the issue (KITTI-like)
NUM_SAMPLES = 5000
OK, NO_POINTS, FEW_INLIERS = 0, 2, 3
URBAN = ["urban1_robotics", "urban2_stereomapper", "urban3_kitti", "urban4_kitti"]
W, HGT = 1242, 375
# cases whose per-hypothesis planes are stored in full (the others store their SHA-256)
FULL_PLANES = ("urban2_stereomapper_s2", "small_s0")


def have_ref():
    return os.path.isfile(os.path.join(REF, "stereomapper", "planeestimation.cpp"))


def build_harness(tmp):
    """compile the reference objects and the driver into tmp; returns the program's path"""
    viso, sm = os.path.join(REF, "libviso2", "src"), os.path.join(REF, "stereomapper")
    objs = [os.path.join(tmp, "matrix.o"), os.path.join(tmp, "planeestimation.o")]
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + viso, "-c", os.path.join(viso, "matrix.cpp"), "-o", objs[0]])
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + sm, "-include", os.path.join(HERE, "plane_prelude.h"), "-c",
                           os.path.join(sm, "planeestimation.cpp"), "-o", objs[1]])
    exe = os.path.join(tmp, "ref_plane_harness")
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + sm, os.path.join(HERE, "ref_plane_harness.cpp")] + objs +
                          ["-o", exe])
    return exe


# ------------------------------------------------------------------------------------------------------------ maps
def urban_d1(name):
    with np.load(os.path.join(H.GOLDEN, name + ".npz")) as z:
        return np.ascontiguousarray(z["d1"], np.float32).reshape(HGT, W)


def noise(h, w, mul=1):
    """a fixed pattern in [0, 1): an integer hash of (u, v), exact in int64 and float32"""
    v, u = np.mgrid[0:h, 0:w].astype(np.int64)
    k = (u * 7919 + v * 104729 + (u * v) % 8191 * 31 * mul) % 1000
    return (k.astype(np.float32) / np.float32(1000)).astype(np.float32)


def wall_map():
    """640x240: a road (d grows with v) right of u = 400 and a fronto-parallel wall (d = 20) left of it, which covers
    more than half of the region of interest"""
    h, w = 240, 640
    v, u = np.mgrid[0:h, 0:w]
    road = (np.float32(0.3) * (v - 100).astype(np.float32) + noise(h, w) - np.float32(0.5)).astype(np.float32)
    wall = (np.float32(20) + noise(h, w, 3) - np.float32(0.5)).astype(np.float32)
    return np.where(u < 400, wall, np.maximum(road, np.float32(0))).astype(np.float32)


def small_map(lo, span):
    """90x60: no third point can be 50 px from a line through two others, and a first point near the middle has no
    second point 50 px away"""
    return (np.float32(lo) + np.float32(span) * noise(60, 90)).astype(np.float32)


def few_map(k):
    """200x120 with k lattice points >= 1, far apart and not on a line"""
    D = np.zeros((120, 200), np.float32)
    for (u, v, d) in [(10, 40, 12.0), (150, 45, 14.0), (80, 115, 30.0)][:k]:
        D[v, u] = d
    return D


def half_map(name):
    """621x187: every second pixel of the first 374 rows"""
    return np.ascontiguousarray(urban_d1(name)[:374:2, ::2])


def cases():
    """[(name, [call, ...])]: the calls run on one object in order, the LAST one is what the fixture records.
    call = (map (h, step) float32, width, seed)"""
    out = []
    for name in URBAN:
        for seed in (0, 2, 12345):
            out.append(("%s_s%d" % (name, seed), [(urban_d1(name), W, seed)]))
    wide = np.zeros((HGT, 1280), np.float32)
    wide[:, :W] = urban_d1("urban2_stereomapper")
    out.append(("embedded_s2", [(wide, W, 2)]))
    for seed in (0, 7):   # the identity branch keeps the pitch of the road call before it
        out.append(("wall_s%d" % seed, [(urban_d1("urban2_stereomapper"), W, 2), (wall_map(), 640, seed)]))
    for seed in (0, 7):
        out.append(("small_s%d" % seed, [(small_map(10, 20), 90, seed)]))
    out.append(("lowd_s0", [(small_map(1, 3.9), 90, 0)]))
    out.append(("two_s0", [(few_map(2), 200, 0)]))
    out.append(("three_s0", [(few_map(3), 200, 0)]))
    out.append(("half_s2", [(half_map("urban4_kitti"), 621, 2)]))
    return out


# --------------------------------------------------------------------------------------------------------- harness
def write_job(path, calls, calib=CALIB):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(calls)))
        for D, width, seed in calls:
            D = np.ascontiguousarray(D, np.float32)
            f.write(struct.pack("<iiiffffI", width, D.shape[0], D.shape[1], *calib, seed))
            f.write(D.tobytes())


def parse_run(b, n_calls):
    """the driver's output (also written by tests/plane/plane_core_check.cpp): one dict per call"""
    at, out = 0, []

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(b, dtype, count, at).copy()
        at += a.nbytes
        return a

    for _ in range(n_calls):
        r = {"status": int(take(np.int32, 1)[0]), "plane_d": take(np.float64, 3), "plane_e": take(np.float64, 3),
             "H": take(np.float64, 16).reshape(4, 4), "pitch": take(np.float32, 1)[0]}
        n = int(take(np.int32, 1)[0])
        r["list"] = take(np.float32, 3 * n).reshape(-1, 3)
        S = int(take(np.int32, 1)[0])
        r["planes"] = take(np.float64, 3 * S).reshape(-1, 3)
        r["draws"] = take(np.int32, S)
        r["votes"] = take(np.int32, S)
        r["best"] = int(take(np.int32, 1)[0])
        nin = int(take(np.int32, 1)[0])
        r["inliers"] = take(np.int32, nin)
        out.append(r)
    assert at == len(b), (at, len(b))
    return out


def run_calls(exe, tmp, calls):
    path = os.path.join(tmp, "job.bin")
    write_job(path, calls)
    b = subprocess.run([exe, "run", path], check=True, capture_output=True).stdout
    return parse_run(b, len(calls))


def run_bench(exe, tmp, calls, reps):
    path = os.path.join(tmp, "job.bin")
    write_job(path, calls)
    return subprocess.run([exe, "bench", path, str(reps)], check=True, capture_output=True, text=True).stdout.strip()


# --------------------------------------------------------------------------------------------------------- fixture
def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def pack_result(out, name, r):
    k = name + "_"
    out[k + "status"] = np.int32(r["status"])
    out[k + "plane_d"], out[k + "plane_e"], out[k + "H"] = r["plane_d"], r["plane_e"], r["H"]
    out[k + "pitch"] = np.float32(r["pitch"])
    out[k + "n"] = np.int32(len(r["list"]))
    out[k + "list_sha"] = sha(r["list"])
    out[k + "planes_sha"] = sha(r["planes"])
    if name in FULL_PLANES:
        out[k + "planes"] = r["planes"]
    assert r["draws"].max() < 32768 and r["votes"].max() < 32768
    out[k + "draws"] = r["draws"].astype(np.int16)
    out[k + "votes"] = r["votes"].astype(np.int16)
    out[k + "best"] = np.int32(r["best"])
    mask = np.zeros(len(r["list"]), np.uint8)
    mask[r["inliers"]] = 1
    assert np.array_equal(np.flatnonzero(mask), r["inliers"])     # ascending, no repeats
    out[k + "inlier_bits"] = np.packbits(mask)


def unpack_result(Z, name):
    k = name + "_"
    n = int(Z[k + "n"])
    r = {"status": int(Z[k + "status"]), "plane_d": Z[k + "plane_d"], "plane_e": Z[k + "plane_e"], "H": Z[k + "H"],
         "pitch": np.float32(Z[k + "pitch"]), "n": n, "list_sha": Z[k + "list_sha"], "planes_sha": Z[k + "planes_sha"],
         "planes": Z.get(k + "planes"), "draws": Z[k + "draws"].astype(np.int32),
         "votes": Z[k + "votes"].astype(np.int32), "best": int(Z[k + "best"]),
         "inliers": np.flatnonzero(np.unpackbits(Z[k + "inlier_bits"])[:n]).astype(np.int32)}
    return r


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def same_result(got, want, where):
    """got: a dict as parse_run gives it; want: unpack_result of the fixture.  Everything is compared exactly; the
    doubles bit for bit."""
    assert got["status"] == want["status"], (where, "status", got["status"], want["status"])
    assert len(got["list"]) == want["n"], (where, "list length", len(got["list"]), want["n"])
    assert np.array_equal(sha(np.ascontiguousarray(got["list"], np.float32)), want["list_sha"]), (where, "list")
    assert np.array_equal(got["draws"], want["draws"]), (where, "draws", np.flatnonzero(got["draws"] != want["draws"])[:5])
    assert np.array_equal(got["votes"], want["votes"]), (where, "votes", np.flatnonzero(got["votes"] != want["votes"])[:5])
    assert got["best"] == want["best"], (where, "best", got["best"], want["best"])
    assert np.array_equal(got["inliers"], want["inliers"]), (where, "inliers")
    if want["planes"] is not None:
        g, w = np.ascontiguousarray(got["planes"], np.float64), want["planes"]
        assert g.shape == w.shape, (where, "planes")
        bad = np.flatnonzero((g.view(np.uint64) != w.view(np.uint64)).any(axis=1))
        assert len(bad) == 0, (where, "planes", bad[:5], g[bad[:1]], w[bad[:1]])
    assert np.array_equal(sha(np.ascontiguousarray(got["planes"], np.float64)), want["planes_sha"]), (where, "planes")
    for key in ("plane_d", "plane_e", "H"):
        g = np.ascontiguousarray(got[key], np.float64).ravel()
        w = np.ascontiguousarray(want[key], np.float64).ravel()
        assert g.tobytes() == w.tobytes(), (where, key, g, w)
    assert np.float32(got["pitch"]).tobytes() == np.float32(want["pitch"]).tobytes(), (where, "pitch", got["pitch"],
                                                                                         want["pitch"])


# ------------------------------------------------------------------------------------------------------------ edges
# tests/golden/plane_edges.npz (make_goldens_plane_edges.py): 640x240 maps whose lattice lists have exactly the lengths
# at which k_plane_grid, k_plane_vote and k_plane_select change rounds, and noiseless planar roads on which votes tie.
EDGE_GOLDEN = os.path.join(H.GOLDEN, "plane_edges.npz")
EDGE_W, EDGE_H = 640, 240
EDGE_NU, EDGE_NV = 128, 32                      # lattice of the region of interest (rows 80..235, every 5th pixel)
EDGE_LENGTHS = (1, 1023, 1024, 1025, 2048)
EDGE_SEED = 3
EDGE_TIE_SEEDS = (2, 4, 8)                      # searched on the reference: make_goldens_plane_edges.py --search


def edge_cells(k):
    """(u, v) of k cells of the lattice, scattered over it: cell t is chosen when 7919 t mod 4096 < k (a bijection)"""
    t = np.arange(EDGE_NU * EDGE_NV, dtype=np.int64)
    t = t[(t * 7919) % (EDGE_NU * EDGE_NV) < k]
    return 5 * (t // EDGE_NV), EDGE_H // 3 + 5 * (t % EDGE_NV)


def list_map(k):
    """an empty map with d >= 1 on exactly k lattice cells: a road with noise in [0, 14), so that no hypothesis gets
    every point (d_threshold is 5)"""
    v, u = np.mgrid[0:EDGE_H, 0:EDGE_W]
    road = (np.float32(0.25) * (v - 70).astype(np.float32) + np.float32(14) * noise(EDGE_H, EDGE_W)).astype(np.float32)
    D = np.zeros((EDGE_H, EDGE_W), np.float32)
    cu, cv = edge_cells(k)
    D[cv, cu] = road[cv, cu]
    return D


def planar_map(off_plane=0):
    """a noiseless planar road over the whole map; `off_plane` lattice cells lie 40 above it"""
    v, u = np.mgrid[0:EDGE_H, 0:EDGE_W]
    D = (np.float32(0.25) * (v - 70).astype(np.float32) + np.float32(0.02) * u.astype(np.float32)).astype(np.float32)
    cu, cv = edge_cells(off_plane)
    D[cv, cu] += np.float32(40)
    return D


def tie_of(votes, lanes=1024):
    """(h0, h1, count, how many reach it): h0 the first hypothesis with the most votes, h1 the first later one with as
    many in a lower lane of k_plane_select; None when there is no such h1"""
    most = np.flatnonzero(votes == votes.max())
    later = [int(h) for h in most[1:] if h % lanes < most[0] % lanes]
    return (int(most[0]), later[0], int(votes.max()), len(most)) if later else None


def edge_cases():
    """as cases(): [(name, [call, ...])]"""
    out = [("list%d_s%d" % (k, EDGE_SEED), [(list_map(k), EDGE_W, EDGE_SEED)]) for k in EDGE_LENGTHS]
    out.append(("planar_s%d" % EDGE_SEED, [(planar_map(), EDGE_W, EDGE_SEED)]))
    for seed in EDGE_TIE_SEEDS:
        out.append(("planar_out_s%d" % seed, [(planar_map(1024), EDGE_W, seed)]))
    return out
