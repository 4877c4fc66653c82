"""CPU: where multiply covered pixels of the ownership rasteriser can lie, which is what the corner form of the fix
pass (k_owner_corner) rests on.  Triangles are rasterised in numpy with the reference's float32 operations (elas.cpp
1026-1115: corners sorted by u with the exchange loop, the three edge lines, v = (int32)(uint32)(a * u + b) for every
column of [uA, uC)), and the slot flag of the product is restated with the same operations:

  M  in a column other than uA, the two truncated lines stand in the order that contradicts the exact orientation of
     the sorted corners and differ (k_owner, plain pass);
  V  a line through a corner P, evaluated at P's own column, does not truncate to Pv - 1 or Pv (k_prior);
  B  for uA < uB < uC, line AC at column uB truncates to the wrong side of the integer Bv (k_prior).

For every mesh whose flag is clear, every multiply covered pixel must lie, for its highest-index coverer, in column uA
or uB of that coverer and in one of the rows va, va + 1, vb - 2, vb - 1 of its span there -- the pixels the corner form
re-checks.  Meshes: both sides of the five 1242x375 goldens that carry triangle lists (none may be flagged), random
lattice triangulations, and adversarial ones (sparse points on widths up to 9000, collinear fans from a far vertex,
tall narrow strips, vertices one row off a long edge).

The last test looks for meshes the flag must catch: coordinates up to 60000 x 3000, where |a * u| passes 2^22 and one
float32 ulp of an edge line is half a row or more.  No inverted pair of bounds (M) and no multiply covered pixel
outside the corner set could be produced there, with |a * u| up to 2^27: random points in a few steep columns, slivers
along a steep edge -- the two lines of a triangle carry nearly the same error.  What does happen is V, a line missing
its own corner by more than a row, in 38 of the 60 meshes.  So the test asserts what it can (a pixel outside the
corner set implies a flag; V fires), and the fallback path behind the flag is exercised on the device with
SVH_OWNER_FORCE_WALK (tests/test_owner_corner_fix_gpu.py)."""
import os

import numpy as np
import pytest

import helpers as H

f32 = np.float32
GOLDENS = ["urban1_robotics", "urban2_kitti", "urban3_kitti", "urban4_kitti", "urban2_stereomapper"]


def f2u2i(x):
    """(int32)(uint32)x of the reference (elas.cpp:1081-1082) for float32 line values"""
    return x.astype(np.int64).astype(np.uint32).astype(np.int32).astype(np.int64)


def line_at(a, b, u):
    return f2u2i((a * u.astype(f32)).astype(f32) + b)


def records(pts, tris):
    """the raster records of k_prior for integer points (n, 2) and corner triples (m, 3)"""
    tu = pts[tris, 0].astype(f32)
    tv = pts[tris, 1].astype(f32)
    for j in range(3):                      # the reference's exchange loop (elas.cpp:1044-1053), not stable on ties
        for k in range(j):
            sw = tu[:, k] > tu[:, j]
            tu[sw, j], tu[sw, k] = tu[sw, k], tu[sw, j]
            tv[sw, j], tv[sw, k] = tv[sw, k], tv[sw, j]
    Au, Bu, Cu = tu.T.copy()
    Av, Bv, Cv = tv.T.copy()
    r = {"uA": Au.astype(np.int64), "uB": Bu.astype(np.int64), "uC": Cu.astype(np.int64),
         "vA": Av.astype(np.int64), "vB": Bv.astype(np.int64), "vC": Cv.astype(np.int64),
         "fA": Au, "fB": Bu}
    with np.errstate(divide="ignore", invalid="ignore"):
        r["ABa"] = np.where(r["uA"] != r["uB"], (Av - Bv) / (Au - Bu), f32(0)).astype(f32)
        r["ACa"] = np.where(r["uA"] != r["uC"], (Av - Cv) / (Au - Cu), f32(0)).astype(f32)
        r["BCa"] = np.where(r["uB"] != r["uC"], (Bv - Cv) / (Bu - Cu), f32(0)).astype(f32)
    r["ABb"] = Av - (r["ABa"] * Au).astype(f32)
    r["ACb"] = Av - (r["ACa"] * Au).astype(f32)
    r["BCb"] = Bv - (r["BCa"] * Bu).astype(f32)
    cr = (r["uB"] - r["uA"]) * (r["vC"] - r["vA"]) - (r["vB"] - r["vA"]) * (r["uC"] - r["uA"])
    r["sgn"] = np.sign(cr)
    return r


def analyse(pts, tris, w, h):
    """-> (flag conditions met: 1 M | 2 V | 4 B, contested pixels, those outside the corner set of their
    highest-index coverer)"""
    r = records(np.asarray(pts, np.int64), np.asarray(tris, np.int64).reshape(-1, 3))
    uA, uB, uC, sgn = r["uA"], r["uB"], r["uC"], r["sgn"]
    # conditions V and B, per triangle
    hasA = uA < uC
    near = lambda k, v: (k == v) | (k == v - 1)
    bad = hasA & ~near(line_at(r["ACa"], r["ACb"], r["fA"]), r["vA"])
    bad |= hasA & (uA < uB) & ~near(line_at(r["ABa"], r["ABb"], r["fA"]), r["vA"])
    hasB = hasA & (uB < uC)
    bad |= hasB & ~near(line_at(r["BCa"], r["BCb"], r["fB"]), r["vB"])
    kACb = line_at(r["ACa"], r["ACb"], r["fB"])
    wrong = np.where(sgn > 0, kACb < r["vB"], np.where(sgn < 0, kACb >= r["vB"], True))
    flagged = 2 * int(bad.any()) + 4 * int((hasB & (uA < uB) & wrong).any())
    # the walk: every column of [max(uA, 2), min(uC, w - 2)) of every triangle
    ulo, uhi = np.maximum(uA, 2), np.minimum(uC, w - 2)
    n = np.maximum(uhi - ulo, 0)
    T = np.repeat(np.arange(len(n)), n)
    if not len(T):
        return flagged, 0, 0
    u = ulo[T] + np.arange(len(T)) - np.repeat(np.cumsum(n) - n, n)
    second = u >= uB[T]
    v1 = line_at(r["ACa"][T], r["ACb"][T], u)
    v2 = line_at(np.where(second, r["BCa"][T], r["ABa"][T]), np.where(second, r["BCb"][T], r["ABb"][T]), u)
    s = sgn[T]
    flagged |= int(((u != uA[T]) & (((v1 < v2) & (s >= 0)) | ((v1 > v2) & (s <= 0)))).any())      # condition M
    va, vb = np.maximum(np.minimum(v1, v2), 0), np.minimum(np.maximum(v1, v2), h)
    keep = va < vb
    T, u, va, vb = T[keep], u[keep], va[keep], vb[keep]
    # columns in which two spans overlap: sorted by (u, va), a span starts below the highest end seen in its column
    o = np.lexsort((va, u))
    T, u, va, vb = T[o], u[o], va[o], vb[o]
    big = h + 2
    top = np.maximum.accumulate(u * big + vb)
    hit = np.zeros(len(u), bool)
    hit[1:] = (u[1:] == u[:-1]) & (u[1:] * big + va[1:] < top[:-1])
    contested = outside = 0
    for col in np.unique(u[hit]):
        lo, hi = np.searchsorted(u, col), np.searchsorted(u, col, "right")
        cT, ca, cb = T[lo:hi], va[lo:hi], vb[lo:hi]
        cnt = np.zeros(h + 1, np.int64)
        np.add.at(cnt, ca, 1)
        np.add.at(cnt, cb, -1)
        for v in np.nonzero(np.cumsum(cnt) > 1)[0]:
            cov = (ca <= v) & (v < cb)
            k = np.argmax(np.where(cov, cT, -1))
            X = cT[k]
            contested += 1
            if not ((col == uA[X] or col == uB[X]) and v in (ca[k], ca[k] + 1, cb[k] - 2, cb[k] - 1)):
                outside += 1
    return flagged, contested, outside


def delaunay(pts):
    from scipy.spatial import Delaunay
    pts = np.unique(np.asarray(pts, np.int64), axis=0)
    return pts, Delaunay(pts.astype(np.float64)).simplices


def lattice_mesh(rng, w, h):
    """support points as the product finds them: a step-5 lattice at 10-20 % density, with a disparity each"""
    uu, vv = np.meshgrid(np.arange(5, w - 5, 5), np.arange(5, h - 5, 5))
    take = rng.random(uu.shape) < rng.uniform(0.10, 0.20)
    u, v = uu[take], vv[take]
    d = rng.integers(0, 64, len(u))
    corners = np.array([[0, 0], [0, h - 1], [w - 1, 0], [w - 1, h - 1]])
    for side in (0, 1):
        yield np.concatenate([np.stack([u - side * d, v], 1), corners - [[side * 10, 0]]])


def adversarial_mesh(rng, kind, h=375):
    w = int(rng.choice([400, 1750, 4000, 9000]))
    base = np.stack([rng.integers(0, w, 12), rng.integers(0, h, 12)], 1)
    if kind == 0:       # sparse points: long thin triangles across the whole width
        return w, np.stack([rng.integers(0, w, 40), rng.integers(0, h, 40)], 1)
    if kind == 1:       # collinear points, seen from a far vertex
        n, du, dv = 30, int(rng.integers(1, 40)), int(rng.integers(-3, 4))
        k = np.arange(n)
        line = np.stack([w // 3 + du * k // 4, h // 2 + dv * k], 1)
        far = [[int(rng.integers(0, w)), int(rng.choice([0, h - 1]))]]
        return w, np.concatenate([line, far, base[:4]])
    if kind == 2:       # tall narrow strips: columns a few pixels apart, full height
        u0 = int(rng.integers(10, w - 20))
        cols = [np.stack([np.full(25, u0 + g), np.sort(rng.choice(h, 25, replace=False))], 1)
                for g in (0, int(rng.integers(1, 4)), int(rng.integers(4, 9)))]
        return w, np.concatenate(cols + [base[:5]])
    # vertices one row off a long edge
    x0, x1 = sorted(rng.choice(w, 2, replace=False))
    y0, y1 = rng.integers(0, h, 2)
    xs = np.unique(rng.integers(x0 + 1, max(x1, x0 + 2), 20))
    ys = np.round(y0 + (y1 - y0) * (xs - x0) / max(x1 - x0, 1)).astype(np.int64) + rng.choice([-1, 1], len(xs))
    return w, np.concatenate([[[x0, y0], [x1, y1]], np.stack([xs, np.clip(ys, 0, h - 1)], 1), base[:4]])


def in_image(pts, w, h):
    pts = np.asarray(pts, np.int64)
    return pts[(pts[:, 0] >= -70) & (pts[:, 0] < w) & (pts[:, 1] >= 0) & (pts[:, 1] < h)]


def test_contested_pixels_lie_in_the_corner_set():
    seen = {"golden": 0, "lattice": 0, "adversarial": 0}
    meshes = {"golden": 0, "lattice": 0, "adversarial": 0}
    for name in GOLDENS:
        z = np.load(os.path.join(H.GOLDEN, name + ".npz"))
        sup = z["support"].reshape(-1, 3).astype(np.int64)
        for side, key in ((0, "tri1"), (1, "tri2")):
            pts = np.stack([sup[:, 0] - side * sup[:, 2], sup[:, 1]], 1)
            flagged, contested, outside = analyse(pts, z[key], 1242, 375)
            assert not flagged, (name, side)
            assert outside == 0, (name, side, contested, outside)
            seen["golden"] += contested
            meshes["golden"] += 1
    pytest.importorskip("scipy")
    rng = np.random.default_rng(20240611)
    for k in range(30):
        w, h = (1242, 375) if k % 3 == 0 else (640, 240)
        for pts in lattice_mesh(rng, w, h):
            pts, tris = delaunay(pts)
            flagged, contested, outside = analyse(pts, tris, w, h)
            assert not flagged, ("lattice", k)          # as on the goldens: the product never leaves the corner form
            assert outside == 0, ("lattice", k, contested, outside)
            seen["lattice"] += contested
            meshes["lattice"] += 1
    unflagged = 0
    for k in range(240):
        w, pts = adversarial_mesh(rng, k % 4)
        pts, tris = delaunay(in_image(pts, w, 375))
        flagged, contested, outside = analyse(pts, tris, w, 375)
        meshes["adversarial"] += 1
        if flagged:
            continue
        unflagged += 1
        assert outside == 0, ("adversarial", k, contested, outside)
        seen["adversarial"] += contested
    print(meshes, seen, "adversarial unflagged:", unflagged)
    assert meshes["lattice"] >= 60 and unflagged >= 200
    assert sum(seen.values()) >= 800, seen          # the claim was not checked on nothing


def test_the_flag_catches_what_large_coordinates_break():
    """beyond |a * u| = 2^22 float32 moves lines off their own corners (V): such meshes are flagged, and a mesh with
    a multiply covered pixel outside the corner set must be flagged by some condition.  (The product sends such
    geometries to the exhaustive pass anyway: `wide` in launch_owner.)"""
    pytest.importorskip("scipy")
    rng = np.random.default_rng(7)
    inverted = broken = flags = 0
    for k in range(60):
        w, h = 60000, 3000
        spread, n = ((6, 80), (30, 40), (300, 60))[k % 3]      # steep edges far to the right, 1.5 to 16 rows per ulp
        pts, tris = delaunay(np.stack([w - 1200 + rng.integers(0, spread, n), rng.integers(0, h, n)], 1))
        flagged, contested, outside = analyse(pts, tris, w, h)
        flags += flagged != 0
        inverted += flagged & 1
        if outside:
            broken += 1
            assert flagged, (k, contested, outside)
    print("large-coordinate meshes: %d with inverted bounds, %d with pixels outside the corner set, %d flagged"
          % (inverted, broken, flags))
    assert flags > 0, "no condition fired: the test shows nothing"
