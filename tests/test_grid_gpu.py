"""GPU: the ground grid (svh_grid_*, include/svh_grid.h; csrc/grid_kernels.hip, csrc/grid_engine.cpp) against the numpy
restatement tests/grid_ref.py, which tests/test_grid.py pins on the CPU.  Every comparison is exact: the seven planes bit
for bit (NaN patterns included), the five statistics, the three renders.  Every accumulated quantity is an integer under
a commutative update, so the grid is the same whatever the schedule.

Shapes: k_grid_bin runs 256 points per workgroup, one lane per point, and is capped at 2048 workgroups, so 2048 * 256 + 1
points need a second pass of the first lane; runs of equal cell are combined by a scan within a wave of 64.  k_grid_finalise and
k_grid_render run 256 cells per workgroup."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_ref as R
import helpers as H
import test_grid as TG
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARG, HIP_ERR, UNSUPPORTED = -1, -2, -3
FULL_PASS = 2048 * 256


@pytest.fixture(scope="module")
def G():
    import svhip
    from svhip import grid
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    grid._bind()
    return grid


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def restore(G):
    yield
    G.lib().svh_test_fail_at(None)


def pair(G, **kw):
    """(the restatement's grid, the device's grid) with the same parameters"""
    P, Pc = TG.both(G, **kw)
    return R.Grid(P), G.Grid(Pc)


def planes_of(G, g):
    return dict(zip(R.PLANES, [g.plane(k) for k in range(7)]))


def check(G, g, ref, tag=""):
    """the device grid equals the restatement's: planes, statistics, the three renders"""
    got, want = planes_of(G, g), ref.planes()
    for k in R.PLANES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k].view(np.uint8 if got[k].itemsize == 1 else np.uint32) !=
                              want[k].view(np.uint8 if got[k].itemsize == 1 else np.uint32))
            raise AssertionError("%s: plane %s differs in %d cells, first (ib, ia) = %s: got %r, wanted %r" % (
                tag, k, len(bad), tuple(bad[0]), got[k][tuple(bad[0])], want[k][tuple(bad[0])]))
    assert g.stats().asdict() == ref.stats, (tag, g.stats(), ref.stats)
    for m in range(3):
        img = g.render(m)
        assert img.shape == (ref.P.nz, ref.P.nx, 3) and np.array_equal(img, ref.render(m)), (tag, "render", m)


def add_both(g, ref, pts):
    g.add_points(pts)
    ref.add(pts)


# ---- the hand cases ---------------------------------------------------------------------------------------------------
def test_hand_cases_and_the_worked_example_on_the_device(G):
    ref, g = pair(G, **TG.hand_kw())
    pts, fate, cell = TG.hand_points()
    add_both(g, ref, pts)
    assert ref.stats == {"added": len(pts), "binned": int((fate == 0).sum()), "overhead": int((fate == 1).sum()),
                         "outside": int((fate == 2).sum()), "unplaced": int((fate == 3).sum())}
    check(G, g, ref, "hand")
    ref, g = pair(G, **TG.hand_kw(cam=2.0))
    add_both(g, ref, TG.EXAMPLE)
    check(G, g, ref, "example")
    TG.example_checks(planes_of(G, g), g.stats().asdict(), g.render(G.RENDER_CLASS))


def test_minus_zero_and_the_hand_cells_on_the_device(G):
    T = R.frame_camera(0.0)
    T[2, 3] = -0.0
    ref, g = pair(G, **dict(TG.HAND_KW, T=T))
    add_both(g, ref, np.array([[-0.25, 0.0, -0.0, 0.0], [-0.25, 0.0, -0.0, 1.0]], F))
    check(G, g, ref, "-0.0")
    assert g.hmin()[0, 1].tobytes() == F(0).tobytes() and g.hmax()[0, 1].tobytes() == F(0).tobytes()
    # cells at the class thresholds, built from points: HMAX == step, one ulp above, HMIN == -drop, one ulp below
    ref, g = pair(G, **dict(TG.hand_kw(), nx=4, nz=1))
    hs = [(0.0, 0.25), (0.0, TG.NA(0.25, 1)), (-0.25, 0.0), (TG.NA(-0.25, -1), 0.0)]
    pts = np.array([[-0.9 + 0.5 * k, -h, 0.1, 0.5] for k, pr in enumerate(hs) for h in pr], F)
    add_both(g, ref, pts)
    check(G, g, ref, "thresholds")
    assert list(g.classes()[0]) == [R.FREE, R.OBSTACLE, R.FREE, R.DROP]


# ---- point counts around the launch shape ---------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, FULL_PASS + 1]
_clouds = {}


def cloud(n):
    if n not in _clouds:
        _clouds[n] = TG.seeded(n, 2000 + n % 991)
    return _clouds[n]


@pytest.mark.parametrize("n", COUNTS)
def test_counts(G, n):
    """around a wave, the workgroup, and one more point than a full pass of the capped launch; n = 0 launches nothing"""
    ref, g = pair(G)
    add_both(g, ref, cloud(n))
    check(G, g, ref, "%d points" % n)
    if n >= 255:
        assert ref.stats["binned"] > 0 and ref.stats["outside"] > 0


# ---- runs of equal cell in store order --------------------------------------------------------------------------------------
RUN_KW = dict(nx=16, nz=16, cell=0.5, x0=-4.0, z0=0.0, T=R.frame_camera(0.0), min_points=2, step=0.25, drop=0.25, clearance=2.0)


def at_cell(ia, ib, h, val, n=1):
    """n points in the middle of cell (ia, ib) of the RUN_KW window at height h (arrays broadcast)"""
    p = np.zeros((n, 4), F)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = -4.0 + 0.5 * ia + 0.25, -np.asarray(h, F), 0.5 * ib + 0.25, val
    return p


def alternating(n, k=0):
    """no runs at all: cells A B A B, heights and intensities moving"""
    i = np.arange(n)
    return at_cell(np.where(i % 2 == 0, 0, 15), np.where(i % 2 == 0, 0, 15), (i % 37) / 64.0 - 0.2, ((i + k) % 11) / 10.0, n)


def run_of(r, length, extreme):
    """a run of `length` points in one cell, all heights distinct (steps of 1/4096 from 1/4096), the highest at position
    `extreme` and the lowest (negative) right after it, cyclically"""
    h = (np.arange(length) + 1) / 4096.0
    hi = {"first": 0, "last": length - 1, "middle": length // 2}[extreme]
    h[[hi, length - 1]] = h[[length - 1, hi]]
    if length > 1:
        h[(hi + 1) % length] = -3.0 / 4096.0
    return at_cell(1 + r % 14, 1 + (r // 14) % 14, h, (np.arange(length) % 7) / 6.0, length)


def run_store():
    """runs of length 1, 2, 63, 64, 65 and 130 that start at lanes 0, 1 and 63 of a wave and at the last lane of a
    workgroup, the extreme height first, last and in the middle, separated by alternating cells"""
    parts, total, r = [], 0, 0
    for start in (0, 1, 63, 255):
        for length in (1, 2, 63, 64, 65, 130):
            for extreme in ("first", "last", "middle"):
                pad = (start - total) % 256
                if pad < 2:
                    pad += 256
                parts += [alternating(pad, r), run_of(r, length, extreme)]
                total += pad + length
                r += 1
    return np.concatenate(parts)


def test_runs_of_equal_cell(G):
    """a dropped, doubled or misattributed lane changes the count, hsum, HMIN or HMAX of a run's cell"""
    ref, g = pair(G, **RUN_KW)
    pts = run_store()
    cells = R.place(ref.P, pts)[1]
    assert (cells[1:] == cells[:-1]).sum() > 3000 and len(pts) > 8 * 256
    add_both(g, ref, pts)
    check(G, g, ref, "runs")
    # neighbouring runs of one cell with nothing between them are one run; and runs over a wave's and a workgroup's end
    ref, g = pair(G, **RUN_KW)
    pts = np.concatenate([run_of(3, 65, "last"), run_of(3, 130, "first"), run_of(4, 64, "middle"), run_of(4, 64, "first"),
                          run_of(5, 256, "last"), run_of(5, 2, "first")])
    add_both(g, ref, pts)
    check(G, g, ref, "abutting runs")


def test_no_runs_at_all(G):
    ref, g = pair(G, **RUN_KW)
    add_both(g, ref, alternating(1000))
    check(G, g, ref, "A B A B")
    assert g.count()[0, 0] == 500 and g.count()[15, 15] == 500


def test_overhead_and_bad_points_inside_runs(G):
    """every 5th point of a run is overhead in the same cell, every 7th NaN, every 11th outside, every 13th overhead in
    another cell: the low points around them are all counted, once"""
    ref, g = pair(G, **RUN_KW)
    pts = np.concatenate([run_of(r, 130, e) for r, e in enumerate(("first", "middle", "last", "middle"))])
    i = np.arange(len(pts))
    pts[i % 5 == 0, 1] = -2.5
    pts[i % 7 == 0, 0] = np.nan
    pts[i % 11 == 0, 2] = 100.0
    k = i % 13 == 0
    pts[k, 0], pts[k, 1] = 3.75, -2.5
    add_both(g, ref, pts)
    st = ref.stats
    assert st["overhead"] > 100 and st["unplaced"] > 50 and st["outside"] > 30 and st["binned"] > 250
    check(G, g, ref, "interleaved")


# ---- contention -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncells", [1, 2])
def test_contention(G, ncells):
    """4096 points in one cell, and over two cells in a random order: counts and both sums are exact"""
    rng = np.random.default_rng(7 + ncells)
    ref, g = pair(G, **RUN_KW)
    pts = at_cell(3 + rng.integers(0, ncells, 4096) * 5, 2, rng.uniform(-1.9, 1.9, 4096), rng.uniform(0, 1, 4096), 4096)
    add_both(g, ref, pts)
    check(G, g, ref, "contention %d" % ncells)
    cnt = g.count()
    assert cnt.sum() == 4096 and (cnt > 0).sum() == ncells and ref.hsum[2 * 16 + 3] != 0 and ref.vsum[2 * 16 + 3] > 100000


# ---- grid shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz", [(1, 1), (1, 257), (257, 1), (63, 65), (8192, 1)])
def test_grid_shapes(G, nx, nz):
    kw = dict(nx=nx, nz=nz, cell=0.25, x0=-0.125 * nx, z0=0.0)
    ref, g = pair(G, **kw)
    rng = np.random.default_rng(nx + nz)
    n = 6000
    pts = np.stack([rng.uniform(-0.13 * nx, 0.13 * nx, n), rng.uniform(-1.5, 2.2, n), rng.uniform(-0.02 * nz, 0.26 * nz, n),
                    rng.uniform(0, 1, n)], 1).astype(F)
    add_both(g, ref, pts)
    assert ref.stats["binned"] > 1000
    check(G, g, ref, "%d x %d" % (nx, nz))


def test_render_row_flip(G):
    """one marked cell per corner: the far row is row 0, left stays left"""
    ref, g = pair(G, **dict(TG.hand_kw(), nx=5, nz=3))
    corner = lambda ia, ib, h, val: [[-1.0 + 0.5 * ia + 0.1, -h, 0.5 * ib + 0.1, val]] * 2
    pts = np.array(corner(0, 0, 0.0, 1.0) + corner(4, 0, 1.0, 0.0) + corner(0, 2, -1.0, 0.0) + corner(4, 2, 0.1, 0.0), F)
    add_both(g, ref, pts)
    check(G, g, ref, "corners")
    img = g.render(G.RENDER_CLASS)
    assert tuple(img[2, 0]) == (0, 255, 0) and tuple(img[2, 4]) == (255, 0, 0)       # near left free (I 255), near right obstacle
    assert tuple(img[0, 0]) == (0, 0, 160) and tuple(img[0, 4]) == (0, 64, 0)        # far left drop, far right free (I 0)
    assert tuple(img[1, 2]) == (32, 32, 32)


# ---- the algebra on the device ------------------------------------------------------------------------------------------------
def test_order_independence_and_two_adds(G):
    pts = TG.seeded(30000, 31)
    ref, g = pair(G)
    add_both(g, ref, pts)
    check(G, g, ref, "whole")
    whole = planes_of(G, g)
    g2 = G.Grid(g.params)
    g2.add_points(pts[np.random.default_rng(1).permutation(len(pts))])
    assert R.same_planes(planes_of(G, g2), whole) and g2.stats().asdict() == ref.stats
    g3 = G.Grid(g.params)
    g3.add_points(pts[:12345])
    g3.add_points(pts[12345:])
    assert R.same_planes(planes_of(G, g3), whole) and g3.stats().asdict() == ref.stats
    assert np.array_equal(g3.render(G.RENDER_HEIGHT), g.render(G.RENDER_HEIGHT))


def test_clear_and_set_window(G):
    ref, g = pair(G)
    empty = R.Grid(ref.P)
    check(G, g, empty, "fresh")
    add_both(g, ref, TG.seeded(5000, 32))
    check(G, g, ref, "filled")
    g.clear()
    check(G, g, empty, "cleared")
    assert g.stats().asdict() == dict.fromkeys(ref.stats, 0)
    pts = TG.seeded(5000, 33)
    g.add_points(pts)
    check(G, g, R.Grid(ref.P).add(pts), "refilled")
    g.set_window(-10.0, 5.5)
    ref.set_window(-10.0, 5.5)
    check(G, g, ref, "moved window")
    add_both(g, ref, pts)
    check(G, g, ref, "moved window, filled")
    assert g._L.svh_grid_set_window(g._h, float("nan"), 0.0) == BAD_ARG and g._L.svh_grid_set_window(g._h, 0.0, float("inf")) == BAD_ARG
    check(G, g, ref, "after a refused window")


def test_device_pointers(G, hip):
    pts = TG.seeded(7000, 34)
    ref, g = pair(G, nx=100, nz=60)
    d = Dev(hip, pts)
    g.add_points_device(d.addr, len(pts))
    ref.add(pts)
    check(G, g, ref, "device input")
    want = ref.planes()
    for k, name in enumerate(R.PLANES):
        nbytes = want[name].nbytes
        out = Dev(hip, nbytes + 16)
        g.plane(k, device_ptr=out.addr)
        got = out.get()
        assert got[:nbytes].tobytes() == want[name].tobytes() and (got[nbytes:] == 0xEE).all(), name
    for m in range(3):
        out = Dev(hip, 100 * 60 * 3 + 16)
        g.render(m, device_ptr=out.addr)
        got = out.get()
        assert np.array_equal(got[:18000].reshape(60, 100, 3), ref.render(m)) and (got[18000:] == 0xEE).all()
    assert g._L.svh_grid_add_points(g._h, d.addr + 4, 10, 1) == BAD_ARG        # not 16-byte aligned
    check(G, g, ref, "after a refused pointer")


def test_bad_arguments_leave_the_object_unchanged(G):
    import svhip
    from svhip import view
    ref, g = pair(G, nx=40, nz=30)
    add_both(g, ref, TG.seeded(3000, 35))
    L, buf, pts = g._L, np.full(40 * 30 * 4, 0xAB, np.uint8), TG.seeded(4, 1)
    st = G.Stats(7, 7, 7, 7, 7)
    calls = [lambda: L.svh_grid_add_points(g._h, pts.ctypes.data, -1, 0), lambda: L.svh_grid_add_points(g._h, None, 3, 0),
             lambda: L.svh_grid_add_points(g._h, None, 3, 1), lambda: L.svh_grid_add_view(g._h, None),
             lambda: L.svh_grid_add_view(None, None), lambda: L.svh_grid_get_stats(g._h, None),
             lambda: L.svh_grid_get(g._h, 7, buf.ctypes.data, 0), lambda: L.svh_grid_get(g._h, -1, buf.ctypes.data, 0),
             lambda: L.svh_grid_get(g._h, 0, None, 0), lambda: L.svh_grid_render(g._h, 3, buf.ctypes.data, 0),
             lambda: L.svh_grid_render(g._h, -1, buf.ctypes.data, 0), lambda: L.svh_grid_render(g._h, 0, None, 0),
             lambda: L.svh_grid_get_stats(None, C.byref(st))]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG, k
        assert "svh_grid" in svhip.last_error()
    assert (buf == 0xAB).all() and st.asdict() == dict.fromkeys(ref.stats, 7)
    assert L.svh_grid_add_points(g._h, None, 0, 0) == 0                             # nothing to add is fine
    check(G, g, ref, "after the refused calls")
    for kw in TG.BAD_PARAMS[:6]:
        assert L.svh_grid_create(C.byref(G.default_params(**kw))) is None


def test_count_limit(G, hip):
    """more than 2^31 - 1 points since the last clear: SVH_ERR_UNSUPPORTED before anything is read"""
    ref, g = pair(G, nx=8, nz=8)
    add_both(g, ref, TG.seeded(100, 36))
    d = Dev(hip, 64)
    assert g._L.svh_grid_add_points(g._h, d.addr, 2 ** 31 - 100, 1) == UNSUPPORTED
    assert g._L.svh_grid_add_points(g._h, d.addr, 2 ** 40, 1) == UNSUPPORTED
    check(G, g, ref, "after the refused adds")


# ---- the view's store ---------------------------------------------------------------------------------------------------------
def test_add_view(G):
    from svhip import view
    lists = [TG.seeded(n, s) for n, s in ((3000, 41), (0, 42), (5000, 43), (700, 44))]
    v = view.View(64, 48)
    ref, g = pair(G)
    g.add_view(v)                                            # an empty view: SVH_OK, nothing changes
    check(G, g, ref, "empty view")
    assert g.stats().added == 0
    for a in lists:
        v.add_points([a])
    g.add_view(v)
    ref.add(v.points())
    assert ref.stats["added"] == 8700
    check(G, g, ref, "view")
    g2 = G.Grid(g.params)
    g2.add_points(v.points())
    assert R.same_planes(planes_of(G, g2), planes_of(G, g))
    st = v.thin(0.25)
    assert 0 < st.after < st.before
    g.clear()
    g.add_view(v)
    check(G, g, R.Grid(ref.P).add(v.points()), "thinned view")
    assert g.stats().added == st.after


def test_urban_map_end_to_end(G):
    """two golden urban crops through svh_map -> svh_view -> grid (640 x 240 crops, as the thinning's test cuts them),
    against the restatement applied to view.points()"""
    from svhip import mapper, view
    m = mapper.Mapper(721.5377, 609.5593, 172.854, 0.5371657, 20.0)
    v = view.View(64, 48)
    for k, name in enumerate(("urban2", "urban3")):
        z = np.load(os.path.join(H.GOLDEN, name + "_kitti.npz"))
        l, _ = H.golden_pair(str(z["crop"]))
        Ht = np.eye(4)
        Ht[2, 3] = 0.3 * k
        m.add(np.ascontiguousarray(z["d1"].reshape(l.shape)[60:300, 300:940]), np.ascontiguousarray(l[60:300, 300:940]), Ht, 0.0)
        v.add_map(m)
    pts = v.points()
    assert len(pts) > 2000
    ref, g = pair(G, nx=128, nz=128, cell=0.2, x0=-12.8)
    g.add_view(v)
    ref.add(pts)
    check(G, g, ref, "urban")
    st = ref.stats
    assert st["binned"] > 500 and ((ref.planes()["cls"] & 3) != 0).sum() > 10


def test_levelled_by_the_estimated_road_plane(G):
    """svh_plane -> svh_grid_frame_plane -> grid: the road plane found in urban2's D1 levels the grid of that frame's
    points; every row of T rounds, and the device still equals the restatement"""
    import plane_ref as PR
    import svhip
    D = PR.urban_d1("urban2_stereomapper")
    pl = svhip.PlaneEstimation()
    assert pl.estimate(D, seed=2) == PR.OK
    e, Hm = pl.plane_euclidean(), pl.transformation()
    T = G.frame_plane(e, Hm)
    norm = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    assert np.array_equal(T[2], [-(e[0] / norm), -(e[1] / norm), -(e[2] / norm), 1.0 / norm])
    assert np.array_equal(T[0, :3], Hm[:3, 0]) and np.array_equal(T[1, :3], Hm[:3, 2]) and T[0, 3] == 0 and T[1, 3] == 0
    assert 0.5 < T[2, 3] < 3.0 and abs(T[2, 1] + 1) < 0.1          # a car's camera: metres above the road, y nearly down
    f, cu, cv, base = PR.CALIB
    v, u = np.nonzero(D >= 1)
    d = D[v, u].astype(np.float64)
    pts = np.stack([(u - cu) * base / d, (v - cv) * base / d, f * base / d, (u % 256) / 255.0], 1).astype(F)
    kw = dict(nx=128, nz=256, cell=0.2, x0=-12.8, z0=0.0)
    ref, g = pair(G, T=T, **kw)
    add_both(g, ref, pts)
    check(G, g, ref, "levelled")
    assert ref.stats["binned"] > 10000
    flat, g2 = pair(G, T=R.frame_camera(T[2, 3]), **kw)
    add_both(g2, flat, pts)
    check(G, g2, flat, "level camera of the same height")
    assert not R.same_planes(ref.planes(), flat.planes())


# ---- failures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["launch:1", "copy:1", "wait:1"])
def test_a_failed_add_leaves_the_empty_grid(G, spec):
    """host-side injection at a guarded call: the add returns SVH_ERR_HIP, the grid is empty with zero statistics, and
    the same add repeated gives the grid of that add alone"""
    ref, g = pair(G, nx=50, nz=50)
    a, b = TG.seeded(4000, 51), TG.seeded(3000, 52)
    add_both(g, ref, a)
    check(G, g, ref, "before")
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.add_points(b)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    check(G, g, R.Grid(ref.P), spec + ": empty")
    g.add_points(b)
    check(G, g, R.Grid(ref.P).add(b), spec + ": the add repeated")


@pytest.mark.parametrize("spec", ["launch:1", "launch:2", "copy:1"])
def test_a_failed_render_leaves_the_grid(G, spec):
    ref, g = pair(G, nx=50, nz=50)
    add_both(g, ref, TG.seeded(4000, 53))
    img = np.full((50, 50, 3), 0xAB, np.uint8)
    G.lib().svh_test_fail_at(spec.encode())
    rc = g._L.svh_grid_render(g._h, G.RENDER_CLASS, img.ctypes.data, 0)
    G.lib().svh_test_fail_at(None)
    assert rc == HIP_ERR and (img == 0xAB).all()
    check(G, g, ref, spec)
    G.lib().svh_test_fail_at(b"launch:1")
    out = np.zeros((50, 50), F)
    rc = g._L.svh_grid_get(g._h, G.HMAX, out.ctypes.data, 0)
    G.lib().svh_test_fail_at(None)
    assert rc == 0              # the planes are finished already: a get launches nothing
    add_both(g, ref, TG.seeded(100, 54))
    G.lib().svh_test_fail_at(b"launch:1")
    rc = g._L.svh_grid_get(g._h, G.HMAX, out.ctypes.data, 0)
    G.lib().svh_test_fail_at(None)
    assert rc == HIP_ERR
    check(G, g, ref, spec + ", then a failed get")


# ---- the pipeline tool -----------------------------------------------------------------------------------------------------------
def read_ppm(path):
    raw = open(path, "rb").read()
    magic, size, mx, body = raw.split(b"\n", 3)
    w, h = (int(t) for t in size.split())
    assert magic == b"P6" and mx == b"255" and len(body) == 3 * w * h
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)


def test_pipeline_grid(G, tmp_path, monkeypatch, capsys):
    """--grid DIR: one PPM of the grid's size per frame, the grid rebuilt from the view's store; it is the restatement's
    render of view.points() at the end.  --level: the road plane of the first frame's D1 levels the grid (the images
    differ), or the fallback note is printed"""
    import sys
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify
    from svhip import kitti
    from test_view_gpu import two_frame_drive
    drive = str(two_frame_drive(tmp_path / "drive"))
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(test_rectify.rig_calib_text())
    plain = None
    imgs = {}
    for tag, extra in (("none", []), ("grid", ["--grid", str(tmp_path / "g0"), "--grid-cell", "0.25", "--grid-size", "96x160"]),
                       ("level", ["--grid", str(tmp_path / "g1"), "--grid-cell", "0.25", "--grid-size", "96x160", "--level"])):
        monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py"] + extra + [drive, str(calib)])
        SP.main()
        out = capsys.readouterr().out.splitlines()
        frames = [l for l in out if l.startswith("frame ")]
        plain = plain or frames
        assert frames == plain and len(frames) == 2                 # the per-frame lines do not change
        if not extra:
            assert not any("grid" in l for l in out)
            continue
        d = extra[1]
        assert sorted(os.listdir(d)) == ["grid_%06d.ppm" % k for k in range(2)]
        imgs[tag] = [read_ppm(os.path.join(d, "grid_%06d.ppm" % k)) for k in range(2)]
        assert all(i.shape == (160, 96, 3) for i in imgs[tag])
        assert any(l.startswith("grid 96 x 160 cells of 0.25") for l in out)
        if tag == "level":
            fell_back = any("falls back to frame_camera(1.65)" in l for l in out)
            assert fell_back or any(not np.array_equal(a, b) for a, b in zip(imgs["grid"], imgs["level"]))
            assert fell_back or any(l.startswith("grid levelled by the road plane") for l in out)
    # the unlevelled grid of the last frame is the restatement's grid of the store at the end
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
    ref = R.Grid(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0)).add(p.view.points())
    assert np.array_equal(imgs["grid"][1], ref.render(R.M_CLASS)) and ref.stats["binned"] > 1000
