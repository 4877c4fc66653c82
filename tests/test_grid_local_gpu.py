"""GPU: the ground grid as a local map (include/svh_grid.h: svh_grid_scroll / follow, svh_grid_add_*_from, svh_grid_get_local,
svh_grid_render_local; csrc/grid_kernels.hip, csrc/grid_engine.cpp) against the numpy restatement tests/grid_local_ref.py,
which tests/test_grid_local.py pins on the CPU.  Every comparison is exact: the seven planes of svh_grid_get bit for bit,
the two local planes, the point and the ray statistics, the window, the three renders and the local one.

Shapes: k_grid_rays casts 64 end cells of one row (forward-major lines) or of one column (lateral-major lines) per wave,
four waves per workgroup; k_grid_enter and k_grid_finalise run 256 cells per workgroup.  The windows 1 x 1, 1 x 9, 9 x 1,
3 x 3, 64 x 1, 65 x 65 and 257 x 129 put lane, wave and workgroup edges on rows, on columns and on both."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_local_ref as LR
import grid_ref as R
import helpers as H
import test_grid as TG
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARG, HIP_ERR = -1, -2
FULL_PASS = 2048 * 256
WINDOWS = [(1, 1), (1, 9), (9, 1), (3, 3), (64, 1), (65, 65), (257, 129)]
CELL = 0.5


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


def win_kw(nx, nz, **kw):
    """cells of 0.5 from (0, 0), a camera on the road (a = x, b = z, h = -y): cell centres are exact in fp32"""
    return dict(dict(nx=nx, nz=nz, cell=CELL, x0=0.0, z0=0.0, T=R.frame_camera(0.0), min_points=2, step=0.25, drop=0.25,
                     clearance=2.0), **kw)


def pair(G, **kw):
    P, Pc = TG.both(G, **kw)
    return LR.Grid(P), G.Grid(Pc)


def snapshot(G, g):
    """everything the object can be asked for"""
    out = {k: g.plane(i) for i, k in enumerate(R.PLANES)}
    out["passed"], out["state"] = g.local_plane(G.LOCAL_PASS), g.local_plane(G.LOCAL_STATE)
    for m in range(3):
        out["render%d" % m] = g.render(m)
    out["local"] = g.render_local()
    out["stats"], out["rays"], out["window"] = g.stats().asdict(), g.ray_stats(), g.window()
    return out


def expected(ref):
    out = ref.planes()
    out.update(ref.local_planes())
    for m in range(3):
        out["render%d" % m] = ref.render(m)
    out["local"] = ref.render_local()
    out["stats"], out["rays"], out["window"] = dict(ref.stats), (ref.rays, ref.ray_cells), ref.window()
    return out


def check(G, g, ref, tag=""):
    got, want = snapshot(G, g), expected(ref)
    assert got["window"] == want["window"], (tag, got["window"], want["window"])
    assert got["stats"] == want["stats"], (tag, got["stats"], want["stats"])
    for k, w in want.items():
        if not isinstance(w, np.ndarray):
            continue
        a = got[k]
        assert a.dtype == w.dtype and a.shape == w.shape, (tag, k)
        if a.tobytes() != w.tobytes():
            view = np.uint8 if a.itemsize == 1 else np.uint32
            bad = np.argwhere(a.view(view) != w.view(view))
            raise AssertionError("%s: %s differs in %d places, first %s: got %r, wanted %r" % (
                tag, k, len(bad), tuple(bad[0]), a[tuple(bad[0])], w[tuple(bad[0])]))
    assert got["rays"] == want["rays"], (tag, got["rays"], want["rays"])
    return got


def same(a, b):
    return all((a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a) and a.keys() == b.keys()


def centre(ref, ia, ib, h=0.0):
    """the map-frame position in the middle of window cell (ia, ib) at height h, in double"""
    return [(ref.oa + ia + 0.5) * CELL, -h, (ref.ob + ib + 0.5) * CELL]


def at_cells(ref, ia, ib, h=0.0, val=0.5):
    """one point in the middle of each window cell (ia, ib) (arrays broadcast)"""
    ia, ib, h, val = np.broadcast_arrays(np.asarray(ia), np.asarray(ib), np.asarray(h, np.float64), np.asarray(val, np.float64))
    p = np.zeros((ia.size, 4), F)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = (ref.oa + ia.ravel() + 0.5) * CELL, -h.ravel(), (ref.ob + ib.ravel() + 0.5) * CELL, val.ravel()
    return p


def every_cell(ref, times=1):
    nx, nz = ref.P.nx, ref.P.nz
    ia, ib = np.meshgrid(np.arange(nx), np.arange(nz))
    i = np.tile(np.arange(nx * nz), times)
    return at_cells(ref, np.tile(ia.ravel(), times), np.tile(ib.ravel(), times), (i % 23) / 16.0 - 0.5, (i % 11) / 10.0)


def origins(nx, nz):
    """the four corners, an edge, the middle, as window cells"""
    seen = []
    for o in ((0, 0), (nx - 1, 0), (0, nz - 1), (nx - 1, nz - 1), (nx // 2, 0), (0, nz // 2), (nx // 2, nz // 2)):
        if o not in seen:
            seen.append(o)
    return seen


def cloud(ref, rng, n):
    """random points over the window as it stands and two cells around it: low, overhead, outside, and a few that are
    no points at all"""
    P = ref.P
    p = np.stack([rng.uniform((ref.oa - 2) * CELL, (ref.oa + P.nx + 2) * CELL, n), rng.uniform(-2.6, 1.0, n),
                  rng.uniform((ref.ob - 2) * CELL, (ref.ob + P.nz + 2) * CELL, n), rng.uniform(-0.1, 1.1, n)], 1).astype(F)
    if n >= 16:
        k = rng.choice(n, n // 16, replace=False)
        p[k, rng.integers(0, 4, len(k))] = rng.choice(np.array([np.nan, np.inf, -3e38, -0.0], F), len(k))
    return p


def from_both(g, ref, pts, origin):
    g.add_points_from(pts, origin)
    ref.add_from(pts, origin)


# ---- rays: every cell of the window once, from every kind of origin ---------------------------------------------------------
@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_every_cell_once_from_each_origin(G, nx, nz):
    """all octants and all lengths the window has; the origin's own cell casts nothing"""
    ref, g = pair(G, **win_kw(nx, nz))
    pts = every_cell(ref)
    for ia, ib in origins(nx, nz):
        g.clear()
        ref.clear()
        from_both(g, ref, pts, centre(ref, ia, ib, h=1.0))
        got = check(G, g, ref, "%d x %d from (%d, %d)" % (nx, nz, ia, ib))
        assert got["rays"][0] == nx * nz and got["passed"][ib, ia] == nx * nz - 1
        assert got["passed"].sum() == got["rays"][1] == ref.ray_cells
    # the origins one after the other without a clear: the rays of all of them, the points seven times
    g.clear()
    ref.clear()
    for ia, ib in origins(nx, nz):
        from_both(g, ref, pts, centre(ref, ia, ib))
    check(G, g, ref, "%d x %d, all origins accumulated" % (nx, nz))


def test_weights(G):
    """2049 points in one cell are one ray of weight 2049; twice every cell is weight 2 everywhere"""
    ref, g = pair(G, **win_kw(65, 65))
    pts = at_cells(ref, np.full(2049, 64), np.full(2049, 3), (np.arange(2049) % 31) / 32.0, 0.25)
    from_both(g, ref, pts, centre(ref, 32, 32))
    got = check(G, g, ref, "2049 in one cell")
    assert got["rays"] == (2049, 2049 * 32) and got["passed"][32, 32] == 2049 and got["passed"].max() == 2049
    from_both(g, ref, every_cell(ref, 2), centre(ref, 0, 64))
    check(G, g, ref, "every cell twice on top")


COUNTS = [0, 1, 63, 64, 65, 257, FULL_PASS + 1]


@pytest.mark.parametrize("n", COUNTS)
def test_counts(G, n):
    """the bin kernel's launch shape with the end counts switched on: a wave, a workgroup, one point more than a full
    pass of the capped launch.  The default window, the existing seeded clouds, the camera 1.65 m above the road"""
    ref, g = pair(G)
    pts = TG.seeded(n, 2000 + n % 991)
    from_both(g, ref, pts, [0.0, 0.0, 0.1])
    got = check(G, g, ref, "%d points" % n)
    assert got["rays"][0] == ref.stats["binned"] and (n < 257 or got["rays"][1] > got["rays"][0])


def test_points_that_cast_nothing(G):
    """overhead, outside and unplaced points cast no ray and leave no end count behind: the next call's rays are its own"""
    ref, g = pair(G, **win_kw(65, 65))
    n = 3000
    pts = at_cells(ref, np.arange(n) % 65, (np.arange(n) // 65) % 65, 2.5, 0.5)      # all overhead
    pts[::3, 0] = -7.0                                                               # outside
    pts[1::3, 2] = np.nan                                                            # unplaced
    from_both(g, ref, pts, centre(ref, 5, 60))
    got = check(G, g, ref, "no low point")
    assert got["rays"] == (0, 0) and got["passed"].sum() == 0 and got["stats"]["overhead"] == 1000
    from_both(g, ref, at_cells(ref, [64, 0], [64, 0]), centre(ref, 32, 32))
    got = check(G, g, ref, "then two rays")
    assert got["rays"] == (2, 64) and got["passed"].sum() == 64


def test_two_origins_order_and_plain_adds_between(G):
    rng = np.random.default_rng(5)
    ref, g = pair(G, **win_kw(65, 65))
    a, b, c = cloud(ref, rng, 9000), cloud(ref, rng, 7000), cloud(ref, rng, 500)
    oa, ob = centre(ref, 3, 61, h=2.0), centre(ref, 64, 0, h=-1.0)
    from_both(g, ref, a, oa)
    g.add_points(c)                                              # a plain add casts nothing
    ref.add(c)
    from_both(g, ref, b, ob)
    whole = check(G, g, ref, "two origins")
    assert whole["rays"][0] == whole["stats"]["binned"] - int((R.place(ref.P, c)[0] == R.LOW).sum()) > 5000
    # the same multisets in another order of points and of calls: identical bytes
    g2 = G.Grid(g.params)
    g2.add_points_from(b[rng.permutation(len(b))], ob)
    g2.add_points_from(a[rng.permutation(len(a))], oa)
    g2.add_points(c[::-1])
    assert same(snapshot(G, g2), whole)
    # and in pieces
    g3 = G.Grid(g.params)
    for part in np.array_split(a, 7):
        g3.add_points_from(part, oa)
    g3.add_points(c)
    g3.add_points_from(b[:1], ob)
    g3.add_points_from(b[1:], ob)
    assert same(snapshot(G, g3), whole)


# ---- the scroll -------------------------------------------------------------------------------------------------------------
def steps(n):
    return [0, 1, -1, n - 1, -(n - 1), n, -n, n + 1, -(n + 1)]


@pytest.mark.parametrize("nx,nz", [(9, 5), (65, 65)])
def test_scroll_keeps_what_stays(G, nx, nz):
    """every pair of steps: nothing, one cell, all but one column, exactly the window, more than the window"""
    rng = np.random.default_rng(nx)
    ref, g = pair(G, **win_kw(nx, nz))
    pts = np.concatenate([every_cell(ref), cloud(ref, rng, 2000)])
    o = centre(ref, nx // 2, nz // 2)
    base = LR.Grid(ref.P).add_from(pts, o)
    for da in steps(nx):
        for db in steps(nz):
            g.set_window(0.0, 0.0)
            g.add_points_from(pts, o)
            g.scroll(da, db)
            ref = LR.Grid(base.P)
            for k, v in vars(base).items():
                setattr(ref, k, v.copy() if isinstance(v, (np.ndarray, dict)) else v)
            ref.scroll(da, db)
            got = check(G, g, ref, "scroll (%d, %d)" % (da, db))
            kept = abs(da) < nx and abs(db) < nz
            assert (got["count"].sum() > 0) == kept and got["stats"]["binned"] == base.stats["binned"]
    # and the window goes on working where it stands
    more = cloud(ref, rng, 3000)
    from_both(g, ref, more, centre(ref, 0, nz - 1))
    check(G, g, ref, "after the last scroll, an add")


def test_twenty_scrolls_around_the_torus(G):
    """steps that sum to several windows in both directions, with adds and rays between them"""
    rng = np.random.default_rng(20)
    nx, nz = 65, 33
    ref, g = pair(G, **win_kw(nx, nz))
    moves = [(7, 3), (31, -5), (40, 16), (-3, 20), (64, 0), (0, 32), (13, 13), (50, -31), (-64, 9), (29, 29),
             (1, -1), (33, 17), (60, 30), (-20, 11), (45, 2), (5, 31), (64, 32), (-1, -32), (37, 8), (-200, 90)]
    assert sum(m[0] for m in moves[:-1]) > 4 * nx and sum(m[1] for m in moves[:-1]) > 4 * nz
    for k, (da, db) in enumerate(moves):
        pts = cloud(ref, rng, 1500)
        if k % 3 == 2:
            g.add_points(pts)
            ref.add(pts)
        else:
            from_both(g, ref, pts, centre(ref, int(rng.integers(0, nx)), int(rng.integers(0, nz)), h=float(rng.uniform(-1, 2))))
        g.scroll(da, db)
        ref.scroll(da, db)
        check(G, g, ref, "move %d by (%d, %d)" % (k, da, db))
    assert ref.window() == (sum(m[0] for m in moves), sum(m[1] for m in moves)) and ref.stats["added"] == 30000


def test_scroll_at_the_offset_limits_and_follow(G):
    rng = np.random.default_rng(21)
    ref, g = pair(G, **win_kw(64, 1))
    Lm = LR.OFFSET_LIMIT
    from_both(g, ref, every_cell(ref), centre(ref, 63, 0))
    g.scroll(Lm, -Lm)                                            # one step to the corner of the range: the grid is empty
    ref.scroll(Lm, -Lm)
    check(G, g, ref, "at the limit")
    from_both(g, ref, every_cell(ref), centre(ref, 0, 0))
    check(G, g, ref, "an add at the limit")
    before = snapshot(G, g)
    assert g._L.svh_grid_scroll(g._h, 1, 0) == BAD_ARG and g._L.svh_grid_scroll(g._h, 0, -1) == BAD_ARG
    assert g._L.svh_grid_scroll(g._h, 2 ** 31 - 1, 0) == BAD_ARG and g._L.svh_grid_scroll(g._h, -2 * Lm - 1, 0) == BAD_ARG
    assert same(snapshot(G, g), before)
    g.scroll(-2 * Lm, 2 * Lm)
    ref.scroll(-2 * Lm, 2 * Lm)
    check(G, g, ref, "at the other limit")
    # follow: the cell of the position becomes window cell (ia, ib)
    ref, g = pair(G, **win_kw(65, 65))
    from_both(g, ref, cloud(ref, rng, 4000), centre(ref, 32, 0))
    for pos, ia, ib in (([20.3, 0.0, 11.9], 32, 32), ([20.3, 0.0, 11.9], 32, 32), ([21.1, 5.0, 12.6], 32, 32), ([-300.2, 0.0, 77.7], 0, 64)):
        g.follow(pos, ia, ib)
        ref.follow(pos, ia, ib)
        ga, gb = g.cell_of(pos)
        assert (ga, gb) == LR.cell_of(ref.P, pos) and g.window() == (ga - ia, gb - ib)
        from_both(g, ref, cloud(ref, rng, 1000), centre(ref, ia, ib))
        check(G, g, ref, "follow %r" % (pos,))
    before = snapshot(G, g)
    xyz, cell = np.array([np.nan, 0, 0]), np.full(2, -7, np.int32)
    assert g._L.svh_grid_follow(g._h, xyz.ctypes.data, 0, 0) == BAD_ARG and g._L.svh_grid_cell_of(g._h, xyz.ctypes.data, cell.ctypes.data) == BAD_ARG
    xyz[0] = 1e9                                                 # finite, but no cell below 2^20
    assert g._L.svh_grid_follow(g._h, xyz.ctypes.data, 0, 0) == BAD_ARG and g._L.svh_grid_cell_of(g._h, xyz.ctypes.data, cell.ctypes.data) == BAD_ARG
    xyz[0] = 524200.0                                            # a cell, but offsets beyond the range
    assert g._L.svh_grid_cell_of(g._h, xyz.ctypes.data, cell.ctypes.data) == 0 and tuple(cell) == (1048400, 0)
    assert g._L.svh_grid_follow(g._h, xyz.ctypes.data, 0, 0) == BAD_ARG
    xyz[0] = 1.0
    assert g._L.svh_grid_follow(g._h, xyz.ctypes.data, 65, 0) == BAD_ARG and g._L.svh_grid_follow(g._h, xyz.ctypes.data, 0, -1) == BAD_ARG
    assert g._L.svh_grid_follow(g._h, None, 0, 0) == BAD_ARG and g._L.svh_grid_cell_of(g._h, xyz.ctypes.data, None) == BAD_ARG
    assert same(snapshot(G, g), before)


def test_clear_and_set_window(G):
    """clear empties the grid where it stands; set_window also puts the offsets back to zero"""
    rng = np.random.default_rng(22)
    ref, g = pair(G, **win_kw(65, 65))
    g.scroll(5, -9)
    ref.scroll(5, -9)                                            # on the empty grid: the offsets alone
    check(G, g, ref, "scrolled while empty")
    from_both(g, ref, cloud(ref, rng, 5000), centre(ref, 10, 10))
    check(G, g, ref, "filled")
    g.clear()
    ref.clear()
    got = check(G, g, ref, "cleared")
    assert got["window"] == (5, -9) and got["passed"].sum() == 0 and got["rays"] == (0, 0) and got["stats"]["added"] == 0
    from_both(g, ref, cloud(ref, rng, 5000), centre(ref, 10, 10))
    g.set_window(-3.0, 4.5)
    ref.set_window(-3.0, 4.5)
    got = check(G, g, ref, "set_window")
    assert got["window"] == (0, 0) and got["passed"].sum() == 0 and got["count"].sum() == 0 and got["rays"] == (0, 0)
    pts = cloud(ref, rng, 5000) + np.array([-3.0, 0, 4.5, 0], F)
    from_both(g, ref, pts, [-3.0 + 1.25, 0.0, 4.5 + 1.25])
    got = check(G, g, ref, "the moved window, filled")
    assert got["rays"][0] > 1000


@pytest.mark.parametrize("k", range(len(TG.CASES)))
def test_a_grid_that_never_scrolls_or_casts_is_the_old_grid(G, k):
    """the existing restatement grid_ref.Grid on the existing seeded clouds, through the existing entries alone; the new
    planes stay zero"""
    import test_grid_gpu as TGG
    P, Pc = TG.both(G, **TG.case_kw(k, G))
    ref, g = R.Grid(P), G.Grid(Pc)
    for n, seed in ((5000, 3), (40000, 4)):
        pts = TG.seeded(n, seed + 10 * k)
        g.add_points(pts)
        ref.add(pts)
    TGG.check(G, g, ref, "case %d" % k)
    assert g.window() == (0, 0) and g.ray_stats() == (0, 0) and not g.local_plane(G.LOCAL_PASS).any()
    assert np.array_equal(g.local_plane(G.LOCAL_STATE), ref.planes()["cls"]) and np.array_equal(g.render_local(), ref.render(R.M_CLASS))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte(G, hip):
    from svhip import view
    rng = np.random.default_rng(23)
    ref, g = pair(G, **win_kw(65, 33))
    g.scroll(-4, 6)
    ref.scroll(-4, 6)
    from_both(g, ref, cloud(ref, rng, 6000), centre(ref, 30, 2))
    before = check(G, g, ref, "before")
    L, pts = g._L, every_cell(ref)
    d = Dev(hip, pts)
    v = view.View(64, 48)
    v.add_points([pts[:100]])
    v.add_points([pts[100:300]])
    ok = np.array(centre(ref, 1, 1))
    buf = np.full(65 * 33 * 4, 0xAB, np.uint8)
    out = np.full(2, -7, np.int64)
    bad_origins = [centre(ref, -1, 5), centre(ref, 5, 33), centre(ref, 65, 0),          # outside the window
                   centre(ref, 5, 5, h=2.5), centre(ref, 5, 5, h=np.nextafter(F(2), F(3))),   # above the clearance
                   [np.nan, 0, 1], [1, np.inf, 1], [1, 0, -np.inf], [1e300, 0, 1], [1, -2e6, 1]]   # not finite; |h| >= 2^20
    for o in bad_origins:
        o = np.array(o, np.float64)
        assert L.svh_grid_add_points_from(g._h, pts.ctypes.data, len(pts), 0, o.ctypes.data) == BAD_ARG, o
        assert L.svh_grid_add_points_from(g._h, None, 0, 0, o.ctypes.data) == BAD_ARG, o      # also with nothing to add
        assert L.svh_grid_add_view_lists_from(g._h, v._h, 0, 2, o.ctypes.data) == BAD_ARG, o
    calls = [lambda: L.svh_grid_add_points_from(g._h, d.addr + 4, 10, 1, ok.ctypes.data),     # not 16-byte aligned
             lambda: L.svh_grid_add_points_from(g._h, pts.ctypes.data, -1, 0, ok.ctypes.data),
             lambda: L.svh_grid_add_points_from(g._h, None, 3, 0, ok.ctypes.data),
             lambda: L.svh_grid_add_points_from(g._h, pts.ctypes.data, 3, 0, None),
             lambda: L.svh_grid_add_view_lists_from(g._h, v._h, 0, 3, ok.ctypes.data),         # a range past the view's lists
             lambda: L.svh_grid_add_view_lists_from(g._h, v._h, 2, 1, ok.ctypes.data),
             lambda: L.svh_grid_add_view_lists_from(g._h, v._h, -1, 1, ok.ctypes.data),
             lambda: L.svh_grid_add_view_lists_from(g._h, v._h, 0, -1, ok.ctypes.data),
             lambda: L.svh_grid_add_view_lists_from(g._h, v._h, 2 ** 31 - 1, 2 ** 31 - 1, ok.ctypes.data),
             lambda: L.svh_grid_add_view_lists_from(g._h, None, 0, 1, ok.ctypes.data),
             lambda: L.svh_grid_add_view_lists_from(g._h, v._h, 0, 1, None),
             lambda: L.svh_grid_scroll(g._h, LR.OFFSET_LIMIT + 5, 0),                          # from (-4, 6): one beyond the range
             lambda: L.svh_grid_scroll(g._h, 0, -LR.OFFSET_LIMIT - 7), lambda: L.svh_grid_scroll(g._h, 1, 2 ** 31 - 1),
             lambda: L.svh_grid_get_local(g._h, 2, buf.ctypes.data, 0), lambda: L.svh_grid_get_local(g._h, -1, buf.ctypes.data, 0),
             lambda: L.svh_grid_get_local(g._h, 0, None, 0), lambda: L.svh_grid_render_local(g._h, None, 0),
             lambda: L.svh_grid_get(g._h, 7, buf.ctypes.data, 0), lambda: L.svh_grid_render(g._h, 3, buf.ctypes.data, 0),
             lambda: L.svh_grid_get_ray_stats(g._h, None), lambda: L.svh_grid_get_window(g._h, None)]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG, k
        assert "svh_grid" in G.last_error()
    assert (buf == 0xAB).all() and (out == -7).all()
    assert same(snapshot(G, g), before)
    # what is allowed: an empty range, nothing to add
    assert L.svh_grid_add_view_lists_from(g._h, v._h, 2, 0, ok.ctypes.data) == 0
    assert L.svh_grid_add_points_from(g._h, None, 0, 1, ok.ctypes.data) == 0 and L.svh_grid_scroll(g._h, 0, 0) == 0
    assert same(snapshot(G, g), before)


# ---- failures --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["launch:1", "launch:2", "copy:1", "wait:1"])
def test_a_failed_add_from_leaves_the_empty_grid(G, spec):
    """launch:1 is the binning, launch:2 the rays: SVH_ERR_HIP, the grid is empty where it stands, the statistics are
    zero, and the same call repeated gives the grid of that call alone -- no end count is left over"""
    rng = np.random.default_rng(24)
    ref, g = pair(G, **win_kw(65, 65))
    g.scroll(3, 3)
    ref.scroll(3, 3)
    a, b = cloud(ref, rng, 4000), cloud(ref, rng, 3000)
    o = centre(ref, 7, 60)
    from_both(g, ref, a, o)
    check(G, g, ref, "before")
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.add_points_from(b, o)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    ref.clear()
    got = check(G, g, ref, spec + ": empty")
    assert got["window"] == (3, 3) and got["rays"] == (0, 0)
    from_both(g, ref, b, o)
    check(G, g, ref, spec + ": the add repeated")


@pytest.mark.parametrize("spec", ["launch:1", "wait:1"])
@pytest.mark.parametrize("step", [(2, -1), (70, 0)])
def test_a_failed_scroll_leaves_the_empty_grid(G, spec, step):
    """the strips' kernel, or the fills of a scroll beyond the window (copy:1 there), fails: the grid is empty at the new
    offsets"""
    rng = np.random.default_rng(25)
    ref, g = pair(G, **win_kw(65, 65))
    from_both(g, ref, cloud(ref, rng, 4000), centre(ref, 7, 60))
    check(G, g, ref, "before")
    if step[0] >= 65 and spec == "launch:1":
        spec = "copy:1"
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.scroll(*step)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    ref.clear()
    ref.scroll(*step)
    got = check(G, g, ref, spec + ": empty")
    assert got["window"] == step and got["stats"]["added"] == 0
    from_both(g, ref, cloud(ref, rng, 2000), centre(ref, 1, 1))
    check(G, g, ref, spec + ": the next add")


# ---- device pointers, the view's lists ----------------------------------------------------------------------------------------------
def test_device_pointers(G, hip):
    rng = np.random.default_rng(26)
    ref, g = pair(G, **win_kw(100, 60))
    pts = cloud(ref, rng, 7000)
    d = Dev(hip, pts)
    o = centre(ref, 50, 0)
    g.add_points_device_from(d.addr, len(pts), o)
    ref.add_from(pts, o)
    check(G, g, ref, "device input")
    want = ref.local_planes()
    for k, name in ((G.LOCAL_PASS, "passed"), (G.LOCAL_STATE, "state")):
        nbytes = want[name].nbytes
        out = Dev(hip, nbytes + 16)
        g.local_plane(k, device_ptr=out.addr)
        got = out.get()
        assert got[:nbytes].tobytes() == want[name].tobytes() and (got[nbytes:] == 0xEE).all(), name
    out = Dev(hip, 100 * 60 * 3 + 16)
    g.render_local(device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:18000].reshape(60, 100, 3), ref.render_local()) and (got[18000:] == 0xEE).all()
    assert d.get(pts.nbytes).tobytes() == pts.tobytes()           # the input is only read


def test_add_view_lists_from(G):
    from svhip import view
    rng = np.random.default_rng(27)
    ref, g = pair(G, **win_kw(65, 65))
    lists = [cloud(ref, rng, n) for n in (3000, 0, 5000, 700)]
    v = view.View(64, 48)
    for a in lists:
        v.add_points([a])
    o1, o2 = centre(ref, 0, 0), centre(ref, 64, 30)
    g.add_view_lists_from(v, 3, 1, o1)                           # the newest list
    ref.add_from(lists[3], o1)
    check(G, g, ref, "the last list")
    g.add_view_lists_from(v, 1, 1, o1)                           # an empty list: nothing changes
    check(G, g, ref, "an empty list")
    g.add_view_lists_from(v, 0, 3, o2)                           # a range, not starting at the store's beginning + not ending at its end
    ref.add_from(np.concatenate(lists[:3]), o2)
    check(G, g, ref, "lists 0..2")
    g.add_view_lists_from(v, 2, 2, o1)
    ref.add_from(np.concatenate(lists[2:]), o1)
    got = check(G, g, ref, "lists 2..3")
    assert got["stats"]["added"] == 700 + (3000 + 0 + 5000) + (5000 + 700)


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------------------
def test_pipeline_grid_local(G, tmp_path, monkeypatch, capsys):
    """--grid-local DIR on the two golden frames: per frame the window follows the camera, the newest list is added with
    rays from the camera centre, and the image is the restatement's after the same steps"""
    import sys
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify
    from svhip import kitti, view
    from test_grid_gpu import read_ppm
    from test_view_gpu import two_frame_drive
    drive = str(two_frame_drive(tmp_path / "drive"))
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(test_rectify.rig_calib_text())
    d = str(tmp_path / "loc")
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cell", "0.25", "--grid-size", "96x160",
                                      drive, str(calib)])
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert len([l for l in out if l.startswith("frame ")]) == 2
    assert any(l.startswith("local grid 96 x 160 cells of 0.25") for l in out)
    assert sorted(os.listdir(d)) == ["local_%06d.ppm" % k for k in range(2)]
    imgs = [read_ppm(os.path.join(d, "local_%06d.ppm" % k)) for k in range(2)]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = LR.Grid(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0))
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre_ = p.H_total[:3, 3]
        ref.follow(centre_, 48, 80)
        ref.add_from(p.view.points(p.view.count(view.LISTS) - 1), centre_)
        assert imgs[k].shape == (160, 96, 3) and np.array_equal(imgs[k], ref.render_local()), k
        k += 1
    assert k == 2 and ref.rays > 1000 and ref.ray_cells > 10 * ref.rays
    assert (ref.local_planes()["state"] == LR.SEEN).sum() > 50      # cells that were looked through and hold nothing
