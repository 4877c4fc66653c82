"""GPU: the traversability layer of the ground grid (include/svh_grid.h: svh_grid_set_traversability, svh_grid_get_trav,
svh_grid_render_cost; csrc/grid_trav_kernels.hip, csrc/grid_engine.cpp) against the numpy restatement
tests/grid_trav_ref.py, which tests/test_grid_trav.py pins on the CPU and whose DIST2 is a brute-force minimum over all
lethal cells.  Every comparison is exact: FLAGS, DIST2, COST and the cost image bit for bit.

Shapes: k_grid_trav_mask and k_grid_render_cost run 256 cells per workgroup; k_grid_dist_cols one lane per column, 64 per
workgroup, and per chunk of 32 rows; k_grid_dist_rows one workgroup per 256 cells of a row with a halo of `reach` on
either side.  The windows 1 x 1, 1 x 9, 9 x 1, 3 x 3, 64 x 1, 65 x 65 and 257 x 129 put lane, wave and tile edges on rows,
on columns and on both; 513 x 3 at reach 256 lets a halo span two neighbouring tiles and the window's end, 9 x 9 at reach
256 makes it wider than the row, 5 x 600 at reach 3 and 200 has chunks of rows that need their neighbours, and reach 1 is
the least halo there is.

The point sets are built as in tests/test_grid_local_gpu.py: cells of 0.5 from (0, 0), points in the cells' centres,
heights in sixteenths -- every HMEAN is exact in fp32."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_ref as R
import grid_trav_ref as TR
import helpers as H
import test_grid as TG
import test_grid_local_gpu as TL
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARG, HIP_ERR = -1, -2
CELL = TL.CELL
PLANES = ("flags", "dist2", "cost")


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


def pair(G, nx, nz, **tkw):
    """the restatement and the device object with the same window and the same traversability parameters"""
    P, Pc = TG.both(G, **TL.win_kw(nx, nz))
    ref, g = TR.Grid(P, TR.TravParams(**tkw)), G.Grid(Pc)
    g.set_traversability(**tkw)
    t, reach = g.traversability()
    assert reach == TR.reach_of(ref.T, CELL) and (t.max_slope, t.inscribed, t.inflate, t.lethal) == (
        ref.T.max_slope, ref.T.inscribed, ref.T.inflate, ref.T.lethal)
    return ref, g


def snapshot(G, g):
    out = {k: g.trav_plane(i) for i, k in enumerate(PLANES)}
    out["image"] = g.render_cost()
    return out


def check(G, g, ref, tag=""):
    want = ref.trav()
    want["image"] = want.pop("rgb")[::-1].copy()
    got = snapshot(G, g)
    for k, w in want.items():
        a = got[k]
        assert a.dtype == w.dtype and a.shape == w.shape, (tag, k)
        if a.tobytes() != w.tobytes():
            bad = np.argwhere(a != w)
            raise AssertionError("%s: %s differs in %d places, first %s: got %r, wanted %r" % (
                tag, k, len(bad), tuple(bad[0]), a[tuple(bad[0])], w[tuple(bad[0])]))
    return got


def fill(ref, rng, lethal, empty=None):
    """two points in the centre of every cell that is not `empty`, at heights of whole sixteenths in -0.25 .. 0.25: a free
    cell whose HMEAN is exact; where `lethal`, one of the two is a metre up: an obstacle.  Neighbouring free cells differ
    by up to 0.5, so with a rise of 0.125 many of them are steep"""
    nz, nx = lethal.shape
    ia, ib = np.meshgrid(np.arange(nx), np.arange(nz))
    keep = np.ones((nz, nx), bool) if empty is None else ~empty
    ia, ib, le = ia[keep], ib[keep], lethal[keep]
    h1 = rng.integers(-4, 5, len(ia)) / 16.0
    h2 = np.where(le, 1.0, rng.integers(-4, 5, len(ia)) / 16.0)
    return np.concatenate([TL.at_cells(ref, ia, ib, h1, 0.5), TL.at_cells(ref, ia, ib, h2, 0.5)])


def patterns(rng, nx, nz, dense=True):
    ia, ib = np.meshgrid(np.arange(nx), np.arange(nz))
    out = [("none", np.zeros((nz, nx), bool)), ("every cell", np.ones((nz, nx), bool)), ("one corner", (ia == nx - 1) & (ib == 0)),
           ("the last row", ib == nz - 1), ("the last column", ia == nx - 1), ("random 0.02", rng.random((nz, nx)) < 0.02)]
    if dense:
        out += [("a checkerboard", (ia + ib) % 2 == 1), ("random 0.3", rng.random((nz, nx)) < 0.3)]
    return out


def add_both(g, ref, pts):
    g.add_points(pts)
    ref.add(pts)


def run_patterns(G, nx, nz, pats, rng, **tkw):
    ref, g = pair(G, nx, nz, **tkw)
    for name, lethal in pats:
        g.clear()
        ref.clear()
        empty = rng.random((nz, nx)) < 0.1                       # unknown and not lethal under this mask: cost 0 becomes 255
        add_both(g, ref, fill(ref, rng, lethal, empty & ~lethal))
        got = check(G, g, ref, "%d x %d, %s" % (nx, nz, name))
        assert np.array_equal((got["flags"] & 2) != 0, lethal), name
        if name == "none":
            assert (got["dist2"] == TR.FAR).all() and set(np.unique(got["cost"])) <= {0, 255}
        if name == "every cell":
            assert not got["dist2"].any() and (got["cost"] == 254).all()
    return g, ref


# ---- lethal patterns on windows that put the edges everywhere ------------------------------------------------------------
@pytest.mark.parametrize("nx,nz", TL.WINDOWS)
def test_patterns(G, nx, nz):
    """reach 3 (inflate 1.5 at cells of 0.5), obstacles alone lethal, a rise of 0.125 so that the stencil finds steep cells"""
    rng = np.random.default_rng(1000 * nx + nz)
    g, ref = run_patterns(G, nx, nz, patterns(rng, nx, nz, dense=nx * nz <= 65 * 65), rng, max_slope=0.25, lethal=TR.L_OBSTACLE)
    if nx * nz >= 64:
        assert (g.trav_plane(G.TRAV_FLAGS) & 1).any()


def test_dense_patterns_on_the_largest_window(G):
    """257 x 129 with three in ten cells lethal, at reach 5"""
    rng = np.random.default_rng(3)
    run_patterns(G, 257, 129, [("random 0.3", rng.random((129, 257)) < 0.3)], rng, inflate=2.5, lethal=TR.L_OBSTACLE)


def test_steep_cells_are_lethal_by_default(G):
    """the default mask: the steep cells of a free window are its lethal cells"""
    rng = np.random.default_rng(4)
    ref, g = pair(G, 65, 65, max_slope=0.5)                                          # rise 0.25, corner 0.35355338
    add_both(g, ref, fill(ref, rng, np.zeros((65, 65), bool)))
    got = check(G, g, ref, "steep")
    steep = (got["flags"] & 1) != 0
    assert 100 < steep.sum() < 65 * 65 and np.array_equal(got["flags"] == 3, steep) and np.array_equal(got["dist2"] == 0, steep)


# ---- the reach ---------------------------------------------------------------------------------------------------------------
def test_reach_256_over_two_tiles_and_the_window_s_end(G):
    """513 x 3, inflate 128 m: the halo of the middle tile covers both neighbours, that of the last tile ends with the window"""
    rng = np.random.default_rng(5)
    ia, ib = np.meshgrid(np.arange(513), np.arange(3))
    pats = [("one corner", (ia == 0) & (ib == 2)), ("the last column", ia == 512), ("one cell", (ia == 256) & (ib == 1)),
            ("random 0.005", rng.random((3, 513)) < 0.005), ("none", np.zeros((3, 513), bool))]
    g, ref = run_patterns(G, 513, 3, pats[:4], rng, inflate=128.0, inscribed=100.0, lethal=TR.L_OBSTACLE)
    assert g.traversability()[1] == 256
    g.clear()
    ref.clear()
    add_both(g, ref, fill(ref, rng, pats[0][1]))
    got = check(G, g, ref, "the corner again, nothing empty")
    assert got["dist2"][2, 256] == 256 * 256 and got["dist2"][2, 257] == TR.FAR and got["dist2"][0, 256] == TR.FAR
    assert got["cost"][2, 256] == 0 and got["cost"][2, 200] == 253 and got["cost"][2, 201] < 253     # 100 m are 200 cells


def test_reach_1(G):
    rng = np.random.default_rng(6)
    g, ref = run_patterns(G, 65, 65, patterns(rng, 65, 65), rng, inflate=0.5, inscribed=0.25, lethal=TR.L_OBSTACLE)
    assert g.traversability()[1] == 1
    assert set(np.unique(g.trav_plane(G.TRAV_DIST2))) == {0, 1, TR.FAR}


def test_reach_256_on_a_window_smaller_than_the_halo(G):
    rng = np.random.default_rng(7)
    run_patterns(G, 9, 9, patterns(rng, 9, 9), rng, inflate=128.0, lethal=TR.L_OBSTACLE)


@pytest.mark.parametrize("inflate", [1.5, 100.0])
def test_columns_longer_than_a_chunk_of_rows(G, inflate):
    """5 x 600: the column sweeps run in chunks of rows; a lethal cell just before, just after and far from a chunk's edge, a reach
    below and far above the chunk's 32 rows"""
    rng = np.random.default_rng(8)
    ia, ib = np.meshgrid(np.arange(5), np.arange(600))
    pats = [("rows 255 and 256", (ib == 255) | ((ib == 256) & (ia == 0))), ("row 0", ib == 0), ("row 599", ib == 599),
            ("one cell at 300", (ib == 300) & (ia == 2)), ("random 0.01", rng.random((600, 5)) < 0.01)]
    run_patterns(G, 5, 600, pats, rng, inflate=inflate, lethal=TR.L_OBSTACLE)


# ---- the whole mask, rays, the scroll ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lethal", [7, TR.L_ALL, TR.L_UNSEEN, TR.L_UNKNOWN_SEEN | TR.L_DROP, 0])
def test_after_a_scroll_and_a_second_add(G, lethal):
    """random clouds with rays: every class, seen and unseen unknown cells; the torus offsets are not zero"""
    rng = np.random.default_rng(9)
    ref, g = pair(G, 65, 33, max_slope=0.25, lethal=lethal)
    TL.from_both(g, ref, TL.cloud(ref, rng, 6000), TL.centre(ref, 30, 2))
    check(G, g, ref, "before the scroll")
    g.scroll(3, -2)
    ref.scroll(3, -2)
    check(G, g, ref, "scrolled")
    TL.from_both(g, ref, TL.cloud(ref, rng, 3000), TL.centre(ref, 10, 20))
    got = check(G, g, ref, "a second add")
    TL.check(G, g, ref, "the grid itself")
    state = g.local_plane(G.LOCAL_STATE)
    assert g.window() == (3, -2) and len(np.unique(state & 0x43)) >= 6
    if lethal == 0:
        assert not (got["flags"] & 2).any() and (got["dist2"] == TR.FAR).all()


# ---- the cache ------------------------------------------------------------------------------------------------------------
def test_the_cache(G):
    rng = np.random.default_rng(10)
    ref, g = pair(G, 65, 65, max_slope=0.25)
    TL.from_both(g, ref, TL.cloud(ref, rng, 5000), TL.centre(ref, 32, 0))
    a = check(G, g, ref, "first")
    b = snapshot(G, g)                                           # nothing changed: the same planes, from the cache
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    g.plane(G.CLASS)                                             # the other gets do not disturb it
    g.render_local()
    assert all(a[k].tobytes() == snapshot(G, g)[k].tobytes() for k in a)
    (b0, a0), (b1, a1) = np.argwhere(a["dist2"] != 0)[[0, -1]]   # two cells that are not lethal become obstacles
    add_both(g, ref, TL.at_cells(ref, [a0, a0, a1, a1], [b0, b0, b1, b1], [0.0, 1.5, 0.0, 1.5]))
    c = check(G, g, ref, "after an add")
    assert c["dist2"][b0, a0] == 0 and c["dist2"][b1, a1] == 0 and c["dist2"].tobytes() != a["dist2"].tobytes()
    for kw in (dict(inflate=4.0), dict(lethal=TR.L_OBSTACLE), dict(max_slope=0.1), dict(inscribed=1.0)):
        g.set_traversability(**kw)
        for k, v in kw.items():
            setattr(ref.T, k, F(v) if k != "lethal" else v)
        d = check(G, g, ref, "after set_traversability(%r)" % kw)
        assert "max_slope" in kw or any(d[k].tobytes() != c[k].tobytes() for k in d), kw
        c = d
    g.clear()
    ref.clear()
    e = check(G, g, ref, "cleared")
    assert (e["dist2"] == TR.FAR).all() and (e["cost"] == 255).all() and not e["flags"].any()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte(G):
    rng = np.random.default_rng(11)
    ref, g = pair(G, 65, 33, max_slope=0.25)
    TL.from_both(g, ref, TL.cloud(ref, rng, 4000), TL.centre(ref, 30, 2))
    before, grid_before = check(G, g, ref, "before"), TL.snapshot(G, g)
    L = g._L
    buf = np.full(65 * 33 * 4, 0xAB, np.uint8)
    import test_grid_trav as TT
    for kw in TT.BAD + [dict(inflate=128.5), dict(inflate=1e30)]:           # 257 cells and more
        t = G.default_trav(**kw)
        assert L.svh_grid_set_traversability(g._h, C.byref(t)) == BAD_ARG and "svh_grid_set_traversability" in G.last_error(), kw
    reach = C.c_int32(-7)
    calls = [lambda: L.svh_grid_set_traversability(g._h, None), lambda: L.svh_grid_get_traversability(g._h, None, None),
             lambda: L.svh_grid_get_trav(g._h, 3, buf.ctypes.data, 0), lambda: L.svh_grid_get_trav(g._h, -1, buf.ctypes.data, 0),
             lambda: L.svh_grid_get_trav(g._h, 0, None, 0), lambda: L.svh_grid_render_cost(g._h, None, 0)]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG and "svh_grid" in G.last_error(), k
    assert (buf == 0xAB).all()
    assert L.svh_grid_get_traversability(g._h, None, C.addressof(reach)) == 0 and reach.value == 3
    assert TL.same(snapshot(G, g), before) and TL.same(TL.snapshot(G, g), grid_before)
    t, _ = g.traversability()
    assert (t.max_slope, t.inscribed, t.inflate, t.lethal) == (F(0.25), F(0.4), F(1.5), 7)


def test_a_cell_the_defaults_do_not_fit(G):
    """cells of 5 mm: the default inflation radius would be 300 cells.  The object exists and works; the layer refuses until
    parameters that fit are set"""
    g = G.Grid(G.default_params(nx=9, nz=9, cell=0.005, x0=0.0, z0=0.0, T=R.frame_camera(0.0), min_points=1))
    g.add_points(np.array([[0.0225, 0.0, 0.0225, 0.5], [0.0125, -0.5, 0.0025, 0.5]], F))   # cell (4, 4) free, cell (2, 0) an obstacle
    buf = np.full(81 * 4, 0xAB, np.uint8)
    assert g.traversability()[1] == 0 and g.classes()[4, 4] == G.FREE and g.classes()[0, 2] == G.OBSTACLE
    assert g._L.svh_grid_get_trav(g._h, G.TRAV_COST, buf.ctypes.data, 0) == BAD_ARG and "svh_grid_set_traversability" in G.last_error()
    assert g._L.svh_grid_render_cost(g._h, buf.ctypes.data, 0) == BAD_ARG and (buf == 0xAB).all()
    with pytest.raises(G.SvhError):
        g.set_traversability()                                   # the defaults again: still refused
    g.set_traversability(inscribed=0.004, inflate=0.02)
    assert g.traversability()[1] == 4
    d2 = g.trav_plane(G.TRAV_DIST2)
    assert d2[0, 2] == 0 and d2[0, 0] == 4 and d2[3, 2] == 9 and d2[4, 2] == 16 and d2[4, 4] == TR.FAR
    assert g.render_cost().shape == (9, 9, 3)


# ---- failures --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["launch:1", "launch:2", "copy:1", "wait:1", "malloc:1"])
def test_a_failed_get_leaves_the_grid(G, spec):
    """after an add: launch:1 is the finalise, launch:2 the layer's three kernels, copy:1 and wait:1 the delivery, malloc:1
    the layer's planes (the object is new).  SVH_ERR_HIP, the accumulated grid is untouched, and the call repeated delivers"""
    rng = np.random.default_rng(12)
    ref, g = pair(G, 65, 65, max_slope=0.25)
    TL.from_both(g, ref, TL.cloud(ref, rng, 4000), TL.centre(ref, 7, 60))
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.trav_plane(G.TRAV_COST)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    TL.check(G, g, ref, spec + ": the grid")
    check(G, g, ref, spec + ": the call repeated")
    # the same inside the render, with the planes cached: its own launch, and a set_traversability whose upload fails
    G.lib().svh_test_fail_at(b"launch:1")
    with pytest.raises(G.SvhError) as e:
        g.render_cost()
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    check(G, g, ref, spec + ": after a failed render")
    G.lib().svh_test_fail_at(b"copy:1")
    with pytest.raises(G.SvhError) as e:
        g.set_traversability(inflate=3.0)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    ref.T.inflate = F(3.0)                                       # the parameters are set; the next get uploads the table
    TL.check(G, g, ref, spec + ": the grid, again")
    check(G, g, ref, spec + ": after a failed upload")


# ---- device pointers -----------------------------------------------------------------------------------------------------------
def test_device_pointers(G, hip):
    rng = np.random.default_rng(13)
    ref, g = pair(G, 100, 60, max_slope=0.25)
    TL.from_both(g, ref, TL.cloud(ref, rng, 7000), TL.centre(ref, 50, 0))
    want = ref.trav()
    for k, name in enumerate(PLANES):
        nbytes = want[name].nbytes
        out = Dev(hip, nbytes + 16)
        g.trav_plane(k, device_ptr=out.addr)
        got = out.get()
        assert got[:nbytes].tobytes() == want[name].tobytes() and (got[nbytes:] == 0xEE).all(), name
    out = Dev(hip, 100 * 60 * 3 + 16)
    g.render_cost(device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:18000].reshape(60, 100, 3), ref.render_cost()) and (got[18000:] == 0xEE).all()
    check(G, g, ref, "to the host afterwards")


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------------
def test_pipeline_grid_cost(G, tmp_path, monkeypatch, capsys):
    """--grid-local DIR --grid-cost DIR2 on the two golden frames: one cost image per frame, the restatement's after the
    same steps"""
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
    d, d2 = str(tmp_path / "loc"), str(tmp_path / "cost")
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-slope", "0.3",
                                      "--grid-inflate", "2.0", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)])
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("cost map: slope 0.3, inscribed 0.4 m, inflation 2 m = 8 cells; 2 images") for l in out), out[-3:]
    assert sorted(os.listdir(d2)) == ["cost_%06d.ppm" % k for k in range(2)] and len(os.listdir(d)) == 2
    imgs = [read_ppm(os.path.join(d2, "cost_%06d.ppm" % k)) for k in range(2)]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = TR.Grid(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0), TR.TravParams(max_slope=0.3, inflate=2.0))
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre_ = p.H_total[:3, 3]
        ref.follow(centre_, 48, 80)
        ref.add_from(p.view.points(p.view.count(view.LISTS) - 1), centre_)
        assert imgs[k].shape == (160, 96, 3) and np.array_equal(imgs[k], ref.render_cost()), k
        k += 1
    tr = ref.trav()
    assert k == 2 and (tr["flags"] & 2).sum() > 50 and ((tr["cost"] > 0) & (tr["cost"] < 253)).sum() > 50
    # and the flags are refused without --grid-local
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-cost", d2, drive, str(calib)])
    with pytest.raises(SystemExit):
        SP.main()
