"""GPU: the archive of the ground grid (include/svh_grid_archive.h: svh_grid_set_archive, svh_grid_archive_*, svh_grid_get_region,
svh_grid_render_region; csrc/grid_archive_kernels.hip, csrc/grid_engine.cpp) against the numpy restatement
tests/grid_archive_ref.py, which tests/test_grid_archive.py pins on the CPU.  Every comparison is exact: the seven planes of
svh_grid_get bit for bit, the two local planes, the planes of the dynamics, the statistics of the archive, its tiles, the regions.

Shapes: windows of 40 x 24 cells at offsets on both sides of 0, so that tiles of 16 x 16 straddle every edge of the window, and of
16 x 16; scrolls of 1, 15, 16, 17, n - 1, n, n + 1 and 3 n cells with each sign, alone and diagonal: strips narrower than a tile, as
wide, wider, the whole window (|d| >= n) and far jumps.  Every kernel of the layer runs 256 lanes per workgroup: the strips of these
windows have from 16 to 960 cells, less than one workgroup and several."""
import ctypes as C

import numpy as np
import pytest

import grid_archive_ref as AR
import grid_dyn_ref as DR
import grid_local_ref as LR
import grid_ref as R
import test_grid as TG
import test_grid_archive as TA
import test_grid_dyn as TD
import test_grid_dyn_gpu as TDG
import test_grid_local_gpu as TL
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARG = -1
CELL = TD.CELL


@pytest.fixture(scope="module")
def G():
    import svhip
    from svhip import grid
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    grid._bind()
    return grid


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def pair(G, nx, nz, off=(0, 0), max_tiles=64, dyn=None):
    """the restatement and the object with the same window (cells of 0.5, h = 1.5 - y) at the same offsets, the archive set and empty"""
    P, Pc = TG.both(G, **TD.hand_kw(nx=nx, nz=nz))
    ref, g = AR.Grid(P, None if dyn is None else DR.DynParams(**dyn), 0), G.Grid(Pc)
    if dyn is not None:
        g.set_dynamics(G.default_dyn(**dyn))
    if off != (0, 0):
        ref.scroll(*off)
        g.scroll(*off)
    ref.set_archive(max_tiles)
    g.set_archive(max_tiles=max_tiles)
    return ref, g


def planes_of(G, g):
    out = {k: g.plane(i) for i, k in enumerate(R.PLANES)}
    out["passed"], out["state"] = g.local_plane(G.LOCAL_PASS), g.local_plane(G.LOCAL_STATE)
    return out


def same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def differing(a, b):
    return [k for k in a if a[k].tobytes() != b[k].tobytes()]


def check(G, g, ref, tag=""):
    """the window, the statistics of the archive and its tiles against the restatement"""
    got = TL.check(G, g, ref, tag)
    assert g.archive_stats() == ref.archive_stats(), (tag, g.archive_stats(), ref.archive_stats())
    assert g.archive_tiles().tolist() == ref.archive_tiles().tolist(), tag
    return got


def check_region(G, g, ref, ga0, gb0, w, h, tag=""):
    want = ref.region(ga0, gb0, w, h)
    for i, k in enumerate(R.PLANES):
        a = g.region(i, ga0, gb0, w, h)
        assert a.dtype == want[k].dtype and a.shape == (h, w) and a.tobytes() == want[k].tobytes(), (tag, k)
    for i, k in enumerate(("passed", "state")):
        a = g.region(i, ga0, gb0, w, h, kind=G.REGION_LOCAL)
        assert a.dtype == want[k].dtype and a.tobytes() == want[k].tobytes(), (tag, k)
    for mode in range(4):
        assert np.array_equal(g.render_region(ga0, gb0, w, h, mode), ref.render_region(ga0, gb0, w, h, mode)), (tag, "mode %d" % mode)
    return want


def fill(g, ref, seed=3):
    rng = np.random.default_rng(seed)
    pts = TA.scene(ref, rng, 6 * ref.P.nx * ref.P.nz)
    o = TA.centre(ref, ref.P.nx // 2, 0)
    for x in (g, ref):
        (x.add_points_from if x is g else x.add_from)(pts, o)
    return pts, o


# ---- away and back equals never moved -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz,off", [(40, 24, (-53, 7)), (40, 24, (9, -70)), (16, 16, (-8, -8))])
def test_away_and_back_equals_never_moved(G, nx, nz, off):
    """the test the layer exists for: after every scroll of the list and its inverse, every plane of svh_grid_get and
    svh_grid_get_local equals that of a twin that never scrolled.  Without svh_grid_set_archive the strips come back empty"""
    ref, g = pair(G, nx, nz, off)
    _, twin = pair(G, nx, nz, off, max_tiles=0)
    pts, o = fill(g, ref)
    twin.add_points_from(pts, o)
    want = planes_of(G, twin)
    assert (want["count"] > 0).sum() > nx * nz // 2 and (want["passed"] > 0).sum() > nx * nz // 4
    for da, db in TA.scrolls(nx, nz):
        g.scroll(da, db)
        g.scroll(-da, -db)
        got = planes_of(G, g)
        assert same(got, want), ((da, db), differing(got, want))
        ref.scroll(da, db).scroll(-da, -db)
    check(G, g, ref, "after the list")
    st = g.archive_stats()
    assert st["lost"] == 0 and st["refused"] == 0 and st["stored"] == st["restored"] > 0 and st["pages"] > 0
    # the same call on today's path: the strips are forgotten
    twin.scroll(1, 0)
    twin.scroll(-1, 0)
    got = planes_of(G, twin)
    assert not same(got, want) and (got["count"][:, 0] == 0).all() and np.array_equal(got["count"][:, 1:], want["count"][:, 1:])
    g.close(), twin.close()


# ---- a walk round a square ------------------------------------------------------------------------------------------------------
def test_a_walk_round_a_square(G):
    nx, nz = 40, 24
    ref, g = pair(G, nx, nz, (-30, -20), max_tiles=256)
    rng = np.random.default_rng(11)
    a0, b0 = ref.window()
    k = 0
    for leg, (ua, ub) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
        done = 0
        while done < 2 * nx:
            step = min((3, 7)[k % 2], 2 * nx - done)
            k += 1
            done += step
            g.scroll(ua * step, ub * step)
            ref.scroll(ua * step, ub * step)
            if k % 3 == 0:
                pts, o = TA.scene(ref, rng, 400), TA.centre(ref, nx // 2, nz // 2)
                g.add_points_from(pts, o)
                ref.add_from(pts, o)
        check(G, g, ref, "leg %d" % leg)
    assert ref.window() == (a0, b0) and ref.archive_stats()["pages"] > 20 and ref.archive_stats()["restored"] > 0 and ref.archive_stats()["lost"] == 0
    # the whole walk, from the window and the archive together; then the window's own box, which is svh_grid_get
    whole = check_region(G, g, ref, a0 - 2, b0 - 2, 2 * nx + nx + 4, 2 * nx + nz + 4, "the whole walk")
    assert (whole["count"] > 0).sum() > 3 * nx * nz
    own = check_region(G, g, ref, a0, b0, nx, nz, "the window")
    got = planes_of(G, g)
    assert same({k: own[k] for k in got}, got)
    assert np.array_equal(g.render_region(a0, b0, nx, nz), g.render_local()) and np.array_equal(g.render_region(a0, b0, nx, nz, 1), g.render(1))
    g.close()


# ---- the dynamics ---------------------------------------------------------------------------------------------------------------
def dyn_check(G, g, ref, tag):
    got = TDG.check(G, g, ref, tag)
    assert g.archive_stats() == ref.archive_stats(), (tag, g.archive_stats(), ref.archive_stats())
    return got


def observe(g, ref, pts, o):
    g.observe_points(pts, o)
    ref.observe(pts, o)


def obstacle(ref):
    """a tall thing in window cell (20, 6) and the ground behind it at (20, 12): a line from the camera's 1.5 to the ground passes the
    obstacle's cell at 0.75, inside its body 0.1 .. 1.8"""
    return TDG.at(ref, [20, 20], [6, 6], [0.1, 1.9]), TDG.at(ref, [20, 20], [12, 12], [0.0, 0.0])


def test_a_cell_emptied_in_the_window_overwrites_its_record(G):
    ref, g = pair(G, 40, 24, (5, -9), dyn=dict(clear_frames=1, min_through=1))
    tall, ground = obstacle(ref)
    o = TDG.centre(ref, 20, 0)
    observe(g, ref, tall, o)
    assert dyn_check(G, g, ref, "the obstacle")["count"][6, 20] == 2
    for d, tag in ((10, "it leaves"), (-10, "it is back")):
        g.scroll(0, d)
        ref.scroll(0, d)
        got = dyn_check(G, g, ref, tag)
    assert got["count"][6, 20] == 2 and got["age"][6, 20] == 0 and ref.archive_stats()["restored"] == 144   # nine rows of the one tile that the obstacle and its sight line lie in
    observe(g, ref, ground, TDG.centre(ref, 20, 0))
    got = dyn_check(G, g, ref, "contradicted")
    assert got["count"][6, 20] == 0 and ref.dyn_stats["cleared"] == 1
    for d, tag in ((10, "the cleared cell leaves"), (-10, "and is back")):
        g.scroll(0, d)
        ref.scroll(0, d)
        got = dyn_check(G, g, ref, tag)
    assert got["count"][6, 20] == 0 and (got["cls"][6, 20] & 3) == 0, "the older record of the obstacle was to be overwritten"
    g.close()


def test_contra_and_last_round_trip_and_age(G):
    """clear_frames 3: one contradiction leaves CONTRA 1, which leaves and comes back; max_age 2: a cell that comes back after more
    observations than that is aged by the next one"""
    ref, g = pair(G, 40, 24, (-45, 3), dyn=dict(clear_frames=3, min_through=1, max_age=2))
    tall, ground = obstacle(ref)
    observe(g, ref, tall, TDG.centre(ref, 20, 0))
    observe(g, ref, ground, TDG.centre(ref, 20, 0))
    assert dyn_check(G, g, ref, "contradicted once")["contra"][6, 20] == 1
    g.scroll(-17, 10)
    ref.scroll(-17, 10)
    dyn_check(G, g, ref, "away")
    g.scroll(17, -10)
    ref.scroll(17, -10)
    got = dyn_check(G, g, ref, "back at once")
    assert got["contra"][6, 20] == 1 and got["age"][6, 20] == 1 and got["count"][6, 20] == 2
    g.scroll(0, 16)
    ref.scroll(0, 16)
    for _ in range(3):
        observe(g, ref, np.zeros((0, 4), F), TDG.centre(ref, 20, 0))
    g.scroll(0, -16)
    ref.scroll(0, -16)
    got = dyn_check(G, g, ref, "back after three observations")
    assert got["age"][6, 20] == 4 and got["count"][6, 20] == 2
    observe(g, ref, np.zeros((0, 4), F), TDG.centre(ref, 20, 0))
    got = dyn_check(G, g, ref, "the next observation")
    assert got["count"][6, 20] == 0 and ref.dyn_stats["aged"] >= 1
    g.close()


# ---- capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity(G):
    """test_grid_archive.test_capacity_by_hand on the device: 16 x 16 over four tiles, two pages"""
    ref, g = pair(G, 16, 16, (8, 8), max_tiles=2)
    ia, ib = np.meshgrid(np.arange(16), np.arange(16))
    pts = TD.at(ia.ravel() + 8, ib.ravel() + 8, 0.1)
    pts = np.concatenate([pts, pts])

    def both(da, db):
        g.scroll(da, db)
        ref.scroll(da, db)

    g.add_points(pts)
    ref.add(pts)
    full = planes_of(G, g)
    both(100, 0)
    both(-100, 0)
    got = check(G, g, ref, "four tiles for two pages")
    assert g.archive_stats() == dict(pages=0, max_tiles=2, stored=0, restored=0, lost=256, refused=1) and (got["count"] == 0).all()
    g.add_points(pts)
    ref.add(pts)
    both(1, 0)
    check(G, g, ref, "two tiles for two pages")
    assert g.archive_stats()["pages"] == 2 and g.archive_tiles().tolist() == [[0, 0], [0, 1]]
    both(8, 0)
    check(G, g, ref, "two paged tiles and two refused")
    assert g.archive_stats() == dict(pages=2, max_tiles=2, stored=16 + 7 * 16, restored=0, lost=256 + 16, refused=2)
    both(-9, 0)
    got = check(G, g, ref, "back")
    assert np.array_equal(got["count"][:, :8], full["count"][:, :8]) and (got["count"][:, 8] == 0).all() and np.array_equal(got["count"][:, 9:], full["count"][:, 9:])
    g.close()
    # one new tile while one page is free, with a paged tile also touched: both are stored
    ref, g = pair(G, 16, 16, (8, 8), max_tiles=2)
    g.add_points(pts)
    ref.add(pts)
    g.scroll(1, 0)
    ref.scroll(1, 0)                                    # tiles (0, 0) and (0, 1)
    g.archive_trim(8, 8, 8, 8)
    ref.archive_trim(8, 8, 8, 8)                         # (0, 0) alone: one page is free again
    check(G, g, ref, "trimmed to one tile")
    g.scroll(0, 8)
    ref.scroll(0, 8)                                    # rows 8 .. 15 leave: tile (0, 0), paged, and (1, 0) of the columns 16 .. 24, new
    check(G, g, ref, "one paged, one new")
    assert g.archive_stats()["pages"] == 2 and g.archive_stats()["refused"] == 0 and g.archive_tiles().tolist() == [[0, 0], [1, 0]]
    g.close()


# ---- trim and clear -------------------------------------------------------------------------------------------------------------
def test_trim_and_clear(G):
    nx, nz = 40, 24
    ref, g = pair(G, nx, nz, (-53, 7), max_tiles=16)
    fill(g, ref)

    def jump(da, db):
        g.scroll(da, db)
        ref.scroll(da, db)

    jump(3 * nx, 0)
    check(G, g, ref, "the window archived")
    tiles = g.archive_tiles()
    assert len(tiles) == 8 and tiles.tolist() == sorted(tiles.tolist(), key=lambda t: (t[1], t[0]))
    g.archive_trim(-40, 0, -30, 40)
    ref.archive_trim(-40, 0, -30, 40)
    check(G, g, ref, "trimmed")
    assert g.archive_tiles().tolist() == [[-3, 0], [-2, 0], [-3, 1], [-2, 1]] and g.archive_stats()["pages"] == 4
    fill(g, ref, seed=4)
    jump(0, 5 * nz)                                     # the pages that the trim returned are used again: 12 tiles at most, 16 pages
    check(G, g, ref, "pages used again")
    assert g.archive_stats()["pages"] > 8 and g.archive_stats()["refused"] == 0
    jump(-3 * nx, -5 * nz)
    check(G, g, ref, "back over the trimmed tiles")
    with pytest.raises(G.SvhError) as e:
        g.archive_trim(5, 0, 4, 0)
    assert e.value.code == BAD_ARG
    with pytest.raises(G.SvhError):
        g.archive_trim(0, 0, 2 ** 20, 0)
    check(G, g, ref, "refusals change nothing")
    # each of these empties the archive
    for name in ("archive_clear", "clear", "set_window", "set_archive"):
        fill(g, ref, seed=5)
        jump(2 * nx, 0)
        assert g.archive_stats()["pages"] > 0
        if name == "set_window":
            g.set_window(1.0, -2.0)
            ref.set_window(1.0, -2.0)
        elif name == "set_archive":
            g.set_archive(max_tiles=17)
            ref.set_archive(17)
        else:
            getattr(g, name)()
            getattr(ref, name)()
        check(G, g, ref, name)
        assert g.archive_stats() == dict(pages=0, max_tiles=g.archive().max_tiles, stored=0, restored=0, lost=0, refused=0) and len(g.archive_tiles()) == 0
        jump(-2 * nx, 0) if name not in ("clear", "set_window") else None
        assert (check(G, g, ref, name + ", back")["count"] == 0).all(), "what was archived was to be forgotten"
    g.set_archive(max_tiles=17)                         # the value in force: nothing changes
    with pytest.raises(G.SvhError):
        g.set_archive(max_tiles=2 ** 20 + 1)
    with pytest.raises(G.SvhError):
        g.set_archive(max_tiles=-1)
    assert g.archive().max_tiles == 17
    g.close()


# ---- regions --------------------------------------------------------------------------------------------------------------------
def test_region_edge_cases(G, hip):
    nx, nz = 40, 24
    ref, g = pair(G, nx, nz, (9, -70))
    fill(g, ref)
    g.scroll(30, 10)
    ref.scroll(30, 10)
    oa, ob = ref.window()
    before = planes_of(G, g)
    empty = check_region(G, g, ref, 5000, -7000, 33, 17, "outside the window and every tile")
    assert (empty["count"] == 0).all() and (empty["cls"] == 0).all() and np.isnan(empty["hmean"]).all()
    check_region(G, g, ref, oa - 1, ob - 1, 1, 1, "one archived cell")
    check_region(G, g, ref, oa + 3, ob + 3, 1, 1, "one cell of the window")
    cut = check_region(G, g, ref, oa - 23, ob - 7, 37, 19, "a box that cuts tiles and the window")
    assert (cut["count"][:7] > 0).sum() > 50 and (cut["count"][7:, 23:] > 0).sum() > 50
    check_region(G, g, ref, -2 ** 20 + 1, 2 ** 20 - 9, 9, 9, "the corner of the global cells")
    # device and host outputs agree
    for kind, plane, size in ((G.REGION_GRID, G.HMEAN, 4), (G.REGION_GRID, G.CLASS, 1), (G.REGION_LOCAL, G.LOCAL_PASS, 4), (G.REGION_LOCAL, G.LOCAL_STATE, 1)):
        d = Dev(hip, 37 * 19 * size + 16)
        g.region(plane, oa - 23, ob - 7, 37, 19, kind=kind, device_ptr=d.addr)
        raw = d.get()
        assert raw[:37 * 19 * size].tobytes() == g.region(plane, oa - 23, ob - 7, 37, 19, kind=kind).tobytes() and (raw[37 * 19 * size:] == 0xEE).all()
    d = Dev(hip, 37 * 19 * 3 + 16)
    g.render_region(oa - 23, ob - 7, 37, 19, device_ptr=d.addr)
    assert d.get()[:37 * 19 * 3].tobytes() == g.render_region(oa - 23, ob - 7, 37, 19).tobytes() and (d.get()[37 * 19 * 3:] == 0xEE).all()
    # bad arguments
    L, buf = g._L, np.zeros(64, np.int64)
    stats = g.archive_stats()
    for args in ((2, 0, 0, 0, 1, 1), (0, 7, 0, 0, 1, 1), (1, 2, 0, 0, 1, 1), (0, -1, 0, 0, 1, 1), (0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 1, 8193),
                 (0, 0, -2 ** 20, 0, 1, 1), (0, 0, 2 ** 20 - 1, 0, 2, 1), (0, 0, 0, 2 ** 20 - 8, 1, 9)):
        assert L.svh_grid_get_region(g._h, *args, buf.ctypes.data, 0) == BAD_ARG, args
    assert L.svh_grid_get_region(g._h, 0, 0, 0, 0, 1, 1, None, 0) == BAD_ARG and L.svh_grid_render_region(g._h, 4, 0, 0, 1, 1, buf.ctypes.data, 0) == BAD_ARG
    assert L.svh_grid_render_region(g._h, 0, 0, 0, 8193, 1, buf.ctypes.data, 0) == BAD_ARG and (buf == 0).all()
    assert same(planes_of(G, g), before) and g.archive_stats() == stats
    # with the layer off the cells outside the window are empty
    g.set_archive(max_tiles=0)
    ref.set_archive(0)
    off = check_region(G, g, ref, oa - 23, ob - 7, 37, 19, "the layer off")
    assert (off["count"][:7] == 0).all() and (off["count"][7:, 23:] > 0).sum() > 50
    g.close()


# ---- the layer off --------------------------------------------------------------------------------------------------------------
def test_layer_off_scrolls_as_ever(G):
    """without svh_grid_set_archive, and after svh_grid_set_archive(0): the scroll of tests/grid_local_ref.py, strips forgotten"""
    nx, nz = 40, 24
    for tag in ("never set", "set and dropped"):
        P, Pc = TG.both(G, **TD.hand_kw(nx=nx, nz=nz))
        ref, g = LR.Grid(P), G.Grid(Pc)
        if tag != "never set":
            g.set_archive(max_tiles=8)
            g.set_archive(max_tiles=0)
        rng = np.random.default_rng(2)
        for k, (da, db) in enumerate(TA.scrolls(nx, nz)[::5]):
            pts, o = TA.scene(ref, rng, 500), TA.centre(ref, nx // 2, 0)
            g.add_points_from(pts, o)
            ref.add_from(pts, o)
            g.scroll(da, db)
            ref.scroll(da, db)
            TL.check(G, g, ref, "%s, scroll %d by (%d, %d)" % (tag, k, da, db))
        assert g.archive_stats() == dict(pages=0, max_tiles=0, stored=0, restored=0, lost=0, refused=0) and len(g.archive_tiles()) == 0
        g.close()


# ---- the pipeline tool ----------------------------------------------------------------------------------------------------------
def test_pipeline_grid_archive(G, tmp_path, monkeypatch, capsys):
    """--grid-archive DIR on the two golden frames: per frame the statistics, at the end the mosaic over the window and every tile,
    both the restatement's after the same steps"""
    import json
    import os
    import sys
    import helpers as H
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify
    from svhip import kitti, view
    from test_grid_gpu import read_ppm
    from test_view_gpu import two_frame_drive
    drive = str(two_frame_drive(tmp_path / "drive"))
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(test_rectify.rig_calib_text())
    d, a = str(tmp_path / "loc"), str(tmp_path / "arch")
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-archive", a, "--grid-archive-tiles", "64",
                                      "--grid-cell", "0.1", "--grid-size", "96x160", drive, str(calib)])
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert sorted(os.listdir(a)) == ["archive.jsonl", "mosaic.ppm"] and any(l.startswith("archive: ") for l in out)
    lines = [json.loads(l) for l in open(os.path.join(a, "archive.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = AR.Grid(R.Params(nx=96, nz=160, cell=0.1, x0=-4.8, z0=0.0), None, 64)
    ref.nx, ref.nz = 96, 160                                      # what mosaic_box asks of an object
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre = p.H_total[:3, 3]
        ref.follow(centre, 48, 80)
        ref.add_from(p.view.points(p.view.count(view.LISTS) - 1), centre)
        assert np.array_equal(read_ppm(os.path.join(d, "local_%06d.ppm" % k)), ref.render_local()), k
        assert lines[k] == dict(ref.archive_stats(), frame=k, window=list(ref.window())), (k, lines[k], ref.archive_stats())
        k += 1
    box = SP.mosaic_box(ref)
    assert k == 2 and box[2] >= 96 and box[3] >= 160
    assert np.array_equal(read_ppm(os.path.join(a, "mosaic.ppm")), ref.render_region(*box))
