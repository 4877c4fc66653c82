"""GPU: the objects of the ground grid and their tracks (include/svh_grid_obj.h, "OBJECTS"; csrc/grid_obj_kernels.hip,
csrc/grid_engine.cpp) against the restatement tests/grid_obj_ref.py, which tests/test_grid_obj.py pins on the CPU and compares with
the header.  Every comparison is exact: FLAGS, LABEL, the ID plane, both tables, ASSIGN, the statistics and the image byte for byte.

Shapes: the labelling runs one workgroup of 256 lanes per tile of T x T cells, T = FRONT_TILE = 16; the per-cell kernels run 256
cells per workgroup, the ordered compactions and the track update 1024.  The windows 16 x 16, 17 x 33 and 48 x 40 are one tile,
ragged tiles and several tiles.  The planes go through the test entry svh_test_grid_obj_device; the steps through the Grid object,
which is rebuilt from points per frame (tests/grid_obj_cases.py).

The issue asks for "a 64 x 64 checkerboard of one-cell objects: 2048 objects".  The cells of a checkerboard touch by their corners,
so under 8-connectivity it is ONE component of 2048 cells; both are played here: the checkerboard as it is, and 2048 one-cell objects
on every second cell of every second row of a 128 x 64 window, which is what exercises the table of pairs and the record-level
kernels beyond one workgroup."""
import ctypes as C

import numpy as np
import pytest

import grid_obj_cases as OC
import grid_obj_ref as OR
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2
LAUNCHES = 14                                                    # a constant of the build: grid_internal.h, OBJ_LAUNCHES
F = np.float32
WINDOWS = [(16, 16), (17, 33), (48, 40)]


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


def differ(tag, name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, name, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %s differs at %d places, first %s: %s, restatement %s" % (tag, name, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def planes(G, frame, tag="", **kw):
    """svh_test_grid_obj_device against the restatement"""
    kw = dict(dict(min_size=1, min_height=0.0), **kw)
    got = G.device_obj(G.default_obj(**kw), frame.state, frame.hmax, frame.count, *frame.off)
    want = OR.objects(OR.ObjParams(**kw), frame.state, frame.hmax, frame.count, *frame.off)
    for k, name in enumerate(("FLAGS", "LABEL", "the table")):
        differ(tag, name, got[k], want[k])
    assert got[3] == want[3] + (LAUNCHES,), (tag, got[3], want[3])
    return got


def random_frame(rng, nx, nz, density, off=(0, 0)):
    f = OC.Frame(nx, nz, off=off)
    f.state = rng.choice(np.array([0, 1, 3, 0x41, 0x82], np.uint8), (nz, nx))     # 0x82: an obstacle under an overhang
    f.state[rng.random((nz, nx)) < density] = 2
    f.hmax = (0.25 * rng.integers(1, 9, (nz, nx))).astype(F)
    f.count = rng.integers(0, 50, (nz, nx)).astype(np.int32)
    return f


def play(G, sc, tag=None):
    """a scenario through the Grid object against the restatement, the image included"""
    got, want = OC.run_device(G, sc), OC.run_ref(sc)
    OC.same(got, want, tag or sc.name)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a["stats"] == b["stats"]
        f = sc.frames[k]
        differ("%s, frame %d" % (tag or sc.name, k), "the image", a["image"], OR.overlay(a["class_image"], b["flags"], f.off, b["ids"], b["ids_off"], b["tracks"]))
    return got


# ---- the objects on planes -------------------------------------------------------------------------------------------------------
CASES = [(dict(), (0, 0)), (dict(min_size=2, max_size=9, min_height=0.5), (5, -7)), (dict(min_size=3, max_size=3), (-(2 ** 20 - 8192), 2 ** 20 - 8192)),
         (dict(max_size=2 ** 26, min_height=1.0), (0, 0))]


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_random_fields(G, nx, nz):
    rng = np.random.default_rng(1000 * nx + nz)
    for c, (kw, off) in enumerate(CASES):
        for density in (0.05, 0.3, 0.6):
            planes(G, random_frame(rng, nx, nz, density, off), "%d x %d, case %d, density %.2f" % (nx, nz, c, density), **kw)


def test_components_across_tile_edges_and_corners(G):
    T = G.FRONT_TILE
    nx, nz = 3 * T, 2 * T + 8
    m = np.zeros((nz, nx), bool)
    m[3, T - 2:T + 2] = True                                      # across a vertical edge
    m[T - 2:T + 2, 5] = True                                      # across a horizontal edge
    for k in range(-3, 4):                                        # a diagonal through a tile corner, both ways
        m[T + k, 2 * T + k] = True
    m[2 * T - 1, T - 1], m[2 * T, T] = True, True                 # two cells that touch by the corner where four tiles meet
    m[2 * T, T - 1 - 2], m[2 * T - 1, T - 2 - 2] = True, True     # ... and an anti-diagonal pair beside it
    m[nz - 1, :] = True                                           # the whole last row, ragged tiles included
    f = OC.Frame.of_mask(m, off=(7, -3), height=0.75, count=2)
    flags, label, recs, stats = planes(G, f, "edges and corners")
    assert stats[1] == 6 and label[T + 3, 2 * T + 3] == (T - 3) * nx + 2 * T - 3 and label[2 * T, T] == (2 * T - 1) * nx + T - 1
    planes(G, f, "edges and corners, size bounds", min_size=3, max_size=7)


def test_a_serpentine_across_tile_borders(G):
    T = G.FRONT_TILE
    nx, nz = 3 * T, 2 * T + 8
    m = np.zeros((nz, nx), bool)
    for row in range(0, nz, 2):                                   # one cell wide: rows joined at alternating ends
        m[row, :] = True
        if row + 1 < nz:
            m[row + 1, nx - 1 if (row // 2) % 2 == 0 else 0] = True
    f = OC.Frame.of_mask(m)
    flags, label, recs, stats = planes(G, f, "serpentine", max_size=2 ** 26)
    assert stats[:4] == (int(m.sum()), 1, 1, int(m.sum())) and (label[m] == 0).all()
    assert planes(G, f, "serpentine, large", max_size=100)[3][2:6] == (0, 0, 1, 0)


def test_an_empty_window_and_one_without_a_kept_component(G):
    for nx, nz in WINDOWS:
        got = planes(G, OC.Frame(nx, nz), "empty %d x %d" % (nx, nz))
        assert got[3][:6] == (0,) * 6 and len(got[2]) == 0 and (got[1] == -1).all()
    rng = np.random.default_rng(5)
    f = random_frame(rng, 48, 40, 0.05)
    got = planes(G, f, "none kept", min_size=40, max_size=41)
    assert got[3][0] > 0 and got[3][2:4] == (0, 0) and len(got[2]) == 0
    got = planes(G, f, "all low", min_height=100.0)
    assert got[3][2] == 0 and got[3][5] == got[3][1] > 0


def test_the_hand_cases_on_the_device(G):
    import test_grid_obj as TO
    f = OC.Frame(8, 6, TO.L_CELLS, off=(100, -50))
    assert planes(G, f)[2].tolist() == [[10, 5, 102, -49, 104, -47, 1649, -767, 0x3FA00000, 25]]
    for counts, want in (([2 ** 30, 2 ** 30 - 2, 0, 0, 0], 2 ** 31 - 2), ([2 ** 30, 2 ** 30, 0, 0, 0], 2 ** 31 - 1), ([2 ** 31 - 1] * 5, 2 ** 31 - 1)):
        g = OC.Frame(8, 6, [(a, b, h, c) for (a, b, h, _), c in zip(TO.L_CELLS, counts)])
        assert planes(G, g)[2][0, 9] == want, counts
    above = float(np.nextafter(F(1.25), F(2)))
    for kw, want in ((dict(min_size=5, max_size=5), (1, 5, 0, 0)), (dict(min_size=6, max_size=6), (0, 0, 0, 0)), (dict(max_size=4), (0, 0, 1, 0)),
                     (dict(min_height=1.25), (1, 5, 0, 0)), (dict(min_height=above), (0, 0, 0, 1))):
        assert planes(G, OC.Frame(8, 6, TO.L_CELLS), **kw)[3][2:6] == want, kw


def test_a_solid_block_of_forty_by_forty(G):
    """every wave inside the block is of one component and of one (object, track) pair: the combine before the atomics"""
    f = OC.Frame(48, 48).block(3, 5, 40, 40, height=1.0, count=7)
    assert planes(G, f, "solid block")[2].tolist() == [[5 * 48 + 3, 1600, 3, 5, 42, 44, 16 * 23, 16 * 25, 0x3F800000, 11200]]
    sc = OC.Scenario("solid block", [OC.Frame(48, 48).block(3 + k, 5, 40, 40) for k in range(3)], max_size=4096, gate=0)
    got = play(G, sc)
    assert [r["tracks"][0, OR.T["overlap"]] for r in got] == [0, 1560, 1560] and got[2]["tracks"][0, OR.T["v16_a"]] == 16


# ---- the steps through the object ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(OC.SCENARIOS)))
def test_the_scenarios_on_the_device(G, k):
    play(G, OC.SCENARIOS[k]())


def test_the_smoothed_velocity_on_the_device(G):
    sc = OC.Scenario("smooth", [OC.Frame(30, 3).block(a, 0, 5, 3) for a in (2, 3, 7)], smooth_shift=1, gate=0)
    assert [r["tracks"][0, OR.T["v16_a"]] for r in play(G, sc)] == [0, 16, 40]


@pytest.mark.parametrize("seed", range(8))
def test_random_histories_on_the_device(G, seed):
    nx, nz = WINDOWS[seed % 3]
    # heights that are exact in fp32 as 1.5 - y: the quarters random_history draws
    play(G, OC.random_history(100 + seed, nx, nz, steps=5, density=0.08 if seed < 4 else 0.25))


def test_two_thousand_one_cell_objects(G):
    """2048 objects and as many tracks: the table of pairs probes, the claims, the gate's loop over 2048 tracks and the update's scans run
    over more than one chunk of 1024"""
    nx, nz = 128, 64
    lattice = np.zeros((nz, nx), bool)
    lattice[::2, ::2] = True
    shifted = np.roll(lattice, 1, axis=1)
    frames = [OC.Frame.of_mask(lattice), OC.Frame.of_mask(lattice), OC.Frame.of_mask(shifted), OC.Frame.of_mask(shifted[:, ::-1] & (np.arange(nx) % 3 != 0))]
    got = play(G, OC.Scenario("lattice", frames, max_tracks=4096, gate=1, max_missed=0))
    assert len(got[0]["tracks"]) == 2048 and got[0]["tstats"][4] == 2048 and got[1]["tstats"][2] == 2048
    assert got[2]["tstats"][3] > 0 and got[2]["tstats"][4] > 0                # by the gate and new: the picks are mutual for some only
    got = play(G, OC.Scenario("lattice, a full table", frames[:2], max_tracks=1500, gate=0))
    assert got[0]["tstats"][7] == 548 and (got[1]["assign"][1500:] == OR.UNTRACKED).all() and got[1]["tstats"][2] == 1500


def test_a_checkerboard_is_one_component(G):
    board = (np.add.outer(np.arange(64), np.arange(64)) % 2) == 0
    flags, label, recs, stats = planes(G, OC.Frame.of_mask(board), "checkerboard", max_size=2 ** 26)
    assert stats[:4] == (2048, 1, 1, 2048) and recs[0, :2].tolist() == [0, 2048]
    sc = OC.Scenario("checkerboard", [OC.Frame.of_mask(board), OC.Frame.of_mask(board), OC.Frame.of_mask(~board)], max_size=4096, gate=1)
    got = play(G, sc)
    assert got[1]["tracks"][0, OR.T["overlap"]] == 2048 and got[2]["tstats"][3] == 1          # the other colour: no overlap, the gate


# ---- buffers, the cache, failures ------------------------------------------------------------------------------------------------
def scene(G, nx=48, nz=40, seed=9):
    sc = OC.random_history(seed, nx, nz, steps=3, density=0.2, max_tracks=4096)
    g = G.Grid(G.default_params(**OC.grid_kw(nx, nz)))
    got, want = OC.run_device(G, sc, g), OC.run_ref(sc)
    OC.same(got, want, "scene")
    assert len(want[-1]["recs"]) > 3 and len(want[-1]["tracks"]) > 3
    return g, sc, want[-1]


def test_host_and_device_output_buffers(G, hip):
    g, sc, w = scene(G)
    nx, nz = sc.nx, sc.nz
    for which, name, nbytes in ((G.OBJ_FLAGS, "flags", nx * nz), (G.OBJ_LABEL, "label", 4 * nx * nz)):
        out = Dev(hip, nbytes + 16)
        assert g.obj_plane(which, device_ptr=out.addr) is None
        got = out.get()
        assert got[:nbytes].tobytes() == w[name].tobytes() and (got[nbytes:] == 0xEE).all(), name
    out = Dev(hip, 4 * nx * nz + 16)
    assert g.track_plane(device_ptr=out.addr) == (None, w["ids_off"])
    got = out.get()
    assert got[:4 * nx * nz].tobytes() == w["ids"].tobytes() and (got[4 * nx * nz:] == 0xEE).all()
    out = Dev(hip, 3 * nx * nz + 16)
    img = g.render_objects()
    g.render_objects(device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:3 * nx * nz].reshape(nz, nx, 3), img) and (got[3 * nx * nz:] == 0xEE).all()
    # a cap below the count: the first records, the count of all
    assert np.array_equal(g.objects(cap=2), w["recs"][:2]) and g.object_count == len(w["recs"])
    assert np.array_equal(g.tracks(cap=3), w["tracks"][:3]) and g.track_count == len(w["tracks"])
    assert g.objects(cap=0).shape == (0, 10) and g.tracks(cap=0).shape == (0, 14)
    # refusals change nothing
    L, buf = g._L, np.full(64, 0xAB, np.uint8)
    assert L.svh_grid_get_obj_plane(g._h, 2, buf.ctypes.data, 0) == BAD_ARG and L.svh_grid_get_obj_plane(g._h, G.OBJ_LABEL, out.addr + 2, 1) == BAD_ARG
    assert L.svh_grid_get_track_plane(g._h, out.addr + 2, 1, None) == BAD_ARG and L.svh_grid_get_objects(g._h, None, 1, buf.ctypes.data) == BAD_ARG
    assert L.svh_grid_objects_step(g._h, None, 1, buf.ctypes.data) == BAD_ARG and (buf == 0xAB).all()
    assert np.array_equal(g.tracks(), w["tracks"]) and g.track_stats() == w["tstats"]
    g.close()


def test_a_second_get_launches_nothing(G):
    g, sc, w = scene(G)
    flags = g.obj_plane(G.OBJ_FLAGS)
    G.lib().svh_test_fail_at(b"launch:1:0")                       # nothing changed: no launch, from the cache
    assert g.obj_plane(G.OBJ_FLAGS).tobytes() == flags.tobytes() == w["flags"].tobytes() and g.obj_plane(G.OBJ_LABEL).tobytes() == w["label"].tobytes()
    assert np.array_equal(g.objects(), w["recs"]) and g.object_stats() == w["stats"] + (LAUNCHES,)
    assert np.array_equal(g.tracks(), w["tracks"]) and g.track_plane()[0].tobytes() == w["ids"].tobytes()
    # the mutators of other layers leave the objects where they are
    g.set_goals([(3, 3)])
    g.set_frontier(G.default_front(min_size=2))
    g.set_plan(G.default_plan(neutral=60))
    assert g.obj_plane(G.OBJ_LABEL).tobytes() == w["label"].tobytes()
    G.lib().svh_test_fail_at(None)
    # their own parameters, and the accumulators, do not
    g.set_objects(min_size=2)
    G.lib().svh_test_fail_at(b"launch:1:0")
    with pytest.raises(G.SvhError) as e:
        g.obj_plane(G.OBJ_FLAGS)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR and g.tracks().shape == (0, 14) and g.track_stats() == (0,) * 8
    f = sc.frames[-1]
    p = OR.ObjParams(**dict(sc.kw, min_size=2))
    want = OR.objects(p, f.state, f.hmax, f.count, *f.off)
    assert g.obj_plane(G.OBJ_FLAGS).tobytes() == want[0].tobytes() and np.array_equal(g.objects(), want[2])
    g.close()


@pytest.mark.parametrize("spec", ["launch:1:0", "launch:2:0", "copy:1:0", "wait:1:0", "wait:2:0", "malloc:1:0"])
def test_a_failure_inside_the_objects(G, spec):
    """the accumulated grid is untouched, the objects are computed again by the next call"""
    g, sc, w = scene(G)
    state, hmax = g.local_plane(G.LOCAL_STATE), g.plane(G.HMAX)
    g.set_objects(g.objects_params())                             # the objects are stale and the tracks empty; a larger window for malloc
    G.lib().svh_test_fail_at(spec.encode())
    try:
        g.obj_plane(G.OBJ_LABEL)
        failed = False
    except G.SvhError as e:
        failed = True
        assert e.code == HIP_ERR
    G.lib().svh_test_fail_at(None)
    assert failed or spec.startswith("malloc")                    # every buffer may exist already
    assert g.obj_plane(G.OBJ_LABEL).tobytes() == w["label"].tobytes() and np.array_equal(g.objects(), w["recs"])
    assert g.local_plane(G.LOCAL_STATE).tobytes() == state.tobytes() and g.plane(G.HMAX).tobytes() == hmax.tobytes()
    g.close()


@pytest.mark.parametrize("spec", ["launch:1:0", "copy:1:0", "copy:4:0", "wait:1:0"])
def test_a_failure_inside_a_step_empties_the_tracks(G, spec):
    g, sc, w = scene(G)
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.objects_step()
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR and g.tracks().shape == (0, 14) and g.track_stats() == (0,) * 8 and (g.track_plane()[0] == -1).all()
    assert np.array_equal(g.objects(), w["recs"])
    # the next step starts afresh: every object is new, the ids from 0
    assign = g.objects_step()
    assert assign.tolist() == list(range(len(w["recs"]))) and (g.tracks()[:, 1] & OR.NEW).all()
    g.close()


def test_clear_keeps_the_tracks_and_the_resets_empty_them(G):
    g, sc, w = scene(G)
    g.clear()
    assert np.array_equal(g.tracks(), w["tracks"]) and g.track_stats() == w["tstats"] and g.track_plane()[0].tobytes() == w["ids"].tobytes()
    assert g.objects().shape == (0, 10) and g.object_stats()[:6] == (0,) * 6
    def refill():
        """the first frame's obstacles into the emptied grid, with the window back at its corner"""
        g.clear()
        oa, ob = g.window()
        g.scroll(-oa, -ob)
        pts = OC.frame_points(OC.Frame.of_mask(sc.frames[0].state == 2))
        pts[:, 0] += g.params.x0
        pts[:, 2] += g.params.z0
        g.add_points(pts)

    for reset in (lambda: g.objects_reset(), lambda: g.set_objects(gate=3), lambda: g.set_window(1.0, 2.0)):
        refill()
        g.objects_step()
        g.objects_step()
        assert len(g.tracks()) > 0 and g.track_stats()[0] >= 2                 # the steps go on counting through a clear
        reset()
        assert g.tracks().shape == (0, 14) and g.track_stats() == (0,) * 8 and (g.track_plane()[0] == -1).all()
        refill()                                                               # svh_grid_set_window empties the grid too
        a = g.objects_step()
        assert len(a) and a.tolist() == list(range(len(a))) and (g.tracks()[:, 1] == OR.NEW).all()      # the ids start again at 0
    bad = g.objects_params().copy(max_tracks=0)
    n = len(g.tracks())
    assert g._L.svh_grid_set_objects(g._h, C.byref(bad)) == BAD_ARG and len(g.tracks()) == n > 0      # a refusal changes nothing
    g.close()


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------------
def test_pipeline_grid_objects(G, tmp_path, monkeypatch, capsys):
    """--grid-objects DIR with --grid-local and --grid-dynamic on the two golden frames: per frame a step after the local step; the
    track table and the image are the restatement's on the planes the local grid holds after the same steps"""
    import json
    import os
    import sys
    import helpers as H
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify
    from svhip import kitti
    from test_grid_gpu import read_ppm
    from test_view_gpu import two_frame_drive
    drive = str(two_frame_drive(tmp_path / "drive"))
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(test_rectify.rig_calib_text())
    d, e, o = str(tmp_path / "loc"), str(tmp_path / "dyn"), str(tmp_path / "obj")
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-dynamic", e, "--grid-objects", o, "--grid-objects-params",
                                      "2,300,0.4,3,1", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)])
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("objects: size 2..300, height 0.4 m, gate 3 cells, 1 misses:") and "after 2 steps" in l for l in out), out
    assert sorted(os.listdir(o)) == ["objects_%06d.ppm" % k for k in range(2)] + ["tracks.jsonl"]
    lines = [json.loads(l) for l in open(os.path.join(o, "tracks.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    p.enable_grid_local(0.25, (96, 160))
    p.enable_grid_dynamic()
    prm, trk, k = OR.ObjParams(min_size=2, max_size=300, min_height=0.4, gate=3, max_missed=1), OR.Tracker(), 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        p.local_step()
        g = p.local
        flags, label, recs, _ = OR.objects(prm, g.local_plane(G.LOCAL_STATE), g.plane(G.HMAX), g.plane(G.COUNT), *g.window())
        trk.step(prm, recs, label, g.window())
        assert lines[k] == dict(frame=k, window=list(g.window()), stats=list(trk.track_stats()), tracks=trk.tracks.tolist()), k
        want = OR.overlay(g.render(G.RENDER_CLASS), flags, g.window(), trk.ids, trk.off, trk.tracks)
        assert np.array_equal(read_ppm(os.path.join(o, "objects_%06d.ppm" % k)), want), k
        k += 1
    assert k == 2 and len(trk.tracks) > 0 and trk.track_stats()[0] == 2
