"""GPU: the time layer of the ground grid on the device (include/svh_grid_time.h, "TIME"; stereo-vision_amd/csrc/grid_time_kernels.hip)
against the header stereo-vision_amd/csrc/grid_time_core.h, byte for byte: TPOT, TDIR, RCOST, RPOT, RDIR, the statistics, the path, the
image.  First the kernels on a caller's planes (svh_test_grid_time_device against svh_test_grid_time, and against the restatement
tests/grid_time_ref.py where the window is small enough for plain Python) at the sizes where they can go wrong -- windows round a
tile of S cells and round the planner's tiles, one layer and layer counts round the chunks of K, one slot and 32 with bit 31, slots that
clamp before the last layer, objects that move a cell per layer across, along and through the corner of a tile, blocks on the window's
edge, an ID frame scrolled against the window on both sides of global 0, goals on corners and outside, the three kinds of wait --,
then the object: frames of tests/grid_pred_cases.py played on it, a step each, and everything it reports compared with the header
on the object's own COST, FLAGS, tracks and PRED (tests/grid_time_cases.py).  tests/test_grid_time.py pins the restatement by hand."""
import ctypes as C

import numpy as np
import pytest

import grid_pred_cases as PC
import grid_pred_ref as PR
import grid_time_cases as TC
import grid_time_ref as TM
import helpers as H   # puts the package on the path

pytestmark = pytest.mark.gpu
FAR = TM.FAR
HIP_ERR = -2
POINT = dict(front=0.0, rear=0.0, half_width=0.0, headings_m=1)


@pytest.fixture(scope="module")
def G():
    import svhip
    from svhip import grid
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    grid._bind()
    return grid


S, K = 32, 8          # the tile and the layers of a chunk of k_grid_time_sweep (csrc/grid_internal.h); pinned below


@pytest.fixture(autouse=True)
def restore(G):
    """the shapes below are derived from S and K: they must be the library's"""
    k = C.c_int32(0)
    assert (G.lib().svh_test_grid_time_tile(C.byref(k)), k.value) == (S, K)
    yield
    G.lib().svh_test_fail_at(None)


def same(G, c, tag="", restate=False):
    """the kernels against the header on one case (and against the restatement when asked); returns the header's answer"""
    dev, core = TC.got(G, G.device_time, c), TC.got(G, G.core_time, c)
    for name in ("rcost", "rpot", "rdir", "tpot", "tdir"):
        assert dev[name].dtype == core[name].dtype and np.array_equal(dev[name], core[name]), (tag, name, np.argwhere(dev[name] != core[name])[:4])
    assert dev["stats"][:5] == core["stats"][:5], (tag, dev["stats"], core["stats"])
    if c.start is not None:
        assert (dev["status"], dev["cost"], dev["path_len"]) == (core["status"], core["cost"], core["path_len"]), (tag, dev["status"], core["status"])
        assert np.array_equal(dev["path"], core["path"]), (tag, dev["path"][:6], core["path"][:6])
    if restate:
        TC.agree(G, G.device_time, c, tag)
    return core


# ---- the kernels on a caller's planes ----------------------------------------------------------------------------------------------
WINDOWS = [(1, 1), (1, 17), (15, 17), (S - 1, S - 1), (S, S), (S + 1, S + 1), (2 * S + 1, S + 2), (257, 129)]


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_windows_round_a_workgroup_and_the_tiles(G, nx, nz):
    for k, L in enumerate((1, 2, K, K + 1)):
        c = TC.random_case(1000 * nx + L, nx, nz, L, slots=32 if k % 2 else 8, wait=(100, -1, 1, 65535)[k], max_cost=0x7FFFFFFE if k < 3 else 400000)
        w = same(G, c, "%d x %d, L = %d" % (nx, nz, L), restate=nx * nz <= 600)
        assert w["stats"][0] == L and (nx * nz < 200 or w["stats"][2] > 0)


@pytest.mark.parametrize("L", [1, 2, K, K + 1, 2 * K, 2 * K + 1])
def test_layer_counts(G, L):
    c = TC.random_case(40 + L, 40, 21, L, share=0.25)
    w = same(G, c, "L = %d" % L, restate=True)
    assert w["stats"][2] > 0 and (L < 8 or w["stats"][3] > 0)


@pytest.mark.parametrize("kw", [dict(slots=1), dict(slots=32), dict(slots=32, stride=1, pps=1, L=40), dict(slots=3, stride=2, pps=2, L=20),
                                dict(slots=4, stride=64, pps=1024, L=12)])
def test_slots_one_and_thirty_two_and_slots_that_clamp_before_the_last_layer(G, kw):
    kw = dict(dict(L=10), **kw)
    c = TC.random_case(7 + kw["slots"], 35, 19, share=0.3, **kw)
    if kw["slots"] == 32:
        c.pred[::3, ::2] |= np.uint32(1 << 31)
        assert TM.slot_of_layer(PR.PredParams(**c.pp), kw["L"] - 1) == min(31, kw["L"] - 1)
    w = same(G, c, str(kw), restate=True)
    assert w["stats"][2] > 0


def mover(nx, nz, cells_of_layer, L, **kw):
    """an open field with an object of one cell (and a margin of one) that is on cells_of_layer(t) at layer t; the slot of layer t is t"""
    pred = np.zeros((nz, nx), np.uint32)
    for t in range(min(L, 32)):
        a, b = cells_of_layer(t)
        pred[max(0, b - 1):max(0, b + 2), max(0, a - 1):max(0, a + 2)] |= np.uint32(1 << t)
    return TC.Case(np.zeros((nz, nx), np.uint8), kw.pop("goals"), pred, pp=dict(slots=32), tp=dict(layers=L, **kw.pop("tp", {})), **kw)


def test_objects_that_move_a_cell_per_layer_across_along_and_through_the_corner_of_a_tile(G):
    """64 x 40: the tiles of the sweep meet at column 31 | 32 and row 31 | 32, and its chunks of K layers at the layers L - 1 - K and
    L - 1 - 2 K.  The objects carry a margin of one cell, so they lie on both sides of a
    border they touch.  The vehicle drives towards the object, or across its way"""
    nx, nz, L = 64, 40, 24
    scenes = {"across": (lambda t: (44 - t, 6), dict(goals=[(60, 6)], start=(24, 6))),        # head on, over the tiles' border at layer 12
              "along": (lambda t: (S, t - 4), dict(goals=[(60, 8)], start=(20, 8))),           # up the border between two tiles
              "corner": (lambda t: (S + 8 - t, S + 8 - t), dict(goals=[(40, 39)], start=(24, 24))),   # through the corner of four tiles
              "wrap": (lambda t: (t % 3, 7), dict(goals=[(0, 15)], start=(0, 0)))}               # on the window's edge, next to the index wrap
    for name, (f, kw) in scenes.items():
        w = same(G, mover(nx, nz, f, L, **kw), name, restate=name != "corner")
        static = same(G, mover(nx, nz, lambda t: (-9, -9), L, **kw), name + ", no object")
        assert w["status"] == TM.FOUND and w["cost"] >= static["cost"], name
        assert name == "wrap" or w["cost"] > static["cost"], name                                # the object is in the way: it costs a wait or a detour
    for wait in (-1, 1, 65535):
        w = same(G, mover(nx, nz, scenes["across"][0], L, tp=dict(wait=wait), **scenes["across"][1]), "wait %d" % wait)
        waits = bool((w["tdir"] == TM.DIR_WAIT).any())
        if wait == -1:
            assert not waits                          # there is no wait move
        elif wait == 1:
            assert waits                              # standing still is all but free: somewhere it beats every step
        else:
            assert w["cost"] < 65535                  # the dearest wait: the path from the start goes round instead


def test_blocks_on_the_edge_cells_goals_on_corners_and_outside(G):
    nx, nz = 48, 33
    pred = np.zeros((nz, nx), np.uint32)
    pred[0, :], pred[-1, :], pred[:, 0], pred[:, -1] = 0x0F, 0xF0, 0x3C, 0xC3
    goals = [(0, 0), (nx - 1, 0), (0, nz - 1), (nx - 1, nz - 1), (15, 15), (16, 16), (-1, 5), (nx, 5), (5, nz), (5, -1), (2 ** 20 - 1, -(2 ** 20 - 1))]
    for off in ((0, 0), (-20, -9)):
        g2 = [(a + off[0], b + off[1]) for a, b in goals[:10]] + goals[10:]
        c = TC.Case(TC.random_cost(np.random.default_rng(3), nx, nz, lethal=0.03), g2, pred, tp=dict(layers=10), off=off, start=(24, 1))
        w = same(G, c, "edges %s" % (off,), restate=True)
        assert (w["tpot"][0, 0, 0], w["tpot"][4, 0, 0]) == (0, FAR) or c.cost[0, 0] > 252    # a goal in the corner, blocked at the layers 2 .. 5


@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-40, 25), (47, 0), (0, -33)])
def test_an_id_frame_scrolled_against_the_window_on_both_sides_of_zero(G, shift):
    """the window spans global 0 on both axes; the ID frame lies `shift` cells from it (the last two: it only touches the window)"""
    off = (-20, -15)
    c = TC.random_case(77, 48, 33, 9, off=off, pred_off=(off[0] + shift[0], off[1] + shift[1]), release=1, with_tracks=True, share=0.3)
    w = same(G, c, "shift %s" % (shift,), restate=True)
    if abs(shift[0]) < 40 and abs(shift[1]) < 30:
        assert w["stats"][4] > 0 and w["stats"][2] > 0
    if abs(shift[1]) >= 33:
        assert w["stats"][4] == 0 and w["stats"][2] == 0 and np.array_equal(w["tpot"][0], w["rpot"])


def test_release_on_a_window_of_many_workgroups(G):
    c = TC.random_case(9, 257, 129, 5, release=1, with_tracks=True)
    w = same(G, c, "release, 257 x 129")
    assert w["stats"][4] > 0 and not np.array_equal(w["rcost"], c.cost)
    c.tp["release"] = 0
    assert np.array_equal(same(G, c, "no release")["rcost"], c.cost)


# ---- the object --------------------------------------------------------------------------------------------------------------------
def crossing(G, release, steps=4, off=(0, 0), **pred):
    """48 x 40, bare: a 2 x 2 block crosses from the left along row 20 at a cell per step; the vehicle is to drive up column 16, which
    the block's prediction covers when the vehicle would be there.  Unknown ground is free for the planner"""
    nx, nz = 48, 40
    g = PC.new_grid(G, nx, nz, roll=POINT, pred=dict(dict(slots=16, margin=1), **pred))
    g.set_plan(unknown=0)
    PC.play(g, PC.moving_block(nx, nz, 4, 20, 2, 2, 1, 0, steps=steps, off=off))
    goals = [(16 + off[0], 30 + off[1])]
    g.set_goals(goals)
    g.set_time(layers=24, wait=100, release=release)
    return g, goals, PC.centre(16 + off[0], 10 + off[1])


@pytest.mark.parametrize("release", [0, 1])
def test_the_entries_on_a_crossing_object(G, release):
    g, goals, start = crossing(G, release)
    w, c = TC.check_object(G, g, goals, start, "crossing", image_layers=(0, 12))
    assert w["status"] == TM.FOUND and w["stats"][2] > 0 and w["stats"][4] == (4 if release else 0)
    assert (g.tracks()[:, PR.T["flags"]] & PR.OR.MOVING).all()
    static = g.plan_plane(G.PLAN_POT)
    assert np.array_equal(w["rpot"], static) == (release == 0) and w["cost"] > w["rpot"][10, 16]    # the block is in the way
    # the path meets no object at its own slots: a point footprint reads PRED at the path's cells
    pp = PR.PredParams(**g.get_predict().asdict())
    masks = g.footprint_pred(np.concatenate([w["path"][:, :2], np.zeros((len(w["path"]), 1), np.int32)], 1))
    for (ga, gb, t), m in zip(w["path"], masks):
        assert not (int(m) >> TM.slot_of_layer(pp, int(t))) & 1, (ga, gb, t)
    # a step makes the field stale: the block moves on, and the answer is that of the header on the new tracks
    PC.play(g, PC.moving_block(48, 40, 8, 20, 2, 2, 1, 0, steps=1))
    g.set_goals(goals)
    TC.check_object(G, g, goals, start, "one step later")
    g.close()


def test_a_scroll_between_the_step_and_the_query_on_both_sides_of_zero(G):
    off = (-20, -25)
    g, goals, start = crossing(G, 1, off=off)
    TC.check_object(G, g, goals, start, "before the scroll")
    for d in ((3, -2), (-7, 4)):
        g.scroll(*d)
        w, c = TC.check_object(G, g, goals, start, "scrolled by %s" % (d,), image_layers=(3,))
        assert c.off != c.pred_off and w["stats"][2] > 0
    g.close()


def test_one_slot_and_thirty_two_on_the_object(G):
    for pred in (dict(slots=1), dict(slots=32, stride=1), dict(slots=4, stride=2, poses_per_step=3)):
        g, goals, start = crossing(G, 1, **pred)
        TC.check_object(G, g, goals, start, str(pred))
        g.close()


def test_the_layer_is_off_until_it_is_set_and_refuses_what_it_must(G):
    g = PC.new_grid(G, 20, 12, pred=dict())
    buf = np.zeros(3 * 20 * 12, np.int32)
    for call in (lambda: g.time_plane(G.TIME_TPOT, 0, 1), g.time_stats, lambda: g.time_path(PC.centre(3, 3)), lambda: g.render_time(0)):
        with pytest.raises(G.SvhError) as e:
            call()
        assert e.value.code == -1 and "svh_grid_set_time" in str(e.value)
    assert g.time_params().asdict() == dict(layers=32, wait=100, release=1)
    with pytest.raises(G.SvhError):
        g.set_time(layers=0)
    g.set_time(layers=4)
    g.set_plan(unknown=0)
    g.set_goals([(5, 5)])
    for t0, count in ((-1, 1), (0, 0), (0, 5), (4, 1), (3, 2)):
        assert G.lib().svh_grid_get_time_plane(g._h, G.TIME_TPOT, t0, count, buf.ctypes.data, 0) == -1 and not buf.any()
    assert G.lib().svh_grid_get_time_plane(g._h, G.TIME_RCOST, 1, 1, buf.ctypes.data, 0) == -1
    assert G.lib().svh_grid_get_time_plane(g._h, 4, 0, 1, buf.ctypes.data, 0) == -1
    assert G.lib().svh_grid_render_time(g._h, 4, None, 0, buf.ctypes.data, 0) == -1 and not buf.any()
    # before the first step PRED is all 0: every layer is the planner's field
    pot, dir_ = g.plan_plane(G.PLAN_POT), g.plan_plane(G.PLAN_DIR)
    assert (pot != FAR).sum() > 100
    for t in range(4):
        assert np.array_equal(g.time_plane(G.TIME_TPOT, t, 1)[0], pot) and np.array_equal(g.time_plane(G.TIME_TDIR, t, 1)[0], dir_)
    assert g.time_path(PC.centre(-3, 3))[0] == G.PATH_OUTSIDE
    g.close()


# ---- failures ----------------------------------------------------------------------------------------------------------------------
def snapshot(G, g):
    return (g.count().tobytes(), g.classes().tobytes(), g.tracks().tobytes(), g.track_plane()[0].tobytes(), g.trav_plane(G.TRAV_COST).tobytes(),
            g.plan_plane(G.PLAN_POT).tobytes(), g.pred_plane()[0].tobytes(), g.object_stats(), g.track_stats())


# the least number of sites of each kind an entry has on a new object whose cost planes, planner's field, objects and PRED are cached,
# from the engine's text.  The planes: the field, the control words and their pinned copy, the static planes, their tile lists, control
# words and pinned copy; the fills of the control words, the count's readback, the planner's fills and readbacks, the statistics'
# readback, the plane's copy; the release, the distance passes, the seed, a batch of rounds, DIR, the sweep; the waits of the count,
# of a batch, of the planner's last readback, of the sweep and of the plane's copy.  The path on a cached field: the triples and (the
# three words exist by then or not) the walk; the words' readback and the triples' copy, a wait each.  The image: the triples' upload
# and the image's copy with their waits, one check of its launches
LEAST = {"plane": dict(malloc=6, copy=8, launch=6, wait=5), "stats": dict(malloc=6, copy=7, launch=6, wait=4), "path": dict(malloc=1, copy=2, launch=1, wait=2),
         "render": dict(malloc=0, copy=2, launch=1, wait=2)}


@pytest.mark.parametrize("kind", ["malloc", "copy", "launch", "wait"])
@pytest.mark.parametrize("entry", ["plane", "stats", "path", "render"])
def test_an_error_at_every_site_leaves_the_grid_the_tracks_and_the_other_layers(G, entry, kind):
    """the n-th allocation, copy (fills included), launch check or wait of the entry fails through the host-side hook, for n = 1, 2, ...
    until the entry succeeds with the hook still armed: every site of that kind is hit.  Each n gets a new object -- a buffer that one
    attempt allocated would not be allocated by the next.  After the failure the grid, the tracks and the other layers are as they
    were and the same call is right.  No device fault is provoked: the hook returns an error instead of making the call"""
    hits = 0
    for n in range(1, 120):
        g, goals, start = crossing(G, 1, steps=3)
        before = snapshot(G, g)
        if entry in ("path", "render"):
            g.time_plane(G.TIME_TPOT)
        call = {"plane": lambda: g.time_plane(G.TIME_TPOT), "stats": g.time_stats, "path": lambda: g.time_path(start),
                "render": lambda: g.render_time(2, [(16, 10, 0), (16, 11, 1)])}[entry]
        G.lib().svh_test_fail_at(("%s:%d" % (kind, n)).encode())
        try:
            call()
            failed = False
        except G.SvhError as e:
            assert e.code == HIP_ERR, (entry, kind, n, e.code)
            failed = True
        G.lib().svh_test_fail_at(None)
        assert snapshot(G, g) == before, (entry, kind, n)
        TC.check_object(G, g, goals, start, "%s, %s:%d: the call repeated" % (entry, kind, n), image_layers=(2,) if entry == "render" else ())
        g.close()
        if not failed:
            break
        hits += 1
    else:
        raise AssertionError("%s still fails at %s:%d" % (entry, kind, n))
    print("%s: %d sites of kind %s" % (entry, hits, kind))
    assert hits >= LEAST[entry][kind], (entry, kind, hits)


# ---- the pipeline tool -------------------------------------------------------------------------------------------------------------
def test_pipeline_grid_time(G, tmp_path, monkeypatch, capsys):
    """--grid-time DIR with --grid-objects and --grid-predict on the two golden frames: two images (the layers 0 and L / 2) and one line
    of time.jsonl per frame.  Two frames make no MOVING track, so nothing predicts and nothing is released: a path that is found is
    the planner's, entry for entry, with the layer beside each cell, and it does not wait"""
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify
    from test_grid_gpu import read_ppm
    from test_view_gpu import two_frame_drive
    drive = str(two_frame_drive(tmp_path / "drive"))
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(test_rectify.rig_calib_text())
    d, d2, d3, d4, d5, d6, d7 = (str(tmp_path / n) for n in ("loc", "cost", "plan", "roll", "obj", "pred", "time"))
    common = ["--grid-slope", "2.0", "--grid-inscribed", "0.1", "--grid-inflate", "0.5", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-plan", d3, "--grid-roll", d4,
                                      "--grid-roll-vehicle", "0,0,0", "--grid-roll-unknown", "0", "--grid-objects", d5, "--grid-objects-params",
                                      "2,300,0.4,3,1", "--grid-predict", d6, "--grid-time", d7, "--grid-time-params", "12,70,1"] + common)
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("time layer: 12 layers, wait 70, release 1: a path in ") and "4 images and time.jsonl" in l for l in out), out[-8:]
    assert sorted(os.listdir(d7)) == ["time.jsonl"] + ["time_%06d_t%03d.ppm" % (k, t) for k in range(2) for t in (0, 6)]
    lines = [json.loads(l) for l in open(os.path.join(d7, "time.jsonl"))]
    plans = [json.loads(l) for l in open(os.path.join(d3, "plan.jsonl"))]
    assert [l["frame"] for l in lines] == [0, 1]
    for l, pl in zip(lines, plans):
        assert set(l) == {"frame", "status", "length", "cost", "waits", "triples", "time_stats"}
        assert (l["status"], l["cost"]) == (pl["status"], pl["cost"]) and l["waits"] == 0 and l["time_stats"][0] == 12 and l["time_stats"][4] == 0
        if l["status"] == 0:
            assert l["length"] == pl["length"] == len(l["triples"]) and [t[2] for t in l["triples"]] == [min(k, 11) for k in range(l["length"])]
    assert read_ppm(os.path.join(d7, "time_%06d_t%03d.ppm" % (1, 6))).shape == (160, 96, 3)
