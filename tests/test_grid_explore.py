"""CPU: the contract of the ground grid's exploration layer (include/svh_grid.h, "EXPLORATION": svh_grid_set_explore,
svh_grid_view_gain, svh_grid_view_mask, svh_grid_explore_rank, svh_grid_plan_set_goal_explore, svh_grid_render_view).
tests/grid_explore_ref.py restates stereo-vision_amd/csrc/grid_explore_core.h in numpy and plain Python; this file pins the
restatement with cases derived by hand, compares the header itself with it -- evaluated on the host by the library's test
entry svh_test_grid_explore (core_explore), and once more as a program of its own under the address and undefined-behaviour
sanitizers --, and checks what needs no device: the refusals, the exports, the C99 header.

tests/test_grid_explore_gpu.py compares the device with the same restatement.

Planes are indexed [ib, ia]; a cell is (a, b) = (ia, ib).  Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_explore_ref as ER
import grid_front_ref as FR
import grid_plan_ref as PR
import helpers as H
import test_grid_front as TF

U, S, F, O, D = TF.U, TF.S, TF.F, TF.O, TF.D
INF = ER.INFEASIBLE


@pytest.fixture(scope="module")
def G():
    from svhip import grid
    grid._bind()
    return grid


def agree(G, state, R, cost=None, cells=None, view=None, start=None, oa=0, ob=0, front=None, plan=None, tag="", **kw):
    """the restatement and the header on the same planes: GAIN of `cells`, the VIEW plane of `view`, the ranking from `start`
    (all global cells); returns the header's dict"""
    state = np.asarray(state, np.uint8)
    cost = np.zeros(state.shape, np.uint8) if cost is None else np.asarray(cost, np.uint8)
    front, plan = front or {}, plan or {}
    fr, pr, er = FR.FrontParams(**front), PR.PlanParams(**plan), ER.ExploreParams(range=float(R), **kw)
    assert ER.range_cells(er.range, 1.0) == R
    got = G.core_explore(G.default_explore(range=float(R), **kw), 1.0, state, cost, G.default_front(**front), G.default_plan(**plan), oa, ob, cells, view,
                         None, start)
    if cells is not None:
        want = ER.gains(fr, R, state, cells, oa, ob)
        assert got["gains"].dtype == np.int32 and np.array_equal(got["gains"], want), (tag, got["gains"], want)
    if view is not None:
        mask, gain = ER.view(fr, R, state, view[0] - oa, view[1] - ob)
        assert np.array_equal(got["mask"], mask), (tag, np.argwhere(got["mask"] != mask)[:4])
        assert gain == ER.gains(fr, R, state, [view], oa, ob)[0] == (mask == 2).sum()
    if start is not None:
        recs, scores, best, feasible = ER.rank(fr, pr, er, R, state, cost, start, oa, ob)
        assert got["recs"].shape == recs.shape and np.array_equal(got["recs"], recs), (tag, got["recs"][:4], recs[:4])
        assert np.array_equal(got["scores"], scores) and got["best"] == best and got["stats"] == (len(recs), feasible), (tag, got["best"], best)
    return got


# ---- by hand -------------------------------------------------------------------------------------------------------------
def test_five_by_five_from_the_centre_and_from_a_corner(G):
    state = np.full((5, 5), U, np.uint8)
    state[2, 2] = F
    got = agree(G, state, 2, cells=[(2, 2)], view=(2, 2))
    # the disc 0 < x^2 + z^2 <= 4: the axes out to 2 and the four diagonal neighbours
    assert got["gains"].tolist() == [12]
    assert got["mask"].tolist() == [[0, 0, 2, 0, 0], [0, 2, 2, 2, 0], [2, 2, 0, 2, 2], [0, 2, 2, 2, 0], [0, 0, 2, 0, 0]]
    got = agree(G, state, 2, cells=[(0, 0), (4, 4), (5, 4), (-1, 0)], view=(0, 0))
    # the quarter of it that the window keeps: (1, 0), (2, 0), (0, 1), (0, 2), (1, 1); the corner itself is unknown and not counted
    assert got["gains"].tolist() == [5, 5, -1, -1]
    assert got["mask"].tolist() == [[0, 2, 2, 0, 0], [2, 2, 0, 0, 0], [2, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]


def test_an_obstacle_at_ring_one_shadows_its_cone(G):
    """R = 3 from the centre of 7 x 7, an obstacle on (1, 0): the rays to (3, -1), (3, 0) and (3, 1) start with (1, 0) and end there.
    (2, 1) and (2, -1) are still visited by the rays to (3, 2) and (3, -2), which start with (1, 1) and (1, -1): the shadow is
    (2, 0) and (3, 0), and the obstacle itself is not visited: 28 - 3 = 25"""
    state = np.full((7, 7), U, np.uint8)
    state[3, 4] = O
    got = agree(G, state, 3, cells=[(3, 3)], view=(3, 3))
    assert got["gains"].tolist() == [25]
    want = np.array([[0, 0, 0, 2, 0, 0, 0], [0, 2, 2, 2, 2, 2, 0], [0, 2, 2, 2, 2, 2, 0], [2, 2, 2, 0, 0, 0, 0], [0, 2, 2, 2, 2, 2, 0], [0, 2, 2, 2, 2, 2, 0],
                     [0, 0, 0, 2, 0, 0, 0]], np.uint8)
    assert np.array_equal(got["mask"], want)
    state[:] = F                                                     # obstacles on all eight neighbours: nothing is visited
    state[2:5, 2:5] = O
    got = agree(G, state, 3, cells=[(3, 3)], view=(3, 3))
    assert got["gains"].tolist() == [0] and not got["mask"].any()


def test_the_diagonal_squeeze(G):
    """from the corner (0, 0) with obstacles on (1, 0) and (0, 1), R = 2: the rays to (2, 2), (2, 1) and (1, 2) all start with
    (1, 1), which is neither of the two: a diagonal step between two obstacle cells passes.  Their next cells lie beyond R"""
    state = np.full((3, 3), U, np.uint8)
    state[0, 1] = state[1, 0] = O
    got = agree(G, state, 2, cells=[(0, 0)], view=(0, 0))
    assert got["gains"].tolist() == [1] and got["mask"].tolist() == [[0, 0, 0], [0, 2, 0], [0, 0, 0]]
    state[0, 0] = O                                                  # a viewpoint on an obstacle cell casts its rays all the same
    assert agree(G, state, 2, cells=[(0, 0)], view=(0, 0))["gains"].tolist() == [1]


def test_a_row_of_obstacles_with_one_gap(G):
    """7 x 5, the viewpoint (3, 0) on a free row, row 1 obstacles but for a free gap at (3, 1), unknown beyond, R = 3.  Through the gap
    go the ray to (0, 3) -- (0, 1), (0, 2), (0, 3) -- and the rays to (-1, 3) and (1, 3), whose cells are (0, 1), (-1, 2) and (1, 2) and
    then (+-1, 3) beyond R; every other ray that leaves row 0 meets the wall at k = 1 or 2"""
    state = np.full((5, 7), U, np.uint8)
    state[0] = F
    state[1] = O
    state[1, 3] = F
    got = agree(G, state, 3, cells=[(3, 0)], view=(3, 0))
    assert got["gains"].tolist() == [4]
    assert got["mask"].tolist() == [[1, 1, 1, 0, 1, 1, 1], [0, 0, 0, 1, 0, 0, 0], [0, 0, 2, 2, 2, 0, 0], [0, 0, 0, 2, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]]


def test_unseen_against_unknown_seen(G):
    state = np.array([[F, U, S, F, U, S, O, U]], np.uint8)            # the obstacle ends the ray: the last cell is never visited
    for m, mask in ((8, [0, 2, 1, 1, 2, 1, 0, 0]), (16, [0, 1, 2, 1, 1, 2, 0, 0]), (24, [0, 2, 2, 1, 2, 2, 0, 0])):
        got = agree(G, state, 7, cells=[(0, 0)], view=(0, 0), front=dict(unexplored=m))
        assert got["mask"].tolist() == [mask] and got["gains"].tolist() == [mask.count(2)], m
    drop = np.array([[F, D, U | 0x80, F | S]], np.uint8)             # a drop does not block; the overhang bit and the seen bit of a free cell play no part
    assert agree(G, drop, 3, view=(0, 0))["mask"].tolist() == [[0, 1, 2, 1]]


ROW = np.array([[U, F, F, F, F, F, F, F, U]], np.uint8)
ROW_COST = np.array([[255, 0, 0, 0, 0, 0, 0, 0, 255]], np.uint8)


def test_the_score_and_its_ties(G):
    """1 x 9: two frontier cells, (1, 0) and (7, 0), each a component of its own.  From (4, 0) each is three edge steps of
    5 * (50 + 50) away, and with R = 2 each sees one unknown cell: 1 * 1500 - 500 * 1 = 1000 twice, the lower index wins"""
    front = dict(min_size=1)
    got = agree(G, ROW, 2, ROW_COST, start=(4, 0), front=front)
    assert got["recs"].tolist() == [[1, 1, 0, 1, 1500], [7, 7, 0, 1, 1500]] and got["scores"].tolist() == [1000, 1000] and got["best"] == 0
    got = agree(G, ROW, 2, ROW_COST, start=(5, 0), front=front)
    assert got["recs"][:, 4].tolist() == [2000, 1000] and got["scores"].tolist() == [1500, 500] and got["best"] == 1
    got = agree(G, ROW, 2, ROW_COST, start=(5, 0), front=front, w_gain=0, w_reach=0)
    assert got["scores"].tolist() == [0, 0] and got["best"] == 0 and got["stats"] == (2, 2)
    got = agree(G, ROW, 2, ROW_COST, start=(7, 0), front=front, w_gain=0)           # the start is a representative: reach 0
    assert got["recs"][:, 4].tolist() == [3000, 0] and got["best"] == 1
    assert agree(G, ROW, 2, ROW_COST, start=(4, 0), front=front, min_gain=1)["stats"] == (2, 2)
    got = agree(G, ROW, 2, ROW_COST, start=(4, 0), front=front, min_gain=2)         # one above what they see
    assert got["scores"].tolist() == [INF, INF] and got["best"] == -1 and got["stats"] == (2, 0)
    for plan, feasible, best in ((dict(max_cost=1500), 2, 0), (dict(max_cost=1499), 0, -1)):     # the horizon met exactly, and one below
        got = agree(G, ROW, 2, ROW_COST, start=(4, 0), front=front, plan=plan)
        assert got["stats"] == (2, feasible) and got["best"] == best
    for start in ((0, 0), (-3, 0), (4, 1)):                          # an impassable start, two outside the window: no error, every reach FAR
        got = agree(G, ROW, 2, ROW_COST, start=start, front=front)
        assert got["recs"][:, 4].tolist() == [ER.FAR, ER.FAR] and got["best"] == -1 and got["recs"][:, 3].tolist() == [1, 1]
    wall = ROW_COST.copy()
    wall[0, 5] = 254                                                  # the far frontier walled off
    got = agree(G, ROW, 2, wall, start=(4, 0), front=front)
    assert got["recs"][:, 4].tolist() == [1500, ER.FAR] and got["scores"].tolist() == [1000, INF] and got["stats"] == (2, 1)
    got = agree(G, ROW, 2, ROW_COST, start=(4, 0))                   # min_size 8: no kept component
    assert len(got["recs"]) == 0 and got["best"] == -1 and got["stats"] == (0, 0)
    got = agree(G, ROW, 2, ROW_COST, start=(14, -7), oa=10, ob=-7, front=front)     # under offsets the records are global cells
    assert got["recs"].tolist() == [[1, 11, -7, 1, 1500], [7, 17, -7, 1, 1500]]
    assert ER.score(ER.ExploreParams(w_gain=65535, w_reach=65535), 2 ** 26, 0x7FFFFFFE) == 65535 * 0x7FFFFFFE - 65535 * 2 ** 26


def test_the_overlay_colours(G):
    mask = np.array([[0, 1, 2], [2, 0, 1]], np.uint8)
    base = np.arange(18, dtype=np.uint8).reshape(2, 3, 3) * 13
    img = ER.overlay(base, mask, 0, 0)
    assert tuple(img[1, 0]) == (255, 255, 255) and tuple(img[1, 2]) == tuple(img[0, 0]) == (255, 0, 255) and (img[0, 1] == base[0, 1]).all()
    assert tuple(img[1, 1]) == tuple(int(c) + (255 - int(c)) // 2 for c in base[1, 1]) and tuple(img[0, 2]) == tuple(int(c) + (255 - int(c)) // 2 for c in base[0, 2])
    state = np.array([[F, F, U], [U, O, F]], np.uint8)                # the header draws the same over the same image
    m, _ = ER.view(FR.FrontParams(), 2, state, 0, 0)
    got = G.core_explore(G.default_explore(range=2.0), 1.0, state, view=(0, 0), rgb=base)
    assert np.array_equal(got["mask"], m) and np.array_equal(got["image"], ER.overlay(base, m, 0, 0))
    assert (G.VIEW_COLOUR, G.VIEWPOINT_COLOUR) == (ER.VIEW_COLOUR, ER.VIEWPOINT_COLOUR)


# ---- properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 7, 8, 9, 31, 32, 33, 127, 128])
def test_the_open_window_is_a_disc(G, R):
    """without obstacles the visited set is exactly 0 < sx^2 + sz^2 <= R^2, clipped to the window"""
    n = 2 * R + 1
    x, z = np.meshgrid(np.arange(n), np.arange(n))
    rng = np.random.default_rng(R)
    state = rng.choice(np.array([U, S, F, D], np.uint8), (n, n))
    for va, vb in ((R, R), (0, R // 2), (n - 1, n - 1)):
        d2 = (x - va) ** 2 + (z - vb) ** 2
        disc = (d2 > 0) & (d2 <= R * R)
        got = G.core_explore(G.default_explore(range=float(R)), 1.0, state, cells=[(va, vb)], view=(va, vb))
        assert np.array_equal(got["mask"] != 0, disc), (R, va, vb)
        assert got["gains"][0] == (disc & (state == U)).sum() == (got["mask"] == 2).sum()
        mask, gain = ER.view(FR.FrontParams(), R, state, va, vb)
        assert np.array_equal(mask, got["mask"]) and gain == got["gains"][0]
    if R in (1, 2, 3, 8, 32, 128):
        full = G.core_explore(G.default_explore(range=float(R)), 1.0, np.zeros((n, n), np.uint8), cells=[(R, R)])["gains"][0]
        assert full == {1: 4, 2: 12, 3: 28, 8: 196, 32: 3208, 128: 51432}[R]


WINDOWS = [(1, 1), (1, 40), (16, 16), (17, 33), (64, 64), (257, 70)]


def planes(rng, nx, nz, p_free=0.6):
    """random STATE with every class and COST that is lethal on the obstacles and drops, so that reach is about the same scene"""
    state, cost = TF.random_planes(rng, nx, nz, p_free)
    cls = state & 3
    cost = np.where((cls == O) | (cls == D), 254, np.where(cls == U, 255, cost % 200)).astype(np.uint8)
    return state, cost


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_the_header_against_the_restatement_on_random_windows(G, nx, nz):
    rng = np.random.default_rng(100 * nx + nz)
    for k, (R, front, plan, kw, oa, ob) in enumerate([(5, dict(min_size=2), dict(), dict(), 0, 0), (12, dict(min_size=1, unexplored=24, border=1), dict(unknown=30), dict(w_gain=3, min_gain=4), 7, -5),
                                                       (40, dict(min_size=3, unexplored=16), dict(max_cost=30000), dict(w_reach=7, w_gain=65535, min_gain=0), -(2 ** 20 - 8192), 2 ** 20 - 8192)]):
        state, cost = planes(rng, nx, nz, (0.5, 0.7, 0.9)[k])
        cells = np.stack([rng.integers(-2, nx + 2, 12) + oa, rng.integers(-2, nz + 2, 12) + ob], 1)
        view = (int(rng.integers(0, nx)) + oa, int(rng.integers(0, nz)) + ob)
        start = (int(rng.integers(0, nx)) + oa, int(rng.integers(0, nz)) + ob)
        got = agree(G, state, R, cost, cells, view, start, oa, ob, front, plan, "%d x %d, case %d" % (nx, nz, k), **kw)
        pot = PR.field(PR.PlanParams(**plan), cost, [start], oa, ob)[0]              # REACH is the planner's POT with the start as the goal
        for r in got["recs"]:
            assert r[4] == pot[r[2] - ob, r[1] - oa]


# ---- refusals and exports ------------------------------------------------------------------------------------------------
BAD = [dict(range=0.0), dict(range=-1.0), dict(range=float("nan")), dict(range=float("inf")), dict(range=0.99), dict(range=129.0), dict(min_gain=-1),
       dict(min_gain=2 ** 26 + 1), dict(w_gain=-1), dict(w_gain=65536), dict(w_reach=-1), dict(w_reach=65536)]
GOOD = [dict(range=1.0), dict(range=128.99), dict(min_gain=0), dict(min_gain=2 ** 26), dict(w_gain=0), dict(w_gain=65535), dict(w_reach=0), dict(w_reach=65535)]


def test_refusals(G):
    import svhip
    L = G._bind()
    state, cost = np.full((2, 2), F, np.uint8), np.zeros((2, 2), np.uint8)
    cells, view, start = np.zeros((1, 2), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    outside = np.array([2, 0], np.int32)
    gains, mask, recs, scores = np.full(1, 0x55, np.int32), np.full((2, 2), 0x55, np.uint8), np.full((4, 5), 0x55, np.int32), np.full(4, 0x55, np.int64)
    n, best, stats = C.c_int64(-7), C.c_int32(-7), np.full(2, 0x55, np.int64)
    fr, pl = G.default_front(), G.default_plan()

    def call(e, f=fr, p=pl, cell=1.0, nx=2, nz=2, oa=0, ob=0, state_=state, cost_=cost, cells_=cells, n_cells=1, gains_=gains, view_=view, start_=start, cap=4,
             n_=n, best_=best):
        ptr = lambda a: a.ctypes.data if a is not None else None
        ref = lambda s: C.byref(s) if s is not None else None
        return L.svh_test_grid_explore(ref(f), ref(p), ref(e), cell, nx, nz, oa, ob, ptr(state_), ptr(cost_), ptr(cells_), n_cells, ptr(gains_), ptr(view_),
                                       ptr(mask), None, ptr(start_), ptr(recs), ptr(scores), cap, C.addressof(n_) if n_ is not None else None,
                                       C.addressof(best_) if best_ is not None else None, ptr(stats))
    good = G.default_explore()
    assert (good.range, good.min_gain, good.w_gain, good.w_reach) == (10.0, 1, 500, 1) and C.sizeof(G.ExploreParams) == 16
    for kw in BAD:
        assert not (ER.ExploreParams(**kw).ok() and ER.range_cells(kw.get("range", 10.0), 1.0)), kw
        assert call(G.default_explore(**kw)) == svhip.ERR_BAD_ARG and "svh_test_grid_explore" in svhip.last_error(), kw
    for bad in (dict(e=None), dict(f=None), dict(p=None), dict(cell=0.0), dict(cell=0.05), dict(cell=11.0), dict(nx=0), dict(nz=8193), dict(oa=2 ** 20),
                dict(state_=None), dict(cost_=None), dict(cells_=None), dict(gains_=None), dict(n_cells=-1), dict(n_cells=2 ** 26 + 1), dict(view_=outside),
                dict(cap=-1), dict(n_=None), dict(best_=None), dict(f=G.default_front(min_size=0)), dict(p=G.default_plan(neutral=0)),
                dict(start_=np.array([2 ** 20, 0], np.int32))):
        assert call(**dict(dict(e=good), **bad)) == svhip.ERR_BAD_ARG, bad
    assert (gains == 0x55).all() and (mask == 0x55).all() and (recs == 0x55).all() and (scores == 0x55).all() and (stats == 0x55).all()
    assert n.value == -7 and best.value == -7
    for kw in GOOD:
        assert ER.ExploreParams(**kw).ok() and call(G.default_explore(**kw)) == 0, kw
    assert call(good, p=None, cost_=None, start_=None) == 0                              # without a ranking neither is needed
    # the entries refuse a null grid before anything else
    buf = np.full(64, 0xAB, np.uint8)
    xyz = np.zeros(3, np.float64)
    for f in (lambda: L.svh_grid_set_explore(None, C.byref(good)), lambda: L.svh_grid_get_explore(None, C.byref(good), buf.ctypes.data),
              lambda: L.svh_grid_view_gain(None, buf.ctypes.data, 1, 0, buf.ctypes.data), lambda: L.svh_grid_view_mask(None, 0, 0, buf.ctypes.data, 0),
              lambda: L.svh_grid_explore_rank(None, xyz.ctypes.data, buf.ctypes.data, None, 1, buf.ctypes.data, buf.ctypes.data),
              lambda: L.svh_grid_plan_set_goal_explore(None, xyz.ctypes.data), lambda: L.svh_grid_get_explore_stats(None, buf.ctypes.data),
              lambda: L.svh_grid_render_view(None, 0, 0, buf.ctypes.data, 0)):
        assert f() == svhip.ERR_BAD_ARG and "svh_grid" in svhip.last_error()
    L.svh_grid_explore_params_default(None)
    assert (buf == 0xAB).all()


ENTRIES = ("svh_grid_explore_params_default", "svh_grid_set_explore", "svh_grid_get_explore", "svh_grid_view_gain", "svh_grid_view_mask",
           "svh_grid_explore_rank", "svh_grid_plan_set_goal_explore", "svh_grid_get_explore_stats", "svh_grid_render_view")


def test_entries_are_declared_and_exported(G):
    import svhip
    text = open(os.path.join(H.ROOT, "include", "svh_grid.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(svhip.lib(), name), name
    for name in ("svh_test_grid_explore", "svh_test_grid_explore_device"):
        assert hasattr(svhip.lib(), name) and name not in text, name          # test entries: exported, not in the public header
    for name, value in (("SVH_GRID_EXPLORE_RECORD", "5"), ("SVH_GRID_VIEW_NONE", "0"), ("SVH_GRID_VIEW_VISITED", "1"), ("SVH_GRID_VIEW_COUNTED", "2")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), hdr), name
    assert "EXPLORATION" in text
    assert (G.EXPLORE_RECORD, G.EXPLORE_FIELDS, G.EXPLORE_INFEASIBLE) == (5, ER.FIELDS, INF)
    assert (G.VIEW_NONE, G.VIEW_VISITED, G.VIEW_COUNTED) == (ER.NONE, ER.VISITED, ER.COUNTED)
    for m in ("set_explore", "explore_params", "view_gain", "view_mask", "explore_rank", "set_goal_explore", "explore_stats", "render_view"):
        assert callable(getattr(G.Grid, m)), m


def test_header_is_c99(tmp_path):
    exe = str(tmp_path / "grid_explore_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cxx", "grid_explore_c99.c"), "-L", H.PKG, "-lsvhip", "-Wl,-rpath," + H.PKG])
    out = subprocess.check_output([exe]).decode()
    assert "exploration C99 ok, view bytes 0..2, records of 5" in out


# ---- the header once more, as a program of its own under the sanitizers --------------------------------------------------
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_explore")
    exe = str(d / "grid_explore_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.PKG, "csrc"), "-o", exe, os.path.join(H.ROOT, "tests", "cxx", "grid_explore_check.cpp")])

    def run(fr, pr, er, cell, state, cost, cells, view, start, oa=0, ob=0):
        state, cost = np.asarray(state, np.uint8), np.asarray(cost, np.uint8)
        cells = np.asarray(cells, np.int32).reshape(-1, 2)
        nz, nx = state.shape
        head = np.array([nx, nz, oa, ob, fr.max_cell_cost, fr.min_size, fr.unexplored, fr.border, pr.neutral, pr.unknown, pr.max_cost, er.min_gain, er.w_gain,
                         er.w_reach, view[0], view[1], start[0], start[1], len(cells)], np.int64).astype(np.int32)
        job = str(d / "job.bin")
        with open(job, "wb") as f:
            f.write(head.tobytes() + np.array([er.range, cell], np.float32).tobytes() + state.tobytes() + cost.tobytes() + cells.tobytes())
        r = subprocess.run([exe, job], capture_output=True)
        if r.returncode == 3:
            assert not r.stdout and not r.stderr
            return None
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out, at = r.stdout, 4 * len(cells)
        res = dict(gains=np.frombuffer(out[:at], np.int32))
        if 0 <= view[0] - oa < nx and 0 <= view[1] - ob < nz:
            res["mask"] = np.frombuffer(out[at:at + nx * nz], np.uint8).reshape(nz, nx)
            at += nx * nz
        n, best, feasible = (int(v) for v in np.frombuffer(out[at:at + 24], np.int64))
        at += 24
        assert len(out) == at + 28 * n
        res.update(recs=np.frombuffer(out[at:at + 20 * n], np.int32).reshape(-1, 5), scores=np.frombuffer(out[at + 20 * n:], np.int64), best=best, feasible=feasible)
        return res
    return run


SAN_CASES = [(dict(min_size=2), 3.0, 0.5, 33, 9, 0, 0), (dict(min_size=1, border=1), 2.0, 2.0, 1, 40, -5, 9),
             (dict(unexplored=24, min_size=2, border=1), 64.0, 0.5, 40, 1, 2 ** 20 - 8192, -(2 ** 20 - 8192)), (dict(unexplored=16, min_size=3), 9.9, 1.0, 17, 17, 0, 0),
             (dict(border=1, min_size=1), 1.0, 1.0, 1, 1, 0, 0)]


@pytest.mark.parametrize("k", range(len(SAN_CASES)))
def test_the_header_under_the_sanitizers(core, k):
    kw, range_, cell, nx, nz, oa, ob = SAN_CASES[k]
    rng = np.random.default_rng(80 + k)
    fr, pr, er = FR.FrontParams(**kw), PR.PlanParams(unknown=20), ER.ExploreParams(range=range_, min_gain=0)
    R = ER.range_cells(range_, cell)
    assert R == int(range_ / cell)
    state, cost = planes(rng, nx, nz, 0.7)
    cells = [(oa, ob), (oa + nx - 1, ob + nz - 1), (oa + nx // 2, ob + nz // 2), (oa - 1, ob), (oa, ob + nz)]        # the corners, the middle, two outside
    view, start = (oa + nx - 1, ob), (oa + nx // 2, ob + nz // 2)
    got = core(fr, pr, er, cell, state, cost, cells, view, start, oa, ob)
    assert np.array_equal(got["gains"], ER.gains(fr, R, state, cells, oa, ob)) and got["gains"][3:].tolist() == [-1, -1]
    assert np.array_equal(got["mask"], ER.view(fr, R, state, nx - 1, 0)[0])
    recs, scores, best, feasible = ER.rank(fr, pr, er, R, state, cost, start, oa, ob)
    assert np.array_equal(got["recs"], recs) and np.array_equal(got["scores"], scores) and (got["best"], got["feasible"]) == (best, feasible)


def test_the_program_refuses_what_the_library_refuses(core):
    one, zero = np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8)
    for kw in BAD:
        assert core(FR.FrontParams(), PR.PlanParams(), ER.ExploreParams(**kw), 1.0, one, zero, [], (0, 0), (0, 0)) is None, kw
    assert core(FR.FrontParams(), PR.PlanParams(), ER.ExploreParams(range=10.0), 0.05, one, zero, [], (0, 0), (0, 0)) is None       # R = 200
