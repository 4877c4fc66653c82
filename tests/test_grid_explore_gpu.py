"""GPU: the exploration layer of the ground grid (include/svh_grid.h, "EXPLORATION"; csrc/grid_explore_kernels.hip,
csrc/grid_engine.cpp) against the header's host form (core_explore) and the restatement tests/grid_explore_ref.py, which
tests/test_grid_explore.py pins on the CPU.  Every comparison is exact: GAIN, the VIEW plane, the records, the scores, the best and
the image byte for byte.

Shapes: k_grid_view_gain runs one workgroup of 256 lanes per viewpoint and deals the 8 R rays to its lanes; the counted cells are
bits of a bitmap of (2 R + 1)^2 bits in LDS.  R = 1, 2, 7, 8, 9, 31, 32, 33, 64, 128 gives 8 .. 1024 rays -- less than a wave, a
wave, one pass of the workgroup and four -- and bitmaps of 9 .. 66049 bits, on both sides of a 32-bit word and of one pass of the
lanes over the words.  The workgroups stride over the viewpoints beyond 16384 of them.  The scenes through the object are those
of tests/test_grid_front_gpu.py: walls of obstacle points with gaps, cells without points, rays from cell (3, 4)."""
import ctypes as C

import numpy as np
import pytest

import grid_explore_ref as ER
import grid_front_ref as FR
import grid_plan_ref as PR
import grid_ref as R_
import test_grid_explore as TE
import test_grid_front as TF
import test_grid_front_gpu as TFG
import test_grid_local_gpu as TL
import test_grid_plan_gpu as TPG
import test_grid_trav_gpu as TT
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2
U, S, F, O, D = TF.U, TF.S, TF.F, TF.O, TF.D
INF, FAR = ER.INFEASIBLE, ER.FAR
RESTATE_CELLS = 65 * 65
CELL = TL.CELL
differ = TPG.differ


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


def run(G, state, R, cost=None, cells=None, view=None, start=None, rgb=None, oa=0, ob=0, front=None, plan=None, tag="", **kw):
    """device_explore against core_explore, and core_explore against the restatement on small windows; the device's dict"""
    state = np.ascontiguousarray(state, np.uint8)
    cost = np.zeros(state.shape, np.uint8) if cost is None else np.ascontiguousarray(cost, np.uint8)
    front, plan = front or {}, plan or {}
    args = (G.default_explore(range=float(R), **kw), 1.0, state, cost, G.default_front(**front), G.default_plan(**plan), oa, ob, cells, view, rgb, start)
    got, want = G.device_explore(*args), G.core_explore(*args)
    assert got.keys() == want.keys(), tag
    for k in got:
        if isinstance(got[k], np.ndarray):
            differ(tag, k, got[k], want[k])
        else:
            assert got[k] == want[k], (tag, k, got[k], want[k])
    if state.size <= RESTATE_CELLS:
        fr = FR.FrontParams(**front)
        if cells is not None:
            differ(tag + " (header against restatement)", "GAIN", want["gains"], ER.gains(fr, R, state, cells, oa, ob))
        if view is not None:
            mask = ER.view(fr, R, state, view[0] - oa, view[1] - ob)[0]
            differ(tag + " (header against restatement)", "VIEW", want["mask"], mask)
            if rgb is not None:
                differ(tag + " (header against restatement)", "the image", want["image"], ER.overlay(rgb, mask, view[0] - oa, view[1] - ob))
        if start is not None:
            recs, scores, best, feasible = ER.rank(fr, PR.PlanParams(**plan), ER.ExploreParams(range=float(R), **kw), R, state, cost, start, oa, ob)
            differ(tag + " (header against restatement)", "the records", want["recs"], recs)
            differ(tag + " (header against restatement)", "the scores", want["scores"], scores)
            assert (want["best"], want["stats"]) == (best, (len(recs), feasible)), tag
    return got


def positions(nx, nz):
    """the four corners, a cell on each edge, one cell inside, the centre, and four outside the window"""
    a, b = nx - 1, nz - 1
    return [(0, 0), (a, 0), (0, b), (a, b), (nx // 2, 0), (nx // 2, b), (0, nz // 2), (a, nz // 2), (min(1, a), min(1, b)), (nx // 2, nz // 2), (-1, 0), (nx, 0),
            (0, -1), (a, nz)]


# ---- rays, blocks and bitmaps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 7, 8, 9, 31, 32, 33, 64, 128])
def test_ranges_windows_and_viewpoint_positions(G, R):
    """1 x 1, 16 x 16, 17 x 33 and 256 x 256: beyond R = 8 the small windows have a side smaller than R"""
    for nx, nz in ((1, 1), (16, 16), (17, 33), (256, 256)):
        rng = np.random.default_rng(1000 * R + nx)
        state, _ = TF.random_planes(rng, nx, nz, 0.4)
        state[rng.random((nz, nx)) < 0.5] &= 0xFC                                       # half the window unknown: obstacles stay rare enough to see far
        oa, ob = (0, 0) if nx != 17 else (-9, 2 ** 20 - 8192)
        cells = np.array(positions(nx, nz)) + (oa, ob)
        tag = "R %d, %d x %d" % (R, nx, nz)
        got = run(G, state, R, cells=cells, oa=oa, ob=ob, tag=tag)
        assert got["gains"][-4:].tolist() == [-1] * 4 and (got["gains"][:-4] >= 0).all()
        for k in (0, 3, 7, 9):                                                          # two corners, an edge, the centre
            m = run(G, state, R, view=tuple(cells[k]), oa=oa, ob=ob, tag=tag + ", the view of %r" % (tuple(cells[k]),))["mask"]
            assert (m == 2).sum() == got["gains"][k] and m[cells[k][1] - ob, cells[k][0] - oa] == 0
    n = min(2 * R + 1, 256)                                                             # an open window: the disc
    x, z = np.meshgrid(np.arange(n), np.arange(n))
    d2 = (x - n // 2) ** 2 + (z - n // 2) ** 2
    got = run(G, np.zeros((n, n), np.uint8), R, cells=[(n // 2, n // 2)], view=(n // 2, n // 2), tag="R %d, open" % R)
    assert np.array_equal(got["mask"] == 2, (d2 > 0) & (d2 <= R * R)) and got["gains"][0] == ((d2 > 0) & (d2 <= R * R)).sum()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025, 16384 + 3])
def test_viewpoint_counts(G, n):
    """with duplicates, and some outside; beyond 16384 the workgroups stride"""
    rng = np.random.default_rng(n)
    big = n > 2000
    nx, nz, R = (9, 7, 2) if big else (64, 64, 9)
    state, _ = TF.random_planes(rng, nx, nz, 0.5)
    cells = np.stack([rng.integers(-1, nx + 1, n), rng.integers(-1, nz + 1, n)], 1)
    half = n // 2
    cells[half:2 * half] = cells[:half]                                                 # every viewpoint twice
    got = run(G, state, R, cells=cells if n else np.zeros((0, 2), np.int32), tag="%d viewpoints" % n)
    assert len(got["gains"]) == n
    assert np.array_equal(got["gains"][half:2 * half], got["gains"][:half])


def test_planes_of_one_kind(G):
    nx, nz, R = 33, 17, 8
    x, z = np.meshgrid(np.arange(nx), np.arange(nz))
    cells = positions(nx, nz)
    inside = (np.array(cells)[:, 0] >= 0) & (np.array(cells)[:, 0] < nx) & (np.array(cells)[:, 1] >= 0) & (np.array(cells)[:, 1] < nz)
    got = run(G, np.full((nz, nx), U, np.uint8), R, cells=cells, view=cells[9], tag="all unexplored")
    d2 = (x - cells[9][0]) ** 2 + (z - cells[9][1]) ** 2
    assert got["gains"][9] == ((d2 > 0) & (d2 <= R * R)).sum() and set(np.unique(got["mask"])) == {0, 2}
    for name, value in (("all free", F), ("all seen", S), ("all drops", D)):
        got = run(G, np.full((nz, nx), value, np.uint8), R, cells=cells, view=cells[9], tag=name)
        assert (got["gains"][inside] == 0).all() and set(np.unique(got["mask"])) == {0, 1}
    assert run(G, np.full((nz, nx), S, np.uint8), R, cells=cells, front=dict(unexplored=16))["gains"][9] == ((d2 > 0) & (d2 <= R * R)).sum()
    got = run(G, np.full((nz, nx), O, np.uint8), R, cells=cells, view=cells[9], tag="all obstacles")
    assert (got["gains"][inside] == 0).all() and not got["mask"].any()
    ring = np.full((nz, nx), U, np.uint8)                                               # obstacles on all eight neighbours
    ring[7:10, 15:18] = O
    got = run(G, ring, R, cells=[(16, 8), (16, 6)], view=(16, 8), tag="ring 1 closed")
    assert got["gains"][0] == 0 and got["gains"][1] > 0 and not got["mask"].any()


def test_the_hand_cases_on_the_device(G):
    state = np.full((5, 5), U, np.uint8)
    state[2, 2] = F
    got = run(G, state, 2, cells=[(2, 2), (0, 0)], view=(2, 2))
    assert got["gains"].tolist() == [12, 5] and got["mask"].tolist() == [[0, 0, 2, 0, 0], [0, 2, 2, 2, 0], [2, 2, 0, 2, 2], [0, 2, 2, 2, 0], [0, 0, 2, 0, 0]]
    shadow = np.full((7, 7), U, np.uint8)
    shadow[3, 4] = O
    assert run(G, shadow, 3, cells=[(3, 3)])["gains"].tolist() == [25]
    squeeze = np.full((3, 3), U, np.uint8)
    squeeze[0, 1] = squeeze[1, 0] = O
    assert run(G, squeeze, 2, cells=[(0, 0)], view=(0, 0))["mask"].tolist() == [[0, 0, 0], [0, 2, 0], [0, 0, 0]]
    gap = np.full((5, 7), U, np.uint8)
    gap[0], gap[1], gap[1, 3] = F, O, F
    got = run(G, gap, 3, cells=[(3, 0)], view=(3, 0))
    assert got["gains"].tolist() == [4] and got["mask"][2].tolist() == [0, 0, 2, 2, 2, 0, 0]
    row = np.array([[F, U, S, F, U, S, O, U]], np.uint8)
    for m, mask in ((8, [0, 2, 1, 1, 2, 1, 0, 0]), (16, [0, 1, 2, 1, 1, 2, 0, 0]), (24, [0, 2, 2, 1, 2, 2, 0, 0])):
        assert run(G, row, 7, view=(0, 0), front=dict(unexplored=m))["mask"].tolist() == [mask]


def test_the_same_bytes_twice_and_in_reversed_order(G):
    rng = np.random.default_rng(11)
    state, cost = TE.planes(rng, 70, 45, 0.6)
    cells = np.stack([rng.integers(-1, 71, 300), rng.integers(-1, 46, 300)], 1)
    e, fr, pl = G.default_explore(range=33.0), G.default_front(min_size=2, unexplored=24), G.default_plan(unknown=40)
    first = G.device_explore(e, 1.0, state, cost, fr, pl, cells=cells, view=(35, 20), start=(10, 10))
    for _ in range(2):
        again = G.device_explore(e, 1.0, state, cost, fr, pl, cells=cells, view=(35, 20), start=(10, 10))
        assert all(first[k].tobytes() == again[k].tobytes() for k in ("gains", "mask", "recs", "scores")) and again["best"] == first["best"]
    back = G.device_explore(e, 1.0, state, cost, fr, pl, cells=cells[::-1].copy())
    assert back["gains"][::-1].tobytes() == first["gains"].tobytes()
    assert len(first["recs"]) > 3


# ---- the ranking on planes -------------------------------------------------------------------------------------------------
def test_the_score_cases_on_the_device(G):
    row, cost, front = TE.ROW, TE.ROW_COST, dict(min_size=1)
    got = run(G, row, 2, cost, start=(4, 0), front=front, tag="a tie")
    assert got["recs"].tolist() == [[1, 1, 0, 1, 1500], [7, 7, 0, 1, 1500]] and got["scores"].tolist() == [1000, 1000] and got["best"] == 0
    got = run(G, row, 2, cost, start=(7, 0), front=front, w_gain=0, tag="the start is a representative")
    assert got["recs"][:, 4].tolist() == [3000, 0] and got["best"] == 1
    got = run(G, row, 2, cost, start=(5, 0), front=front, w_gain=0, w_reach=0, tag="no weights")
    assert got["scores"].tolist() == [0, 0] and got["best"] == 0 and got["stats"] == (2, 2)
    assert run(G, row, 2, cost, start=(4, 0), front=front, min_gain=1)["stats"] == (2, 2)
    got = run(G, row, 2, cost, start=(4, 0), front=front, min_gain=2, tag="min_gain one above")
    assert got["scores"].tolist() == [INF, INF] and got["best"] == -1 and got["stats"] == (2, 0)
    for plan, feasible, best in ((dict(max_cost=1500), 2, 0), (dict(max_cost=1499), 0, -1)):
        got = run(G, row, 2, cost, start=(4, 0), front=front, plan=plan, tag="the horizon")
        assert got["stats"] == (2, feasible) and got["best"] == best
    for start in ((0, 0), (-3, 0), (4, 1)):
        got = run(G, row, 2, cost, start=start, front=front, tag="a start that reaches nothing")
        assert got["recs"][:, 4].tolist() == [FAR, FAR] and got["best"] == -1
    wall = cost.copy()
    wall[0, 5] = 254
    got = run(G, row, 2, wall, start=(4, 0), front=front, tag="walled off")
    assert got["recs"][:, 4].tolist() == [1500, FAR] and got["scores"].tolist() == [1000, INF] and got["stats"] == (2, 1) and got["best"] == 0
    got = run(G, row, 2, cost, start=(4, 0), tag="no kept component")
    assert len(got["recs"]) == 0 and got["best"] == -1 and got["stats"] == (0, 0)
    got = run(G, row, 2, cost, start=(14, -7), oa=10, ob=-7, front=front, tag="offsets")
    assert got["recs"].tolist() == [[1, 11, -7, 1, 1500], [7, 17, -7, 1, 1500]]


@pytest.mark.parametrize("nx,nz", [(1, 1), (16, 16), (17, 33), (64, 64), (257, 70)])
def test_the_ranking_on_random_windows(G, nx, nz):
    rng = np.random.default_rng(7 * nx + nz)
    for k, (R, front, plan, kw, oa, ob) in enumerate([(5, dict(min_size=2), dict(), dict(), 0, 0), (12, dict(min_size=1, unexplored=24, border=1), dict(unknown=30), dict(w_gain=3, min_gain=4), 7, -5),
                                                       (40, dict(min_size=3, unexplored=16), dict(max_cost=30000), dict(w_reach=7, w_gain=65535, min_gain=0), -(2 ** 20 - 8192), 2 ** 20 - 8192)]):
        state, cost = TE.planes(rng, nx, nz, (0.5, 0.7, 0.9)[k])
        start = (int(rng.integers(0, nx)) + oa, int(rng.integers(0, nz)) + ob)
        view = (int(rng.integers(0, nx)) + oa, int(rng.integers(0, nz)) + ob)
        base = rng.integers(0, 256, (nz, nx, 3)).astype(np.uint8)
        run(G, state, R, cost, view=view, start=start, rgb=base, oa=oa, ob=ob, front=front, plan=plan, tag="%d x %d, case %d" % (nx, nz, k), **kw)


# ---- through the object --------------------------------------------------------------------------------------------------
def expected(ref, er, R, start_cell=None, view=None, cells=None):
    """the restatement on the restated grid's own STATE and COST"""
    tr, state = ref.trav(), ref.local_planes()["state"]
    out = dict(front=TFG.expected(ref))
    if cells is not None:
        out["gains"] = ER.gains(ref.front, R, state, cells, ref.oa, ref.ob)
    if view is not None:
        out["mask"] = ER.view(ref.front, R, state, view[0] - ref.oa, view[1] - ref.ob)[0]
        out["image"] = ER.overlay(out["front"]["image"], out["mask"], view[0] - ref.oa, view[1] - ref.ob)
    if start_cell is not None:
        out["recs"], out["scores"], out["best"], out["feasible"] = ER.rank(ref.front, ref.plan, er, R, state, tr["cost"], start_cell, ref.oa, ref.ob,
                                                                           front_recs=out["front"]["recs"])
    return out


def check(G, g, ref, er, start_ab, tag=""):
    """gains, a VIEW plane, the image and the ranking from window cell start_ab against the restatement; what it expects"""
    p, R = g.explore_params()
    assert R == ER.range_cells(er.range, CELL) and (p.min_gain, p.w_gain, p.w_reach) == (er.min_gain, er.w_gain, er.w_reach)
    nx, nz = ref.P.nx, ref.P.nz
    cells = np.array(positions(nx, nz)) + (ref.oa, ref.ob)
    start_cell = (ref.oa + start_ab[0], ref.ob + start_ab[1])
    view = tuple(int(v) for v in cells[9])
    w = expected(ref, er, R, start_cell, view, cells)
    differ(tag, "GAIN", g.view_gain(cells), w["gains"])
    assert g.explore_stats()[3] == 1
    differ(tag, "VIEW", g.view_mask(*view), w["mask"])
    differ(tag, "the image", g.render_view(*view), w["image"])
    best, recs, scores = g.explore_rank(TL.centre(ref, *start_ab))
    differ(tag, "the records", recs, w["recs"])
    differ(tag, "the scores", scores, w["scores"])
    assert best == w["best"] and g.explore_count == len(w["recs"]) and g.explore_stats()[:2] == (len(w["recs"]), w["feasible"]), (tag, best, w["best"])
    assert g.explore_stats()[3] == (1 if len(w["recs"]) else 0)
    for cap in (0, 1):                                                                # the table with less room, with none
        b, r, s = g.explore_rank(TL.centre(ref, *start_ab), cap=cap)
        assert b == best and np.array_equal(r, recs[:cap]) and np.array_equal(s, scores[:cap]) and g.explore_count == len(recs)
    return w


@pytest.mark.parametrize("shape", ["65 x 65", "33 x 17"])
def test_scenes_of_walls_with_gaps(G, shape):
    nx, nz = (65, 65) if shape == "65 x 65" else (33, 17)
    ref, g, rng = TFG.build(G, nx, nz, 41)
    er = ER.ExploreParams()
    assert g.explore_params()[1] == 20
    w = check(G, g, ref, er, (3, 4), "the defaults")
    if shape == "65 x 65":
        assert len(w["recs"]) >= 2 and w["feasible"] >= 1 and w["best"] >= 0 and (w["recs"][:, 3] > 0).all() and (w["mask"] == 1).any()
    for kw in (dict(range=4.0, w_gain=0), dict(range=64.0, min_gain=50, w_reach=0), dict(range=3.3, w_gain=65535, w_reach=65535)):
        g.set_explore(**kw)
        for k, v in kw.items():
            setattr(er, k, np.float32(v) if k == "range" else v)
        check(G, g, ref, er, (3, 4), "%r" % kw)
    g.set_frontier(unexplored=24)                                                     # what is counted follows the frontier parameters in force
    ref.front.unexplored = 24
    check(G, g, ref, er, (nx // 2, nz - 2), "unexplored 24")


def test_after_a_scroll_as_a_fresh_grid(G):
    """the window scrolls by (5, -3), no multiple of 16: the accumulators wrap round the torus; a fresh grid that was fed the same
    points at the same offsets says the same"""
    nx = nz = 65
    rng = np.random.default_rng(46)
    ref, g = TPG.pair(G, nx, nz)
    walls = TPG.walls(nx, nz)
    first = TT.fill(ref, rng, walls, TFG.holes(nx, nz, rng) & ~walls)
    TT.add_both(g, ref, first)
    g.set_frontier(**TFG.FRONT)
    ref.front = FR.FrontParams(**TFG.FRONT)
    more = TL.at_cells(ref, rng.integers(0, nx + 5, 400), rng.integers(-3, nz, 400), 0.0)     # global cells: the offsets are still zero
    g.scroll(5, -3)
    ref.scroll(5, -3)
    TT.add_both(g, ref, np.concatenate([more, more]))
    er = ER.ExploreParams()
    w = check(G, g, ref, er, (3, 9), "scrolled")
    assert g.window() == (5, -3)
    ref2, g2 = TPG.pair(G, nx, nz)
    g2.set_frontier(**TFG.FRONT)
    g2.scroll(5, -3)
    g2.add_points(first)
    g2.add_points(np.concatenate([more, more]))
    cells = np.array(positions(nx, nz)) + (5, -3)
    start = TL.centre(ref, 3, 9)
    assert g2.view_gain(cells).tobytes() == g.view_gain(cells).tobytes() and g2.view_mask(*cells[9]).tobytes() == g.view_mask(*cells[9]).tobytes()
    a, b = g.explore_rank(start), g2.explore_rank(start)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and len(a[1]) == len(w["recs"])


def test_a_ranking_leaves_the_planner_alone_and_the_reach_field_is_cached(G):
    nx = nz = 65
    ref, g, rng = TFG.build(G, nx, nz, 47)
    er = ER.ExploreParams()
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    f = TPG.check(G, g, ref, "the field")
    pot, dir_, stats = g.plan_plane(G.PLAN_POT), g.plan_plane(G.PLAN_DIR), g.plan_stats()
    fields = g.explore_stats()[2]
    assert fields == 0
    start = TL.centre(ref, 3, 4)
    best, recs, scores = g.explore_rank(start)
    assert g.explore_stats()[2] == 1
    assert g.plan_stats() == stats
    G.lib().svh_test_fail_at(b"launch:1:0")                                           # the planner's field: from the cache, not computed again
    assert g.plan_plane(G.PLAN_POT).tobytes() == pot.tobytes() and g.plan_plane(G.PLAN_DIR).tobytes() == dir_.tobytes()
    G.lib().svh_test_fail_at(None)
    for k, ab in enumerate([(3, 4), (3, 4), (4, 4), (4, 4), (3, 4)]):                  # one field per new start cell, none for a repeated one
        g.explore_rank(TL.centre(ref, *ab))
        assert g.explore_stats()[2] == [1, 1, 2, 2, 3][k], k
    g.view_gain([(3, 4)]), g.view_mask(3, 4), g.render_view(3, 4)                      # none of these needs it
    assert g.explore_stats()[2] == 3
    for change in (lambda: g.set_plan(neutral=60), lambda: g.set_traversability(inflate=1.5), lambda: g.scroll(1, 0),
                   lambda: g.add_points(TL.at_cells(ref, [5, 5], [5, 5], 0.0))):      # each invalidates the field
        before = g.explore_stats()[2]
        change()
        g.explore_rank(TL.centre(ref, 6, 6))
        assert g.explore_stats()[2] == before + 1


def test_the_goal_from_the_ranking(G):
    nx = nz = 65
    ref, g, rng = TFG.build(G, nx, nz, 43)
    er = ER.ExploreParams()
    w = check(G, g, ref, er, (3, 4), "before")
    assert w["best"] >= 0
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    start = TL.centre(ref, 3, 4)
    assert g.set_goal_explore(start) == 1
    rec = w["recs"][w["best"]]
    ref.set_goals([rec[1:3]])
    fld = TPG.check(G, g, ref, "the goal from the ranking")
    assert g.plan_stats()[:2] == (1, 1)
    st, cells, cost = TPG.check_path(G, g, ref, fld, start, "to the best frontier")
    assert st == G.PATH_FOUND and cost == rec[4] and tuple(cells[-1]) == tuple(rec[1:3])
    g.set_explore(min_gain=2 ** 26)                                                   # no best: the goals are left alone
    assert g.set_goal_explore(start) == 0 and g.plan_stats()[:2] == (1, 1)
    TPG.check(G, g, ref, "the goal afterwards")


# ---- failures and refusals -----------------------------------------------------------------------------------------------
def test_a_failed_ranking_leaves_everything_but_the_reach_field(G):
    """with the cost planes, the planner's field and the frontier result cached, the first launch of a ranking is the seed of the
    reach field"""
    nx = nz = 65
    ref, g, rng = TFG.build(G, nx, nz, 44)
    er = ER.ExploreParams()
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    f = TPG.check(G, g, ref, "the field")
    w = check(G, g, ref, er, (3, 4), "before")
    fields = g.explore_stats()[2]
    before = TL.snapshot(G, g)
    pot, front, roll = g.plan_plane(G.PLAN_POT), g.front_plane(G.FRONT_FLAGS), g.roll_params()
    start = TL.centre(ref, 9, 4)
    G.lib().svh_test_fail_at(b"launch:1")
    with pytest.raises(G.SvhError) as e:
        g.explore_rank(start)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR and g.explore_stats()[2] == fields
    G.lib().svh_test_fail_at(b"launch:1:0")                                           # the cost planes, the field and the frontier result: from the cache
    assert g.plan_plane(G.PLAN_POT).tobytes() == pot.tobytes() and g.trav_plane(G.TRAV_COST).tobytes() == f["trav"]["cost"].tobytes()
    assert g.front_plane(G.FRONT_FLAGS).tobytes() == front.tobytes() and np.array_equal(g.frontiers(), w["front"]["recs"])
    G.lib().svh_test_fail_at(None)
    assert TL.same(TL.snapshot(G, g), before) and g.plan_stats()[0] == 7 and g.roll_params()[1:] == roll[1:]
    for spec in (b"copy:1", b"wait:1"):                                               # with the field cached as well: the table's way to the host
        g.explore_rank(start)
        count = g.explore_stats()[2]
        G.lib().svh_test_fail_at(spec)
        with pytest.raises(G.SvhError) as e:
            g.explore_rank(start)
        G.lib().svh_test_fail_at(None)
        assert e.value.code == HIP_ERR
        g.explore_rank(start)
        assert g.explore_stats()[2] == count + 1                                      # the reach field was invalid and is computed again
    check(G, g, ref, er, (9, 4), "the call repeated")
    TPG.check(G, g, ref, "the field afterwards")


def test_refusals_leave_every_byte(G, hip):
    nx, nz = 65, 33
    ref, g, rng = TFG.build(G, nx, nz, 45)
    er = ER.ExploreParams()
    w = check(G, g, ref, er, (3, 4), "before")
    before, stats = TL.snapshot(G, g), g.explore_stats()
    L = g._L
    for kw in TE.BAD:
        if kw.get("range") in (0.99, 129.0):
            kw = dict(range=kw["range"] * CELL)
        p = G.default_explore(**kw)
        assert L.svh_grid_set_explore(g._h, C.byref(p)) == BAD_ARG and "svh_grid_set_explore" in G.last_error(), kw
    assert g.explore_params()[0].asdict() == dict(range=10.0, min_gain=1, w_gain=500, w_reach=1) and g.explore_params()[1] == 20
    buf = np.full(nx * nz * 3, 0xAB, np.uint8)
    dev = Dev(hip, 64)
    n, best = C.c_int64(-7), C.c_int32(-7)
    xyz = np.array(TL.centre(ref, 3, 4), np.float64)
    nan = np.array([np.nan, 0, 0], np.float64)
    calls = [lambda: L.svh_grid_set_explore(g._h, None), lambda: L.svh_grid_get_explore(g._h, None, None),
             lambda: L.svh_grid_view_gain(g._h, None, 1, 0, buf.ctypes.data), lambda: L.svh_grid_view_gain(g._h, buf.ctypes.data, 1, 0, None),
             lambda: L.svh_grid_view_gain(g._h, buf.ctypes.data, -1, 0, buf.ctypes.data), lambda: L.svh_grid_view_gain(g._h, buf.ctypes.data, 2 ** 26 + 1, 0, buf.ctypes.data),
             lambda: L.svh_grid_view_gain(g._h, dev.addr + 1, 1, 1, dev.addr + 16), lambda: L.svh_grid_view_gain(g._h, dev.addr, 1, 1, dev.addr + 18),
             lambda: L.svh_grid_view_mask(g._h, ref.oa, ref.ob, None, 0), lambda: L.svh_grid_view_mask(g._h, ref.oa - 1, ref.ob, buf.ctypes.data, 0),
             lambda: L.svh_grid_view_mask(g._h, ref.oa, ref.ob + nz, buf.ctypes.data, 0),
             lambda: L.svh_grid_explore_rank(g._h, None, buf.ctypes.data, None, 1, C.addressof(n), C.addressof(best)),
             lambda: L.svh_grid_explore_rank(g._h, nan.ctypes.data, buf.ctypes.data, None, 1, C.addressof(n), C.addressof(best)),
             lambda: L.svh_grid_explore_rank(g._h, xyz.ctypes.data, buf.ctypes.data, None, -1, C.addressof(n), C.addressof(best)),
             lambda: L.svh_grid_explore_rank(g._h, xyz.ctypes.data, buf.ctypes.data, None, 1, None, C.addressof(best)),
             lambda: L.svh_grid_explore_rank(g._h, xyz.ctypes.data, buf.ctypes.data, None, 1, C.addressof(n), None),
             lambda: L.svh_grid_plan_set_goal_explore(g._h, None), lambda: L.svh_grid_plan_set_goal_explore(g._h, nan.ctypes.data),
             lambda: L.svh_grid_get_explore_stats(g._h, None), lambda: L.svh_grid_render_view(g._h, ref.oa, ref.ob, None, 0),
             lambda: L.svh_grid_render_view(g._h, ref.oa + nx, ref.ob, buf.ctypes.data, 0)]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG and "svh_grid" in G.last_error(), k
    assert (buf == 0xAB).all() and (dev.get() == 0xEE).all() and n.value == -7 and best.value == -7
    assert TL.same(TL.snapshot(G, g), before) and g.explore_stats() == stats
    check(G, g, ref, er, (3, 4), "after")
    # device pointers: the gains, the VIEW plane and the image, nothing beyond them
    cells = (np.array(positions(nx, nz)) + (ref.oa, ref.ob)).astype(np.int32)
    d_cells, d_out = Dev(hip, cells), Dev(hip, 4 * len(cells) + 16)
    g.view_gain(device_ptrs=(d_cells.addr, d_out.addr), n=len(cells))
    got = d_out.get()
    assert got[:4 * len(cells)].tobytes() == w["gains"].tobytes() and (got[4 * len(cells):] == 0xEE).all()
    view = tuple(int(v) for v in cells[9])
    out = Dev(hip, nx * nz + 16)
    g.view_mask(*view, device_ptr=out.addr)
    got = out.get()
    assert got[:nx * nz].tobytes() == w["mask"].tobytes() and (got[nx * nz:] == 0xEE).all()
    out = Dev(hip, 3 * nx * nz + 16)
    g.render_view(*view, device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:3 * nx * nz].reshape(nz, nx, 3), w["image"]) and (got[3 * nx * nz:] == 0xEE).all()


def test_exploration_needs_a_range_and_a_traversability_that_fit(G):
    """cells of 5 cm: the default range would be 200 cells; the entries refuse until svh_grid_set_explore succeeds, as the rollouts do"""
    g = G.Grid(G.default_params(nx=9, nz=9, cell=0.05, x0=0.0, z0=0.0, T=R_.frame_camera(0.0), min_points=1))
    g.set_traversability(inscribed=0.04, inflate=0.2)
    g.set_frontier(min_size=1)
    g.add_points(np.array([[0.225, 0.0, 0.225, 0.5]], np.float32))
    assert g.explore_params()[1] == 0
    buf = np.full(81 * 3, 0xAB, np.uint8)
    n, best = C.c_int64(-7), C.c_int32(-7)
    xyz = np.array([0.225, 0.0, 0.225], np.float64)
    L = g._L
    calls = (lambda: L.svh_grid_view_gain(g._h, buf.ctypes.data, 1, 0, buf.ctypes.data), lambda: L.svh_grid_view_mask(g._h, 4, 4, buf.ctypes.data, 0),
             lambda: L.svh_grid_explore_rank(g._h, xyz.ctypes.data, buf.ctypes.data, None, 1, C.addressof(n), C.addressof(best)),
             lambda: L.svh_grid_plan_set_goal_explore(g._h, xyz.ctypes.data), lambda: L.svh_grid_render_view(g._h, 4, 4, buf.ctypes.data, 0))
    for call in calls:
        assert call() == BAD_ARG and "svh_grid_set_explore" in G.last_error()
    assert (buf == 0xAB).all() and n.value == -7 and best.value == -7 and g.explore_stats() == (0, 0, 0, 0)
    g.set_explore(range=0.1)
    assert g.explore_params()[1] == 2
    assert g.view_gain([(4, 4)]).tolist() == [12] and g.view_mask(4, 4).tolist() == [[0] * 9] * 2 + [[0, 0, 0, 0, 2, 0, 0, 0, 0], [0, 0, 0, 2, 2, 2, 0, 0, 0],
                                                                                                   [0, 0, 2, 2, 0, 2, 2, 0, 0], [0, 0, 0, 2, 2, 2, 0, 0, 0],
                                                                                                   [0, 0, 0, 0, 2, 0, 0, 0, 0]] + [[0] * 9] * 2
    best_, recs, scores = g.explore_rank(xyz)
    assert recs.tolist() == [[40, 4, 4, 12, 0]] and scores.tolist() == [-6000] and best_ == 0 and g.set_goal_explore(xyz) == 1
    t = G.Grid(G.default_params(nx=9, nz=9, cell=0.005, x0=0.0, z0=0.0, T=R_.frame_camera(0.0), min_points=1))     # no traversability either
    t.set_explore(range=0.05)
    for call in (lambda: t._L.svh_grid_view_gain(t._h, buf.ctypes.data, 1, 0, buf.ctypes.data), lambda: t._L.svh_grid_view_mask(t._h, 4, 4, buf.ctypes.data, 0),
                 lambda: t._L.svh_grid_explore_rank(t._h, xyz.ctypes.data, buf.ctypes.data, None, 1, C.addressof(n), C.addressof(best)),
                 lambda: t._L.svh_grid_render_view(t._h, 4, 4, buf.ctypes.data, 0)):
        assert call() == BAD_ARG and "svh_grid_set_traversability" in G.last_error()
    assert (buf == 0xAB).all()


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------
def test_pipeline_grid_explore(G, tmp_path, monkeypatch, capsys):
    """--grid-local DIR --grid-cost DIR2 --grid-explore DIR3 --grid-unexplored both --grid-frontier-min 2 --grid-explore-range 4 on the
    two golden frames: one image and one line of explore.jsonl per frame, the restatement's after the same steps"""
    import json
    import os
    import sys
    import grid_local_ref as LR
    import grid_trav_ref as TR
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
    d, d2, d3 = str(tmp_path / "loc"), str(tmp_path / "cost"), str(tmp_path / "explore")
    common = ["--grid-slope", "2.0", "--grid-inscribed", "0.1", "--grid-inflate", "0.5", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-explore", d3, "--grid-unexplored", "both",
                                      "--grid-frontier-min", "2", "--grid-explore-range", "4"] + common)
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("exploration: ") and "within 16 cells" in l and "2 images and explore.jsonl" in l for l in out), out[-4:]
    assert sorted(os.listdir(d3)) == ["explore.jsonl"] + ["explore_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(d3, "explore.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = PR.Grid(R_.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0), TR.TravParams(max_slope=2.0, inscribed=0.1, inflate=0.5), PR.PlanParams(unknown=100))
    ref.front = FR.FrontParams(unexplored=24, min_size=2)
    er = ER.ExploreParams(range=4.0)
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre_ = p.H_total[:3, 3]
        ref.follow(centre_, 48, 80)
        ref.add_from(p.view.points(p.view.count(view.LISTS) - 1), centre_)
        start_cell = LR.cell_of(ref.P, centre_)
        w = expected(ref, er, 16, start_cell)
        best = w["best"]
        want = dict(frame=k, kept=w["front"]["stats"][2], records=len(w["recs"]), feasible=w["feasible"], best=best, rep=None, gain=None, reach=None, score=None,
                    status=-1, length=0, cost=FAR)
        image, cells = w["front"]["image"].copy(), []
        if best >= 0:
            rec = w["recs"][best]
            ref.set_goals([rec[1:3]])
            status, cells, cost = ref.path(centre_, ref.field())
            want.update(rep=[int(rec[1]), int(rec[2])], gain=int(rec[3]), reach=int(rec[4]), score=int(w["scores"][best]), status=status, length=len(cells), cost=cost)
            image = expected(ref, er, 16, view=(int(rec[1]), int(rec[2])))["image"]
        assert lines[k] == want, (k, lines[k], want)
        for ga, gb in cells:
            image[160 - 1 - (gb - ref.ob), ga - ref.oa] = PR.PATH_COLOUR
        img = read_ppm(os.path.join(d3, "explore_%06d.ppm" % k))
        assert img.shape == (160, 96, 3) and np.array_equal(img, image), k
        k += 1
    assert k == 2 and len(lines) == 2 and lines[1]["records"] > 0
    for line in lines:                                                                # the path to the goal costs what the ranking said
        assert line["best"] < 0 or (line["status"] == 0 and line["cost"] == line["reach"])
    # --grid-explore is refused without --grid-cost, --grid-explore-range without --grid-explore or with a range that is none
    for argv in (["--grid-local", d, "--grid-explore", d3], ["--grid-local", d, "--grid-cost", d2, "--grid-explore-range", "4"],
                 ["--grid-local", d, "--grid-cost", d2, "--grid-explore", d3, "--grid-explore-range", "0"]):
        monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py"] + argv + common)
        with pytest.raises(SystemExit):
            SP.main()
