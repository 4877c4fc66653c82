"""GPU: the planner of the ground grid (include/svh_grid.h, "PLANNING"; csrc/grid_plan_kernels.hip, csrc/grid_engine.cpp)
against the header's host Dijkstra (core_plan) and the numpy / heapq restatement tests/grid_plan_ref.py, which
tests/test_grid_plan.py pins on the CPU.  Every comparison is exact: POT, DIR, the path and the plan image bit for bit.

Shapes: k_grid_plan_relax runs one workgroup of 256 lanes per active tile of T x T cells, T = PLAN_TILE, with a halo of one
cell; k_grid_plan_seed and k_grid_plan_dir run 256 cells per workgroup.  The windows 1 x 1, 1 x 9, 9 x 1, 3 x 3, (T - 1)^2,
T^2, (T + 1)^2, (2 T + 1) x (T + 1), (T + 1) x (2 T + 1) and 257 x 129 put lane, wave and tile edges on rows, on columns and
on both.  The mazes (device_plan on a caller's cost plane) make POT cross tile borders hundreds of times, so the lists of
active tiles do the work; the scenes through the object are walls of obstacle points with gaps, built with the helpers of
tests/test_grid_trav_gpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import grid_plan_ref as PR
import grid_ref as R
import grid_trav_ref as TR
import helpers as H
import test_grid as TG
import test_grid_local_gpu as TL
import test_grid_plan as TP
import test_grid_trav_gpu as TT
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2
FAR, WALL = PR.FAR, 254
RESTATE_CELLS = 65 * 65                                          # the Python Dijkstra runs on windows up to this


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


def differ(tag, name, a, w):
    assert a.dtype == w.dtype and a.shape == w.shape, (tag, name)
    if a.tobytes() != w.tobytes():
        bad = np.argwhere(a != w)
        raise AssertionError("%s: %s differs in %d places, first %s: got %r, wanted %r" % (tag, name, len(bad), tuple(bad[0]), a[tuple(bad[0])],
                                                                                         w[tuple(bad[0])]))


def run(G, cost, goals, tag="", **kw):
    """device_plan against core_plan, and core_plan against the restatement on small windows; (pot, dir, rounds)"""
    cost = np.ascontiguousarray(cost, np.uint8)
    nz, nx = cost.shape
    plan = G.default_plan(**kw)
    pot, dir_, rounds = G.device_plan(nx, nz, plan, cost, goals)
    hp, hd, _ = G.core_plan(G.default_params(nx=nx, nz=nz), plan, cost, goals)
    differ(tag, "POT", pot, hp)
    differ(tag, "DIR", dir_, hd)
    if nx * nz <= RESTATE_CELLS:
        rp, rd, _ = PR.field(PR.PlanParams(**kw), cost, goals)
        differ(tag + " (header against restatement)", "POT", hp, rp)
        differ(tag + " (header against restatement)", "DIR", hd, rd)
    return pot, dir_, rounds


# ---- windows that put the edges everywhere -------------------------------------------------------------------------------
def windows(T):
    return [(1, 1), (1, 9), (9, 1), (3, 3), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, T + 1), (T + 1, 2 * T + 1), (257, 129)]


def four_tiles(nx, nz, T):
    """a goal in each of up to four different tiles"""
    return sorted({(min(nx - 1, x), min(nz - 1, y)) for x in (T // 2, T + T // 2) for y in (T // 2, T + T // 2)})


@pytest.mark.parametrize("k", range(10))
def test_patterns(G, k):
    T = G.PLAN_TILE
    nx, nz = windows(T)[k]
    rng = np.random.default_rng(1000 * nx + nz)
    ia, ib = np.meshgrid(np.arange(nx), np.arange(nz))
    middle, corner = [(nx // 2, nz // 2)], [(nx - 1, 0)]
    rand = TP.random_cost(rng, nx, nz, p_wall=0.2)
    rand[nz // 2, nx // 2] = 0
    last_row, last_col = np.where(ib == nz - 1, WALL, 0), np.where(ia == nx - 1, WALL, 0)
    cases = [("an open field", np.zeros((nz, nx)), middle, {}), ("an open field, a goal in a corner", np.zeros((nz, nx)), corner, {}),
             ("random prices", rand, middle, {}), ("random prices, unknown 30, four tiles", rand, four_tiles(nx, nz, T), dict(unknown=30)),
             ("a checkerboard", np.where((ia + ib) % 2 == 1, WALL, 0), middle + corner + [(0, 0)], {}),
             ("the last row impassable", last_row, [(0, 0)] + corner, {}), ("the last column impassable", last_col, [(0, nz - 1)], {}),
             ("goals in four tiles", np.zeros((nz, nx)), four_tiles(nx, nz, T), dict(neutral=1)),
             ("random prices, a horizon", rand, four_tiles(nx, nz, T), dict(max_cost=20000, neutral=255))]
    for name, cost, goals, kw in cases:
        pot, dir_, _ = run(G, cost, goals, "%d x %d, %s" % (nx, nz, name), **kw)
        if name == "an open field":
            assert (pot != FAR).all() and (dir_ <= 8).all()
        if name == "a checkerboard":
            assert set(np.unique(pot)) <= {0, FAR} and set(np.unique(dir_)) <= {8, 9}
        if name == "the last row impassable" and nz > 1:
            assert (pot[-1] == FAR).all() and (pot[:-1] != FAR).all()


# ---- mazes ---------------------------------------------------------------------------------------------------------------
def serpentine(n):
    """n x n: the even rows are corridors of one cell, the odd rows walls with one opening at alternating ends; the only
    route from (0, 0) runs through every corridor"""
    cost = np.zeros((n, n), np.uint8)
    cost[1::2] = WALL
    for k, b in enumerate(range(1, n, 2)):
        cost[b, n - 1 if k % 2 == 0 else 0] = 0
    return cost


def crossings(path, T):
    """how often a path steps from one tile into another"""
    t = path // T
    return int((np.abs(np.diff(t, axis=0)).sum(axis=1) != 0).sum())


def route_end(pot):
    b, a = np.unravel_index(np.argmax(np.where(pot == FAR, -1, pot)), pot.shape)
    return int(a), int(b)


@pytest.mark.parametrize("turned", [False, True])
def test_a_serpentine(G, turned):
    T = G.PLAN_TILE
    n = 4 * T
    cost = serpentine(n)
    cost = cost.T.copy() if turned else cost
    pot, dir_, rounds = run(G, cost, [(0, 0)], "serpentine")
    a, b = route_end(pot)
    path = G.core_path(dir_, a, b)
    corridor_cells = int((cost == 0).sum())
    assert len(path) == corridor_cells and pot[b, a] == 500 * (corridor_cells - 1)     # one route, edge steps of 500 only
    assert crossings(path, T) >= 3 * (n // 2) and rounds >= crossings(path, T)            # the lists of tiles did the work
    assert (pot[cost == 0] != FAR).all()


def spiral(n):
    """a corridor of one cell wound inwards from (0, 0) between walls of one cell"""
    c = np.full((n, n), WALL, np.uint8)
    a = b = 0
    da, db = 1, 0
    c[0, 0] = 0
    while True:
        for _ in range(2):
            x, y, x2, y2 = a + da, b + db, a + 2 * da, b + 2 * db
            if 0 <= x < n and 0 <= y < n and c[y, x] == WALL and not (0 <= x2 < n and 0 <= y2 < n and c[y2, x2] == 0):
                a, b = x, y
                c[b, a] = 0
                break
            da, db = -db, da
        else:
            return c


def test_a_spiral(G):
    T = G.PLAN_TILE
    n = 2 * T + 1
    cost = spiral(n)
    cells = int((cost == 0).sum())
    assert cells > n * n // 3
    for goal in ((0, 0), None):
        if goal is None:
            goal = route_end(pot)                                    # and back out from the innermost cell
        pot, dir_, rounds = run(G, cost, [goal], "spiral from %r" % (goal,))
        a, b = route_end(pot)
        path = G.core_path(dir_, a, b)
        assert len(path) == cells and pot[b, a] == 500 * (cells - 1) and crossings(path, T) > 8 and rounds > 8


def test_a_diagonal_wall(G):
    """the cells (i, i) are impassable: the only gaps are corners, which the corner rule closes; one edge gap opens it"""
    T = G.PLAN_TILE
    n = 2 * T + 1
    ia, ib = np.meshgrid(np.arange(n), np.arange(n))
    cost = np.where(ia == ib, WALL, 0).astype(np.uint8)
    pot, dir_, _ = run(G, cost, [(0, n - 1)], "closed")
    assert (pot[ia < ib] != FAR).all() and (pot[ia >= ib] == FAR).all()
    k = T                                                          # the gap lies on a tile's corner
    cost[k, k] = 0
    pot, dir_, _ = run(G, cost, [(0, n - 1)], "one gap")
    assert (pot[cost == 0] != FAR).all()
    for start in ((n - 1, 0), (k + 1, k), (n - 1, n - 2), (1, 0)):
        path = G.core_path(dir_, *start)
        assert [k, k] in path.tolist(), start                        # every route from the far side passes the gap


def test_a_horizon_inside_a_tile_and_on_its_border(G):
    T = G.PLAN_TILE
    cost = serpentine(4 * T)
    for reach in (T + T // 2, T - 1, T, 2 * T - 1, 4 * T - 1, 4 * T + 1):      # cells of the first corridor beyond the goal
        pot, dir_, _ = run(G, cost, [(0, 0)], "horizon %d" % reach, max_cost=500 * reach)
        want = np.full(cost.shape, FAR, np.int64)
        line = np.concatenate([np.stack([np.arange(4 * T), np.zeros(4 * T, int)], 1), [[4 * T - 1, 1]], np.stack([np.arange(4 * T)[::-1], np.full(4 * T, 2)], 1)])
        for i, (a, b) in enumerate(line[:reach + 1]):
            want[b, a] = 500 * i
        assert np.array_equal(pot, want), reach
    pot, _, _ = run(G, cost, [(0, 0)], "one below", max_cost=500 * T - 1)
    assert pot[0, T - 1] == 500 * (T - 1) and pot[0, T] == FAR and (pot != FAR).sum() == T


def test_the_largest_window_against_the_header(G):
    """1024 x 1024, random costs, three cells in ten impassable"""
    rng = np.random.default_rng(21)
    cost = TP.random_cost(rng, 1024, 1024, p_wall=0.3, p_unknown=0.02)
    goals = np.stack([rng.integers(0, 1024, 6), rng.integers(0, 1024, 6)], 1)
    cost[goals[:, 1], goals[:, 0]] = 0
    pot, dir_, rounds = run(G, cost, goals, "1024 x 1024")
    assert (pot != FAR).mean() > 0.4 and rounds > 16


def test_the_same_bytes_twice_and_under_a_permutation_of_the_goals(G):
    T = G.PLAN_TILE
    rng = np.random.default_rng(22)
    nx, nz = 3 * T + 5, 2 * T + 3
    cost = TP.random_cost(rng, nx, nz, p_wall=0.25)
    goals = TP.random_goals(rng, nx, nz, 40)
    goals = np.concatenate([goals, goals[:7]])                       # with duplicates, goals outside and goals on walls
    plan = G.default_plan(unknown=100)
    first = G.device_plan(nx, nz, plan, cost, goals)
    for other in (goals, goals[::-1], goals[rng.permutation(len(goals))]):
        again = G.device_plan(nx, nz, plan, cost, other)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    hp, hd, _ = G.core_plan(G.default_params(nx=nx, nz=nz), plan, cost, goals)
    assert first[0].tobytes() == hp.tobytes() and first[1].tobytes() == hd.tobytes()


# ---- through the object --------------------------------------------------------------------------------------------------
TRAV = dict(max_slope=4.0, inscribed=0.4, inflate=1.0, lethal=TR.L_OBSTACLE)     # reach 2: the cells beside a wall cost 210, 123


def pair(G, nx, nz, **pkw):
    P, Pc = TG.both(G, **TL.win_kw(nx, nz))
    ref, g = PR.Grid(P, TR.TravParams(**TRAV), PR.PlanParams(**pkw)), G.Grid(Pc)
    g.set_traversability(**TRAV)
    g.set_plan(**pkw)
    assert g.plan_params().asdict() == dict(neutral=ref.plan.neutral, unknown=ref.plan.unknown, max_cost=ref.plan.max_cost)
    return ref, g


def walls(nx, nz):
    """two walls across the window with a gap each, and a closed room in the corner (nx - 8 .. nx - 2, 1 .. 7)"""
    ia, ib = np.meshgrid(np.arange(nx), np.arange(nz))
    w = ((ia == nx // 3) & ~((ib >= 4) & (ib <= 7))) | ((ia == 2 * nx // 3) & ~((ib >= nz - 9) & (ib <= nz - 6)))
    room = (ia >= nx - 8) & (ia <= nx - 2) & (ib >= 1) & (ib <= 7)
    return w | (room & ~((ia >= nx - 7) & (ia <= nx - 3) & (ib >= 2) & (ib <= 6)))


def build(G, nx, nz, seed, **pkw):
    rng = np.random.default_rng(seed)
    ref, g = pair(G, nx, nz, **pkw)
    TT.add_both(g, ref, TT.fill(ref, rng, walls(nx, nz)))
    return ref, g, rng


def set_goals(g, ref, goals):
    g.set_goals(goals)
    ref.set_goals(goals)


def check(G, g, ref, tag="", path=()):
    """POT, DIR, the statistics and the plan image against the restatement on its own COST; returns its field"""
    f = ref.field()
    differ(tag, "COST", g.trav_plane(G.TRAV_COST), f["trav"]["cost"])
    differ(tag, "POT", g.plan_plane(G.PLAN_POT), f["pot"])
    differ(tag, "DIR", g.plan_plane(G.PLAN_DIR), f["dir"])
    st = g.plan_stats()
    assert st[:3] == (len(ref.goals), f["counted"], f["reached"]), (tag, st)
    differ(tag, "the plan image", g.render_plan(path), ref.render_plan(path, f))
    return f


def check_path(G, g, ref, f, xyz, tag=""):
    want = ref.path(xyz, f)
    got = g.path(xyz)
    assert got[0] == want[0] and got[2] == want[2] and np.array_equal(got[1], want[1]) and got[1].dtype == np.int32, (tag, got, want)
    assert g.path_len == len(want[1])
    return got


def goals_of(ref, nx, nz):
    """beyond both walls; with a duplicate, a goal on a wall, one in the closed room's wall and two outside the window"""
    o = np.array([ref.oa, ref.ob])
    return np.array([(nx - 3, nz - 3), (nx - 2, nz // 2), (nx - 3, nz - 3), (nx // 3, 0), (nx - 8, 3), (-1, 0), (nx, nz)]) + o


@pytest.mark.parametrize("shape", ["65 x 65", "(2T + 1) x (T + 1)"])
def test_scenes_of_walls_with_gaps(G, shape):
    T = G.PLAN_TILE
    nx, nz = (65, 65) if shape == "65 x 65" else (2 * T + 1, T + 1)
    ref, g, rng = build(G, nx, nz, 31)
    f = check(G, g, ref, "no goals")
    assert f["counted"] == 0 and f["reached"] == 0
    assert check_path(G, g, ref, f, TL.centre(ref, 1, 1), "no goals")[0] == G.PATH_UNREACHABLE
    set_goals(g, ref, goals_of(ref, nx, nz))
    f = check(G, g, ref, "goals")
    assert f["counted"] == 2 and g.plan_stats()[3] >= 1
    starts = [(1, 1), (0, nz - 1), (nx // 3 - 1, nz // 2), (nx // 2, 0), (nx // 2, nz - 1), (nx - 1, nz - 1), (nx // 3 + 1, 5)]
    starts += [(int(rng.integers(0, nx)), int(rng.integers(0, nz))) for _ in range(5)]
    found = 0
    for a, b in starts:
        st, cells, cost = check_path(G, g, ref, f, TL.centre(ref, a, b), "from (%d, %d)" % (a, b))
        if st == G.PATH_FOUND:
            found += 1
            assert tuple(cells[0]) == (a, b) and f["pot"][cells[-1][1], cells[-1][0]] == 0 and cost == f["pot"][b, a]
    assert found >= 7
    st, cells, cost = check_path(G, g, ref, f, TL.centre(ref, 1, 1), "the long way")
    assert st == G.PATH_FOUND and len(cells) > nx // 2
    differ("the path drawn", "the plan image", g.render_plan(cells), ref.render_plan(cells, f))
    assert (g.render_plan(cells) == 255).all(axis=2).sum() == len(cells)
    # cap: smaller than the path, 0, exactly the length
    for cap in (3, 0, len(cells), len(cells) + 5):
        got = g.path(TL.centre(ref, 1, 1), cap=cap)
        assert got[0] == G.PATH_FOUND and got[2] == cost and g.path_len == len(cells) and np.array_equal(got[1], cells[:cap]), cap
    # the start on a goal, on an obstacle, in the closed room, outside the window
    st, cells, cost = check_path(G, g, ref, f, TL.centre(ref, nx - 3, nz - 3), "on a goal")
    assert (st, len(cells), cost) == (G.PATH_FOUND, 1, 0)
    assert check_path(G, g, ref, f, TL.centre(ref, nx // 3, nz // 2), "on a wall")[::2] == (G.PATH_BLOCKED, FAR)
    assert check_path(G, g, ref, f, TL.centre(ref, nx - 5, 4), "in the room")[::2] == (G.PATH_UNREACHABLE, FAR)
    for a, b in ((-1, 0), (nx, 0), (0, -1), (0, nz)):
        assert check_path(G, g, ref, f, TL.centre(ref, a, b), "outside")[::2] == (G.PATH_OUTSIDE, FAR)


def test_scroll_goals_and_the_cache(G):
    nx = nz = 65
    ref, g, rng = build(G, nx, nz, 32)
    set_goals(g, ref, goals_of(ref, nx, nz))
    f = check(G, g, ref, "before")
    start = TL.centre(ref, 8, 20)
    st, route, cost = check_path(G, g, ref, f, start, "before")
    assert st == G.PATH_FOUND
    pot = g.plan_plane(G.PLAN_POT)
    assert g.plan_plane(G.PLAN_POT).tobytes() == pot.tobytes()         # nothing changed: the same plane, from the cache
    # path cells are global: after a scroll the same route comes back where it still lies inside the window
    g.scroll(3, -2)
    ref.scroll(3, -2)
    f2 = check(G, g, ref, "scrolled")
    st2, route2, cost2 = check_path(G, g, ref, f2, start, "scrolled")
    assert g.window() == (3, -2) and g.plan_stats()[0] == 7
    local = route - np.array([3, -2])
    assert ((local >= 0) & (local < 65)).all() and st2 == G.PATH_FOUND and np.array_equal(route2, route) and cost2 == cost
    # a new obstacle across the route changes the field
    a, b = route[len(route) // 2] - np.array([3, -2])
    TT.add_both(g, ref, TL.at_cells(ref, [a, a], [b, b], [0.0, 1.5]))
    f3 = check(G, g, ref, "an obstacle on the route")
    st3, route3, cost3 = check_path(G, g, ref, f3, start, "an obstacle on the route")
    assert f3["pot"][b, a] == FAR and cost3 >= cost and not np.array_equal(route3, route)
    # the traversability and the plan parameters each invalidate the field
    g.set_traversability(inflate=2.0)
    ref.T.inflate = np.float32(2.0)
    f4 = check(G, g, ref, "after set_traversability")
    assert f4["pot"].tobytes() != f3["pot"].tobytes()
    g.set_plan(neutral=10, unknown=40)
    ref.plan.neutral, ref.plan.unknown = 10, 40
    f5 = check(G, g, ref, "after set_plan")
    assert f5["pot"].tobytes() != f4["pot"].tobytes() and f5["reached"] > f4["reached"]     # the strips that entered are unknown
    g.set_plan(max_cost=3000)
    ref.plan.max_cost = 3000
    f6 = check(G, g, ref, "a horizon")
    assert 0 < f6["reached"] < f5["reached"]
    # clear forgets the goals; so does set_window
    g.clear()
    ref.clear()
    assert g.plan_stats() == (0, 0, 0, 0) and len(ref.goals) == 0
    check(G, g, ref, "cleared")
    g.set_goals([(1, 1)])
    g.set_window(0.0, 0.0)
    assert g.plan_stats()[0] == 0


def test_a_goal_that_scrolls_out_and_back(G):
    T = G.PLAN_TILE
    nx, nz = 2 * T + 1, T + 1
    ref, g, rng = build(G, nx, nz, 33, unknown=10)
    set_goals(g, ref, [(1, nz // 2)])
    f = check(G, g, ref, "inside")
    assert f["counted"] == 1 and f["reached"] > 100
    g.scroll(3, 0)
    ref.scroll(3, 0)
    f = check(G, g, ref, "scrolled out")
    assert f["counted"] == 0 and f["reached"] == 0 and g.plan_stats()[0] == 1
    g.scroll(-3, 0)
    ref.scroll(-3, 0)
    f = check(G, g, ref, "scrolled back")                              # its cell is unknown now, and passable at unknown = 10
    assert f["counted"] == 1 and f["reached"] > 100
    g.follow(TL.centre(ref, 10, 5), 4, 4)
    ref.follow(TL.centre(ref, 10, 5), 4, 4)
    check(G, g, ref, "followed")


# ---- failures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["malloc:1", "launch:1", "launch:2", "copy:1", "wait:1", "wait:2"])
def test_a_failed_plan_leaves_the_grid_and_the_goals(G, spec):
    """with the cost planes cached and a new object: malloc:1 is the planner's planes, copy:1 and wait:1 the upload of the
    goals, launch:1 the seed, launch:2 and wait:2 the first rounds"""
    nx, nz = 65, 65
    ref, g, rng = build(G, nx, nz, 34)
    set_goals(g, ref, goals_of(ref, nx, nz))
    TT.check(G, g, ref, "the cost planes")
    before = TL.snapshot(G, g)
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.plan_plane(G.PLAN_POT)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    assert TL.same(TL.snapshot(G, g), before)
    f = check(G, g, ref, spec + ": the call repeated")
    assert f["counted"] == 2
    # with the field cached: the walk's and the image's own launches
    for call in (lambda: g.path(TL.centre(ref, 1, 1)), lambda: g.render_plan([(1, 1)])):
        G.lib().svh_test_fail_at(b"launch:1")
        with pytest.raises(G.SvhError) as e:
            call()
        G.lib().svh_test_fail_at(None)
        assert e.value.code == HIP_ERR
        check(G, g, ref, spec + ": after a failed call on the cached field")
        check_path(G, g, ref, f, TL.centre(ref, 1, 1), spec)
    assert TL.same(TL.snapshot(G, g), before)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte(G, hip):
    nx, nz = 65, 33
    ref, g, rng = build(G, nx, nz, 35)
    set_goals(g, ref, [(nx - 2, nz - 2)])
    f = check(G, g, ref, "before")
    L = g._L
    buf = np.full(nx * nz * 4, 0xAB, np.uint8)
    dev = Dev(hip, nx * nz * 4 + 16)
    for kw in TP.BAD:
        p = G.default_plan(**kw)
        assert L.svh_grid_set_plan(g._h, C.byref(p)) == BAD_ARG and "svh_grid_set_plan" in G.last_error(), kw
    assert g.plan_params().asdict() == dict(neutral=50, unknown=-1, max_cost=0x7FFFFFFE)
    one, far, neg = np.array([[1, 1]], np.int32), np.array([[0, 2 ** 20]], np.int32), np.array([[-(2 ** 20), 0]], np.int32)
    xyz, nan = np.array(TL.centre(ref, 1, 1)), np.array([0.0, np.nan, 0.0])
    n, cost = C.c_int64(-7), C.c_int32(-7)
    calls = [lambda: L.svh_grid_set_plan(g._h, None), lambda: L.svh_grid_get_plan(g._h, None),
             lambda: L.svh_grid_plan_set_goals(g._h, one.ctypes.data, -1), lambda: L.svh_grid_plan_set_goals(g._h, one.ctypes.data, 65537),
             lambda: L.svh_grid_plan_set_goals(g._h, None, 1), lambda: L.svh_grid_plan_set_goals(g._h, far.ctypes.data, 1),
             lambda: L.svh_grid_plan_set_goals(g._h, neg.ctypes.data, 1), lambda: L.svh_grid_plan_set_goal(g._h, None),
             lambda: L.svh_grid_plan_set_goal(g._h, nan.ctypes.data),
             lambda: L.svh_grid_get_plan_plane(g._h, 2, buf.ctypes.data, 0), lambda: L.svh_grid_get_plan_plane(g._h, -1, buf.ctypes.data, 0),
             lambda: L.svh_grid_get_plan_plane(g._h, 0, None, 0), lambda: L.svh_grid_get_plan_plane(g._h, G.PLAN_POT, dev.addr + 1, 1),
             lambda: L.svh_grid_get_plan_stats(g._h, None),
             lambda: L.svh_grid_plan_path(g._h, nan.ctypes.data, buf.ctypes.data, 4, C.addressof(n), C.addressof(cost)),
             lambda: L.svh_grid_plan_path(g._h, None, buf.ctypes.data, 4, C.addressof(n), C.addressof(cost)),
             lambda: L.svh_grid_plan_path(g._h, xyz.ctypes.data, None, 4, C.addressof(n), C.addressof(cost)),
             lambda: L.svh_grid_plan_path(g._h, xyz.ctypes.data, buf.ctypes.data, -1, C.addressof(n), C.addressof(cost)),
             lambda: L.svh_grid_plan_path(g._h, xyz.ctypes.data, buf.ctypes.data, 4, None, C.addressof(cost)),
             lambda: L.svh_grid_plan_path(g._h, xyz.ctypes.data, buf.ctypes.data, 4, C.addressof(n), None),
             lambda: L.svh_grid_render_plan(g._h, one.ctypes.data, 1, None, 0), lambda: L.svh_grid_render_plan(g._h, None, 1, buf.ctypes.data, 0),
             lambda: L.svh_grid_render_plan(g._h, one.ctypes.data, -1, buf.ctypes.data, 0)]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG and "svh_grid" in G.last_error(), k
    assert (buf == 0xAB).all() and (dev.get() == 0xEE).all() and (n.value, cost.value) == (-7, -7)
    assert g.plan_stats()[:3] == (1, f["counted"], f["reached"])
    check(G, g, ref, "after")
    # device pointers: POT, DIR and the image, nothing beyond them
    for which, name, nbytes in ((G.PLAN_POT, "pot", 4 * nx * nz), (G.PLAN_DIR, "dir", nx * nz)):
        out = Dev(hip, nbytes + 16)
        g.plan_plane(which, device_ptr=out.addr)
        got = out.get()
        assert got[:nbytes].tobytes() == f[name].tobytes() and (got[nbytes:] == 0xEE).all(), name
    out = Dev(hip, 3 * nx * nz + 16)
    g.render_plan([(1, 1), (2, 2)], device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:3 * nx * nz].reshape(nz, nx, 3), ref.render_plan([(1, 1), (2, 2)], f)) and (got[3 * nx * nz:] == 0xEE).all()


def test_planning_needs_a_traversability_that_fits(G):
    """cells of 5 mm: the default inflation radius would be 300 cells; the planner refuses as svh_grid_get_trav does"""
    g = G.Grid(G.default_params(nx=9, nz=9, cell=0.005, x0=0.0, z0=0.0, T=R.frame_camera(0.0), min_points=1))
    g.add_points(np.array([[0.0225, 0.0, 0.0225, 0.5]], np.float32))
    g.set_goals([(4, 4)])
    buf = np.full(81 * 4, 0xAB, np.uint8)
    n, cost = C.c_int64(-7), C.c_int32(-7)
    xyz = np.array([0.0225, 0.0, 0.0225])
    L = g._L
    for call in (lambda: L.svh_grid_get_plan_plane(g._h, 0, buf.ctypes.data, 0), lambda: L.svh_grid_get_plan_stats(g._h, buf.ctypes.data),
                 lambda: L.svh_grid_plan_path(g._h, xyz.ctypes.data, buf.ctypes.data, 4, C.addressof(n), C.addressof(cost)),
                 lambda: L.svh_grid_render_plan(g._h, None, 0, buf.ctypes.data, 0)):
        assert call() == BAD_ARG and "svh_grid_set_traversability" in G.last_error()
    assert (buf == 0xAB).all()
    g.set_traversability(inscribed=0.004, inflate=0.02)
    g.set_plan(unknown=0)
    pot = g.plan_plane(G.PLAN_POT)
    assert pot[4, 4] == 0 and pot[4, 5] == 500 and g.path(xyz)[0] == G.PATH_FOUND


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------
def test_pipeline_grid_plan(G, tmp_path, monkeypatch, capsys):
    """--grid-local DIR --grid-cost DIR2 --grid-plan DIR3 on the two golden frames: one plan image and one line of plan.jsonl
    per frame, the restatement's after the same steps"""
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
    d, d2, d3 = str(tmp_path / "loc"), str(tmp_path / "cost"), str(tmp_path / "plan")
    common = ["--grid-slope", "0.3", "--grid-inflate", "2.0", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-plan", d3,
                                      "--grid-goal-ahead", "10"] + common)
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("plan: goals 10 m ahead, a route in ") and "2 images and plan.jsonl" in l for l in out), out[-4:]
    assert sorted(os.listdir(d3)) == ["plan.jsonl"] + ["plan_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(d3, "plan.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = PR.Grid(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0), TR.TravParams(max_slope=0.3, inflate=2.0), PR.PlanParams(unknown=100))
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre_ = p.H_total[:3, 3]
        ref.follow(centre_, 48, 80)
        ref.add_from(p.view.points(p.view.count(view.LISTS) - 1), centre_)
        ref.set_goals([(ref.oa + ia, ref.ob + 80 + 40) for ia in range(96)])     # the camera stands in row 80; 10 m are 40 cells
        f = ref.field()
        status, cells, cost = ref.path(centre_, f)
        assert lines[k] == dict(frame=k, status=status, length=len(cells), cost=cost), (k, lines[k])
        img = read_ppm(os.path.join(d3, "plan_%06d.ppm" % k))
        assert img.shape == (160, 96, 3) and np.array_equal(img, ref.render_plan(cells, f)), k
        k += 1
    assert k == 2 and len(lines) == 2 and f["counted"] > 10 and f["reached"] > 500
    # --grid-plan is refused without --grid-cost, --grid-goal-ahead without --grid-plan
    for argv in (["--grid-local", d, "--grid-plan", d3], ["--grid-local", d, "--grid-cost", d2, "--grid-goal-ahead", "10"],
                 ["--grid-local", d, "--grid-cost", d2, "--grid-plan", d3, "--grid-goal-ahead", "-1"]):
        monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py"] + argv + common)
        with pytest.raises(SystemExit):
            SP.main()
