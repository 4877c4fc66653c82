"""GPU: the pose planner's kernels (stereo-vision_amd/csrc/grid_pose_kernels.hip) against the header, byte for byte.

svh_test_grid_pose_device runs k_grid_pose_foot, the seed, the goals, the tiled relaxation with the engine's round loop and
k_grid_pose_dir on a caller's COST plane; svh_test_grid_pose runs the loops of csrc/grid_pose_core.h on the host.  Small windows
are compared with tests/grid_pose_ref.py as well.  The entries of include/svh_grid_pose.h are driven on objects whose COST plane
the device computed (tests/test_grid_trav_gpu.py pins that plane): what they return is compared with the header on that plane.

Fields are indexed [d, ib, ia]; a state is (a, b, d)."""
import ctypes as C

import numpy as np
import pytest

import grid_pose_ref as QR
import grid_roll_ref as RR
import helpers as H
import test_grid_local_gpu as TL
import test_grid_plan_gpu as PG
import test_grid_pose as TQ
import test_grid_trav_gpu as TT
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2
FAR, WALL, CELL = QR.FAR, 254, TQ.CELL
POINT, BAR = TQ.POINT, TQ.BAR
RESTATE_CELLS = 33 * 18                                          # the Python restatement runs on windows up to this
T = 16                                                           # the tile side of k_grid_pose_relax
differ = PG.differ


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


def run(G, rkw, cost, goals, tag="", cell=CELL, oa=0, ob=0, **kw):
    """device_pose against core_pose, and core_pose against the restatement on small windows; (cf, pot, dir, (counted, reached, rounds))"""
    cost = np.ascontiguousarray(cost, np.uint8)
    nz, nx = cost.shape
    roll, pose = G.default_roll(**rkw), G.default_pose(**kw)
    cf, pot, dir_, st = G.device_pose(roll, pose, cell, cost, goals, oa, ob)
    hc, hp, hd, counted = G.core_pose(roll, pose, cell, cost, goals, oa, ob)
    differ(tag, "CF", cf, hc)
    differ(tag, "PPOT", pot, hp)
    differ(tag, "PDIR", dir_, hd)
    assert st[:2] == (counted, int((hp != FAR).sum())), (tag, st, counted)
    if nx * nz <= RESTATE_CELLS:
        rc, rp, rd, rn = QR.field(RR.RollParams(**rkw), QR.PoseParams(**kw), TQ.lists_of(rkw, cell), cost, goals, oa, ob)
        differ(tag + " (header against restatement)", "CF", hc, rc)
        differ(tag + " (header against restatement)", "PPOT", hp, rp)
        differ(tag + " (header against restatement)", "PDIR", hd, rd)
        assert rn == counted
    return cf, pot, dir_, st


# ---- windows that put the edges everywhere -------------------------------------------------------------------------------
WINDOWS = [(1, 1), (1, 17), (16, 16), (17, 17), (33, 18), (257, 129)]


def tile_goals(nx, nz):
    """on a tile's corner cells (both sides of it), on a tile's edge, in the window's corner and outside it"""
    c = [(T - 1, T - 1, -1), (T, T, 1), (T, 5, -1), (5, T - 1, 6), (nx - 1, nz - 1, -1), (nx, 0, -1), (0, 0, 3)]
    return np.array([(min(a, nx), min(b, nz - 1), d) for a, b, d in c], np.int32)


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_windows(G, nx, nz):
    rng = np.random.default_rng(100 * nx + nz)
    cost = TQ.random_cost(rng, nx, nz, lethal=0.08)
    goals = tile_goals(nx, nz)
    for k, (rkw, kw) in enumerate([(POINT, {}), (BAR, {}), (BAR, dict(reverse=30, spin=500)), (POINT, dict(max_cost=6000, turn=0))]):
        cf, pot, dir_, st = run(G, rkw, cost, goals, "%d x %d, case %d" % (nx, nz, k), **kw)
        if k == 0 and nx * nz > 1:
            assert st[0] >= 1 and st[1] > st[0]
    if nx >= 17 and nz >= 17:
        run(G, BAR, cost, goals + (7, -9, 0), "offsets", oa=7, ob=-9)


def test_a_turn_into_the_diagonal_neighbour_tile(G):
    """the one goal state (16, 16, 2) is the corner cell of tile (1, 1); (15, 15, 1) in tile (0, 0) reaches it by forward and left,
    700 + 100, and only the corner cell of its tile borders that tile"""
    free = np.zeros((33, 33), np.uint8)
    _, pot, dir_, st = run(G, POINT, free, [(16, 16, 2)])
    assert pot[1, 15, 15] == 800 and dir_[1, 15, 15] == 1 and pot[2, 15, 16] == 500 and pot[3, 15, 17] == 800 and dir_[3, 15, 17] == 2
    assert pot[1, 14, 14] == 1500 and st[0] == 1
    _, pot, dir_, _ = run(G, POINT, free, [(15, 15, 6)], reverse=0)         # and back across the same corner, reversing
    assert pot[5, 16, 16] == 800 and pot[6, 16, 15] == 500 and pot[6, 14, 15] == 500 and dir_[6, 14, 15] == 3


def test_a_directed_dead_end(G):
    """a corridor one cell wide along a, b = 5, a = 0 .. 20, all headings of (0, 5) goals.  A point facing up the corridor can only
    drive on to its end; backing down it needs reverse.  The corridor crosses the tile border at a = 16"""
    cost = np.full((18, 33), WALL, np.uint8)
    cost[5, :21] = 0
    _, pot, _, _ = run(G, POINT, cost, [(0, 5, -1)])
    assert (pot[0, 5, :21] == [0] + [FAR] * 20).all() and list(pot[4, 5, :21]) == [500 * a for a in range(21)]
    _, pot, dir_, _ = run(G, POINT, cost, [(0, 5, -1)], reverse=50)
    assert list(pot[0, 5, :21]) == [550 * a for a in range(21)] and (dir_[0, 5, 1:21] == 3).all()


def test_the_default_car_on_cells_of_20_cm(G):
    rng = np.random.default_rng(7)
    cost = np.where(rng.random((64, 64)) < 0.004, WALL, rng.integers(0, 60, (64, 64))).astype(np.uint8)
    car = dict()
    cf, pot, dir_, st = run(G, car, cost, [(32, 32, -1), (10, 40, 16 // 8)], cell=0.2)
    assert st[0] >= 1 and st[1] > 2000 and (cf == 255).any() and (cf < 60).any()
    run(G, car, cost, [(32, 32, -1)], cell=0.2, reverse=200, spin=3000)


def test_a_footprint_too_long_for_the_staged_tile(G):
    """a bar of 241 cells: along a diagonal its list spans 171 x 171 cells, the staged region would have 187 x 187 bytes, above the
    32 KiB of k_grid_pose_foot, which then reads COST from global memory; along an axis it spans 241 x 1 and is staged"""
    rng = np.random.default_rng(8)
    cost = np.where(rng.random((300, 300)) < 0.0005, WALL, 0).astype(np.uint8)
    long_bar = dict(front=60.0, rear=60.0, half_width=0.0, headings_m=1)
    lists = TQ.lists_of(long_bar)
    assert len(lists[0]) == 241 and np.ptp(lists[1][:, 0]) == 170 and (16 + 170) ** 2 > 32 * 1024 > (16 + 240) * 16
    cf, pot, _, st = run(G, long_bar, cost, [(150, 150, -1)])
    assert (cf[1] != 255).any() and (cf[0] != 255).any() and st[0] >= 1


def test_the_same_bytes_twice_and_under_a_permutation_of_the_goals(G):
    rng = np.random.default_rng(9)
    cost = TQ.random_cost(rng, 70, 50, lethal=0.08)
    goals = np.stack([rng.integers(0, 70, 12), rng.integers(0, 50, 12), rng.integers(-1, 8, 12)], 1).astype(np.int32)
    a = run(G, BAR, cost, goals, reverse=80)
    b = run(G, BAR, cost, goals[::-1], reverse=80)
    c = run(G, BAR, cost, goals, reverse=80)
    for k in range(3):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes()
    assert a[3][:2] == b[3][:2] == c[3][:2]


# ---- the entries on an object --------------------------------------------------------------------------------------------
VEHICLE = dict(front=1.0, rear=0.5, half_width=0.25, headings_m=4)         # 4 x 1 cells of 0.5 m


def build(G, nx, nz, seed, rkw=VEHICLE, **kw):
    ref, g, rng = PG.build(G, nx, nz, seed)
    g.set_roll(**rkw)
    g.set_pose(**kw)
    return ref, g, rng


def expect(G, g):
    """the header on the object's own COST plane, vehicle, parameters and offsets; `goals` as they were given to the object"""
    cost, (oa, ob) = g.trav_plane(G.TRAV_COST), g.window()
    return G.core_pose(g.roll_params()[0], g.pose_params(), CELL, cost, g._goals, oa, ob)


def set_goals(g, goals):
    g._goals = np.asarray(goals, np.int32).reshape(-1, 3)
    g.pose_set_goals(g._goals)


def check(G, g, tag="", path=()):
    cf, pot, dir_, counted = expect(G, g)
    differ(tag, "CF", g.pose_plane(G.POSE_CF), cf)
    differ(tag, "PPOT", g.pose_plane(G.POSE_POT), pot)
    differ(tag, "PDIR", g.pose_plane(G.POSE_DIR), dir_)
    st = g.pose_stats()
    assert st[:3] == (len(g._goals), counted, int((pot != FAR).sum())), (tag, st, counted)
    rp = g.roll_params()[0]
    price = QR.prices(QR.PoseParams(**g.pose_params().asdict()), rp.stop_cost, cf)
    oa, ob = g.window()
    differ(tag, "the pose image", g.render_pose(path), QR.overlay(g.render_cost(), price, g._goals, path, oa, ob))
    return cf, pot, dir_, counted


def check_path(G, g, f, a, b, d, tag=""):
    """svh_grid_pose_path from the window state (a, b, d) against the header's walk; every pose passes svh_grid_footprint_cost and
    the weights between the poses sum to the cost"""
    cf, pot, dir_, _ = f
    (oa, ob), rp = g.window(), g.roll_params()[0]
    xyz = [(oa + a + 0.5) * CELL, 0.0, (ob + b + 0.5) * CELL]
    status, poses, cost = g.pose_path(xyz, d)
    want, ln = G.core_pose_walk(dir_, a, b, d, rp.headings_m, oa, ob)
    assert np.array_equal(poses, want) and g.pose_path_len == ln and poses.dtype == np.int32, (tag, poses[:4], want[:4])
    assert cost == pot[d, b, a], tag
    if status == G.PATH_FOUND:
        F = g.footprint_cost(poses)
        assert len(poses) >= 1 and (F >= 0).all() and (F < rp.stop_cost).all() and (F <= 252).all(), tag
        price = QR.prices(QR.PoseParams(**g.pose_params().asdict()), rp.stop_cost, cf)
        assert QR.path_cost(QR.PoseParams(**g.pose_params().asdict()), price, poses, rp.headings_m, oa, ob) == cost, tag
        assert pot[poses[-1][2] // rp.headings_m, poses[-1][1] - ob, poses[-1][0] - oa] == 0
    else:
        assert len(poses) == 0 and status == (G.PATH_BLOCKED if cf[d, b, a] > 252 else G.PATH_UNREACHABLE), (tag, status)
    return status, poses, cost


def far_goals(g, nx, nz):
    oa, ob = g.window()
    return np.array([(nx - 3, nz - 3, -1), (nx - 3, nz - 3, 2), (nx - 2, nz // 2, -1), (nx // 3, 0, -1), (-1, 0, 0), (nx, nz, -1)]) + (oa, ob, 0)


def test_cf_is_svh_grid_footprint_cost(G):
    nx, nz = 40, 33
    ref, g, rng = build(G, nx, nz, 41)
    cf = g.pose_plane(G.POSE_CF)
    oa, ob = g.window()
    m = g.roll_params()[0].headings_m
    poses = np.array([(oa + a, ob + b, d * m) for d in range(8) for b in range(nz) for a in range(nx)], np.int32)
    F = g.footprint_cost(poses).reshape(8, nz, nx)
    differ("CF", "against svh_grid_footprint_cost", cf, np.where(F < 0, 255, F).astype(np.uint8))
    assert (F < 0).any() and (F == 0).any() and (F >= 253).any()


def test_scenes_of_walls_with_gaps_and_their_paths(G):
    nx, nz = 65, 65
    ref, g, rng = build(G, nx, nz, 42, reverse=150)
    set_goals(g, far_goals(g, nx, nz))
    f = check(G, g, "walls")
    assert f[3] >= 8
    found = 0
    for a, b, d in ((8, 20, 0), (8, 20, 4), (3, 60, 6), (30, 30, 1), (nx // 3, 10, 0), (nx - 5, 4, 2)):
        status, poses, cost = check_path(G, g, f, a, b, d, "from (%d, %d, %d)" % (a, b, d))
        found += status == G.PATH_FOUND
    assert found >= 2                                                        # the two starts left of both walls at the least
    status, poses, cost = check_path(G, g, f, 8, 20, 0)
    check(G, g, "with a path", poses)
    assert g.pose_path(TL.centre(ref, 8, 20), 0, cap=3)[1].shape == (3, 3) and g.pose_path_len == len(poses)
    assert g.pose_path(TL.centre(ref, -1, 0), 0)[::2] == (G.PATH_OUTSIDE, FAR)
    assert g.pose_heading_of([1.0, 0.0, 0.0]) == 0 and g.pose_heading_of([0.0, 0.0, 1.0]) == 2 and g.pose_heading_of([-1.0, 5.0, -1.1]) == 5


def gap_object(G, rkw):
    """9 x 9 cells, a wall along b = 4 with the one free cell (4, 4), nothing inflated beyond the wall's own cells"""
    import grid_plan_ref as PR
    import grid_trav_ref as TR
    import test_grid as TG
    P, Pc = TG.both(G, **TL.win_kw(9, 9))
    trav = dict(max_slope=4.0, inscribed=0.1, inflate=0.2, lethal=TR.L_OBSTACLE)
    ref, g = PR.Grid(P, TR.TravParams(**trav), PR.PlanParams()), G.Grid(Pc)
    g.set_traversability(**trav)
    ia, ib = np.meshgrid(np.arange(9), np.arange(9))
    TT.add_both(g, ref, TT.fill(ref, np.random.default_rng(3), (ib == 4) & (ia != 4)))
    g.set_roll(**rkw)
    return g


def test_the_gap_scene_through_the_object(G):
    """the point's field and the bar's on one scene, every heading of (4, 7) a goal: across the gap the bar lies on the wall, so its
    states of heading 0 and 4 in the gap cell are impassable; from (4, 1) the bar arrives at heading 2 alone, the point at every
    heading but 6, straight away from the wall"""
    fields = {}
    for name, rkw in (("point", POINT), ("bar", BAR)):
        g = gap_object(G, rkw)
        cost = g.trav_plane(G.TRAV_COST)
        assert (cost[4, [3, 5]] >= 253).all() and cost[4, 4] <= 252 and (cost[[3, 5], 4] <= 252).all()
        set_goals(g, [(4, 7, -1)])
        fields[name] = check(G, g, name)
    (pc, pp, _, pn), (bc, bp, _, bn) = fields["point"], fields["bar"]
    assert pn == bn == 8
    assert (pc[[0, 4], 4, 4] <= 252).all() and (bc[[0, 4], 4, 4] >= 253).all() and (bp[[0, 4], 4, 4] == FAR).all()
    assert bp[2, 1, 4] != FAR and (bp[[0, 1, 3, 4, 5, 6, 7], 1, 4] == FAR).all()
    assert (pp[[0, 1, 2, 3, 4, 5, 7], 1, 4] != FAR).all() and pp[6, 1, 4] == FAR
    assert (pp[:, :4] != FAR).sum() > (bp[:, :4] != FAR).sum() > 0


def test_scroll_obstacle_clear_and_another_vehicle(G):
    nx = nz = 65
    ref, g, rng = build(G, nx, nz, 43)
    set_goals(g, far_goals(g, nx, nz))
    f = check(G, g, "before")
    assert g.pose_plane(G.POSE_POT).tobytes() == f[1].tobytes()               # nothing changed: the same planes, from the cache
    status, route, cost = check_path(G, g, f, 8, 20, 0, "before")
    assert status == G.PATH_FOUND
    # what the planner, the candidates and the prediction are told does not reach this layer: with every launch failing, the
    # planes still come, from the cache
    g.set_plan(neutral=10)
    g.set_goals([(3, 3)])
    g.set_candidates(np.zeros((1, 1, 1, 3), np.int32))
    g.set_predict(slots=4)
    G.lib().svh_test_fail_at(b"launch:1")
    assert g.pose_plane(G.POSE_POT).tobytes() == f[1].tobytes() and g.pose_plane(G.POSE_CF).tobytes() == f[0].tobytes()
    G.lib().svh_test_fail_at(None)
    # new goals leave CF in its cache: the first launch is then the seed's.  After it failed the whole layer is computed again
    set_goals(g, far_goals(g, nx, nz)[:3])
    G.lib().svh_test_fail_at(b"launch:1")
    with pytest.raises(G.SvhError):
        g.pose_plane(G.POSE_POT)
    G.lib().svh_test_fail_at(None)
    check(G, g, "three goals")
    set_goals(g, far_goals(g, nx, nz))
    # a new obstacle across the route changes the field
    a, b = route[len(route) // 2][:2]
    TT.add_both(g, ref, TL.at_cells(ref, [a, a], [b, b], [0.0, 1.5]))
    f2 = check(G, g, "an obstacle on the route")
    status2, route2, cost2 = check_path(G, g, f2, 8, 20, 0, "an obstacle on the route")
    assert (f2[1][:, b, a] == FAR).all() and cost2 >= cost and not np.array_equal(route2, route)
    # goals and poses are global: after a scroll the goals are still the six, the start is the same global cell, and the field is
    # the header's under the new offsets (the strips that entered are unknown, and the far goals now lie beside them)
    g.scroll(3, -2)
    ref.scroll(3, -2)
    f3 = check(G, g, "scrolled")
    status3, route3, cost3 = check_path(G, g, f3, 8 - 3, 20 + 2, 0, "scrolled")
    assert g.window() == (3, -2) and g.pose_stats()[0] == 6 and f3[1].tobytes() != f2[1].tobytes()
    assert status3 != G.PATH_FOUND or tuple(route3[0]) == tuple(route[0])
    # another footprint, then other parameters of this layer
    g.set_roll(front=0.0, rear=0.0, half_width=0.0)
    f4 = check(G, g, "a point")
    assert (f4[1] != FAR).sum() > (f3[1] != FAR).sum() and f4[0].tobytes() != f3[0].tobytes()
    g.set_roll(stop_cost=150)
    f5 = check(G, g, "stop_cost 150")
    assert (f5[1] != FAR).sum() < (f4[1] != FAR).sum()
    g.set_pose(spin=40, max_cost=9000)
    f6 = check(G, g, "spin and a horizon")
    assert f6[1].tobytes() != f5[1].tobytes() and f6[0].tobytes() == f5[0].tobytes()
    # clear forgets the goals; so does set_window
    g.clear()
    ref.clear()
    g._goals = np.zeros((0, 3), np.int32)
    assert g.pose_stats() == (0, 0, 0, 0)
    f7 = check(G, g, "cleared")
    assert (f7[1] == FAR).all() and (f7[0] == 254).sum() > 0                   # everything is unknown: CF 254 at unknown_cost 254
    g.pose_set_goals([(1, 1, -1)])
    g.set_window(0.0, 0.0)
    assert g.pose_stats()[0] == 0


# ---- failures ------------------------------------------------------------------------------------------------------------
# the least number of sites of each kind an entry has, from the engine's text.  svh_grid_get_pose_plane on a new object with the cost
# planes cached: the planes, the tile lists, the control words and their pinned copy; the goals' upload, the two fills, a readback
# per batch of rounds, the last readback, the copy of the plane; k_grid_pose_foot, the seed with the goals, a batch of rounds,
# k_grid_pose_dir; the waits of the upload, of a batch, of the last readback and of the plane's copy.  svh_grid_pose_path on a cached
# field: the poses and the three words with their pinned copy; the walk; the words' readback and the poses' copy, a wait each.
# svh_grid_render_pose: the poses' device buffer (the image's buffers and the pinned staging exist by then: the snapshot before the
# armed call renders, and the goals went through the staging); the poses' upload and the image's copy with their waits; the one
# check of its three launches
LEAST = {"plane": dict(malloc=4, copy=6, launch=4, wait=4), "path": dict(malloc=2, copy=2, launch=1, wait=2),
         "render": dict(malloc=1, copy=2, launch=1, wait=2)}


@pytest.mark.parametrize("kind", ["malloc", "copy", "launch", "wait"])
@pytest.mark.parametrize("entry", ["plane", "path", "render"])
def test_an_error_at_every_site_leaves_the_grid_and_the_goals(G, entry, kind):
    """the n-th allocation, copy (fills included), launch check or wait of the entry fails through the host-side hook, for n = 1, 2, ...
    until the entry succeeds with the hook still armed: every site of that kind is hit, whatever the number of rounds.  Each n gets a
    new object -- a buffer that one attempt allocated would not be allocated by the next -- with the cost planes cached, and for the
    path and the image the field too.  After the failure the grid is as it was and the same call is right.  No device fault is
    provoked: the hook returns an error instead of making the call"""
    nx, nz = 40, 33
    hits = 0
    for n in range(1, 200):
        ref, g, rng = build(G, nx, nz, 44)
        set_goals(g, far_goals(g, nx, nz))
        g.trav_plane(G.TRAV_COST)
        if entry != "plane":
            g.pose_plane(G.POSE_POT)
        before = TL.snapshot(G, g)
        call = {"plane": lambda: g.pose_plane(G.POSE_POT), "path": lambda: g.pose_path(TL.centre(ref, 1, 1), 0),
                "render": lambda: g.render_pose([(1, 1, 0), (2, 2, 4)])}[entry]
        G.lib().svh_test_fail_at(("%s:%d" % (kind, n)).encode())
        try:
            call()
            failed = False
        except G.SvhError as e:
            assert e.code == HIP_ERR, (entry, kind, n, e.code)
            failed = True
        G.lib().svh_test_fail_at(None)
        assert TL.same(TL.snapshot(G, g), before), (entry, kind, n)
        f = check(G, g, "%s, %s:%d: the call repeated" % (entry, kind, n), [(1, 1, 0), (2, 2, 4)])
        check_path(G, g, f, 1, 1, 0, "%s, %s:%d" % (entry, kind, n))
        assert f[3] >= 8
        g.close()
        if not failed:
            break
        hits += 1
    else:
        raise AssertionError("%s still fails at %s:%d" % (entry, kind, n))
    print("%s: %d sites of kind %s" % (entry, hits, kind))
    assert hits >= LEAST[entry][kind], (entry, kind, hits)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte(G, hip):
    nx, nz = 40, 33
    ref, g, rng = build(G, nx, nz, 45)
    set_goals(g, [(nx - 2, nz - 2, -1)])
    f = check(G, g, "before")
    L = g._L
    states = 8 * nx * nz
    buf = np.full(states * 4, 0xAB, np.uint8)
    dev = Dev(hip, states * 4 + 16)
    for kw in TQ.BAD:
        p = G.default_pose(**kw)
        assert L.svh_grid_set_pose(g._h, C.byref(p)) == BAD_ARG and "svh_grid_set_pose" in G.last_error(), kw
    assert g.pose_params().asdict() == dict(neutral=50, max_cost=0x7FFFFFFE, turn=100, reverse=-1, spin=-1)
    tri = lambda *t: np.array([t], np.int32)
    one, far, neg, h8, hm2 = tri(1, 1, 0), tri(0, 2 ** 20, 0), tri(-(2 ** 20), 0, 0), tri(1, 1, 8), tri(1, 1, -2)
    xyz, nan = np.array(TL.centre(ref, 1, 1)), np.array([0.0, np.nan, 0.0])
    n, cost, d = C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    path = lambda s=xyz.ctypes.data, d_=0, out=buf.ctypes.data, cap=4, ln=C.addressof(n), c=C.addressof(cost): L.svh_grid_pose_path(g._h, s, d_, out, cap, ln, c)
    calls = [lambda: L.svh_grid_set_pose(g._h, None), lambda: L.svh_grid_get_pose(g._h, None),
             lambda: L.svh_grid_pose_set_goals(g._h, one.ctypes.data, -1), lambda: L.svh_grid_pose_set_goals(g._h, one.ctypes.data, 65537),
             lambda: L.svh_grid_pose_set_goals(g._h, None, 1), lambda: L.svh_grid_pose_set_goals(g._h, far.ctypes.data, 1),
             lambda: L.svh_grid_pose_set_goals(g._h, neg.ctypes.data, 1), lambda: L.svh_grid_pose_set_goals(g._h, h8.ctypes.data, 1),
             lambda: L.svh_grid_pose_set_goals(g._h, hm2.ctypes.data, 1), lambda: L.svh_grid_pose_set_goal(g._h, None, 0),
             lambda: L.svh_grid_pose_set_goal(g._h, nan.ctypes.data, 0), lambda: L.svh_grid_pose_set_goal(g._h, xyz.ctypes.data, 8),
             lambda: L.svh_grid_get_pose_plane(g._h, 3, buf.ctypes.data, 0), lambda: L.svh_grid_get_pose_plane(g._h, -1, buf.ctypes.data, 0),
             lambda: L.svh_grid_get_pose_plane(g._h, 0, None, 0), lambda: L.svh_grid_get_pose_plane(g._h, G.POSE_POT, dev.addr + 1, 1),
             lambda: L.svh_grid_get_pose_stats(g._h, None),
             lambda: L.svh_grid_pose_heading_of(g._h, nan.ctypes.data, C.addressof(d)), lambda: L.svh_grid_pose_heading_of(g._h, xyz.ctypes.data, None),
             lambda: L.svh_grid_pose_heading_of(g._h, np.array([0.0, 1.0, 0.0]).ctypes.data, C.addressof(d)),
             lambda: path(s=nan.ctypes.data), lambda: path(s=None), lambda: path(out=None), lambda: path(cap=-1), lambda: path(ln=None),
             lambda: path(c=None), lambda: path(d_=8), lambda: path(d_=-1),
             lambda: L.svh_grid_render_pose(g._h, one.ctypes.data, 1, None, 0), lambda: L.svh_grid_render_pose(g._h, None, 1, buf.ctypes.data, 0),
             lambda: L.svh_grid_render_pose(g._h, one.ctypes.data, -1, buf.ctypes.data, 0)]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG and "svh_grid" in G.last_error(), k
    assert (buf == 0xAB).all() and (dev.get() == 0xEE).all() and (n.value, cost.value, d.value) == (-7, -7, -7)
    assert g.pose_stats()[:3] == (1, f[3], int((f[1] != FAR).sum()))
    check(G, g, "after")
    # device pointers: the three fields and the image, nothing beyond them
    for which, k, nbytes in ((G.POSE_CF, 0, states), (G.POSE_POT, 1, 4 * states), (G.POSE_DIR, 2, states)):
        out = Dev(hip, nbytes + 16)
        g.pose_plane(which, device_ptr=out.addr)
        got = out.get()
        assert got[:nbytes].tobytes() == f[k].tobytes() and (got[nbytes:] == 0xEE).all(), which
    out = Dev(hip, 3 * nx * nz + 16)
    g.render_pose([(1, 1, 0), (2, 2, 4)], device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:3 * nx * nz].reshape(nz, nx, 3), g.render_pose([(1, 1, 0), (2, 2, 4)])) and (got[3 * nx * nz:] == 0xEE).all()


def test_the_layer_needs_a_vehicle_and_a_traversability_that_fit(G):
    """cells of 2 cm: with a traversability that fits, the default car's reach is 221 cells, beyond 128, and the layer asks for
    svh_grid_set_roll.  Cells of 5 mm: the default inflation radius does not fit either, and the layer asks for
    svh_grid_set_traversability first, as the planner does.  With both set on the small grid the field is there"""
    import grid_ref as R
    buf = np.full(8 * 81 * 4, 0xAB, np.uint8)
    n, cost = C.c_int64(-7), C.c_int32(-7)

    def small(cell):
        g = G.Grid(G.default_params(nx=9, nz=9, cell=cell, x0=0.0, z0=0.0, T=R.frame_camera(0.0), min_points=1))
        g.pose_set_goals([(4, 4, -1)])
        return g, np.array([4.5 * cell, 0.0, 4.5 * cell])

    def refused(g, xyz, needs):
        L = g._L
        for call in (lambda: L.svh_grid_get_pose_plane(g._h, 0, buf.ctypes.data, 0), lambda: L.svh_grid_get_pose_stats(g._h, buf.ctypes.data),
                     lambda: L.svh_grid_pose_path(g._h, xyz.ctypes.data, 0, buf.ctypes.data, 4, C.addressof(n), C.addressof(cost)),
                     lambda: L.svh_grid_render_pose(g._h, None, 0, buf.ctypes.data, 0)):
            assert call() == BAD_ARG and needs in G.last_error(), (needs, G.last_error())
        assert (buf == 0xAB).all() and (n.value, cost.value) == (-7, -7)

    coarse, xyz_c = small(0.02)
    coarse.set_traversability(inscribed=0.008, inflate=0.04)
    refused(coarse, xyz_c, "svh_grid_set_roll")
    fine, xyz_f = small(0.005)
    refused(fine, xyz_f, "svh_grid_set_traversability")
    fine.set_traversability(inscribed=0.004, inflate=0.02)
    refused(fine, xyz_f, "svh_grid_set_roll")
    fine.set_roll(front=0.0, rear=0.0, half_width=0.0, unknown_cost=0)
    fine.add_points(np.array([[0.0225, 0.0, 0.0225, 0.5]], np.float32))
    pot = fine.pose_plane(G.POSE_POT)
    assert pot[0, 4, 4] == 0 and pot[0, 4, 3] == 500 and pot[4, 4, 5] == 500 and fine.pose_path(xyz_f, 0)[0] == G.PATH_FOUND
    # no room for poses: the walk still counts them, and writes none
    status, poses, c = fine.pose_path([3.5 * 0.005, 0.0, 4.5 * 0.005], 0, cap=0)
    assert (status, len(poses), c, fine.pose_path_len) == (G.PATH_FOUND, 0, 500, 2)
    # an image takes at most 8 nx nz poses
    many = np.zeros((8 * 81 + 1, 3), np.int32)
    assert fine._L.svh_grid_render_pose(fine._h, many.ctypes.data, len(many), buf.ctypes.data, 0) == BAD_ARG and "8 nx nz" in G.last_error()
    assert fine.render_pose(many[:8 * 81]).shape == (9, 9, 3)


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------
def test_pipeline_grid_pose(G, tmp_path, monkeypatch, capsys):
    """--grid-local DIR --grid-cost DIR2 --grid-pose DIR3 on the two golden frames: one pose image and one line of pose.jsonl per
    frame; a sequence that was found starts at the camera's heading, moves by the contract's moves and ends on the goal row"""
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
    d, d2, d3 = str(tmp_path / "loc"), str(tmp_path / "cost"), str(tmp_path / "pose")
    common = ["--grid-slope", "0.3", "--grid-inflate", "2.0", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-pose", d3, "--grid-goal-ahead", "10",
                                      "--grid-pose-params", "80,300,-1", "--grid-roll-vehicle", "1.0,0.5,0.4", "--grid-roll-unknown", "100"] + common)
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("pose plan: goals 10 m ahead, turn 80, reverse 300, spin -1: a pose sequence in ") and "2 images and pose.jsonl" in l
               for l in out), out[-4:]
    assert sorted(os.listdir(d3)) == ["pose.jsonl"] + ["pose_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(d3, "pose.jsonl"))]
    assert [l["frame"] for l in lines] == [0, 1]
    for k, l in enumerate(lines):
        img = read_ppm(os.path.join(d3, "pose_%06d.ppm" % k))
        assert img.shape == (160, 96, 3) and l["status"] in (0, 1, 2) and l["heading"] == 2 and l["length"] == len(l["poses"])
        if l["status"] == 0:
            poses = np.array(l["poses"])
            assert poses[0][2] == 2 * 8 and (poses[:, 2] % 8 == 0).all() and (img.reshape(-1, 3) == (255, 255, 255)).all(1).sum() >= 1
            for (a, b, k0), (a1, b1, k1) in zip(poses[:-1], poses[1:]):
                hits = [m for m in range(6) if QR.arrival(a, b, k0 // 8, m) == (a1, b1, k1 // 8)]
                assert hits and max(hits) <= 3, (a, b, k0, a1, b1, k1)        # a move of the contract, and no spin: none was allowed
            assert l["cost"] < FAR
        else:
            assert l["poses"] == [] and l["cost"] == FAR
