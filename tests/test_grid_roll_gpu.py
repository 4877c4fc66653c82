"""GPU: the rollouts of the ground grid on the device (include/svh_grid.h, "ROLLOUT"; stereo-vision_amd/csrc/grid_roll_kernels.hip)
against stereo-vision_amd/csrc/grid_roll_core.h on the host (svh_test_grid_roll) and its restatement tests/grid_roll_ref.py, byte for
byte: the kernels on a caller's planes through svh_test_grid_roll_device at the sizes where they take another path -- footprints
below, at and above a wave and a workgroup, K and T round 64, windows round the tiles of the other layers --, then the object on the
wall-with-gap scenes of tests/test_grid_trav_gpu.py and tests/test_grid_plan_gpu.py, its refusals, its injected failures and the
pipeline tool.  tests/test_grid_roll.py pins the restatement by hand."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import grid_plan_ref as PR
import grid_ref as R
import grid_roll_ref as RR
import grid_trav_ref as TR
import helpers as H
import test_grid_local_gpu as TL
import test_grid_plan_gpu as TPG
import test_grid_roll as TRL
import test_grid_trav_gpu as TT
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2
FAR, INF = RR.FAR, RR.INFEASIBLE
CELL = TL.CELL
POINT = TRL.POINT
ROW3 = dict(front=1.0, rear=1.0, half_width=0.0)                  # cells of 1: a row of 3 along an axis heading, group 4
CELLS65 = dict(front=32.0, rear=32.0, half_width=0.0)             # 65 cells: one more than a wave
CELLS289 = dict(front=8.0, rear=8.0, half_width=8.0)              # 17 x 17: more than a workgroup
RESTATE = 40000                                                   # the restatement is plain Python: K * T * cells up to this


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


differ = TPG.differ


def run(G, cost, pot, tab, anchor, cell=1.0, oa=0, ob=0, set_=0, poses=None, tag="", **kw):
    """device_roll against core_roll, and core_roll against the restatement where that is quick; returns the device's"""
    q = G.default_roll(**kw)
    tab = np.ascontiguousarray(tab, np.int32)
    got = G.device_roll(q, cell, cost, pot, tab, set_, anchor, oa, ob, poses)
    want = G.core_roll(q, cell, cost, pot, tab, set_, anchor, oa, ob, poses)
    for name in ("recs", "scores") + (("f",) if poses is not None else ()):
        differ(tag, name, got[name], want[name])
    assert got["best"] == want["best"], (tag, got["best"], want["best"])
    p = RR.RollParams(**kw)
    _, lists = RR.table(p, cell)
    if tab.shape[1] * tab.shape[2] * max(len(l) for l in lists) <= RESTATE:
        recs, scores, best = RR.score(p, lists, np.asarray(cost), pot, tab[set_], anchor, oa, ob)
        differ(tag + " (header against restatement)", "recs", want["recs"], recs)
        differ(tag + " (header against restatement)", "scores", want["scores"], scores)
        assert want["best"] == best
    return got


def case(rng, nx, nz, K, T, m, S=1):
    cost, pot, tab, poses, kw = TRL.random_case(rng, nx, nz, K=K, T=T, S=S, m=m)
    return cost, pot, tab, poses, {k: kw[k] for k in ("stop_cost", "unknown_cost", "w_pot", "w_cost", "w_cut")}


WINDOWS = [(1, 1), (1, 9), (9, 1), (3, 3), (15, 15), (16, 16), (17, 17), (33, 17), (257, 129)]
KS, TS, MS = (1, 63, 64, 65, 257), (1, 2, 63, 64, 65), (1, 2, 8)
VEHICLES = (POINT, ROW3, CELLS65, CELLS289)


@pytest.mark.parametrize("k", range(len(WINDOWS)))
def test_windows(G, k):
    """every window with each footprint; K, T and m rotate through their sets, the anchor lies inside or one cell outside"""
    nx, nz = WINDOWS[k]
    rng = np.random.default_rng(500 + k)
    statuses = set()
    for v, car in enumerate(VEHICLES):
        K, T, m = KS[(k + v) % 5], TS[(k + 2 * v) % 5], MS[(k + v) % 3]
        cost, pot, tab, poses, kw = case(rng, nx, nz, K, T, m, S=2)
        anchor = (int(rng.integers(-1, nx + 1)), int(rng.integers(-1, nz + 1)))
        got = run(G, cost, pot, tab, anchor, set_=v % 2, poses=poses, tag="%dx%d vehicle %d K %d T %d m %d" % (nx, nz, v, K, T, m), headings_m=m,
                  **dict(kw, **car))
        statuses |= set(got["recs"][:, 1].tolist())
    if nx * nz >= 500:
        assert statuses == {0, 1, 2, 3}                                              # every status


@pytest.mark.parametrize("K", KS)
def test_every_k_with_every_t(G, K):
    rng = np.random.default_rng(600 + K)
    for T in TS:
        cost, pot, tab, poses, kw = case(rng, 33, 17, K, T, 2)
        run(G, cost, pot, tab, (16, 8), tag="K %d T %d" % (K, T), headings_m=2, **dict(kw, **ROW3))


def test_footprints_of_every_group_width(G):
    """lists of 1, 2, 3, 6, 12, 24, 48, 65 and 289 cells along the axes: groups of 1, 2, 4, 8, 16, 32, 64 lanes, a wave that strides
    once and a list longer than a workgroup"""
    rng = np.random.default_rng(610)
    widths = []
    for front, hw in ((0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (5.0, 0.0), (11.0, 0.0), (23.0, 0.0), (47.0, 0.0), (64.0, 0.0), (16.0, 8.0)):
        for m in MS:
            q = G.default_roll(front=front, rear=0.0, half_width=hw, headings_m=m)
            _, lists = G.core_roll_table(1.0, q)
            widths.append(G.roll_group(max(len(l) for l in lists)))
            cost, pot, tab, poses, kw = case(rng, 80, 70, 5, 7, m)
            tab[..., :2] = np.cumsum(rng.integers(-4, 7, tab[..., :2].shape), axis=2)
            run(G, cost, pot, tab, (30, 25), poses=poses, tag="front %g hw %g m %d" % (front, hw, m), front=front, rear=0.0, half_width=hw,
                headings_m=m, **kw)
    assert set(widths) == {1, 2, 4, 8, 16, 32, 64}


def test_anchors_in_the_corners(G):
    """a car of 5 x 3 cells turning through every heading two cells from each corner: its footprint leaves the window on each side"""
    nx, nz, m = 21, 19, 8
    rng = np.random.default_rng(620)
    cost = rng.integers(0, 200, (nz, nx)).astype(np.uint8)
    tab = np.zeros((1, 64, 3, 3), np.int32)
    tab[0, :, :, 2] = np.arange(64).reshape(-1, 1)
    tab[0, :, 1, 0], tab[0, :, 2, 1] = 1, 1
    car = dict(front=2.0, rear=2.0, half_width=1.0, headings_m=m, w_pot=0)
    for a, b in ((2, 2), (nx - 3, 2), (2, nz - 3), (nx - 3, nz - 3), (0, 0), (nx - 1, nz - 1), (nx // 2, nz // 2)):
        got = run(G, cost, None, tab, (a, b), tag="anchor %d %d" % (a, b), **car)
        st = got["recs"][:, 1]
        if (a, b) == (nx // 2, nz // 2):
            assert (st == 0).all()
        elif a in (0, nx - 1):
            assert (st == 2).all() and (got["recs"][:, 0] == 0).all()
        elif (a, b) != (2, 2):
            assert (st == 2).any() and (got["recs"][:, 0] > 0).any()                 # some headings fit beside the walls, a step on none does
    poses = np.array([(a, b, k) for a in (-1, 0, 2, nx - 3, nx - 1, nx) for b in (-1, 0, 2, nz - 3, nz - 1, nz) for k in range(0, 64, 5)], np.int32)
    got = run(G, cost, None, tab, (5, 5), poses=poses, **car)
    assert (got["f"] == -1).any() and (got["f"] >= 0).any()


def test_cost_planes_all_0_all_254_and_one_lethal_cell(G):
    nx, nz, m, T = 40, 30, 2, 9
    tab = np.zeros((1, 3, T, 3), np.int32)
    tab[0, :, :, 1] = np.arange(T) + 1                                               # straight ahead from the anchor, pose t at b + t + 1
    tab[0, :, :, 2] = 2 * m
    tab[0, 1, :, 0], tab[0, 2, :, 0] = 4, -4
    car = dict(front=2.0, rear=1.0, half_width=1.0, headings_m=m, w_pot=0, w_cut=9)
    _, lists = RR.table(RR.RollParams(**car), 1.0)
    foot = lists[2 * m]
    assert len(foot) == 12
    got = run(G, np.zeros((nz, nx), np.uint8), None, tab, (20, 3), **car)
    assert got["recs"].tolist() == [[T, 0, 0, 0, FAR]] * 3 and got["best"] == 0
    got = run(G, np.full((nz, nx), 254, np.uint8), None, tab, (20, 3), **car)
    assert got["recs"].tolist() == [[0, 1, -1, 0, FAR]] * 3 and got["best"] == -1
    got = run(G, np.full((nz, nx), 254, np.uint8), None, tab, (20, 3), **dict(car, stop_cost=255))
    assert got["recs"].tolist() == [[T, 0, 254, 254 * T, FAR]] * 3
    # one lethal cell under exactly one footprint cell of exactly one pose: the first, a middle and the last entry of the list, at
    # the first, a middle and the last pose; the poses are one cell apart, so the cell must lie under no earlier pose -- the front row
    # of the footprint (the entries with the largest db) is what a step ahead newly covers
    front_row = np.flatnonzero(foot[:, 1] == foot[:, 1].max())
    for t in (0, T // 2, T - 1):
        for e in (0, len(foot) - 1, int(front_row[0]), int(front_row[len(front_row) // 2])):
            cost = np.zeros((nz, nx), np.uint8)
            a, b = 20 + int(foot[e, 0]), 3 + t + 1 + int(foot[e, 1])
            cost[b, a] = 254
            got = run(G, cost, None, tab, (20, 3), tag="pose %d entry %d" % (t, e), **car)
            first = min(s for s in range(T) if any(20 + int(o[0]) == a and 3 + s + 1 + int(o[1]) == b for o in foot))
            assert got["recs"][0].tolist() == [first, 1, 0 if first else -1, 0, FAR] and (first == t or e not in front_row), (t, e)
            assert got["recs"][1:].tolist() == [[T, 0, 0, 0, FAR]] * 2
            cost[b, a] = 77                                                          # and a cell that is merely dear: one pose's F, no cut
            got = run(G, cost, None, tab, (20, 3), **car)
            assert got["recs"][0, :3].tolist() == [T, 0, 77] and got["recs"][0, 3] % 77 == 0


def test_ties_in_the_score_across_the_strides_of_the_arg_min(G):
    """4097 candidates: the arg-min's 1024 lanes take four or five each; equal scores in different lanes, waves and strides"""
    K, nx, nz = 4097, 9, 9
    cost = np.full((nz, nx), 5, np.uint8)
    cost[4, 5:] = 3
    tab = np.zeros((1, K, 2, 3), np.int32)
    tab[0, :, 1, 0] = -1                                                             # every candidate: (0, 0) then (-1, 0): sumF = 10
    kw = dict(headings_m=1, w_pot=0, **POINT)
    assert run(G, cost, None, tab, (4, 4), **kw)["best"] == 0
    for ties, want in (((4096, 1024, 1025), 1024), ((4096,), 4096), ((1023, 2047, 63, 64), 63), ((3000, 2999, 1976), 1976)):
        t = tab.copy()
        for c in ties:
            t[0, c, 1, 0] = 1                                                        # (0, 0) then (1, 0): sumF = 8
        got = run(G, cost, None, t, (4, 4), **kw)
        assert got["best"] == want and (got["scores"][list(ties)] == 8).all() and (got["scores"] == 8).sum() == len(ties)
    t = tab.copy()
    t[0, :, 0, 2] = -1                                                               # none has a pose: none is feasible
    got = run(G, cost, None, t, (4, 4), **kw)
    assert got["best"] == -1 and (got["scores"] == INF).all() and (got["recs"][:, 1] == 3).all()


def test_the_same_bytes_twice(G):
    rng = np.random.default_rng(640)
    cost, pot, tab, poses, kw = case(rng, 129, 65, 257, 65, 8)
    q = G.default_roll(front=3.0, rear=1.0, half_width=1.0, headings_m=8, **kw)
    a = G.device_roll(q, 0.5, cost, pot, tab, 0, (124, 61), 0, 0, poses)
    b = G.device_roll(q, 0.5, cost, pot, tab, 0, (124, 61), 0, 0, poses)
    for name in ("recs", "scores", "f"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["best"] == b["best"] and (a["recs"][:, 0] > 0).any() and (a["f"] >= 0).any()
    w = G.device_roll(G.default_roll(front=3.0, rear=1.0, half_width=1.0, headings_m=8, **dict(kw, w_pot=0)), 0.5, cost, None, tab, 0, (124, 61))
    assert (w["recs"][:, 4] == FAR).all() and np.array_equal(w["recs"][:, :4], a["recs"][:, :4])   # w_pot = 0: no field is read


# ---- through the object --------------------------------------------------------------------------------------------------
def roll_of(g):
    """the restatement's parameters and lists for the object's"""
    q = g.roll_params()[0]
    p = RR.RollParams(**q.asdict())
    return p, RR.table(p, g.params.cell)[1]


def check(G, g, tab, xyz, set_=0, tag=""):
    """best, records, scores and the image against the restatement on the object's own COST and POT planes"""
    p, lists = roll_of(g)
    cost = g.trav_plane(G.TRAV_COST)
    pot = g.plan_plane(G.PLAN_POT) if p.w_pot else None
    (oa, ob), anchor = g.window(), g.cell_of(xyz)
    recs, scores, best = RR.score(p, lists, cost, pot, tab[set_], anchor, oa, ob)
    got = g.roll_score(xyz, set_)
    assert got[0] == best, (tag, got[0], best)
    differ(tag, "the records", got[1], recs)
    differ(tag, "the scores", got[2], scores)
    differ(tag, "the image", g.render_roll(), RR.overlay(g.render_cost(), tab[set_], recs, best, anchor, oa, ob))
    return best, recs, scores


def fan(m=8, T=14, step=0.75):
    """arcs of seven curvatures from every heading"""
    from svhip import grid
    return grid.arc_candidates(CELL, m, [-0.3, -0.15, -0.06, 0.0, 0.06, 0.15, 0.3], step, T)


def test_footprint_cost_host_and_device_pointers(G, hip):
    nx, nz = 65, 33
    ref, g, rng = TPG.build(G, nx, nz, 71)
    p, lists = roll_of(g)
    assert g.roll_params()[1:] == (10, sum(len(l) for l in lists)) and G.roll_group(max(len(l) for l in lists)) == 64
    for k in (0, 16, 37):
        assert np.array_equal(g.roll_footprint(k), lists[k])
    cost = g.trav_plane(G.TRAV_COST)
    differ("", "COST", cost, ref.trav()["cost"])
    poses = np.stack([rng.integers(-2, nx + 2, 300), rng.integers(-2, nz + 2, 300), rng.integers(0, 64, 300)], axis=1).astype(np.int32)
    want = RR.footprint_costs(p, lists, cost, poses)
    assert (want == -1).any() and (want == 254).any() and ((want >= 0) & (want < 253)).any()
    differ("", "F, host", g.footprint_cost(poses), want)
    poses[7, 2], poses[9, 2] = 64, -1                                                # on the device path a heading that does not exist gives -1
    d_in, d_out = Dev(hip, poses), Dev(hip, 4 * 300 + 16)
    g.footprint_cost(device_ptrs=(d_in.addr, d_out.addr), n=300)
    out = d_out.get()
    want[[7, 9]] = -1
    assert np.array_equal(out[:1200].view(np.int32), want) and (out[1200:] == 0xEE).all()
    assert len(g.footprint_cost(np.zeros((0, 3), np.int32))) == 0
    g.scroll(3, -2)
    poses[[7, 9], 2] = 5
    differ("", "F after a scroll", g.footprint_cost(poses), RR.footprint_costs(p, lists, g.trav_plane(G.TRAV_COST), poses, 3, -2))
    for d in ((0, 0, 1), (1, 0, 0), (-1, 0, 1), (0.3, 5.0, -0.9)):                    # a = x, b = z
        assert g.heading_of(d) == RR.heading_of(8, d[0], d[2]) and 0 <= g.heading_of(d) < 64


def test_a_gap_that_a_point_passes_and_the_car_does_not(G):
    """the wall at ia = nx // 3 has a gap over ib = 4 .. 7; along row 4, beside the wall's end, a point meets a cost of 210 and passes;
    the default car (seven cells to the front, five wide on cells of 0.5 m) meets the wall itself four poses on.  Along row 1 the point
    runs into the wall and the car does not fit the window"""
    nx, nz = 65, 33
    ref, g, rng = TPG.build(G, nx, nz, 72)
    w = nx // 3
    tab = np.zeros((1, 2, 16, 3), np.int32)
    tab[0, :, :, 0] = np.arange(16) + 1                                              # heading 0 is +a
    tab[0, 1, :, 1] = -3                                                             # the second runs along row 1, into the wall
    g.set_candidates(tab)
    start = TL.centre(ref, w - 12, 4)
    g.set_roll(w_pot=0, w_cut=1000, **POINT)                                          # a pose not driven weighs more than the costs collected
    best, recs, scores = check(G, g, tab, start, tag="a point")
    assert recs[0].tolist()[:3] == [16, 0, 210] and recs[1].tolist()[:2] == [11, 1] and best == 0
    g.set_roll(G.default_roll(w_pot=0, w_cut=1000))
    best, recs, scores = check(G, g, tab, start, tag="the car")
    assert recs[0].tolist()[:2] == [4, 1] and recs[1].tolist()[:2] == [0, 2] and best == 0
    img = g.render_roll()
    assert (img == G.ROLL_BEST_COLOUR).all(axis=2).sum() == 4 and (img == G.ROLL_COLOUR).all(axis=2).sum() == 0


def test_scores_after_a_scroll_a_new_obstacle_and_a_clear(G):
    nx, nz = 65, 65
    ref, g, rng = TPG.build(G, nx, nz, 73, unknown=100)
    tab = fan()
    g.set_candidates(tab)
    g.set_roll(front=1.0, rear=0.5, half_width=0.5)
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    start = TL.centre(ref, 5, 20)
    s = g.heading_of((1.0, 0.0, 0.3))
    best, recs, scores = check(G, g, tab, start, s, "before")
    assert best >= 0 and set(recs[:, 1].tolist()) >= {0, 1}
    G.lib().svh_test_fail_at(b"malloc:1:0")                                          # a second scoring allocates nothing
    assert g.roll_score(start, s)[0] == best
    G.lib().svh_test_fail_at(None)
    g.scroll(4, 3)
    ref.scroll(4, 3)
    differ("scrolled", "the old records over the new window", g.render_roll(), RR.overlay(g.render_cost(), tab[s], recs, best, g.cell_of(start), 4, 3))
    best2, recs2, _ = check(G, g, tab, start, s, "scrolled")
    pts = TL.at_cells(ref, np.arange(8, 13), 22, 1.0)                                # a new obstacle across the way
    TT.add_both(g, ref, np.concatenate([pts, pts]))
    best3, recs3, _ = check(G, g, tab, start, s, "a new obstacle")
    assert recs3.tobytes() != recs2.tobytes()
    for set_ in (0, 17, 63):
        check(G, g, tab, start, set_, "set %d" % set_)
    best4, recs4, _ = check(G, g, tab, TL.centre(ref, -3, 20), s, "an anchor outside the window")
    assert best4 == -1 and (recs4[:, :2] == (0, 2)).all()
    g.clear()                                                                        # both tables survive; the goals do not
    ref.clear()
    assert g.roll_params()[0].asdict()["front"] == 1.0 and g.plan_stats()[0] == 0
    best5, recs5, scores5 = check(G, g, tab, start, s, "cleared")                     # every cell unknown: 255 counts as 254 and cuts
    assert best5 == -1 and (recs5[:, 0] == 0).all()
    g.set_roll(unknown_cost=0, w_pot=0)
    best6, recs6, _ = check(G, g, tab, start, s, "cleared, unknown cells free")
    assert best6 >= 0 and (recs6[:, 2] <= 0).all()
    g.set_window(1.0, 2.0)
    check(G, g, tab, TL.centre(ref, 9, 9), s, "a new window")
    g.set_roll(headings_m=4)                                                         # another enumeration forgets the candidates
    with pytest.raises(G.SvhError) as e:
        g.roll_score(start, 0)
    assert e.value.code == BAD_ARG and "no candidates" in G.last_error()


def test_the_best_leads_toward_the_goal(G):
    nx, nz = 65, 65
    ref, g, rng = TPG.build(G, nx, nz, 74)
    tab = fan(T=10)
    g.set_candidates(tab)
    g.set_roll(front=0.5, rear=0.5, half_width=0.5, w_cost=0)
    start_cell = (32, 30)                                                            # midway between the two walls
    start = TL.centre(ref, *start_cell)
    for goal in ((32, 50), (32, 10), (25, 30), (33, 31)):
        g.set_goal(TL.centre(ref, *goal))
        pot = g.plan_plane(G.PLAN_POT)
        for s in (0, 16, 32, 48):
            best, recs, scores = check(G, g, tab, start, s, "goal %r set %d" % (goal, s))
            assert best >= 0
            end = tab[s, best, recs[best, 0] - 1, :2] + start_cell                   # w_cost = 0: the score is POT where the arc ends
            assert pot[end[1], end[0]] == recs[best, 4] == scores[best] == min(r[4] for r in recs if r[0] >= 1)
    g.set_goals([])                                                                # no goals: POT is FAR, nothing is feasible
    best, recs, scores = check(G, g, tab, start, 16, "no goals")
    assert best == -1 and (recs[:, 4] == FAR).all() and (scores == INF).all() and (recs[:, 0] > 0).any()


# ---- failures ------------------------------------------------------------------------------------------------------------
def cached(G, g):
    """what the other layers have cached, fetched without a launch"""
    G.lib().svh_test_fail_at(b"launch:1:0")
    out = dict(cost=g.trav_plane(G.TRAV_COST), pot=g.plan_plane(G.PLAN_POT), label=g.front_plane(G.FRONT_LABEL), recs=g.frontiers())
    G.lib().svh_test_fail_at(None)
    return out


def scene(G, seed):
    """walls with gaps, goals beyond them, the field and the frontiers computed; a small car and a fan of arcs not yet given"""
    nx, nz = 65, 33
    ref, g, rng = TPG.build(G, nx, nz, seed)
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    g.set_frontier(min_size=1, border=1)
    g.plan_plane(G.PLAN_POT), g.frontiers()
    return ref, g, fan(T=8), TL.centre(ref, 30, 12)


def fails(G, call, spec):
    G.lib().svh_test_fail_at(spec if isinstance(spec, bytes) else spec.encode())
    with pytest.raises(G.SvhError) as e:
        call()
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR, spec


@pytest.mark.parametrize("spec", ["malloc:1", "malloc:2", "malloc:3", "malloc:4", "launch:1", "copy:1", "copy:2", "copy:3", "wait:1"])
def test_a_failed_scoring_leaves_everything_else(G, spec):
    """a new object with both tables on the device and the planes, the field and the frontiers cached, so that a scoring does: malloc 1
    to 3 the records, the scores and the best, 4 the pinned buffer; launch 1 its two kernels; copy 1 to 3 the scores, the records and
    the best, wait 1 their arrival"""
    ref, g, tab, start = scene(G, 75)
    g.set_roll(front=1.0, rear=0.5, half_width=0.5)
    g.set_candidates(tab)
    before, grid_before = cached(G, g), TL.snapshot(G, g)
    fails(G, lambda: g.roll_score(start, 16), spec)
    with pytest.raises(G.SvhError) as e:                                             # no records to draw
        g.render_roll()
    assert e.value.code == BAD_ARG
    after = cached(G, g)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before) and g.plan_stats()[0] == 7
    assert TL.same(TL.snapshot(G, g), grid_before)
    best, recs, scores = check(G, g, tab, start, 16, spec + ": the call repeated")    # both tables are what was set
    assert best >= 0
    TPG.check(G, g, ref, "the field afterwards")


def test_failed_uploads_are_repeated(G):
    """svh_grid_set_roll and svh_grid_roll_set_candidates keep what they were given when their upload fails -- two allocations, two
    copies and a wait each -- and the next scoring sends it; a scoring that fails there leaves it to the next"""
    ref, g, tab, start = scene(G, 77)
    before = cached(G, g)
    for spec in (b"malloc:1", b"malloc:2", b"copy:1", b"copy:2", b"wait:1"):
        fails(G, lambda: g.set_roll(front=1.0, rear=0.5, half_width=0.5), spec)
        assert g.roll_params()[0].asdict()["front"] == 1.0 and g.roll_params()[1] == 4
        assert np.array_equal(g.roll_footprint(16), roll_of(g)[1][16])                # the host's copy of the table
    g.set_roll()                                                                     # the same parameters; now the table is on the device
    assert g.candidates() == (0, 0, 0)
    for spec in (b"malloc:1", b"malloc:2", b"copy:1", b"copy:2", b"wait:1"):
        fails(G, lambda: g.set_candidates(tab), spec)
        assert g.candidates() == tab.shape[:3] == (64, 7, 8)                           # the table is in force
    for spec in (b"copy:1", b"copy:2", b"wait:1"):                                   # the scoring sends the candidates first
        fails(G, lambda: g.roll_score(start, 16), spec)
    best, recs, scores = check(G, g, tab, start, 16, "after the failed uploads")
    assert best >= 0
    fails(G, lambda: g.set_roll(front=0.5), b"copy:1")                               # the footprint table alone, sent by a footprint cost
    poses = np.array([[30, 12, 3], [2, 2, 40]], np.int32)
    p, lists = roll_of(g)
    assert np.array_equal(g.footprint_cost(poses), RR.footprint_costs(p, lists, before["cost"], poses))
    check(G, g, tab, start, 16, "a smaller car")
    after = cached(G, g)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)


def test_failed_footprint_costs_and_images(G):
    """with everything cached and allocated: svh_grid_footprint_cost copies the poses (copy 1), launches (launch 1) and brings F (copy
    2, wait 1); svh_grid_render_roll launches (launch 1) and brings the image (copy 1, wait 1)"""
    ref, g, tab, start = scene(G, 78)
    g.set_roll(front=1.0, rear=0.5, half_width=0.5)
    g.set_candidates(tab)
    best, recs, scores = check(G, g, tab, start, 16, "before")
    poses = np.array([[30, 12, 3], [2, 2, 40]], np.int32)
    f, img = g.footprint_cost(poses), g.render_roll()
    before = cached(G, g)
    for call, specs in ((lambda: g.footprint_cost(poses), ("copy:1", "launch:1", "copy:2", "wait:1")), (lambda: g.render_roll(), ("launch:1", "copy:1", "wait:1"))):
        for spec in specs:
            fails(G, call, spec)
            assert np.array_equal(g.footprint_cost(poses), f) and np.array_equal(g.render_roll(), img)      # the records of the last scoring are still there
    after = cached(G, g)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)
    fresh = G.Grid(g.params)                                                         # a new object: the allocations of a footprint cost
    fresh.set_traversability(**TPG.TRAV)
    fresh.add_points(TL.at_cells(ref, [3, 3], [4, 4]))
    fresh.trav_plane(G.TRAV_COST)
    for what in ("the footprint table's lists", "its starts", "the poses", "F"):       # each attempt fails the next buffer that is missing
        fails(G, lambda: fresh.footprint_cost(poses), "malloc:1")
    assert (fresh.footprint_cost(poses) >= -1).all()


def test_a_failed_first_image_allocates_again(G):
    """a new object that has scored and has neither fetched a plane nor drawn an image: svh_grid_render_roll allocates the image on the
    device (malloc 1) and its pinned copy (malloc 2); either failing leaves the records of the scoring and everything cached"""
    nx, nz = 65, 33
    ref, g, rng = TPG.build(G, nx, nz, 79)
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    tab, start = fan(T=8), TL.centre(ref, 30, 12)
    g.set_roll(front=1.0, rear=0.5, half_width=0.5)
    g.set_candidates(tab)
    best, recs, scores = g.roll_score(start, 16)
    assert best >= 0
    for spec in ("malloc:1", "malloc:2"):
        fails(G, lambda: g.render_roll(), spec)
    G.lib().svh_test_fail_at(b"launch:1:0")                                          # the cost planes and the field: still cached, no launch
    cost, pot = g.trav_plane(G.TRAV_COST), g.plan_plane(G.PLAN_POT)
    G.lib().svh_test_fail_at(None)
    p, lists = roll_of(g)
    want = RR.score(p, lists, cost, pot, tab[16], g.cell_of(start), 0, 0)
    assert want[2] == best and np.array_equal(want[0], recs) and np.array_equal(want[1], scores)
    differ("", "the image drawn from the records of that scoring", g.render_roll(), RR.overlay(g.render_cost(), tab[16], recs, best, g.cell_of(start)))
    check(G, g, tab, start, 16, "a scoring after the failed allocations")
    assert g.plan_stats()[0] == 7
    TPG.check(G, g, ref, "the field afterwards")


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte(G, hip):
    nx, nz = 65, 33
    ref, g, rng = TPG.build(G, nx, nz, 76)
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    tab = fan(T=6)
    start = np.array(TL.centre(ref, 30, 12), np.float64)
    L = g._L
    buf = np.full(4096, 0xAB, np.uint8)
    best = C.c_int32(-7)
    score = lambda set_=0, xyz=start, recs=buf.ctypes.data, scores=buf.ctypes.data, dev=0, b=C.addressof(best): L.svh_grid_roll_score(
        g._h, xyz.ctypes.data if xyz is not None else None, set_, recs, scores, dev, b)
    assert score() == BAD_ARG and "no candidates" in G.last_error()
    assert L.svh_grid_render_roll(g._h, buf.ctypes.data, 0) == BAD_ARG and "nothing was scored" in G.last_error()
    g.set_candidates(tab)
    for kw in TRL.BAD:
        p = G.default_roll(**kw)
        assert L.svh_grid_set_roll(g._h, C.byref(p)) == BAD_ARG and "svh_grid_set_roll" in G.last_error(), kw
    assert L.svh_grid_set_roll(g._h, C.byref(G.default_roll(front=63.0))) == BAD_ARG                  # R = ceil(64.4 / 0.5) = 129
    assert L.svh_grid_set_roll(g._h, None) == BAD_ARG
    assert g.roll_params()[0].asdict() == G.default_roll().asdict() and g.roll_params()[1] == 10
    dev = Dev(hip, 8 * 7 + 20 * 7 + 32)
    n = C.c_int64(-7)
    bad_tab = tab.copy()
    bad_tab[3, 2, 1, 2] = 64
    far_tab = tab.copy()
    far_tab[0, 0, 0, 0] = 16385
    calls = [lambda: score(set_=64), lambda: score(set_=-1), lambda: score(xyz=None), lambda: score(b=None),
             lambda: score(xyz=np.array([np.nan, 0, 0])), lambda: score(xyz=np.array([1e30, 0, 0])),
             lambda: score(recs=dev.addr + 2, scores=None, dev=1), lambda: score(recs=None, scores=dev.addr + 4, dev=1),
             lambda: L.svh_grid_get_roll(g._h, None, None, None), lambda: L.svh_grid_heading_of(g._h, None, buf.ctypes.data),
             lambda: L.svh_grid_heading_of(g._h, start.ctypes.data, None), lambda: L.svh_grid_heading_of(g._h, np.array([0.0, 1.0, 0.0]).ctypes.data, buf.ctypes.data),
             lambda: L.svh_grid_heading_of(g._h, np.array([np.inf, 1.0, 0.0]).ctypes.data, buf.ctypes.data),
             lambda: L.svh_grid_roll_footprint(g._h, 64, buf.ctypes.data, 1, C.addressof(n)), lambda: L.svh_grid_roll_footprint(g._h, -1, buf.ctypes.data, 1, C.addressof(n)),
             lambda: L.svh_grid_roll_footprint(g._h, 0, None, 1, C.addressof(n)), lambda: L.svh_grid_roll_footprint(g._h, 0, buf.ctypes.data, 1, None),
             lambda: L.svh_grid_footprint_cost(g._h, None, 1, 0, buf.ctypes.data), lambda: L.svh_grid_footprint_cost(g._h, buf.ctypes.data, 1, 0, None),
             lambda: L.svh_grid_footprint_cost(g._h, buf.ctypes.data, -1, 0, buf.ctypes.data),
             lambda: L.svh_grid_footprint_cost(g._h, np.array([0, 0, 64], np.int32).ctypes.data, 1, 0, buf.ctypes.data),
             lambda: L.svh_grid_footprint_cost(g._h, np.array([0, 0, -1], np.int32).ctypes.data, 1, 0, buf.ctypes.data),
             lambda: L.svh_grid_footprint_cost(g._h, dev.addr + 1, 1, 1, dev.addr + 16), lambda: L.svh_grid_footprint_cost(g._h, dev.addr, 1, 1, dev.addr + 18),
             lambda: L.svh_grid_roll_set_candidates(g._h, None, 1, 1, 1), lambda: L.svh_grid_roll_set_candidates(g._h, tab.ctypes.data, 0, 7, 6),
             lambda: L.svh_grid_roll_set_candidates(g._h, tab.ctypes.data, 64, 7, 1025), lambda: L.svh_grid_roll_set_candidates(g._h, tab.ctypes.data, 64, 65537, 1),
             lambda: L.svh_grid_roll_set_candidates(g._h, tab.ctypes.data, 2 ** 20, 4, 2), lambda: L.svh_grid_roll_set_candidates(g._h, bad_tab.ctypes.data, 64, 7, 6),
             lambda: L.svh_grid_roll_set_candidates(g._h, far_tab.ctypes.data, 64, 7, 6), lambda: L.svh_grid_render_roll(g._h, None, 0)]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG and "svh_grid" in G.last_error(), k
    assert (buf == 0xAB).all() and (dev.get() == 0xEE).all() and n.value == -7 and best.value == -7
    best_, recs, scores = check(G, g, tab, start, 16, "after the refusals")           # the table is the one that was set
    # device pointers: the records, the scores, either alone, nothing beyond them; the image
    d_recs, d_scores = Dev(hip, 20 * 7 + 16), Dev(hip, 8 * 7 + 16)
    assert g.roll_score(start, 16, device_ptrs=(d_recs.addr, d_scores.addr)) == best_
    a, b = d_recs.get(), d_scores.get()
    assert a[:140].tobytes() == recs.tobytes() and (a[140:] == 0xEE).all() and b[:56].tobytes() == scores.tobytes() and (b[56:] == 0xEE).all()
    d_recs = Dev(hip, 20 * 7 + 16)
    assert g.roll_score(start, 16, device_ptrs=(d_recs.addr, None)) == best_ and d_recs.get()[:140].tobytes() == recs.tobytes()
    assert g.roll_score(start, 16, device_ptrs=(None, None)) == best_
    bst = C.c_int32(-7)
    assert L.svh_grid_roll_score(g._h, start.ctypes.data, 16, None, None, 0, C.addressof(bst)) == 0 and bst.value == best_
    out = Dev(hip, 3 * nx * nz + 16)
    g.render_roll(device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:3 * nx * nz].reshape(nz, nx, 3), g.render_roll()) and (got[3 * nx * nz:] == 0xEE).all()


def test_rollouts_need_a_traversability_and_a_vehicle_that_fit(G):
    """cells of 5 mm: the default inflation radius would be 300 cells and the default car reaches 881; the object exists and the
    scoring entries refuse until both are set"""
    g = G.Grid(G.default_params(nx=9, nz=9, cell=0.005, x0=0.0, z0=0.0, T=R.frame_camera(0.0), min_points=1))
    g.add_points(np.array([[0.0225, 0.0, 0.0225, 0.5]], np.float32))
    tab = np.zeros((1, 1, 2, 3), np.int32)
    tab[0, 0, :, 2] = 16
    tab[0, 0, 1, 1] = 1
    g.set_candidates(tab)                                                            # needs neither
    assert g.roll_params()[1:] == (0, 0) and g.heading_of((0, 0, 1)) == 16 and g.candidates() == (1, 1, 2)
    buf = np.full(64, 0xAB, np.uint8)
    xyz = np.array([0.0225, 0.0, 0.0225])
    L = g._L
    calls = (lambda: L.svh_grid_roll_score(g._h, xyz.ctypes.data, 0, buf.ctypes.data, None, 0, buf.ctypes.data),
             lambda: L.svh_grid_footprint_cost(g._h, tab.ctypes.data, 1, 0, buf.ctypes.data), lambda: L.svh_grid_render_roll(g._h, buf.ctypes.data, 0))
    for call in calls:
        assert call() == BAD_ARG and "svh_grid_set_traversability" in G.last_error()
    g.set_traversability(inscribed=0.004, inflate=0.02)
    for call in calls[:2] + (lambda: L.svh_grid_roll_footprint(g._h, 0, buf.ctypes.data, 1, buf.ctypes.data),):
        assert call() == BAD_ARG and "svh_grid_set_roll" in G.last_error()
    assert (buf == 0xAB).all()
    g.set_roll(front=0.01, rear=0.005, half_width=0.005, w_pot=0, unknown_cost=7)
    assert g.roll_params()[1] == 4 and len(g.roll_footprint(16)) == 3 * 4
    best, recs, scores = check(G, g, tab, xyz, 0, "a grid of 5 mm")
    assert best == 0 and recs[0].tolist() == [2, 0, 7, 14, FAR]                       # one free cell, the others unknown: 255 counts as 7


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------
def test_pipeline_grid_roll(G, tmp_path, monkeypatch, capsys):
    """--grid-local DIR --grid-cost DIR2 --grid-plan DIR3 --grid-roll DIR4 on the two golden frames: one image and one line of
    roll.jsonl per frame, the restatement's after the same steps on the object's planes.  Two frames leave the camera's cell unknown,
    so under the defaults every arc is cut at pose 0; the test gives --grid-roll-vehicle 0,0,0 and --grid-roll-unknown 0 -- a point
    that may cross unknown cells --, for which the restatement has a feasible arc in both frames"""
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
    d, d2, d3, d4 = (str(tmp_path / n) for n in ("loc", "cost", "plan", "roll"))
    common = ["--grid-slope", "2.0", "--grid-inscribed", "0.1", "--grid-inflate", "0.5", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-plan", d3, "--grid-roll", d4,
                                      "--grid-roll-vehicle", "0,0,0", "--grid-roll-unknown", "0"] + common)
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("rollouts: ") and "2 images and roll.jsonl" in l for l in out), out[-4:]
    assert sorted(os.listdir(d4)) == ["roll.jsonl"] + ["roll_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(d4, "roll.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = PR.Grid(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0), TR.TravParams(max_slope=2.0, inscribed=0.1, inflate=0.5), PR.PlanParams(unknown=100))
    rp = RR.RollParams(front=0.0, rear=0.0, half_width=0.0, unknown_cost=0)
    _, lists = RR.table(rp, 0.25)
    tab = G.arc_candidates(0.25, 8, SP.ROLL_CURVATURES, 0.5, SP.ROLL_POSES)
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre_ = p.H_total[:3, 3]
        ref.follow(centre_, 48, 80)
        ref.add_from(p.view.points(p.view.count(view.LISTS) - 1), centre_)
        ga, gb = TL.LR.cell_of(ref.P, centre_)
        ref.set_goals([(ref.oa + ia, min(gb + 80, ref.ob + 159)) for ia in range(96)])
        f = ref.field()
        s = RR.heading_of(8, p.H_total[0, 2], p.H_total[2, 2])
        recs, scores, best = RR.score(rp, lists, f["trav"]["cost"], f["pot"], tab[s], (ga, gb), ref.oa, ref.ob)
        assert best >= 0
        assert lines[k] == dict(frame=k, set=s, best=best, feasible=int((scores != INF).sum()), length=int(recs[best, 0]), status=int(recs[best, 1]),
                                score=int(scores[best])), (k, lines[k])
        img = read_ppm(os.path.join(d4, "roll_%06d.ppm" % k))
        assert np.array_equal(img, RR.overlay(f["trav"]["rgb"][::-1].copy(), tab[s], recs, best, (ga, gb), ref.oa, ref.ob)), k
        k += 1
    assert k == 2 and len(lines) == 2
    # --grid-roll is refused without --grid-plan, its options without it or with a vehicle that is no three lengths
    for argv in (["--grid-local", d, "--grid-cost", d2, "--grid-roll", d4], ["--grid-local", d, "--grid-cost", d2, "--grid-plan", d3, "--grid-roll-vehicle", "0,0,0"],
                 ["--grid-local", d, "--grid-cost", d2, "--grid-plan", d3, "--grid-roll", d4, "--grid-roll-vehicle", "1,2"],
                 ["--grid-local", d, "--grid-cost", d2, "--grid-plan", d3, "--grid-roll", d4, "--grid-roll-unknown", "255"]):
        monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py"] + argv + common)
        with pytest.raises(SystemExit):
            SP.main()
