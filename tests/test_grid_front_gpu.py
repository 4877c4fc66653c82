"""GPU: the frontiers of the ground grid (include/svh_grid.h, "FRONTIERS"; csrc/grid_front_kernels.hip, csrc/grid_engine.cpp)
against the header's host form (core_front) and the restatement tests/grid_front_ref.py, which tests/test_grid_front.py pins on
the CPU.  Every comparison is exact: FRONT, LABEL, the table, the statistics and the image byte for byte.

Shapes: k_grid_front_tile runs one workgroup of 256 lanes per tile of T x T cells, T = FRONT_TILE; the per-cell kernels run 256
cells per workgroup and the ordered compactions 1024.  The windows 1 x 1, 1 x 9, 9 x 1, 3 x 3, (T - 1)^2, T^2, (T + 1)^2,
(2 T + 1) x (T + 1), (T + 1) x (2 T + 1) and 257 x 129 put lane, wave and tile edges on rows, on columns and on both.  The masks
(device_front_label on a caller's mask) make components cross tile borders by edges and by corners, so the merge does the
work; the scenes through the object are walls of obstacle points with gaps and cells without points, built with the helpers
of tests/test_grid_trav_gpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import grid_front_ref as FR
import grid_plan_ref as PR
import grid_ref as R
import grid_trav_ref as TR
import helpers as H
import test_grid as TG
import test_grid_front as TF
import test_grid_local_gpu as TL
import test_grid_plan_gpu as TPG
import test_grid_trav_gpu as TT
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2
U, S, F, O = TF.U, TF.S, TF.F, TF.O
RESTATE_CELLS = 65 * 65
LAUNCHES = 14                                                    # a constant of the build: grid_internal.h, FRONT_LAUNCHES


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


def run(G, state, cost=None, oa=0, ob=0, tag="", **kw):
    """device_front against core_front, and core_front against the restatement on small windows"""
    state = np.ascontiguousarray(state, np.uint8)
    cost = np.zeros(state.shape, np.uint8) if cost is None else np.ascontiguousarray(cost, np.uint8)
    p = G.default_front(**kw)
    got, want = G.device_front(p, state, cost, oa, ob), G.core_front(p, state, cost, oa, ob)
    for k, name in enumerate(("FRONT", "LABEL", "the table")):
        differ(tag, name, got[k], want[k])
    assert got[3][:4] == want[3][:4] and got[3][4] == LAUNCHES, (tag, got[3], want[3])
    if state.size <= RESTATE_CELLS:
        ref = FR.frontiers(FR.FrontParams(**kw), state, cost, oa, ob)
        for k, name in enumerate(("FRONT", "LABEL", "the table")):
            differ(tag + " (header against restatement)", name, want[k], ref[k])
        assert want[3][:4] == ref[3]
    return got


def label(G, mask, tag=""):
    """device_front_label against the restatement's flood fill"""
    mask = np.asarray(mask).astype(bool)
    got, launches = G.device_front_label(mask)
    differ(tag, "LABEL", got, FR.labels(mask))
    assert launches == 3, tag
    return got


def windows(T):
    return [(1, 1), (1, 9), (9, 1), (3, 3), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, T + 1), (T + 1, 2 * T + 1), (257, 129)]


# ---- the full chain on planes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(10))
def test_windows(G, k):
    T = G.FRONT_TILE
    nx, nz = windows(T)[k]
    rng = np.random.default_rng(1000 * nx + nz)
    for c, (kw, oa, ob) in enumerate(TF.CASES):
        for p_free in (0.3, 0.6, 0.9):
            state, cost = TF.random_planes(rng, nx, nz, p_free)
            run(G, state, cost, oa, ob, "%d x %d, case %d, %.1f free" % (nx, nz, c, p_free), **kw)
    free = np.full((nz, nx), F, np.uint8)
    flags, lab, recs, stats = run(G, free, None, 0, 0, "a free window, the border", border=1, min_size=1)
    assert stats[:4] == (nx * nz - max(nx - 2, 0) * max(nz - 2, 0), 1, 1, stats[0]) and (lab[flags != 0] == 0).all()
    assert run(G, free, None, 0, 0, "a free window")[3][:4] == (0, 0, 0, 0)


def test_the_hand_cases_on_the_device(G):
    ring = np.array([[O, F, O], [F, U, F], [O, F, O]], np.uint8)
    assert run(G, ring, min_size=4)[2].tolist() == [[1, 4, 0, 0, 2, 2, 1, 1, 1, 0]]
    corner = np.array([[F, U, O], [U, F, U], [O, U, O]], np.uint8)
    assert run(G, corner, min_size=2)[2].tolist() == [[0, 2, 0, 0, 1, 1, 1, 1, 1, 1]]
    assert run(G, np.full((4, 5), F, np.uint8), border=1, min_size=1)[2].tolist() == [[0, 14, 0, 0, 4, 3, 2, 2, 2, 3]]
    for n, kept in ((8, 1), (7, 0)):
        assert run(G, np.full((1, n), F, np.uint8), border=1, min_size=8)[3][:4] == (n, 1, kept, n * kept)
    row = np.array([[F, U, F, O, F, S, F]], np.uint8)
    for m, want in ((8, [1, 0, 1, 0, 0, 0, 0]), (16, [0, 0, 0, 0, 1, 0, 1]), (24, [1, 0, 1, 0, 1, 0, 1])):
        assert list(run(G, row, unexplored=m, min_size=1)[0][0] & 1) == want
    state = np.array([[U, F, U, F, U, F, U, F]], np.uint8)
    cost = np.array([[0, 100, 0, 101, 0, 99, 0, 253]], np.uint8)
    assert list(run(G, state, cost, min_size=1, max_cell_cost=100)[0][0]) == [0, 7, 0, 0, 0, 7, 0, 0]
    scrolled = run(G, ring, None, 5, -7, min_size=4)[2].tolist()
    assert scrolled == [[1, 4, 5, -7, 7, -5, 6, -6, 6, -7]]
    _, _, recs, _ = run(G, np.full((4, 1), F, np.uint8), border=1, min_size=1)        # sum 6 of 4: 1.5 -> 2
    assert recs[0, 6:].tolist() == [0, 2, 0, 2]


# ---- masks through the labelling stage ---------------------------------------------------------------------------------------
def masks(T, rng):
    n = 3 * T + 1
    ia, ib = np.meshgrid(np.arange(n), np.arange(n))
    out = [("empty", np.zeros((T + 1, 2 * T + 1), bool)), ("full", np.ones((T + 1, 2 * T + 1), bool)), ("the diagonal", ia == ib),
           ("the anti-diagonal", ia + ib == n - 1), ("a checkerboard", (ia + ib) % 2 == 0)]
    u = np.zeros((3 * T, 2 * T), bool)                           # a U upside down: the arms join in another tile, two labels merge late
    u[:2 * T + 3, 2] = u[:2 * T + 3, T + 3] = True
    u[2 * T + 2, 2:T + 4] = True
    out.append(("a U", u))
    comb = np.zeros((2 * T + 2, 3 * T + 1), bool)
    comb[0] = True
    comb[:, ::2] = True
    out.append(("a comb", comb))
    sp = TPG.spiral(4 * T) == 0
    out += [("a spiral", sp), ("a spiral wound the other way", sp[:, ::-1].copy())]
    for gap in (0, 1):                                           # two blobs that meet at the corner where four tiles meet, and one cell apart
        b = np.zeros((2 * T, 2 * T), bool)
        b[T - 3:T, T - 3:T] = True
        b[T + gap:T + gap + 3, T + gap:T + gap + 3] = True
        out.append(("two blobs, %d apart" % gap, b))
    for d in (0.05, 0.3, 0.6):
        out.append(("random %.2f" % d, rng.random((2 * T + 1, 4 * T + 3)) < d))
        out.append(("random %.2f, 257 x 129" % d, rng.random((129, 257)) < d))
    return out


def test_masks(G):
    T = G.FRONT_TILE
    for name, m in masks(T, np.random.default_rng(5)):
        lab = label(G, m, name)
        n = len(np.unique(lab[lab >= 0]))
        if name in ("full", "the diagonal", "the anti-diagonal", "a checkerboard", "a U", "a comb", "a spiral", "a spiral wound the other way",
                    "two blobs, 0 apart"):
            assert n == 1 and (lab[m] == np.flatnonzero(m.ravel())[0]).all(), name
        if name == "two blobs, 1 apart":
            assert n == 2
        if name == "empty":
            assert (lab == -1).all()


def test_the_largest_mask(G):
    """1024 x 1024 at a density of 0.3"""
    mask = np.random.default_rng(6).random((1024, 1024)) < 0.3
    lab = label(G, mask, "1024 x 1024")
    assert len(np.unique(lab[lab >= 0])) > 1000


def test_the_same_bytes_twice(G):
    T = G.FRONT_TILE
    rng = np.random.default_rng(7)
    state, cost = TF.random_planes(rng, 3 * T + 5, 2 * T + 3, 0.7)
    p = G.default_front(min_size=3, border=1)
    first = G.device_front(p, state, cost, 3, -4)
    for _ in range(3):
        again = G.device_front(p, state, cost, 3, -4)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], again[:3])) and again[3] == first[3]
    sp = TPG.spiral(4 * T) == 0
    one = G.device_front_label(sp)[0]
    assert all(G.device_front_label(sp)[0].tobytes() == one.tobytes() for _ in range(3))


def test_the_launch_count_does_not_depend_on_the_scene(G):
    T = G.FRONT_TILE
    n = 4 * T
    sp = TPG.spiral(n) == 0
    rng = np.random.default_rng(8)
    scenes = [("no frontier", np.full((n, n), O, np.uint8)), ("a spiral of free cells between unknown walls", np.where(sp, F, U).astype(np.uint8)),
              ("random", TF.random_planes(rng, n, n, 0.7)[0])]
    counts = []
    for name, state in scenes:
        flags, lab, recs, stats = run(G, state, None, 0, 0, name, min_size=2, border=1)   # the border: the corridor's outer corners too
        counts.append(stats[4])
        if name.startswith("a spiral"):
            assert stats[:4] == (int(sp.sum()), 1, 1, int(sp.sum())) and (flags[sp] != 0).all()     # every corridor cell is a frontier cell
        if name == "no frontier":
            assert stats[:4] == (0, 0, 0, 0)
    assert counts == [LAUNCHES] * 3
    assert [G.device_front_label(m)[1] for m in (np.zeros((n, n), bool), sp, rng.random((n, n)) < 0.3)] == [3, 3, 3]


# ---- through the object --------------------------------------------------------------------------------------------------
FRONT = dict(min_size=6)                                         # the four cells round a single hole are dropped


def holes(nx, nz, rng):
    """cells without points: a block in the far corner, a strip along the near edge, and single cells (noise: components too
    small to keep)"""
    ia, ib = np.meshgrid(np.arange(nx), np.arange(nz))
    return ((ia >= nx - 12) & (ib >= nz - 10)) | ((ib <= 1) & (ia >= 6) & (ia < nx // 2)) | (rng.random((nz, nx)) < 0.01)


def build(G, nx, nz, seed, rays=True, **pkw):
    rng = np.random.default_rng(seed)
    ref, g = TPG.pair(G, nx, nz, **pkw)
    walls = TPG.walls(nx, nz)
    pts = TT.fill(ref, rng, walls, holes(nx, nz, rng) & ~walls)
    if rays:                                                      # rays from cell (3, 4): the holes they cross are seen
        origin = TL.centre(ref, 3, 4)
        g.add_points_from(pts, origin)
        ref.add_from(pts, origin)
    else:
        TT.add_both(g, ref, pts)
    g.set_frontier(**FRONT)
    ref.front = FR.FrontParams(**FRONT)
    return ref, g, rng


def expected(ref):
    tr = ref.trav()
    flags, lab, recs, stats = FR.frontiers(ref.front, ref.local_planes()["state"], tr["cost"], ref.oa, ref.ob)
    return dict(flags=flags, label=lab, recs=recs, stats=stats, image=FR.overlay(tr["rgb"][::-1].copy(), flags), cost=tr["cost"])


def check(G, g, ref, tag=""):
    """planes, table, statistics and image against the restatement on its own STATE and COST; returns what it expects"""
    w = expected(ref)
    differ(tag, "COST", g.trav_plane(G.TRAV_COST), w["cost"])
    differ(tag, "FRONT", g.front_plane(G.FRONT_FLAGS), w["flags"])
    differ(tag, "LABEL", g.front_plane(G.FRONT_LABEL), w["label"])
    differ(tag, "the table", g.frontiers(), w["recs"])
    assert g.frontier_count == len(w["recs"])
    assert g.frontier_stats() == w["stats"] + (LAUNCHES,), (tag, g.frontier_stats(), w["stats"])
    differ(tag, "the image", g.render_frontiers(), w["image"])
    return w


@pytest.mark.parametrize("shape", ["65 x 65", "(2T + 1) x (T + 1)"])
def test_scenes_of_walls_with_gaps(G, shape):
    T = G.FRONT_TILE
    nx, nz = (65, 65) if shape == "65 x 65" else (2 * T + 1, T + 1)
    ref, g, rng = build(G, nx, nz, 41)
    w = check(G, g, ref, "unseen")
    assert w["stats"][0] > 0
    if shape == "65 x 65":
        assert w["stats"][2] >= 1 and w["stats"][1] > w["stats"][2]                    # kept components, and dropped noise
    img = g.render_frontiers()
    for colour, bits in ((G.FRONT_REP_COLOUR, 7), (G.FRONT_KEPT_COLOUR, 3), (G.FRONT_DROPPED_COLOUR, 1)):
        assert np.array_equal((img == colour).all(axis=2), w["flags"][::-1] == bits)
    # the table with less room, with none
    for cap in (1, 0, len(w["recs"]), len(w["recs"]) + 3):
        assert np.array_equal(g.frontiers(cap=cap), w["recs"][:cap]) and g.frontier_count == len(w["recs"])
    seen = []
    for m in (16, 24, 8):
        g.set_frontier(unexplored=m)
        ref.front.unexplored = m
        seen.append(check(G, g, ref, "unexplored %d" % m)["stats"][0])
    assert seen[1] >= max(seen[0], seen[2])
    if shape == "65 x 65":
        assert seen[0] > 0 and seen[1] > seen[2] and seen[1] > seen[0]                 # some holes are seen, some are not


def test_the_cache_and_every_invalidation(G):
    nx = nz = 65
    ref, g, rng = build(G, nx, nz, 42)
    w = check(G, g, ref, "before")
    flags = g.front_plane(G.FRONT_FLAGS)
    G.lib().svh_test_fail_at(b"launch:1:0")                                           # nothing changed: no launch, from the cache
    assert g.front_plane(G.FRONT_FLAGS).tobytes() == flags.tobytes() and np.array_equal(g.frontiers(), w["recs"])
    assert g.frontier_stats() == w["stats"] + (LAUNCHES,)
    G.lib().svh_test_fail_at(None)
    # an add: the hole in the far corner is closed by free cells
    ia, ib = np.meshgrid(np.arange(nx - 12, nx), np.arange(nz - 10, nz))
    TT.add_both(g, ref, np.concatenate([TL.at_cells(ref, ia.ravel(), ib.ravel(), 0.0)] * 2))
    w2 = check(G, g, ref, "after an add")
    assert w2["stats"][0] < w["stats"][0]
    # a scroll: the labels are window indexes and the boxes global cells; the strips that enter are unknown
    g.scroll(3, -2)
    ref.scroll(3, -2)
    w3 = check(G, g, ref, "scrolled")
    assert g.window() == (3, -2) and w3["label"].tobytes() != w2["label"].tobytes() and w3["stats"][0] > w2["stats"][0]
    g.follow(TL.centre(ref, 10, 5), 4, 4)
    ref.follow(TL.centre(ref, 10, 5), 4, 4)
    w4 = check(G, g, ref, "followed")
    # the traversability: cells beside the walls cost more than max_cell_cost
    g.set_frontier(max_cell_cost=100)
    ref.front.max_cell_cost = 100
    w5 = check(G, g, ref, "max_cell_cost")
    g.set_traversability(inflate=2.0)
    ref.T.inflate = np.float32(2.0)
    w6 = check(G, g, ref, "after set_traversability")
    assert w6["flags"].tobytes() != w5["flags"].tobytes()
    # the frontier parameters
    for kw in (dict(min_size=1), dict(border=1), dict(min_size=30, max_cell_cost=252)):
        g.set_frontier(**kw)
        for k, v in kw.items():
            setattr(ref.front, k, v)
        check(G, g, ref, "set_frontier %r" % kw)
    assert g.frontier_params().asdict() == dict(max_cell_cost=252, min_size=30, unexplored=8, border=1)
    g.clear()
    ref.clear()
    w7 = check(G, g, ref, "cleared")                                                  # nothing is free
    assert w7["stats"] == (0, 0, 0, 0) and w4["stats"][0] > 0


def test_goals_from_the_frontiers(G):
    nx = nz = 65
    ref, g, rng = build(G, nx, nz, 43)
    w = check(G, g, ref, "before")
    kept = len(w["recs"])
    assert kept >= 2
    assert g.set_goals_frontiers() == kept
    ref.set_goals(w["recs"][:, 8:10])
    f = TPG.check(G, g, ref, "goals from the frontiers")
    assert g.plan_stats()[:2] == (kept, kept) and f["counted"] == kept              # every representative is passable and inside
    start = TL.centre(ref, 3, 4)
    st, cells, cost = TPG.check_path(G, g, ref, f, start, "from the origin's cell")
    assert st == G.PATH_FOUND and tuple(cells[-1]) in {tuple(r) for r in w["recs"][:, 8:10]}
    assert w["flags"][cells[-1][1] - ref.ob, cells[-1][0] - ref.oa] == 7
    # a snapshot: the goals are global cells and stay when the frontier changes
    g.scroll(2, 1)
    ref.scroll(2, 1)
    check(G, g, ref, "scrolled")
    assert g.plan_stats()[0] == kept
    TPG.check(G, g, ref, "the goals after a scroll")
    g.set_frontier(min_size=10 ** 6)
    assert g.set_goals_frontiers() == 0 and g.plan_stats()[:2] == (0, 0)


# ---- failures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["malloc:1", "malloc:2", "malloc:5", "malloc:7", "launch:1", "launch:2", "copy:1", "copy:2", "copy:4", "copy:6",
                                  "copy:7", "wait:1", "wait:2", "wait:3"])
def test_a_failed_frontier_call_leaves_the_grid_and_the_field(G, spec):
    """with the cost planes and the field cached and a new object: malloc:1 is the two planes, 2 to 4 the block counts and the
    control words, 5 to 7 what the components size; launch:1 the labelling, launch:2 the table; copy:1 clears the control words,
    copy:2 and wait:1 bring the number of components, copy:3 to 5 clear the accumulators, copy:6 and wait:2 bring the kept
    count, copy:7 and wait:3 the plane"""
    nx, nz = 65, 65
    ref, g, rng = build(G, nx, nz, 44)
    TPG.set_goals(g, ref, TPG.goals_of(ref, nx, nz))
    f = TPG.check(G, g, ref, "the field")
    before = TL.snapshot(G, g)
    pot = g.plan_plane(G.PLAN_POT)
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.front_plane(G.FRONT_LABEL)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    G.lib().svh_test_fail_at(b"launch:1:0")                                           # the grid, the cost planes and the field: from the cache
    assert g.plan_plane(G.PLAN_POT).tobytes() == pot.tobytes() and g.trav_plane(G.TRAV_COST).tobytes() == f["trav"]["cost"].tobytes()
    G.lib().svh_test_fail_at(None)
    assert TL.same(TL.snapshot(G, g), before) and g.plan_stats()[0] == 7
    w = check(G, g, ref, spec + ": the call repeated")
    # with the result cached: the image's own launch, the table's copy
    for call, what in ((lambda: g.render_frontiers(), b"launch:1"), (lambda: g.frontiers(), b"copy:1"), (lambda: g.set_goals_frontiers(), b"wait:1")):
        G.lib().svh_test_fail_at(what)
        with pytest.raises(G.SvhError) as e:
            call()
        G.lib().svh_test_fail_at(None)
        assert e.value.code == HIP_ERR and g.plan_stats()[0] == 7                     # the goals are as they were
        check(G, g, ref, spec + ": after a failed call on the cached result")
    TPG.check(G, g, ref, "the field afterwards")


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte(G, hip):
    nx, nz = 65, 33
    ref, g, rng = build(G, nx, nz, 45)
    w = check(G, g, ref, "before")
    L = g._L
    buf = np.full(nx * nz * 4, 0xAB, np.uint8)
    dev = Dev(hip, nx * nz * 4 + 16)
    for kw in TF.BAD:
        p = G.default_front(**kw)
        assert L.svh_grid_set_frontier(g._h, C.byref(p)) == BAD_ARG and "svh_grid_set_frontier" in G.last_error(), kw
    assert g.frontier_params().asdict() == dict(max_cell_cost=252, min_size=FRONT["min_size"], unexplored=8, border=0)
    n = C.c_int64(-7)
    calls = [lambda: L.svh_grid_set_frontier(g._h, None), lambda: L.svh_grid_get_frontier(g._h, None),
             lambda: L.svh_grid_get_front_plane(g._h, 2, buf.ctypes.data, 0), lambda: L.svh_grid_get_front_plane(g._h, -1, buf.ctypes.data, 0),
             lambda: L.svh_grid_get_front_plane(g._h, 0, None, 0), lambda: L.svh_grid_get_front_plane(g._h, G.FRONT_LABEL, dev.addr + 1, 1),
             lambda: L.svh_grid_get_frontiers(g._h, None, 1, C.addressof(n)), lambda: L.svh_grid_get_frontiers(g._h, buf.ctypes.data, -1, C.addressof(n)),
             lambda: L.svh_grid_get_frontiers(g._h, buf.ctypes.data, 1, None), lambda: L.svh_grid_get_frontier_stats(g._h, None),
             lambda: L.svh_grid_render_frontiers(g._h, None, 0)]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG and "svh_grid" in G.last_error(), k
    assert (buf == 0xAB).all() and (dev.get() == 0xEE).all() and n.value == -7
    check(G, g, ref, "after")
    # device pointers: FRONT, LABEL and the image, nothing beyond them
    for which, name, nbytes in ((G.FRONT_FLAGS, "flags", nx * nz), (G.FRONT_LABEL, "label", 4 * nx * nz)):
        out = Dev(hip, nbytes + 16)
        g.front_plane(which, device_ptr=out.addr)
        got = out.get()
        assert got[:nbytes].tobytes() == w[name].tobytes() and (got[nbytes:] == 0xEE).all(), name
    out = Dev(hip, 3 * nx * nz + 16)
    g.render_frontiers(device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:3 * nx * nz].reshape(nz, nx, 3), w["image"]) and (got[3 * nx * nz:] == 0xEE).all()


def test_frontiers_need_a_traversability_that_fits(G):
    """cells of 5 mm: the default inflation radius would be 300 cells; the frontier entries refuse as svh_grid_get_trav does"""
    g = G.Grid(G.default_params(nx=9, nz=9, cell=0.005, x0=0.0, z0=0.0, T=R.frame_camera(0.0), min_points=1))
    g.add_points(np.array([[0.0225, 0.0, 0.0225, 0.5]], np.float32))
    buf = np.full(81 * 4, 0xAB, np.uint8)
    n = C.c_int64(-7)
    L = g._L
    for call in (lambda: L.svh_grid_get_front_plane(g._h, 0, buf.ctypes.data, 0), lambda: L.svh_grid_get_frontier_stats(g._h, buf.ctypes.data),
                 lambda: L.svh_grid_get_frontiers(g._h, buf.ctypes.data, 1, C.addressof(n)), lambda: L.svh_grid_plan_set_goals_frontiers(g._h),
                 lambda: L.svh_grid_render_frontiers(g._h, buf.ctypes.data, 0)):
        assert call() == BAD_ARG and "svh_grid_set_traversability" in G.last_error()
    assert (buf == 0xAB).all() and n.value == -7
    g.set_traversability(inscribed=0.004, inflate=0.02)
    g.set_frontier(min_size=1)
    assert g.front_plane(G.FRONT_FLAGS)[4, 4] == 7 and g.frontiers().tolist() == [[40, 1, 4, 4, 4, 4, 4, 4, 4, 4]]
    assert g.set_goals_frontiers() == 1


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------
def test_pipeline_grid_frontiers(G, tmp_path, monkeypatch, capsys):
    """--grid-local DIR --grid-cost DIR2 --grid-frontiers DIR3 --grid-unexplored both --grid-frontier-min 2 on the two golden
    frames: one image and one line of frontiers.jsonl per frame, the restatement's after the same steps.  Two frames leave ten
    free cells, none beside a cell that no ray passed: the cells that were looked through count as unexplored too, and a
    component of two cells is kept"""
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
    d, d2, d3 = str(tmp_path / "loc"), str(tmp_path / "cost"), str(tmp_path / "front")
    common = ["--grid-slope", "2.0", "--grid-inscribed", "0.1", "--grid-inflate", "0.5", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-frontiers", d3, "--grid-unexplored", "both", "--grid-frontier-min", "2"] + common)
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("frontiers: ") and "2 images and frontiers.jsonl" in l for l in out), out[-4:]
    assert sorted(os.listdir(d3)) == ["frontiers.jsonl"] + ["frontiers_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(d3, "frontiers.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = PR.Grid(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0), TR.TravParams(max_slope=2.0, inscribed=0.1, inflate=0.5), PR.PlanParams(unknown=100))
    ref.front = FR.FrontParams(unexplored=24, min_size=2)
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre_ = p.H_total[:3, 3]
        ref.follow(centre_, 48, 80)
        ref.add_from(p.view.points(p.view.count(view.LISTS) - 1), centre_)
        w = expected(ref)
        ref.set_goals(w["recs"][:, 8:10])
        f = ref.field()
        status, cells, cost = ref.path(centre_, f)
        assert lines[k] == dict(frame=k, frontier_cells=w["stats"][0], components=w["stats"][1], kept=w["stats"][2], status=status,
                                length=len(cells), cost=cost), (k, lines[k])
        img = read_ppm(os.path.join(d3, "frontiers_%06d.ppm" % k))
        want = w["image"].copy()
        for ga, gb in cells:
            want[160 - 1 - (gb - ref.ob), ga - ref.oa] = PR.PATH_COLOUR
        assert img.shape == (160, 96, 3) and np.array_equal(img, want), k
        k += 1
    assert k == 2 and len(lines) == 2 and w["stats"][2] > 0
    # --grid-frontiers is refused without --grid-cost, --grid-unexplored without --grid-frontiers or with another word
    for argv in (["--grid-local", d, "--grid-frontiers", d3], ["--grid-local", d, "--grid-cost", d2, "--grid-unexplored", "both"],
                 ["--grid-local", d, "--grid-cost", d2, "--grid-frontiers", d3, "--grid-unexplored", "all"],
                 ["--grid-local", d, "--grid-cost", d2, "--grid-frontiers", d3, "--grid-frontier-min", "0"]):
        monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py"] + argv + common)
        with pytest.raises(SystemExit):
            SP.main()
