"""GPU: the dynamics of the ground grid (include/svh_grid.h, "DYNAMICS": svh_grid_set_dynamics, svh_grid_observe_*,
svh_grid_get_dyn, svh_grid_get_dyn_stats, svh_grid_render_dyn; csrc/grid_dyn_kernels.hip, csrc/grid_engine.cpp) against the numpy
restatement tests/grid_dyn_ref.py, which tests/test_grid_dyn.py pins on the CPU.  Every comparison is exact, per observation: the
seven planes of svh_grid_get bit for bit, the two local planes, the three planes of the layer, the point, ray and layer statistics,
the window, the renders.

Shapes: k_grid_sight casts 64 end cells of one row (forward-major lines) or of one column (lateral-major lines) per wave, four
waves per workgroup; k_grid_body, k_grid_settle and k_grid_dyn_enter run 256 cells per workgroup.  The windows 1 x 1, 1 x 9, 9 x 1,
64 x 1, 65 x 65 and 257 x 129 put lane, wave and workgroup edges on rows, on columns and on both."""
import ctypes as C

import numpy as np
import pytest

import grid_dyn_ref as DR
import grid_local_ref as LR
import grid_ref as R
import test_grid as TG
import test_grid_dyn as TD
import test_grid_local_gpu as TL
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARG, HIP_ERR = -1, -2
CELL = TD.CELL
WINDOWS = [(1, 1), (1, 9), (9, 1), (64, 1), (65, 65), (257, 129)]


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


def pair(G, dyn=None, **kw):
    """the restatement and the object with the same window (the hand case's: cells of 0.5, h = 1.5 - y) and the same layer"""
    P, Pc = TG.both(G, **TD.hand_kw(**kw))
    dyn = dict(dyn or {})
    ref, g = DR.Grid(P, DR.DynParams(**dyn)), G.Grid(Pc)
    g.set_dynamics(G.default_dyn(**dyn))
    return ref, g


def centre(ref, ia, ib, h=1.5):
    """the map-frame position in the middle of window cell (ia, ib) at height h, in double"""
    return [(ref.oa + ia + 0.5) * CELL, 1.5 - h, (ref.ob + ib + 0.5) * CELL]


def at(ref, ia, ib, h, val=0.5):
    p = TD.at(ia, ib, h, val)
    p[:, 0] += F(ref.oa * CELL)                                      # cell centres stay exact in fp32
    p[:, 2] += F(ref.ob * CELL)
    return p


def check(G, g, ref, tag=""):
    """everything the object can be asked for against the restatement"""
    got = TL.check(G, g, ref, tag)
    want = ref.dyn_planes()
    for k, name in ((G.DYN_AGE, "age"), (G.DYN_CONTRA, "contra"), (G.DYN_THROUGH, "through")):
        a = g.dyn_plane(k)
        assert a.dtype == np.int32 and a.shape == want[name].shape, (tag, name)
        if not np.array_equal(a, want[name]):
            bad = np.argwhere(a != want[name])
            raise AssertionError("%s: %s differs in %d places, first %s: got %d, wanted %d" % (
                tag, name, len(bad), tuple(bad[0]), a[tuple(bad[0])], want[name][tuple(bad[0])]))
        got[name] = a
    got["dyn_stats"] = g.dyn_stats()
    assert got["dyn_stats"] == ref.dyn_stats, (tag, got["dyn_stats"], ref.dyn_stats)
    got["render_dyn"] = g.render_dyn()
    assert np.array_equal(got["render_dyn"], ref.render_dyn()), (tag, "render_dyn")
    return got


def snapshot(G, g):
    out = TL.snapshot(G, g)
    for k, name in ((G.DYN_AGE, "age"), (G.DYN_CONTRA, "contra"), (G.DYN_THROUGH, "through")):
        out[name] = g.dyn_plane(k)
    out["dyn_stats"], out["render_dyn"] = g.dyn_stats(), g.render_dyn()
    return out


def both(g, ref, pts, origin):
    g.observe_points(pts, origin)
    ref.observe(pts, origin)


def scene(ref, rng, n, tall=0.3):
    """n random points over the window as it stands and a little around it: ground near h = 0, tall things up to 1.9, overhead
    points, drops, a few that are no points at all"""
    P = ref.P
    ia, ib = rng.uniform(-1, P.nx + 1, n), rng.uniform(-1, P.nz + 1, n)
    kind = rng.random(n)
    h = np.where(kind < tall, rng.uniform(0.21, 1.9, n), np.where(kind < 0.9, rng.uniform(-0.05, 0.15, n), np.where(kind < 0.95, 2.5, -1.0)))
    p = np.stack([(ref.oa + ia) * CELL, 1.5 - h, (ref.ob + ib) * CELL, rng.uniform(-0.1, 1.1, n)], 1).astype(F)
    if n >= 32:
        k = rng.choice(n, n // 32, replace=False)
        p[k, rng.integers(0, 4, len(k))] = rng.choice(np.array([np.nan, np.inf, -3e38, -0.0], F), len(k))
    return p


def origins(nx, nz):
    """a corner, an edge, the middle and, in the smaller windows, the opposite corner, as window cells"""
    seen = []
    for o in ((0, 0), (nx // 2, 0), (nx // 2, nz // 2)) + (((nx - 1, nz - 1),) if nx * nz < 10000 else ()):
        if o not in seen:
            seen.append(o)
    return seen


# ---- windows and origins -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_windows_and_origins(G, nx, nz):
    """from each origin three observations on one grid: a scene with tall things, then twice the ground alone, whose lines go
    through what the first left (clear_frames 2: the second clears)"""
    rng = np.random.default_rng(100 + nx)
    n = min(6 * nx * nz, 12000)
    for ia, ib in origins(nx, nz):
        ref, g = pair(G, dict(min_through=1), nx=nx, nz=nz)
        o = centre(ref, ia, ib, h=1.5)
        both(g, ref, scene(ref, rng, n), o)
        check(G, g, ref, "%d x %d from (%d, %d): the scene" % (nx, nz, ia, ib))
        for k in range(2):
            both(g, ref, scene(ref, rng, n, tall=0.0), o)
            check(G, g, ref, "%d x %d from (%d, %d): ground %d" % (nx, nz, ia, ib, k))
        if nx * nz >= 64:
            assert ref.dyn_stats["cleared"] > 0 and ref.dyn_stats["confirmed"] > 0, (nx, nz, ia, ib)


def test_every_cell_an_end_cell(G):
    """65 x 65 with one point per cell at random heights, on top of a grid in every state"""
    rng = np.random.default_rng(7)
    ia, ib = np.meshgrid(np.arange(65), np.arange(65))
    ref, g = pair(G, dict(min_through=2, clear_frames=1, max_age=2), nx=65, nz=65)
    for t, (oa, ob) in enumerate(((32, 32), (0, 64), (64, 3))):
        pts = at(ref, ia.ravel(), ib.ravel(), rng.choice(np.array([0.0, 0.0, 0.1, 0.3, 0.9, 1.9, -0.4]), 65 * 65), 0.25)
        both(g, ref, pts[rng.permutation(len(pts))], centre(ref, oa, ob, h=[1.5, 0.4, 2.0][t]))
        got = check(G, g, ref, "frame %d" % t)
        assert got["rays"][0] == 65 * 65 * (t + 1)
    assert ref.dyn_stats["cleared"] > 50 and (ref.dyn_planes()["through"] > 0).sum() > 50


def test_runs_with_mixed_verdicts(G):
    """the end cells of one row, far away: near the origin their lines stand in the same cell at step k, at heights that straddle the
    body of the tall cell there, so the sum of a run mixes lanes that go through with lanes that do not"""
    ref, g = pair(G, dict(clear_frames=0), nx=65, nz=65)
    stored = at(ref, [32] * 4 + [31] * 2, [2] * 4 + [3] * 2, [0.25, 0.5, 1.0, 1.0, 0.3, 0.8])
    g.add_points(stored)
    ref.add(stored)
    rng = np.random.default_rng(8)
    h = rng.uniform(-40.0, 1.9, 3 * 65)                            # q_2 = 1536 + rdiv(2 (q_e - 1536), 64): in the body for h in about -39 .. -18
    pts = at(ref, np.tile(np.arange(65), 3), np.full(3 * 65, 64), h)
    both(g, ref, pts, centre(ref, 32, 0))
    got = check(G, g, ref, "a row of ends")
    run = got["passed"][2, 32]
    assert 0 < got["through"][2, 32] < run and run > 64 and 0 < got["through"][3, 31] < got["passed"][3, 31]
    # the same down a column: lateral-major lines
    ref, g = pair(G, dict(clear_frames=0), nx=65, nz=65)
    stored = at(ref, [2] * 3, [32] * 3, [0.25, 0.5, 1.0])
    g.add_points(stored)
    ref.add(stored)
    pts = at(ref, np.full(3 * 65, 64), np.tile(np.arange(65), 3), h)
    both(g, ref, pts, centre(ref, 0, 32))
    got = check(G, g, ref, "a column of ends")
    assert 0 < got["through"][32, 2] < got["passed"][32, 2]


@pytest.mark.parametrize("case", ["down", "up", "level", "n1"])
def test_heights_at_the_limits(G, case):
    """end points just inside +-2^20 and an origin at the clearance: dq of either sign near 2^31 and zero, lines of one step"""
    top = 1048575.0
    kw = dict(nx=70, nz=9, cell=CELL, x0=0.0, z0=0.0, T=R.frame_camera(0.0), min_points=1, step=0.2, drop=0.3, clearance=top)
    P, Pc = TG.both(G, **kw)
    ref, g = DR.Grid(P, DR.DynParams(min_through=1, margin=0.0)), G.Grid(Pc)
    g.set_dynamics(min_through=1, margin=0.0)

    def pt(ia, ib, h):
        ia, ib, h = np.broadcast_arrays(np.asarray(ia), np.asarray(ib), np.asarray(h, np.float64))
        p = np.zeros((ia.size, 4), F)
        p[:, 0], p[:, 1], p[:, 2], p[:, 3] = (ia.ravel() + 0.5) * CELL, -h.ravel(), (ib.ravel() + 0.5) * CELL, 0.5
        return p
    rng = np.random.default_rng(9)
    cols = np.arange(0, 69)
    stored = np.concatenate([pt(cols, 4, rng.uniform(-top, 0.0, 69)), pt(cols, 4, rng.uniform(1.0, top, 69)), pt(cols, 3, -top), pt(cols, 3, top)])
    g.add_points(stored)
    ref.add(stored)
    h_o, h_e = dict(down=(top, -top), up=(-top, top), level=(top, top), n1=(top, -top))[case]
    o = [0.5 * CELL, -h_o, 4.5 * CELL]                              # cell (0, 4)
    ends = pt([1, 1, 0], [4, 5, 3], h_e) if case == "n1" else np.concatenate([pt(69, np.arange(9), h_e), pt(np.arange(40, 69), 0, h_e), pt(35, 8, [h_e, 0.0])])
    both(g, ref, ends, o)
    got = check(G, g, ref, case)
    assert LR.place(P, 0, 0, np.array([[o[0], o[1], o[2], 0]], F))[3][0] == int(h_o * 1024)
    if case in ("down", "up"):
        assert (got["through"] > 0).sum() > 20 and got["contra"].sum() > 20
    both(g, ref, ends, o)
    check(G, g, ref, case + ": again, clearing")


# ---- bit-equality with the _from entry ----------------------------------------------------------------------------------------------
def test_without_clearing_an_observation_is_an_add_from(G):
    rng = np.random.default_rng(10)
    ref, g = pair(G, dict(clear_frames=0, max_age=0), nx=65, nz=33)
    plain = G.Grid(g.params)
    moves = [(0, 0), (1, 0), (70, 0), (0, -1), (-3, 5), (7, 7)]
    for t, (da, db) in enumerate(moves):
        if (da, db) != (0, 0):
            for x in (g, plain, ref):
                x.scroll(da, db)
        pts = scene(ref, rng, 5000)
        o = centre(ref, int(rng.integers(0, 65)), int(rng.integers(0, 33)), h=float(rng.uniform(0.0, 2.0)))
        both(g, ref, pts, o)
        plain.add_points_from(pts, o)
        a, b = TL.snapshot(G, g), TL.snapshot(G, plain)
        assert TL.same(a, b), "frame %d" % t
        check(G, g, ref, "frame %d" % t)
    assert g.dyn_stats()["cleared"] == 0 and g.dyn_plane(G.DYN_CONTRA).max() >= 1 and plain.ray_stats() == g.ray_stats()


# ---- the scenario -------------------------------------------------------------------------------------------------------------------
def test_scenario_a_block_crosses_the_ground(G):
    """what the layer is for: with plain adds the block's whole trail is obstacle at the end; with observations and clear_frames 2
    only where it stands and the column it left last"""
    P, Pc = TG.both(G, **TD.SCENE_KW)
    plain, g, ref = G.Grid(Pc), G.Grid(Pc), DR.Grid(P, DR.DynParams(clear_frames=2))
    g.set_dynamics(clear_frames=2)
    for t in range(TD.SCENE_FRAMES):
        pts = TD.scene_frame(t)
        plain.add_points_from(pts, TD.SCENE_ORIGIN)
        both(g, ref, pts, TD.SCENE_ORIGIN)
        check(G, g, ref, "frame %d" % t)
    assert TD.scene_obstacles(plain.classes()) == TD.SCENE_TRAIL
    cls = g.classes()
    assert TD.scene_obstacles(cls) == TD.SCENE_LEFT
    assert all((cls[b, a] & 3) == R.FREE for a, b in TD.SCENE_TRAIL - TD.SCENE_LEFT)
    assert g.dyn_stats() == ref.dyn_stats == dict(observations=8, cleared=12, aged=0, confirmed=32)
    assert np.array_equal(plain.local_plane(G.LOCAL_PASS), g.local_plane(G.LOCAL_PASS))
    img = g.render_dyn()[::-1]
    assert tuple(img[4, 9]) == G.DYN_EVENT_COLOUR and tuple(img[4, 10]) == (255, 127, 0) and tuple(img[4, 11]) == (255, 0, 0)


# ---- the torus ------------------------------------------------------------------------------------------------------------------------
def test_state_follows_the_torus(G):
    rng = np.random.default_rng(11)
    nx, nz = 65, 33
    ref, g = pair(G, dict(min_through=1, clear_frames=3, max_age=2), nx=nx, nz=nz)
    moves = [(1, 0), (0, -1), (-3, 5), (0, 0), (40, -20), (nx, 0), (2, 2), (0, -nz), (-1, 1), (-200, 90)]
    for t, (da, db) in enumerate(moves):
        both(g, ref, scene(ref, rng, 3000, tall=0.3 if t % 2 == 0 else 0.0), centre(ref, int(rng.integers(0, nx)), int(rng.integers(0, nz))))
        check(G, g, ref, "frame %d" % t)
        if (da, db) != (0, 0):
            g.scroll(da, db)
            ref.scroll(da, db)
            got = check(G, g, ref, "frame %d, scrolled by (%d, %d)" % (t, da, db))
            if abs(da) >= nx or abs(db) >= nz:
                assert (got["age"] == -1).all() and not got["contra"].any() and not got["through"].any() and got["dyn_stats"]["observations"] == t + 1
    assert ref.dyn_stats["cleared"] > 0 and ref.dyn_stats["aged"] > 0


def test_clear_set_window_drop_and_set_again(G):
    rng = np.random.default_rng(12)
    ref, g = pair(G, dict(min_through=1), nx=65, nz=65)
    g.scroll(5, -9)
    ref.scroll(5, -9)

    def two_frames(tag):
        both(g, ref, scene(ref, rng, 4000), centre(ref, 10, 10))
        both(g, ref, scene(ref, rng, 4000, tall=0.0), centre(ref, 10, 10))
        got = check(G, g, ref, tag)
        assert got["contra"].any() and got["through"].any()
        return got
    two_frames("filled")
    g.clear()
    ref.clear()
    got = check(G, g, ref, "cleared")
    assert got["window"] == (5, -9) and (got["age"] == -1).all() and not got["contra"].any() and got["dyn_stats"] == dict.fromkeys(DR.STATS, 0)
    assert two_frames("after the clear")["dyn_stats"]["observations"] == 2
    g.set_window(0.0, 0.0)
    ref.set_window(0.0, 0.0)
    got = check(G, g, ref, "set_window")
    assert got["window"] == (0, 0) and (got["age"] == -1).all() and got["dyn_stats"]["observations"] == 0
    two_frames("after set_window")
    # new parameters keep CONTRA and LAST
    before = snapshot(G, g)
    g.set_dynamics(clear_frames=5, margin=0.3)
    ref.set_dynamics(DR.DynParams(clear_frames=5, min_through=1, margin=0.3))
    assert g.dynamics().asdict() == dict(clear_frames=5, min_through=1, margin=F(0.3), max_age=0) and TL.same(snapshot(G, g), before)
    both(g, ref, scene(ref, rng, 4000, tall=0.0), centre(ref, 10, 10))
    check(G, g, ref, "new parameters")
    # dropping the layer: its entries refuse, the grid stands; setting it again starts from empty planes, the stamp goes on
    grid_before = TL.snapshot(G, g)
    g.drop_dynamics()
    ref.set_dynamics(None)
    o = np.array(centre(ref, 10, 10))
    buf = np.zeros(65 * 65 * 3, np.int32)
    assert g._L.svh_grid_observe_points(g._h, None, 0, 0, o.ctypes.data) == BAD_ARG and "svh_grid_set_dynamics" in G.last_error()
    assert g._L.svh_grid_get_dyn(g._h, 0, buf.ctypes.data, 0) == BAD_ARG and g._L.svh_grid_render_dyn(g._h, buf.ctypes.data, 0) == BAD_ARG
    assert TL.same(TL.snapshot(G, g), grid_before)
    g.set_dynamics(min_through=1)
    ref.set_dynamics(DR.DynParams(min_through=1))
    got = check(G, g, ref, "set again")
    assert (got["age"] == -1).all() and not got["contra"].any() and got["dyn_stats"]["observations"] == 3
    two_frames("after setting again")


def test_plain_adds_with_the_layer_set(G):
    """interleaved adds write the accumulators and leave CONTRA and LAST alone"""
    rng = np.random.default_rng(13)
    ref, g = pair(G, dict(min_through=1, clear_frames=3, max_age=3), nx=65, nz=33)
    for t in range(6):
        both(g, ref, scene(ref, rng, 3000, tall=0.3 if t < 2 else 0.0), centre(ref, 32, 0))
        before = check(G, g, ref, "frame %d" % t)
        a, b = scene(ref, rng, 2000), scene(ref, rng, 1000)
        g.add_points(a)
        ref.add(a)
        g.add_points_from(b, centre(ref, 3, 30, h=0.5))
        ref.add_from(b, centre(ref, 3, 30, h=0.5))
        got = check(G, g, ref, "frame %d, then adds" % t)
        assert all(np.array_equal(got[k], before[k]) for k in ("age", "contra", "through")) and got["dyn_stats"] == before["dyn_stats"]
        assert got["stats"]["added"] == before["stats"]["added"] + 3000
    assert ref.dyn_stats["aged"] > 0                                 # cells that only the adds filled have LAST 0: aged by stamp max_age + 1


# ---- device pointers, the view's lists ------------------------------------------------------------------------------------------------
def test_device_pointers_and_view_lists(G, hip):
    from svhip import view
    rng = np.random.default_rng(14)
    ref, g = pair(G, dict(min_through=1), nx=100, nz=60)
    lists = [scene(ref, rng, n, tall) for n, tall in ((3000, 0.4), (0, 0.0), (5000, 0.0), (700, 0.0))]
    v = view.View(64, 48)
    for a in lists:
        v.add_points([a])
    o = centre(ref, 50, 0)
    d = Dev(hip, lists[0])
    g.observe_points_device(d.addr, len(lists[0]), o)
    ref.observe(lists[0], o)
    check(G, g, ref, "device input")
    assert d.get(lists[0].nbytes).tobytes() == lists[0].tobytes()   # the input is only read
    g.observe_view_lists(v, 1, 1, o)                                 # an empty list is an observation too: the stamp moves
    ref.observe(lists[1], o)
    check(G, g, ref, "an empty list")
    g.observe_view_lists(v, 2, 2, o)
    ref.observe(np.concatenate(lists[2:]), o)
    got = check(G, g, ref, "lists 2..3")
    assert got["dyn_stats"]["observations"] == 3 and got["contra"].any()
    twin = G.Grid(g.params)                                          # the same points as host lists
    twin.set_dynamics(min_through=1)
    twin.observe_points(lists[0], o)
    twin.observe_points(lists[1], o)
    twin.observe_points(np.concatenate(lists[2:])[::-1], o)
    assert TL.same(snapshot(G, twin), snapshot(G, g))
    want = ref.dyn_planes()
    for k, name in ((G.DYN_AGE, "age"), (G.DYN_CONTRA, "contra"), (G.DYN_THROUGH, "through")):
        out = Dev(hip, want[name].nbytes + 16)
        g.dyn_plane(k, device_ptr=out.addr)
        got = out.get()
        assert got[:want[name].nbytes].tobytes() == want[name].tobytes() and (got[want[name].nbytes:] == 0xEE).all(), name
    out = Dev(hip, 100 * 60 * 3 + 16)
    g.render_dyn(device_ptr=out.addr)
    got = out.get()
    assert np.array_equal(got[:18000].reshape(60, 100, 3), ref.render_dyn()) and (got[18000:] == 0xEE).all()


# ---- refusals and failures --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_byte(G, hip):
    from svhip import view
    rng = np.random.default_rng(15)
    ref, g = pair(G, dict(min_through=1), nx=65, nz=33)
    g.scroll(-4, 6)
    ref.scroll(-4, 6)
    both(g, ref, scene(ref, rng, 5000), centre(ref, 30, 2))
    both(g, ref, scene(ref, rng, 5000, tall=0.0), centre(ref, 30, 2))
    before = check(G, g, ref, "before")
    L, pts = g._L, scene(ref, rng, 300)
    d = Dev(hip, pts)
    v = view.View(64, 48)
    v.add_points([pts[:100]])
    ok = np.array(centre(ref, 1, 1))
    buf = np.full(65 * 33 * 4, 0xAB, np.uint8)
    bad_origins = [centre(ref, -1, 5), centre(ref, 5, 33), centre(ref, 5, 5, h=2.5), [np.nan, 0, 1], [1, -2e6, 1]]
    for o in bad_origins:
        o = np.array(o, np.float64)
        assert L.svh_grid_observe_points(g._h, pts.ctypes.data, len(pts), 0, o.ctypes.data) == BAD_ARG, o
        assert L.svh_grid_observe_points(g._h, None, 0, 0, o.ctypes.data) == BAD_ARG, o
        assert L.svh_grid_observe_view_lists(g._h, v._h, 0, 1, o.ctypes.data) == BAD_ARG, o
    P = G.default_dyn
    calls = [lambda: L.svh_grid_observe_points(g._h, d.addr + 4, 10, 1, ok.ctypes.data),      # not 16-byte aligned
             lambda: L.svh_grid_observe_points(g._h, pts.ctypes.data, -1, 0, ok.ctypes.data),
             lambda: L.svh_grid_observe_points(g._h, None, 3, 0, ok.ctypes.data),
             lambda: L.svh_grid_observe_points(g._h, pts.ctypes.data, 3, 0, None),
             lambda: L.svh_grid_observe_view_lists(g._h, v._h, 0, 2, ok.ctypes.data),          # a range past the view's lists
             lambda: L.svh_grid_observe_view_lists(g._h, None, 0, 1, ok.ctypes.data),
             lambda: L.svh_grid_observe_view_lists(g._h, v._h, 0, 1, None),
             lambda: L.svh_grid_get_dyn(g._h, 3, buf.ctypes.data, 0), lambda: L.svh_grid_get_dyn(g._h, -1, buf.ctypes.data, 0),
             lambda: L.svh_grid_get_dyn(g._h, 0, None, 0), lambda: L.svh_grid_render_dyn(g._h, None, 0),
             lambda: L.svh_grid_get_dyn_stats(g._h, None), lambda: L.svh_grid_get_dynamics(g._h, None),
             lambda: L.svh_grid_set_dynamics(g._h, C.byref(P(clear_frames=-1))), lambda: L.svh_grid_set_dynamics(g._h, C.byref(P(clear_frames=65536))),
             lambda: L.svh_grid_set_dynamics(g._h, C.byref(P(min_through=0))), lambda: L.svh_grid_set_dynamics(g._h, C.byref(P(margin=-0.5))),
             lambda: L.svh_grid_set_dynamics(g._h, C.byref(P(margin=float("nan")))), lambda: L.svh_grid_set_dynamics(g._h, C.byref(P(margin=1048576.0))),
             lambda: L.svh_grid_set_dynamics(g._h, C.byref(P(max_age=-1)))]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG, k
        assert "svh_grid" in G.last_error()
    assert (buf == 0xAB).all() and g.dynamics().asdict() == dict(clear_frames=2, min_through=1, margin=F(0.1), max_age=0)
    assert TL.same(snapshot(G, g), before)
    # a grid without the layer refuses before it looks at anything else
    bare = G.Grid(g.params)
    assert L.svh_grid_observe_points(bare._h, pts.ctypes.data, len(pts), 0, ok.ctypes.data) == BAD_ARG and "svh_grid_set_dynamics" in G.last_error()
    assert L.svh_grid_observe_view_lists(bare._h, v._h, 0, 1, ok.ctypes.data) == BAD_ARG and bare.stats().asdict()["added"] == 0
    assert bare.dyn_stats() == dict.fromkeys(DR.STATS, 0)


@pytest.mark.parametrize("spec", ["copy:1", "launch:1", "launch:2", "launch:3", "wait:1", "malloc:1"])
def test_a_failed_observation_leaves_the_empty_grid(G, spec):
    """copy:1 is the upload of the points, launch:1 the frame record, launch:2 the sight lines, launch:3 the settle, wait:1 the one
    wait, malloc:1 the first buffer a fresh object needs: SVH_ERR_HIP names the call, the grid is empty where it stands, the layer
    stays set, and the same observation repeated is exact, with stamp 1"""
    rng = np.random.default_rng(16)
    ref, g = pair(G, dict(min_through=1), nx=65, nz=65)
    g.scroll(3, 3)
    ref.scroll(3, 3)
    a, b = scene(ref, rng, 4000), scene(ref, rng, 3000, tall=0.0)
    o = centre(ref, 7, 60)
    if spec != "malloc:1":
        both(g, ref, a, o)
        check(G, g, ref, "before")
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        g.observe_points(b, o)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR and "injected" in str(e.value)
    ref.clear()
    got = check(G, g, ref, spec + ": empty")
    assert got["window"] == (3, 3) and got["rays"] == (0, 0) and got["dyn_stats"]["observations"] == 0 and g.dynamics().min_through == 1
    both(g, ref, a, o)
    both(g, ref, b, o)
    got = check(G, g, ref, spec + ": the observations repeated")
    assert got["dyn_stats"]["observations"] == 2 and got["contra"].any()


def test_a_failed_scroll_and_a_failed_getter(G):
    """the layer's strips kernel is the scroll's second launch: the grid is empty at the new offsets; a getter that fails leaves
    everything as it was"""
    rng = np.random.default_rng(17)
    ref, g = pair(G, dict(min_through=1), nx=65, nz=65)
    both(g, ref, scene(ref, rng, 4000), centre(ref, 7, 60))
    before = check(G, g, ref, "before")
    for spec, call in (("launch:1", lambda: g.dyn_plane(G.DYN_AGE)), ("copy:1", lambda: g.dyn_plane(G.DYN_CONTRA)), ("launch:1", lambda: g.render_dyn())):
        G.lib().svh_test_fail_at(spec.encode())
        with pytest.raises(G.SvhError) as e:
            call()
        G.lib().svh_test_fail_at(None)
        assert e.value.code == HIP_ERR
        assert TL.same(snapshot(G, g), before), spec
    G.lib().svh_test_fail_at(b"launch:2")
    with pytest.raises(G.SvhError) as e:
        g.scroll(2, -1)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    ref.clear()
    ref.scroll(2, -1)
    check(G, g, ref, "a failed scroll: empty")
    both(g, ref, scene(ref, rng, 2000), centre(ref, 1, 1))
    check(G, g, ref, "the next observation")


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------------------
def test_pipeline_grid_dynamic(G, tmp_path, monkeypatch, capsys):
    """--grid-dynamic DIR on the two golden frames: per frame the window follows the camera, the newest list is observed from the
    camera centre, and the images and the statistics are the restatement's after the same steps"""
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
    d, e = str(tmp_path / "loc"), str(tmp_path / "dyn")
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-dynamic", e, "--grid-dynamic-params", "1,2,0.05,1",
                                      "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)])
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("dynamics: clear after 1 frames of 2 through-lines, margin 0.05 m, age 1: 2 observations") for l in out)
    assert sorted(os.listdir(e)) == ["dyn.jsonl"] + ["dyn_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(e, "dyn.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    ref = DR.Grid(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0), DR.DynParams(clear_frames=1, min_through=2, margin=0.05, max_age=1))
    k = 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre_ = p.H_total[:3, 3]
        ref.follow(centre_, 48, 80)
        ref.observe(p.view.points(p.view.count(view.LISTS) - 1), centre_)
        assert np.array_equal(read_ppm(os.path.join(e, "dyn_%06d.ppm" % k)), ref.render_dyn()), k
        assert np.array_equal(read_ppm(os.path.join(d, "local_%06d.ppm" % k)), ref.render_local()), k
        assert lines[k] == dict(ref.dyn_stats, frame=k), k
        k += 1
    assert k == 2 and ref.dyn_stats["confirmed"] > 100 and ref.rays > 1000
