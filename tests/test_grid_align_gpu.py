"""GPU: the alignment layer of the ground grid (include/svh_grid.h, "ALIGN"; csrc/grid_align_kernels.hip, csrc/grid_engine.cpp)
against the header's host form (core_align) and, on windows of at most 65 x 65 cells, the restatement tests/grid_align_ref.py, which
tests/test_grid_align.py pins on the CPU.  Every comparison is exact: the field, the scan, the counts, the volume, the record and
the image byte for byte.

Shapes: k_grid_align_mark runs one lane per point in workgroups of 256 and strides beyond 2048 * 256 points; the compaction counts
and scatters 256 words of the bitmap per workgroup; k_grid_align_score gives a workgroup one rotation, 256 translations and slices
of 1024 scan subs; k_grid_align_best is one workgroup of 1024 lanes; the row pass of the field has one workgroup per 256 cells of a
row and the column sweep chunks of 32 rows."""
import ctypes as C

import numpy as np
import pytest

import grid_align_ref as AR
import grid_ref as R
import test_grid_align as TA
import test_grid_local_gpu as TL
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2
O, FREE, U = TA.O, TA.FREE, TA.U
CELL = TL.CELL
RESTATE_CELLS = 65 * 65


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


def equal(tag, got, want):
    assert got.keys() == want.keys(), tag
    for k in got:
        if isinstance(got[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
            assert got[k].tobytes() == want[k].tobytes(), (tag, k, np.argwhere(got[k] != want[k])[:4], got[k].ravel()[:8], want[k].ravel()[:8])
        else:
            assert got[k] == want[k], (tag, k, got[k], want[k])


def run(G, state, cell=1.0, x0=0.0, z0=0.0, oa=0, ob=0, points=None, pivot=None, subs=None, pivot_sub=None, restate=True, tag="", **kw):
    """device_align against core_align, and core_align against the restatement on small windows; the device's dict"""
    state = np.ascontiguousarray(state, np.uint8)
    nz, nx = state.shape
    P = G.default_params(nx=nx, nz=nz, cell=cell, x0=x0, z0=z0, T=TA.LEVEL, step=0.2, clearance=2.0)
    args = (P, G.default_align(**kw), state, oa, ob, points, pivot, subs, pivot_sub)
    got, want = G.device_align(*args), G.core_align(*args)
    equal(tag, got, want)
    if restate and state.size <= RESTATE_CELLS:
        TA.both(G, state, cell, x0, z0, oa, ob, points, pivot, subs, pivot_sub, tag=tag + " (header against restatement)", **kw)
    return got


def at_subs(subs, cell, y=-1.0):
    """one point in the middle of each global sub, x0 = z0 = 0, an obstacle's height"""
    u = np.asarray(subs, np.float64).reshape(-1, 2)
    p = np.zeros((len(u), 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = (u[:, 0] + 0.5) * cell / 4, y, (u[:, 1] + 0.5) * cell / 4, 0.5
    return p


def wall_state(nx, nz, rng, p=0.15):
    state = rng.choice(np.array([FREE, O, U, U | 0x40, O | 0x80], np.uint8), (nz, nx), p=[1 - 2.5 * p, p, p / 2, p / 2, p / 2])
    return state


# ---- the scan: sizes on both sides of a wave, a workgroup, a chunk -----------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_scan_sizes(G, n):
    """n distinct subs, each from one to three points that lie 300 and more apart in the array: lanes of different workgroups mark
    the same bit"""
    rng = np.random.default_rng(1000 + n)
    state = wall_state(33, 17, rng)
    side = 8 * 16 + 1
    bits = np.sort(rng.choice(side * side, n, replace=False))
    subs = np.stack([bits % side - 64 + 66, bits // side - 64 + 34], axis=1)
    twice = subs[rng.random(n) < 0.5]
    pts = np.concatenate([at_subs(subs, 0.5), at_subs(np.full((300, 2), 4000), 0.5), at_subs(twice, 0.5, -1.5), at_subs(np.full((300, 2), -4000), 0.5),
                          at_subs(twice[::2], 0.5, -0.3)])
    got = run(G, state, 0.5, points=pts, pivot=(66.5 / 8, 0.0, 34.5 / 8), reach=1.0, range=8.0, rot_n=1, trans_n=1, min_scan=1, tag="n = %d" % n)
    assert len(got["scan"]) == n and got["n_points"] == n + len(twice) + len(twice[::2]) and (got["rec"][0] == AR.FEW) == (n == 0)


@pytest.mark.parametrize("n", [1, 256, 257, 2048 * 256 + 300])
def test_point_counts(G, n):
    rng = np.random.default_rng(1100 + n % 1000)
    state = wall_state(40, 40, rng)
    pts = np.stack([rng.uniform(-2, 22, n), rng.uniform(-2.2, 0.0, n), rng.uniform(-2, 22, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
    got = run(G, state, 0.5, points=pts, pivot=(10.1, 0.0, 9.9), reach=1.5, range=9.0, rot_n=1, trans_n=2, min_scan=1, restate=n <= 257, tag="points = %d" % n)
    assert n < 1000 or (got["n_points"] > 1000 and got["rec"][0] == AR.OK)


def test_subs_given_directly(G):
    rng = np.random.default_rng(12)
    state = wall_state(21, 30, rng)
    subs = rng.integers(-40, 160, (3000, 2)).astype(np.int32)
    run(G, state, oa=-3, ob=4, subs=subs, pivot_sub=(30, 70), reach=2.0, range=20.0, rot_den=64, rot_n=3, trans_n=4, min_scan=5, tag="subs")


# ---- the search window -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", [(0, 0), (0, 1), (1, 0), (2, 3), (8, 8), (32, 32)])
def test_search_windows(G, K, W):
    state, cells, subs = TA.recovery()
    if (K, W) == (32, 32):
        subs = subs[::5][:65]
        assert len(subs) == 65
    moved = AR.placed(AR.AlignParams(rot_den=64, rot_n=K), 65, 14, subs, -min(K, 2), min(W, 3), -min(W, 1))
    got = run(G, state, subs=moved, rot_n=K, trans_n=W, restate=K <= 8, tag="K, W = %d, %d" % (K, W), **TA.SCENE)
    assert got["volume"].shape == (2 * K + 1, 2 * W + 1, 2 * W + 1) and got["rec"][0] == AR.OK
    if (K, W) == (8, 8):
        assert got["rec"][1:4].tolist() == [2, -3, 1]


# ---- grids -----------------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1, 1, 1), (5, 5, 1, 2), (17, 33, 128, 2), (33, 17, 129, 1), (256, 256, 256, 32), (257, 9, 128, 32), (513, 40, 129, 3), (40, 70, 8, 32)]


@pytest.mark.parametrize("nx,nz,Rg,reach", GRIDS)
def test_grids(G, nx, nz, Rg, reach):
    """the pivot in each corner of the window: placed subs leave it on two sides; an obstacle in every corner"""
    rng = np.random.default_rng(nx * 1000 + nz)
    state = wall_state(nx, nz, rng, 0.05)
    state[0, 0] = state[0, -1] = state[-1, 0] = state[-1, -1] = O
    oa, ob = 11, -7
    for ca, cb in ((0, 0), (nx - 1, 0), (0, nz - 1), (nx - 1, nz - 1)):
        Pa, Pb = 4 * (oa + ca) + 1, 4 * (ob + cb) + 2
        n = 600
        spread = min(4 * Rg + 3, 4 * max(nx, nz) + 8)
        subs = np.stack([Pa + rng.integers(-spread, spread + 1, n), Pb + rng.integers(-spread, spread + 1, n)], 1).astype(np.int32)
        subs[:4] = [(Pa - 4 * Rg, Pb), (Pa + 4 * Rg, Pb + 4 * Rg), (Pa - 4 * Rg - 1, Pb), (Pa, Pb + 4 * Rg + 1)]
        got = run(G, state, oa=oa, ob=ob, subs=subs, pivot_sub=(Pa, Pb), reach=float(reach), range=float(Rg), rot_den=16, rot_n=2, trans_n=2, min_scan=1,
                  tag="%d x %d, corner (%d, %d)" % (nx, nz, ca, cb))
        assert got["n_points"] <= n - 2 and got["field"][cb, ca] == 255


# ---- ties that span the partitions of the reduction --------------------------------------------------------------------------
def test_ties_across_the_reduction(G):
    state = np.full((24, 40), FREE, np.uint8)
    state[10, :] = O
    subs = np.array([(u, 4 * 10 + j) for u in range(40, 120) for j in (1, 2)], np.int32)
    K, W = 2, 8                                         # 1445 candidates for 1024 lanes
    got = run(G, state, subs=subs + np.array((0, 3), np.int32), pivot_sub=(80, 42), reach=3.0, range=64.0, rot_den=4096, rot_n=K, trans_n=W, min_scan=1, tag="wall")
    assert got["rec"][2] == 0 and got["rec"][7] % (2 * W + 1) == 0 and got["rec"][7] >= 2 * W + 1
    flat = run(G, np.full((24, 40), FREE, np.uint8), subs=subs, pivot_sub=(80, 42), reach=3.0, range=64.0, rot_n=K, trans_n=W, min_scan=1, tag="flat")
    assert flat["rec"].tolist() == [AR.FLAT, 0, 0, 0, 0, 0, len(subs), 5 * 17 * 17]
    few = run(G, state, subs=subs[:9], pivot_sub=(80, 42), reach=3.0, range=64.0, rot_n=K, trans_n=W, min_scan=10, tag="few")
    assert few["rec"].tolist() == [AR.FEW, 0, 0, 0, 0, 0, 9, 0] and few["volume"] is None


# ---- the three forms of the score kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2, 4])
def test_every_form_of_the_score_kernel(G, form):
    """the chunk form (kept), the plain form (one lane per candidate) and the tiled form (F in LDS, translations a whole cell apart
    share their weights; the chunk form where the cells do not fit the LDS) give the same bytes; so does the field in three launches,
    the mask first (form 4), instead of two"""
    assert G.align_form(form) == 0
    try:
        for K, W in [(0, 0), (0, 1), (1, 0), (2, 3), (8, 8), (32, 32)]:
            test_search_windows(G, K, W)
        for shape in GRIDS:
            test_grids(G, *shape)
        test_ties_across_the_reduction(G)
        test_scan_sizes(G, 1025)
        test_point_counts(G, 2048 * 256 + 300)
        test_subs_given_directly(G)
    finally:
        assert G.align_form(0) == form


# ---- through the object ------------------------------------------------------------------------------------------------------
def build(G, nx, nz, seed):
    """a window of cells of 0.5 with two walls of obstacle cells, a lone one, free ground elsewhere; the restatement and the object"""
    ref, g = TL.pair(G, **TL.win_kw(nx, nz))
    rng = np.random.default_rng(seed)
    ia = np.concatenate([np.arange(4, nx - 6), np.full(nz // 2 - 6, 4), [nx - 5]])
    ib = np.concatenate([np.full(nx - 10, 6), np.arange(6, nz // 2), [nz - 4]])
    ja, jb = np.meshgrid(np.arange(nx), np.arange(nz))
    pts = np.concatenate([TL.at_cells(ref, ia, ib, 1.0)] * 2 + [TL.at_cells(ref, ja.ravel(), jb.ravel(), 0.0)] * 2)
    g.add_points(pts)
    ref.add(pts)
    return ref, g, rng, np.stack([ia, ib], 1)


def frame_of(ref, walls, shift=(0, 0), n_each=3, rng=None):
    """obstacle points in the subs of the wall cells, moved by `shift` subs, and ground points that are no scan points"""
    subs = np.array([(4 * (ref.oa + a) + i, 4 * (ref.ob + b) + j) for a, b in walls for i in range(4) for j in (0, 2)]) + np.array(shift)
    p = np.concatenate([at_subs(subs, CELL, -1.0 - 0.1 * k) for k in range(n_each)] + [at_subs(subs[::3], CELL, 0.0)])
    return p if rng is None else p[rng.permutation(len(p))]


def object_check(G, g, pts, pivot, tag, rec=None):
    rec = g.align_points(pts, pivot) if rec is None else rec
    oa, ob = g.window()
    want = G.core_align(g.params, g.align_params, g.local_plane(G.LOCAL_STATE), oa, ob, points=pts, pivot=pivot)
    assert rec.tobytes() == want["rec"].tobytes(), (tag, rec, want["rec"])
    assert g.align_field().tobytes() == want["field"].tobytes(), tag
    assert g.align_scan().tobytes() == want["scan"].tobytes(), tag
    if rec[0] != AR.FEW:
        assert g.align_volume().tobytes() == want["volume"].tobytes(), tag
    return want


def test_the_object_recovers_a_shift_after_scrolls(G):
    nx, nz = 65, 49
    ref, g, rng, walls = build(G, nx, nz, 5)
    g.set_align(reach=1.5, range=40.0, rot_den=256, rot_n=2, trans_n=6, min_scan=8)
    pivot = TL.centre(ref, 30, 2)
    want = object_check(G, g, frame_of(ref, walls, (-3, 5), rng=rng), pivot, "before any scroll")
    assert want["rec"][:4].tolist() == [AR.OK, 0, 3, -5]
    for da, db in ((3, 0), (0, -2), (-7, 0), (0, 5)):
        g.scroll(da, db)
        ref.scroll(da, db)
        walls = walls - (da, db)
        walls = walls[(walls[:, 0] >= 0) & (walls[:, 0] < nx) & (walls[:, 1] >= 0) & (walls[:, 1] < nz)]     # what the window still holds
        pts = frame_of(ref, walls, (2, -1), rng=rng)
        want = object_check(G, g, pts, TL.centre(ref, 30, 2), "after a scroll by (%d, %d)" % (da, db))
        assert want["rec"][0] == AR.OK and g.window() == ref.window()
    TL.check(G, g, ref, "the grid afterwards")


def test_an_alignment_changes_nothing_else(G):
    nx, nz = 65, 49
    ref, g, rng, walls = build(G, nx, nz, 6)
    g.set_traversability(inflate=1.5)
    g.set_goal(TL.centre(ref, 40, 30))
    g.set_align(reach=1.0, range=30.0, rot_n=1, trans_n=2, min_scan=4)
    others = lambda: dict(trav=g.trav_plane(G.TRAV_COST), dist=g.trav_plane(G.TRAV_DIST2), pot=g.plan_plane(G.PLAN_POT), front=g.front_plane(G.FRONT_FLAGS),
                          frontiers=g.frontiers(), roll=g.roll_params()[1:], explore=g.explore_stats(), plan=g.plan_stats())
    before, more = TL.snapshot(G, g), others()
    pivot = TL.centre(ref, 30, 2)
    for pts in (frame_of(ref, walls, (1, 1)), frame_of(ref, walls[:1])[:2], np.zeros((0, 4), np.float32)):
        object_check(G, g, pts, pivot, "%d points" % len(pts))
        g.render_align()
    assert TL.same(TL.snapshot(G, g), before)
    after = others()
    for k in more:
        assert (more[k].tobytes() == after[k].tobytes()) if isinstance(more[k], np.ndarray) else more[k] == after[k], k
    TL.check(G, g, ref, "the grid afterwards")


def test_the_field_is_cached_until_something_changes(G):
    ref, g, rng, walls = build(G, 40, 40, 7)
    g.set_align(reach=1.0, range=20.0, rot_n=1, trans_n=1, min_scan=1)
    pts, pivot = frame_of(ref, walls), TL.centre(ref, 20, 2)
    object_check(G, g, pts, pivot, "first")
    vol = g.align_volume()
    for change in (lambda: None, lambda: g.scroll(1, 0), lambda: g.add_points(np.concatenate([TL.at_cells(ref, [20], [20], 1.0)] * 2)),
                   lambda: g.set_align(reach=2.0, range=20.0, rot_n=1, trans_n=1, min_scan=1), lambda: g.clear()):
        change()
        object_check(G, g, pts, pivot, "after a change")
    assert g.align_volume().shape == vol.shape


def test_the_image(G):
    nx, nz = 40, 33
    ref, g, rng, walls = build(G, nx, nz, 8)
    g.set_align(reach=1.5, range=30.0, rot_den=64, rot_n=3, trans_n=5, min_scan=4)
    pivot = TL.centre(ref, 20, 2)
    A = AR.AlignParams(rot_den=64, rot_n=3)
    Pa, Pb = AR.pivot_sub(ref.P, pivot)
    for pts in (frame_of(ref, walls, (4, -3)), frame_of(ref, walls[:1])[:1], np.concatenate([frame_of(ref, walls, (2, 2)), at_subs([(-9, 5), (4 * nx + 3, 9)], CELL)])):
        rec = g.align_points(pts, pivot)
        scan = g.align_scan()
        want = AR.overlay(ref.render_local(), 0, 0, Pa, Pb, scan, AR.placed(A, Pa, Pb, scan, *rec[1:4]))
        assert g.render_align().tobytes() == want.tobytes(), len(pts)
    assert tuple(want[nz - 1 - 2, 20]) == AR.PIVOT_COLOUR and (want == AR.BEST_COLOUR).all(axis=2).sum() > 10


@pytest.mark.parametrize("spec", [b"malloc:1", b"malloc:3", b"malloc:9", b"copy:1", b"copy:2", b"copy:3", b"copy:4", b"copy:5", b"launch:1", b"launch:2", b"launch:3",
                                  b"wait:1"])
def test_a_failed_alignment_leaves_the_grid(G, spec):
    """the host-side hook at each guarded call of an alignment of host points with a stale field -- its three launch checks (the
    field; the marks; compaction + scores + best: the finished planes are valid again once the snapshot below has read them); the
    three fills, the points' upload, the record's copy; the wait; and, in a grid that has not aligned yet, the first, the third and
    the ninth allocation: SVH_ERR_HIP, the grid untouched, the next call correct"""
    ref, g, rng, walls = build(G, 40, 33, 9)
    g.set_align(reach=1.0, range=20.0, rot_n=1, trans_n=2, min_scan=1)
    pts, pivot = frame_of(ref, walls, (1, -2)), TL.centre(ref, 20, 2)
    if not spec.startswith(b"malloc"):
        object_check(G, g, pts, pivot, "before")
        g.add_points(np.concatenate([TL.at_cells(ref, [20], [20], 1.0)] * 2))          # the field is stale: an alignment launches the finished planes and the field
        ref.add(np.concatenate([TL.at_cells(ref, [20], [20], 1.0)] * 2))
    before = TL.snapshot(G, g)
    G.lib().svh_test_fail_at(spec)
    with pytest.raises(G.SvhError) as e:
        g.align_points(pts, pivot)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    for f in (g.align_volume, g.align_scan, g.render_align):
        with pytest.raises(G.SvhError) as e:
            f()
        assert e.value.code == BAD_ARG
    assert TL.same(TL.snapshot(G, g), before)
    object_check(G, g, pts, pivot, "the call repeated")
    TL.check(G, g, ref, "the grid afterwards")


def test_device_pointers_and_the_view_lists(G, hip):
    from svhip import view
    ref, g, rng, walls = build(G, 50, 40, 10)
    g.set_align(reach=1.0, range=25.0, rot_n=2, trans_n=3, min_scan=1)
    pivot = TL.centre(ref, 25, 2)
    lists = [frame_of(ref, walls, (1, 2), rng=rng), np.zeros((0, 4), np.float32), frame_of(ref, walls[::2], (-2, 0), rng=rng), TL.cloud(ref, rng, 900)]
    d = Dev(hip, lists[0])
    want = object_check(G, g, lists[0], pivot, "device input", rec=g.align_points_device(d.addr, len(lists[0]), pivot))
    assert d.get(lists[0].nbytes).tobytes() == lists[0].tobytes()                       # the input is only read
    for get, arr in ((g.align_field, want["field"]), (g.align_volume, want["volume"]), (g.render_align, g.render_align())):
        out = Dev(hip, arr.nbytes + 16)
        get(device_ptr=out.addr)
        got = out.get()
        assert got[:arr.nbytes].tobytes() == arr.tobytes() and (got[arr.nbytes:] == 0xEE).all()
    v = view.View(64, 48)
    for a in lists:
        v.add_points([a])
    for first, n in ((3, 1), (1, 1), (0, 3), (2, 2)):
        object_check(G, g, np.concatenate(lists[first:first + n]), pivot, "lists %d..%d" % (first, first + n - 1), rec=g.align_view_lists(v, first, n, pivot))
    with pytest.raises(G.SvhError) as e:
        g.align_view_lists(v, 3, 2, pivot)
    assert e.value.code == BAD_ARG
    TL.check(G, g, ref, "the grid afterwards")


def test_the_correction_through_the_object(G):
    ref, g = TL.pair(G, **TL.win_kw(9, 9, T=R.frame_camera(1.65)))
    g.set_align(reach=1.0, range=4.0, rot_den=256, rot_n=8, trans_n=8, min_scan=1)
    A = AR.AlignParams(rot_den=256, rot_n=8, trans_n=8)
    pivot = (3.7, 1.1, -12.9)
    for cand in ((0, 0, 0), (0, 3, -5), (5, 2, 7), (-8, -8, 8)):
        assert g.align_correction(*cand, pivot).tobytes() == AR.correction(ref.P, A, *cand, pivot).tobytes(), cand
    assert g.align_correction(0, 4, -8, pivot).tolist() == [[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, -1.0], [0, 0, 0, 1]]
    for cand in ((9, 0, 0), (0, -9, 0), (0, 0, 9)):
        with pytest.raises(G.SvhError) as e:
            g.align_correction(*cand, pivot)
        assert e.value.code == BAD_ARG


def test_refusals_leave_every_byte(G, hip):
    ref, g, rng, walls = build(G, 40, 33, 11)
    L = g._L
    pts, pivot = frame_of(ref, walls), np.array(TL.centre(ref, 20, 2), np.float64)
    buf, rec = np.full(40 * 33 * 3, 0xAB, np.uint8), np.full(8, 0x55, np.int32)
    n = C.c_int64(-7)
    M = np.full(16, -7.0)
    entries = (lambda: L.svh_grid_get_align_field(g._h, buf.ctypes.data, 0), lambda: L.svh_grid_align_points(g._h, pts.ctypes.data, len(pts), 0, pivot.ctypes.data, rec.ctypes.data),
               lambda: L.svh_grid_get_align_volume(g._h, buf.ctypes.data, 0), lambda: L.svh_grid_get_align_scan(g._h, buf.ctypes.data, 4, C.addressof(n)),
               lambda: L.svh_grid_align_correction(g._h, 0, 0, 0, pivot.ctypes.data, M.ctypes.data), lambda: L.svh_grid_render_align(g._h, buf.ctypes.data, 0))
    before = TL.snapshot(G, g)
    for f in entries:                                                                   # no align parameters yet
        assert f() == BAD_ARG and "svh_grid_set_align" in G.last_error()
    for kw in TA.BAD:
        if "reach" in kw or "range" in kw:
            kw = {k: v * CELL for k, v in kw.items()}
        p = G.default_align(**dict(dict(reach=1.0, range=5.0), **kw))
        assert L.svh_grid_set_align(g._h, C.byref(p)) == BAD_ARG and "svh_grid_set_align" in G.last_error(), kw
    for f in entries:
        assert f() == BAD_ARG
    g.set_align(reach=1.0, range=20.0, rot_n=1, trans_n=1, min_scan=10 ** 6)
    for f in entries[2:4] + entries[5:]:                                                # nothing aligned yet
        assert f() == BAD_ARG
    nan = np.array([np.nan, 0, 0], np.float64)
    far = np.array([2.0 ** 21, 0, 0], np.float64)
    dev = Dev(hip, 64)
    for bad in (lambda: L.svh_grid_align_points(g._h, pts.ctypes.data, len(pts), 0, nan.ctypes.data, rec.ctypes.data),
                lambda: L.svh_grid_align_points(g._h, pts.ctypes.data, len(pts), 0, far.ctypes.data, rec.ctypes.data),
                lambda: L.svh_grid_align_points(g._h, pts.ctypes.data, len(pts), 0, None, rec.ctypes.data),
                lambda: L.svh_grid_align_points(g._h, None, 5, 0, pivot.ctypes.data, rec.ctypes.data),
                lambda: L.svh_grid_align_points(g._h, pts.ctypes.data, -1, 0, pivot.ctypes.data, rec.ctypes.data),
                lambda: L.svh_grid_align_points(g._h, pts.ctypes.data, len(pts), 0, pivot.ctypes.data, None),
                lambda: L.svh_grid_align_points(g._h, dev.addr + 4, 1, 1, pivot.ctypes.data, rec.ctypes.data),
                lambda: L.svh_grid_get_align_field(g._h, None, 0), lambda: L.svh_grid_align_correction(g._h, 0, 0, 0, nan.ctypes.data, M.ctypes.data)):
        assert bad() == BAD_ARG
    assert (rec == 0x55).all() and (buf == 0xAB).all() and n.value == -7 and (M == -7.0).all()
    got = g.align_points(pts, pivot)                                                    # too few subs: a scan, no volume
    assert got[0] == AR.FEW and got[6] == len(g.align_scan()) > 0
    with pytest.raises(G.SvhError) as e:
        g.align_volume()
    assert e.value.code == BAD_ARG
    g.render_align()
    assert TL.same(TL.snapshot(G, g), before)
    TL.check(G, g, ref, "the grid afterwards")


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------------------
def test_pipeline_grid_align(G, tmp_path, monkeypatch, capsys):
    """--grid-align DIR on the two golden frames: before a frame's list is added it is aligned from the camera's position; the record
    and the image are those of the header on the grid as it stood.  With --grid-align-apply the run completes and says what it did"""
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
    d, a = str(tmp_path / "loc"), str(tmp_path / "align")
    size = ["--grid-cell", "0.25", "--grid-size", "96x160"]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-align", a, "--grid-align-window", "2,3"] + size + [drive, str(calib)])
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("alignment: 5 rotations x 7 x 7 translations per frame") for l in out)
    assert sorted(os.listdir(a)) == ["align.jsonl"] + ["align_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(a, "align.jsonl"))]
    c = kitti.read_cam_to_cam(str(calib))
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    p.enable_grid_local(0.25, (96, 160))
    p.enable_grid_align(False, (2, 3))
    g, k = p.local, 0
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
        centre = p.H_total[:3, 3].copy()
        g.follow(centre, 48, 80)
        pts = p.view.points(p.view.count(view.LISTS) - 1)
        oa, ob = g.window()
        want = G.core_align(g.params, g.align_params, g.local_plane(G.LOCAL_STATE), oa, ob, points=pts, pivot=centre)
        assert [lines[k][f] for f in G.ALIGN_FIELDS] == want["rec"].tolist() and lines[k]["frame"] == k and lines[k]["applied"] is False, k
        Pa, Pb = AR.pivot_sub(R.Params(nx=96, nz=160, cell=0.25, x0=-12.0, z0=0.0), centre)
        img = AR.overlay(g.render_local(), oa, ob, Pa, Pb, want["scan"], AR.placed(AR.AlignParams(rot_n=2), Pa, Pb, want["scan"], *want["rec"][1:4]))
        assert np.array_equal(read_ppm(os.path.join(a, "align_%06d.ppm" % k)), img), k
        g.add_view_lists_from(p.view, p.view.count(view.LISTS) - 1, 1, centre)
        k += 1
    assert k == 2 and lines[0]["status"] == AR.FLAT and lines[0]["n_scan"] > 100 and lines[1]["status"] == AR.OK and lines[1]["score"] > 0
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-align", a, "--grid-align-apply"] + size + [drive, str(calib)])
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any("applied to the local grid" in l for l in out)
    lines = [json.loads(l) for l in open(os.path.join(a, "align.jsonl"))]
    assert len(lines) == 2 and lines[0]["applied"] is False and lines[1]["applied"] == (lines[1]["status"] == 0 and lines[1]["ties"] == 1 and any(lines[1][f] for f in ("k", "ta", "tb")))
