"""CPU: the contract of the ground grid's traversability layer (include/svh_grid.h: svh_grid_set_traversability,
svh_grid_get_trav, svh_grid_render_cost).  tests/grid_trav_ref.py restates that part of stereo-vision_amd/csrc/grid_core.h
in numpy, with DIST2 as a brute-force minimum; this file pins the restatement with cases derived by hand, compares the
header itself with it -- evaluated on the host by the library's test entries svh_test_grid_trav / svh_test_grid_cost_table,
and once more as a program of its own under the undefined-behaviour sanitizer --, and checks what needs no device: the
thresholds to the float, the refusals, the exports.

tests/test_grid_trav_gpu.py compares the device with the same restatement.

The hand cases use cells of 0.5: max_slope 0.25 gives rise4 = 0.125 and rise8 = 0.125 * 1.41421354f = 0.17677669, max_slope
0.35 gives rise4 = 0.175; a kerb of 0.15 lies between them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_local_ref as LR
import grid_ref as R
import grid_trav_ref as TR
import helpers as H

F = np.float32
NAN = F(np.nan)
U, FR, OB, DR = R.UNKNOWN, R.FREE, R.OBSTACLE, R.DROP
SEEN = LR.SEEN


@pytest.fixture(scope="module")
def G():
    from svhip import grid
    grid._bind()
    return grid


def both(G, nx, nz, cell=0.5, **tkw):
    """(restatement's TravParams, library's Params of an nx x nz window, library's TravParams)"""
    return TR.TravParams(**tkw), G.default_params(nx=nx, nz=nz, cell=cell), G.default_trav(**tkw)


def header(G, P, Tc, cls, hmean, state):
    fl, d2, c, rgb = G.core_trav(P, Tc, cls, hmean, state)
    return dict(flags=fl, dist2=d2, cost=c, rgb=rgb)


def agree(G, nx, nz, cls, hmean, state, cell=0.5, tag="", **tkw):
    """the restatement and the header on the same planes: every plane bit for bit; returns the planes"""
    T, P, Tc = both(G, nx, nz, cell, **tkw)
    cls, state = np.asarray(cls, np.uint8).reshape(nz, nx), np.asarray(state, np.uint8).reshape(nz, nx)
    hmean = np.asarray(hmean, F).reshape(nz, nx)
    want, got = TR.layer(T, cell, cls, hmean, state), header(G, P, Tc, cls, hmean, state)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (tag, k)
        assert np.array_equal(got[k], w), (tag, k, np.argwhere(got[k] != w)[:4])
    return want


# ---- by hand -------------------------------------------------------------------------------------------------------------
def test_a_kerb_across_one_edge(G):
    """3 x 3, all free, column 0 at height 0 and columns 1 and 2 at 0.15.  Against max_slope 0.25 the edge pairs differ by
    0.15 > 0.125: columns 0 and 1 are steep, column 2 is not (its neighbours are level; the corner pairs across the kerb,
    0.15 < 0.1768, would not have made anything steep).  Against 0.35, 0.15 < 0.175: nothing is steep."""
    cls = np.full((3, 3), FR, np.uint8)
    h = np.tile(np.array([0.0, 0.15, 0.15], F), (3, 1))
    got = agree(G, 3, 3, cls, h, cls, max_slope=0.25, inflate=1.0)
    assert np.array_equal(got["flags"], np.tile(np.array([3, 3, 0], np.uint8), (3, 1)))     # steep is lethal by default
    assert np.array_equal(got["dist2"], np.tile(np.array([0, 0, 1], np.int32), (3, 1)))
    got = agree(G, 3, 3, cls, h, cls, max_slope=0.35, inflate=1.0)
    assert not got["flags"].any() and (got["dist2"] == TR.FAR).all() and not got["cost"].any()


def test_a_pair_that_is_steep_across_an_edge_but_not_across_a_corner(G):
    """two free cells 0.15 apart in height among unknown ones, max_slope 0.25: side by side 0.15 > 0.125, corner to corner
    0.15 < 0.1768"""
    for (a, b), steep in ((((1, 1), (1, 2)), True), (((1, 1), (2, 1)), True), (((1, 1), (2, 2)), False), (((1, 1), (0, 2)), False)):
        cls, h = np.zeros((3, 3), np.uint8), np.full((3, 3), NAN, F)
        cls[a], cls[b], h[a], h[b] = FR, FR, 0.0, -0.15
        got = agree(G, 3, 3, cls, h, cls, max_slope=0.25, inflate=1.0)
        want = np.zeros((3, 3), np.uint8)
        if steep:
            want[a] = want[b] = 3
        assert np.array_equal(got["flags"], want), (a, b)


def test_an_obstacle_does_not_make_its_neighbour_steep(G):
    """the obstacle's HMEAN is a metre above the free cells: only free-free pairs are tested"""
    cls = np.array([[FR, OB, FR], [FR, FR, FR], [DR, FR, U]], np.uint8)
    h = np.array([[0, 1.0, 0], [0, 0, 0], [-1.0, 0, 0.9]], F)
    got = agree(G, 3, 3, cls, h, cls, max_slope=0.25, inflate=1.0)
    assert np.array_equal(got["flags"], np.array([[0, 2, 0], [0, 0, 0], [2, 0, 0]], np.uint8))


def test_the_costs_around_an_obstacle_and_a_drop(G):
    """the same window, cell 0.5, inscribed 0.4, inflate 1.0 (reach 2): a neighbour across an edge is 0.5 away, costs
    1 + floor(251 * 0.5 / 0.6) = 210; across a corner 0.7071 away, 1 + floor(251 * 0.29289 / 0.6) = 123; two cells away
    1.0 == inflate: 0.  The unknown cell (2, 2) is sqrt(5) cells from the obstacle and 2 from the drop: 0 from the table,
    so it says 255"""
    cls = np.array([[FR, OB, FR], [FR, FR, FR], [DR, FR, U]], np.uint8)
    h = np.array([[0, 1.0, 0], [0, 0, 0], [-1.0, 0, 0.9]], F)
    got = agree(G, 3, 3, cls, h, cls, max_slope=0.25, inflate=1.0)
    assert np.array_equal(got["dist2"], np.array([[1, 0, 1], [1, 1, 2], [0, 1, 4]], np.int32))
    assert np.array_equal(got["cost"], np.array([[210, 254, 210], [210, 210, 123], [254, 210, 255]], np.uint8))
    assert tuple(got["rgb"][0, 0]) == (210, 0, 45) and tuple(got["rgb"][0, 1]) == (255, 0, 0) and tuple(got["rgb"][2, 2]) == (32, 32, 32)


def test_dist2_of_a_single_lethal_corner(G):
    """cell (0, 0) is an obstacle in a free, level 7 x 5 window, reach 3: ia^2 + ib^2 where that is at most 9"""
    cls = np.full((5, 7), FR, np.uint8)
    cls[0, 0] = OB
    got = agree(G, 7, 5, cls, np.zeros((5, 7), F), cls, inflate=1.5)
    ia, ib = np.meshgrid(np.arange(7), np.arange(5))
    d = ia * ia + ib * ib
    assert np.array_equal(got["dist2"], np.where(d <= 9, d, TR.FAR))
    assert got["dist2"][0, 3] == 9 and got["dist2"][2, 2] == 8 and got["dist2"][1, 3] == TR.FAR and got["cost"][0, 3] == 0


def test_the_default_cost_table(G):
    T, t = TR.TravParams(), G.default_trav()
    assert (t.max_slope, t.inscribed, t.inflate, t.lethal) == (F(0.35), F(0.4), F(1.5), 7)
    want = TR.cost_table(T, 0.2)
    got = G.core_cost_table(0.2, t)
    assert TR.reach_of(T, 0.2) == 8 and len(got) == 65 and got.dtype == np.uint8 and np.array_equal(got, want)
    assert list(got[:8]) == [254, 253, 253, 253, 253, 241, 231, 222]
    assert (np.diff(got.astype(int)) <= 0).all() and got[56] == 1 and got[57] == 0     # sqrt(56) * 0.2 = 1.4967 < 1.5 <= sqrt(57) * 0.2


def test_the_colours(G):
    cost = np.array([254, 253, 252, 1, 100, 0, 255, 254, 0, 17], np.uint8)
    fl = np.array([2, 0, 0, 0, 0, 0, 0, 3, 1, 1], np.uint8)
    want = [(255, 0, 0), (255, 128, 0), (252, 0, 3), (1, 0, 254), (100, 0, 155), (0, 96, 0), (32, 32, 32), (255, 255, 0), (0, 255, 0),
            (17, 255, 238)]
    assert [tuple(c) for c in TR.colours(cost, fl)] == want


# ---- thresholds, to the float --------------------------------------------------------------------------------------------
def test_a_difference_of_exactly_the_rise_is_not_steep(G):
    up = np.nextafter(F(0.125), F(1))
    for hb, diag, steep in ((F(0.125), False, False), (up, False, True), (F(-0.125), False, False), (-up, False, True),
                            (F(0.125) * TR.SQRT2, True, False), (np.nextafter(F(0.125) * TR.SQRT2, F(1)), True, True)):
        cls, h = np.zeros((2, 2), np.uint8), np.full((2, 2), NAN, F)
        b = (1, 1) if diag else (0, 1)
        cls[0, 0], cls[b], h[0, 0], h[b] = FR, FR, 0.0, hb
        got = agree(G, 2, 2, cls, h, cls, max_slope=0.25, inflate=1.0)
        assert bool(got["flags"][0, 0] & 1) == steep and bool(got["flags"][b] & 1) == steep, (hb, diag)
    assert TR.rises(TR.TravParams(max_slope=0.25), 0.5) == (F(0.125), F(0.17677669))


def test_the_table_at_the_inscribed_and_the_inflation_radius(G):
    """cell 0.5, inscribed 1.0, inflate 1.5: reach 3; d2 = 4 is exactly 1.0 -> 253, d2 = 9 is exactly 1.5 -> 0"""
    kw = dict(inscribed=1.0, inflate=1.5)
    got = G.core_cost_table(0.5, G.default_trav(**kw))
    assert np.array_equal(got, TR.cost_table(TR.TravParams(**kw), 0.5)) and len(got) == 10
    assert list(got) == [254, 253, 253, 253, 253, 1 + int(251 * (1.5 - 5 ** 0.5 / 2) / 0.5), 1 + int(251 * (1.5 - 6 ** 0.5 / 2) / 0.5),
                         1 + int(251 * (1.5 - 7 ** 0.5 / 2) / 0.5), 1 + int(251 * (1.5 - 2 ** 0.5) / 0.5), 0]
    just = np.nextafter(F(1.0), F(0))
    assert G.core_cost_table(0.5, G.default_trav(inscribed=just, inflate=1.5))[4] == 251     # d just beyond the inscribed radius:
    # 1 + floor(251 * 0.5 / 0.50000006) = 1 + floor(250.99997)
    assert G.core_cost_table(0.5, G.default_trav(inscribed=1.0, inflate=np.nextafter(F(1.5), F(2))))[9] == 1   # d just inside the inflation


TABLE_CASES = [(0.2, {}), (0.5, {}), (1.0, dict(inscribed=0.0, inflate=256.0)), (1.0, dict(inscribed=255.5, inflate=256.0)),
               (0.05, dict(inflate=12.0)), (7.0, {}), (1e30, dict(inscribed=1e30, inflate=2.5e32)),
               (1e-38, dict(inscribed=0.0, inflate=2.5e-36)), (0.3, dict(inscribed=1.0, inflate=np.nextafter(F(1.0), F(2)))),
               (3e38, dict(inscribed=0.0, inflate=3.4e38))]


@pytest.mark.parametrize("k", range(len(TABLE_CASES)))
def test_cost_tables_against_the_restatement(G, k):
    cell, kw = TABLE_CASES[k]
    T = TR.TravParams(**kw)
    got, want = G.core_cost_table(cell, G.default_trav(**kw)), TR.cost_table(T, cell)
    assert len(got) == TR.reach_of(T, cell) ** 2 + 1 and np.array_equal(got, want)
    assert got[0] == 254 and got[1:].max() <= 253 and (np.diff(got.astype(int)) <= 0).all()


# ---- random planes -------------------------------------------------------------------------------------------------------
def random_planes(rng, nx, nz, p_lethal=0.2, quant=None):
    """CLASS with the overhang bit, STATE with the seen bit, HMEAN NaN where nothing was counted"""
    p_free = 1.0 - p_lethal
    c = rng.choice(np.array([U, FR, OB, DR], np.uint8), (nz, nx), p=[p_free * 0.25, p_free * 0.75, p_lethal * 0.6, p_lethal * 0.4])
    cls = (c | np.where(rng.random((nz, nx)) < 0.1, R.OVERHANG, 0)).astype(np.uint8)
    state = (cls | np.where(rng.random((nz, nx)) < 0.5, SEEN, 0)).astype(np.uint8)
    h = rng.uniform(-0.2, 0.2, (nz, nx)).astype(F)
    if quant:
        h = (np.rint(h / F(quant)) * F(quant)).astype(F)
    h[(c == U) & (rng.random((nz, nx)) < 0.7)] = NAN
    return cls, h, state


WINDOWS = [(1, 1), (1, 9), (9, 1), (3, 3), (40, 7), (65, 33)]


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_the_header_against_the_restatement_on_random_planes(G, nx, nz):
    rng = np.random.default_rng(100 * nx + nz)
    for k, (cell, kw, p) in enumerate([(0.5, dict(max_slope=0.25), 0.05), (0.2, {}, 0.0), (0.5, dict(inflate=0.4, inscribed=0.1), 0.3),
                                       (0.125, dict(max_slope=1.0, inflate=8.0, lethal=TR.L_ALL), 0.02),
                                       (1.0, dict(inflate=256.0, lethal=TR.L_OBSTACLE), 0.02),
                                       (0.5, dict(max_slope=1e-3, lethal=TR.L_STEEP | TR.L_UNKNOWN_SEEN), 0.1)]):
        cls, h, state = random_planes(rng, nx, nz, p, quant=0.125 if k == 0 else None)
        got = agree(G, nx, nz, cls, h, state, cell=cell, tag="case %d" % k, **kw)
        reach = TR.reach_of(TR.TravParams(**kw), cell)
        sep, g = TR.separable((got["flags"] & 2) != 0, reach)
        assert np.array_equal(sep, got["dist2"]) and g.max() <= reach + 1


def test_brute_force_and_separable_agree():
    """the form of the header against the minimum over all lethal cells, windows 1 x 1 to 40 x 7"""
    rng = np.random.default_rng(7)
    for nx, nz in ((1, 1), (2, 1), (1, 5), (7, 7), (40, 7), (7, 40)):
        for reach in (1, 2, 5, 64):
            for p in (0.0, 0.02, 0.3, 1.0):
                lethal = rng.random((nz, nx)) < p
                assert np.array_equal(TR.separable(lethal, reach)[0], TR.dist2(lethal, reach)), (nx, nz, reach, p)


# ---- the lethal mask -----------------------------------------------------------------------------------------------------
def test_every_mask_bit_on_its_own(G):
    """a row of: obstacle, drop, a steep pair, unknown and not seen, unknown and seen, free -- far enough apart (unknown
    cells between them) that nothing else is steep"""
    cls = np.array([[OB, U, DR, U, FR, FR, U, U, U, FR]], np.uint8)
    state = cls.copy()
    state[0, [1, 3, 8]] |= SEEN
    h = np.array([[1.0, NAN, -1.0, NAN, 0.0, 0.5, 0.0, NAN, 0.3, 0.0]], F)
    kinds = {TR.L_OBSTACLE: [0], TR.L_DROP: [2], TR.L_STEEP: [4, 5], TR.L_UNSEEN: [6, 7], TR.L_UNKNOWN_SEEN: [1, 3, 8]}
    for bit, cells in kinds.items():
        got = agree(G, 10, 1, cls, h, state, lethal=bit, tag="bit %d" % bit)
        assert list(np.nonzero(got["flags"][0] & 2)[0]) == cells, bit
        assert list(np.nonzero(got["flags"][0] & 1)[0]) == [4, 5]                    # steep is steep whatever is lethal
        assert (got["cost"][0, cells] == 254).all()
    got = agree(G, 10, 1, cls, h, state, lethal=0)
    assert not (got["flags"] & 2).any() and (got["dist2"] == TR.FAR).all()
    assert list(got["cost"][0]) == [0, 255, 0, 255, 0, 0, 255, 255, 255, 0]             # nothing lethal: free 0, unknown 255
    got = agree(G, 10, 1, cls, h, state, lethal=TR.L_ALL)
    assert list(np.nonzero(got["flags"][0] & 2)[0]) == list(range(9))


# ---- refusals and exports ----------------------------------------------------------------------------------------------------
BAD = [dict(max_slope=0.0), dict(max_slope=-1.0), dict(max_slope=float("nan")), dict(max_slope=float("inf")), dict(inscribed=-0.1),
       dict(inscribed=float("nan")), dict(inscribed=float("inf")), dict(inflate=float("inf")), dict(inflate=float("nan")),
       dict(inflate=0.4), dict(inflate=0.3), dict(inscribed=0.0, inflate=0.0),       # a reach of 0 cells
       dict(lethal=32), dict(lethal=0x80000000), dict(lethal=7 | 64)]


def test_refusals(G):
    import svhip
    L = G._bind()
    reach, buf = C.c_int32(-7), np.full(64, 0xAB, np.uint8)
    P = G.default_params(nx=2, nz=2, cell=0.5)
    z, zf = np.zeros(4, np.uint8), np.zeros(4, F)
    for kw in BAD:
        t = G.default_trav(**kw)
        assert TR.reach_of(TR.TravParams(**kw), 0.5) is None, kw
        assert L.svh_test_grid_cost_table(0.5, C.byref(t), C.addressof(reach), buf.ctypes.data, 64) == svhip.ERR_BAD_ARG, kw
        assert "svh_test_grid_cost_table" in svhip.last_error()
        assert L.svh_test_grid_trav(C.byref(P), C.byref(t), z.ctypes.data, zf.ctypes.data, z.ctypes.data, buf.ctypes.data, None, None,
                                    None) == svhip.ERR_BAD_ARG, kw
    # the reach: 256 cells are allowed, 257 are not
    for cell, inflate, want in ((1.0, 256.0, 256), (1.0, 256.5, None), (1.0, np.nextafter(F(256.0), F(300)), None), (0.5, 128.0, 256),
                                (0.005, 1.5, None), (0.2, 1.5, 8), (7.0, 1.5, 1), (1e-30, 1.5, None), (3e38, 1e-30, 1)):
        t = G.default_trav(inflate=inflate, inscribed=0.0)
        assert TR.reach_of(TR.TravParams(inflate=inflate, inscribed=0.0), cell) == want
        rc = L.svh_test_grid_cost_table(cell, C.byref(t), C.addressof(reach), None, 0)
        assert (rc, reach.value) == ((0, want) if want else (svhip.ERR_BAD_ARG, reach.value)), (cell, inflate)
    good = G.default_trav()
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert L.svh_test_grid_cost_table(cell, C.byref(good), C.addressof(reach), None, 0) == svhip.ERR_BAD_ARG
    assert L.svh_test_grid_cost_table(0.5, None, C.addressof(reach), None, 0) == svhip.ERR_BAD_ARG
    assert L.svh_test_grid_cost_table(0.5, C.byref(good), None, None, 0) == svhip.ERR_BAD_ARG
    assert L.svh_test_grid_cost_table(0.5, C.byref(good), C.addressof(reach), None, 3) == svhip.ERR_BAD_ARG
    assert L.svh_test_grid_trav(C.byref(P), C.byref(good), None, zf.ctypes.data, z.ctypes.data, None, None, None, None) == svhip.ERR_BAD_ARG
    assert L.svh_test_grid_trav(C.byref(G.default_params(nx=0)), C.byref(good), z.ctypes.data, zf.ctypes.data, z.ctypes.data, None, None,
                                None, None) == svhip.ERR_BAD_ARG
    assert (buf == 0xAB).all()
    # the entries refuse a null grid before anything else
    for call in (lambda: L.svh_grid_set_traversability(None, C.byref(good)), lambda: L.svh_grid_get_traversability(None, C.byref(good), None),
                 lambda: L.svh_grid_get_trav(None, 0, buf.ctypes.data, 0), lambda: L.svh_grid_render_cost(None, buf.ctypes.data, 0)):
        assert call() == svhip.ERR_BAD_ARG and "svh_grid" in svhip.last_error()
    L.svh_grid_trav_params_default(None)
    assert (buf == 0xAB).all()


ENTRIES = ("svh_grid_trav_params_default", "svh_grid_set_traversability", "svh_grid_get_traversability", "svh_grid_get_trav",
           "svh_grid_render_cost")


def test_entries_are_declared_and_exported(G):
    import svhip
    text = open(os.path.join(H.ROOT, "include", "svh_grid.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(svhip.lib(), name), name
    for name, value in (("SVH_GRID_TRAV_FLAGS", "0"), ("SVH_GRID_TRAV_DIST2", "1"), ("SVH_GRID_TRAV_COST", "2"),
                        ("SVH_GRID_LETHAL_OBSTACLE", "1u"), ("SVH_GRID_LETHAL_DROP", "2u"), ("SVH_GRID_LETHAL_STEEP", "4u"),
                        ("SVH_GRID_LETHAL_UNSEEN", "8u"), ("SVH_GRID_LETHAL_UNKNOWN_SEEN", "16u"), ("SVH_GRID_DIST2_FAR", "0x7FFFFFFF")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), hdr), name
    assert "Not done: slope" not in text
    assert (G.TRAV_FLAGS, G.TRAV_DIST2, G.TRAV_COST, G.DIST2_FAR) == (0, 1, 2, TR.FAR)
    assert C.sizeof(G.TravParams) == 16


# ---- the header once more, as a program of its own under the sanitizer -------------------------------------------------------
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_trav")
    exe = str(d / "grid_trav_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.PKG, "csrc"), "-o", exe, os.path.join(H.ROOT, "tests", "cxx", "grid_trav_check.cpp")])

    def run(nx, nz, cell, T, cls, hmean, state):
        head = np.zeros(7, np.uint32)
        head[:3] = [nx, nz, T.lethal & 0xFFFFFFFF]
        head[3:] = np.array([cell, T.max_slope, T.inscribed, T.inflate], F).view(np.uint32)
        job = str(d / "job.bin")
        with open(job, "wb") as f:
            f.write(head.tobytes() + np.asarray(cls, np.uint8).tobytes() + np.asarray(state, np.uint8).tobytes() + np.asarray(hmean, F).tobytes())
        r = subprocess.run([exe, job], capture_output=True)
        if r.returncode == 3:
            assert not r.stdout and not r.stderr
            return None
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out, n = r.stdout, nx * nz
        reach = int(np.frombuffer(out[:4], np.int32)[0])
        at = 4 + reach * reach + 1
        assert len(out) == at + 9 * n
        return dict(reach=reach, table=np.frombuffer(out[4:at], np.uint8), flags=np.frombuffer(out[at:at + n], np.uint8).reshape(nz, nx),
                    dist2=np.frombuffer(out[at + n:at + 5 * n], np.int32).reshape(nz, nx),
                    cost=np.frombuffer(out[at + 5 * n:at + 6 * n], np.uint8).reshape(nz, nx),
                    rgb=np.frombuffer(out[at + 6 * n:], np.uint8).reshape(nz, nx, 3))
    return run


SAN_CASES = [(0.5, dict(inflate=0.5, inscribed=0.0, max_slope=0.25), 33, 9, 0.1),        # reach 1
             (1.0, dict(inflate=256.0, inscribed=0.0, lethal=TR.L_OBSTACLE), 300, 3, 0.005),   # reach 256, wider than it
             (1.0, dict(inflate=256.0, inscribed=255.5, lethal=TR.L_ALL), 9, 9, 0.02),   # reach 256 on a window smaller than it
             (1e30, dict(inscribed=1e30, inflate=2.5e32, max_slope=3e38), 17, 5, 0.1),   # rise4 overflows to +Inf: nothing is steep
             (1e-38, dict(inscribed=0.0, inflate=2.5e-36, max_slope=1e-38), 17, 5, 0.1)]  # rise4 underflows to 0: every difference is steep


@pytest.mark.parametrize("k", range(len(SAN_CASES)))
def test_the_header_under_the_sanitizer(core, k):
    cell, kw, nx, nz, p = SAN_CASES[k]
    rng = np.random.default_rng(40 + k)
    T = TR.TravParams(**kw)
    cls, h, state = random_planes(rng, nx, nz, p)
    got = core(nx, nz, cell, T, cls, h, state)
    want = TR.layer(T, cell, cls, h, state)
    assert got["reach"] == TR.reach_of(T, cell) == (1 if k == 0 else 256 if k < 3 else got["reach"])
    assert np.array_equal(got["table"], TR.cost_table(T, cell))
    for name, w in want.items():
        assert np.array_equal(got[name], w), name
    if k == 3:
        assert not (got["flags"] & 1).any()
    if k == 4:
        assert (got["flags"] & 1).any()


def test_the_program_refuses_what_the_library_refuses(core):
    z = np.zeros((1, 1), np.uint8)
    for kw in BAD:
        assert core(1, 1, 0.5, TR.TravParams(**kw), z, np.zeros((1, 1), F), z) is None, kw
    for cell, inflate in ((1.0, 256.5), (0.005, 1.5), (1e-30, 1.5), (1e-45, 3e38)):
        assert core(1, 1, cell, TR.TravParams(inflate=inflate), z, np.zeros((1, 1), F), z) is None, (cell, inflate)
