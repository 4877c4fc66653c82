"""CPU: the contract of the ground grid's time layer (include/svh_grid_time.h: svh_grid_set_time, svh_grid_get_time_plane,
svh_grid_get_time_stats, svh_grid_time_path, svh_grid_render_time).  tests/grid_time_ref.py restates
stereo-vision_amd/csrc/grid_time_core.h in numpy and plain Python; this file pins the restatement with cases derived by hand,
compares the header itself with it -- evaluated on the host by the library's test entry svh_test_grid_time (core_time), and once more
as a program of its own under the address and undefined-behaviour sanitizers --, and checks what needs no device: the refusals, the
exports, the C99 header.

tests/test_grid_time_gpu.py compares the device with the header and the restatement.

Fields are indexed [t, ib, ia].  With neutral 50 a step between two cells of COST 0 weighs 5 * (50 + 50) = 500 across an edge and
700 across a corner; the default wait weighs 100.  With the default prediction parameters the slot of layer t is min(7, t)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_plan_ref as PL
import grid_pred_ref as PR
import grid_time_cases as TC
import grid_time_ref as TM
import grid_trav_ref as TR
import helpers as H

FAR = TM.FAR
WAIT = TM.DIR_WAIT
PP = PR.PredParams()


@pytest.fixture(scope="module")
def G():
    from svhip import grid
    grid._bind()
    return grid


def corridor(n, goal, blocked, **kw):
    """1 x n, all free, the goal at (goal, 0); blocked: {cell: layers at which an object stands on it}"""
    pred = np.zeros((1, n), np.uint32)
    for a, layers in blocked.items():
        pred[0, a] = TC.word(layers, PP)
    return TC.Case(np.zeros((1, n), np.uint8), [(goal, 0)], pred, **kw)


# ---- by hand -------------------------------------------------------------------------------------------------------------
def test_a_corridor_waits_for_the_object_that_crosses_it(G):
    """1 x 7, start (0, 0), goal (6, 0), an object on cell 3 at the layers 3, 4, 5.  Undisturbed the vehicle is on cell t at layer t
    and would enter cell 3 at layer 3; it may enter at layer 6 at the earliest: three waits.  A move that attains the minimum is
    preferred to the wait, so it drives to cell 2 first and waits there at the layers 2, 3, 4"""
    c = corridor(7, 6, {3: (3, 4, 5)}, tp=dict(layers=12), start=(0, 0))
    w = TC.agree(G, G.core_time, c)
    assert list(w["rpot"][0]) == [3000, 2500, 2000, 1500, 1000, 500, 0]
    assert w["tpot"][0, 0, 0] == 3000 + 3 * 100 and w["cost"] == 3300 and w["status"] == TM.FOUND
    assert list(w["tdir"][:6, 0, 2]) == [0, 0, WAIT, WAIT, WAIT, 0] and list(w["tdir"][:2, 0, 0]) == [0, 0]
    assert [tuple(p) for p in w["path"]] == [(0, 0, 0), (1, 0, 1), (2, 0, 2), (2, 0, 3), (2, 0, 4), (2, 0, 5), (3, 0, 6), (4, 0, 7), (5, 0, 8), (6, 0, 9)]
    assert (w["tpot"][3:6, 0, 3] == FAR).all() and (w["tdir"][3:6, 0, 3] == 9).all() and w["tpot"][6, 0, 3] == 1500
    assert TM.path_cost(PL.PlanParams(), TM.TimeParams(layers=12), w["rcost"], w["path"]) == 3300
    assert w["stats"] == (12, 12 * 7 - 3, 3, int((w["tdir"] == WAIT).sum()), 0) and w["stats"][3] >= 3
    # the last layer is the static field; beyond it the path follows RDIR with t kept at L - 1
    short = TC.agree(G, G.core_time, corridor(7, 6, {}, tp=dict(layers=3), start=(0, 0)))
    assert [tuple(p) for p in short["path"]] == [(0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 0, 2), (4, 0, 2), (5, 0, 2), (6, 0, 2)]


def test_without_the_wait_move_the_same_scene_detours_in_time_or_is_cut(G):
    """wait = -1 on the corridor: the vehicle can only go back and forth, two layers a pair; it enters cell 3 at the layers 3, 5, 7...,
    so at 7 -- four moves more.  With its back to the window's edge and the object on the next cell there is no move at all"""
    w = TC.agree(G, G.core_time, corridor(7, 6, {3: (3, 4, 5)}, tp=dict(layers=12, wait=-1), start=(0, 0)))
    assert w["tpot"][0, 0, 0] == 3000 + 4 * 500 and not (w["tdir"] == WAIT).any() and len(w["path"]) == 11
    w = TC.agree(G, G.core_time, corridor(5, 4, {1: (1, 2, 3)}, tp=dict(layers=8, wait=-1), start=(0, 0)))
    assert w["tpot"][0, 0, 0] == FAR and w["tdir"][0, 0, 0] == 9 and w["status"] == TM.UNREACHABLE and len(w["path"]) == 0
    w = TC.agree(G, G.core_time, corridor(5, 4, {1: (1, 2, 3)}, tp=dict(layers=8), start=(0, 0)))
    assert w["tpot"][0, 0, 0] == 2000 + 3 * 100 and list(w["tdir"][:4, 0, 0]) == [WAIT, WAIT, WAIT, 0]


def test_a_goal_that_is_blocked_at_a_layer(G):
    """1 x 3, the goal (2, 0) blocked at the layers 1 and 2: it is FAR there and 0 elsewhere; its neighbour waits twice"""
    w = TC.agree(G, G.core_time, corridor(3, 2, {2: (1, 2)}, tp=dict(layers=6), start=(1, 0)))
    assert list(w["tpot"][:, 0, 2]) == [0, FAR, FAR, 0, 0, 0] and list(w["tdir"][:, 0, 2]) == [8, 9, 9, 8, 8, 8]
    assert list(w["tpot"][:4, 0, 1]) == [700, 600, 500, 500] and list(w["tdir"][:3, 0, 1]) == [WAIT, WAIT, 0]
    assert [tuple(p) for p in w["path"]] == [(1, 0, 0), (1, 0, 1), (1, 0, 2), (2, 0, 3)]


def test_a_start_that_is_blocked_now(G):
    c = corridor(4, 3, {0: (0,)}, tp=dict(layers=4), start=(0, 0))
    w = TC.agree(G, G.core_time, c)
    assert w["status"] == TM.BLOCKED and len(w["path"]) == 0 and w["tpot"][0, 0, 0] == FAR and w["tpot"][1, 0, 0] == 1500
    c = TC.Case(np.array([[254, 0, 0]], np.uint8), [(2, 0)], tp=dict(layers=4), start=(0, 0))
    assert TC.agree(G, G.core_time, c)["status"] == TM.BLOCKED


def test_a_candidate_is_dropped_above_max_cost_inside_the_layers(G):
    """1 x 4, POT of the start 1500; an object on cell 1 at layer 1 costs one wait.  With max_cost = 1500 the static field reaches the
    start and the wait's candidate 1600 is dropped; with 1600 it is kept"""
    w = TC.agree(G, G.core_time, corridor(4, 3, {1: (1,)}, plan=dict(max_cost=1500), tp=dict(layers=6), start=(0, 0)))
    assert w["rpot"][0, 0] == 1500 and w["tpot"][0, 0, 0] == FAR and w["tpot"][1, 0, 0] == 1500 and w["status"] == TM.UNREACHABLE
    w = TC.agree(G, G.core_time, corridor(4, 3, {1: (1,)}, plan=dict(max_cost=1600), tp=dict(layers=6), start=(0, 0)))
    assert w["tpot"][0, 0, 0] == 1600 and w["tdir"][0, 0, 0] == WAIT


def test_one_layer_is_the_static_field_with_the_blocks(G):
    c = TC.random_case(5, 9, 6, 1)
    w = TC.agree(G, G.core_time, c)
    blk = TM.blocks(PR.PredParams(**c.pp), TM.TimeParams(**c.tp), c.pred, c.cost.shape, c.off, c.pred_off)[0]
    assert blk.any() and np.array_equal(w["tpot"][0], np.where(blk, FAR, w["rpot"])) and np.array_equal(w["tdir"][0], np.where(blk, 9, w["rdir"]))


def test_a_corner_step_needs_both_side_cells_free_at_the_next_layer(G):
    """2 x 2, start (0, 0), goal (1, 1): the corner step weighs 700.  An object on (1, 0) at layer 1 forbids it at layer 0; going
    round by (0, 1) weighs 1000, waiting one layer 800"""
    pred = np.zeros((2, 2), np.uint32)
    pred[0, 1] = TC.word((1,), PP)
    w = TC.agree(G, G.core_time, TC.Case(np.zeros((2, 2), np.uint8), [(1, 1)], pred, tp=dict(layers=4), start=(0, 0)))
    assert w["tpot"][0, 0, 0] == 800 and w["tdir"][0, 0, 0] == WAIT and w["tdir"][1, 0, 0] == 1
    w = TC.agree(G, G.core_time, TC.Case(np.zeros((2, 2), np.uint8), [(1, 1)], pred, tp=dict(layers=4, wait=400), start=(0, 0)))
    assert w["tpot"][0, 0, 0] == 1000 and w["tdir"][0, 0, 0] == 2


def wall_scene(release):
    """9 x 9 on cells of 0.5 m, inflation to 1.5 m (reach 3): a wall on column 0 and an object of 2 x 2 cells beside it, the id of a
    moving track on its cells"""
    flags, cls, ids = np.zeros((9, 9), np.uint8), np.full((9, 9), TC.FREE, np.uint8), np.full((9, 9), -1, np.int32)
    flags[:, 0] = TR.LETHAL
    flags[3:5, 2:4] = TR.LETHAL
    cls[flags != 0] = TC.OBSTACLE
    ids[3:5, 2:4] = 4
    trav = TR.TravParams(**TC.TRAV)
    cost = TR.cost(trav, TC.CELL, cls, flags, TR.dist2(flags != 0, 3))
    return TC.Case(cost, [(8, 8)], flags=flags, cls=cls, ids=ids, tracks=[TC.track(4)], trav=TC.TRAV, tp=dict(layers=3, release=release), start=(8, 0))


def test_release_takes_the_object_out_of_the_cost_map_and_leaves_the_wall(G):
    c = wall_scene(1)
    w = TC.agree(G, G.core_time, c)
    only_wall = np.zeros((9, 9), np.uint8)
    only_wall[:, 0] = TR.LETHAL
    alone = TR.cost(TR.TravParams(**TC.TRAV), TC.CELL, c.cls, only_wall, TR.dist2(only_wall != 0, 3))
    assert np.array_equal(w["rcost"], alone) and w["stats"][4] == 4
    assert (c.cost[3:5, 2:4] == 254).all() and (w["rcost"][3:5, 2] == alone[0, 2]).all() and alone[0, 2] not in (0, 254)   # the wall's inflation stays
    assert c.cost[4, 5] > 0 and w["rcost"][4, 5] == 0                                                                         # the object's is gone
    keep = TC.agree(G, G.core_time, wall_scene(0))
    assert np.array_equal(keep["rcost"], c.cost) and keep["stats"][4] == 0
    still = wall_scene(1)
    still.tracks[0, TM.PR.T["flags"]] = 0                                       # not moving: it does not predict under only_moving = 1
    assert np.array_equal(TC.agree(G, G.core_time, still)["rcost"], c.cost)
    still.pp = dict(only_moving=0)
    assert np.array_equal(TC.agree(G, G.core_time, still)["rcost"], alone)


# ---- the invariant, and the header against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_without_predictions_every_layer_is_the_static_field(G, seed):
    c = TC.random_case(20 + seed, 12 + 5 * seed, 7 + 2 * seed, 5, release=seed % 2, wait=1 if seed == 3 else 100, with_tracks=seed == 1)
    c.pred[:] = 0
    if seed == 1:
        c.tracks = c.tracks[:0]                                                 # nothing predicts: nothing is released
    pot, dir_, _ = PL.field(PL.PlanParams(**c.plan), c.cost, c.goals, c.off[0], c.off[1])
    g = TC.got(G, G.core_time, c)
    assert (pot != FAR).sum() > 1
    for t in range(5):
        assert np.array_equal(g["tpot"][t], pot) and np.array_equal(g["tdir"][t], dir_), t
    TC.agree(G, G.core_time, c)


RANDOM = [dict(nx=33, nz=18, L=9), dict(nx=1, nz=1, L=2), dict(nx=1, nz=17, L=4, wait=-1), dict(nx=18, nz=33, L=17, slots=32, stride=1, pps=1),
          dict(nx=20, nz=11, L=12, slots=3, stride=2, pps=2), dict(nx=16, nz=16, L=6, slots=1), dict(nx=25, nz=13, L=8, wait=65535, max_cost=90000),
          dict(nx=21, nz=14, L=6, release=1, with_tracks=True), dict(nx=14, nz=21, L=4, release=1, with_tracks=True, slots=32),
          dict(nx=30, nz=10, L=5, off=(2 ** 20 - 8192 - 30, -(2 ** 20 - 8192)), pred_off=(2 ** 20 - 8192 - 33, -(2 ** 20 - 8192) + 2))]


@pytest.mark.parametrize("k", range(len(RANDOM)))
def test_header_against_the_restatement_on_random_windows(G, k):
    c = TC.random_case(100 + k, **RANDOM[k])
    w = TC.agree(G, G.core_time, c, tag=str(RANDOM[k]))
    if RANDOM[k].get("slots") == 32:
        assert (c.pred >> 31).any()                                            # bit 31 is in play
    if k == 0:
        assert (w["tdir"] == WAIT).any() and w["stats"][2] > 0
    if RANDOM[k].get("with_tracks"):
        assert w["stats"][4] > 0 and not np.array_equal(w["rcost"], c.cost)


def test_the_slot_of_a_layer(G):
    assert [TM.slot_of_layer(PP, t) for t in (0, 1, 6, 7, 8, 40)] == [0, 1, 6, 7, 7, 7]
    q = PR.PredParams(slots=4, stride=2, poses_per_step=3)                      # rdiv(t, 6), halves up, clamped at 3
    assert [TM.slot_of_layer(q, t) for t in (0, 2, 3, 8, 9, 15, 21, 200)] == [0, 0, 1, 1, 2, 3, 3, 3]
    # the header says the same: a cell whose PRED word has the one bit s is FAR at exactly the layers of slot s
    for s_ in range(4):
        pred = np.array([[0, 1 << s_]], np.uint32)
        got = TC.got(G, G.core_time, TC.Case(np.zeros((1, 2), np.uint8), [(1, 0)], pred, pp=dict(slots=4, stride=2, poses_per_step=3), tp=dict(layers=30)))
        assert [t for t in range(30) if got["tpot"][t, 0, 1] == FAR] == [t for t in range(30) if TM.slot_of_layer(q, t) == s_], s_


# ---- what needs no device: the refusals, the exports, the headers -----------------------------------------------------------
BAD = [dict(layers=0), dict(layers=257), dict(wait=0), dict(wait=-2), dict(wait=65536), dict(release=2), dict(release=-1)]


def test_refusals(G):
    import svhip
    L = G._bind()
    for kw in BAD:
        p = G.default_time(**kw)
        assert L.svh_grid_set_time(None, C.byref(p)) == svhip.ERR_BAD_ARG
        with pytest.raises(svhip.SvhError):
            G.core_time(G.default_plan(), G.default_pred(), p, np.zeros((2, 2), np.uint8), goals=[(0, 0)])
    assert G.default_time().asdict() == dict(layers=32, wait=100, release=1) and C.sizeof(G.TimeParams) == 12
    with pytest.raises(svhip.SvhError):                                         # L nx nz above 2^28 is refused before anything is allocated
        G.core_time(G.default_plan(), G.default_pred(), G.default_time(layers=256), np.zeros((1025, 1024), np.uint8))
    with pytest.raises(svhip.SvhError):                                         # release = 1 with tracks needs CLASS and the traversability
        G.core_time(G.default_plan(), G.default_pred(), G.default_time(), np.zeros((2, 2), np.uint8), ids=np.zeros((2, 2), np.int32), tracks=[TC.track(0)])
    with pytest.raises(svhip.SvhError):                                         # the table in ascending order of id
        G.core_time(G.default_plan(), G.default_pred(), G.default_time(release=0), np.zeros((2, 2), np.uint8), ids=np.zeros((2, 2), np.int32),
                    tracks=[TC.track(3), TC.track(3)])
    buf = np.full(64, 0xAB, np.uint8)
    for f in (lambda: L.svh_grid_get_time(None, buf.ctypes.data_as(C.POINTER(G.TimeParams))), lambda: L.svh_grid_get_time_plane(None, 0, 0, 1, buf.ctypes.data, 0),
              lambda: L.svh_grid_get_time_stats(None, buf.ctypes.data), lambda: L.svh_grid_time_path(None, buf.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data),
              lambda: L.svh_grid_render_time(None, 0, buf.ctypes.data, 1, buf.ctypes.data, 0)):
        assert f() == svhip.ERR_BAD_ARG and "svh_grid" in svhip.last_error()
    L.svh_grid_time_params_default(None)
    assert (buf == 0xAB).all()


ENTRIES = ("svh_grid_time_params_default", "svh_grid_set_time", "svh_grid_get_time", "svh_grid_get_time_plane", "svh_grid_get_time_stats",
           "svh_grid_time_path", "svh_grid_render_time")


def test_entries_live_in_their_own_header_and_are_exported(G):
    import svhip
    inc = os.path.join(H.ROOT, "include")
    text = open(os.path.join(inc, "svh_grid_time.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    main = open(os.path.join(inc, "svh_grid.h")).read()
    assert '#include "svh_grid_time.h"' in main and main.index('#include "svh_grid_pred.h"') < main.index('#include "svh_grid_time.h"')
    assert sorted(set(re.findall(r"\b(svh_grid_[a-z0-9_]+)\s*\(", hdr))) == sorted(ENTRIES)
    others = {n: open(os.path.join(inc, n)).read() for n in sorted(os.listdir(inc)) if n.endswith(".h") and n != "svh_grid_time.h"}
    for name in ENTRIES:
        assert hasattr(svhip.lib(), name), name
        for other, body in others.items():
            assert name + "(" not in body, (name, other)
    for name in ("svh_test_grid_time", "svh_test_grid_time_device"):
        assert hasattr(svhip.lib(), name) and name not in text, name            # test entries: exported, not in the public header
    for k, name in enumerate(("SVH_GRID_TIME_TPOT", "SVH_GRID_TIME_TDIR", "SVH_GRID_TIME_RCOST", "SVH_GRID_TIME_RPOT")):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, k), hdr), name
    assert re.search(r"#define\s+SVH_GRID_TIME_WAIT\s+10\b", hdr) and G.TIME_WAIT == TM.DIR_WAIT == 10
    assert (G.TIME_TPOT, G.TIME_TDIR, G.TIME_RCOST, G.TIME_RPOT) == (0, 1, 2, 3) and len(G.TIME_STATS) == 6
    assert "CACHE" in text and "svh_grid_set_time" in text and "svh_grid_set_archive" in text   # the cache contract is in the head comment
    core = open(os.path.join(H.PKG, "csrc", "grid_time_core.h")).read()
    assert "INVARIANT" in core and "every layer of TPOT equals POT" in core    # the invariant is stated where the contract is
    for method in ("set_time", "time_params", "time_plane", "time_stats", "time_path", "render_time"):
        assert callable(getattr(G.Grid, method)), method


def test_header_is_c99(tmp_path):
    exe = str(tmp_path / "grid_time_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cxx", "grid_time_c99.c"), "-L", H.PKG, "-lsvhip", "-Wl,-rpath," + H.PKG])
    out = subprocess.check_output([exe]).decode()
    assert "svh_grid_time.h: C99 ok, planes 0..3, wait 10, statuses 0..3" in out


# ---- the header once more, as a program of its own under the sanitizers ------------------------------------------------------
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_time")
    exe = str(d / "grid_time_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.PKG, "csrc"), "-o", exe, os.path.join(H.ROOT, "tests", "cxx", "grid_time_check.cpp")])

    def run(c):
        nz, nx = c.cost.shape
        plan, pp, tp = PL.PlanParams(**c.plan), PR.PredParams(**c.pp), TM.TimeParams(**c.tp)
        trav = TR.TravParams(**(c.trav or TC.TRAV))
        table = TR.cost_table(trav, c.cell)
        reach = TR.reach_of(trav, c.cell)
        start = c.start if c.start is not None else (-1, -1)
        head = np.array([nx, nz, c.off[0], c.off[1], c.pred_off[0], c.pred_off[1], plan.neutral, plan.unknown, plan.max_cost, pp.slots, pp.stride,
                         pp.poses_per_step, pp.only_moving, tp.layers, tp.wait, tp.release, reach, len(c.goals), len(c.tracks), start[0], start[1]],
                        np.int64).astype(np.int32)
        cls = c.cls if c.cls is not None else np.full((nz, nx), TC.FREE, np.uint8)
        ids = c.ids if c.ids is not None else np.full((nz, nx), -1, np.int32)
        job = str(d / "job.bin")
        with open(job, "wb") as f:
            f.write(head.tobytes() + c.goals.tobytes() + c.tracks.tobytes() + c.cost.tobytes() + c.flags.tobytes() + np.ascontiguousarray(cls, np.uint8).tobytes()
                    + table.tobytes() + c.pred.tobytes() + np.ascontiguousarray(ids, np.int32).tobytes())
        r = subprocess.run([exe, job], capture_output=True)
        if r.returncode == 3:
            assert not r.stdout and not r.stderr
            return None
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out, n, L = r.stdout, nx * nz, tp.layers
        at = [0]

        def take(dtype, count, shape=None):
            size = np.dtype(dtype).itemsize * count
            v = np.frombuffer(out[at[0]:at[0] + size], dtype)
            at[0] += size
            return v.reshape(shape) if shape else v
        released = int(take(np.int64, 1)[0])
        got = dict(rcost=take(np.uint8, n, (nz, nx)), rpot=take(np.int32, n, (nz, nx)), rdir=take(np.uint8, n, (nz, nx)),
                   tpot=take(np.int32, L * n, (L, nz, nx)), tdir=take(np.uint8, L * n, (L, nz, nx)))
        got["stats"] = tuple(int(v) for v in take(np.int64, 4)) + (released,)
        status, ln = (int(v) for v in take(np.int64, 2))
        got.update(status=status, path=take(np.int32, 3 * ln, (ln, 3)))
        assert at[0] == len(out)
        return got
    return run


SAN_CASES = [dict(nx=33, nz=9, L=7), dict(nx=1, nz=40, L=3, wait=-1), dict(nx=17, nz=17, L=34, slots=32, share=0.4),
             dict(nx=19, nz=12, L=5, release=1, with_tracks=True), dict(nx=1, nz=1, L=1),
             dict(nx=40, nz=2, L=4, off=(2 ** 20 - 8192 - 40, -(2 ** 20 - 8192)), pred_off=(2 ** 20 - 8192 - 38, -(2 ** 20 - 8192) + 1), slots=32)]


@pytest.mark.parametrize("k", range(len(SAN_CASES)))
def test_the_header_under_the_sanitizers(core, k):
    c = TC.random_case(60 + k, **SAN_CASES[k])
    got, w = core(c), TC.want(c)
    for name in ("rcost", "rpot", "rdir", "tpot", "tdir"):
        assert np.array_equal(got[name], w[name]), name
    assert got["stats"] == w["stats"] and got["status"] == w["status"] and np.array_equal(got["path"], w["path"])


def test_the_heaviest_candidates_under_the_sanitizers(core):
    """a row of prices 507 with the horizon one below FAR and the heaviest wait: 39 steps of 5 * 1014, and 65535 where the object makes
    the vehicle wait; bit 31 is the slot of every layer from 31 on"""
    pp = dict(slots=32)
    pred = np.zeros((1, 40), np.uint32)
    pred[0, 20] = TC.word((33,), PR.PredParams(**pp))
    c = TC.Case(np.full((1, 40), 252, np.uint8), [(0, 0)], pred, plan=dict(neutral=255, max_cost=0x7FFFFFFE), pp=pp, tp=dict(layers=60, wait=65535), start=(39, 0))
    got, w = core(c), TC.want(c)
    assert np.array_equal(got["tpot"], w["tpot"]) and np.array_equal(got["tdir"], w["tdir"]) and np.array_equal(got["path"], w["path"])
    assert pred[0, 20] == 1 << 31 and (w["tpot"][31:, 0, 20] == FAR).all() and w["tpot"][30, 0, 20] == 20 * 5070
    assert w["rpot"][0, 39] == 39 * 5070 and w["tpot"][0, 0, 39] == 39 * 5070   # it passes cell 20 at layer 19, before the object


def test_the_program_refuses_what_the_library_refuses(core):
    for kw in BAD:
        assert core(TC.Case(np.zeros((1, 1), np.uint8), [(0, 0)], tp=kw)) is None, kw
