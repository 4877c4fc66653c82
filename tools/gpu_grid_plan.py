#!/usr/bin/env python3
"""Time the planner of the ground grid (svh_grid_plan_*, include/svh_grid.h, "PLANNING") on the device.

Scenes, on windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m, filled once from seeded points, one per cell,
min_points 1, an inflation radius of one cell (so the COST plane is 0 or 254 and a corridor of one cell stays open):
  open         every cell free, one goal in the middle: ties everywhere
  random       three cells in ten an obstacle, one goal in the middle (its cell is free)
  serpentine   corridors of one cell along the rows, openings at alternating ends, the goal in a corner: one route through
               every corridor, which crosses a tile border every PLAN_TILE cells (not at 8192: its route has 33 million cells)

One repetition of a side is timed with the host clock around whole calls, which return after their last stream wait:
  field        svh_grid_add_points of one point (the cached planes are stale), svh_grid_plan_set_goals and
               svh_grid_get_plan_plane(POT) into a device buffer: k_grid_finalise, the three kernels of the cost map, the
               planner's seed, goals, rounds and DIR, and the copy of the plane
  plan         svh_grid_plan_set_goals and svh_grid_get_plan_plane(POT) alone: the cost map is cached, the planner runs
  host         what a caller did before the planner existed: the same add, svh_grid_get_trav(COST) to the host and the heap
               Dijkstra of csrc/grid_plan_core.h on the host (svh_test_grid_plan)
The sides alternate repetition by repetition in one process, the order reversed every other time.  Where the library has
the switches, further sides alternate with them: `plain` (svh_test_grid_plan_form: one lane per cell, one whole-window sweep
per launch, repeated until nothing changes) and plan_w1, plan_w2, plan_w8, plan_w16 (svh_test_grid_plan_rounds_per_wait: the
rounds the host enqueues per wait; the library's default is 4).  Paired differences are given with their 10th and 90th
percentiles.  The rounds of the last field are reported per side.

Paths: svh_grid_plan_path on the cached field of the 256 x 256 serpentine, from starts whose paths have about 100, 1 000 and
10 000 cells: ms per call and ns per cell.

Per case 3 warm-up and 20 timed repetitions (fewer where one repetition takes more than a second): median, 10th and 90th
percentile in ms.  One JSON line per case goes to profiles/grid_plan_times.jsonl, with the tile side the library was built
with.  There is no threshold: this is a measurement.

--lib PATH loads another build of libsvhip.so, for the comparison of tile sides: -DSVH_PLAN_TILE=16, 32 or 64 on
csrc/grid_plan_kernels.hip and csrc/grid_engine.cpp; each build is a process of its own, so tile sides do not alternate.

    python tools/gpu_grid_plan.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED] [--tag TEXT] [--lib PATH]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))

CELL = 0.2
PIECE = 1 << 22
WAITS = (1, 2, 8, 16)


def pct(ms, q):
    return round(float(np.percentile(np.array(ms), q)), 4)


def summary(prefix, ms):
    return {prefix + "_median_ms": pct(ms, 50), prefix + "_p10_ms": pct(ms, 10), prefix + "_p90_ms": pct(ms, 90)}


def paired(sides, warmup, timed):
    """sides: name -> callable returning the ms it timed; they alternate, the order reversed every other repetition"""
    names = list(sides)
    ms = {n: [] for n in names}
    for k in range(warmup + timed):
        for n in (names if k % 2 == 0 else names[::-1]):
            t = sides[n]()
            if k >= warmup:
                ms[n].append(t)
    return ms


def blocked(scene, nx, nz, rng):
    """bool [nz, nx]: the cells that hold an obstacle"""
    if scene == "open":
        return np.zeros((nz, nx), bool)
    if scene == "random":
        w = rng.random((nz, nx)) < 0.3
        w[nz // 2, nx // 2] = False
        return w
    w = np.zeros((nz, nx), bool)
    w[1::2] = True
    for k, b in enumerate(range(1, nz, 2)):
        w[b, nx - 1 if k % 2 == 0 else 0] = False
    return w


def fill(g, wall):
    """one point in the middle of every cell, a metre up where `wall`"""
    nz, nx = wall.shape
    flat = wall.ravel()
    for at in range(0, nx * nz, PIECE):
        i = np.arange(at, min(at + PIECE, nx * nz))
        p = np.zeros((len(i), 4), np.float32)
        p[:, 0], p[:, 2] = (i % nx + 0.5) * CELL, (i // nx + 0.5) * CELL
        p[:, 1] = np.where(flat[i], -1.0, 0.0)
        p[:, 3] = 0.5
        g.add_points(p)


def main():
    out = os.path.join(ROOT, "profiles", "grid_plan_times.jsonl")
    sizes, warmup, timed, tag, lib_path = [256, 1024, 8192], 3, 20, "", None
    argv = sys.argv[1:]
    try:
        while argv:
            flag, value = argv[0], argv[1]
            argv = argv[2:]
            if flag == "--out":
                out = value
            elif flag == "--sizes":
                sizes = [int(v) for v in value.split(",")]
            elif flag == "--reps":
                warmup, timed = (int(v) for v in value.split(","))
            elif flag == "--tag":
                tag = value
            elif flag == "--lib":
                lib_path = value
            else:
                raise ValueError(flag)
    except (IndexError, ValueError):
        raise SystemExit(__doc__)
    import svhip
    if lib_path:
        svhip.LIB_PATH = lib_path          # a build of the library with another -DSVH_PLAN_TILE
    from svhip import grid as G
    L = G._bind()
    hip = C.CDLL("libamdhip64.so")
    has_form, has_wait = hasattr(L, "svh_test_grid_plan_form"), hasattr(L, "svh_test_grid_plan_rounds_per_wait")
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], np.float64)
    lines = []

    def emit(rec):
        rec = dict(dict(tile=G.PLAN_TILE, version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in sizes:
        dev = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), C.c_size_t(4 * n * n)) == 0
        for scene in ("open", "random", "serpentine"):
            if scene == "serpentine" and n > 1024:
                continue
            rng = np.random.default_rng(n)
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            g.set_traversability(max_slope=4.0, inscribed=0.5 * CELL, inflate=CELL, lethal=G.LETHAL_OBSTACLE)
            fill(g, blocked(scene, n, n, rng))
            goal = np.array([(0, 0) if scene == "serpentine" else (n // 2, n // 2)], np.int32)
            one = np.array([[(goal[0, 0] + 0.5) * CELL, 0.0, (goal[0, 1] + 0.5) * CELL, 0.5]], np.float32)
            P, plan = G.default_params(nx=n, nz=n), G.default_plan()
            rounds = {}

            def field(name="field"):
                t0 = time.perf_counter()
                g.add_points(one)
                g.set_goals(goal)
                g.plan_plane(G.PLAN_POT, device_ptr=dev.value)
                t = (time.perf_counter() - t0) * 1e3
                rounds[name] = g.plan_stats()[3]
                return t

            def plan_only(name="plan"):
                t0 = time.perf_counter()
                g.set_goals(goal)
                g.plan_plane(G.PLAN_POT, device_ptr=dev.value)
                t = (time.perf_counter() - t0) * 1e3
                rounds[name] = g.plan_stats()[3]
                return t

            def host():
                t0 = time.perf_counter()
                g.add_points(one)
                cost = g.trav_plane(G.TRAV_COST)
                G.core_plan(P, plan, cost, goal)
                return (time.perf_counter() - t0) * 1e3

            def switched(call, name, form=None, wait=None):
                def side():
                    was_f = L.svh_test_grid_plan_form(form) if form is not None else None
                    was_w = L.svh_test_grid_plan_rounds_per_wait(wait) if wait is not None else None
                    try:
                        return call(name)
                    finally:
                        if form is not None:
                            L.svh_test_grid_plan_form(was_f)
                        if wait is not None:
                            L.svh_test_grid_plan_rounds_per_wait(was_w)
                return side
            sides = {"field": field, "plan": plan_only, "host": host}
            if has_form and not (scene == "serpentine" and n > 256):     # the plain serpentine needs a round per cell of the route
                sides["plain"] = switched(plan_only, "plain", form=1)
            if has_wait:
                for w in WAITS:
                    sides["plan_w%d" % w] = switched(plan_only, "plan_w%d" % w, wait=w)
            # the device's POT against the host's, once, before anything is timed
            g.set_goals(goal)
            pot = g.plan_plane(G.PLAN_POT)
            want = G.core_plan(P, plan, g.trav_plane(G.TRAV_COST), goal)[0]
            assert np.array_equal(pot, want), (n, scene)
            t0 = time.perf_counter()
            field()
            slow = time.perf_counter() - t0 > 1.0 or n > 1024
            ms = paired(sides, 1 if slow else warmup, 5 if slow else timed)
            rec = dict(case="field", size=n, scene=scene, reached=g.plan_stats()[2], rounds=rounds)
            for name, v in ms.items():
                rec.update(summary(name, v))
            for a, b in (("host", "field"), ("plain", "plan")) + tuple(("plan_w%d" % w, "plan") for w in WAITS):
                if a in ms and b in ms:
                    rec.update(summary("%s_minus_%s" % (a, b), [x - y for x, y in zip(ms[a], ms[b])]))
            emit(rec)
            if scene == "serpentine" and n == 256:
                pot = g.plan_plane(G.PLAN_POT)
                for want_len in (100, 1000, 10000):
                    b, a = np.argwhere(pot == 500 * (want_len - 1))[0]
                    xyz = np.array([(a + 0.5) * CELL, 0.0, (b + 0.5) * CELL])
                    st, cells, _ = g.path(xyz)
                    assert st == G.PATH_FOUND and len(cells) == want_len
                    v = []
                    for k in range(warmup + timed):
                        t0 = time.perf_counter()
                        g.path(xyz, cap=want_len)
                        if k >= warmup:
                            v.append((time.perf_counter() - t0) * 1e3)
                    emit(dict(dict(case="path", cells=want_len, ns_per_cell=round(pct(v, 50) * 1e6 / want_len, 1)), **summary("path", v)))
            g.close()
        hip.hipFree(dev)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
