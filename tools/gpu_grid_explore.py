#!/usr/bin/env python3
"""Time the ranking of the frontiers (svh_grid_explore_rank, include/svh_grid.h, "EXPLORATION") on the device.

Scenes, on windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m with R = 16, 50 and 128 cells, filled as
tools/gpu_grid_front.py fills them (one point per cell that has any, min_points 1, an inflation radius of one cell, no obstacle;
a cell without a point is unknown and was never looked at):
  rim      an open field with an unexplored rim of two cells: one closed frontier round the window
  clutter  three cells in ten unknown: many small components, most of them dropped (min_size 8)
  spiral   the corridor of one free cell between walls of one unknown cell: one component, and a reach field that runs the whole
           corridor -- the shape on which the planner's relaxation needs a round per tile crossing
The ranking starts from a free cell near the middle of the window.  --unknown N is the planner's price of an unknown cell: 100 by
default, as tools/stereomapper_pipeline.py sets it, so that the reach field crosses unknown cells; -1 makes them impassable, and
the spiral then is a maze of one corridor, the shape on which the planner's relaxation loses to the host's heap.

One repetition of a side is timed with the host clock around whole calls, which return after their last stream wait:
  device   svh_grid_add_points of one point (every cached plane is stale), then svh_grid_explore_rank into a host table: the
           finished planes, the cost map, the frontiers, the reach field, the gains, the scores and the copy of the table
  host     what a caller does without it: the same add, STATE, COST and the frontier table to the host, then the header's host
           forms there -- gain_window of csrc/grid_explore_core.h on the representatives (svh_test_grid_explore), the heap Dijkstra
           of csrc/grid_plan_core.h from the start (svh_test_grid_plan) -- and the scores in numpy
The sides alternate repetition by repetition in one process, the order reversed every other time.  Before anything is timed the
two tables are compared.  Per case 3 warm-up and 20 timed repetitions (1 and 5 where one repetition takes more than a second or
the window has more than 1024 x 1024 cells): median, 10th and 90th percentile in ms, and the paired difference host - device.
One JSON line per case goes to profiles/grid_explore_times.jsonl.  There is no threshold: this is a measurement.

    python tools/gpu_grid_explore.py [--out FILE] [--sizes 256,1024,8192] [--ranges 16,50,128] [--scenes rim,clutter,spiral]
                                     [--unknown N] [--reps WARMUP,TIMED] [--tag TEXT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_grid_front import fill, filled           # noqa: E402
from gpu_grid_plan import CELL, paired, summary   # noqa: E402


def main():
    out = os.path.join(ROOT, "profiles", "grid_explore_times.jsonl")
    sizes, ranges, scenes, warmup, timed, tag, unknown = [256, 1024, 8192], [16, 50, 128], ["rim", "clutter", "spiral"], 3, 20, "", 100
    argv = sys.argv[1:]
    try:
        while argv:
            flag, value = argv[0], argv[1]
            argv = argv[2:]
            if flag == "--out":
                out = value
            elif flag == "--sizes":
                sizes = [int(v) for v in value.split(",")]
            elif flag == "--ranges":
                ranges = [int(v) for v in value.split(",")]
            elif flag == "--scenes":
                scenes = value.split(",")
            elif flag == "--reps":
                warmup, timed = (int(v) for v in value.split(","))
            elif flag == "--tag":
                tag = value
            elif flag == "--unknown":
                unknown = int(value)
            else:
                raise ValueError(flag)
    except (IndexError, ValueError):
        raise SystemExit(__doc__)
    import svhip
    from svhip import grid as G
    L = G._bind()
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], np.float64)
    lines = []

    def emit(rec):
        rec = dict(dict(version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in sizes:
        for scene in scenes:
            rng = np.random.default_rng(n)
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            g.set_traversability(max_slope=4.0, inscribed=0.5 * CELL, inflate=CELL, lethal=G.LETHAL_OBSTACLE)
            g.set_plan(unknown=unknown)
            has = filled(scene, n, rng)
            fill(g, has)
            b, a = np.argwhere(has)[len(has) // 2]
            one = np.array([[(a + 0.5) * CELL, 0.0, (b + 0.5) * CELL, 0.5]], np.float32)     # a second point on a free cell
            near = np.argwhere(has[n // 2 - 2:n // 2 + 3, n // 2 - 2:n // 2 + 3])[0] + (n // 2 - 2)
            start_cell = np.array([near[1], near[0]], np.int32)                               # a free cell near the middle
            start = np.array([(start_cell[0] + 0.5) * CELL, 0.0, (start_cell[1] + 0.5) * CELL], np.float64)
            front, plan = g.frontier_params(), g.plan_params()
            for R in ranges:
                g.set_explore(range=(R + 0.5) * CELL)
                explore, got_R = g.explore_params()
                assert got_R == R
                kept = g.frontier_stats()[2]
                cap = max(min(kept, 65536), 1)
                recs, scores = np.zeros((cap, G.EXPLORE_RECORD), np.int32), np.zeros(cap, np.int64)
                n_recs, best = C.c_int64(-1), C.c_int32(-9)
                host = {}

                def device_side():
                    t0 = time.perf_counter()
                    g.add_points(one)
                    G._check(L.svh_grid_explore_rank(g._h, start.ctypes.data, recs.ctypes.data, scores.ctypes.data, cap, C.addressof(n_recs), C.addressof(best)))
                    return (time.perf_counter() - t0) * 1e3

                def host_side():
                    t0 = time.perf_counter()
                    g.add_points(one)
                    state, cost, table = g.local_plane(G.LOCAL_STATE), g.trav_plane(G.TRAV_COST), g.frontiers()[:65536]
                    reps = np.ascontiguousarray(table[:, 8:10])
                    gains = G.core_explore(explore, CELL, state, front=front, cells=reps)["gains"] if len(reps) else np.zeros(0, np.int32)
                    pot = G.core_plan(g.params, plan, cost, [start_cell])[0]
                    reach = pot[reps[:, 1], reps[:, 0]].astype(np.int64)
                    ok = (reach != G.PLAN_FAR) & (gains >= explore.min_gain)
                    sc = np.where(ok, explore.w_reach * reach - explore.w_gain * gains.astype(np.int64), G.EXPLORE_INFEASIBLE)
                    host["recs"] = np.stack([table[:, 0], reps[:, 0], reps[:, 1], gains, reach.astype(np.int32)], 1).astype(np.int32)
                    host["scores"], host["best"] = sc, (int(np.argmin(sc)) if ok.any() else -1)
                    return (time.perf_counter() - t0) * 1e3
                # the device's table against the host's, once, before anything is timed
                t0 = time.perf_counter()
                host_side()
                slow = time.perf_counter() - t0 > 1.0 or n > 1024
                device_side()
                m = n_recs.value
                assert m == len(host["recs"]) and np.array_equal(recs[:m], host["recs"]) and np.array_equal(scores[:m], host["scores"]) and \
                    best.value == host["best"], (n, scene, R)
                ms = paired({"device": device_side, "host": host_side}, 1 if slow else warmup, 5 if slow else timed)
                st = g.explore_stats()
                rec = dict(case="explore_rank", size=n, scene=scene, R=R, unknown=unknown, records=st[0], feasible=st[1], best=best.value, reps=len(ms["device"]))
                for name, v in ms.items():
                    rec.update(summary(name, v))
                rec.update(summary("host_minus_device", [x - y for x, y in zip(ms["host"], ms["device"])]))
                emit(rec)
            g.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
