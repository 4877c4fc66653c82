#!/usr/bin/env python3
"""Time the rollouts of the ground grid (svh_grid_roll_score, include/svh_grid.h, "ROLLOUT") on the device.

Scenes, on windows of 256 x 256 and 1024 x 1024 cells of 0.2 m, filled once from seeded points, one per cell, min_points 1, an
inflation radius of one cell (so the COST plane is 0 or 254), one goal near the far edge:
  open         every cell free
  random       three cells in ten an obstacle (the anchor's cell is free): nearly every candidate is cut within a few poses
Candidates: K constant-curvature arcs (-0.3 .. 0.3 per metre) of T poses, one every two cells, from the window's middle straight
ahead (svhip.grid.arc_candidates), K x T = 64 x 16, 256 x 32 and 1024 x 64; the default car (3.5 m + 1.0 m x 1.8 m, 207 cells under
it straight ahead) and a point vehicle (one cell).

One repetition of a side is timed with the host clock around whole calls, which return after their last stream wait:
  device       svh_grid_add_points of one point (the cached planes are stale) and svh_grid_roll_score into host records: k_grid_finalise,
               the three kernels of the cost map, the planner, the two rollout kernels and the copy of records, scores and best
  score        svh_grid_roll_score alone: the cost map and the field are cached, the two rollout kernels run
  host         what a caller did before the rollouts existed: the same add, svh_grid_get_trav(COST) and svh_grid_get_plan_plane(POT) to
               the host and the loop of csrc/grid_roll_core.h there (svh_test_grid_roll).  Such a caller fills its footprint table
               once, not per frame, and so does this side: svh_test_grid_roll keeps the table of the last vehicle and cell side, and
               the call that builds it is the comparison below, before anything is timed (host_first_call_ms, the planes already on
               the host, says what that call took).  What is timed besides the two copies and the loop is the binding: two
               contiguity checks and the allocation of the records in numpy
The sides alternate repetition by repetition in one process, the order reversed every other time; host - device is a paired
difference, given with its 10th and 90th percentiles.  Before anything is timed the device's records, scores and best are compared
with the host's.  Per case 3 warm-up and 20 timed repetitions: median, 10th and 90th percentile in ms.  One JSON line per case goes to
profiles/grid_roll_times.jsonl.  There is no threshold: this is a measurement.

    python tools/gpu_grid_roll.py [--out FILE] [--sizes 256,1024] [--reps WARMUP,TIMED] [--tag TEXT]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_grid_plan import CELL, fill, paired, summary   # noqa: E402

SHAPES = ((64, 16), (256, 32), (1024, 64))
VEHICLES = (("car", {}), ("point", dict(front=0.0, rear=0.0, half_width=0.0)))


def main():
    out = os.path.join(ROOT, "profiles", "grid_roll_times.jsonl")
    sizes, warmup, timed, tag = [256, 1024], 3, 20, ""
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
            else:
                raise ValueError(flag)
    except (IndexError, ValueError):
        raise SystemExit(__doc__)
    import svhip
    from svhip import grid as G
    G._bind()
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], np.float64)
    lines = []

    def emit(rec):
        rec = dict(dict(version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in sizes:
        for scene in ("open", "random"):
            rng = np.random.default_rng(n)
            wall = rng.random((n, n)) < 0.3 if scene == "random" else np.zeros((n, n), bool)
            mid = n // 2
            wall[mid, mid] = False
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            g.set_traversability(max_slope=4.0, inscribed=0.5 * CELL, inflate=CELL, lethal=G.LETHAL_OBSTACLE)
            fill(g, wall)
            g.set_goals(np.array([(mid, n - 2)], np.int32))
            anchor = np.array([(mid + 0.5) * CELL, 0.0, (mid + 0.5) * CELL])
            one = np.array([[anchor[0], 0.0, anchor[2], 0.5]], np.float32)
            for vehicle, vkw in VEHICLES:
                g.set_roll(G.default_roll(**vkw))
                roll, R, cells = g.roll_params()
                for K, T in SHAPES:
                    tab = G.arc_candidates(CELL, roll.headings_m, np.linspace(-0.3, 0.3, K), 2 * CELL, T)
                    s = 2 * roll.headings_m                            # straight ahead
                    tab = np.ascontiguousarray(tab[s:s + 1])
                    g.set_candidates(tab)

                    def device():
                        t0 = time.perf_counter()
                        g.add_points(one)
                        g.roll_score(anchor, 0)
                        return (time.perf_counter() - t0) * 1e3

                    def score():
                        t0 = time.perf_counter()
                        g.roll_score(anchor, 0)
                        return (time.perf_counter() - t0) * 1e3

                    def host():
                        t0 = time.perf_counter()
                        g.add_points(one)
                        cost, pot = g.trav_plane(G.TRAV_COST), g.plan_plane(G.PLAN_POT)
                        G.core_roll(roll, CELL, cost, pot, tab, 0, (mid, mid))
                        return (time.perf_counter() - t0) * 1e3
                    # the device's records against the host's, once, before anything is timed
                    best, recs, scores = g.roll_score(anchor, 0)
                    cost, pot = g.trav_plane(G.TRAV_COST), g.plan_plane(G.PLAN_POT)
                    t0 = time.perf_counter()
                    want = G.core_roll(roll, CELL, cost, pot, tab, 0, (mid, mid))   # the first call for a vehicle builds the host's table
                    first = (time.perf_counter() - t0) * 1e3
                    assert best == want["best"] and np.array_equal(recs, want["recs"]) and np.array_equal(scores, want["scores"]), (n, scene, vehicle, K, T)
                    ms = paired({"device": device, "score": score, "host": host}, warmup, timed)
                    rec = dict(case="roll", size=n, scene=scene, vehicle=vehicle, K=K, T=T, reach=R, footprint_cells=len(g.roll_footprint(s)),
                               group=G.roll_group(max(len(g.roll_footprint(k)) for k in range(8 * roll.headings_m))), best=best,
                               feasible=int((scores != G.ROLL_INFEASIBLE).sum()), poses_before_the_cuts=int(recs[:, 0].sum()),
                               host_first_call_ms=round(first, 4))
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
