#!/usr/bin/env python3
"""Time the pose planner of the ground grid (svh_grid_pose_*, include/svh_grid_pose.h) on the device.

Scenes, on windows of 256 x 256 and 1024 x 1024 cells of 0.2 m, filled once from seeded points, one per cell, min_points 1, an
inflation radius of one cell (so the COST plane is 0 or 254 and a corridor of one cell stays open), as tools/gpu_grid_plan.py:
  open         every cell free, every heading of the middle cell a goal
  random       three cells in ten an obstacle, every heading of the middle cell (free) a goal
  serpentine   corridors of one cell along the rows, openings at alternating ends, the goal in a corner.  Only the point vehicle
               with spin = 100 gets through: the turn at a corridor's end is a spin on the spot
Vehicles: the point (front = rear = half_width = 0) and the default car (3.5 m, 1.0 m, 0.9 m: 23 x 9 cells).

One repetition of a side is timed with the host clock around whole calls, which return after their last stream wait:
  field   svh_grid_add_points of one point (the cached planes are stale), svh_grid_pose_set_goals and
          svh_grid_get_pose_plane(POT) into a device buffer: k_grid_finalise, the three kernels of the cost map,
          k_grid_pose_foot, the seed, goals, rounds and PDIR, and the copy of the eight planes
  pose    svh_grid_pose_set_goals and svh_grid_get_pose_plane(POT) alone: the cost map and CF are cached
  host    what a caller can do without the layer: the same add, svh_grid_get_trav(COST) to the host, then the CF loop and the
          heap Dijkstra of csrc/grid_pose_core.h there (svh_test_grid_pose)
The sides alternate repetition by repetition in one process, the order reversed every other time; paired differences are given
with their 10th and 90th percentiles.

CF alone (case "cf"): svh_grid_set_roll with the parameters in force (CF and the uploaded table are stale), then
svh_grid_get_pose_plane(CF) into a device buffer, against svh_grid_footprint_cost(on_device) over all 8 nx nz poses after the same
svh_grid_set_roll; alternating as above.
Paths (case "path"): svh_grid_pose_path on the cached field of the 256 x 256 serpentine for paths of 100 and 1 000 poses.

Per case 3 warm-up and 20 timed repetitions (1 and 3 where one repetition takes more than a second).  One JSON line per case goes
to profiles/grid_pose_times.jsonl.  There is no threshold: this is a measurement.

    python tools/gpu_grid_pose.py [--out FILE] [--sizes 256,1024] [--reps WARMUP,TIMED] [--tag TEXT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gpu_grid_plan as GP  # noqa: E402  the scenes, the fill and the paired loop are the planner tool's

CELL = GP.CELL
POINT = dict(front=0.0, rear=0.0, half_width=0.0)
CAR = dict(front=3.5, rear=1.0, half_width=0.9)


def main():
    out = os.path.join(ROOT, "profiles", "grid_pose_times.jsonl")
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
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], np.float64)
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def emit(rec):
        rec = dict(dict(tile=16, version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        with open(out, "a") as f:                     # line by line: a run that is cut short keeps what it measured
            f.write(lines[-1] + "\n")

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        return p

    for n in sizes:
        states = 8 * n * n
        dev = alloc(4 * states)
        for scene in ("open", "random", "serpentine"):
            rng = np.random.default_rng(n)
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            g.set_traversability(max_slope=4.0, inscribed=0.5 * CELL, inflate=CELL, lethal=G.LETHAL_OBSTACLE)
            GP.fill(g, GP.blocked(scene, n, n, rng))
            cell = (0, 0) if scene == "serpentine" else (n // 2, n // 2)
            goal = np.array([(cell[0], cell[1], -1)], np.int32)
            one = np.array([[(cell[0] + 0.5) * CELL, 0.0, (cell[1] + 0.5) * CELL, 0.5]], np.float32)
            for vehicle, rkw in (("point", POINT), ("car", CAR)):
                if scene == "serpentine" and vehicle == "car":
                    continue
                g.set_roll(**rkw)
                g.set_pose(spin=100 if scene == "serpentine" else -1)
                roll, pose = g.roll_params()[0], g.pose_params()
                rounds = {}

                def field():
                    t0 = time.perf_counter()
                    g.add_points(one)
                    g.pose_set_goals(goal)
                    g.pose_plane(G.POSE_POT, device_ptr=dev.value)
                    t = (time.perf_counter() - t0) * 1e3
                    rounds["field"] = g.pose_stats()[3]
                    return t

                def pose_only():
                    t0 = time.perf_counter()
                    g.pose_set_goals(goal)
                    g.pose_plane(G.POSE_POT, device_ptr=dev.value)
                    t = (time.perf_counter() - t0) * 1e3
                    rounds["pose"] = g.pose_stats()[3]
                    return t

                def host():
                    t0 = time.perf_counter()
                    g.add_points(one)
                    cost = g.trav_plane(G.TRAV_COST)
                    G.core_pose(roll, pose, CELL, cost, goal)
                    return (time.perf_counter() - t0) * 1e3

                # the device's field against the host's, once, before anything is timed
                g.pose_set_goals(goal)
                pot = g.pose_plane(G.POSE_POT)
                t0 = time.perf_counter()
                want = G.core_pose(roll, pose, CELL, g.trav_plane(G.TRAV_COST), goal)
                slow = time.perf_counter() - t0 > 1.0
                assert np.array_equal(pot, want[1]) and np.array_equal(g.pose_plane(G.POSE_CF), want[0]), (n, scene, vehicle)
                del want
                ms = GP.paired({"field": field, "pose": pose_only, "host": host}, 1 if slow else warmup, 3 if slow else timed)
                st = g.pose_stats()
                rec = dict(case="field", size=n, scene=scene, vehicle=vehicle, counted=st[1], reached=st[2], rounds=rounds)
                for name, v in ms.items():
                    rec.update(GP.summary(name, v))
                rec.update(GP.summary("host_minus_field", [x - y for x, y in zip(ms["host"], ms["field"])]))
                emit(rec)
                if scene == "open":
                    # CF alone against the form that exists without the layer: svh_grid_footprint_cost over every pose
                    m = roll.headings_m
                    d, b, a = np.meshgrid(np.arange(8), np.arange(n), np.arange(n), indexing="ij")
                    poses = np.stack([a.ravel(), b.ravel(), d.ravel() * m], 1).astype(np.int32)
                    d_poses, d_f = alloc(poses.nbytes), alloc(4 * states)
                    assert hip.hipMemcpy(d_poses, poses.ctypes.data, poses.nbytes, 1) == 0
                    del poses, d, b, a

                    def cf_layer():
                        t0 = time.perf_counter()
                        g.set_roll()
                        g.pose_plane(G.POSE_CF, device_ptr=dev.value)
                        return (time.perf_counter() - t0) * 1e3

                    def cf_poses():
                        t0 = time.perf_counter()
                        g.set_roll()
                        g.footprint_cost(device_ptrs=(d_poses.value, d_f.value), n=states)
                        return (time.perf_counter() - t0) * 1e3
                    ms = GP.paired({"cf_layer": cf_layer, "cf_poses": cf_poses}, warmup, timed)
                    rec = dict(case="cf", size=n, vehicle=vehicle, footprint_cells=int(len(g.roll_footprint(0))))
                    for name, v in ms.items():
                        rec.update(GP.summary(name, v))
                    rec.update(GP.summary("cf_poses_minus_cf_layer", [x - y for x, y in zip(ms["cf_poses"], ms["cf_layer"])]))
                    emit(rec)
                    hip.hipFree(d_poses)
                    hip.hipFree(d_f)
                if scene == "serpentine" and n == 256:
                    g.pose_set_goals(goal)
                    far = [(n - 1.5) * CELL, 0.0, 40.5 * CELL]                   # a start in the corridor of row 40, facing along it
                    st_, whole, _ = g.pose_path(far, 0)
                    assert st_ == G.PATH_FOUND and len(whole) > 1000, (st_, len(whole))
                    for want_len in (100, 1000):
                        ga, gb, k = (int(v) for v in whole[len(whole) - want_len])
                        xyz = np.array([(ga + 0.5) * CELL, 0.0, (gb + 0.5) * CELL])
                        st_, poses, _ = g.pose_path(xyz, k // roll.headings_m)
                        assert st_ == G.PATH_FOUND and len(poses) == want_len
                        v = []
                        for k_ in range(warmup + timed):
                            t0 = time.perf_counter()
                            g.pose_path(xyz, k // roll.headings_m, cap=want_len)
                            if k_ >= warmup:
                                v.append((time.perf_counter() - t0) * 1e3)
                        emit(dict(dict(case="path", poses=want_len, ns_per_pose=round(GP.pct(v, 50) * 1e6 / want_len, 1)), **GP.summary("path", v)))
            g.close()
        hip.hipFree(dev)


if __name__ == "__main__":
    main()
