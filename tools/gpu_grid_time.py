#!/usr/bin/env python3
"""Time the time layer of the ground grid (svh_grid_set_time, svh_grid_get_time_plane, include/svh_grid_time.h) on the device.

Scenes are those of tools/gpu_grid_pred.py: windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m, a seeded random field of
obstacle cells at a density of 0.01 and of 0.3, one point 1 m high per obstacle cell, min_points 1, the object parameters the defaults
but max_tracks 4096, three steps taken.  The field stands, so only_moving is 0: every track with a label predicts, is RELEASED from
the cost map (release = 1: the release kernel, the second distance pass and the second planner job all run) and is blocked by its own
PRED bits in every layer.  The scenes have no ground points, so the planner's `unknown` is 0: unknown ground is passable.  The goal is
the middle cell; layers = 32 (4 at 8192 x 8192, where layers nx nz may not exceed 2^28), wait = 100.  One repetition is timed with the
host clock around whole calls, which return after their last stream wait.  Cases:

  sweep   the sweep alone, on cached static planes: svh_grid_set_time with the other wait (TPOT is stale, RCOST and RPOT are not) and
          svh_grid_get_time_plane(TPOT, all layers) into a device buffer: k_grid_time_last, the launches of k_grid_time_sweep, the
          readback of the statistics and the copy of the layers.  (The records of case "forms" in the profile are this case for the
          time-blocked form and for the plain form, one launch per layer, alternating in one process, before the plain form was
          deleted.)
  host    svh_grid_add_points of one point, svh_grid_objects_step, svh_grid_plan_set_goals and svh_grid_get_time_plane(TPOT) into a
          device buffer -- everything from the cost map up --, against what a caller must do without the layer: the same add and step,
          then the ID plane, the track table, COST, FLAGS, CLASS and PRED to the host and the header's own loops there
          (svh_test_grid_time).  Before anything is timed TPOT, TDIR, RCOST and RPOT of the two sides are compared.

The sides alternate repetition by repetition in one process, the order reversed every other time.  Per case 3 warm-up and 20 timed
repetitions (1 and 3 where one repetition takes more than a second; the host side of 8192 x 8192 is run once, which is also its
comparison): median, 10th and 90th percentile in ms, and the paired difference with its 10th and 90th percentile.  One JSON line per
case goes to profiles/grid_time_times.jsonl.  There is no threshold: this is a measurement.

    python tools/gpu_grid_time.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED] [--tag TEXT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_grid_obj import DENSITIES, Dev, points_of   # noqa: E402
from gpu_grid_plan import CELL, PIECE, paired, pct, summary   # noqa: E402


def main():
    out = os.path.join(ROOT, "profiles", "grid_time_times.jsonl")
    sizes, warmup, timed, tag = [256, 1024, 8192], 3, 20, ""
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
    L_ = G._bind()
    hip = C.CDLL("libamdhip64.so")
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 1.5]], np.float64)      # a camera 1.5 above the road: h = 1.5 - y
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    k = C.c_int32(0)
    tile = L_.svh_test_grid_time_tile(C.byref(k))

    def emit(rec):
        line = json.dumps(dict(dict(version=svhip.lib().svh_version().decode(), tag=tag, tile=tile, k=k.value), **rec))
        print(line, flush=True)
        with open(out, "a") as f:                                                    # line by line: a run cut short keeps what it measured
            f.write(line + "\n")

    for n in sizes:
        layers = 32 if n <= 1024 else 4
        for density in DENSITIES:
            rng = np.random.default_rng(n)
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            g.set_objects(G.default_obj(max_tracks=4096))
            pred = G.default_pred(only_moving=0)
            g.set_predict(pred)
            g.set_plan(unknown=0)
            cells = np.flatnonzero(rng.random(n * n) < density)
            for at in range(0, len(cells), PIECE):
                g.add_points(points_of(cells[at:at + PIECE], n, 1.0))
            for _ in range(3):
                g.objects_step(0)
            goal = np.array([(n // 2, n // 2)], np.int32)
            g.set_goals(goal)
            g.set_time(layers=layers, wait=100, release=1)
            plan, tp, trav = g.plan_params(), g.time_params(), g.traversability()[0]
            dev = Dev(hip, nbytes=4 * layers * n * n)
            slow = n > 1024
            common = dict(size=n, density=density, layers=layers, track_stats=list(g.track_stats()))

            # ---- case "sweep": the field alone, the static planes cached -------------------------------------------------------------
            flip = [100]

            def sweep():
                flip[0] = 201 - flip[0]                # 100, 101, 100, ...: the field is stale, the static planes are not
                t0 = time.perf_counter()
                g.set_time(wait=flip[0])
                g.time_plane(G.TIME_TPOT, device_ptr=dev.p.value)
                return (time.perf_counter() - t0) * 1e3
            ms = paired({"sweep": sweep}, *((1, 5) if slow else (warmup, timed)))
            g.set_time(wait=100)
            rec = dict(common, case="sweep", time_stats=list(g.time_stats()), reps=len(ms["sweep"]))
            rec.update(summary("sweep", ms["sweep"]))
            rec["sweep_ns_per_state"] = round(pct(ms["sweep"], 50) * 1e6 / (layers * n * n), 3)
            emit(rec)

            # ---- case "host": the whole chain against the caller's host round trip --------------------------------------------------
            one = points_of(cells[len(cells) // 2:len(cells) // 2 + 1], n, 1.0)
            last = {}

            def device_step():
                t0 = time.perf_counter()
                g.add_points(one)
                g.objects_step(0)
                g.set_goals(goal)
                g.time_plane(G.TIME_TPOT, device_ptr=dev.p.value)
                return (time.perf_counter() - t0) * 1e3

            def host_step():
                t0 = time.perf_counter()
                g.add_points(one)
                g.objects_step(0)
                (ids, off), tracks, (plane, _) = g.track_plane(), g.tracks(), g.pred_plane()
                cost, flags, cls = g.trav_plane(G.TRAV_COST), g.trav_plane(G.TRAV_FLAGS), g.classes()
                last["host"] = G.core_time(plan, pred, tp, cost, flags, goal, plane, 0, 0, off, ids, tracks, cls, trav, CELL)
                return (time.perf_counter() - t0) * 1e3
            t_host = host_step()
            device_step()                                                             # one more point in one cell: the same objects and tracks
            for which, name in ((G.TIME_TPOT, "tpot"), (G.TIME_TDIR, "tdir"), (G.TIME_RCOST, "rcost"), (G.TIME_RPOT, "rpot")):
                assert np.array_equal(g.time_plane(which), last["host"][name]), (n, density, name)
            assert g.time_stats()[:5] == last["host"]["stats"][:5], (n, density)
            last.clear()
            if slow:
                ms = {"device": [device_step() for _ in range(5)], "host": [t_host]}
            else:
                ms = paired({"device": device_step, "host": host_step}, *((1, 3) if t_host > 1000.0 else (warmup, timed)))
            rec = dict(common, case="host", time_stats=list(g.time_stats()), pred_stats=list(g.pred_stats()), reps=[len(ms["device"]), len(ms["host"])])
            for name, v in ms.items():
                rec.update(summary(name, v))
            if not slow:
                rec.update(summary("host_minus_device", [x - y for x, y in zip(ms["host"], ms["device"])]))
            emit(rec)
            dev.free()
            g.close()


if __name__ == "__main__":
    main()
