#!/usr/bin/env python3
"""Time the prediction of the ground grid (svh_grid_roll_score_pred, include/svh_grid_pred.h, "PREDICTION") on the device.

Scenes are those of tools/gpu_grid_obj.py: windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m, a seeded random field of
obstacle cells at a density of 0.01 and of 0.3, one point 1 m high per obstacle cell, min_points 1, the object parameters the
defaults but max_tracks 4096, three steps taken.  The field stands, so only_moving is 0: every track with a label predicts, all
slots of a track onto its own cells (the scatter's cheapest case: one atomic per cell); the other prediction parameters are the
defaults.  The vehicle is the default car with w_pot 0 (no field is planned) and unknown_cost 0 (the scenes have no ground points:
an arc runs until it meets an obstacle), the candidates a fan of arcs, curvatures within +-0.03 per metre, straight ahead from the
middle of the window.  One repetition is timed with the host clock around whole calls, which return after their last stream wait.  Cases:

  score   svh_grid_roll_score_pred against svh_grid_roll_score, both on cached planes (COST and PRED are valid), at K x T = 64 x 16
          and 1024 x 64 poses on a window of 1024 x 1024 cells whose obstacles (density 0.3) all lie behind the vehicle: every arc
          runs to its end, so both kernels gather under every footprint cell of every pose: the price of the second gather.
  host    svh_grid_add_points of one point, svh_grid_objects_step and svh_grid_roll_score_pred (64 x 16), against what a caller must do
          without the layer: the same add and step, then the ID plane, the track table and COST to the host and the header's own host
          loops there (svh_test_grid_pred, svh_test_grid_pred_roll).  Before anything is timed PRED, the records, the scores and the
          best of the two sides are compared.
  local   a local step -- svh_grid_follow by one cell, svh_grid_add_points_from of a frame of at most 65536 of the scene's points that
          lies on the device, svh_grid_render_local into a device image, svh_grid_objects_step -- followed by svh_grid_roll_score
          (WITHOUT) or by svh_grid_roll_score_pred (WITH), 64 x 16: what the layer adds per frame.

The sides alternate repetition by repetition in one process, the order reversed every other time.  Per case 3 warm-up and 20 timed
repetitions (1 and 5 at 8192 x 8192 or where one repetition takes more than a second): median, 10th and 90th percentile in ms, and
the paired difference with its 10th and 90th percentile.  One JSON line per case goes to profiles/grid_pred_times.jsonl.  There is
no threshold: this is a measurement.

    python tools/gpu_grid_pred.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED] [--tag TEXT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_grid_obj import DENSITIES, FRAME_POINTS, Dev, points_of   # noqa: E402
from gpu_grid_plan import CELL, PIECE, paired, summary   # noqa: E402

SHAPES = ((64, 16), (1024, 64))


def fan(G, K, T):
    """one set of K arcs of T poses, straight ahead (heading 16 of 64) and to both sides"""
    return G.arc_candidates(CELL, 8, np.linspace(-0.03, 0.03, K), 0.5, T)[16:17].copy()


def score_case(G, emit, frame, cells, roll, pred, reps, n=1024):
    """case "score": the obstacles `cells` lie behind the vehicle, which stands in the middle and looks along +b"""
    g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
    g.set_objects(G.default_obj(max_tracks=4096))
    g.set_roll(roll)
    g.set_predict(pred)
    g.add_points(points_of(cells, n, 1.0))
    for _ in range(3):
        g.objects_step(0)
    middle = [(n // 2 + 0.5) * CELL, 0.0, (n // 2 + 0.5) * CELL]
    for K, T in SHAPES:
        g.set_candidates(fan(G, K, T))
        plain, with_pred = g.roll_score(middle, 0), g.roll_score_pred(middle, 0)
        assert plain[0] == with_pred[0] and np.array_equal(plain[1], with_pred[1][:, :5]) and np.array_equal(plain[2], with_pred[2])

        def score(entry):
            def run():
                t0 = time.perf_counter()
                entry(middle, 0)
                return (time.perf_counter() - t0) * 1e3
            return run
        ms = paired({"roll_score": score(g.roll_score), "roll_score_pred": score(g.roll_score_pred)}, *reps)
        rec = dict(case="score", size=n, density="0.3 behind the vehicle", K=K, T=T, pred_params=pred.asdict(),
                   footprint_cells_longest=int(max(len(g.roll_footprint(k)) for k in range(64))), poses_scored=int(plain[1][:, 0].sum()),
                   pred_stats=list(g.pred_stats()), track_stats=list(g.track_stats()), reps=len(ms["roll_score"]))
        for name, v in ms.items():
            rec.update(summary(name, v))
        rec.update(summary("pred_minus_plain", [x - y for x, y in zip(ms["roll_score_pred"], ms["roll_score"])]))
        emit(rec)
    g.close()


def main():
    out = os.path.join(ROOT, "profiles", "grid_pred_times.jsonl")
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
    G._bind()
    hip = C.CDLL("libamdhip64.so")
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 1.5]], np.float64)      # a camera 1.5 above the road: h = 1.5 - y
    os.makedirs(os.path.dirname(out), exist_ok=True)

    def emit(rec):
        rec = dict(dict(version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:                                                    # line by line: a run cut short keeps what it measured
            f.write(line + "\n")

    for n in sizes:
        for density in DENSITIES:
            rng = np.random.default_rng(n)
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            g.set_objects(G.default_obj(max_tracks=4096))
            roll, pred = G.default_roll(w_pot=0, unknown_cost=0), G.default_pred(only_moving=0)
            g.set_roll(roll)
            g.set_predict(pred)
            cells = np.flatnonzero(rng.random(n * n) < density)
            if n == 1024 and density == DENSITIES[-1]:
                score_case(G, emit, frame, cells[cells // n < n // 2 - 40], roll, pred, (warmup, timed))
            for at in range(0, len(cells), PIECE):
                g.add_points(points_of(cells[at:at + PIECE], n, 1.0))
            for _ in range(3):
                g.objects_step(0)
            slow = n > 1024
            reps = (1, 5) if slow else (warmup, timed)
            middle = [(n // 2 + 0.5) * CELL, 0.0, (n // 2 + 0.5) * CELL]
            anchor = g.cell_of(middle)
            common = dict(size=n, density=density, pred_params=pred.asdict(), track_stats=list(g.track_stats()))

            # ---- case "host": a step and a scoring against the caller's host round trip -----------------------------------------
            K, T = SHAPES[0]
            tab = fan(G, K, T)
            g.set_candidates(tab)
            one = points_of(cells[len(cells) // 2:len(cells) // 2 + 1], n, 1.0)
            last = {}

            def device_step():
                t0 = time.perf_counter()
                g.add_points(one)
                g.objects_step(0)
                last["device"] = g.roll_score_pred(middle, 0)
                return (time.perf_counter() - t0) * 1e3

            def host_step():
                t0 = time.perf_counter()
                g.add_points(one)
                g.objects_step(0)
                (ids, off), tracks, cost = g.track_plane(), g.tracks(), g.trav_plane(G.TRAV_COST)
                plane, _ = G.core_pred(pred, ids, tracks)
                r = G.core_pred_roll(roll, pred, CELL, cost, plane, table=tab, anchor=anchor, oa=0, ob=0, pred_off=off)
                last["host"], last["plane"] = (r["best"], r["recs"], r["scores"]), plane
                return (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            host_step()
            slow = slow or time.perf_counter() - t0 > 1.0
            reps = (1, 5) if slow else reps
            device_step()                                                             # one more point in one cell: the same objects and tracks
            assert np.array_equal(g.pred_plane()[0], last["plane"]), (n, density, "PRED")
            assert last["device"][0] == last["host"][0] and all(np.array_equal(a, b) for a, b in zip(last["device"][1:], last["host"][1:])), (n, density)
            ms = paired({"device": device_step, "host": host_step}, *reps)
            rec = dict(common, case="host", K=K, T=T, pred_stats=list(g.pred_stats()), object_stats=list(g.object_stats()), reps=len(ms["device"]))
            for name, v in ms.items():
                rec.update(summary(name, v))
            rec.update(summary("host_minus_device", [x - y for x, y in zip(ms["host"], ms["device"])]))
            emit(rec)

            # ---- case "local": what the layer adds to a local step with objects ----------------------------------------------------
            pick = rng.choice(cells, min(FRAME_POINTS, len(cells)), replace=False)
            pts = Dev(hip, points_of(pick, n, 1.0))
            image = Dev(hip, nbytes=3 * n * n)
            at = dict(k=0)

            def local(with_pred):
                def run():
                    at["k"] += 1
                    pos = [(n // 2 + 0.5) * CELL, 0.0, (n // 2 + at["k"] + 0.5) * CELL]      # the camera, one cell further along b
                    t0 = time.perf_counter()
                    g.follow(pos, n // 2, n // 2)
                    g.add_points_device_from(pts.p.value, len(pick), pos)
                    g.render_local(device_ptr=image.p.value)
                    g.objects_step(0)
                    (g.roll_score_pred if with_pred else g.roll_score)(pos, 0)
                    return (time.perf_counter() - t0) * 1e3
                return run
            ms = paired({"without": local(False), "with": local(True)}, *reps)
            rec = dict(common, case="local", K=K, T=T, frame_points=len(pick), pred_stats=list(g.pred_stats()), track_stats=list(g.track_stats()),
                       reps=len(ms["with"]))
            for name, v in ms.items():
                rec.update(summary(name, v))
            rec.update(summary("with_minus_without", [x - y for x, y in zip(ms["with"], ms["without"])]))
            emit(rec)
            pts.free()
            image.free()
            g.close()


if __name__ == "__main__":
    main()
