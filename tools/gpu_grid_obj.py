#!/usr/bin/env python3
"""Time the objects of the ground grid and their tracks (svh_grid_objects_step, include/svh_grid_obj.h, "OBJECTS") on the device.

Scenes, on windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m: a seeded random field of obstacle cells at a density of
0.01 (mostly single cells: few components reach min_size) and of 0.3 (below the percolation threshold of the 8-neighbourhood: many
components of every size, some above max_size), one point 1 m high per obstacle cell, min_points 1; the object parameters are the
defaults but max_tracks 4096.  One repetition of a side is timed with the host clock around whole calls, which return after
their last stream wait.  Two cases per scene:

  local   a local step -- svh_grid_follow by one cell, svh_grid_add_points_from of a frame of at most 65536 of the scene's points
          that lies on the device, svh_grid_render_local into a device image -- WITHOUT and WITH svh_grid_objects_step after it:
          what tracking adds to a step.  The add makes the objects stale, so every step computes them (14 launches, two waits)
          and then steps the tracks (7 launches, one wait).
  host    svh_grid_add_points of one point (the objects are stale), then svh_grid_objects_step, against what a caller did before:
          the same add, STATE, HMAX and COUNT to the host, and the header's own host form there (svh_test_grid_obj, then
          svh_test_grid_obj_step on the ID plane and the track table the caller keeps).  Before anything is timed the two
          object tables, the two track tables and ASSIGN are compared.

The sides alternate repetition by repetition in one process, the order reversed every other time.  Per case 3 warm-up and 20 timed
repetitions (1 and 5 where one repetition takes more than a second or the window has more than 1024 x 1024 cells): median, 10th and
90th percentile in ms, and the paired difference with its 10th and 90th percentile.  One JSON line per case goes to
profiles/grid_obj_times.jsonl with the statistics of the objects and of the last step.  There is no threshold: this is a measurement.

    python tools/gpu_grid_obj.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED] [--tag TEXT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_grid_plan import CELL, PIECE, paired, summary   # noqa: E402

FRAME_POINTS = 65536
DENSITIES = (0.01, 0.3)


class Dev:
    """device memory through the HIP runtime the library links"""

    def __init__(self, hip, host=None, nbytes=0):
        self.hip, self.p = hip, C.c_void_p()
        nbytes = host.nbytes if host is not None else nbytes
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(nbytes, 16))) == 0
        if host is not None and host.nbytes:
            assert hip.hipMemcpy(self.p, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), 1) == 0

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = C.c_void_p()


def points_of(cells, n, height):
    p = np.zeros((len(cells), 4), np.float32)
    p[:, 0], p[:, 2] = (cells % n + 0.5) * CELL, (cells // n + 0.5) * CELL
    p[:, 1], p[:, 3] = 1.5 - height, 0.5
    return p


def main():
    out = os.path.join(ROOT, "profiles", "grid_obj_times.jsonl")
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
    L = G._bind()
    hip = C.CDLL("libamdhip64.so")
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 1.5]], np.float64)      # a camera 1.5 above the road: h = 1.5 - y
    lines = []

    def emit(rec):
        rec = dict(dict(tile=G.FRONT_TILE, version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in sizes:
        for density in DENSITIES:
            rng = np.random.default_rng(n)
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            obj = G.default_obj(max_tracks=4096)
            g.set_objects(obj)
            cells = np.flatnonzero(rng.random(n * n) < density)
            for at in range(0, len(cells), PIECE):
                g.add_points(points_of(cells[at:at + PIECE], n, 1.0))
            stats = g.object_stats()
            slow = n > 1024
            reps = (1, 5) if slow else (warmup, timed)

            # ---- case "host": the step against the caller's host round trip ---------------------------------------------------
            one = points_of(cells[len(cells) // 2:len(cells) // 2 + 1], n, 1.0)
            cap = max(stats[2], 1)
            host = dict(tracks=np.zeros((0, G.TRACK_RECORD), np.int32), ids=None, next=0)
            last = {}

            def device_step():
                t0 = time.perf_counter()
                g.add_points(one)
                last["assign"] = g.objects_step(cap)
                return (time.perf_counter() - t0) * 1e3

            def host_step():
                t0 = time.perf_counter()
                g.add_points(one)
                state, hmax, count = g.local_plane(G.LOCAL_STATE), g.plane(G.HMAX), g.plane(G.COUNT)
                flags, label, recs, st = G.core_obj(obj, state, hmax, count)
                tracks, assign, ids, ts, nxt = G.core_obj_step(obj, recs, label, (0, 0), host["ids"], (0, 0),
                                                               host["tracks"] if host["ids"] is not None else host["tracks"][:0], host["next"])
                host.update(tracks=tracks, ids=ids, next=nxt, recs=recs, assign=assign)
                return (time.perf_counter() - t0) * 1e3
            # the two sides once, compared, before anything is timed; both have then taken one step
            t0 = time.perf_counter()
            host_step()
            slow = slow or time.perf_counter() - t0 > 1.0
            reps = (1, 5) if slow else reps
            assert np.array_equal(g.objects(), host["recs"]), (n, density)          # the same state: the device's table is the host's
            device_step()                                                             # one more point in one cell: the same objects
            assert np.array_equal(g.tracks(), host["tracks"]) and np.array_equal(last["assign"], host["assign"]), (n, density)
            ms = paired({"device": device_step, "host": host_step}, *reps)
            assert np.array_equal(g.tracks(), host["tracks"]), (n, density, "after the timed steps")
            rec = dict(case="host", size=n, density=density, object_cells=stats[0], components=stats[1], kept=stats[2], kept_cells=stats[3],
                       large=stats[4], low=stats[5], launches=stats[6], track_stats=list(g.track_stats()), reps=len(ms["device"]))
            for name, v in ms.items():
                rec.update(summary(name, v))
            rec.update(summary("host_minus_device", [x - y for x, y in zip(ms["host"], ms["device"])]))
            emit(rec)

            # ---- case "local": what the step adds to a local step ---------------------------------------------------------------
            g.objects_reset()
            pick = rng.choice(cells, min(FRAME_POINTS, len(cells)), replace=False)
            pts = Dev(hip, points_of(pick, n, 1.0))
            image = Dev(hip, nbytes=3 * n * n)
            at = dict(k=0)

            def local(track):
                def run():
                    at["k"] += 1
                    pos = [(n // 2 + 0.5) * CELL, 0.0, (n // 2 + at["k"] + 0.5) * CELL]      # the camera, one cell further along b
                    t0 = time.perf_counter()
                    g.follow(pos, n // 2, n // 2)
                    g.add_points_device_from(pts.p.value, len(pick), pos)
                    g.render_local(device_ptr=image.p.value)
                    if track:
                        g.objects_step(0)
                    return (time.perf_counter() - t0) * 1e3
                return run
            ms = paired({"without": local(False), "with": local(True)}, *reps)
            rec = dict(case="local", size=n, density=density, frame_points=len(pick), object_stats=list(g.object_stats()),
                       track_stats=list(g.track_stats()), reps=len(ms["with"]))
            for name, v in ms.items():
                rec.update(summary(name, v))
            rec.update(summary("with_minus_without", [x - y for x, y in zip(ms["with"], ms["without"])]))
            emit(rec)
            pts.free()
            image.free()
            g.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
