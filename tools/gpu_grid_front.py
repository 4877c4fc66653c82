#!/usr/bin/env python3
"""Time the frontiers of the ground grid (svh_grid_get_frontiers, include/svh_grid.h, "FRONTIERS") on the device.

Scenes, on windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m, filled once from seeded points, one per cell that
has any, min_points 1, an inflation radius of one cell and no obstacle (so the COST of a free cell is 0); a cell without a point
is unknown and was never looked at:
  rim      an open field, every cell free but a rim of two cells: one closed frontier round the window
  clutter  three cells in ten hold no point: many small components, most of them dropped (min_size 8)
  spiral   a corridor of one free cell wound inwards between walls of one cell without points: every cell of the corridor is a
           frontier cell, ONE component of half the window that crosses a tile border every FRONT_TILE cells -- the shape on
           which a labelling by propagation in rounds needs a round per cell

One repetition of a side is timed with the host clock around whole calls, which return after their last stream wait:
  device   svh_grid_add_points of one point (the cached planes are stale), then svh_grid_get_frontiers into a host table:
           k_grid_finalise, the three kernels of the cost map, the launches of the frontiers and the copy of the table
  host     what a caller did before: the same add, svh_grid_get_local(STATE) and svh_grid_get_trav(COST) to the host and the
           flood fill of csrc/grid_front_core.h on the host (svh_test_grid_front, the table alone)
The sides alternate repetition by repetition in one process, the order reversed every other time.  Before anything is timed
the two tables are compared.  Per case 3 warm-up and 20 timed repetitions (1 and 5 where one repetition takes more than a second
or the window has more than 1024 x 1024 cells): median, 10th and 90th percentile in ms, and the paired difference host - device
with its 10th and 90th percentile.  One JSON line per case goes to profiles/grid_front_times.jsonl with the tile side, the
statistics and the launches of a computation.  There is no threshold: this is a measurement.

    python tools/gpu_grid_front.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED] [--tag TEXT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_grid_plan import CELL, PIECE, paired, pct, summary   # noqa: E402


def spiral(n):
    """bool [n, n]: the corridor.  The rings of even depth, each cut one cell above its first corner and joined to the next ring
    through the wall beside the cut"""
    i = np.arange(n)
    depth = np.minimum(np.minimum(i[None, :], i[:, None]), np.minimum(n - 1 - i[None, :], n - 1 - i[:, None]))
    c = depth % 2 == 0
    for d in range(0, n // 2 - 2, 2):
        c[d + 1, d] = False
        c[d + 2, d + 1] = True
    return c


def filled(scene, n, rng):
    """bool [n, n]: the cells that hold a point"""
    if scene == "rim":
        f = np.zeros((n, n), bool)
        f[2:-2, 2:-2] = True
        return f
    if scene == "clutter":
        return rng.random((n, n)) >= 0.3
    return spiral(n)


def fill(g, has):
    """one point on the road in the middle of every cell of `has`"""
    n = has.shape[1]
    cells = np.flatnonzero(has.ravel())
    for at in range(0, len(cells), PIECE):
        i = cells[at:at + PIECE]
        p = np.zeros((len(i), 4), np.float32)
        p[:, 0], p[:, 2], p[:, 3] = (i % n + 0.5) * CELL, (i // n + 0.5) * CELL, 0.5
        g.add_points(p)


def main():
    out = os.path.join(ROOT, "profiles", "grid_front_times.jsonl")
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
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], np.float64)
    lines = []

    def emit(rec):
        rec = dict(dict(tile=G.FRONT_TILE, version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in sizes:
        for scene in ("rim", "clutter", "spiral"):
            rng = np.random.default_rng(n)
            g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1))
            g.set_traversability(max_slope=4.0, inscribed=0.5 * CELL, inflate=CELL, lethal=G.LETHAL_OBSTACLE)
            has = filled(scene, n, rng)
            fill(g, has)
            b, a = np.argwhere(has)[len(has) // 2]
            one = np.array([[(a + 0.5) * CELL, 0.0, (b + 0.5) * CELL, 0.5]], np.float32)     # a second point on a free cell
            front = g.frontier_params()
            stats = g.frontier_stats()
            cap = max(stats[2], 1)
            table, host_table = np.zeros((cap, G.FRONT_RECORD), np.int32), np.zeros((cap, G.FRONT_RECORD), np.int32)
            kept, host_stats = C.c_int64(-1), np.zeros(5, np.int64)

            def device():
                t0 = time.perf_counter()
                g.add_points(one)
                G._check(L.svh_grid_get_frontiers(g._h, table.ctypes.data, cap, C.addressof(kept)))
                return (time.perf_counter() - t0) * 1e3

            def host():
                t0 = time.perf_counter()
                g.add_points(one)
                state, cost = g.local_plane(G.LOCAL_STATE), g.trav_plane(G.TRAV_COST)
                G._check(L.svh_test_grid_front(C.byref(front), n, n, 0, 0, state.ctypes.data, cost.ctypes.data, None, None,
                                               host_table.ctypes.data, cap, C.addressof(kept), host_stats.ctypes.data))
                return (time.perf_counter() - t0) * 1e3
            # the device's table against the host's, once, before anything is timed
            t0 = time.perf_counter()
            host()
            slow = time.perf_counter() - t0 > 1.0 or n > 1024
            device()
            assert kept.value == stats[2] and np.array_equal(table, host_table) and tuple(int(v) for v in host_stats[:4]) == stats[:4], (n, scene)
            ms = paired({"device": device, "host": host}, 1 if slow else warmup, 5 if slow else timed)
            rec = dict(case="frontiers", size=n, scene=scene, frontier_cells=stats[0], components=stats[1], kept=stats[2], kept_cells=stats[3],
                       launches=stats[4], reps=len(ms["device"]))
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
