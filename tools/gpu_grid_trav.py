#!/usr/bin/env python3
"""Time the traversability layer of the ground grid (svh_grid_get_trav, include/svh_grid.h) on the device.

Cases: windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m, an inflation radius of 8 cells (1.5 m, the
default) and of 64 cells (12.7 m), and about 1 and 30 lethal cells in 100.  The grid is filled once per window and
density from seeded points, one per cell, min_points 1: a cell is an obstacle (one point a metre up) with the given
probability, free (one point within 0.1 m of the road; max_slope is 2, so the slope stencil has work and finds nothing)
with probability 0.5, and unknown otherwise.

One repetition adds one point -- which makes the cached planes stale -- and then times, with the host clock, one whole
svh_grid_get_trav(COST) into a device buffer: the entry returns after its last stream wait, so the interval holds
k_grid_finalise, k_grid_trav_mask, k_grid_dist_cols, k_grid_dist_rows and the copy of the plane.  Beside it, alternating
repetition by repetition in one process: the same add followed by svh_grid_get(CLASS) into a device buffer (k_grid_finalise
and the copy of a plane of the same size: what the layer adds is the difference), and a second svh_grid_get_trav without an
add (the cache: the copy alone).  If the library has the switch svh_test_grid_cols_chunk, the two forms of k_grid_dist_cols
(plain: one lane sweeps a whole column; chunks: one lane per column and 256 rows, started `reach` rows early) alternate
too, and the paired saving plain - chunks is reported; without the switch the one form the library has is timed.

For comparison -- nothing else exists to compare with -- the same process times the local step the grid had before this
layer: svh_grid_follow by one cell, svh_grid_add_view_lists_from of the newest fused urban list, svh_grid_render_local, on
256 x 256 cells (as tools/gpu_grid.py --local does).

Per case 5 warm-up and 20 timed repetitions: median, 10th and 90th percentile in ms.  One JSON line per case goes to
profiles/grid_trav_times.jsonl.  There is no threshold: this is a measurement.  The split over the kernels is not
measured here; a kernel trace of this program gives it.

    python tools/gpu_grid_trav.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CELL = 0.2
REACHES = ((8, 1.5), (64, 12.7))
DENSITIES = (0.01, 0.3)
PIECE = 1 << 22


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


def fill(g, n, density, seed):
    """one point in the centre of most cells of an n x n window, row block by row block; returns (lethal, free) cells"""
    rng = np.random.default_rng(seed)
    lethal = free = 0
    rows = max(1, PIECE // n)
    ia = np.arange(n, dtype=np.float32)[None, :]
    for b0 in range(0, n, rows):
        b1 = min(n, b0 + rows)
        u = rng.random((b1 - b0, n), dtype=np.float32)
        obstacle, level = u < density, (u >= density) & (u < density + 0.5)
        keep = obstacle | level
        pts = np.zeros((int(keep.sum()), 4), np.float32)
        ib = np.arange(b0, b1, dtype=np.float32)[:, None]
        pts[:, 0] = np.broadcast_to((ia + 0.5) * CELL - 0.5 * n * CELL, keep.shape)[keep]
        pts[:, 2] = np.broadcast_to((ib + 0.5) * CELL, keep.shape)[keep]
        h = np.where(obstacle, 1.0, rng.uniform(-0.1, 0.1, keep.shape)).astype(np.float32)
        pts[:, 1] = 1.65 - h[keep]                               # the default frame: a level camera 1.65 m above the road
        pts[:, 3] = 0.5
        g.add_points(pts)
        lethal += int(obstacle.sum())
        free += int(level.sum())
    return lethal, free


def main():
    import svhip
    from svhip import grid, view
    import gpu_view
    out = os.path.join(ROOT, "profiles", "grid_trav_times.jsonl")
    sizes, warmup, timed = (256, 1024, 8192), 5, 20
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a == "--out":
            out = args.pop(0)
        elif a == "--sizes":
            sizes = tuple(int(v) for v in args.pop(0).split(","))
        elif a == "--reps":
            warmup, timed = (int(v) for v in args.pop(0).split(","))
        else:
            raise SystemExit(__doc__)
    if svhip.device_count() < 1:
        raise SystemExit("gpu_grid_trav needs a GPU: libsvhip has no CPU fallback")
    hip = C.CDLL("libamdhip64.so")
    L = svhip.lib()
    grid._bind()
    set_chunk = None
    if hasattr(L, "svh_test_grid_cols_chunk"):
        L.svh_test_grid_cols_chunk.argtypes = [C.c_int32]
        L.svh_test_grid_cols_chunk.restype = None
        set_chunk = L.svh_test_grid_cols_chunk
    build = L.svh_version().decode()
    lines = []

    def emit(rec):
        rec.update(warmup=warmup, timed=timed, build=build,
                   timed_with="host clock around the entries named; every entry returns after its last wait")
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    one = np.array([[0.05, 1.65, 0.1, 0.5]], np.float32)         # a point on the road in front of the camera
    for n in sizes:
        dev = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), C.c_size_t(n * n)) == 0
        for density in DENSITIES:
            g = grid.Grid(grid.default_params(nx=n, nz=n, cell=CELL, x0=-0.5 * n * CELL, z0=0.0, min_points=1))
            lethal, free = fill(g, n, density, seed=n + int(1000 * density))
            for reach, inflate in REACHES:
                g.set_traversability(inflate=inflate, max_slope=2.0)
                assert g.traversability()[1] == reach

                def trav(chunk=None):
                    if chunk is not None:
                        set_chunk(chunk)
                    g.add_points(one)
                    t0 = time.perf_counter()
                    g.trav_plane(grid.TRAV_COST, device_ptr=dev.value)
                    return (time.perf_counter() - t0) * 1e3

                def finalise_only():
                    g.add_points(one)
                    t0 = time.perf_counter()
                    g.plane(grid.CLASS, device_ptr=dev.value)
                    return (time.perf_counter() - t0) * 1e3

                def cached():
                    g.trav_plane(grid.TRAV_COST, device_ptr=dev.value)
                    t0 = time.perf_counter()
                    g.trav_plane(grid.TRAV_COST, device_ptr=dev.value)
                    return (time.perf_counter() - t0) * 1e3

                sides = {"plain": lambda: trav(1 << 20), "chunks": lambda: trav(256)} if set_chunk else {"get_trav": trav}
                sides["finalise_and_copy"] = finalise_only
                sides["cached"] = cached
                ms = paired(sides, warmup, timed)
                if set_chunk:
                    set_chunk(0)
                flags = g.trav_plane(grid.TRAV_FLAGS)
                rec = {"leg": "get_trav_cost", "nx": n, "nz": n, "cell": CELL, "reach": reach, "inflate": inflate, "density": density,
                       "lethal_cells": int(((flags & 2) != 0).sum()), "steep_cells": int((flags & 1).sum()), "obstacle_cells": lethal,
                       "free_cells": free}
                for name, t in ms.items():
                    rec.update(summary(name, t))
                if set_chunk:
                    rec.update(summary("saving_plain_minus_chunks", [a - b for a, b in zip(ms["plain"], ms["chunks"])]))
                best = "chunks" if set_chunk else "get_trav"
                rec.update(summary("layer_%s_minus_finalise_and_copy" % best, [a - b for a, b in zip(ms[best], ms["finalise_and_copy"])]))
                emit(rec)
            g.close()
        hip.hipFree(dev)
    # the local step of the grid as it was before this layer, 256 x 256
    urban = gpu_view.urban_view(view, (64, 48))
    newest = urban.points(urban.count(view.LISTS) - 1)
    v = view.View(64, 48)
    v.add_points([newest])
    rgb = C.c_void_p()
    assert hip.hipMalloc(C.byref(rgb), C.c_size_t(256 * 256 * 3)) == 0
    local = grid.Grid(grid.default_params(nx=256, nz=256, cell=CELL, x0=-25.6, z0=0.0))
    state = {"k": 0}

    def local_step():
        state["k"] += 1
        centre = [0.0, 0.0, 0.1 + CELL * (state["k"] % 2)]       # one cell forward and back: a strip enters every time
        t0 = time.perf_counter()
        local.follow(centre, 128, 0)
        local.add_view_lists_from(v, 0, 1, centre)
        local.render_local(device_ptr=rgb.value)
        return (time.perf_counter() - t0) * 1e3

    def local_step_and_cost():
        t = local_step()
        t0 = time.perf_counter()
        local.render_cost(device_ptr=rgb.value)
        return t + (time.perf_counter() - t0) * 1e3

    ms = paired({"local_step": local_step, "local_step_and_render_cost": local_step_and_cost}, warmup, timed)
    rec = {"leg": "local_step", "newest_list_points": len(newest), "nx": 256, "nz": 256, "cell": CELL, "reach": local.traversability()[1]}
    for name, t in ms.items():
        rec.update(summary(name, t))
    emit(rec)
    hip.hipFree(rgb)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
