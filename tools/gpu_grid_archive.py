#!/usr/bin/env python3
"""Time the ground grid's archive (svh_grid_set_archive, svh_grid_get_region, include/svh_grid_archive.h) against the grid without it.

Every repetition is a whole call or a whole local step, timed with the host clock; the sides of a leg alternate repetition by
repetition in one process, the order reversed every other repetition, and the paired difference against the first side is given with
its 10th and 90th percentile (the scheme of tools/gpu_grid_dyn.py).  Windows of n x n cells of 0.2 m.

    local_step   svh_grid_follow by one cell (forward and back: a strip of n cells leaves and one enters every time), 65 536 points
                 from device memory through svh_grid_add_points_from, svh_grid_render_local into a device buffer.  Sides: `off`, a
                 grid without the layer -- the yardstick, the step of tools/gpu_grid_dyn.py's `add`; `on_empty`, the layer on and
                 svh_grid_archive_clear before every step, outside the clock: no entering cell finds a page, every leaving tile
                 claims one, and the lazy refill of the table (two fills and one launch) falls into the step; `on_restore`, the
                 layer on and left alone: after the first cycle every entering cell is restored from a page.  256 and 1024; 8192 with
                 fewer repetitions.
    jump         svh_grid_scroll by the whole window, there and back, one call per repetition, the window holding a point in every
                 cell: `off` refills the planes, `on` stores n x n cells and restores as many.  256 and 1024.
    region       svh_grid_get_region of CLASS over a box of n x n global cells into a device buffer, half of it the window and half
                 archived tiles (at 8192 the box lies round a window of 1024 x 1024 and its archived half, the rest has no tile),
                 against svh_grid_get of CLASS on a window of n x n that is current (`get_cached`: a copy) and on one an add made
                 stale (`get_stale`: finalise and copy).

One JSON line per case goes to profiles/grid_archive_times.jsonl.  There is no threshold: this is a measurement.

    python tools/gpu_grid_archive.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_grid_dyn import CELL, all_cells, paired, summary   # noqa: E402

POINTS = 65536
BIG = 8192


def frame_points(n, seed):
    """65 536 points over the middle of an n x n window whose low corner is (-n / 2 cells, 0), one in ten a metre high"""
    rng = np.random.default_rng(seed)
    pts = np.zeros((POINTS, 4), np.float32)
    pts[:, 0] = rng.uniform(-0.4 * n * CELL, 0.4 * n * CELL, POINTS)
    pts[:, 2] = rng.uniform(2 * CELL, 0.8 * n * CELL, POINTS)
    pts[:, 1] = 1.65 - np.where(rng.random(POINTS) < 0.1, 1.0, rng.uniform(-0.05, 0.05, POINTS))
    pts[:, 3] = 0.5
    return pts


class DevArray:
    def __init__(self, hip, host=None, nbytes=0):
        self.hip, self.p = hip, C.c_void_p()
        nbytes = host.nbytes if host is not None else nbytes
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(nbytes, 16))) == 0
        if host is not None:
            assert hip.hipMemcpy(self.p, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), 1) == 0

    def free(self):
        self.hip.hipFree(self.p)


def record(leg, n, ms, first, extra):
    rec = dict(leg=leg, nx=n, nz=n, cell=CELL, **extra)
    for name, t in ms.items():
        rec.update(summary(name, t))
        if name != first:
            rec.update(summary("%s_minus_%s" % (name, first), [a - b for a, b in zip(t, ms[first])]))
    print(json.dumps(rec), flush=True)
    return json.dumps(rec)


def main():
    import svhip
    from svhip import grid
    out = os.path.join(ROOT, "profiles", "grid_archive_times.jsonl")
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
        raise SystemExit("gpu_grid_archive needs a GPU: libsvhip has no CPU fallback")
    hip = C.CDLL("libamdhip64.so")
    grid._bind()
    build = svhip.lib().svh_version().decode()
    common = dict(warmup=warmup, timed=timed, build=build)
    lines = []

    def params(n):
        return grid.default_params(nx=n, nz=n, cell=CELL, x0=-0.5 * n * CELL, z0=0.0)

    for n in sizes:
        w, t = (warmup, timed) if n < BIG else (1, 3)
        # ---- a local step ----
        rgb, pts = DevArray(hip, nbytes=n * n * 3), DevArray(hip, frame_points(n, n))
        grids = {"off": grid.Grid(params(n)), "on_empty": grid.Grid(params(n)), "on_restore": grid.Grid(params(n))}
        grids["on_empty"].set_archive(grid.default_archive())
        grids["on_restore"].set_archive(grid.default_archive())
        state = {"k": 0}

        def step(name):
            g = grids[name]
            state["k"] += 1
            centre = [0.0, 0.0, 0.1 + CELL * (((state["k"] - 1) // len(grids)) % 2)]   # one cell forward and back, the same for the sides of a repetition
            if name == "on_empty":
                g.archive_clear()
            t0 = time.perf_counter()
            g.follow(centre, n // 2, 0)
            g.add_points_device_from(pts.p.value, POINTS, centre)
            g.render_local(device_ptr=rgb.p.value)
            return (time.perf_counter() - t0) * 1e3

        ms = paired({name: (lambda name=name: step(name)) for name in grids}, w, t)
        lines.append(record("local_step", n, ms, "off", dict(common, warmup=w, timed=t, points=POINTS, max_tiles=grid.ARCHIVE_DEFAULT_TILES,
                                                             archive_on_restore=grids["on_restore"].archive_stats(),
                                                             timed_with="host clock around follow, add_points_from, render_local; every entry returns after its last wait")))
        for g in grids.values():
            g.close()
        rgb.free(), pts.free()
        if n >= BIG:
            continue
        # ---- a jump of the whole window ----
        full = DevArray(hip, all_cells(n, n))
        grids = {"off": grid.Grid(params(n)), "on": grid.Grid(params(n))}
        grids["on"].set_archive(grid.default_archive())
        for g in grids.values():
            g.add_points_device(full.p.value, n * n)
        state = {"k": 0}

        def jump(name):
            state["k"] += 1
            d = n if ((state["k"] - 1) // len(grids)) % 2 == 0 else -n
            t0 = time.perf_counter()
            grids[name].scroll(d, 0)
            return (time.perf_counter() - t0) * 1e3

        ms = paired({name: (lambda name=name: jump(name)) for name in grids}, warmup, timed)
        lines.append(record("jump", n, ms, "off", dict(common, cells=n * n, archive=grids["on"].archive_stats(), timed_with="host clock around svh_grid_scroll by (n, 0) or (-n, 0)")))
        for g in grids.values():
            g.close()
        full.free()

    # ---- a region ----
    for n in sizes:
        w, t = (warmup, timed) if n < BIG else (1, 3)
        m = min(n, 1024)
        full, some = DevArray(hip, all_cells(m, m)), DevArray(hip, frame_points(n, n))
        src, whole = grid.Grid(params(m)), grid.Grid(params(n))
        src.set_archive(grid.default_archive())
        src.add_points_device(full.p.value, m * m)
        src.scroll(m // 2, 0)                            # half of the old window is archived now
        oa, ob = src.window()
        whole.add_points_device(some.p.value, POINTS)
        dst = DevArray(hip, nbytes=n * n)
        ga0, gb0 = oa - m // 2 - (n - m) // 2, ob - (n - m) // 2

        def region():
            t0 = time.perf_counter()
            src.region(grid.CLASS, ga0, gb0, n, n, device_ptr=dst.p.value)
            return (time.perf_counter() - t0) * 1e3

        def get(stale):
            if stale:
                whole.add_points_device(some.p.value, 256)
            t0 = time.perf_counter()
            whole.plane(grid.CLASS, device_ptr=dst.p.value)
            return (time.perf_counter() - t0) * 1e3

        ms = paired({"get_cached": lambda: get(False), "get_stale": lambda: get(True), "region": region}, w, t)
        lines.append(record("region", n, ms, "get_cached", dict(common, warmup=w, timed=t, window=m, archive=src.archive_stats(),
                                                                timed_with="host clock around svh_grid_get_region / svh_grid_get of CLASS into a device buffer")))
        src.close(), whole.close()
        full.free(), some.free(), dst.free()

    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
