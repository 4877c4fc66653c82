#!/usr/bin/env python3
"""Time an observation of the ground grid's dynamics (svh_grid_observe_*, include/svh_grid.h "DYNAMICS") against the add it stands for.

One repetition is one whole local step, timed with the host clock: svh_grid_follow by one cell (a strip enters every time), the
frame's points from device memory with the camera as the origin, svh_grid_render_local into a device buffer.  Three sides alternate
repetition by repetition in one process, the order reversed every other repetition:

    add            the frame through svh_grid_add_view_lists_from / svh_grid_add_points_from, on a grid without the layer
    observe_body   the frame through svh_grid_observe_view_lists / svh_grid_observe_points; k_grid_sight reads the bodies from the layer's
                   plane, which k_grid_settle keeps
    observe_slot   the same, k_grid_sight reads count, kmin and kmax of the cell at its slot

The two observe sides share one grid and need the library's test switch svh_test_grid_dyn_form (int32 form: 0 body, 1 slot); the form
that lost was deleted with the switch (its run is profiles/grid_dyn_forms_ab.jsonl), and without it the one form the library has is
timed as `observe`.  Windows of 256 x 256, 1024 x 1024 and 8192 x 8192 cells of 0.2 m.  Scenes: `urban`, the newest list of the two
fused urban frames (a view's list); `all_cells`, one point in every cell of the window, one cell in ten a metre high (a device array;
256 and 1024 only: at 8192 x 8192 it is 67 million lines of up to 8192 steps).

Per case 5 warm-up and 20 timed repetitions: median, 10th and 90th percentile in ms of each side and of the paired differences observe -
add and slot - body.  One JSON line per case goes to profiles/grid_dyn_times.jsonl.  There is no threshold: this is a measurement.  The
split over the kernels (the settle's own time) is not measured here; a kernel trace of this program gives it.

    python tools/gpu_grid_dyn.py [--out FILE] [--sizes 256,1024,8192] [--reps WARMUP,TIMED]"""
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
ALL_CELLS_MAX = 1024


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


def all_cells(n, seed):
    """one point in the centre of every cell of an n x n window whose low corner is (-n / 2 cells, 0): one in ten a metre up"""
    rng = np.random.default_rng(seed)
    ia, ib = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32))
    pts = np.zeros((n * n, 4), np.float32)
    pts[:, 0] = ((ia + 0.5) * CELL - 0.5 * n * CELL).ravel()
    pts[:, 2] = ((ib + 0.5) * CELL).ravel()
    h = np.where(rng.random(n * n) < 0.1, 1.0, rng.uniform(-0.05, 0.05, n * n)).astype(np.float32)
    pts[:, 1] = 1.65 - h                                         # the default frame: a level camera 1.65 m above the road
    pts[:, 3] = 0.5
    return pts


def main():
    import svhip
    from svhip import grid, view
    import gpu_view
    out = os.path.join(ROOT, "profiles", "grid_dyn_times.jsonl")
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
        raise SystemExit("gpu_grid_dyn needs a GPU: libsvhip has no CPU fallback")
    hip = C.CDLL("libamdhip64.so")
    L = svhip.lib()
    grid._bind()
    forms = hasattr(L, "svh_test_grid_dyn_form")
    if forms:
        L.svh_test_grid_dyn_form.argtypes = [C.c_int32]
    build = L.svh_version().decode()
    lines = []
    urban = gpu_view.urban_view(view, (64, 48))
    newest = urban.points(urban.count(view.LISTS) - 1)
    v = view.View(64, 48)
    v.add_points([newest])
    for n in sizes:
        rgb = C.c_void_p()
        assert hip.hipMalloc(C.byref(rgb), C.c_size_t(n * n * 3)) == 0
        for scene in ("urban", "all_cells"):
            if scene == "all_cells" and n > ALL_CELLS_MAX:
                continue
            dev, npts = C.c_void_p(), len(newest)
            if scene == "all_cells":
                pts = all_cells(n, n)
                npts = len(pts)
                assert hip.hipMalloc(C.byref(dev), C.c_size_t(pts.nbytes)) == 0
                assert hip.hipMemcpy(dev, C.c_void_p(pts.ctypes.data), C.c_size_t(pts.nbytes), 1) == 0
            prm = grid.default_params(nx=n, nz=n, cell=CELL, x0=-0.5 * n * CELL, z0=0.0)
            plain, dyn = grid.Grid(prm), grid.Grid(prm)
            dyn.set_dynamics()
            state = {"k": 0}

            def step(g, observe, form=None):
                if form is not None:
                    L.svh_test_grid_dyn_form(form)
                state["k"] += 1
                centre = [0.0, 0.0, 0.1 + CELL * (((state["k"] - 1) // state["sides"]) % 2)]    # one cell forward and back, the same for the sides of a repetition
                t0 = time.perf_counter()
                g.follow(centre, n // 2, 0)
                if scene == "urban":
                    (g.observe_view_lists if observe else g.add_view_lists_from)(v, 0, 1, centre)
                elif observe:
                    g.observe_points_device(dev.value, npts, centre)
                else:
                    g.add_points_device_from(dev.value, npts, centre)
                g.render_local(device_ptr=rgb.value)
                return (time.perf_counter() - t0) * 1e3

            sides = {"add": lambda: step(plain, False)}
            if forms:
                sides["observe_body"] = lambda: step(dyn, True, 0)
                sides["observe_slot"] = lambda: step(dyn, True, 1)
            else:
                sides["observe"] = lambda: step(dyn, True)
            state["sides"] = len(sides)
            ms = paired(sides, warmup, timed)
            if forms:
                L.svh_test_grid_dyn_form(0)
            rec = {"leg": "local_step", "scene": scene, "nx": n, "nz": n, "cell": CELL, "points": npts, "dyn_stats": dyn.dyn_stats(),
                   "rays": dyn.ray_stats()[0], "warmup": warmup, "timed": timed, "build": build,
                   "timed_with": "host clock around follow, the frame, render_local; every entry returns after its last wait"}
            for name, t in ms.items():
                rec.update(summary(name, t))
            first = "observe_body" if forms else "observe"
            rec.update(summary("%s_minus_add" % first, [a - b for a, b in zip(ms[first], ms["add"])]))
            if forms:
                rec.update(summary("observe_slot_minus_add", [a - b for a, b in zip(ms["observe_slot"], ms["add"])]))
                rec.update(summary("slot_minus_body", [a - b for a, b in zip(ms["observe_slot"], ms["observe_body"])]))
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            plain.close()
            dyn.close()
            if dev:
                hip.hipFree(dev)
        hip.hipFree(rgb)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
