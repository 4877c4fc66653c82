#!/usr/bin/env python3
"""Time the ground grid (svh_grid_*, include/svh_grid.h) on the device.

Cases: stores of 10^5, 10^6 and 10^7 seeded synthetic points at the densities tools/gpu_view_thin.py uses (about 1, 4
and 16 points per 5 cm voxel, in random order: no runs of equal cell), and the fused lists of the golden urban crops
(urban2 and urban3 through svh_map_add, as tools/gpu_view.py builds them: frame order, column by column).  Grids of
256 x 256 and 1024 x 1024 cells of 0.2 m.

One repetition is the whole sequence a consumer runs per frame -- svh_grid_clear, svh_grid_add_view (the view's store,
device to device), svh_grid_render into a device buffer -- timed with the host clock: every entry returns after its last
stream wait, so the interval holds the three fills of the clear, k_grid_bin, the copy back of the statistics,
k_grid_finalise and k_grid_render.  The time up to the end of svh_grid_add_view is recorded too.

If the library has the switch svh_test_grid_form, the two forms of k_grid_bin (plain: five atomics per low point;
run-combining: a segmented wave scan, atomics only from the last lane of a run of equal cells) ALTERNATE in one process,
repetition by repetition, and the paired saving plain - runs is reported with its 10th and 90th percentile; without the
switch the one form the library has is timed.  Per case 5 warm-up and 20 timed repetitions (per form): median, 10th and
90th percentile in ms.  One JSON line per case and grid goes to profiles/grid_times.jsonl, and with it, as a point of
comparison only, the time of one svh_view_thin of a store of that size from profiles/view_thin_times.jsonl: one pass over
the same bytes.

    python tools/gpu_grid.py [--out FILE] [--max-points N]
    python tools/gpu_grid.py --local [--out FILE]

There is no threshold: this is a measurement.  The split over the kernels is not measured here (no trace is taken).

--local: the grid as a local map (svh_grid_follow, svh_grid_add_view_lists_from, svh_grid_render_local); the records are
APPENDED to profiles/grid_local_times.jsonl.  Same clock, same 5 + 20 repetitions, the two sides of every comparison
alternating repetition by repetition in one process, the paired difference with its 10th and 90th percentile.
  (a) the rays.  If the library has the switch svh_test_grid_ray_form, the two forms of k_grid_rays (plain: one lane per
      end cell, one atomic per step; runs: 64 end cells of a row or column per wave, equal cells combined by a segmented
      scan) are timed on the fused urban store, list by list from one origin (svh_grid_clear, then one
      svh_grid_add_view_lists_from per list), and on 10^6 random low points in a 256 x 256 window from its middle; without
      the switch the one form the library has is timed.  The same sequence through svh_grid_add_view, which casts
      nothing, is timed beside it: the difference is what the end counts and the rays cost.
  (b) one local step -- svh_grid_follow by one cell, svh_grid_add_view_lists_from of the newest list, svh_grid_render_local
      -- against the rebuild -- svh_grid_clear, svh_grid_add_view of the whole store, svh_grid_render -- at a store of
      1, 50 and 200 frames (the newest urban list, moved 0.3 m forward per frame), 256 x 256 cells of 0.2 m."""
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

WARMUP, TIMED = 5, 20
GRIDS = ((256, 256), (1024, 1024))
CELL = 0.2


def pct(ms, q):
    return round(float(np.percentile(np.array(ms), q)), 4)


def summary(prefix, ms):
    return {prefix + "_median_ms": pct(ms, 50), prefix + "_p10_ms": pct(ms, 10), prefix + "_p90_ms": pct(ms, 90)}


def thin_reference():
    """case -> (thin median, p10, p90) of profiles/view_thin_times.jsonl"""
    path, out = os.path.join(ROOT, "profiles", "view_thin_times.jsonl"), {}
    if os.path.exists(path):
        for line in open(path):
            if line.strip():
                r = json.loads(line)
                out[r["case"]] = (r["thin_median_ms"], r["thin_p10_ms"], r["thin_p90_ms"])
    return out


def run_case(name, v, grid, hip, forms, set_form, build, thin_ref):
    lines = []
    n = v.count(1)
    for nx, nz in GRIDS:
        g = grid.Grid(grid.default_params(nx=nx, nz=nz, cell=CELL, x0=-0.5 * nx * CELL, z0=0.0))
        rgb = C.c_void_p()
        assert hip.hipMalloc(C.byref(rgb), C.c_size_t(nx * nz * 3)) == 0
        whole = {f: [] for f in forms}
        upto_add = {f: [] for f in forms}
        for k in range(WARMUP + TIMED):
            for f in (forms if k % 2 == 0 else forms[::-1]):
                if set_form:
                    set_form(f)
                assert hip.hipDeviceSynchronize() == 0
                t0 = time.perf_counter()
                g.clear()
                g.add_view(v)
                t1 = time.perf_counter()
                g.render(grid.RENDER_CLASS, device_ptr=rgb.value)
                t2 = time.perf_counter()
                if k >= WARMUP:
                    whole[f].append((t2 - t0) * 1e3)
                    upto_add[f].append((t1 - t0) * 1e3)
        st = g.stats()
        count = g.count()
        rec = {"case": name, "points": n, "nx": nx, "nz": nz, "cell": CELL, "binned": int(st.binned), "overhead": int(st.overhead),
               "outside": int(st.outside), "unplaced": int(st.unplaced), "occupied_cells": int((count > 0).sum()),
               "warmup": WARMUP, "timed": TIMED}
        for f in forms:
            tag = {0: "plain", 1: "runs", None: "only"}[f]
            rec.update(summary(tag, whole[f]))
            rec.update(summary(tag + "_clear_add", upto_add[f]))
            rec[tag + "_mpoints_per_s"] = round(n / (pct(whole[f], 50) * 1e-3) / 1e6, 1)
        if len(forms) == 2:
            saving = [a - b for a, b in zip(whole[0], whole[1])]
            rec.update(summary("saving_plain_minus_runs", saving))
        if name in thin_ref:
            rec["view_thin_same_store_median_p10_p90_ms"] = list(thin_ref[name])
        rec["timed_with"] = "host clock around svh_grid_clear + svh_grid_add_view + svh_grid_render (device output); every entry returns after its last wait"
        rec["build"] = build
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        g.close()
        hip.hipFree(rgb)
    return lines


def paired(sides):
    """sides: name -> callable; they alternate, the order reversed every other repetition; name -> [ms]"""
    names = list(sides)
    ms = {n: [] for n in names}
    for k in range(WARMUP + TIMED):
        for n in (names if k % 2 == 0 else names[::-1]):
            t0 = time.perf_counter()
            sides[n]()
            if k >= WARMUP:
                ms[n].append((time.perf_counter() - t0) * 1e3)
    return ms


def local_leg(out):
    import svhip
    from svhip import grid, view
    import gpu_view
    hip = C.CDLL("libamdhip64.so")
    L = svhip.lib()
    set_form = None
    if hasattr(L, "svh_test_grid_ray_form"):
        L.svh_test_grid_ray_form.argtypes = [C.c_int32]
        set_form = L.svh_test_grid_ray_form
    build = L.svh_version().decode()
    lines = []

    def emit(rec):
        rec.update(warmup=WARMUP, timed=TIMED, build=build,
                   timed_with="host clock around the entries named; every entry returns after its last wait")
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    # (a) the rays
    urban = gpu_view.urban_view(view, (64, 48))
    rng = np.random.default_rng(1)
    rnd = view.View(64, 48)
    rnd.add_points([np.stack([rng.uniform(-25.6, 25.6, 10 ** 6), rng.uniform(0.0, 1.6, 10 ** 6), rng.uniform(0.0, 51.2, 10 ** 6),
                              rng.uniform(0, 1, 10 ** 6)], 1).astype(np.float32)])
    for name, v, shapes, origin in (("urban2_urban3_fused_by_list", urban, GRIDS, [0.0, 0.0, 0.1]),
                                    ("random_1e6_low", rnd, ((256, 256),), [0.0, 0.0, 25.6])):
        nl = v.count(view.LISTS)
        for nx, nz in shapes:
            g = grid.Grid(grid.default_params(nx=nx, nz=nz, cell=CELL, x0=-0.5 * nx * CELL, z0=0.0))

            def cast(form=None):
                if form is not None:
                    set_form(form)
                g.clear()
                for k in range(nl):
                    g.add_view_lists_from(v, k, 1, origin)

            def no_rays():
                g.clear()
                g.add_view(v)

            sides = {"plain": lambda: cast(0), "runs": lambda: cast(1)} if set_form else {"only": cast}
            sides["add_view_no_rays"] = no_rays
            ms = paired(sides)
            cast(1 if set_form else None)
            rays, ray_cells = g.ray_stats()
            rec = {"leg": "rays", "case": name, "points": v.count(view.POINTS), "lists": nl, "nx": nx, "nz": nz, "cell": CELL,
                   "rays": rays, "ray_cells": ray_cells, "end_cells": int((g.count() > 0).sum())}
            for n, t in ms.items():
                rec.update(summary(n, t))
            if set_form:
                rec.update(summary("saving_plain_minus_runs", [a - b for a, b in zip(ms["plain"], ms["runs"])]))
            best = "runs" if set_form else "only"
            rec.update(summary("rays_cost_%s_minus_add_view" % best, [a - b for a, b in zip(ms[best], ms["add_view_no_rays"])]))
            emit(rec)
            g.close()
    if set_form:
        set_form(1)
    # (b) one local step against the rebuild
    newest = urban.points(urban.count(view.LISTS) - 1)
    rgb = C.c_void_p()
    assert hip.hipMalloc(C.byref(rgb), C.c_size_t(256 * 256 * 3)) == 0
    for frames in (1, 50, 200):
        v = view.View(64, 48)
        for k in range(frames):
            v.add_points([newest + np.array([0, 0, 0.3 * k, 0], np.float32)])
        kw = dict(nx=256, nz=256, cell=CELL, x0=-25.6, z0=0.0)
        local, rebuilt = grid.Grid(grid.default_params(**kw)), grid.Grid(grid.default_params(**kw))
        z = 0.3 * (frames - 1)
        state = {"k": 0}

        def local_step():
            state["k"] += 1
            centre = [0.0, 0.0, z + 0.1 + CELL * (state["k"] % 2)]     # one cell forward and back: a strip enters every time
            local.follow(centre, 128, 0)
            local.add_view_lists_from(v, frames - 1, 1, centre)
            local.render_local(device_ptr=rgb.value)

        def rebuild():
            rebuilt.clear()
            rebuilt.add_view(v)
            rebuilt.render(grid.RENDER_CLASS, device_ptr=rgb.value)

        ms = paired({"local_step": local_step, "rebuild": rebuild})
        rec = {"leg": "local_vs_rebuild", "frames": frames, "store_points": v.count(view.POINTS), "newest_list_points": len(newest),
               "nx": 256, "nz": 256, "cell": CELL}
        for n, t in ms.items():
            rec.update(summary(n, t))
        rec.update(summary("saving_rebuild_minus_local", [a - b for a, b in zip(ms["rebuild"], ms["local_step"])]))
        emit(rec)
        local.close(), rebuilt.close(), v.close()
    hip.hipFree(rgb)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


def main():
    import svhip
    from svhip import grid, view
    import gpu_view
    import gpu_view_thin
    out = os.path.join(ROOT, "profiles", "grid_times.jsonl")
    max_points = 10 ** 7
    args = sys.argv[1:]
    local = "--local" in args
    if local:
        args.remove("--local")
        out = os.path.join(ROOT, "profiles", "grid_local_times.jsonl")
    while args:
        a = args.pop(0)
        if a == "--out":
            out = args.pop(0)
        elif a == "--max-points":
            max_points = int(args.pop(0))
        else:
            raise SystemExit(__doc__)
    if svhip.device_count() < 1:
        raise SystemExit("gpu_grid needs a GPU: libsvhip has no CPU fallback")
    if local:
        return local_leg(out)
    hip = C.CDLL("libamdhip64.so")
    L = svhip.lib()
    forms, set_form = [None], None
    if hasattr(L, "svh_test_grid_form"):
        L.svh_test_grid_form.argtypes = [C.c_int32]
        forms, set_form = [0, 1], L.svh_test_grid_form
    build = L.svh_version().decode()
    thin_ref = thin_reference()
    lines = []
    for n in (10 ** 5, 10 ** 6, 10 ** 7):
        if n > max_points:
            continue
        for dup in (1, 4, 16):
            v = view.View(64, 48)
            v.add_points([gpu_view_thin.synthetic(n, dup)])
            lines += run_case("synthetic_%d_x%d" % (n, dup), v, grid, hip, forms, set_form, build, thin_ref)
            v.close()
    v = gpu_view.urban_view(view, (64, 48))
    lines += run_case("urban2_urban3_fused", v, grid, hip, forms, set_form, build, thin_ref)
    v.close()
    if set_form:
        set_form(1)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
