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

There is no threshold: this is a measurement.  The split over the kernels is not measured here (no trace is taken)."""
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


def main():
    import svhip
    from svhip import grid, view
    import gpu_view
    import gpu_view_thin
    out = os.path.join(ROOT, "profiles", "grid_times.jsonl")
    max_points = 10 ** 7
    args = sys.argv[1:]
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
