#!/usr/bin/env python3
"""Time the voxel-grid thinning of the map view (svh_view_thin, include/svh_view.h) on the device.

Cases: stores of 10^5, 10^6 and 10^7 seeded synthetic points with about 1, 4 and 16 points per occupied voxel, and the
fused lists of the golden urban crops (urban2 and urban3 through svh_map_add, as tools/gpu_view.py builds them), all at
a voxel of 0.05.  A thinning changes the store, so every repetition refills the view device to device from a copy of
the raw lists (not timed) and then times ONE whole svh_view_thin call with the host clock: the call returns after its
last stream wait, so the interval holds the two table fills, the five kernels, the copy back of the list boundaries and
the exchange of the stores.  Per case 5 warm-up and 20 timed calls: median, 10th and 90th percentile in ms.

In the same process the 1242 x 375 render of the store before and after the thinning is timed with the method of
tools/gpu_view.py (HIP events around svh_view_render, device output, 5 + 20 renders), so the figures compare with
profiles/view_render_times.jsonl.

Also recorded: the survivor ratio, the unplaceable points, and the scratch bytes per point of that call (table slots
of 12 bytes at the capacity the library chose, 4 + 1 bytes per point, 4 per block of 1024, and the second store's 16).
One JSON line per case goes to profiles/view_thin_times.jsonl.

    python tools/gpu_view_thin.py [--out FILE] [--max-points N]

There is no threshold: this is a measurement.  The split over the kernels is not measured here."""
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
VOXEL = 0.05
RENDER = (1242, 375)


def synthetic(n, dup, seed=1):
    """n points, about `dup` in every occupied voxel of side VOXEL, in a corridor like a drive's map, in random order"""
    rng = np.random.default_rng(seed)
    nv = max(n // dup, 1)
    cell = np.stack([rng.integers(-160, 160, nv), rng.integers(-40, 40, nv), rng.integers(20, 2400, nv)], 1)
    pick = rng.permutation(np.arange(n) % nv)
    pts = np.empty((n, 4), np.float32)
    pts[:, :3] = (cell[pick] + rng.uniform(0.05, 0.95, (n, 3))) * VOXEL
    pts[:, 3] = rng.uniform(0, 1, n)
    return pts


class DeviceLists:
    """the raw lists once on the device; refill(v) makes v hold exactly them"""

    def __init__(self, hip, lists):
        self.hip, self.ptrs, self.counts = hip, [], [len(a) for a in lists]
        for a in lists:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 16))) == 0
            if a.nbytes:
                assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
            self.ptrs.append(p)

    def refill(self, v):
        v.clear()
        for p, n in zip(self.ptrs, self.counts):
            v.add_points_device([p.value], [n])

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


def percentile(sorted_ms, q):
    return float(np.percentile(np.array(sorted_ms), q))


def scratch_bytes_per_point(n):
    cap = 1024
    while cap < 2 * n:
        cap *= 2
    return (12 * cap + 5 * n + 4 * ((n + 1023) // 1024) + 16 * n) / max(n, 1), cap


def run_case(name, lists, dup, view, timer, rgb, build, cameras=()):
    import gpu_view
    dl = DeviceLists(timer.hip, lists)
    v = view.View(*RENDER)
    ms, st = [], None
    for k in range(WARMUP + TIMED):
        dl.refill(v)
        assert timer.hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        st = v.thin(VOXEL)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= WARMUP:
            ms.append(dt)
    ms.sort()
    # the render before and after, with the cameras (svh_view_clear dropped them; a thinning does not look at them)
    dl.refill(v)
    for Ht in cameras:
        v.add_camera(Ht, 0.1, True)
    r0 = gpu_view.measure(timer, v, rgb)
    st2 = v.thin(VOXEL)
    assert (st2.before, st2.after, st2.unplaced) == (st.before, st.after, st.unplaced)
    r1 = gpu_view.measure(timer, v, rgb)
    med = lambda s: 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    per_point, cap = scratch_bytes_per_point(st.before)
    rec = {"case": name, "points": int(st.before), "lists": len(lists), "per_voxel": dup, "voxel": VOXEL,
           "survivors": int(st.after), "unplaced": int(st.unplaced), "survivor_ratio": round(st.after / max(st.before, 1), 4),
           "warmup": WARMUP, "timed": TIMED, "thin_median_ms": round(med(ms), 4), "thin_p10_ms": round(percentile(ms, 10), 4),
           "thin_p90_ms": round(percentile(ms, 90), 4), "thin_mpoints_per_s": round(st.before / (med(ms) * 1e-3) / 1e6, 1),
           "table_slots": cap, "scratch_bytes_per_point": round(per_point, 2),
           "render_width": RENDER[0], "render_height": RENDER[1], "render_before_median_ms": round(med(r0), 4),
           "render_after_median_ms": round(med(r1), 4),
           "timed_with": "host clock around svh_view_thin (returns after its last wait); HIP events around svh_view_render",
           "build": build}
    print(json.dumps(rec), flush=True)
    v.close()
    dl.free()
    return json.dumps(rec)


def urban_lists(view):
    """the fused lists of the two golden urban crops and their camera poses"""
    import gpu_view
    v = gpu_view.urban_view(view, RENDER)
    lists = [v.points(i) for i in range(v.count(view.LISTS))]
    v.close()
    cams = []
    for k in range(2):
        Ht = np.eye(4)
        Ht[2, 3] = 0.3 * k
        cams.append(Ht)
    return lists, cams


def main():
    import svhip
    from svhip import view
    import gpu_view
    out = os.path.join(ROOT, "profiles", "view_thin_times.jsonl")
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
        raise SystemExit("gpu_view_thin needs a GPU: libsvhip has no CPU fallback")
    timer = gpu_view.Timer()
    rgb = timer.malloc(RENDER[0] * RENDER[1] * 3)
    build = svhip.lib().svh_version().decode()
    lines = []
    for n in (10 ** 5, 10 ** 6, 10 ** 7):
        if n > max_points:
            continue
        for dup in (1, 4, 16):
            lines.append(run_case("synthetic_%d_x%d" % (n, dup), [synthetic(n, dup)], dup, view, timer, rgb, build))
    lists, cams = urban_lists(view)
    lines.append(run_case("urban2_urban3_fused", lists, None, view, timer, rgb, build, cams))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
